"""HipProcessor: the MI355X backend behind raw2film's processor surface.

Mirrors `CpuProcessor.process` (cpu_processor.py:269-414) / `GpuProcessor.process`,
`.extract_image_data_cpu`, `.process_preloaded` (gpu_processor.py:715-783, 1541-1693): same
keyword names and defaults, unknown keywords swallowed, LUTs / stencils rebuilt and
re-uploaded only when their parameter dict changes (cpu_processor.py:104-105,157-158,...).

Scope: the post-decode per-pixel path plus what sits either side of it: aspect crop, zoom,
quarter turns, free rotation, the preview / `max_scale` down-scale and the pre-path chroma NR before; the highlight
burn (S7) inside; uint8, the LANCZOS4 way back from `max_scale`, canvas and histogram after.  Lens correction runs on the
device from numbers the caller supplies (`lens_profile=`, raw2film_amd.lens.LensProfile: the first device pre-path step), and so
does what LibRaw does behind its file parser (`raw_profile=`, raw2film_amd.raw.RawProfile, with a uint16 (H, W) Bayer mosaic as
`src`: black / scale, demosaic, camera matrix on the device, ahead of everything else).  Parsing RAW files
and the lensfun database lookup are out of scope: a call that would need the lookup -- `lens_correction=True` WITH a
camera and a lens, the only case in which the reference corrects anything (effects.py:22-30) -- raises NotImplementedError
instead of silently rendering something else.

`src` is therefore a decoded frame: a float32 (H, W, 3|4) array / CUDA tensor in linear CIE XYZ
(what `raw_to_linear` returns, raw_conversion.py:33-53), LibRaw's uint16 output of the same shape, or -- with a `raw_profile` --
the uint16 (H, W) Bayer mosaic itself; or the path of a `.npy` file holding one of these.
"""

from __future__ import annotations

import inspect
import math
import random
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, NamedTuple

import numpy as np

from . import _lib, filmstock, geometry, payload as phase1, stencils, tiff
from .bands import StreamedFrame, band_source, plan_bands, stage_schedule
from .context import LOG_EPS, LUT3D_SCALE, HipContext
from .jpeg_options import _check_jpeg_image, checked_options
from .exports import JpegExport, TiffExport
from .payload import DEVICE_EXPOSURE, host_stream_gate, stream_rejection
from .results import ResultBuffers

REC709_TO_XYZ = np.array(  # data.py:128-135
    [[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]],
    dtype=np.float32,
)


def check_output_bits(output_bits, dst_texture=None) -> int:
    """`output_bits` of a render: 8 (upstream's (image * 255).astype(uint8), cpu_processor.py:407) or 16 (the same rule with
    2 ** 16 - 1); anything else raises before any work starts, and so does 16 with a widget texture, which is RGBA8."""
    if isinstance(output_bits, (bool, np.bool_)) or not isinstance(output_bits, (int, np.integer)) or int(output_bits) not in (8, 16):
        raise ValueError(f"output_bits must be 8 or 16, got {output_bits!r}")
    if int(output_bits) == 16 and dst_texture is not None:
        raise ValueError("output_bits=16 cannot be combined with dst_texture: the widget texture is RGBA8")
    return int(output_bits)


class OutputDepth(NamedTuple):
    """What the output side knows of a sample width, 8 or 16 bits (check_output_bits validates the number, HipProcessor keeps one of
    these per width): the dtypes of a result, the context's entry points that write and resample it -- each pair behind one call
    shape -- and the pool its host buffers come from.  (The canvas colour's multiplier, 1 or 257, is geometry.add_canvas's, which
    reads it off the frame's dtype.)"""
    bits: int
    torch_dtype: object  # of the device and the pinned buffers (int16 holds the bits of a 16-bit result)
    numpy_dtype: type  # of the array the caller gets
    render: Callable  # (image, params, out_f32, out, want_f32, want_out, layout) -> (out_f32, out): r2f_render / r2f_render16
    front: Callable  # (rows, params, out, **row range): the fused LUTs-only pass of a band, straight to the result
    tail: Callable  # (density, params, out, **row range)
    resize_lanczos4: Callable  # (frame, rows, cols): cv.resize(..., INTER_LANCZOS4) / INTER_AREA as applied to this dtype
    resize_area: Callable
    pool: ResultBuffers  # a pool per width: a lent 8-bit buffer never comes back as a 16-bit result, nor the other way round


def output_depths(torch, ctx) -> dict:
    """{8: OutputDepth, 16: OutputDepth} of one processor's context."""
    def depth(bits, torch_dtype, numpy_dtype, *calls):
        return OutputDepth(bits, torch_dtype, numpy_dtype, *calls,
                           ResultBuffers(lambda shape: torch.empty(shape, dtype=torch_dtype, pin_memory=True), numpy_dtype))

    return {
        8: depth(8, torch.uint8, np.uint8,
                 lambda image, p, out_f32, out, want_f32, want_out, layout: ctx.render(
                     image, p, out_f32=out_f32, out_u8=out, want_f32=want_f32, want_u8=want_out, layout=layout),
                 lambda rows, p, out, **kw: ctx.stage_front(rows, p, 2, out_u8=out, **kw),
                 lambda density, p, out, **kw: ctx.stage_tail(density, p, out_u8=out, **kw),
                 ctx.resize_lanczos4_u8, ctx.resize_area_u8),
        16: depth(16, torch.int16, np.uint16,  # (r2f_render16 always writes its 16-bit result: no want_out)
                  lambda image, p, out_f32, out, want_f32, want_out, layout: ctx.render16(
                      image, p, out_f32=out_f32, out_u16=out, want_f32=want_f32, layout=layout),
                  lambda rows, p, out, **kw: ctx.stage_front16(rows, p, out_u16=out, **kw),
                  lambda density, p, out, **kw: ctx.stage_tail16(density, p, out_u16=out, **kw),
                  ctx.resize_lanczos4_u16, ctx.resize_area_u16),
    }


def _host16(arr):
    """The host array of a result: the uint16 view of a 16-bit frame (carried as int16, the same bits), else the array itself."""
    return arr.view(np.uint16) if arr.dtype == np.int16 else arr


def exposure_on_device(exposure) -> bool:
    """Is `exposure` the device mode?  None (measured on the host) and a number (stops) are not; any other string raises."""
    if isinstance(exposure, (str, bytes, bytearray)):
        if exposure == DEVICE_EXPOSURE:
            return True
        raise ValueError(f"exposure must be None (measured on the host), a number of stops or {DEVICE_EXPOSURE!r}, got {exposure!r}")
    return False


class PendingFrame:
    """A frame submitted with HipProcessor.submit_preloaded: `.result()` waits for its download and returns the uint8 array (the
    uint16 one of a frame submitted with output_bits=16)."""

    def __init__(self, host, done, array=None):
        self._host, self._done, self._array = host, done, array

    @classmethod
    def finished(cls, array):
        """A frame that is back already (a payload that streamed through the pipeline: submit_preloaded)."""
        return cls(None, None, array)

    def ready(self) -> bool:
        return self._array is not None or self._done.query()

    def result(self) -> np.ndarray:
        if self._array is not None:
            return self._array
        self._done.synchronize()
        return _host16(self._host.numpy())


class HipProcessor:
    """Drop-in for the hot path of CpuProcessor / GpuProcessor (gui.py:1584-1585)."""

    # class-level defaults: what the host-only entry points (extract_image_data_cpu, the early refusals) read without a constructed processor
    payload_alpha = True
    profile_stages = False  # settable: process() then times its stages into `last_stage_ms` (see there)
    _texture = _texture_src = image_param_dict = None  # the frame cache, empty
    _raw_repair = None

    def __init__(self, cameras=None, lenses=None, device: int = 0, payload_alpha: bool = True, result_buffers: int = 0,
                 lib_path: str | None = None):
        """payload_alpha: extract_image_data_cpu appends the constant alpha plane like upstream (gpu_processor.py:765: its wgpu
        texture is rgba32float).  Nothing on this backend reads it -- the device path takes 3- and 4-channel frames alike -- and
        batch export is bound by the upload of the payload: with payload_alpha=False the frame crosses PCIe a quarter smaller.
        result_buffers: see _download (pinned result buffers for interactive use).
        lib_path: another build of libr2f_hip.so for this processor's context (development A/B; default: the in-tree library)."""
        import torch

        self._torch = torch
        self.cameras, self.lenses = cameras, lenses
        self.payload_alpha = bool(payload_alpha)
        self.result_buffers = int(result_buffers)  # 0: process() returns a fresh array; n: views of n pinned buffers in turn (_download)
        # process(host array, cache=False) with pinned result buffers streams a large frame through the pipeline in row bands while it
        # is still arriving (_process_streamed): at most this many, of at least 512 rows each (100 MP: 16 bands of 512 rows = 23.3 ms
        # against 24.7 with 8, 27.2 with 4, 24.9 with 24 -- tools/stream_bands_probe.py); 0: upload, render, download one after the other
        self.stream_bands = 16
        self.stream_taper = 2  # ... and the last two of them are halved (what runs behind the last byte of the upload gets shorter)
        self.ctx = HipContext(device, lib_path=lib_path)
        self._depths = output_depths(torch, self.ctx)  # output_bits -> what differs between an 8- and a 16-bit result
        self.device = self.ctx.device  # NB: a torch device, not a wgpu device (gui.py:1652 uses bitmap mode)
        # comparison dicts, same role as cpu_processor.py:41-45 / gpu_processor.py
        self.input_param_dict = self.curve_param_dict = self.output_param_dict = self.highlight_burn_param_dict = None
        self.halation_param_dict = self.mtf_param_dict = self.grain_kernel_param_dict = self.grain_lut_param_dict = None
        self.pipeline_resolution = None  # (w, h) of the frame prepared last
        self.matrix_key = None
        self.uploads = 0  # number of table uploads, for the caching tests
        self.last_output = None  # device uint8 (H, W, 3) of the last process()/process_preloaded(): histogram source
        # stops the device measured for the last exposure="device" frame this processor uploaded (calc_exposure's, in fp64); frames of
        # the other modes leave it alone
        self._last_auto_exposure = None
        self._auto_exposure_pending = False  # the device-side record holds stops that have not been read back yet
        self._defer_exposure_read = False  # submit_preloaded's frame in flight: read them when asked, not when the frame is queued
        # why the uint16 frame the last process / process_preloaded / submit_preloaded / *_jpeg call uploaded was measured on the host
        # although it asked for exposure="device"; None for every other call (one that re-rendered a cached frame included)
        self.exposure_rejected = None
        # why the last export, or the last call that tried the row-band path, rendered its frame in one piece; None: it streamed
        self.stream_rejected = None
        # a deferred profile's resolved scale ({"data_maximum", "maximum_used", "adjusted"}) of the frame the last process /
        # process_preloaded / submit_preloaded / export call rendered -- a cached frame's is kept with the frame, which is not measured
        # again --; None when that frame's profile was numeric (streamed or in one piece), or it was no mosaic
        self.last_raw_scale = None
        # what the wavelet denoise of that frame's mosaic ran with ({"threshold", "maximum", "shift"}: raw_denoise), kept with a cached
        # frame like the scale; None when the call had no raw_denoise
        self.last_raw_denoise = None
        # what the hot-pixel repair of that frame's mosaic ran with and did ({"threshold", "q", "min_neighbours", "repaired"}:
        # raw_repair; the property `last_raw_repair`), kept with a cached frame like the scale; None when the call had no raw_repair
        self._raw_repair = None
        self.last_stage_ms = None  # process()'s wall clock per stage with `profile_stages` on (bench.py's host_device_copies)
        self._load_stage_ms = None  # ... load_image_texture's share of it, until process() folds it in
        # the frame cache (load_image_texture): (frame, layout, payload geometry) kept on the device, a weak reference to its array, its load parameters
        self._texture = self._texture_src = self.image_param_dict = None
        self._halation_reach = self._mtf_reach = (0, 0)  # (rows above, rows below) of the stencils uploaded last: a band's halo
        self._stream_bufs = None  # the device buffers of the streamed frame, kept for the next one of its kind (_stream_buffers)
        self._jpeg_host = None  # the export buffers: the pinned buffer a one-piece JPEG comes down into (_encode_device) ...
        self._jpeg_staging = None  # ... and the streamed JPEG export's host side (jpeg_stream.JpegStaging), made on first use
        self._up_stream = self._down_stream = None  # the copy streams (_copy_streams), made on first use

    def close(self):
        """Let go of every buffer, stream and helper thread the processor holds (a second call finds nothing left to do)."""
        for depth in self._depths.values():
            depth.pool.close()
        if self._jpeg_staging is not None:
            self._jpeg_staging.close()
        self._texture = self._texture_src = self.image_param_dict = self.last_output = None
        self._stream_bufs = self._jpeg_host = self._jpeg_staging = None
        self._up_stream = self._down_stream = None
        self.ctx.close()

    # ------------------------------------------------------------------ cached loaders
    def load_input_lut(self, negative_film, exp_kelvin, tint, exp_comp):
        """cpu_processor.py:142-164"""
        new = {"negative_film": negative_film.name, "exp_kelvin": exp_kelvin, "tint": tint, "exp_comp": exp_comp}
        if new == self.input_param_dict:
            return
        self.ctx.set_lut2d(negative_film.get_input_lut(exp_kelvin, tint, exp_comp))
        self.uploads += 1
        self.input_param_dict = new

    def load_density_curve(self, negative_film, push_pull, color_masking=None):
        """cpu_processor.py:166-188"""
        new = {"negative_film": negative_film.name, "push_pull": push_pull, "color_masking": color_masking}
        if new == self.curve_param_dict:
            return
        self.ctx.set_curve1d(negative_film.get_density_curve(push_pull=push_pull, color_masking=color_masking))
        self.uploads += 1
        self.curve_param_dict = new

    def load_output_lut(self, negative_film, print_film=None, red_light=0.0, green_light=0.0, blue_light=0.0,
                        projector_kelvin=6500, shadow_comp=0.0, sat_adjust=1.0, gamma_func="sRGB",
                        inversion_gamma=4.0, idealized_curve=False, inversion=False, white_balance=False,
                        white_clip=False, icc_transform=None, color_masking=None):
        """cpu_processor.py:190-267"""
        new = {
            "negative_film": negative_film.name,
            "print_film": print_film.name if print_film is not None else None,
            "red_light": red_light, "green_light": green_light, "blue_light": blue_light,
            "projector_kelvin": projector_kelvin, "shadow_comp": shadow_comp, "sat_adjust": sat_adjust,
            "gamma_func": gamma_func, "inversion_gamma": inversion_gamma, "idealized_curve": idealized_curve,
            "inversion": inversion, "white_balance": white_balance, "white_clip": white_clip,
            "icc_transform": icc_transform, "color_masking": color_masking,
        }
        if new == self.output_param_dict:
            return
        lut = filmstock.create_lut(
            negative_film, print_film, mode="print", input_colorspace=None, adx_coding=False, cube=False,
            red_light=red_light, green_light=green_light, blue_light=blue_light, projector_kelvin=projector_kelvin,
            shadow_comp=shadow_comp, sat_adjust=sat_adjust, gamma_func=gamma_func, inversion_gamma=inversion_gamma,
            idealized_curve=idealized_curve, inversion=inversion, white_balance=white_balance, white_clip=white_clip,
            linear_scaling=4.0, color_masking=color_masking,
        )
        if icc_transform is not None:  # cpu_processor.py:255-263: 8-bit ICC pass over the LUT itself
            from PIL import Image, ImageCms

            shape = lut.shape
            img = Image.fromarray((lut * 255).astype(np.uint8).reshape(shape[0], -1, shape[-1]))
            ImageCms.applyTransform(img, icc_transform, inPlace=True)
            lut = (np.array(img, np.uint8).reshape(shape) / 255.0).astype(np.float32)
        self.ctx.set_lut3d(lut)
        self.uploads += 1
        self.output_param_dict = new

    def load_halation_kernel(self, scale, halation_size=1.0, halation_red_factor=1.0, halation_green_factor=0.4,
                             halation_blue_factor=0.0, halation_intensity=1.0, bw=False):
        """gpu_processor.py:818-854"""
        new = {"scale": scale, "halation_size": halation_size, "halation_red_factor": halation_red_factor,
               "halation_green_factor": halation_green_factor, "halation_blue_factor": halation_blue_factor,
               "halation_intensity": halation_intensity, "bw": bw}
        if new == self.halation_param_dict:
            return
        k = stencils.halation_stencil(scale, halation_size, halation_red_factor, halation_green_factor,
                                      halation_blue_factor, halation_intensity, bw=bw)
        self.ctx.set_kernel(_lib.KERNEL_HALATION, k)
        self._halation_reach = stencils.vertical_reach(k)  # (rows above, rows below): what a row band needs of its neighbours
        self.uploads += 1
        self.halation_param_dict = new

    def load_mtf_kernel(self, negative_film, scale, sharpening_strength, sharpening_sigma):
        """gpu_processor.py:792-816"""
        new = {"negative_film": negative_film.name, "scale": scale, "sharpening_strength": sharpening_strength,
               "sharpening_sigma": sharpening_sigma}
        if new == self.mtf_param_dict:
            return
        k = stencils.mtf_stencil(negative_film, scale, sharpening_strength, sharpening_sigma)
        self.ctx.set_kernel(_lib.KERNEL_MTF, k)
        self._mtf_reach = stencils.vertical_reach(k)
        self.uploads += 1
        self.mtf_param_dict = new

    def load_grain(self, negative_film, scale, grain_size_mm=0.01, grain_sigma=0.4, bw_grain=False):
        """gpu_processor.py:904-936 (the seed is an explicit argument of the render here)"""
        new_lut = {"negative_film": negative_film.name, "scale": scale, "bw_grain": bw_grain}
        if new_lut != self.grain_lut_param_dict:
            self.ctx.set_grain_lut(negative_film.get_grain_curve(scale, adx=False, bw_grain=bw_grain))
            self.uploads += 1
            self.grain_lut_param_dict = new_lut
        new = {"scale": scale, "grain_size_mm": grain_size_mm, "grain_sigma": grain_sigma, "bw_grain": bw_grain}
        if new == self.grain_kernel_param_dict:
            return
        k = filmstock.grain_kernel(1 / scale, grain_size_mm=grain_size_mm, grain_sigma=grain_sigma)
        if k is None:
            k = np.ones((1, 1), dtype=np.float32)  # gpu_processor.py:931-932
        self.ctx.set_kernel(_lib.KERNEL_GRAIN, k)
        self.uploads += 1
        self.grain_kernel_param_dict = new

    # ------------------------------------------------------------------ phase 1 (host)
    def load_highlight_burn(self, negative_film, highlight_burn, burn_scale, pipeline_resolution=None):
        """Parameters of the highlight burn for the frame size at hand -- the counterpart of GpuProcessor.load_highlight_burn
        (gpu_processor.py:856-878): reference density, strength, the low-resolution grid.  Nothing is uploaded here: the device
        side takes them by value in r2f_params (the reference keeps them in a uniform buffer).  `pipeline_resolution` = (w, h);
        default: the frame prepared last (the reference reads self.pipeline_resolution).  Returns the dict it keeps in
        `highlight_burn_param_dict`; "cell" is the size in pixels of a low-resolution cell (effects.py:365)."""
        if pipeline_resolution is None:
            pipeline_resolution = self.pipeline_resolution
        if pipeline_resolution is None:
            raise ValueError("load_highlight_burn: no pipeline_resolution (prepare a frame first or pass (w, h))")
        w, h = int(pipeline_resolution[0]), int(pipeline_resolution[1])
        d_ref = negative_film.d_ref[1 if len(negative_film.d_ref) > 1 else 0]  # effects.py:406
        cell = math.ceil(min(w, h) / burn_scale)
        self.highlight_burn_param_dict = {"d_ref": d_ref, "highlight_burn": highlight_burn, "lowres_w": max(1, w // cell),
                                          "lowres_h": max(1, h // cell), "cell": cell}
        return self.highlight_burn_param_dict

    def read_texture(self, texture):
        """A device "texture" (an (h, w, 4) or (h, w, 3) uint8 tensor, e.g. `dst_texture` after process()) as an (h, w, 3) uint8
        array on the host -- GpuProcessor.read_texture (gpu_processor.py:1311-1356)."""
        torch = self._torch
        if not (isinstance(texture, torch.Tensor) and texture.is_cuda and texture.dtype == torch.uint8 and texture.dim() == 3
                and texture.shape[2] in (3, 4)):
            raise NotImplementedError("read_texture: wgpu textures are not supported; pass a uint8 (h, w, 3 or 4) CUDA tensor")
        return self._download(texture[:, :, :3].contiguous())

    def extract_image_data_cpu(self, src, cam=None, lens=None, lens_correction=True, frame_width=36, frame_height=24,
                               rotation=0.0, zoom=1.0, rotate_times=0, flip=False, resolution=None, half_size=True,
                               cache=True, chroma_nr=0, max_scale=400.0, canvas_mode="No", canvas_scale=1.0,
                               canvas_ratio=1.0, exposure=None, metadata=None, lens_profile=None, raw_profile=None, raw_denoise=None,
                               raw_repair=None, **kwargs):
        """PHASE 1 of the two-phase batch API (gpu_processor.py:715-783): pure host work, touches
        no instance state.  Returns the same payload dict; `image_array` is (H, W, 4) float32 ((H, W, 3) with payload_alpha=False).
        exposure="device" (a uint16 frame): no pass over the frame here.  `image_array` is then the WHOLE decoded frame -- the caller's
        array itself when that is contiguous --, `u16_window` the (row0, col0, rows, cols) the aspect and zoom crops keep of it,
        `exposure_root` calc_exposure's exponent and `u16_factor` the marker "device": phase 2 measures the exposure on the uploaded
        frame and decodes the window with it.  A frame that is turned or rotated is measured here as with exposure=None, and the
        payload's `exposure_rejected` says why.
        lens_profile (a raw2film_amd.lens.LensProfile) with lens_correction=True: the lens correction moves to the device.  Upstream
        corrects before any crop, so `image_array` stays the WHOLE frame and the payload gains `lens`: the r2f_lens_params of the
        frame's size, the `window` (row0, col0, rows, cols) of the corrected frame the aspect crop keeps (with the zoom crop when
        there is no rotation) and the quarter turns still to be applied to it; every crop-derived value (`pipeline_resolution`
        ...) is that of the same call without a profile.  A profile with `tca` adds the r2f_lens_tca_params under `tca`, and the
        step is r2f_lens_correct_tca; without one the step has no such key.  A profile with `projection` adds the
        r2f_lens_projection_params under `projection` in the same way, and the step is r2f_lens_correct_projected.
        lens_correction=False ignores the profile.
        raw_profile (a raw2film_amd.raw.RawProfile): `src` is a Bayer mosaic, uint16 (H, W), demosaiced on the device (include/r2f.h,
        r2f_demosaic_u16; `half_size` selects the half-size form) into the uint16 frame every other word of this text is about.
        `image_array` is the mosaic and the payload gains `demosaic`: the r2f_demosaic_params, and the `window` (row0, col0, rows,
        cols) and quarter turns that the host applies to a decoded frame's array here and the device applies to the demosaiced one.
        No RGB frame exists on the host, so exposure=None is measured on the device like exposure="device"; where that is refused (a
        turned or rotated frame) the call needs explicit stops.  With the stops given, no quarter turn and no lens step, the payload
        of a large mosaic streams in row bands (payload.stream_rejection): band k travels as the mosaic rows its demosaic reads
        (payload.mosaic_upload_bounds) and is demosaiced straight into the float frame (r2f_demosaic_f32).
        A raw2film_amd.raw.XTransProfile in its place: `src` is an X-Trans mosaic (6 x 6 array, at least 6 x 6 samples), demosaiced by
        r2f_demosaic_xtrans_u16 -- the project's own interpolation, not LibRaw's; `demosaic` holds the r2f_xtrans_params; half_size
        yields a third of the mosaic's sides; such a payload takes the one-piece path (it does not stream yet).
        A profile with an `orientation` (LibRaw's sizes.flip): the demosaic writes the frame that way round (r2f_demosaic_oriented_u16),
        so every crop-derived number is that of the oriented frame, as upstream's is; the `demosaic` step then carries
        `orientation` (an upright payload has no such key), and the payload takes the one-piece path.
        A deferred profile (its multipliers are a raw2film_amd.raw.RawLevels): `params` are provisional, those of the nominal
        scale, and the `demosaic` step carries the profile under `levels` (a numeric profile's step has no such key).  A numeric
        profile with highlight=("blend", clip) adds `clip` to the step (r2f_demosaic_blend_u16 / _f32 take the place of the plain
        entry points; it streams where a plain numeric profile does); a deferred one's highlight mode is resolved with its scale.  Phase 2
        measures the uploaded mosaic's data maximum (r2f_mosaic_maximum), resolves the profile with it and plans the params the
        demosaic runs with; `last_raw_scale` then holds the numbers.  Such a payload takes the one-piece path.
        A profile with median_passes=n > 0 (LibRaw's med_passes) adds `median` to the step (a step without passes has no such key):
        n passes of the 3 x 3 median of the colour differences between the interpolation and the highlight blend
        (r2f_demosaic_median_u16 / _f32, r2f_demosaic_xtrans_median_u16); a Bayer mosaic streams with it where it streams without.
        raw_denoise (a raw2film_amd.raw.WaveletDenoise; rawpy's noise_thr=): the Bayer mosaic is denoised on the device ahead of its
        demosaic (include/r2f.h, r2f_mosaic_denoise; parity with LibRaw's bytes is unpinned, the pull of the two greens, X-Trans
        mosaics and streaming are not built).  The `demosaic` step carries the record under `denoise` (a step without one has no such
        key).  Phase 2 measures and resolves a deferred profile on the UNdenoised mosaic first, denoises with the record's maximum
        (None: the resolved scale's `maximum_used`), then demosaics with black 0 and the multipliers times 2^-shift;
        `last_raw_denoise` holds {"threshold", "maximum", "shift"}.  ValueError without a raw_profile, with an XTransProfile, with
        maximum=None on a numeric profile, and for a mosaic with an odd side or a side below 64.  The one-piece path.
        raw_repair (a raw2film_amd.raw.HotPixels): hot pixels of the mosaic, Bayer or X-Trans, are repaired on the device ahead of
        everything else that reads it -- the data maximum of a deferred profile, the denoise, the demosaic -- by the project's own
        rule (include/r2f.h, r2f_mosaic_repair; not LibRaw's bad_pixels).  The `demosaic` step carries the record under `repair` (a
        step without one has no such key).  It changes no gate: a mosaic that streams streams with it, each band travelling with 2
        more mosaic rows (payload.mosaic_upload_bounds(repair=2)).  ValueError without a raw_profile and for a mosaic below 6 x 6."""
        on_device = exposure_on_device(exposure)
        phase1.check_profiles(raw_profile, lens_profile, lens_correction, cam, lens)
        # _internal (load_image_texture: the payload never leaves this object): no alpha plane, and the clamp of
        # gpu_processor.py:275 runs on the device after the upload instead of as a 12 B/px pass over host memory
        internal = bool(kwargs.get("_internal"))
        image = phase1.load_decoded(src, clip=not internal, mosaic=raw_profile is not None)
        rows, cols, is_u16 = image.shape[0], image.shape[1], image.dtype == np.uint16
        demosaic_params = lens_params = lens_projection = lens_tca = None
        phase1.check_denoise(raw_denoise, raw_profile, rows, cols)
        phase1.check_repair(raw_repair, raw_profile, rows, cols)
        if raw_profile is not None:  # the crops are those of the demosaiced frame, which is uint16
            demosaic_params = raw_profile.plan(rows, cols, half_size)
            rows, cols = raw_profile.oriented_shape(rows, cols, half_size)  # (the params' out_h, out_w, the way round the sensor was held)
        on_device, exposure, exposure_rejected = phase1.exposure_mode(exposure, on_device, is_u16, raw_profile is not None, rotation,
                                                                      rotate_times)
        if lens_correction and lens_profile is not None:
            lens_params, lens_projection, lens_tca = lens_profile.plan_projected(rows, cols)
        u16_factor = exposure_root = None
        if is_u16:
            from . import decode

            if on_device:
                # the statistic is the whole frame's (upstream measures before any crop), so the whole frame goes up and the crops
                # become a window the device decodes
                u16_factor, exposure_root = DEVICE_EXPOSURE, float(decode.exposure_root(metadata))
            else:
                # raw_to_linear's tail (raw_conversion.py:50-52) moves to the device: the auto exposure is measured here, on the
                # whole decoded frame like upstream (before any crop), unless the caller brings the stops along
                stops = decode.auto_exposure(image, metadata=metadata) if exposure is None else float(exposure)
                u16_factor = float(decode.exposure_factor(stops))
        crops = phase1.plan_crops(rows, cols, is_u16, frame_width / frame_height, flip, zoom, rotation, rotate_times, on_device,
                                  lens_params is not None, demosaic_params is not None)
        if crops.host is not None:
            image = phase1.cut_and_turn(image, **crops.host)
        res = phase1.plan_resolution(*crops.size, frame_width, frame_height, resolution, max_scale, canvas_mode, canvas_scale,
                                     canvas_ratio)
        image = phase1.pack_image(image, demosaic_params is not None or crops.u16_window is not None, is_u16,
                                  self.payload_alpha and not internal)
        return {
            "image_array": image,
            # float32 exposure factor of a uint16 payload (converted on the device), else None; "device": measured there too, on the
            # whole frame `image_array` then is, of which the pipeline takes `u16_window` (calc_exposure's exponent: `exposure_root`)
            "u16_factor": u16_factor,
            "u16_window": crops.u16_window,
            "exposure_root": exposure_root,
            "exposure_rejected": exposure_rejected,  # why exposure="device" was measured on the host after all, or None
            "clip_on_device": internal and u16_factor is None,  # the float frame still has to be clamped to [0, 65504]
            "final_resolution": res.final_resolution,
            "output_resolution": res.output_resolution,
            "canvas_resolution": res.canvas_resolution,
            "pipeline_resolution": res.pipeline_resolution,
            # upstream filters on the host here (gpu_processor.py:750-751); this backend filters on the device in phase 2
            "chroma_nr": int(chroma_nr),
            "resize_to": res.resize_to,  # (rows, cols) of the INTER_AREA down-scale still to be applied, or None
            "warp": crops.warp,  # free rotation still to be applied (first of the device pre-path steps), or None
            "upscale_to": res.upscale_to,  # (rows, cols) the rendered uint8 frame is LANCZOS4-scaled back into, or None
            # the lens step (first of the device pre-path steps)
            # (with `tca`, the r2f_lens_tca_params, only for a profile that has TCA; with `projection`, the
            # r2f_lens_projection_params, only for one that has a projection)
            **({"lens": {"params": lens_params, **crops.lens, **({"tca": lens_tca} if lens_tca is not None else {}),
                         **({"projection": lens_projection} if lens_projection is not None else {})}}
               if lens_params is not None else {}),
            # `image_array` is a Bayer mosaic (ahead of all)
            **({"demosaic": {"params": demosaic_params, **crops.demosaic,
                             **({"orientation": raw_profile.orientation} if raw_profile.orientation else {}),
                             **({"levels": raw_profile} if raw_profile.deferred else {}),
                             **({"denoise": raw_denoise, "profile": raw_profile} if raw_denoise is not None else {}),
                             **({"repair": raw_repair, "profile": raw_profile} if raw_repair is not None else {}),
                             **({"clip": raw_profile.blend_clip} if raw_profile.blend_clip is not None else {}),
                             **({"median": raw_profile.median_passes} if raw_profile.median_passes else {})}}
               if demosaic_params is not None else {}),
        }

    # ------------------------------------------------------------------ the operator surface
    def process(self, src, negative_film, grain_size, grain_sigma, dst_texture=None, histogram_texture=None,
                lens_correction=True, print_film=None, exp_comp=0.0, red_light=0.0, green_light=0.0, blue_light=0.0,
                projector_kelvin=6500, shadow_comp=0.0, sat_adjust=1.0, gamma_func="sRGB", exp_kelvin=6500, tint=0.0,
                inversion_gamma=4.0, idealized_curve=False, inversion=False, push_pull=0.0, white_balance=False,
                white_clip=False, icc_transform=None, resolution=None, frame_width=36, frame_height=24, rotation=0.0,
                zoom=1.0, rotate_times=0, flip=False, cam=None, lens=None, canvas_mode="No", canvas_scale=1.0,
                canvas_ratio=1.0, halation_intensity=1.0, halation=True, halation_size=1.0, halation_green_factor=0.4,
                sharpness=True, sharpening_strength=0.0, sharpening_sigma=1.0, chroma_nr=0, grain=2,
                highlight_burn=0.0, burn_scale=50.0, half_size=True, cache=True, color_masking=None, max_scale=400.0,
                seed=None, exposure=None, metadata=None, src_version=None, output_bits=8, lens_profile=None, raw_profile=None,
                raw_denoise=None, raw_repair=None, **_):
        """Load (decoded) frame and render it: np.uint8 (H, W, 3), like cpu_processor.py:414 -- including the CPU processor's
        last step, resolution_scaling of the finished (canvas-framed) frame to the requested resolution (cpu_processor.py:411-412).
        With `dst_texture` (a uint8 (h, w, 4) CUDA tensor standing in for the preview widget's wgpu texture) the call behaves
        like GpuProcessor.process with a destination (gpu_processor.py:1865-1890): the frame is letterboxed into it on the
        device, `histogram_texture` (same kind of tensor) receives the histogram image, and None is returned.
        A uint16 `src` is LibRaw's 16-bit output before raw_to_linear's last two lines (raw_conversion.py:50-52): those run on
        the device with the auto exposure measured on the host (`metadata`: the EXIF dict calc_exposure reads), given in stops
        (`exposure`), or -- exposure="device" -- measured on the device on the uploaded frame: upstream's formula in fp64, a few
        1e-5 stops at most from upstream's own float32 evaluation and not bit-equal to it; `last_auto_exposure` then holds the stops.
        An array `src` that is the array of the previous call is taken for the same frame when a fingerprint of it agrees (shape,
        dtype, address and a checksum of up to 32 evenly spaced rows -- an edit confined to other rows is NOT seen: pass
        cache=False after a partial in-place edit, or `src_version`, any hashable token of the caller's that changes whenever
        the buffer's content does and then replaces the checksum).
        output_bits=16: np.uint16 (H, W, 3) instead -- clip(x * 65535, 0, 65535) truncated, cpu_processor.py:407's rule with
        2 ** 16 - 1 -- with the whole post-path at 16 bits: the canvas colour c * 257, the LANCZOS4 way back from `max_scale` and
        the final INTER_AREA as cv.resize applies them to uint16, the result lent from a pinned pool of its own and a large
        cache=False frame streamed in row bands exactly where an 8-bit one is.  Not with dst_texture (RGBA8).
        lens_profile (raw2film_amd.lens.LensProfile) with lens_correction=True: the whole frame is uploaded and corrected on the
        device before any crop (extract_image_data_cpu); such a frame never streams in row bands.
        raw_profile (raw2film_amd.raw.RawProfile): `src` is a Bayer mosaic, uint16 (H, W) -- 2 bytes per pixel across PCIe --,
        demosaiced on the device (`half_size` selects the form) into the uint16 frame the rest of the call reads.  exposure=None is
        then measured on the device (extract_image_data_cpu).  A large cache=False mosaic streams in row bands like a decoded frame
        when its exposure is given in stops, rotate_times is a multiple of 4 and no lens step follows: each band is demosaiced
        into the float frame as its mosaic rows arrive (r2f_demosaic_f32), with the bytes of the one-piece call.  Without stops
        (the device's statistic is the whole demosaiced frame's), turned, or with a lens_profile it is demosaiced whole, and
        `stream_rejected` of an export names the demosaic step and the reason.  With a raw2film_amd.raw.XTransProfile `src` is an
        X-Trans mosaic (r2f_demosaic_xtrans_u16: the project's own interpolation; half_size yields a third); it is always demosaiced
        whole ("X-Trans mosaics do not stream yet").  A profile's `orientation` turns the demosaiced frame the way the sensor was
        held before anything else sees it (crops, exposure statistic, lens step, rotate_times); such a mosaic is demosaiced whole.
        A profile whose multipliers are a raw2film_amd.raw.RawLevels is deferred: the uploaded mosaic's data maximum is measured on
        the device (r2f_mosaic_maximum) and the profile resolved with it ahead of the demosaic -- LibRaw's adjust_maximum rule,
        parity unpinned; `last_raw_scale` holds the numbers, a cached frame keeps them.  Such a mosaic is demosaiced whole too.
        raw_denoise (raw2film_amd.raw.WaveletDenoise; rawpy's noise_thr=): the Bayer mosaic is denoised on the device ahead of the
        demosaic (extract_image_data_cpu; r2f_mosaic_denoise), in one piece; `last_raw_denoise` holds the threshold, the maximum
        and the shift it ran with, and a cached frame keeps them.
        raw_repair (raw2film_amd.raw.HotPixels): hot pixels of the mosaic are repaired on the device first of all, ahead of the data
        maximum, the denoise and the demosaic, which then run unchanged on the repaired mosaic (extract_image_data_cpu;
        r2f_mosaic_repair: the project's own rule, not LibRaw's bad_pixels).  It needs a raw_profile, of either kind, and changes no
        gate: a mosaic that streams streams with it.  `last_raw_repair` holds the threshold, q, min_neighbours and the number of
        samples repaired (read back from the device when the attribute is read); a cached frame keeps them."""
        settings = dict(locals())  # every keyword of the signature (the unknown ones in `_` aside), named nowhere else
        exposure_on_device(exposure)  # (any string but "device" raises before any work starts)
        settings["output_bits"] = check_output_bits(output_bits, dst_texture)
        self.exposure_rejected = self.last_raw_scale = self.last_raw_denoise = self.last_raw_repair = None
        for k in _PROCESS_POSITIONAL:
            del settings[k]
        # load_image_texture's share; prepare() and the render take what they need of all of them and swallow the rest
        load = {k: settings[k] for k in _LOAD_KEYWORDS}
        if dst_texture is not None:
            self._check_texture(dst_texture, "dst_texture")
        if histogram_texture is not None:
            self._check_texture(histogram_texture, "histogram_texture")
        # profile_stages (bench.py's host_device_copies): wall clock per stage of this call, with a device synchronisation behind
        # each -- a measuring mode (the syncs serialise what otherwise overlaps), off by default
        prof = self.profile_stages
        if prof:
            import time

            self._torch.cuda.synchronize(self.device)
            t_start = time.perf_counter()
        if not prof and not cache and dst_texture is None and self._host_stream_gate(src, settings) is None:
            # a large host frame that is uploaded for this one render: streamed through the pipeline in row bands while it arrives
            payload = self.extract_image_data_cpu(src, **load, _internal=True)
            res = self._process_streamed(payload, negative_film, grain_size, grain_sigma, settings)
            if res is not None:
                return res
            # its payload did not qualify: uploaded whole like any cache=False array (nothing is recorded for the frame cache)
            self.prepare_gpu_textures(payload)
        else:
            # GpuProcessor.load_image_texture (gpu_processor.py:655-719): the pre-processed frame stays on the device while the
            # load parameters do not change -- a re-render with other film settings neither prepares nor uploads it again
            self.load_image_texture(src, **load)
        image, layout, payload = self._texture
        self.last_raw_scale = payload.get("raw_scale")  # (the frame's own: a cached frame was not measured again)
        self.last_raw_denoise = payload.get("raw_denoise")
        self.last_raw_repair = payload.get("raw_repair")
        if prof:
            self._torch.cuda.synchronize(self.device)
            t_loaded = time.perf_counter()
        out = self._render_prepared(image, layout, payload, negative_film, grain_size, grain_sigma, dst_texture, histogram_texture,
                                    "cpu", **settings)
        if prof:
            self._torch.cuda.synchronize(self.device)
            t_rendered = time.perf_counter()
        res = None if out is None else self._download(out)  # DEVICE -> HOST, the reference's read_texture/map_sync
        if prof:
            t_end = time.perf_counter()
            self.last_stage_ms = {"load_and_upload": (t_loaded - t_start) * 1e3, "prepare_and_render": (t_rendered - t_loaded) * 1e3,
                                  "download": (t_end - t_rendered) * 1e3, "total": (t_end - t_start) * 1e3,
                                  **(self._load_stage_ms or {})}
            self._load_stage_ms = None
        return res

    def load_image_texture(self, src, cam=None, lens=None, lens_correction=True, frame_width=36, frame_height=24, rotation=0.0,
                           zoom=1.0, rotate_times=0, flip=False, resolution=None, half_size=True, cache=True, chroma_nr=0,
                           max_scale=400.0, canvas_mode="No", canvas_scale=1.0, canvas_ratio=1.0, exposure=None, metadata=None,
                           src_version=None, lens_profile=None, raw_profile=None, raw_denoise=None, raw_repair=None):
        """GpuProcessor.load_image_texture (gpu_processor.py:655-719): prepare and upload the frame unless the load parameters
        are those of the frame that is already on the device.  A path compares by value like upstream's `src`.  An array
        compares by identity AND by a fingerprint of its content (shape, dtype, address, a checksum of up to 32 evenly spaced
        rows), so a decode buffer that was refilled is uploaded again -- a SAMPLE: an in-place edit that touches none of the sampled
        rows is not seen.  `src_version` (any hashable token that the caller changes with the content) replaces the
        checksum and saves its ~5 MB pass per call; `cache=False` always uploads.  The processor holds the array by weak reference
        only (upstream's cache never sees arrays: this is this backend's own rule, kept conservative)."""
        load = {k: v for k, v in locals().items() if k in _LOAD_KEYWORDS}  # every keyword of the signature, named nowhere else
        if isinstance(src, str):
            src_key = src
        elif src_version is not None:
            src_key = (getattr(src, "shape", None), str(getattr(src, "dtype", "")), "version", src_version)
        elif not cache:
            # cache=False uploads whatever the fingerprint says: its pass over 32 rows (4.7 MB of a 100 MP frame, ~4 ms of crc32 --
            # the unexplained part of process(host array)'s 35 ms in round 5) is skipped, and nothing is recorded that a later
            # cache=True call could take for "the same frame"
            src_key = None
        else:
            src_key = self._array_fingerprint(src)
        # (`cache` and `src_version` decide how the frame is compared, above; they are not part of what it is compared by)
        new_param_dict = {"src": src_key, **{k: v for k, v in load.items() if k not in ("cache", "src_version")}}
        held = self._texture_src
        same_src = isinstance(src, str) or (held is not None and held() is src)
        if cache and same_src and self._texture is not None and new_param_dict == self.image_param_dict:
            return
        prof = self.profile_stages
        if prof:
            import time

            t0 = time.perf_counter()
        cpu_payload = self.extract_image_data_cpu(src, **load, _internal=True)
        if prof:
            t1 = time.perf_counter()
        self.prepare_gpu_textures(cpu_payload)
        if prof:
            self._torch.cuda.synchronize(self.device)
            self._load_stage_ms = {"host_phase": (t1 - t0) * 1e3, "upload_and_device_prepath": (time.perf_counter() - t1) * 1e3}
        self.image_param_dict = new_param_dict if (src_key is not None or isinstance(src, str)) else None
        self._texture_src = None
        if not isinstance(src, str) and src_key is not None:
            import weakref

            try:
                self._texture_src = weakref.ref(src)
            except TypeError:  # an object that cannot be weakly referenced is simply never taken for "the same frame"
                self._texture_src = None

    @staticmethod
    def _array_fingerprint(src):
        """(shape, dtype, address, strides, crc32 of a SAMPLE) of a decoded frame handed in as an array: of up to 32 evenly spaced
        rows the first, the middle and the last 512 samples each (<= 192 KB of a frame of any size).  A refilled decode buffer, an
        exposure change, any operation on the whole frame shows in it; an edit confined to other samples does not (cache=False or
        src_version for those).  Until round 6 the whole of the 32 rows went into the checksum: 2.4 ms per call on a 100 MP frame
        -- 87 % of a preview re-render (2.76 ms; tools/preview_latency_probe.py), paid on every slider step."""
        if not isinstance(src, np.ndarray):
            return None
        import zlib

        rows = src.shape[0] if src.ndim else 0
        step = max(1, rows // 32)
        crc = 0
        for r in range(0, rows, step):
            row = src[r].reshape(-1)  # (a view for the usual C-contiguous frame)
            n, k = row.size, min(row.size, 512)
            for a in sorted({0, (n - k) // 2, n - k}):
                crc = zlib.crc32(row[a:a + k].tobytes(), crc)
        return (src.shape, src.dtype.str, src.__array_interface__["data"][0], src.strides, crc)

    def prepare_gpu_textures(self, cpu_payload):
        """PHASE 2's stateful half (gpu_processor.py:785-790): upload the payload's frame and run the device pre-path on it
        (uint16 conversion, free rotation, chroma NR, preview scaling); the result is the frame the pipeline reads."""
        self.last_raw_scale = self.last_raw_denoise = self.last_raw_repair = None
        image, layout = self._upload_payload(cpu_payload)
        # (what is kept next to the device frame is the payload's geometry, not its host frame: the processor must not keep a
        # 1.2 GB decode buffer alive; and the scale a deferred profile resolved to, which belongs to this frame: `raw_scale`)
        self._texture = (image, layout, {**{k: v for k, v in cpu_payload.items() if k != "image_array"}, "raw_scale": self.last_raw_scale,
                                         "raw_denoise": self.last_raw_denoise, "raw_repair": self._raw_repair})
        self.image_param_dict = None  # (a payload from outside: no load parameters to compare the next process() with)
        self._texture_src = None

    def _upload_payload(self, cpu_payload):
        """Upload the payload's frame and run the device pre-path on it -> (frame, layout); keeps nothing (prepare_gpu_textures
        keeps the result as the processor's device frame, the JPEG exports do not)."""
        host = self._payload_tensor(cpu_payload)
        if cpu_payload.get("clip_on_device") and not host.is_cuda and host.dim() == 3 and host.numel() >= (1 << 24):
            # A large float frame of this object's own making (process(host array)): the clamp of gpu_processor.py:275 rides on the
            # upload -- the frame goes up in row chunks on a copy stream and every chunk is clamped on the launch stream while the
            # next one travels, so that of its 2.4 GB pass (0.5 ms at 100 MP) only the last chunk's share is left behind the copy
            torch = self._torch
            up, _ = self._copy_streams()
            compute = torch.cuda.current_stream(self.device)
            image = torch.empty(host.shape, dtype=host.dtype, device=self.device)
            up.wait_stream(compute)  # (the block may have been another frame's a moment ago)
            rows = int(host.shape[0])
            step = -(-rows // 8)
            for a0 in range(0, rows, step):
                a1 = min(a0 + step, rows)
                with torch.cuda.stream(up):
                    image[a0:a1].copy_(host[a0:a1], non_blocking=True)
                    arrived = up.record_event()
                compute.wait_event(arrived)
                image[a0:a1].clamp_(0.0, 65504.0)
            image.record_stream(up)
            cpu_payload = dict(cpu_payload, clip_on_device=False)
        else:
            image = host.to(self.device, non_blocking=True)  # HOST -> DEVICE, the reference's write_texture
        return self._prepare_device_frame(image, cpu_payload)

    def _check_texture(self, t, what):
        import torch

        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 4
                and t.is_contiguous()):
            raise NotImplementedError(f"{what}: wgpu textures are not supported; pass a contiguous uint8 (h, w, 4) CUDA tensor "
                                      "(or use the bitmap branch, gui.py:2219-2228)")

    def process_preloaded(self, cpu_payload, negative_film, grain_size, grain_sigma, dst_texture=None,
                          histogram_texture=None, final_scaling="gpu", **settings):
        """PHASE 2 (gpu_processor.py:1643-1693): upload the payload and run the device pipeline.

        final_scaling: "gpu" -- like GpuProcessor, the canvas keeps its size and only a `max_scale` render is scaled back up;
        "cpu" -- like CpuProcessor.process (cpu_processor.py:411-412), the finished frame, canvas included, is scaled to the
        requested resolution (INTER_AREA down, LANCZOS4 up).  dst_texture / histogram_texture, output_bits: see process()."""
        check_output_bits(settings.get("output_bits", 8), dst_texture)
        self.exposure_rejected = self.last_raw_scale = self.last_raw_denoise = self.last_raw_repair = None
        if dst_texture is None and histogram_texture is None and self.stream_bands > 1:
            res = self._stream_payload(cpu_payload, negative_film, grain_size, grain_sigma, final_scaling, **settings)
            if res is not None:  # a large frame without a device pre-path: through the pipeline in row bands while it arrives
                return res
        self.prepare_gpu_textures(cpu_payload)
        image, layout, _ = self._texture
        out = self._render_prepared(image, layout, cpu_payload, negative_film, grain_size, grain_sigma, dst_texture,
                                    histogram_texture, final_scaling, **settings)
        return None if out is None else self._download(out)  # DEVICE -> HOST, the reference's read_texture/map_sync

    # ------------------------------------------------------------------ JPEG export (gui.py:2338-2341)
    def encode_jpeg(self, image, quality=100, *, subsampling=-1, optimize=False, exif=b"", progressive=False, icc_profile=b"",
                    xmp=b"", comment=b"", dpi=(0, 0), restart_marker_blocks=0, restart_marker_rows=0) -> bytes:
        """`Image.fromarray(image).save(f, "JPEG", quality=quality, subsampling=subsampling, optimize=optimize, exif=exif, ...)`
        on the device: the same bytes Pillow writes (JFIF, standard or optimized Huffman tables).  image: uint8 (H, W, 3), a NumPy
        array or a torch tensor (a CUDA tensor may be a row-strided view); quality: an int 0 .. 100 like the reference's slider
        (gui.py:2532-2588).  subsampling: -1 (libjpeg's default, 4:2:0), 0 / "4:4:4", 1 / "4:2:2", 2 / "4:2:0".  optimize: truthy
        for per-image Huffman tables (the call then waits once for the frame's symbol counts).  exif: bytes or a PIL.Image.Exif,
        written as an APP1 segment after the JFIF one (empty: none).  progressive: True for Pillow's progressive=True (SOF2, libjpeg's
        ten scans, each with its own optimized tables, so optimize makes no difference); False, 0 or 1 -- anything else raises.
        icc_profile, xmp (bytes), comment (bytes, or str written as UTF-8): the APP2 chunks, the APP1 XMP segment and the COM
        segment Pillow writes for them, in its order behind the EXIF.  dpi: (x, y), rounded like Pillow's into APP0's density in
        dots per inch when both are positive.  restart_marker_blocks: MCUs per restart interval, 0 .. 65535;
        restart_marker_rows: MCU rows per interval (it wins over blocks; the interval is clamped to 65535 MCUs).  A restart
        interval with progressive=True raises ValueError: baseline only."""
        o = checked_options(quality, subsampling, optimize, exif, progressive, icc_profile, xmp, comment, dpi, restart_marker_blocks,
                            restart_marker_rows)
        torch = self._torch
        if isinstance(image, np.ndarray):
            _check_jpeg_image(image.dtype == np.uint8, image.shape, image.dtype)
            image = torch.from_numpy(np.ascontiguousarray(image)).to(self.device)
        elif isinstance(image, torch.Tensor):
            _check_jpeg_image(image.dtype == torch.uint8, tuple(image.shape), image.dtype)
            if not image.is_cuda:
                image = image.to(self.device)
        else:
            raise ValueError(f"encode_jpeg: expected a uint8 (H, W, 3) NumPy array or torch tensor, got {type(image).__name__}")
        return self._encode_device(image, o)

    def process_jpeg(self, src, negative_film, grain_size, grain_sigma, quality=100, stream=False, file=None, *, subsampling=-1,
                     optimize=False, exif=b"", progressive=False, icc_profile=b"", xmp=b"", comment=b"", dpi=(0, 0),
                     restart_marker_blocks=0, restart_marker_rows=0, **settings):
        """The export of one frame (gui.py:2338-2341): process()'s render with the same keywords -- the pixels process() returns
        for them -- encoded on the device as encode_jpeg does; only the file comes back to the host.  The frame a preview keeps on
        the device (cache=True) is left alone: the next preview re-render uploads nothing.  The export always extracts and uploads
        its frame afresh -- also with cache=True when the preview holds the same frame.
        stream=False: the frame is rendered in one piece, then encoded -- its pixels are those of process()'s one-piece render.
        stream=True: the file is Pillow's of process(src, cache=False, ...)'s pixels.  A large host frame that process(cache=False)
        streams (see _process_streamed) goes through the same row bands and stage calls, and each band's finished MCU rows are
        encoded behind its tail: the file's final bytes go down (and into `file`) while later bands are still arriving.  A frame
        that does not stream takes the one-piece path, and `stream_rejected` says why.
        file: a path or a binary file object the bytes are written into (as they arrive, when streaming); the call then returns
        their count.  Without it the call returns the bytes.
        subsampling, optimize, exif: Pillow's, as in encode_jpeg.  optimize=True needs the whole frame's symbol counts before the
        first scan byte: with stream=True it takes the one-piece path, and `stream_rejected` says so.  progressive (as in
        encode_jpeg) needs the whole frame for every scan: the same.  icc_profile, xmp, comment, dpi, restart_marker_blocks,
        restart_marker_rows: as in encode_jpeg; they stream (the segments are written ahead of the first scan byte, and a
        restart interval may straddle bands)."""
        o = checked_options(quality, subsampling, optimize, exif, progressive, icc_profile, xmp, comment, dpi, restart_marker_blocks,
                            restart_marker_rows)
        exposure_on_device(settings.get("exposure"))
        return self._export(JpegExport(o), src, None, negative_film, grain_size, grain_sigma, "cpu", stream, file, settings)

    def process_preloaded_jpeg(self, cpu_payload, negative_film, grain_size, grain_sigma, quality=100, final_scaling="gpu",
                               stream=False, file=None, *, subsampling=-1, optimize=False, exif=b"", progressive=False,
                               icc_profile=b"", xmp=b"", comment=b"", dpi=(0, 0), restart_marker_blocks=0, restart_marker_rows=0,
                               **settings):
        """The batch export on the two-phase API: process_preloaded's render of a phase-1 payload, encoded on the device like
        process_jpeg.  The processor's device frame (prepare_gpu_textures') is left alone.  stream=True: the file is Pillow's of
        process_preloaded(cpu_payload, final_scaling=..., ...)'s pixels, and a payload process_preloaded streams in row bands is
        encoded band by band as in process_jpeg (else `stream_rejected` says why not).  file, subsampling, optimize, exif,
        progressive, icc_profile, xmp, comment, dpi, restart_marker_blocks, restart_marker_rows: see process_jpeg."""
        o = checked_options(quality, subsampling, optimize, exif, progressive, icc_profile, xmp, comment, dpi, restart_marker_blocks,
                            restart_marker_rows)
        return self._export(JpegExport(o), None, cpu_payload, negative_film, grain_size, grain_sigma, final_scaling, stream, file,
                            settings)

    def _export(self, fmt, src, payload, negative_film, grain_size, grain_sigma, final_scaling, stream, file, settings):
        """Every export behind its option checks; `fmt` (exports.py) is the file format.  Of `src` (payload None: process_jpeg,
        process_tiff): no textures, then process()'s keywords with process()'s defaults (the unknown ones swallowed like there) and
        the frame's payload, extracted afresh; with stream=True process(cache=False)'s gates in its order into `stream_rejected`
        -- the format's own `early` reasons, the host gate, then the payload's (_stream_plan's).  Of a phase-1 `payload`: no
        textures, and with stream=True the format's reasons, the processor's `stream_bands`, the payload's.  Then the row-band
        path into fmt.sink where nothing refused it, else the one-piece render into fmt.whole."""
        what = f"process_{fmt.name}" if payload is None else f"process_preloaded_{fmt.name}"
        self.exposure_rejected = self.stream_rejected = self.last_raw_scale = self.last_raw_denoise = self.last_raw_repair = None
        self._refuse_textures(what, settings, " (use process() for the preview)" if payload is None else "")
        early = next((why for why in fmt.early if why), None) if stream else None
        if payload is None:
            bound = inspect.signature(HipProcessor.process).bind(self, src, negative_film, grain_size, grain_sigma, **settings)
            bound.apply_defaults()
            settings = {k: v for k, v in bound.arguments.items() if k not in _PROCESS_POSITIONAL}
            if stream:
                self.stream_rejected = early or ("profile_stages is on" if self.profile_stages else self._host_stream_gate(src, settings))
            payload = self.extract_image_data_cpu(src, **{k: settings[k] for k in _LOAD_KEYWORDS}, _internal=True)
        elif stream:
            self.stream_rejected = early or (None if self.stream_bands > 1 else f"stream_bands = {self.stream_bands}")
        if stream and self.stream_rejected is None:
            res = self._stream(payload, negative_film, grain_size, grain_sigma, final_scaling, dict(settings, output_bits=fmt.bits),
                               lambda depth, out, bounds: fmt.sink(self, depth, out, bounds, file))
            if res is not None:
                return res
        return fmt.whole(self, self._render_export(payload, negative_film, grain_size, grain_sigma, final_scaling, settings), file)

    def _host_stream_gate(self, src, settings):
        """payload.host_stream_gate of a call's `settings` (process()'s keywords): why its frame is rendered in one piece, or None."""
        profile = settings["raw_profile"]
        mosaic = profile is not None
        exposure = settings["exposure"]
        return host_stream_gate(src, self.stream_bands, settings["rotation"], settings["chroma_nr"], settings["canvas_mode"],
                                settings["highlight_burn"], bool(settings["lens_correction"]) and settings["lens_profile"] is not None,
                                mosaic, stops=exposure is not None and not isinstance(exposure, str),
                                rotate_times=settings["rotate_times"],
                                frame_samples=phase1.mosaic_frame_samples(src, settings["half_size"],
                                                                          settings["frame_width"] / settings["frame_height"],
                                                                          settings["flip"], settings["zoom"],
                                                                          getattr(profile, "reduction", 2),
                                                                          getattr(profile, "orientation", 0)) if mosaic else None,
                                xtrans=isinstance(profile, phase1.XTransProfile), orientation=getattr(profile, "orientation", 0),
                                levels=bool(getattr(profile, "deferred", False)), denoise=settings.get("raw_denoise") is not None)

    @staticmethod
    def _refuse_textures(what, settings, hint=""):
        for k in ("dst_texture", "histogram_texture"):
            if settings.pop(k, None) is not None:
                raise ValueError(f"{what} writes a file: {k} is not taken{hint}")

    def _render_export(self, payload, negative_film, grain_size, grain_sigma, final_scaling, settings):
        """The one-piece render of an export: its frame is uploaded for this render alone (the processor's device frame, a
        preview's, is left alone) -> the device result."""
        image, layout = self._upload_payload(payload)
        return self._render_prepared(image, layout, payload, negative_film, grain_size, grain_sigma, None, None, final_scaling,
                                     **settings)

    # ------------------------------------------------------------------ TIFF export (8 or 16 bits per sample)
    def process_tiff(self, src, negative_film, grain_size, grain_sigma, file=None, *, output_bits=16, icc_profile=b"", stream=False,
                     **params):
        """The export of one frame at full depth: process()'s render with the same keywords -- the pixels
        process(..., output_bits=output_bits) returns for them -- as a baseline TIFF 6.0 file (tiff.py: little-endian, uncompressed,
        chunky RGB, 8 or 16 bits per sample, `icc_profile` bytes in tag 34675).  Returns the file's bytes, or with `file` (a path or
        a binary file object) their count.  Like process_jpeg it takes no textures, extracts and uploads its frame afresh and
        leaves the frame a preview keeps on the device alone.
        stream=True: the file is the one-piece file of process(src, cache=False, output_bits=..., ...)'s pixels.  A large host frame
        that process(cache=False) streams goes through the same row bands: the header (every offset is known in advance) is written
        first, then each band's finished rows go down and into the file while later bands arrive.  A frame that does not stream
        is exported in one piece, and `stream_rejected` says why.  A file past a classic TIFF's 4 GiB raises ValueError."""
        bits = check_output_bits(output_bits)
        icc = tiff.check_icc(icc_profile)
        exposure_on_device(params.get("exposure"))
        return self._export(TiffExport(bits, icc), src, None, negative_film, grain_size, grain_sigma, "cpu", stream, file,
                            dict(params, output_bits=bits))

    def process_preloaded_tiff(self, cpu_payload, negative_film, grain_size, grain_sigma, file=None, final_scaling="gpu", *,
                               output_bits=16, icc_profile=b"", stream=False, **settings):
        """The batch export on the two-phase API: process_preloaded's render of a phase-1 payload as a TIFF file like
        process_tiff's.  The processor's device frame is left alone.  stream=True: a payload process_preloaded streams in row bands
        is written band by band (else `stream_rejected` says why not)."""
        settings["output_bits"] = bits = check_output_bits(output_bits)
        return self._export(TiffExport(bits, tiff.check_icc(icc_profile)), None, cpu_payload, negative_film, grain_size, grain_sigma,
                            final_scaling, stream, file, settings)

    def _encode_device(self, image_u8, o):
        """A uint8 (H, W, 3) device frame -> the JPEG file's bytes, with the checked options `o` (jpeg_options.checked_options).
        The encoder runs on the current stream; reading its 8-byte
        length back is the one synchronisation (optimize and progressive add one for the symbol counts), then only the file crosses PCIe, into a
        pinned buffer this processor keeps (grown to the largest file so far; a pageable download of a 47 MB file cost up to 34 ms)
        and from there into the bytes object -- with the EXIF APP1 and the other segments of `o.extras` spliced in
        on the way, in the same single copy."""
        if image_u8.stride(2) != 1 or image_u8.stride(1) != 3 or image_u8.stride(0) < 3 * image_u8.shape[1]:
            image_u8 = image_u8.contiguous()  # (a row-strided view is encoded in place)
        out, length = self.ctx.jpeg_encode(image_u8, o.quality, o.subsampling, o.optimize, o.progressive,
                                           o.extras.restart(int(image_u8.shape[1]), o.subsampling), o.extras.density)
        n = int(length.item())
        if n <= 0:
            raise RuntimeError("r2f_jpeg_encode reported an empty file")
        host = self._jpeg_host
        if host is None or host.numel() < n:
            host = self._jpeg_host = self._torch.empty(max(n, 1 << 20), dtype=self._torch.uint8, pin_memory=True)
        host[:n].copy_(out[:n])  # (synchronous: the bytes are there when it returns)
        segments = o.extras.segments(o.exif)
        if segments:
            data = host[:n].numpy().data
            return b"".join((data[:20], segments, data[20:]))
        return host[:n].numpy().tobytes()

    def _process_streamed(self, payload, negative_film, grain_size, grain_sigma, settings):
        """process() of a large host frame that is uploaded for this one render (cache=False: the GUI's export calls,
        gui.py:2374,2458,2479): the frame goes through the pipeline in `stream_bands` row bands WHILE IT ARRIVES -- band k is clamped and taken through S0 + S1
        as soon as it is on the device, the halation of band k - 1 follows (its stencil reads the first rows of band k), then the
        MTF and the tail of band k - 2, whose uint8 rows start their way back while later bands are still coming up: the stage
        entry points are row-range calls (the ones a row shard makes: grain hashed at global coordinates, reflection at the frame
        edges only, the exposure-range record kept like r2f_render keeps it), PCIe is full duplex, and what remains of the render
        and the download behind the upload is the last two bands' share.  At 100 MP: upload 21.1 ms, render 4.7, download 5.3
        one after the other = 32.5 ms; streamed 23.3 (bench.py host_device_copies, tools/stream_bands_probe.py).
        The FFT stencils' windows are anchored at a call's first row, so a band's outputs agree with the whole-frame render's to the
        FFT form's rounding (an fp32 ulp on a handful of samples, like a row shard's); pointwise configurations agree bit for bit.
        A uint16 frame (LibRaw's 16-bit output: half the upload) is converted band by band on the device as it arrives.
        A Bayer mosaic (a sixth of the upload) is demosaiced band by band into the float frame: its bands reach 4 mosaic rows into
        their neighbours, which travel with the band that needs them first (payload.mosaic_upload_bounds).
        bands.py holds the host-side plan: the bands (plan_bands), the order in which the stages take them (stage_schedule) and
        what each kind of payload does to get its rows into the float frame (band_source); _run_bands holds the mechanics.
        `payload`: the frame's, as process() extracted it.  Returns None when it does not qualify (the caller then takes the
        one-after-the-other path with the same payload): a device pre-path (rotation, chroma NR, scaling), a canvas, a highlight burn
        (a function of the whole grained frame), a small frame.
        The two-phase API's device phase (process_preloaded, submit_preloaded: batch export) streams its payload the same way."""
        return self._stream_payload(payload, negative_film, grain_size, grain_sigma, "cpu", **settings)

    def _stream_payload(self, payload, negative_film, grain_size, grain_sigma, final_scaling="cpu", **settings):
        """A phase-1 payload (extract_image_data_cpu) through the pipeline in row bands while it arrives: see _process_streamed.
        Returns the uint8 frame, or None (with `stream_rejected` saying why) when the payload does not qualify."""
        def make_sink(depth, out, bounds):
            return depth.pool.sink(tuple(out.shape), self.result_buffers), None

        res = self._stream(payload, negative_film, grain_size, grain_sigma, final_scaling, settings, make_sink)
        return None if res is None else _host16(res)

    def _stream(self, payload, negative_film, grain_size, grain_sigma, final_scaling, settings, make_sink):
        """The streamed render behind _stream_payload and _export, which differ in where the finished rows go:
        plan the bands, make the sink -- make_sink(depth, the frame's result buffer on the device, band bounds) -> (sink, band_done):
        a ResultSink or one with its interface and None, or a sink that downloads nothing itself and its band_done(b), called once
        band b's tail is queued --, run the bands, finish.  A finish() that raises is drained and abandoned like a band that does.
        Returns sink.finish()'s value, or None (with `stream_rejected` saying why) when the payload does not qualify."""
        frame = self._stream_plan(payload, negative_film, grain_size, grain_sigma, final_scaling, settings)
        if frame is None:
            return None
        depth = self._depths[settings.get("output_bits", 8)]
        out = self._stream_result(frame.bufs, depth)
        sink, band_done = make_sink(depth, out, frame.bounds)
        try:
            self._run_bands(frame, sink, out, depth, band_done)
            self._collect_auto_exposure()
            res = sink.finish()
        except BaseException:
            # a stage call refused, a write raised (or the caller interrupted): let the queued work drain, hand a lent buffer back,
            # stop the copies and the writes, pass it on (the next export begins a new row-wise encode)
            self._torch.cuda.synchronize(self.device)
            sink.abandon()
            raise
        # (the frame kept on the device for re-renders -- a preview's, typically -- is left alone: an export in between does not cost
        # the preview its cached frame, which the one-after-the-other path has to overwrite because it works in it)
        self.last_output = out
        return res

    def _stream_plan(self, payload, negative_film, grain_size, grain_sigma, final_scaling, settings):
        """Qualify a payload for the row-band path and set its frame up: its bands.StreamedFrame, or None with `stream_rejected`
        saying why it does not stream."""
        host = self._payload_tensor(payload)
        self.stream_rejected = stream_rejection(payload, tuple(host.shape), str(host.dtype), host.is_cuda, final_scaling,
                                                settings.get("canvas_mode", "No"))
        if self.stream_rejected is not None:
            return None
        self.exposure_rejected = payload.get("exposure_rejected")
        repair = (payload.get("demosaic") or {}).get("repair")  # (every band's repair adds to the frame's count word: bands.band_source)
        source = band_source(payload, tuple(host.shape), str(host.dtype), None if repair is None else self._begin_repair_record(repair))
        H, W = source.frame[:2]
        params = self.prepare(negative_film, grain_size, grain_sigma, (W, H), **settings)
        hal, mtf = bool(params.flags & _lib.F_HALATION), bool(params.flags & _lib.F_MTF)
        ha = self._halation_reach if hal else (0, 0)
        ma = self._mtf_reach if mtf else (0, 0)
        bounds, self.stream_rejected = plan_bands(H, int(params.flags), ha, ma, self.stream_bands, self.stream_taper)
        if bounds is None:
            return None
        bufs = self._stream_buffers(source, mtf, settings.get("output_bits", 8))
        p = _lib.Params.from_buffer_copy(params)
        p.flags |= _lib.F_FRAME_RESIDENT  # the seed is written once, here; the stage calls read it from the frame block
        self.ctx.write_frame_params(p)     # (and the exposure-range record starts empty)
        return StreamedFrame(host, source, p, bounds, bufs, ha, ma)

    def _stream_buffers(self, source, mtf, bits=8):
        """The device buffers the streamed frame of `source` (a bands.BandSource) works in, kept for the next frame of the same kind:
        the float frame, the stages' planes, the result, and the int16 buffer a uint16 frame or a Bayer mosaic lands in, which has
        the payload tensor's shape (a mosaic is demosaiced straight into the float frame: no uint16 (H, W, 3) frame exists)."""
        torch = self._torch
        H, W, _ = shape = source.frame  # (a float payload with upstream's alpha plane, gpu_processor.py:765: 4 channels)
        bufs = self._stream_bufs
        if bufs is None or bufs["shape"] != shape or bufs["mtf"] != mtf:
            bufs = self._stream_bufs = {"shape": shape, "mtf": mtf, "image": torch.empty(shape, dtype=torch.float32, device=self.device)}
            for k in ("E", "D", "D2") if mtf else ("E", "D"):
                bufs[k] = torch.empty((3, H, W), dtype=torch.float32, device=self.device)
        if bufs.get(source.landing) is None or tuple(bufs[source.landing].shape) != source.landing_shape:  # (never the float frame)
            bufs[source.landing] = torch.empty(source.landing_shape, dtype=torch.int16, device=self.device)
        self._stream_result(bufs, self._depths[bits])
        return bufs

    def _stream_result(self, bufs, depth):
        """The result buffer of a streamed frame at `depth` among its device buffers, made when a frame first asks for that width
        (int16 holds the bits of a 16-bit one)."""
        key = ("out", depth.bits)
        if bufs.get(key) is None:
            bufs[key] = self._torch.empty(bufs["shape"][:2] + (3,), dtype=depth.torch_dtype, device=self.device)
        return bufs[key]

    def _run_bands(self, frame, sink, out, depth, band_done=None):
        """_stream's band loop (see _process_streamed) over `frame`, _stream_plan's StreamedFrame: the copies, their events and the
        one context call that each pair of bands.stage_schedule stands for; frame.source (bands.band_source) knows how the rows of
        frame.host reach the float frame.  The tail's rows -- written into `out`, the result at `depth` -- go back into `sink` -- or,
        with `band_done`, band_done(b) is called instead once band b's tail is queued (on the launching stream; the JPEG export's sink)."""
        torch, ctx = self._torch, self.ctx
        host, source, p, bounds, bufs, ha, ma = frame
        H, n = int(bounds[-1]), len(bounds) - 1
        hal, mtf, grain = (bool(p.flags & f) for f in (_lib.F_HALATION, _lib.F_MTF, _lib.F_GRAIN))
        pointwise = not (hal or mtf or grain)
        image, E, D = bufs["image"], bufs["E"], bufs["D"]
        landing, ub = bufs[source.landing], source.upload_bounds(bounds)
        up, down = self._copy_streams()
        compute = torch.cuda.current_stream(self.device)
        up.wait_stream(compute)  # (the buffers may still be read by the previous frame's launches)
        down.wait_stream(compute)

        def send_up(k):
            with torch.cuda.stream(up):
                landing[ub[k]:ub[k + 1]].copy_(host[ub[k]:ub[k + 1]], non_blocking=True)
                return up.record_event()

        def send_back(b):
            if band_done is not None:
                band_done(b)
                return
            y0, y1 = bounds[b], bounds[b + 1]
            done = compute.record_event()
            with torch.cuda.stream(down):
                down.wait_event(done)
                sink.target[y0:y1].copy_(out[y0:y1], non_blocking=True)
                sink.band_back(down.record_event() if sink.per_band else down, y0, y1)

        # A copy out of ordinary (pageable) host memory -- any NumPy array that was not made from pinned memory -- returns only when
        # its bytes have left the host: issued from this thread, every band's copy would hold back the launches of the band before
        # it (measured: 35.5 ms against 32.7 one after the other).  So such a source is sent up by a helper thread of its own, band
        # by band, and this thread launches a band when its arrival event is there.
        uploader = None if host.is_pinned() else ThreadPoolExecutor(max_workers=1, thread_name_prefix="r2f-upload",
                                                                     initializer=torch.cuda.set_device, initargs=(self.device,))
        arrivals = None if uploader is None else [uploader.submit(send_up, k) for k in range(n)]
        queued = [send_up(k) for k in range(n)] if source.queue_all and uploader is None else None

        def arrival(k):
            if queued is not None:
                return queued[k]
            return send_up(k) if arrivals is None else arrivals[k].result()

        awaited = set()

        def wait(k):  # the launching stream awaits upload k: once, ahead of whatever reads it first
            if k not in awaited:
                awaited.add(k)
                compute.wait_event(arrival(k))

        ident = 0  # the last front call's identity flag
        try:
            if source.measure is not None:
                source.measure(ctx, landing, ub, wait)
                self._auto_exposure_pending = True
            for stage, b in stage_schedule(n, hal, mtf, pointwise):
                y0, y1 = bounds[b], bounds[b + 1]
                if stage == "front":
                    wait(b)
                    source.decode(ctx, landing, image, y0, y1)
                    rows = image[y0:y1]
                    if pointwise:  # LUTs only: one fused pass per band, straight to the result
                        depth.front(rows, p, out, in_gy0=y0, out_gy0=0, y0=y0, y1=y1, H_global=H)
                    elif hal:
                        ident = ctx.stage_front_split(rows, p, E, D, in_gy0=y0, y0=y0, y1=y1, H_global=H, track_range=True)
                    else:
                        ctx.stage_front(rows, p, 1, in_gy0=y0, dst=D, dst_gy0=0, y0=y0, y1=y1, H_global=H)
                elif stage == "halation":
                    lo, hi = max(y0 - ha[0], 0), min(y1 + ha[1], H)
                    ctx.stage_halation(E[:, lo:hi], D, p, src_gy0=lo, dst_gy0=0, y0=y0, y1=y1, H_global=H, identity_done=ident,
                                       range_valid=True)
                elif stage == "mtf":
                    lo, hi = max(y0 - ma[0], 0), min(y1 + ma[1], H)
                    ctx.stage_mtf(D[:, lo:hi], bufs["D2"], p, src_gy0=lo, dst_gy0=0, y0=y0, y1=y1, H_global=H)
                else:  # "tail": a pointwise band is finished already
                    if not pointwise:
                        depth.tail(bufs["D2"] if mtf else D, p, out, src_gy0=0, out_gy0=0, y0=y0, y1=y1, H_global=H)
                    send_back(b)
        finally:
            if uploader is not None:
                uploader.shutdown(cancel_futures=True)

    def _copy_streams(self):
        """(host-to-device, device-to-host) copy streams of this processor, made on first use."""
        if self._up_stream is None:
            self._up_stream = self._torch.cuda.Stream(device=self.device)
            self._down_stream = self._torch.cuda.Stream(device=self.device)
        return self._up_stream, self._down_stream

    def _download(self, out):
        """The result, uint8 or 16-bit, as a NumPy array (results.py): with result_buffers = n > 0 a view of one of n pinned buffers
        (24 MP: 1.5 instead of 6 ms to come down); else the caller's own array, from 3 M samples up a lent pinned buffer (2.7 instead
        of 7.8 ms)."""
        sink = None
        depth = self._depths[8 * out.element_size()]  # a 16-bit result: the same ways back, from the pool of its own width
        if self.result_buffers > 0 or out.numel() >= (3 << 20):
            sink = depth.pool.sink(tuple(out.shape), self.result_buffers, staged=False)
        if sink is None:
            return _host16(out.cpu().numpy())
        sink.target.copy_(out, non_blocking=True)
        sink.band_back(self._torch.cuda.current_stream(self.device), 0, int(out.shape[0]))
        return _host16(sink.finish())

    def _payload_tensor(self, cpu_payload):
        """The payload's frame as a torch tensor: float32, or the 16 bits of a uint16 frame (as int16: same bytes)."""
        torch = self._torch
        image = cpu_payload["image_array"]
        if isinstance(image, np.ndarray):
            if image.dtype == np.uint16:
                return torch.from_numpy(np.ascontiguousarray(image).view(np.int16))
            return torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32))
        return image

    def submit_preloaded(self, cpu_payload, negative_film, grain_size, grain_sigma, final_scaling="gpu", **settings):
        """process_preloaded without waiting: the upload runs on a copy stream, the render on the current stream, the download
        of the uint8 result into pinned host memory on a second copy stream; returns a `PendingFrame` whose `.result()` is
        process_preloaded's return value.  Keeping one frame pending while the next one is submitted overlaps both PCIe
        directions with the render (raw2film_amd.sharding.BatchSharder.run(..., collect=...) does exactly that) -- what the
        reference's queue.write_texture / read_texture pair serialises."""
        check_output_bits(settings.get("output_bits", 8))
        torch = self._torch
        self.exposure_rejected = self.last_raw_scale = self.last_raw_denoise = self.last_raw_repair = None
        src = cpu_payload.get("image_array")
        if self.stream_bands > 1 and not (isinstance(src, torch.Tensor) and (src.is_cuda or src.is_pinned())):
            # a large frame in ordinary (pageable) host memory: its copy blocks this thread, so nothing of the next frame's host work
            # would overlap it -- it overlaps its own upload, render and download band by band instead (_process_streamed; 24 MP:
            # 7.0 against 7.5 ms, uint16 4.7 against 5.0) and is back when this call returns.  A pinned payload keeps the
            # frame-in-flight scheme below (2.9 against 3.5 ms for uint16: tools/batch_pageable_probe.py)
            res = self._stream_payload(cpu_payload, negative_film, grain_size, grain_sigma, final_scaling, **settings)
            if res is not None:
                return PendingFrame.finished(res)
        up, down = self._copy_streams()
        image = self._payload_tensor(cpu_payload)
        # (A pageable source -- an ordinary NumPy array -- makes the "asynchronous" copy below a synchronous one: this thread waits
        # for the frame's bytes to leave the host.  That is fine: the frame before is already queued on the device and its render
        # and download run meanwhile.  Pinning the array first, which this method did until round 6, is a fresh pinned allocation
        # and a single-threaded host copy per frame: 64 instead of 6.3 ms per 24 MP frame, tools/batch_pageable_probe.py.)
        compute = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(up):
            dev = image.to(self.device, non_blocking=True)
            uploaded = up.record_event()
        compute.wait_event(uploaded)
        dev.record_stream(compute)
        # (a frame in flight: the stops of exposure="device" are read back when `last_auto_exposure` is asked for, not here -- the read
        # waits for this frame's upload and statistic, the time in which the caller prepares the next frame)
        self._defer_exposure_read = True
        try:
            out = self._render_preloaded(dev, cpu_payload, negative_film, grain_size, grain_sigma, None, None, final_scaling, **settings)
        finally:
            self._defer_exposure_read = False
        rendered = compute.record_event()
        with torch.cuda.stream(down):
            down.wait_event(rendered)
            host = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
            host.copy_(out, non_blocking=True)
            out.record_stream(down)
            done = down.record_event()
        return PendingFrame(host, done)

    def _render_preloaded(self, image, cpu_payload, negative_film, grain_size, grain_sigma, dst_texture, histogram_texture,
                          final_scaling, **settings):
        """The device half of process_preloaded on an uploaded frame; returns the uint8 device result (None with a dst_texture)."""
        image, layout = self._prepare_device_frame(image, cpu_payload)
        return self._render_prepared(image, layout, cpu_payload, negative_film, grain_size, grain_sigma, dst_texture,
                                     histogram_texture, final_scaling, **settings)

    def _prepare_device_frame(self, image, cpu_payload):
        """The device pre-path on an uploaded payload frame -> (frame, layout) as the pipeline reads it."""
        torch, cut_and_turn = self._torch, self._cut_and_turn
        demosaic_step = cpu_payload.get("demosaic")
        if demosaic_step:  # a mosaic: LibRaw's share of raw_to_linear on the device -> the uint16 frame of the lines below
            image = self._demosaic_mosaic(image.contiguous(), demosaic_step)
        if image.dtype in (torch.int16, torch.uint16):  # a decoded 16-bit frame: raw_conversion.py:50-52 on the device
            if cpu_payload.get("u16_factor") is None:
                raise ValueError("a uint16 payload needs its exposure factor (`u16_factor`, extract_image_data_cpu sets it)")
            self.exposure_rejected = cpu_payload.get("exposure_rejected")
            if cpu_payload["u16_factor"] == DEVICE_EXPOSURE:
                # statistic, finish, decode from the record: queued one behind the other, no host synchronisation in between
                image = image.contiguous()
                root = cpu_payload["exposure_root"]
                self.ctx.exposure_rows(image, root)
                self.ctx.exposure_finish(int(image.shape[0]), int(image.shape[1]), root)
                self._auto_exposure_pending = True
                image = self.ctx.decode_u16_auto(image, cpu_payload["u16_window"])
            else:
                image = self.ctx.decode_u16(image.contiguous(), cpu_payload["u16_factor"])
        elif cpu_payload.get("clip_on_device"):
            image = image.clamp_(0.0, 65504.0)  # np.clip(image, 0, 65504) of gpu_processor.py:275, on the uploaded copy
        layout = None  # the payload is (H, W, C) like the reference's; the device pre-path hands on (3, H, W) planes
        lens_step = cpu_payload.get("lens")
        if lens_step:  # lens correction (effects.lens_correction) of the whole frame, into the window the crops keep
            corrected = self.ctx.lens_correct(image.contiguous(), lens_step["params"], lens_step["window"], tca=lens_step.get("tca"),
                                              projection=lens_step.get("projection"))
            image = cut_and_turn(corrected, None, lens_step.get("rotate_times")).contiguous()  # (the planes themselves unless they were turned)
            layout = "chw"
        warp = cpu_payload.get("warp")
        if warp:  # free rotation (effects.rotate) + the crops behind it + quarter turns (np.rot90 on the planes)
            image = cut_and_turn(self.ctx.warp_affine(image.contiguous(), warp["m_dst_to_src"], warp["window"], layout=layout), None,
                                 warp["rotate_times"]).contiguous()
            layout = "chw"
        if cpu_payload.get("chroma_nr"):  # pre-path chroma NR (effects.py:547-561): XYZ planes out, CHW into the pipeline
            image, layout = self.ctx.chroma_nr(image.contiguous(), cpu_payload["chroma_nr"], layout=layout), "chw"
        if cpu_payload.get("resize_to"):  # preview scaling, after the NR like cpu_processor.py:119-134
            _, h_in, w_in = self.ctx.layout_of(image, layout)
            rt = cpu_payload["resize_to"]
            if rt[0] <= h_in and rt[1] <= w_in:  # cv.INTER_AREA
                image, layout = self.ctx.resize_area(image.contiguous(), *rt, layout=layout), "chw"
            else:  # cv.INTER_LANCZOS4 on the float frame (utils.py:237-242)
                image, layout = self.ctx.resize_lanczos4_f32(image.contiguous(), *rt, layout=layout), "chw"
        return image, layout

    def _render_prepared(self, image, layout, cpu_payload, negative_film, grain_size, grain_sigma, dst_texture, histogram_texture,
                         final_scaling, **settings):
        """The pipeline and the post-path on a prepared device frame (which is only read: it can be rendered again).  At 16 bits
        (r2f_render16; an int16 tensor holds the uint16 frame's bits) the post-path is the same on the wider frame: the canvas colour
        c * 257 (255 -> 65535), cv.resize(uint16, ...) for the two scalings."""
        if dst_texture is not None:
            self._check_texture(dst_texture, "dst_texture")
        if histogram_texture is not None:
            self._check_texture(histogram_texture, "histogram_texture")
            if dst_texture is None:
                raise ValueError("histogram_texture needs dst_texture (gpu_processor.py:1883: the histogram is only drawn on the "
                                 "destination-texture branch)")
        depth = self._depths[check_output_bits(settings.get("output_bits", 8), dst_texture)]
        out_f32, out = self._execute_pipeline(image, negative_film, grain_size, grain_sigma, want_f32=dst_texture is not None,
                                              want_out=True, layout=layout, **settings)
        self._collect_auto_exposure()
        if dst_texture is not None:
            # GpuProcessor's destination branch (gpu_processor.py:1865-1890): letterbox the float frame into the widget's
            # texture with copy_to_int.wgsl's transform, draw the histogram into its own texture, return nothing
            H, W = int(out_f32.shape[0]), int(out_f32.shape[1])
            color = None
            if settings.get("canvas_mode", "No") != "No":
                _, color, _ = geometry.canvas_layout((H, W), settings["canvas_mode"], settings.get("canvas_scale", 1.0),
                                                     settings.get("canvas_ratio", 1.0))
            t = geometry.blit_transform((W, H), (int(dst_texture.shape[1]), int(dst_texture.shape[0])),
                                        pipeline_resolution=cpu_payload.get("pipeline_resolution"),
                                        output_resolution=cpu_payload.get("output_resolution"),
                                        canvas_resolution=cpu_payload.get("canvas_resolution"), canvas_color=color)
            self.ctx.blit_rgba8(out_f32, dst_texture, t)
            self.last_output = out
            if histogram_texture is not None:
                from . import histogram

                self.ctx.histogram_render(self.ctx.histogram_counts(out), histogram.MIX_TABLE, 256, target=histogram_texture)
            return None
        # canvas on the device result (cpu_processor.py:409 / copy_to_int.wgsl): a paste, no arithmetic
        out = geometry.add_canvas(out, settings.get("canvas_mode", "No"), settings.get("canvas_scale", 1.0),
                                  settings.get("canvas_ratio", 1.0))
        target = cpu_payload.get("final_resolution") if final_scaling == "cpu" else cpu_payload.get("upscale_to")
        if target:  # cpu_processor.py:411-412 -> utils.resolution_scaling (utils.py:226-244) on the finished frame
            f = min(target[0] / out.shape[0], target[1] / out.shape[1])
            size = (round(out.shape[0] * f), round(out.shape[1] * f))
            if f > 1:  # cv.INTER_LANCZOS4
                out = depth.resize_lanczos4(out.contiguous(), *size)
            elif f < 1 and final_scaling == "cpu":  # cv.INTER_AREA: the CPU processor shrinks the canvas-framed frame
                out = depth.resize_area(out.contiguous(), *size)
        self.last_output = out
        return out

    def _begin_repair_record(self, repair):
        """Begin the frame's `last_raw_repair` -> the device word, at 0, to which its repair adds the samples it replaces."""
        count = self._torch.zeros(1, dtype=self._torch.int32, device=self.device)
        self._raw_repair = {"threshold": repair.threshold, "q": repair.q, "min_neighbours": repair.min_neighbours, "repaired": count}
        return count

    def _repair_mosaic(self, mosaic, repair, profile):
        """process(raw_repair=)'s device step in one piece: r2f_mosaic_repair of `mosaic` into the context's second mosaic, which is
        returned."""
        params = repair.plan(profile, int(mosaic.shape[0]), int(mosaic.shape[1]))
        return self.ctx.mosaic_repair(mosaic, params, count=self._begin_repair_record(repair))

    def _cut_and_turn(self, image, window, k, dims=(1, 2)):
        """How a whole-frame step ends: the window it did not cut itself (None: it did), then k quarter turns (np.rot90's)."""
        if window is not None:
            r0, c0, nr, nc = window
            image = image[r0:r0 + nr, c0:c0 + nc]
        return self._torch.rot90(image, k, dims) if k else image

    def _demosaic_mosaic(self, image, step):
        """The payload's `demosaic` step on an uploaded mosaic in one piece: repair, measure and resolve, denoise, demosaic, cut and
        turn -> the uint16 frame the hand-off decodes."""
        params, kind = step["params"], _lib.MOSAIC_KINDS[type(step["params"])]
        deferred, clip = step.get("levels"), step.get("clip")
        repair = step.get("repair")
        if repair is not None:
            # ahead of everything else that reads the mosaic: the measurement, the denoise and the demosaic below run unchanged,
            # on the second mosaic the context keeps
            image = self._repair_mosaic(image, repair, step["profile"])
        H, W = int(image.shape[0]), int(image.shape[1])
        if deferred is not None:
            # the scale is the frame's own: the whole uploaded mosaic's data maximum (one read of it, 4 bytes back, the one
            # synchronisation of this path), LibRaw's rule on it, and the params planned again with the resolved numbers
            d = self.ctx.mosaic_maximum(image, deferred)
            resolved, scale = deferred.resolve_scale(d)
            self.last_raw_scale = {"data_maximum": d, "maximum_used": int(scale.maximum_used), "adjusted": bool(scale.adjusted)}
            params, clip = resolved.plan(H, W, kind.reduced(params)), resolved.blend_clip
        denoise = step.get("denoise")
        if denoise is not None:
            # behind the measurement and the resolve, which see the UNdenoised mosaic as LibRaw's adjust_maximum does; the
            # denoised mosaic is black-free and in units of t << shift, and the demosaic is planned again for that
            profile = resolved if deferred is not None else step["profile"]
            maximum = denoise.maximum if denoise.maximum is not None else int(scale.maximum_used)
            dn = denoise.plan(profile.black, H, W, maximum)
            self.last_raw_denoise = {"threshold": denoise.threshold, "maximum": int(maximum), "shift": int(dn.shift)}
            image = self.ctx.mosaic_denoise(image, dn)
            params = denoise.shifted(profile, dn.shift).plan(H, W, kind.reduced(params))
        # (clip: highlight mode 2's level or None; median: LibRaw's med_passes or 0 -- the options pick the entry point)
        frame = self.ctx.demosaic(image, params, clip=clip, passes=step.get("median", 0), orientation=step.get("orientation", 0))
        return self._cut_and_turn(frame, step["window"], step["rotate_times"], dims=(0, 1))

    @property
    def last_raw_repair(self):
        """What the hot-pixel repair of the frame rendered last ran with and did: {"threshold", "q", "min_neighbours", "repaired"},
        or None when the call had no raw_repair.  `repaired`, the number of samples replaced, is counted on the device and read back
        by the first look at this attribute (4 bytes; it waits for the repair, not for the render): nothing on the render path
        waits for it.  A cached frame keeps its record."""
        record = self._raw_repair
        if record is not None and not isinstance(record["repaired"], int):
            record["repaired"] = int(record["repaired"].item())
        return record

    @last_raw_repair.setter
    def last_raw_repair(self, record):
        self._raw_repair = record

    def _collect_auto_exposure(self, now=False):
        """exposure="device": once the frame is queued, the stops the device measured come back into `last_auto_exposure` (the wait
        is for the finish kernel behind the upload, not for the render).  submit_preloaded's frame in flight leaves the read to the
        first look at `last_auto_exposure` (now=True)."""
        if self._auto_exposure_pending and (now or not self._defer_exposure_read):
            self._auto_exposure_pending = False
            self._last_auto_exposure = self.ctx.exposure_result()[0]

    @property
    def last_auto_exposure(self):
        """Stops the device measured for the last exposure="device" frame, else what was stored last.  After submit_preloaded
        the first read synchronises with the device: it may block until the frame in flight has been uploaded and measured
        (not until it is rendered).  After process / process_preloaded the value is already on the host and the read is free."""
        self._collect_auto_exposure(now=True)
        return self._last_auto_exposure

    @last_auto_exposure.setter
    def last_auto_exposure(self, stops):
        self._auto_exposure_pending = False
        self._last_auto_exposure = stops

    def generate_histogram(self, image=None, mix_table=None, height=100):
        """utils.generate_histogram (utils.py:145-223) of `image` (uint8 (H, W, 3), NumPy or device) -- or, with no image,
        of the frame the last process() call rendered, counted on the device before it ever left it (the GUI calls this
        right after process(), gui.py:2225).  Returns the (height, 256, 4) uint8 bar image."""
        from . import histogram

        if image is None:
            image = self.last_output
            if image is None:
                raise ValueError("generate_histogram(): no frame has been rendered yet")
            if image.dtype == self._torch.int16:
                # a 16-bit render: v // 257 is the bin of the 8-bit render of the same float (both truncate), counted on the device
                image = torch_div257(self._torch, image)
        return histogram.generate_histogram(image, histogram.MIX_TABLE if mix_table is None else mix_table, height,
                                            ctx=self.ctx)

    def process_array(self, image, negative_film, grain_size=6, grain_sigma=0.4, *, colorspace="XYZ", seed=None,
                      return_float=False, output="host", out=None, output_bits=8, **settings):
        """Render a decoded frame given as an array / CUDA tensor (synthetic benchmark frames).

        colorspace: "XYZ" (S0 skipped) or "linear-rec709" (S0 = data.py:128-135).
        return_float: float32 display-referred (H, W, 3) instead of uint8.  output: "host" | "device".
        out: a device tensor (H, W, 3) of the result's dtype to render into (a stream of frames then keeps its buffers, and
        r2f_render its captured graph).
        output_bits=16: the uint16 result of r2f_render16 (clip(x * 65535, 0, 65535) truncated) instead of uint8; with
        output="device" the device tensor (torch.uint16).  Not together with return_float.
        """
        if check_output_bits(output_bits) == 16 and return_float:
            raise ValueError("output_bits=16 and return_float=True name two different results")
        torch = self._torch
        if colorspace not in ("XYZ", "linear-rec709"):
            raise ValueError("colorspace must be 'XYZ' or 'linear-rec709'")
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32))
        image = image.to(self.device).contiguous()
        if out is not None:
            _, H, W = self.ctx.layout_of(image, settings.get("layout"))
            want = torch.float32 if return_float else torch.uint8 if output_bits == 8 else torch.uint16
            if output_bits == 16 and isinstance(out, torch.Tensor) and out.dtype == torch.int16:
                want = torch.int16  # (the same bits)
            if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == want and tuple(out.shape) == (H, W, 3) and out.is_contiguous()):
                raise ValueError(f"out must be a contiguous {want} CUDA tensor of shape {(H, W, 3)}")
        f32, res = self._execute_pipeline(
            image, negative_film, grain_size, grain_sigma, want_f32=return_float, want_out=not return_float,
            matrix=REC709_TO_XYZ if colorspace == "linear-rec709" else None, seed=seed,
            out_f32=out if return_float else None, out=None if return_float else out, output_bits=output_bits, **settings,
        )
        out = f32 if return_float else res
        if output_bits == 16:
            out = out.view(torch.uint16)
            return out if output == "device" else out.view(torch.int16).cpu().numpy().view(np.uint16)
        return out if output == "device" else out.cpu().numpy()

    # ------------------------------------------------------------------ device pipeline
    def prepare(self, negative_film, grain_size, grain_sigma, pipeline_resolution, *, print_film=None, exp_comp=0.0,
                red_light=0.0, green_light=0.0, blue_light=0.0, projector_kelvin=6500, shadow_comp=0.0, sat_adjust=1.0,
                gamma_func="sRGB", exp_kelvin=6500, tint=0.0, inversion_gamma=4.0, idealized_curve=False,
                inversion=False, push_pull=0.0, white_balance=False, white_clip=False, icc_transform=None,
                frame_width=36, frame_height=24, halation_intensity=1.0, halation=True, halation_size=1.0,
                halation_green_factor=0.4, sharpness=True, sharpening_strength=0.0, sharpening_sigma=1.0, grain=2,
                highlight_burn=0.0, burn_scale=50.0, color_masking=None, matrix=None, seed=None, lut3d_mode=0, **_):
        """Upload whatever changed and return the r2f_params for this render: the table half of
        `_execute_gpu_pipeline` (gpu_processor.py:1735-1756, 1772-1825)."""
        self.pipeline_resolution = (int(pipeline_resolution[0]), int(pipeline_resolution[1]))
        self.load_input_lut(negative_film, exp_kelvin, tint, exp_comp)
        self.load_density_curve(negative_film, push_pull, color_masking)
        self.load_output_lut(negative_film, print_film, red_light, green_light, blue_light, projector_kelvin,
                             shadow_comp, sat_adjust, gamma_func, inversion_gamma, idealized_curve, inversion,
                             white_balance, white_clip, icc_transform, color_masking)
        scale = max(pipeline_resolution) / max(frame_width, frame_height)  # px per mm, cpu_processor.py:366
        do_hal = bool(halation)
        do_mtf = bool(sharpness) and negative_film.mtf is not None
        do_grain = bool(grain) and negative_film.rms_density is not None
        if do_hal:
            self.load_halation_kernel(scale, halation_size=halation_size, halation_green_factor=halation_green_factor,
                                      halation_intensity=halation_intensity, bw=negative_film.density_measure == "bw")
        if do_mtf:
            self.load_mtf_kernel(negative_film, scale, sharpening_strength, sharpening_sigma)
        if do_grain:
            self.load_grain(negative_film, scale, grain_size / 1000, grain_sigma, grain == 1)
        mkey = None if matrix is None else np.asarray(matrix, dtype=np.float32).tobytes()
        if mkey != self.matrix_key:
            self.ctx.set_matrix3x3(matrix)
            self.matrix_key = mkey
        if seed is None:
            seed = random.randint(0, 100000000)  # gpu_processor.py:591: a new seed every render
        # S7 gate: cpu_processor.py:399-402
        do_burn = bool(highlight_burn) and (print_film is not None or negative_film.density_measure in ["status_m", "bw"])
        burn_kw = {}
        if do_burn:
            burn = self.load_highlight_burn(negative_film, highlight_burn, burn_scale, pipeline_resolution)
            burn_kw = dict(burn_strength=float(burn["highlight_burn"]), burn_d_ref=float(burn["d_ref"]), burn_cell=burn["cell"])
        return self.ctx.make_params(matrix=matrix is not None, halation=do_hal, mtf=do_mtf, grain=do_grain,
                                    grain_mono=grain == 1, seed=seed, lut3d_mode=lut3d_mode,
                                    log_eps=LOG_EPS, lut3d_scale=LUT3D_SCALE, **burn_kw)

    def _execute_pipeline(self, image, negative_film, grain_size, grain_sigma, want_f32=False, want_out=True, layout=None,
                          out_f32=None, out=None, **settings):
        """Tables (re-uploaded only when their parameters changed) + ONE r2f_render (r2f_render16 with output_bits=16, whose result
        `out` then names): the frame's launches are captured into a HIP graph the second time the same buffers come by and replayed
        from then on -- the counterpart of the reference's single command encoder and submit (gpu_processor.py:1760, 1877); the
        per-render seed travels in a device-side block.  -> (out_f32 or None, the result or None)."""
        _, H, W = self.ctx.layout_of(image, layout)
        params = self.prepare(negative_film, grain_size, grain_sigma, (W, H), **settings)
        return self._depths[settings.get("output_bits", 8)].render(image, params, out_f32, out, want_f32, want_out, layout)


def torch_div257(torch, image16):
    """uint8 v // 257 of a 16-bit device frame (int16 or uint16 holding uint16 bits): the 8-bit render's value of every sample."""
    v = image16.view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.div(v, 257, rounding_mode="floor").to(torch.uint8).contiguous()


_PROCESS_POSITIONAL = ("self", "src", "negative_film", "grain_size", "grain_sigma", "dst_texture", "histogram_texture", "_")  # no settings
_LOAD_KEYWORDS = tuple(inspect.signature(HipProcessor.load_image_texture).parameters)[2:]  # (self, src, then these)
