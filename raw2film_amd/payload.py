"""Phase 1 of the two-phase API as plain functions: what HipProcessor.extract_image_data_cpu derives from a decoded frame and the
load settings before anything is uploaded, and why a payload does not stream in row bands.  Pure host work: no torch, no
processor state.

The crop rule (plan_crops states it once).  There is one aspect box `a` of the frame -- for a mosaic, of the demosaiced frame, the
way round its profile's orientation puts it.
Without a free rotation there is one full window, `a` composed with the zoom box, and k = rotate_times % 4 quarter turns; with
one, the warp owns its own window (rotation_plan composed with the zoom box) and k, and what is left to cut ahead of it is `a`.
Either way the cut (and the turns that go with it) is applied once, by the last step that still sees the whole frame:
the lens step; else the device decode of an exposure="device" frame (`u16_window`; never turned or rotated: exposure_mode);
else the demosaic step; else the host, as a view of the frame plus np.rot90."""

from __future__ import annotations

import math
from collections import namedtuple
from typing import NamedTuple

import numpy as np

from . import _lib, geometry
from .lens import LensProfile
from .raw import HotPixels, RawProfile, WaveletDenoise, XTransProfile

_DEMOSAIC_REJECTED = "the demosaic step (raw_profile): "  # every refusal of a mosaic begins with it, then says why
_LENS_REJECTED = "the lens step (lens_profile): its gather reads the whole frame, which a row band does not hold"
STREAM_MIN_SAMPLES = 1 << 24  # samples of the pipeline's frame from which a frame streams (16.7 M)
DEMOSAIC_REACH = 4  # mosaic rows above and below an output row that the full-size demosaic reads (r2f_demosaic_f32): the Python
                    # statement of BayerPattern::kReachY in csrc/r2f_demosaic.hip, which the entry point checks a call against
DEVICE_EXPOSURE = "device"  # exposure="device": the auto exposure of a uint16 frame is measured on the device; also the marker a
                            # payload carries in place of its float `u16_factor`


_LEVELS_REJECTED = _DEMOSAIC_REJECTED + ("its multipliers are a RawLevels: the scale follows the mosaic's data maximum, which is known "
                                         "only after the last mosaic row has arrived")
_DENOISE_REJECTED = _DEMOSAIC_REJECTED + ("raw_denoise: the wavelet denoise ahead of it is five whole-frame passes that reach 31 plane rows "
                                          "either side; a row band does not hold them")


def mosaic_rejection(stops, rotate_times, lens, samples, xtrans=False, orientation=0, *, levels=False, denoise=False):
    """Why a mosaic is demosaiced whole instead of band by band (r2f_demosaic_f32), or None.  stops: the exposure is given in
    stops; samples: rows x cols x 3 of the window of the demosaiced frame that the pipeline takes, or None when nobody cut one;
    xtrans: the mosaic is an X-Trans one (r2f_demosaic_xtrans_u16 has the row-range contract, the band loop does not use it yet);
    orientation: the profile's (the fused demosaic-to-float of the band loop is upright; a turned band reads every mosaic row);
    levels: the profile is deferred (its multipliers are a RawLevels: r2f_mosaic_maximum of the whole mosaic comes first) -- the
    last reason asked for but one; denoise: the call denoises the mosaic (raw_denoise: r2f_mosaic_denoise of the whole mosaic comes
    first) -- the last."""
    if orientation:
        return _DEMOSAIC_REJECTED + (f"orientation = {orientation!r}: an oriented mosaic is demosaiced in one piece "
                                     "(r2f_demosaic_oriented_u16), the band loop's demosaic is upright")
    if xtrans:
        return _DEMOSAIC_REJECTED + "X-Trans mosaics do not stream yet"
    if not stops:
        return _DEMOSAIC_REJECTED + ("the exposure is not given in stops: measured on the device, its statistic is the whole demosaiced "
                                     "frame's, which is demosaiced in one piece for it")
    if int(rotate_times) % 4:
        return _DEMOSAIC_REJECTED + f"rotate_times = {rotate_times!r}: the quarter turns are applied to the whole demosaiced frame"
    if lens:
        return _DEMOSAIC_REJECTED + "the lens step (lens_profile) behind it reads the whole demosaiced frame"
    if samples is None:
        return _DEMOSAIC_REJECTED + "no window of the demosaiced frame is known for it"
    if samples < STREAM_MIN_SAMPLES:
        return _DEMOSAIC_REJECTED + f"its window of the demosaiced frame has {samples} samples, below 16.7 M"
    if levels:
        return _LEVELS_REJECTED
    if denoise:
        return _DENOISE_REJECTED
    return None


REPAIR_REACH = 2  # mosaic rows above and below a row that its repair reads (r2f_mosaic_repair; kReach of csrc/r2f_repair_math.h)


def mosaic_upload_bounds(bounds, window, Hm, half_size, median=0, repair=0) -> list:
    """The mosaic rows that travel with each band of a streamed mosaic: upload k is rows [ub[k], ub[k + 1]), and band k's demosaic
    (r2f_demosaic_f32 of the window's rows [bounds[k], bounds[k + 1])) reads nothing outside [ub[0], ub[k + 1]).  bounds: plan_bands'
    of the window's rows; window: (row0, col0, rows, cols) of the demosaiced frame; Hm: the mosaic's rows.  Full size reaches
    DEMOSAIC_REACH rows past a band's ends, half size reads the two mosaic rows of each output row; rows outside [ub[0], ub[-1])
    are never uploaded.  median: the profile's median_passes n (r2f_demosaic_median_f32: a band edge is no border of step M) --
    a band then reads the frame n output rows further either side, clipped to the frame: full size DEMOSAIC_REACH + n mosaic rows
    past its ends, half size the mosaic rows of n more output rows (2 n).  repair: REPAIR_REACH for a call with a raw_repair (band
    k then repairs the rows [rb[k], rb[k + 1]) of the answer for repair=0 before it demosaics from them, and the repair of a row
    reads `repair` rows either side of it): that many more mosaic rows travel with each band, clipped to the frame."""
    row0, rows, n, e = int(window[0]), int(window[2]), int(median), int(repair)
    assert bounds[0] == 0 and bounds[-1] == rows and n >= 0 and e >= 0
    if half_size:
        ub = [2 * max(row0 - n, 0)] + [2 * min(row0 + int(b) + n, Hm // 2) for b in bounds[1:]]
    else:
        r = DEMOSAIC_REACH + n
        ub = [max(row0 - r, 0)] + [min(row0 + int(b) + r, Hm) for b in bounds[1:-1]] + [min(row0 + rows + r, Hm)]
    return [max(ub[0] - e, 0)] + [min(b + e, Hm) for b in ub[1:]]


def frame_shape(payload, shape) -> tuple:
    """The shape of the frame the pipeline renders of a payload whose tensor has `shape`: the window of the uploaded uint16 frame
    (`u16_window`), or of the demosaiced frame (a mosaic's `demosaic` step, where it names one), else the tensor's own shape."""
    step = payload.get("demosaic")
    if step:
        window = step.get("window")
        return tuple(shape) if window is None else (int(window[2]), int(window[3]), 3)
    if payload.get("u16_window") is not None and len(shape) == 3:
        return tuple(int(v) for v in payload["u16_window"][2:]) + tuple(shape[2:])
    return tuple(shape)


def stream_rejection(payload, shape, dtype, on_device, final_scaling="cpu", canvas_mode="No"):
    """Why a phase-1 payload cannot stream through the pipeline in row bands, or None (its render's stages have the last word:
    plan_bands).  `shape`, `dtype`: of its tensor (_payload_tensor: "torch.float32", or "torch.int16" for uint16); the frame that
    is judged is frame_shape's."""
    is_u16 = dtype == "torch.int16"  # LibRaw's 16-bit output: converted band by band on the device (raw_conversion.py:50-52)
    step = payload.get("demosaic")
    if step:
        window = step.get("window")
        why = mosaic_rejection(isinstance(payload.get("u16_factor"), float), step.get("rotate_times") or 0, payload.get("lens"),
                               None if window is None else int(window[2]) * int(window[3]) * 3, is_xtrans(step.get("params")),
                               step.get("orientation", 0), levels=step.get("levels") is not None,
                               denoise=step.get("denoise") is not None)
        if why is not None:
            return why
    if payload.get("lens"):
        return _LENS_REJECTED
    shape = frame_shape(payload, shape)
    if (payload.get("warp") or payload.get("resize_to") or payload.get("upscale_to") or payload.get("chroma_nr")
            or payload.get("canvas_resolution") or canvas_mode != "No" or on_device or len(shape) != 3
            or int(shape[2]) not in (3, 4) or math.prod(shape) < STREAM_MIN_SAMPLES or dtype not in ("torch.float32", "torch.int16")
            or (payload.get("u16_factor") is None) == is_u16):  # (a uint16 frame comes with its exposure factor, a float one without)
        return ("a device pre-path, a canvas, or a frame below 16.7 M samples: " + ", ".join(
            f"{k} = {payload.get(k)!r}" for k in ("warp", "resize_to", "upscale_to", "chroma_nr", "canvas_resolution", "u16_factor",
                                                  "clip_on_device")) + f", frame {tuple(shape)} {dtype}")
    fr = payload.get("final_resolution") if final_scaling == "cpu" else None  # (cpu_processor.py:411-412: the final scaling)
    if fr is not None and (int(fr[0]), int(fr[1])) != (int(shape[0]), int(shape[1])):
        return f"the finished frame is scaled to {fr}"
    return None


def is_xtrans(params) -> bool:
    """A demosaic step's `params` are those of an X-Trans mosaic (r2f_xtrans_params), not of a Bayer one."""
    return isinstance(params, _lib.XTransParams)


def host_stream_gate(src, stream_bands, rotation=0.0, chroma_nr=0, canvas_mode="No", highlight_burn=0.0, lens=False, demosaic=False, *,
                     stops=False, rotate_times=0, frame_samples=None, xtrans=False, orientation=0, levels=False, denoise=False):
    """Why process(src, cache=False) renders a frame in one piece before it extracts its payload (stream_rejection and plan_bands
    come after that), or None.  lens: the call corrects the lens (lens_correction with a lens_profile); demosaic: its source is a
    mosaic (raw_profile), for which stops says that the exposure is given in stops, rotate_times is the call's, frame_samples the
    samples of the window of the demosaiced frame that the pipeline takes (mosaic_frame_samples), xtrans that the profile is an
    XTransProfile (which does not stream yet), orientation the profile's (not 0: the one-piece path), and levels that the profile
    is deferred (RawLevels: the one-piece path, the last reason asked for but one); denoise: the call has a raw_denoise (the
    one-piece path, the last reason asked for)."""
    if stream_bands <= 1:
        return f"stream_bands = {stream_bands}"
    if demosaic:
        why = mosaic_rejection(stops, rotate_times, lens, frame_samples, xtrans, orientation)
        if why is not None:
            return why
    if lens:
        return _LENS_REJECTED
    if not isinstance(src, np.ndarray):
        return f"the source is a {type(src).__name__}, not a host array"
    if not demosaic and src.size < STREAM_MIN_SAMPLES:
        return f"a frame of {src.size} samples, below 16.7 M"
    if rotation or chroma_nr or canvas_mode != "No" or highlight_burn:
        return (f"a device pre-path, a canvas or a highlight burn: rotation = {rotation!r}, chroma_nr = {chroma_nr!r}, "
                f"canvas_mode = {canvas_mode!r}, highlight_burn = {highlight_burn!r}")
    if demosaic and levels:
        return _LEVELS_REJECTED
    if demosaic and denoise:
        return _DENOISE_REJECTED
    return None


def mosaic_frame_samples(src, half_size, aspect, flip, zoom, reduction=2, orientation=0):
    """host_stream_gate's frame_samples for a mosaic `src`: rows x cols x 3 of the window that the aspect and zoom crops keep of
    its demosaiced frame (plan_crops without a rotation, which the gate refuses by itself), or None when `src` is no 2-D array.
    reduction: what half_size divides the mosaic's sides by, as its profile states it (2 for a Bayer quad, 3 for X-Trans cells);
    orientation: the profile's -- with bit 4 the crops see the frame with its sides swapped."""
    if not isinstance(src, np.ndarray) or src.ndim != 2:
        return None
    rows, cols = (src.shape[0] // reduction, src.shape[1] // reduction) if half_size else src.shape
    if int(orientation) & 4:
        rows, cols = cols, rows
    if rows < 1 or cols < 1:
        return None
    window = plan_crops(rows, cols, True, aspect, flip, zoom, 0.0, 0, False, False, True).demosaic["window"]
    return max(int(window[2]), 0) * max(int(window[3]), 0) * 3


def check_profiles(raw_profile, lens_profile, lens_correction, cam, lens):
    """The caller's profiles are of their types, and the call needs no lensfun lookup."""
    if raw_profile is not None and not isinstance(raw_profile, (RawProfile, XTransProfile)):
        raise ValueError(f"raw_profile must be a raw2film_amd.raw.RawProfile or XTransProfile, got {type(raw_profile).__name__}")
    if lens_profile is not None and not isinstance(lens_profile, LensProfile):
        raise ValueError(f"lens_profile must be a raw2film_amd.lens.LensProfile, got {type(lens_profile).__name__}")
    if lens_correction and cam is not None and lens is not None:
        # the reference corrects only when both are given (cpu_processor.py:107-108, effects.py:22-30); the lensfun lookup is
        # not part of the accelerated path, and rendering an uncorrected frame in its place would be a silent difference
        raise NotImplementedError("lens correction (lensfunpy, effects.py:22-43) is outside the accelerated path: "
                                  "pass lens_correction=False or no cam / lens (the calibration's numbers go in lens_profile)")


def check_denoise(raw_denoise, raw_profile, rows, cols):
    """The caller's raw_denoise is a WaveletDenoise that this profile and this rows x cols mosaic can run (None passes)."""
    if raw_denoise is None:
        return
    if not isinstance(raw_denoise, WaveletDenoise):
        raise ValueError(f"raw_denoise must be a raw2film_amd.raw.WaveletDenoise, got {type(raw_denoise).__name__}")
    if raw_profile is None:
        raise ValueError("raw_denoise needs a raw_profile: the wavelet denoise runs on a Bayer mosaic, ahead of its demosaic")
    if isinstance(raw_profile, XTransProfile):
        raise ValueError("raw_denoise with an XTransProfile: the wavelet denoise is not built for X-Trans mosaics")
    if raw_denoise.maximum is None and not raw_profile.deferred:
        raise ValueError("raw_denoise has maximum=None and the raw_profile's multipliers are numbers: no scale is resolved whose "
                         "maximum it could take; give WaveletDenoise(threshold, maximum) or a RawLevels as the profile's multipliers")
    if rows % 2 or cols % 2 or rows < 64 or cols < 64:
        raise ValueError(f"raw_denoise on a {rows} x {cols} mosaic: both sides must be even and at least 64 (the five levels reflect "
                         "inside a plane of at least 32 samples a side)")


def check_repair(raw_repair, raw_profile, rows, cols):
    """The caller's raw_repair is a HotPixels that this rows x cols mosaic can run, and comes with a profile (None passes)."""
    if raw_repair is None:
        return
    if not isinstance(raw_repair, HotPixels):
        raise ValueError(f"raw_repair must be a raw2film_amd.raw.HotPixels, got {type(raw_repair).__name__}")
    if raw_profile is None:
        raise ValueError("raw_repair needs a raw_profile: the repair runs on a mosaic, ahead of its demosaic")
    if rows < 6 or cols < 6:
        raise ValueError(f"raw_repair on a {rows} x {cols} mosaic: both sides must be at least 6")


def load_decoded(src, clip=True, mosaic=False):
    """The decoded frame behind `src` (an array, or the path of a .npy file): float32 (H, W, 3|4), clamped like
    gpu_processor.py:275 unless clip=False; LibRaw's uint16 output as it is; with mosaic=True the uint16 (H, W) Bayer mosaic."""
    if isinstance(src, np.ndarray):
        image = src
    elif isinstance(src, str) and src.lower().endswith(".npy"):
        image = np.load(src)
    elif isinstance(src, str):
        raise NotImplementedError(
            f"{src!r}: RAW decoding (LibRaw/rawpy, raw_conversion.py:33-53) is outside the accelerated path; "
            "pass the decoded linear-XYZ frame (array or .npy)"
        )
    else:
        raise TypeError(f"unsupported src type {type(src)!r}")
    if mosaic:
        if image.ndim != 2 or image.dtype != np.uint16:
            raise ValueError(f"with a raw_profile the source is a Bayer mosaic, uint16 (H, W); got {image.dtype} {image.shape}")
        return image
    if image.ndim != 3 or image.shape[2] not in (3, 4):
        raise ValueError(f"decoded frame must be (H, W, 3|4), got {image.shape}" +
                         (" (a Bayer mosaic needs its raw_profile)" if image.ndim == 2 else ""))
    if image.dtype == np.uint16:  # LibRaw's 16-bit output: converted on the device (decode.py, r2f_decode_u16)
        return image
    image = np.asarray(image, dtype=np.float32)
    return np.clip(image, 0, 65504) if clip else image  # gpu_processor.py:275 (clip=False: clamped after the upload)


def exposure_mode(exposure, on_device, is_u16, mosaic, rotation, rotate_times):
    """Where the auto exposure of a uint16 frame is measured -> (on the device?, `exposure`, `exposure_rejected`).  The device
    measures the whole frame as it was uploaded, so a turned or rotated frame is measured on the host as with exposure=None, and
    `exposure_rejected` says why.  A mosaic (raw_profile) has no RGB frame on the host: without stops it is measured on the device
    like exposure="device", and where that is refused the call needs explicit stops."""
    if mosaic and (exposure is None or on_device):
        if rotation or int(rotate_times) % 4:
            raise ValueError(f"rotation = {rotation!r}, rotate_times = {rotate_times!r}: a turned or rotated frame is measured on "
                             "the host, and a mosaic (raw_profile) has no RGB frame there: pass the exposure in stops")
        on_device = True
    if is_u16 and on_device and (rotation or int(rotate_times) % 4):
        return False, None, (f"rotation = {rotation!r}, rotate_times = {rotate_times!r}: a turned or rotated frame is measured on "
                             "the host")
    return on_device, exposure, None


class CropPlan(NamedTuple):
    """plan_crops' answer.  A step's share is {"window": (row0, col0, rows, cols) or None, "rotate_times": k}: the payload's
    fields of that step, next to its `params`; None without the step."""
    size: tuple  # (h, w) of the frame the crops, the rotation and the quarter turns leave
    u16_window: tuple | None  # what the device decode of an exposure="device" frame keeps of the uploaded frame
    warp: dict | None  # the payload's `warp`
    lens: dict | None
    demosaic: dict | None
    host: dict | None  # the host's share: cut_and_turn's arguments


def plan_crops(rows, cols, is_u16, aspect, flip, zoom, rotation, rotate_times, on_device, lens, demosaic) -> CropPlan:
    """The crops of a rows x cols frame (raw_conversion.crop_rotate_zoom's index arithmetic, raw_conversion.py:56-72, with the
    interpolating part of a free rotation deferred to the device) and who applies them: see the module's text.  is_u16, on_device:
    the frame is uint16 / measured on the device (exposure_mode's answer: then neither turned nor rotated); lens, demosaic: the
    step exists."""
    k = int(rotate_times) % 4
    device_decode = is_u16 and on_device
    r0, c0, nr, nc = aspect_box = geometry.crop_box(rows, cols, 1, aspect, flip)
    if rotation:  # the zoom box lies in the window effects.rotate's centred crop keeps of the rotated aspect crop
        m_inv, (r0, c0, nr, nc) = geometry.rotation_plan(nr, nc, rotation)
    zr0, zc0, znr, znc = geometry.crop_box(nr, nc, zoom, aspect, False)
    window = (r0 + zr0, c0 + zc0, znr, znc)
    if rotation:
        if znr <= 0 or znc <= 0:
            raise ValueError(f"rotation {rotation} / zoom {zoom} leave an empty frame")
        warp = {"m_dst_to_src": m_inv, "window": window, "rotate_times": k}
        share = {"window": aspect_box, "rotate_times": 0}  # ahead of the warp: the aspect crop alone
    else:
        warp, share = None, {"window": window, "rotate_times": k}
    idle = {"window": None, "rotate_times": 0}
    u16_window = None
    if device_decode:  # (with a lens step the frame is decoded whole: the step reads all of it)
        u16_window = (0, 0, rows, cols) if lens else window
    return CropPlan(
        size=(znc, znr) if k % 2 else (znr, znc), u16_window=u16_window, warp=warp,
        lens=share if lens else None,
        demosaic=None if not demosaic else idle if lens or device_decode else share,
        host=None if lens or device_decode or demosaic else share)


def cut_and_turn(image, window, rotate_times):
    """The host's share of a CropPlan: a view of the frame, turned with np.rot90 (raw_conversion.py:66-70)."""
    r0, c0, nr, nc = window
    view = image[r0:r0 + nr, c0:c0 + nc]
    return np.rot90(view, k=rotate_times) if rotate_times else view


Resolutions = namedtuple("Resolutions", "final_resolution resize_to upscale_to output_resolution canvas_resolution pipeline_resolution")


def plan_resolution(h, w, frame_width, frame_height, resolution, max_scale, canvas_mode, canvas_scale, canvas_ratio) -> Resolutions:
    """The payload's fields of these names for a cropped h x w frame.  cpu_processor.py:119-134: without a preview resolution the
    frame's own size is the target; a target finer than `max_scale` px/mm is rendered at max_scale and scaled back up at the very
    end (cpu_processor.py:411-412)."""
    if resolution is None and max_scale is not None:
        resolution = (h, w)
    resize_to, upscale_to = None, None
    # what CpuProcessor.load_image returns as `orig_resolution` (cpu_processor.py:122) and process() hands to the final
    # resolution_scaling (cpu_processor.py:411-412)
    final_resolution = (int(resolution[0]), int(resolution[1])) if resolution is not None else None
    scale_factor = 1.0
    if resolution is not None:
        resolution = (int(resolution[0]), int(resolution[1]))
        scale = max(resolution) / max(frame_width, frame_height)
        if max_scale is not None and scale > max_scale:
            scale_factor = max_scale / scale
            upscale_to = resolution
            resolution = tuple(round(x * scale_factor) for x in resolution)
        # utils.resolution_scaling (utils.py:226-244), applied on the device in phase 2
        factor = min(resolution[0] / h, resolution[1] / w)
        if factor != 1:
            # cv.resize(dsize=(round(w f), round(h f))): INTER_AREA down, INTER_LANCZOS4 up (a preview larger than the frame)
            resize_to = (round(h * factor), round(w * factor))
            h, w = resize_to
    # gpu_processor.py:764: the size the frame has once it is back from the max_scale pipeline -- the UN-shrunk output size,
    # which is also what the canvas is laid out for (:767-771), not the pipeline's
    out_h, out_w = (round(x / scale_factor) for x in (h, w))
    if upscale_to is not None and min(upscale_to[0] / h, upscale_to[1] / w) <= 1:
        upscale_to = None  # (the uint8 result goes back up with LANCZOS4 only when that enlarges it)
    canvas_res = None
    if canvas_mode != "No":  # gpu_processor.py:767-771
        res, _, _ = geometry.canvas_layout((out_h, out_w), canvas_mode, canvas_scale, canvas_ratio)
        canvas_res = (res[1], res[0])
    return Resolutions(final_resolution, resize_to, upscale_to, (out_w, out_h), canvas_res, (w, h))


def pack_image(image, whole, is_u16, alpha):
    """The payload's `image_array`.  whole: a mosaic, or the uint16 frame the device measures -- the array itself when it is
    contiguous (a fourth channel is dropped on the device).  Another uint16 frame: its three channels.  A float frame: float32,
    with the constant alpha plane of gpu_processor.py:765 when `alpha`, else without a fourth channel."""
    if whole:
        return np.ascontiguousarray(image)
    if is_u16:
        return np.ascontiguousarray(image[..., :3])
    if image.shape[2] == 3 and alpha:
        image = np.concatenate([image, np.ones_like(image[..., :1])], axis=-1)  # gpu_processor.py:765
    elif image.shape[2] == 4 and not alpha:
        image = image[..., :3]
    return np.ascontiguousarray(image, dtype=np.float32)
