"""HipContext: a thin object over the C ABI (include/r2f.h), torch tensors as device buffers.

One context per GPU, entered by one thread at a time (the reference's processors have the
same rule, gui.py:2119-2129).  All launches go to torch's current stream on that device.
torch is used for memory and streams only; every computation is a HIP kernel of libr2f_hip.so.
"""

from __future__ import annotations

import ctypes as C
import numbers

import numpy as np

from . import _lib

LOG_EPS = 1e-6  # lut_1d.wgsl:24
LUT3D_SCALE = 0.25  # cpu_processor.py:405


class R2FError(RuntimeError):
    pass


def _host_f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


class HipContext:
    def __init__(self, device: int = 0, lib_path: str | None = None):
        import torch

        self._torch = torch
        # raises ImportError if the HIP library is missing -- no fallback.  lib_path: a development variant of the library bound
        # beside the in-tree one (A/B of two builds in one process)
        self._lib = _lib.load(lib_path)
        if not torch.cuda.is_available():
            raise R2FError("raw2film_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU path")
        self.device = torch.device("cuda", device)
        handle = C.c_void_p()
        rc = self._lib.r2f_create(int(device), C.byref(handle))
        if rc != 0 or not handle.value:
            raise R2FError(f"r2f_create(device={device}) failed with code {rc}")
        self._h = handle
        self._workspace = None
        self._denoise_workspace = None  # mosaic_denoise's, apart from the render's: growing it moves no buffer a captured frame holds
        self._repair_mosaic = None  # mosaic_repair's second mosaic, kept for the next mosaic of its size

    # ------------------------------------------------------------------ plumbing
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.r2f_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            msg = self._lib.r2f_last_error(self._h).decode(errors="replace")
            if rc == _lib.EINVAL:
                raise ValueError(msg)
            raise R2FError(f"r2f error {rc}: {msg}")

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def make_params(self, *, matrix=False, halation=False, mtf=False, grain=False, grain_mono=False, seed=0,
                    lut3d_mode=0, log_eps=LOG_EPS, lut3d_scale=LUT3D_SCALE, burn_strength=0.0, burn_cell=0,
                    burn_d_ref=0.0) -> _lib.Params:
        """burn_strength != 0 switches S7 on; burn_cell = ceil(min(H, W) / burn_scale) (effects.py:365)."""
        flags = (
            (_lib.F_MATRIX if matrix else 0)
            | (_lib.F_HALATION if halation else 0)
            | (_lib.F_MTF if mtf else 0)
            | (_lib.F_GRAIN if grain else 0)
            | (_lib.F_GRAIN_MONO if grain_mono else 0)
            | (_lib.F_BURN if burn_strength else 0)
        )
        return _lib.Params(flags, int(seed) & 0xFFFFFFFF, float(log_eps), float(lut3d_scale), int(lut3d_mode),
                           int(burn_cell), float(burn_strength), float(burn_d_ref))

    def planes(self, t, gy0: int = 0) -> _lib.Planes:
        """Describe a float32 (3, rows, W) device tensor holding global rows gy0..: contiguous, or a ROW SLICE of such a tensor
        (t[:, a:b, :]: rows contiguous, planes a fixed stride apart -- r2f_planes carries the plane stride)."""
        torch = self._torch
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3 or t.shape[0] != 3 or not t.is_cuda:
            raise ValueError("planes: need a float32 CUDA tensor of shape (3, rows, W)")
        rows, W = int(t.shape[1]), int(t.shape[2])
        if t.is_contiguous():
            stride = rows * W
        elif rows > 0 and t.stride(2) == 1 and t.stride(1) == W and t.stride(0) >= rows * W:
            stride = int(t.stride(0))
        else:
            raise ValueError("planes: need a contiguous (3, rows, W) tensor or a row slice t[:, a:b, :] of one")
        self._same_device(t, "planes")
        return _lib.Planes(t.data_ptr(), stride, int(gy0), rows)

    def _check_out(self, t, dtype, W, what, *, rows=None, gy0=0, y0=None, y1=None):
        """A caller's output tensor before its pointer crosses the C ABI (which cannot check it): (rows, W, 3) of `dtype`,
        contiguous, on this context's device, holding the global rows [gy0, gy0 + rows) and covering [y0, y1)."""
        if t is None:
            return
        torch = self._torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.dim() == 3 and t.shape[2] == 3
                and int(t.shape[1]) == int(W) and t.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous {dtype} CUDA tensor of shape (rows, {int(W)}, 3)")
        self._same_device(t, what)
        if rows is not None and int(t.shape[0]) != int(rows):
            raise ValueError(f"{what} has {int(t.shape[0])} rows, the frame {int(rows)}")
        if y0 is not None and (y0 < gy0 or y1 > gy0 + int(t.shape[0])):
            raise ValueError(f"{what} holds rows [{gy0}, {gy0 + int(t.shape[0])}), asked to write [{y0}, {y1})")

    def generation(self) -> int:
        """Change counter of the context's tables, options and internal buffers (r2f_generation): a captured HIP graph of this
        context's launches is stale once it moves."""
        return int(self._lib.r2f_generation(self._h))

    def render_stats(self) -> dict:
        """Counters of `render` (r2f_render_stats): frames replayed from a captured HIP graph, graphs captured, frames launched
        kernel by kernel, graphs dropped."""
        out = (C.c_uint64 * 4)()
        self._check(self._lib.r2f_render_stats(self._h, out))
        return {"replays": int(out[0]), "captures": int(out[1]), "eager": int(out[2]), "dropped": int(out[3])}

    def frame_exposure_range(self) -> dict:
        """r2f_frame_exposure_range: min / max |.| of the exposure planes the last whole-frame render's halation read, the rule
        (bound, floor) and whether its FFT passes took the 12-byte scratch element (synchronises the device)."""
        out, armed, packed = (C.c_float * 4)(), C.c_int(), C.c_int()
        self._check(self._lib.r2f_frame_exposure_range(self._h, out, C.byref(armed), C.byref(packed)))
        pairs, packed_pairs = C.c_int(), C.c_int()
        self._check(self._lib.r2f_frame_scratch_choice(self._h, C.byref(pairs), C.byref(packed_pairs)))
        # the choice is made per window pair: `twelve_byte_element` = every pair of the last halation call took it; the counts beside it
        return {"min": float(out[0]), "max_abs": float(out[1]), "bound": float(out[2]), "floor": float(out[3]),
                "armed": bool(armed.value), "twelve_byte_element": bool(packed.value),
                "pairs": int(pairs.value), "packed_pairs": int(packed_pairs.value)}

    def frame_scratch_flags(self):
        """r2f_frame_scratch_flags: one flag per window pair (per channel) of the last halation call that chose its scratch element on
        the device -- 1 = the 12-byte element -- as a numpy int32 array (empty when it did not choose).  Synchronises the device."""
        import numpy as np

        n = C.c_int()
        self._check(self._lib.r2f_frame_scratch_flags(self._h, None, 0, C.byref(n)))
        flags = np.zeros(max(int(n.value), 0), dtype=np.int32)
        if flags.size:
            self._check(self._lib.r2f_frame_scratch_flags(self._h, flags.ctypes.data_as(C.POINTER(C.c_int32)), int(flags.size), C.byref(n)))
        return flags

    def write_frame_params(self, params):
        """The per-render uniform write (r2f_write_frame_params): params.seed -> the context's device-side frame block, in
        stream order.  Stage calls whose params carry F_FRAME_RESIDENT read it instead of writing their own seed."""
        self._check(self._lib.r2f_write_frame_params(self._h, C.byref(params), self._stream()))

    def set_option(self, name: str, value: int):
        self._check(self._lib.r2f_set_option(self._h, name.encode(), int(value)))

    # ------------------------------------------------------------------ uploads
    def set_matrix3x3(self, m):
        if m is None:
            self._check(self._lib.r2f_set_matrix3x3(self._h, None))
            return
        m = _host_f32(m)
        if m.shape != (3, 3):
            raise ValueError("matrix must be 3x3")
        self._check(self._lib.r2f_set_matrix3x3(self._h, m.ctypes.data))

    def set_lut2d(self, lut):
        lut = _host_f32(lut)
        if lut.ndim != 3 or lut.shape[0] != lut.shape[1] or lut.shape[2] != 3:
            raise ValueError(f"input LUT must be (n, n, 3), got {lut.shape}")
        self._check(self._lib.r2f_set_lut2d(self._h, lut.ctypes.data, lut.shape[0]))

    def set_curve1d(self, lut):
        lut = _host_f32(lut)
        if lut.ndim != 2 or lut.shape[0] != 4:
            raise ValueError(f"density curve must be (4, m), got {lut.shape}")
        self._check(self._lib.r2f_set_curve1d(self._h, lut.ctypes.data, lut.shape[1]))

    def set_lut3d(self, lut):
        lut = _host_f32(lut)
        if lut.ndim != 4 or lut.shape[3] != 3 or not (lut.shape[0] == lut.shape[1] == lut.shape[2]):
            raise ValueError(f"output LUT must be (n, n, n, 3), got {lut.shape}")
        self._check(self._lib.r2f_set_lut3d(self._h, lut.ctypes.data, lut.shape[0]))

    def set_grain_lut(self, lut):
        lut = _host_f32(lut)
        if lut.ndim != 2 or lut.shape[0] != 4:
            raise ValueError(f"grain LUT must be (4, m), got {lut.shape}")
        self._check(self._lib.r2f_set_grain_lut(self._h, lut.ctypes.data, lut.shape[1]))

    def set_kernel(self, which: int, k):
        k = _host_f32(k)
        if k.ndim == 2:
            k = k[..., None]
        if k.ndim != 3 or k.shape[2] not in (1, 3):
            raise ValueError(f"stencil must be (kh, kw) or (kh, kw, 1|3), got {k.shape}")
        k = np.ascontiguousarray(k)
        self._check(self._lib.r2f_set_kernel(self._h, int(which), k.ctypes.data, k.shape[0], k.shape[1], k.shape[2]))

    # ------------------------------------------------------------------ whole frame
    @staticmethod
    def layout_of(t, layout=None) -> tuple[int, int, int]:
        """(layout, H, W) of an image tensor: (H, W, 3) / (H, W, 4) interleaved or (3, H, W) planar.

        A (3, H, 3) or (3, H, 4) tensor is ambiguous; interleaved wins (the reference only knows (H, W, C) frames),
        so pass ``layout="chw"`` for a planar frame that is 3 or 4 pixels wide."""
        if t.dim() != 3:
            raise ValueError("image must be 3-D")
        if layout is not None:
            want = {"hwc3": (_lib.LAYOUT_HWC3, 2, 3), "hwc4": (_lib.LAYOUT_HWC4, 2, 4), "chw": (_lib.LAYOUT_CHW, 0, 3)}.get(layout)
            if want is None or t.shape[want[1]] != want[2]:
                raise ValueError(f"layout {layout!r} does not fit image shape {tuple(t.shape)}")
            hw = (t.shape[1], t.shape[2]) if layout == "chw" else (t.shape[0], t.shape[1])
            return want[0], int(hw[0]), int(hw[1])
        if t.shape[2] == 3:
            return _lib.LAYOUT_HWC3, int(t.shape[0]), int(t.shape[1])
        if t.shape[2] == 4:
            return _lib.LAYOUT_HWC4, int(t.shape[0]), int(t.shape[1])
        if t.shape[0] == 3:
            return _lib.LAYOUT_CHW, int(t.shape[1]), int(t.shape[2])
        raise ValueError(f"cannot interpret image shape {tuple(t.shape)}")

    def _same_device(self, t, what):
        if t.device.index is not None and self.device.index is not None and t.device.index != self.device.index:
            raise ValueError(f"{what} lives on {t.device}, this context on {self.device}")

    def _check_image(self, t):
        torch = self._torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("image must be a contiguous float32 CUDA tensor")
        self._same_device(t, "image")

    def workspace_bytes(self, params, H, W) -> int:
        return int(self._lib.r2f_workspace_bytes(C.byref(params), H, W))

    def _get_workspace(self, nbytes: int):
        torch = self._torch
        if nbytes == 0:
            return None
        if self._workspace is None or self._workspace.numel() < nbytes:
            self._workspace = None
            self._workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._workspace

    def _check_outs(self, W, out_f32=None, out_u8=None, out_u16=None, **kw):
        """The output tensors of a call, each checked like _check_out, -> their pointers (None for one that is not asked for)."""
        self._check_out(out_f32, self._torch.float32, W, "out_f32", **kw)
        self._check_out(out_u8, self._torch.uint8, W, "out_u8", **kw)
        self._check_out16(out_u16, W, "out_u16", **kw)
        return [t.data_ptr() if t is not None else None for t in (out_f32, out_u8, out_u16)]

    def _check_out16(self, t, W, what, **kw):
        """A 16-bit output tensor: uint16, or int16 holding the same bits (torch's uint16 knows few operations)."""
        if t is not None and t.dtype not in (self._torch.int16, self._torch.uint16):
            raise ValueError(f"{what} must be a contiguous 16-bit CUDA tensor of shape (rows, {int(W)}, 3)")
        self._check_out(t, None if t is None else t.dtype, W, what, **kw)

    def _render(self, wide, image, params, out_f32, out, want_f32, want_out, layout):
        """render / render16: r2f_render with the uint8 result, or (`wide`) r2f_render16 with the 16-bit one."""
        torch = self._torch
        self._check_image(image)
        layout, H, W = self.layout_of(image, layout)
        if out_f32 is None and want_f32:
            out_f32 = torch.empty((H, W, 3), dtype=torch.float32, device=self.device)
        if out is None and want_out:
            out = torch.empty((H, W, 3), dtype=torch.int16 if wide else torch.uint8, device=self.device)
        if wide:
            fn, (p32, _, p_out) = self._lib.r2f_render16, self._check_outs(W, out_f32, out_u16=out, rows=H)
        else:
            fn, (p32, p_out, _) = self._lib.r2f_render, self._check_outs(W, out_f32, out_u8=out, rows=H)
        nbytes = self.workspace_bytes(params, H, W)
        ws = self._get_workspace(nbytes)
        self._check(fn(self._h, C.byref(params), image.data_ptr(), layout, p32, p_out, H, W,
                       ws.data_ptr() if ws is not None else None, nbytes, self._stream()))
        return out_f32, out

    def render(self, image, params, out_f32=None, out_u8=None, want_f32=True, want_u8=False, layout=None):
        """Full pipeline on one frame: S0..S8 (+S9).  Returns (out_f32, out_u8) device tensors (H, W, 3)."""
        return self._render(False, image, params, out_f32, out_u8, want_f32, want_u8, layout)

    # ------------------------------------------------------------------ 16-bit output (r2f_render16 and the stage calls beside it)
    def render16(self, image, params, out_f32=None, out_u16=None, want_f32=False, layout=None):
        """render() with the 16-bit result of r2f_render16: clip(x * 65535, 0, 65535) truncated, from the float out_f32 holds.
        Returns (out_f32 or None, out_u16): device tensors (H, W, 3); out_u16 is int16 holding the uint16 bits unless one is given."""
        return self._render(True, image, params, out_f32, out_u16, want_f32, True, layout)

    def stage_front16(self, image, params, *, in_gy0=0, out_f32=None, out_u16=None, out_gy0=0, y0=None, y1=None, H_global=None,
                      layout=None):
        """stage_front(upto = output) with the 16-bit output (r2f_stage_front16)."""
        self._stage_front(image, params, None, in_gy0, None, 0, (out_f32, None, out_u16), out_gy0, y0, y1, H_global, layout)

    def stage_tail16(self, density, params, *, src_gy0=0, out_f32=None, out_u8=None, out_u16=None, out_gy0=0, y0, y1, H_global,
                     burn_map=None, field=None, field_gy0=0):
        """stage_tail (or, with `field`, stage_tail_field) with the 16-bit output beside the other two (r2f_stage_tail16,
        r2f_stage_tail_field16)."""
        self._stage_tail(True, density, params, src_gy0, (out_f32, out_u8, out_u16), out_gy0, y0, y1, H_global, burn_map, field,
                         field_gy0)

    def _resize_hwc3(self, fn, what, wide, image, out_h, out_w):
        """The four resamplers of a finished (H, W, 3) frame: uint8, or (`wide`) 16-bit -> a new frame of the same dtype."""
        torch = self._torch
        dtypes = (torch.int16, torch.uint16) if wide else (torch.uint8,)
        if not (isinstance(image, torch.Tensor) and image.is_cuda and image.dtype in dtypes and image.is_contiguous()
                and image.dim() == 3 and image.shape[2] == 3):
            raise ValueError(f"{what} needs a contiguous {'16-bit' if wide else 'uint8'} (H, W, 3) CUDA tensor")
        self._same_device(image, "image")
        out = torch.empty((int(out_h), int(out_w), 3), dtype=image.dtype, device=self.device)
        self._check(fn(self._h, image.data_ptr(), int(image.shape[0]), int(image.shape[1]), out.data_ptr(), int(out_h), int(out_w),
                       self._stream()))
        return out

    def resize_lanczos4_u16(self, image_u16, out_h: int, out_w: int):
        """cv.resize(uint16 (H, W, 3), (out_w, out_h), interpolation=cv.INTER_LANCZOS4) on the device (int16 tensors: same bits)."""
        return self._resize_hwc3(self._lib.r2f_resize_lanczos4_u16, "resize_lanczos4_u16", True, image_u16, out_h, out_w)

    def resize_area_u16(self, image_u16, out_h: int, out_w: int):
        """cv.resize(uint16 (H, W, 3), (out_w, out_h), interpolation=cv.INTER_AREA), shrinking, on the device."""
        return self._resize_hwc3(self._lib.r2f_resize_area_u16, "resize_area_u16", True, image_u16, out_h, out_w)

    def resize_lanczos4_u8(self, image_u8, out_h: int, out_w: int):
        """cv.resize(uint8 (H, W, 3), (out_w, out_h), interpolation=cv.INTER_LANCZOS4) on the device."""
        return self._resize_hwc3(self._lib.r2f_resize_lanczos4_u8, "resize_lanczos4_u8", False, image_u8, out_h, out_w)

    def resize_area_u8(self, image_u8, out_h: int, out_w: int):
        """cv.resize(uint8 (H, W, 3), (out_w, out_h), interpolation=cv.INTER_AREA), shrinking, on the device (utils.py:226-236 as
        the CPU processor applies it to the finished frame, cpu_processor.py:411-412)."""
        return self._resize_hwc3(self._lib.r2f_resize_area_u8, "resize_area_u8", False, image_u8, out_h, out_w)

    # ------------------------------------------------------------------ stages (row-shard aware)
    def _stage_front(self, image, params, upto, in_gy0, dst, dst_gy0, outs, out_gy0, y0, y1, H_global, layout, track_range=False):
        """stage_front (r2f_stage_front: up to stage `upto`, into the planes `dst` or the outputs) and, with upto=None, stage_front16
        (r2f_stage_front16: the output stage with the 16-bit result); `outs`: (out_f32, out_u8, out_u16)."""
        self._check_image(image)
        if track_range:
            params = _lib.Params.from_buffer_copy(params)
            params.flags |= _lib.F_TRACK_RANGE
        layout, rows, W = self.layout_of(image, layout)
        y0 = in_gy0 if y0 is None else y0
        y1 = in_gy0 + rows if y1 is None else y1
        H_global = in_gy0 + rows if H_global is None else H_global
        pl = self.planes(dst, dst_gy0) if dst is not None else None
        p32, p8, p16 = self._check_outs(W, *outs, gy0=out_gy0, y0=y0, y1=y1)
        head = (self._h, C.byref(params), image.data_ptr(), layout, in_gy0, rows)
        rows_of = (out_gy0, y0, y1, W, H_global, self._stream())
        if upto is None:
            self._check(self._lib.r2f_stage_front16(*head, p32, p16, *rows_of))
        else:
            self._check(self._lib.r2f_stage_front(*head, int(upto), C.byref(pl) if pl is not None else None, p32, p8, *rows_of))

    def stage_front(self, image, params, upto, *, in_gy0=0, dst=None, dst_gy0=0, out_f32=None, out_u8=None,
                    out_gy0=0, y0=None, y1=None, H_global=None, layout=None, track_range=False):
        """track_range (upto = exposure): the kernel merges the range of the exposure samples it writes for the halation's FFT
        channels into the context's exposure-range record, a grid of 64 x 256-pixel tiles (R2F_F_TRACK_RANGE), like r2f_render's
        front kernel does for a whole frame."""
        self._stage_front(image, params, upto, in_gy0, dst, dst_gy0, (out_f32, out_u8, None), out_gy0, y0, y1, H_global, layout,
                          track_range)

    def stage_front_split(self, image, params, exposure, density, *, in_gy0=0, exposure_gy0=0, density_gy0=0, y0=None, y1=None,
                          H_global=None, layout=None, track_range=False) -> int:
        """S0 + S1 for a frame that goes on to stage_halation: channels with a real halation stencil -> `exposure`; channels
        whose halation stencil is one tap at the anchor are finished (tap weight, log, curve) straight into `density`.  Returns
        the mask of channels finished that way: pass it to stage_halation(identity_done=mask).  track_range: see stage_front."""
        self._check_image(image)
        if track_range:
            params = _lib.Params.from_buffer_copy(params)
            params.flags |= _lib.F_TRACK_RANGE
        layout, rows, W = self.layout_of(image, layout)
        y0 = in_gy0 if y0 is None else y0
        y1 = in_gy0 + rows if y1 is None else y1
        H_global = in_gy0 + rows if H_global is None else H_global
        pe, pd = self.planes(exposure, exposure_gy0), self.planes(density, density_gy0)
        mask = C.c_int(0)
        self._check(self._lib.r2f_stage_front_split(self._h, C.byref(params), image.data_ptr(), layout, in_gy0, rows, C.byref(pe),
                                                    C.byref(pd), y0, y1, W, H_global, C.byref(mask), self._stream()))
        return mask.value

    def _stencil_call(self, fn, first, src, src_gy0, dst, dst_gy0, y0, y1, H_global):
        ps, pd = self.planes(src, src_gy0), self.planes(dst, dst_gy0)
        W = int(src.shape[2])
        if int(dst.shape[2]) != W:
            raise ValueError("source and destination widths differ")
        self._check(fn(self._h, first, C.byref(ps), C.byref(pd), y0, y1, W, H_global, self._stream()))

    def stage_exposure_range(self, exposure, *, src_gy0=0, y0, y1, y2=0, y3=0):
        """Merge min / max |.| of rows [y0, y1) and [y2, y3) of the exposure planes (the halation's FFT channels) into the exposure-range record's tiles:
        the halo rows a row shard received from above and below, one launch (r2f_stage_exposure_range)."""
        if y1 <= y0 and y3 <= y2:
            return
        pe = self.planes(exposure, src_gy0)
        self._check(self._lib.r2f_stage_exposure_range(self._h, C.byref(pe), int(y0), int(y1), int(y2), int(y3), int(exposure.shape[2]),
                                                       self._stream()))

    def stage_halation(self, exposure, density, params, *, src_gy0=0, dst_gy0=0, y0, y1, H_global, identity_done=0, range_valid=False):
        """range_valid: the caller has kept the exposure-range record for the rows `exposure` holds this frame (R2F_F_RANGE_VALID): the
        FFT passes then choose their scratch element on the device, window pair by window pair, like r2f_render's."""
        if identity_done or range_valid:
            params = _lib.Params.from_buffer_copy(params)
        if identity_done:  # stage_front_split already wrote the identity channels' density for these rows
            params.flags |= _lib.F_IDENTITY_DONE
        if range_valid:
            params.flags |= _lib.F_RANGE_VALID
        self._stencil_call(self._lib.r2f_stage_halation, C.byref(params), exposure, src_gy0, density, dst_gy0, y0, y1, H_global)

    def stage_mtf(self, density_in, density_out, params, *, src_gy0=0, dst_gy0=0, y0, y1, H_global):
        self._stencil_call(self._lib.r2f_stage_mtf, C.byref(params), density_in, src_gy0, density_out, dst_gy0, y0, y1, H_global)

    def stage_stencil(self, which, src, dst, *, src_gy0=0, dst_gy0=0, y0, y1, H_global):
        self._stencil_call(self._lib.r2f_stage_stencil, int(which), src, src_gy0, dst, dst_gy0, y0, y1, H_global)

    def _stage_tail(self, wide, density, params, src_gy0, outs, out_gy0, y0, y1, H_global, burn_map=None, field=None, field_gy0=0):
        """The four tail entry points: r2f_stage_tail, or with a grain `field` r2f_stage_tail_field, each with (`wide`) its ...16
        twin that takes the 16-bit output beside the other two; `outs`: (out_f32, out_u8, out_u16)."""
        pd = self.planes(density, src_gy0)
        W = int(density.shape[2])
        ptrs = self._check_outs(W, *outs, gy0=out_gy0, y0=y0, y1=y1)
        if not wide:
            ptrs = ptrs[:2]  # (r2f_stage_tail and r2f_stage_tail_field take out_f32 and out_u8 only)
        if field is not None:
            pf = self.planes(field, field_gy0)
            fn = self._lib.r2f_stage_tail_field16 if wide else self._lib.r2f_stage_tail_field
            second = C.byref(pf)
        else:
            if burn_map is not None:
                self._check_lowres(burn_map, params, H_global, W, "burn_map")
            fn = self._lib.r2f_stage_tail16 if wide else self._lib.r2f_stage_tail
            second = burn_map.data_ptr() if burn_map is not None else None
        self._check(fn(self._h, C.byref(params), C.byref(pd), second, *ptrs, out_gy0, y0, y1, W, H_global, self._stream()))

    def stage_tail(self, density, params, *, src_gy0=0, out_f32=None, out_u8=None, out_gy0=0, y0, y1, H_global,
                   burn_map=None):
        self._stage_tail(False, density, params, src_gy0, (out_f32, out_u8, None), out_gy0, y0, y1, H_global, burn_map)

    def stage_grain_field(self, field, params, *, dst_gy0=0, y0, y1, H_global):
        """The grain field K_g * N for rows [y0, y1) -> (3, rows, W) planes; no image involved."""
        pf = self.planes(field, dst_gy0)
        self._check(self._lib.r2f_stage_grain_field(self._h, C.byref(params), C.byref(pf), y0, y1, int(field.shape[2]), H_global,
                                                    self._stream()))

    def stage_tail_field(self, density, field, params, *, src_gy0=0, field_gy0=0, out_f32=None, out_u8=None, out_gy0=0, y0, y1,
                         H_global):
        """stage_tail with a grain field made by stage_grain_field instead of generating it in the same kernel."""
        self._stage_tail(False, density, params, src_gy0, (out_f32, out_u8, None), out_gy0, y0, y1, H_global, None, field, field_gy0)

    def stage_grain(self, density_in, density_out, params, *, src_gy0=0, dst_gy0=0, y0, y1, H_global):
        """S6 + clip alone (planes -> planes): first half of the tail when S7 is on."""
        self._stencil_call(self._lib.r2f_stage_grain, C.byref(params), density_in, src_gy0, density_out, dst_gy0, y0, y1, H_global)

    def burn_shape(self, params, H_global, W):
        return H_global // params.burn_cell, W // params.burn_cell

    def _check_lowres(self, t, params, H_global, W, what):
        torch = self._torch
        shape = self.burn_shape(params, H_global, W)
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"{what} must be a contiguous float32 CUDA tensor of shape {shape} (the highlight burn's low-resolution grid)")
        self._same_device(t, what)

    def stage_burn_sums(self, density, params, *, src_gy0=0, y0, y1, H_global):
        """S7 part 1: area-weighted partial sums of the green density over rows [y0, y1) -> (h_lo, w_lo) tensor."""
        torch = self._torch
        W = int(density.shape[2])
        h_lo, w_lo = self.burn_shape(params, H_global, W)
        sums = torch.empty((h_lo, w_lo), dtype=torch.float32, device=self.device)
        pd = self.planes(density, src_gy0)
        self._check(self._lib.r2f_stage_burn_sums(self._h, C.byref(params), C.byref(pd), sums.data_ptr(), y0, y1, W, H_global,
                                                  self._stream()))
        return sums

    def stage_burn_map(self, sums, params, *, W, H_global):
        """S7 part 2: clip(x - d_ref, 0) + Gaussian(sigma 3) on the low-res map."""
        torch = self._torch
        self._check_lowres(sums, params, H_global, W, "sums")
        out = torch.empty_like(sums)
        scratch = torch.empty((2,) + tuple(sums.shape), dtype=torch.float32, device=self.device)
        self._check(self._lib.r2f_stage_burn_map(self._h, C.byref(params), sums.data_ptr(), out.data_ptr(), scratch.data_ptr(), W,
                                                 H_global, self._stream()))
        return out

    def stage_chroma_nr_h(self, image, dst, size, *, in_gy0=0, dst_gy0=0, y0=None, y1=None, layout=None):
        """Pre-path chroma NR pass 1: image rows -> planes (x blurred horizontally, y blurred horizontally, Y)."""
        self._check_image(image)
        layout, rows, W = self.layout_of(image, layout)
        y0 = in_gy0 if y0 is None else y0
        y1 = in_gy0 + rows if y1 is None else y1
        pd = self.planes(dst, dst_gy0)
        self._check(self._lib.r2f_stage_chroma_nr_h(self._h, image.data_ptr(), layout, in_gy0, rows, C.byref(pd), int(size), y0, y1,
                                                    W, self._stream()))

    def stage_chroma_nr_v(self, src, dst, size, *, src_gy0=0, dst_gy0=0, y0, y1, H_global):
        """Pre-path chroma NR pass 2: vertical blur + xyY -> XYZ planes (CHW input for the front stage)."""
        ps, pd = self.planes(src, src_gy0), self.planes(dst, dst_gy0)
        self._check(self._lib.r2f_stage_chroma_nr_v(self._h, C.byref(ps), C.byref(pd), int(size), y0, y1, int(src.shape[2]),
                                                    H_global, self._stream()))

    def chroma_nr(self, image, size, layout=None):
        """effects.chroma_nr_filter on a whole frame: (H, W, 3|4) or (3, H, W) in -> (3, H, W) XYZ planes out."""
        torch = self._torch
        _, H, W = self.layout_of(image, layout)
        tmp = torch.empty((3, H, W), dtype=torch.float32, device=self.device)
        out = torch.empty((3, H, W), dtype=torch.float32, device=self.device)
        self.stage_chroma_nr_h(image, tmp, size, layout=layout)
        self.stage_chroma_nr_v(tmp, out, size, y0=0, y1=H, H_global=H)
        return out

    def resize_area(self, image, out_h, out_w, layout=None):
        """Pre-path INTER_AREA down-scale of a whole frame -> (3, out_h, out_w) planes."""
        torch = self._torch
        self._check_image(image)
        layout, H, W = self.layout_of(image, layout)
        out = torch.empty((3, int(out_h), int(out_w)), dtype=torch.float32, device=self.device)
        pd = self.planes(out, 0)
        self._check(self._lib.r2f_resize_area(self._h, image.data_ptr(), layout, H, W, C.byref(pd), int(out_h), int(out_w),
                                              self._stream()))
        return out

    def resize_lanczos4_f32(self, image, out_h, out_w, layout=None):
        """Pre-path cv.resize(float32 frame, INTER_LANCZOS4) up-scale of a whole frame -> (3, out_h, out_w) planes."""
        torch = self._torch
        self._check_image(image)
        layout, H, W = self.layout_of(image, layout)
        out = torch.empty((3, int(out_h), int(out_w)), dtype=torch.float32, device=self.device)
        pd = self.planes(out, 0)
        self._check(self._lib.r2f_resize_lanczos4_f32(self._h, image.data_ptr(), layout, H, W, C.byref(pd), int(out_h), int(out_w),
                                                      self._stream()))
        return out

    def warp_affine(self, image, m_dst_to_src, window=None, layout=None):
        """cv.warpAffine(image, M, same size, INTER_LINEAR) restricted to `window` = (row0, col0, rows, cols) -> (3, rows, cols)
        planes.  m_dst_to_src: inverse of M, 2 x 3 (geometry.rotation_plan)."""
        torch = self._torch
        self._check_image(image)
        layout, H, W = self.layout_of(image, layout)
        r0, c0, nr, nc = (0, 0, H, W) if window is None else [int(v) for v in window]
        out = torch.empty((3, nr, nc), dtype=torch.float32, device=self.device)
        if nr == 0 or nc == 0:
            return out
        m = np.ascontiguousarray(np.asarray(m_dst_to_src, dtype=np.float64).reshape(6))
        pd = self.planes(out, 0)
        self._check(self._lib.r2f_warp_affine(self._h, image.data_ptr(), layout, H, W, m.ctypes.data, C.byref(pd), nr, nc, r0, c0,
                                              self._stream()))
        return out

    def lens_correct(self, image, profile_or_params, window=None, layout=None, tca=None, projection=None):
        """The lens correction of include/r2f.h (r2f_lens_correct: radial map, 8 x 8 LANCZOS4 gather, clamp at 0, vignetting gain)
        of a whole frame, restricted to `window` = (row0, col0, rows, cols) of the corrected frame -> (3, rows, cols) planes.
        profile_or_params: a raw2film_amd.lens.LensProfile (planned for this frame's size, its `tca` and `projection` included) or
        the r2f_lens_params of that size.  tca: the r2f_lens_tca_params that go with such params; with them the call is
        r2f_lens_correct_tca (red and blue sample at coordinates of their own).  projection: the r2f_lens_projection_params that go
        with such params; with them the call is r2f_lens_correct_projected (a fisheye frame is straightened), with or without `tca`."""
        torch = self._torch
        self._check_image(image)
        layout, H, W = self.layout_of(image, layout)
        if isinstance(profile_or_params, _lib.LensParams):
            params = profile_or_params
        elif tca is not None:
            raise ValueError("lens_correct: `tca` goes with r2f_lens_params; a LensProfile carries its own")
        elif projection is not None:
            raise ValueError("lens_correct: `projection` goes with r2f_lens_params; a LensProfile carries its own")
        else:
            params, projection, tca = profile_or_params.plan_projected(H, W)
        r0, c0, nr, nc = (0, 0, H, W) if window is None else [int(v) for v in window]
        out = torch.empty((3, nr, nc), dtype=torch.float32, device=self.device)
        if nr == 0 or nc == 0:
            return out
        pd = self.planes(out, 0)
        # which entry point, and the records it takes between the params and the planes
        if projection is not None:
            fn, records = self._lib.r2f_lens_correct_projected, (C.byref(projection), None if tca is None else C.byref(tca))
        elif tca is not None:
            fn, records = self._lib.r2f_lens_correct_tca, (C.byref(tca),)
        else:
            fn, records = self._lib.r2f_lens_correct, ()
        self._check(fn(self._h, image.data_ptr(), layout, H, W, C.byref(params), *records, C.byref(pd), nr, nc, r0, c0, self._stream()))
        return out

    def _mosaic_size(self, mosaic, what, m):
        """A mosaic as the entry points take it: uint16 or int16 bits, (H, W) of at least m x m samples, pitched rows allowed -> (H, W)."""
        torch = self._torch
        if not (isinstance(mosaic, torch.Tensor) and mosaic.is_cuda and mosaic.dtype in (torch.uint16, torch.int16) and mosaic.dim() == 2
                and mosaic.shape[0] >= m and mosaic.shape[1] >= m and mosaic.stride(1) == 1 and mosaic.stride(0) >= mosaic.shape[1]):
            raise ValueError(f"{what} needs a uint16 (H, W) CUDA mosaic of at least {m} x {m} samples with contiguous rows")
        self._same_device(mosaic, "mosaic")
        return int(mosaic.shape[0]), int(mosaic.shape[1])

    @staticmethod
    def _blend_clip(clip) -> int:
        if isinstance(clip, bool) or not isinstance(clip, numbers.Integral) or not 1 <= clip <= 65535:
            raise ValueError(f"demosaic: clip must be an integer in [1, 65535], got {clip!r}")
        return int(clip)

    @staticmethod
    def _median_passes(passes) -> int:
        n = _lib.MEDIAN_MAX_PASSES
        if isinstance(passes, bool) or not isinstance(passes, numbers.Integral) or not 1 <= passes <= n:
            raise ValueError(f"demosaic: passes must be an integer in [1, {n}] (LibRaw's med_passes; R2F_MEDIAN_MAX_PASSES), got {passes!r}")
        return int(passes)

    def demosaic(self, mosaic, params, factor=None, divisor=65535.0, *, clip=None, passes=0, orientation=0, window=None, out=None,
                 rows=None):
        """Every demosaic of include/r2f.h through one call: the kind of mosaic is the params' (a RawProfile or r2f_demosaic_params:
        Bayer; an XTransProfile or r2f_xtrans_params: X-Trans), the entry point is the one the options select (_lib.demosaic_entry).
        factor: None yields the uint16 (out_h, out_w, 3) frame; a factor yields the float32 frame decode_u16(that frame, factor,
        divisor) would, of `window` = (row0, col0, rows, cols) of it (default: all of it; Bayer only).
        clip: None, or Blend's level, an integer in [1, 65535] (LibRaw's highlight mode 2).  passes: 0, or step M's count, 1 ..
        MEDIAN_MAX_PASSES (LibRaw's med_passes).  orientation: 0 .. 7 (LibRaw's sizes.flip bits), not 0 with the uint16 frame only:
        `out` and `rows` are then those of the oriented frame O.  out: the tensor to write (default: a new one).  rows = (y0, y1):
        only those rows of `out` are written (default: all).  The methods below say what each form computes."""
        torch = self._torch
        what = "demosaic"
        if clip is not None:
            clip = self._blend_clip(clip)
        if passes != 0 or isinstance(passes, bool):
            passes = self._median_passes(passes)
        params_type = type(params) if type(params) in _lib.MOSAIC_KINDS else params._c_params
        H, W = self._mosaic_size(mosaic, what, _lib.MOSAIC_KINDS[params_type].min_side)
        if not isinstance(params, params_type):
            params = params.plan(H, W)
        if isinstance(orientation, bool) or not isinstance(orientation, numbers.Integral) or not 0 <= orientation <= 7:
            raise ValueError(f"{what}: orientation must be an integer 0 .. 7 (LibRaw's sizes.flip bits), got {orientation!r}")
        f32 = factor is not None
        if window is not None and not f32:
            raise ValueError(f"{what}: a window goes with the float epilogue (a factor); the uint16 frame is written whole")
        name, between = _lib.demosaic_entry(params_type, f32, orientation, clip, passes)
        r0, c0, nr, nc = (0, 0, int(params.out_h), int(params.out_w)) if window is None else (int(v) for v in window)
        if not (0 <= r0 and 0 <= c0 and nr > 0 and nc > 0 and r0 + nr <= params.out_h and c0 + nc <= params.out_w):
            raise ValueError(f"{what}: window {(r0, c0, nr, nc)} is not inside the {params.out_h} x {params.out_w} frame")
        given = {"orientation": (int(orientation),), "clip": (clip or 0,), "passes": (passes,), "window": (r0, c0, nr, nc)}
        if f32:
            given["decode"] = (float(np.float32(divisor)), float(np.float32(factor)))
        shape = (nc, nr, 3) if orientation & 4 else (nr, nc, 3)  # (no window with an orientation: the oriented frame's sides)
        dtypes, dtype_name = ((torch.float32,), "float32") if f32 else ((torch.uint16, torch.int16), "uint16")
        if out is None:
            out = torch.empty(shape, dtype=torch.float32 if f32 else mosaic.dtype, device=self.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype in dtypes and out.is_contiguous() and tuple(out.shape) == shape):
            raise ValueError(f"{what}: out must be a contiguous {dtype_name} CUDA tensor of shape {shape}")
        else:
            self._same_device(out, "out")
        y0, y1 = (0, shape[0]) if rows is None else (int(rows[0]), int(rows[1]))
        self._check(getattr(self._lib, name)(self._h, mosaic.data_ptr(), 0, H, int(mosaic.stride(0)), H, W, C.byref(params),
                                             *(v for arg in between for v in given[arg]), out.data_ptr(), y0, y1, self._stream()))
        return out

    def demosaic_u16(self, mosaic, params, out=None, rows=None, orientation=0):
        """The Bayer demosaic of include/r2f.h (r2f_demosaic_u16: black / scale, PPG or the half-size form, camera matrix, clip)
        of a uint16 (H, W) CUDA mosaic (int16 tensors are read as the same bits; rows may be pitched: stride(0) >= W, stride(1)
        = 1) -> uint16 (out_h, out_w, 3), the frame decode_u16 / decode_u16_auto / exposure_rows take.
        params: a raw2film_amd.raw.RawProfile (planned full size for this mosaic) or the r2f_demosaic_params of its size.
        rows = (y0, y1): only those output rows of `out` are written (default: all).
        orientation (0 .. 7, LibRaw's sizes.flip bits; not taken from a profile: name it): not 0 writes the oriented frame O of
        include/r2f.h (r2f_demosaic_oriented_u16) -- (out_w, out_h, 3) with bit 4 --, and `out` and `rows` are O's."""
        return self.demosaic(mosaic, params, out=out, rows=rows, orientation=orientation)

    def demosaic_xtrans(self, mosaic, params, out=None, rows=None, orientation=0):
        """The X-Trans demosaic of include/r2f.h (r2f_demosaic_xtrans_u16: black / scale, the project's own directional-green /
        colour-difference interpolation or the reduced third-size form, camera matrix, clip -- not LibRaw's algorithm) of a uint16
        (H, W) CUDA mosaic of at least 6 x 6 samples (int16 tensors are read as the same bits; rows may be pitched) -> uint16
        (out_h, out_w, 3), the frame decode_u16 / decode_u16_auto / exposure_rows take.
        params: a raw2film_amd.raw.XTransProfile (planned full size for this mosaic) or the r2f_xtrans_params of its size.
        rows = (y0, y1): only those output rows of `out` are written (default: all).
        orientation: demosaic_u16's (r2f_demosaic_xtrans_oriented_u16)."""
        return self.demosaic(mosaic, params, out=out, rows=rows, orientation=orientation)

    def demosaic_f32(self, mosaic, params, factor: float, divisor: float = 65535.0, window=None, out=None, rows=None):
        """demosaic_u16 and decode_u16 in one kernel (r2f_demosaic_f32): window = (row0, col0, rows, cols) of the demosaiced frame
        (default: all of it) -> float32 (rows, cols, 3), bit-identical to decode_u16(demosaic_u16(mosaic)[window], factor, divisor).
        mosaic, params: demosaic_u16's; the mosaic may be the whole landing buffer of which only some rows have arrived -- a call
        reads the rows its contract names and no others.  rows = (y0, y1): only those rows of the window are written."""
        return self.demosaic(mosaic, params, factor, divisor, window=window, out=out, rows=rows)

    def demosaic_blend_u16(self, mosaic, params, clip, out=None, rows=None, orientation=0):
        """demosaic_u16 with Blend (r2f_demosaic_blend_u16; include/r2f.h, LibRaw's highlight mode 2): a pixel with a channel above
        `clip` (an integer in [1, 65535]; a resolved "blend" profile's `blend_clip`) takes the chroma of its clipped version ahead of
        the camera matrix.  Everything else is demosaic_u16's, `orientation` included; clip = 65535 yields its bytes."""
        return self.demosaic(mosaic, params, clip=self._blend_clip(clip), out=out, rows=rows, orientation=orientation)

    def demosaic_xtrans_blend(self, mosaic, params, clip, out=None, rows=None, orientation=0):
        """demosaic_xtrans with Blend (r2f_demosaic_xtrans_blend_u16): demosaic_blend_u16's `clip` for an X-Trans mosaic."""
        return self.demosaic(mosaic, params, clip=self._blend_clip(clip), out=out, rows=rows, orientation=orientation)

    def demosaic_blend_f32(self, mosaic, params, clip, factor: float, divisor: float = 65535.0, window=None, out=None, rows=None):
        """demosaic_f32 with Blend (r2f_demosaic_blend_f32): bit-identical to decode_u16(demosaic_blend_u16(mosaic, params,
        clip)[window], factor, divisor)."""
        return self.demosaic(mosaic, params, factor, divisor, clip=self._blend_clip(clip), window=window, out=out, rows=rows)

    def demosaic_median_u16(self, mosaic, params, passes, clip=None, out=None, rows=None, orientation=0):
        """demosaic_u16 with step M (r2f_demosaic_median_u16; include/r2f.h, LibRaw's med_passes): `passes` (1 .. 4) passes of the
        3 x 3 median of R - G and B - G of the whole demosaiced frame between the interpolation and Blend.  clip: None for no
        Blend, else demosaic_blend_u16's.  Everything else is demosaic_u16's, `orientation` included; rows = (y0, y1) read the
        mosaic rows of `passes` more output rows either side."""
        return self.demosaic(mosaic, params, clip=clip, passes=self._median_passes(passes), out=out, rows=rows, orientation=orientation)

    def demosaic_xtrans_median(self, mosaic, params, passes, clip=None, out=None, rows=None, orientation=0):
        """demosaic_xtrans with step M (r2f_demosaic_xtrans_median_u16): demosaic_median_u16's `passes` and `clip` for an X-Trans
        mosaic."""
        return self.demosaic(mosaic, params, clip=clip, passes=self._median_passes(passes), out=out, rows=rows, orientation=orientation)

    def demosaic_median_f32(self, mosaic, params, passes, factor: float, divisor: float = 65535.0, clip=None, window=None, out=None,
                            rows=None):
        """demosaic_f32 with step M (r2f_demosaic_median_f32): bit-identical to decode_u16(demosaic_median_u16(mosaic, params,
        passes, clip)[window], factor, divisor).  The median at a window or row-range edge that is no frame edge reads the frame
        beyond it: a call reads the mosaic rows of `passes` more output rows either side."""
        return self.demosaic(mosaic, params, factor, divisor, clip=clip, passes=self._median_passes(passes), window=window, out=out, rows=rows)

    def mosaic_maximum(self, mosaic, profile_or_black, period=None, rows=None, out=None):
        """The data maximum of include/r2f.h (r2f_mosaic_maximum): the largest black-subtracted sample, clamped at 0, of a uint16
        (H, W) CUDA mosaic (int16 tensors are read as the same bits; rows may be pitched) -> int, read back from the device (4
        bytes, one synchronisation of the stream).  What a deferred profile's `resolve` takes.
        profile_or_black: a RawProfile or XTransProfile (its black table and its array's period), or period * period black levels
        in [0, 65535] with `period` 2 or 6 (default: 2 for 4 levels, 6 for 36).
        rows = (y0, y1): only those mosaic rows are read (default: all).
        out: a one-element int32 or uint32 CUDA tensor the maximum is folded into -- out = max(out, d of the rows) -- in place of
        a word of this call's own that starts at 0; `out` is then returned, and nothing is read back or waited for: bands in any
        order and any cut compose to the whole frame's value."""
        torch = self._torch
        black = getattr(profile_or_black, "black", profile_or_black)
        try:
            black = [int(b) for b in black]
        except (TypeError, ValueError):
            raise ValueError(f"mosaic_maximum: a profile or a sequence of black levels is required, got {profile_or_black!r}") from None
        if period is None:
            period = {4: 2, 36: 6}.get(len(black))
        if period not in (2, 6) or len(black) != period * period:
            raise ValueError(f"mosaic_maximum: {len(black)} black levels with period {period!r}; 4 go with period 2 and 36 with period 6")
        H, W = self._mosaic_size(mosaic, "mosaic_maximum", period)
        word = out
        if word is None:
            word = torch.zeros(1, dtype=torch.int32, device=self.device)
        elif not (isinstance(word, torch.Tensor) and word.is_cuda and word.dtype in (torch.int32, torch.uint32) and word.numel() == 1):
            raise ValueError("mosaic_maximum: out must be a one-element int32 or uint32 CUDA tensor")
        else:
            self._same_device(word, "out")
        y0, y1 = (0, H) if rows is None else (int(rows[0]), int(rows[1]))
        self._check(self._lib.r2f_mosaic_maximum(self._h, mosaic.data_ptr(), 0, H, int(mosaic.stride(0)), H, W, period,
                                                 (C.c_int32 * len(black))(*black), y0, y1, word.data_ptr(), self._stream()))
        return int(word.item()) if out is None else out

    def mosaic_denoise(self, mosaic, params, out=None):
        """The wavelet denoise of include/r2f.h (r2f_mosaic_denoise: rawpy's noise_thr=, ahead of the demosaic) of a uint16 (H, W)
        CUDA Bayer mosaic with even sides of at least 64 samples (int16 tensors are read as the same bits; rows may be pitched) ->
        the denoised mosaic, black-free and in units of t << shift, of the mosaic's dtype.
        params: the r2f_denoise_params of raw2film_amd.raw.WaveletDenoise.plan.
        out: a uint16 or int16 (H, W) CUDA tensor with contiguous samples along a row to write into (rows may be pitched); the
        mosaic itself is allowed.  The 12 bytes per sample of workspace are a buffer the context keeps and reuses."""
        torch = self._torch
        if not isinstance(params, _lib.DenoiseParams):
            raise ValueError(f"mosaic_denoise: params must be the r2f_denoise_params of WaveletDenoise.plan, got {type(params).__name__}")
        H, W = self._mosaic_size(mosaic, "mosaic_denoise", 64)
        if out is None:
            out = torch.empty((H, W), dtype=mosaic.dtype, device=self.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype in (torch.uint16, torch.int16) and tuple(out.shape) == (H, W)
                  and out.stride(1) == 1 and out.stride(0) >= W):
            raise ValueError(f"mosaic_denoise: out must be a uint16 CUDA tensor of shape {(H, W)} with contiguous rows")
        else:
            self._same_device(out, "out")
        nbytes = int(self._lib.r2f_mosaic_denoise_workspace_bytes(H, W))
        if nbytes == 0:
            raise ValueError(f"mosaic_denoise: a {H} x {W} mosaic; both sides must be even and at least 64")
        ws = self._denoise_workspace
        if ws is None or ws.numel() < nbytes:
            self._denoise_workspace = None
            ws = self._denoise_workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._check(self._lib.r2f_mosaic_denoise(self._h, mosaic.data_ptr(), int(mosaic.stride(0)), H, W, C.byref(params), out.data_ptr(),
                                                 int(out.stride(0)), ws.data_ptr(), int(ws.numel()), self._stream()))
        return out

    def mosaic_repair(self, mosaic, params, rows=None, count=None, out=None):
        """The hot-pixel repair of include/r2f.h (r2f_mosaic_repair: the project's own rule, ahead of everything else that reads the
        mosaic) of a uint16 (H, W) CUDA mosaic of at least 6 x 6 samples (int16 tensors are read as the same bits; rows may be
        pitched) -> the repaired mosaic, of the mosaic's dtype.
        params: the r2f_repair_params of raw2film_amd.raw.HotPixels.plan.
        rows = (y0, y1): only those mosaic rows are written (default: all); the call reads rows [y0 - 2, y1 + 2) of `mosaic`, clipped
        to the frame.
        count: a one-element int32 or uint32 CUDA tensor to which the call ADDS the number of samples it replaced in its rows (the
        caller zeroes it; nothing is read back or waited for); None: not counted.
        out: a uint16 or int16 (H, W) CUDA tensor with contiguous samples along a row to write into (rows may be pitched), which
        must not share bytes with the mosaic; None: the second mosaic is a buffer the context keeps and reuses for mosaics of this
        size -- the next call with out=None overwrites it, and row-range calls fill it band by band."""
        torch = self._torch
        if not isinstance(params, _lib.RepairParams):
            raise ValueError(f"mosaic_repair: params must be the r2f_repair_params of HotPixels.plan, got {type(params).__name__}")
        H, W = self._mosaic_size(mosaic, "mosaic_repair", 6)
        if out is None:
            out = self._repair_mosaic
            if out is None or tuple(out.shape) != (H, W) or out.dtype != mosaic.dtype:
                self._repair_mosaic = None
                out = self._repair_mosaic = torch.empty((H, W), dtype=mosaic.dtype, device=self.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype in (torch.uint16, torch.int16) and tuple(out.shape) == (H, W)
                  and out.stride(1) == 1 and out.stride(0) >= W):
            raise ValueError(f"mosaic_repair: out must be a uint16 CUDA tensor of shape {(H, W)} with contiguous rows")
        else:
            self._same_device(out, "out")
        if count is not None:
            if not (isinstance(count, torch.Tensor) and count.is_cuda and count.dtype in (torch.int32, torch.uint32) and count.numel() == 1):
                raise ValueError("mosaic_repair: count must be a one-element int32 or uint32 CUDA tensor")
            self._same_device(count, "count")
        y0, y1 = (0, H) if rows is None else (int(rows[0]), int(rows[1]))
        self._check(self._lib.r2f_mosaic_repair(self._h, mosaic.data_ptr(), 0, H, int(mosaic.stride(0)), H, W, C.byref(params),
                                                out.data_ptr(), int(out.stride(0)), y0, y1,
                                                None if count is None else count.data_ptr(), self._stream()))
        return out

    def decode_u16(self, image_u16, factor: float, divisor: float = 65535.0, out=None):
        """raw_to_linear's last two lines (raw_conversion.py:50-52) on the device: float32(u) / divisor * float32(factor) for a
        uint16 (H, W, 3 | 4) CUDA tensor (LibRaw's 16-bit output; int16 tensors are read as the same bits) -> float32 (H, W, 3).
        out: a contiguous float32 (H, W, 3) CUDA tensor to write into (e.g. a band of rows of a larger frame)."""
        torch = self._torch
        if not (image_u16.is_cuda and image_u16.dtype in (torch.uint16, torch.int16) and image_u16.is_contiguous()
                and image_u16.dim() == 3 and image_u16.shape[2] in (3, 4)):
            raise ValueError("decode_u16 needs a contiguous uint16 (H, W, 3 or 4) CUDA tensor")
        self._same_device(image_u16, "image")
        shape = (int(image_u16.shape[0]), int(image_u16.shape[1]), 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape):
            raise ValueError(f"decode_u16: out must be a contiguous float32 CUDA tensor of shape {shape}")
        else:
            self._same_device(out, "out")
        self._check(self._lib.r2f_decode_u16(self._h, image_u16.data_ptr(), int(image_u16.shape[0]), int(image_u16.shape[1]),
                                             int(image_u16.shape[2]), float(np.float32(divisor)), float(np.float32(factor)),
                                             out.data_ptr(), self._stream()))
        return out

    def _check_u16(self, t, what):
        torch = self._torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in (torch.uint16, torch.int16) and t.is_contiguous()
                and t.dim() == 3 and t.shape[2] in (3, 4) and t.shape[0] > 0 and t.shape[1] > 0):
            raise ValueError(f"{what} needs a contiguous, non-empty uint16 (rows, W, 3 or 4) CUDA tensor")
        self._same_device(t, what)

    def exposure_rows(self, rows_u16, root: float, *, H=None, gy0: int = 0, y0=None, y1=None):
        """The auto exposure's row statistic (r2f_exposure_rows; calc_exposure, color_processing.py:71-99): the fp64 sums of
        pow(green / 65535, 1 / root) over the sampled rows (global index even) of [y0, y1) into the context's per-row array.
        rows_u16: the uint16 rows [gy0, gy0 + rows) of a frame of H rows (default: the whole frame).  A row's sum depends on
        nothing but its bytes, W, channels and root, so bands of any size, in any order, give the frame's statistic bit for bit."""
        self._check_u16(rows_u16, "exposure_rows")
        rows, W, ch = (int(v) for v in rows_u16.shape)
        gy0 = int(gy0)
        H = gy0 + rows if H is None else int(H)
        y0 = gy0 if y0 is None else int(y0)
        y1 = gy0 + rows if y1 is None else int(y1)
        if not (0 <= gy0 <= y0 <= y1 <= gy0 + rows <= H):
            raise ValueError(f"exposure_rows: rows [{y0}, {y1}) of a buffer holding [{gy0}, {gy0 + rows}) of a frame of {H} rows")
        self._check(self._lib.r2f_exposure_rows(self._h, rows_u16.data_ptr(), gy0, rows, H, W, ch, y0, y1, float(root), self._stream()))

    def exposure_finish(self, H: int, W: int, root: float, ref_exposure: float = 0.18):
        """r2f_exposure_finish: the row sums of an H x W frame (every sampled row summed on this stream before) -> stops and the
        float32 factor in the context's device-side record, which decode_u16_auto reads.  Nothing comes back to the host here."""
        self._check(self._lib.r2f_exposure_finish(self._h, int(H), int(W), float(root), float(ref_exposure), self._stream()))

    def exposure_result(self):
        """(stops, float32 factor) of the last exposure_finish (r2f_exposure_result): waits for that kernel, not for what was
        queued behind it."""
        stops, factor = C.c_double(), C.c_float()
        self._check(self._lib.r2f_exposure_result(self._h, C.byref(stops), C.byref(factor)))
        return float(stops.value), np.float32(factor.value)

    def decode_u16_auto(self, frame_u16, window=None, divisor: float = 65535.0, out=None):
        """decode_u16 with the factor read from the context's exposure record (r2f_decode_u16_auto) -- the same floats as
        decode_u16 gives for that factor.  window = (row0, col0, rows, cols) of `frame_u16` to decode (default: all of it): a
        crop costs a pointer offset and a pitch, not a copy.  -> float32 (rows, cols, 3), into `out` when given."""
        torch = self._torch
        self._check_u16(frame_u16, "decode_u16_auto")
        rows, W, ch = (int(v) for v in frame_u16.shape)
        r0, c0, nr, nc = (0, 0, rows, W) if window is None else (int(v) for v in window)
        if not (0 <= r0 and 0 <= c0 and nr > 0 and nc > 0 and r0 + nr <= rows and c0 + nc <= W):
            raise ValueError(f"decode_u16_auto: window {(r0, c0, nr, nc)} is not inside the {rows} x {W} frame")
        shape = (nr, nc, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                  and tuple(out.shape) == shape):
            raise ValueError(f"decode_u16_auto: out must be a contiguous float32 CUDA tensor of shape {shape}")
        else:
            self._same_device(out, "out")
        src = frame_u16.data_ptr() + 2 * ch * (r0 * W + c0)
        self._check(self._lib.r2f_decode_u16_auto(self._h, src, nr, nc, ch, W, float(np.float32(divisor)), out.data_ptr(),
                                                  self._stream()))
        return out

    def blit_rgba8(self, image_f32, dst_rgba, transform: dict):
        """shaders/copy_to_int.wgsl: the float (H, W, 3) frame letterboxed into the uint8 (h, w, 4) destination tensor.
        `transform`: the dict of geometry.blit_transform (the shader's uniform block)."""
        torch = self._torch
        if not (image_f32.is_cuda and image_f32.dtype == torch.float32 and image_f32.is_contiguous() and image_f32.dim() == 3
                and image_f32.shape[2] == 3):
            raise ValueError("blit_rgba8 needs a contiguous float32 (H, W, 3) CUDA tensor")
        if not (dst_rgba.is_cuda and dst_rgba.dtype == torch.uint8 and dst_rgba.is_contiguous() and dst_rgba.dim() == 3
                and dst_rgba.shape[2] == 4):
            raise ValueError("blit_rgba8 needs a contiguous uint8 (h, w, 4) CUDA destination")
        self._same_device(image_f32, "image")
        self._same_device(dst_rgba, "destination")
        t = _lib.Blit(transform["scale_x"], transform["scale_y"], transform["offset_x"], transform["offset_y"],
                      transform["canvas_min_x"], transform["canvas_min_y"], transform["canvas_max_x"], transform["canvas_max_y"],
                      (C.c_float * 3)(*transform["canvas_color"]))
        self._check(self._lib.r2f_blit_rgba8(self._h, image_f32.data_ptr(), int(image_f32.shape[0]), int(image_f32.shape[1]),
                                             dst_rgba.data_ptr(), int(dst_rgba.shape[0]), int(dst_rgba.shape[1]), C.byref(t),
                                             self._stream()))
        return dst_rgba

    def histogram_render(self, counts, mix_table, height: int, target=None):
        """histogram.wgsl passes 2 + 3 (+ scale_texture.wgsl into `target`, a uint8 (h, w, 4) device tensor) from the (3, 256)
        device counts of `histogram_counts`; returns the (height, 256, 4) uint8 device bar image."""
        torch = self._torch
        mix = np.ascontiguousarray(np.asarray(mix_table, dtype=np.uint8).reshape(8, 4))
        image = torch.empty((int(height), 256, 4), dtype=torch.uint8, device=self.device)
        if not (isinstance(counts, torch.Tensor) and counts.is_cuda and counts.dtype in (torch.int32, torch.uint32)
                and tuple(counts.shape) == (3, 256)):
            raise ValueError("histogram_render needs the (3, 256) int32 CUDA counts of histogram_counts")
        self._same_device(counts, "counts")
        counts = counts.contiguous()
        if target is not None and not (target.is_cuda and target.dtype == torch.uint8 and target.is_contiguous() and target.dim() == 3
                                       and target.shape[2] == 4):
            raise ValueError("histogram_render needs a contiguous uint8 (h, w, 4) CUDA target")
        if target is not None:
            self._same_device(target, "target")
        self._check(self._lib.r2f_histogram_render(
            self._h, counts.data_ptr(), mix.ctypes.data, int(height), image.data_ptr(),
            target.data_ptr() if target is not None else None, int(target.shape[0]) if target is not None else 0,
            int(target.shape[1]) if target is not None else 0, self._stream()))
        return image

    def stencil_stats(self, which: int):
        """Per channel: dict(entries, rowsteps, phases, sym, unrolled, kh, kw, q, fft, window, real_spectrum) of the device form of
        stencil `which` (bench.py); fft = 1: the channel takes the FFT form, window = (rows, columns) of its last launch or None."""
        out = (C.c_int * 24)()
        self._check(self._lib.r2f_stencil_stats(self._h, int(which), out))
        keys = ("entries", "rowsteps", "phases", "sym", "kh", "kw", "q")
        stats = []
        for c in range(3):
            d = dict(zip(keys, out[8 * c:8 * c + 7]))
            word = out[8 * c + 7]
            d["unrolled"] = (d["sym"] >> 1) & 0x7F  # R of the fully unrolled (2 R + 1)^2 direct form, 0: the entry list
            d["separable"] = (d["sym"] >> 8) & 1  # grain stencil only: two 1-D passes of 2 R + 1 taps
            d["xpass_registers"] = (d["sym"] >> 9) & 1  # ... the one along x in registers as the noise is hashed (R <= 4)
            d["sym"] &= 1
            d["fft"] = word & 1
            dims = (word >> 1) & 0x1FFFFFFF
            d["window"] = (dims // 4096, dims % 4096) if dims else None
            d["real_spectrum"] = (word >> 30) & 1  # its last FFT launch multiplied by a real kernel spectrum (centred symmetric taps)
            stats.append(d)
        return stats

    def stream_copy(self, src, dst):
        """dst <- src with a float4 streaming kernel (bench.py's copy ceiling: 2 x the bytes of HBM traffic, no arithmetic)."""
        nbytes = src.numel() * src.element_size()
        if dst.numel() * dst.element_size() != nbytes or not (src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous()):
            raise ValueError("stream_copy needs two contiguous CUDA tensors of the same size in bytes")
        self._same_device(src, "source")
        self._same_device(dst, "destination")
        self._check(self._lib.r2f_stream_copy(self._h, src.data_ptr(), dst.data_ptr(), nbytes, self._stream()))

    def kernel_timing(self, cls: int):
        """(total ms, launches, algorithmic bytes) of FFT pass `cls` since the last call; needs set_option("kernel_timing", 1)."""
        ms, n, b = C.c_double(), C.c_int(), C.c_double()
        self._check(self._lib.r2f_kernel_timing(self._h, int(cls), C.byref(ms), C.byref(n), C.byref(b)))
        return ms.value, n.value, b.value

    def histogram_counts(self, image_u8):
        """Per-channel bin counts of a uint8 (H, W, 3) device image -> int32 (3, 256) device tensor (utils.py:160-165)."""
        torch = self._torch
        if not (image_u8.is_cuda and image_u8.dtype == torch.uint8 and image_u8.is_contiguous() and image_u8.dim() == 3
                and image_u8.shape[2] == 3):
            raise ValueError("histogram_counts needs a contiguous uint8 (H, W, 3) CUDA tensor")
        self._same_device(image_u8, "image")
        counts = torch.empty((3, 256), dtype=torch.int32, device=self.device)
        self._check(self._lib.r2f_histogram_u8(self._h, image_u8.data_ptr(), int(image_u8.shape[0]), int(image_u8.shape[1]),
                                               counts.data_ptr(), self._stream()))
        return counts

    def jpeg_bound_bytes(self, H: int, W: int, subsampling: int = 2) -> int:
        """Largest JPEG file r2f_jpeg_encode(_ex) can write for an H x W frame (subsampling: 0 4:4:4, 1 4:2:2, 2 4:2:0)."""
        if int(subsampling) == 2:
            return int(self._lib.r2f_jpeg_bound_bytes(int(H), int(W)))
        return int(self._lib.r2f_jpeg_bound_bytes_ex(int(H), int(W), int(subsampling)))

    def jpeg_bound_bytes_opts(self, H: int, W: int, quality: int, subsampling: int = 2, optimize: bool = False,
                              progressive: bool = False, restart: int = 0) -> int:
        """Largest JPEG file r2f_jpeg_encode_ex can write for an H x W frame with these options (r2f_jpeg_bound_bytes_opts)."""
        opts = _lib.JpegOpts(int(quality), int(subsampling), 1 if optimize else 0, 1 if progressive else 0, int(restart))
        return int(self._lib.r2f_jpeg_bound_bytes_opts(C.byref(opts), int(H), int(W)))

    def jpeg_encode(self, image_u8, quality: int, subsampling: int = 2, optimize: bool = False, progressive: bool = False,
                    restart: int = 0, density=(0, 0)):
        """Baseline JPEG of a uint8 (H, W, 3) device image (rows may be strided; pixels packed) -> (uint8 device buffer of
        jpeg_bound_bytes, int64 device tensor of 1 holding the file's length).  Asynchronous on the current stream, except with
        optimize, whose call waits once for the frame's symbol counts (r2f_jpeg_encode_ex), and progressive, whose call waits for
        the ten scans' counts and then for the file's length (the buffer is then the progressive bound).  subsampling: 0 4:4:4,
        1 4:2:2, 2 4:2:0.  restart: MCUs per restart interval (0: none; the buffer is then jpeg_bound_bytes_opts); density: APP0's
        (x, y) dots per inch, (0, 0) for none."""
        torch = self._torch
        if not (isinstance(image_u8, torch.Tensor) and image_u8.is_cuda and image_u8.dtype == torch.uint8 and image_u8.dim() == 3
                and image_u8.shape[2] == 3 and image_u8.stride(2) == 1 and image_u8.stride(1) == 3):
            raise ValueError("jpeg_encode needs a uint8 (H, W, 3) CUDA tensor with packed pixels (row stride free)")
        self._same_device(image_u8, "image")
        H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
        plain = not restart and not any(density)
        bound = (self.jpeg_bound_bytes_opts(H, W, quality, subsampling, optimize, bool(progressive), restart)
                 if progressive or restart else self.jpeg_bound_bytes(H, W, subsampling))
        if bound == 0:
            raise ValueError(f"jpeg_encode: a JPEG holds 1 .. 65535 pixels per side, got {H} x {W} (subsampling {subsampling})")
        out = torch.empty(bound, dtype=torch.uint8, device=self.device)
        length = torch.empty(1, dtype=torch.int64, device=self.device)
        if int(subsampling) == 2 and not optimize and not progressive and plain:
            self._check(self._lib.r2f_jpeg_encode(self._h, image_u8.data_ptr(), H, W, int(image_u8.stride(0)), int(quality),
                                                  out.data_ptr(), bound, length.data_ptr(), self._stream()))
        else:
            opts = _lib.JpegOpts(int(quality), int(subsampling), 1 if optimize else 0, 1 if progressive else 0, int(restart),
                                 int(density[0]), int(density[1]))
            self._check(self._lib.r2f_jpeg_encode_ex(self._h, image_u8.data_ptr(), H, W, int(image_u8.stride(0)), C.byref(opts),
                                                     out.data_ptr(), bound, length.data_ptr(), self._stream()))
        return out, length

    def jpeg_rows(self, H: int, W: int, quality: int, subsampling: int = 2, restart: int = 0, density=(0, 0)):
        """Open a row-wise JPEG encode of an H x W frame (r2f_jpeg_rows_begin) on the current stream -> a JpegRows: feed it the
        frame's rows in order with .rows(image_u8, y0, y1); .out holds the file, .length the count of its leading bytes that are
        final.  A one-shot jpeg_encode or another jpeg_rows on this context ends it.  subsampling: 0 4:4:4, 1 4:2:2 (8-row
        MCUs), 2 4:2:0 (16-row MCUs).  restart, density: as in jpeg_encode."""
        return JpegRows(self, H, W, quality, subsampling, restart, density)

    def stage_noise(self, params, y0, y1, W, want_hash=True, want_noise=True):
        torch = self._torch
        rows = y1 - y0
        h = torch.empty((3, rows, W), dtype=torch.int32, device=self.device) if want_hash else None
        n = torch.empty((3, rows, W), dtype=torch.float32, device=self.device) if want_noise else None
        rc = self._lib.r2f_stage_noise(
            self._h, C.byref(params), h.data_ptr() if h is not None else None,
            n.data_ptr() if n is not None else None, y0, y1, W, self._stream(),
        )
        self._check(rc)
        return h, n


class JpegRows:
    """A row-wise JPEG encode on a HipContext (HipContext.jpeg_rows).  `out`: uint8 device buffer of jpeg_bound_bytes(H, W) holding
    the file; `length`: int64 device tensor of 1, the number of leading bytes of `out` that are final -- the header and every
    stuffed scan byte no later rows can change -- and, once the last rows are in (`done`), the file's length.  Everything runs
    asynchronously on the stream that is current at each call."""

    def __init__(self, ctx, H, W, quality, subsampling=2, restart=0, density=(0, 0)):
        torch = ctx._torch
        H, W = int(H), int(W)
        plain = not restart and not any(density)
        bound = ctx.jpeg_bound_bytes_opts(H, W, quality, subsampling, restart=restart) if restart else ctx.jpeg_bound_bytes(H, W, subsampling)
        if bound == 0:
            raise ValueError(f"jpeg_rows: a JPEG holds 1 .. 65535 pixels per side, got {H} x {W} (subsampling {subsampling})")
        self._ctx, self.H, self.W, self.quality, self.subsampling = ctx, H, W, int(quality), int(subsampling)
        self.out = torch.empty(bound, dtype=torch.uint8, device=ctx.device)
        self.length = torch.empty(1, dtype=torch.int64, device=ctx.device)
        if self.subsampling == 2 and plain:
            ctx._check(ctx._lib.r2f_jpeg_rows_begin(ctx._h, H, W, self.quality, self.out.data_ptr(), bound, self.length.data_ptr(),
                                                    ctx._stream()))
        else:
            opts = _lib.JpegOpts(self.quality, self.subsampling, 0, 0, int(restart), int(density[0]), int(density[1]))
            ctx._check(ctx._lib.r2f_jpeg_rows_begin_ex(ctx._h, H, W, C.byref(opts), self.out.data_ptr(), bound,
                                                       self.length.data_ptr(), ctx._stream()))
        self.next_row, self.done = 0, False

    def rows(self, image_u8, y0: int, y1: int):
        """Encode rows [y0, y1) of `image_u8`, the whole uint8 (H, W, 3) device frame (rows may be strided, pixels packed; only
        these rows are read).  y0: where the call before ended (0 at first); y1: a multiple of the MCU height (16, or 8 for 4:2:2
        and 4:4:4) past y0, or H (the last call)."""
        torch, ctx = self._ctx._torch, self._ctx
        if not (isinstance(image_u8, torch.Tensor) and image_u8.is_cuda and image_u8.dtype == torch.uint8 and image_u8.dim() == 3
                and tuple(image_u8.shape) == (self.H, self.W, 3) and image_u8.stride(2) == 1 and image_u8.stride(1) == 3):
            raise ValueError(f"jpeg_rows.rows needs the uint8 ({self.H}, {self.W}, 3) CUDA frame with packed pixels (row stride free)")
        ctx._same_device(image_u8, "image")
        # (the library refuses rows out of order or misaligned, and rows of an encode that has ended: R2F_EINVAL)
        ctx._check(ctx._lib.r2f_jpeg_rows(ctx._h, image_u8.data_ptr(), int(image_u8.stride(0)), int(y0), int(y1), ctx._stream()))
        self.next_row, self.done = int(y1), int(y1) == self.H
