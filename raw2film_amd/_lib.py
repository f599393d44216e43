"""ctypes binding of libr2f_hip.so (C ABI declared in include/r2f.h).

The product path has NO CPU fallback: if the library is missing or a symbol is absent the
import of the binding raises, and every render call goes through these entry points.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libr2f_hip.so")

# enums of include/r2f.h
LAYOUT_HWC3, LAYOUT_HWC4, LAYOUT_CHW = 0, 1, 2
LENS_NONE, LENS_POLY3, LENS_POLY5, LENS_PTLENS = 0, 1, 2, 3
TCA_NONE, TCA_LINEAR, TCA_POLY3 = 0, 1, 2
PROJ_NONE, PROJ_FISHEYE, PROJ_STEREOGRAPHIC, PROJ_EQUISOLID, PROJ_ORTHOGRAPHIC = 0, 1, 2, 3, 4
CFA_RGGB, CFA_BGGR, CFA_GRBG, CFA_GBRG = 0, 1, 2, 3
DEMOSAIC_TILE_W, DEMOSAIC_TILE_H = 64, 32  # R2F_DEMOSAIC_TILE_*
XTRANS_TILE_W, XTRANS_TILE_H = 64, 32  # R2F_XTRANS_TILE_*
MOSAIC_MAX_VEC, MOSAIC_MAX_ROWS = 8, 4  # R2F_MOSAIC_MAX_*
MOSAIC_REPAIR_VEC, MOSAIC_REPAIR_ROWS = 8, 4  # R2F_MOSAIC_REPAIR_*
DENOISE_TILE_W, DENOISE_TILE_H = 64, 32  # R2F_DENOISE_TILE_*
KERNEL_HALATION, KERNEL_MTF, KERNEL_GRAIN = 0, 1, 2
F_MATRIX, F_HALATION, F_MTF, F_GRAIN, F_GRAIN_MONO, F_BURN, F_IDENTITY_DONE, F_FRAME_RESIDENT = 1, 2, 4, 8, 16, 32, 64, 128
F_TRACK_RANGE, F_RANGE_VALID = 256, 512
UPTO_EXPOSURE, UPTO_DENSITY, UPTO_OUTPUT = 0, 1, 2
OK, EINVAL, EHIP, ETOOLARGE = 0, -1, -2, -3


class Params(C.Structure):
    _fields_ = [
        ("flags", C.c_uint32),
        ("seed", C.c_uint32),
        ("log_eps", C.c_float),
        ("lut3d_scale", C.c_float),
        ("lut3d_mode", C.c_int32),
        ("burn_cell", C.c_int32),
        ("burn_strength", C.c_float),
        ("burn_d_ref", C.c_float),
    ]


class Planes(C.Structure):
    _fields_ = [
        ("data", C.c_void_p),
        ("plane_stride", C.c_int64),
        ("gy0", C.c_int32),
        ("rows", C.c_int32),
    ]


class FftPlan(C.Structure):  # r2f_fft_plan
    _fields_ = [("ny", C.c_int32), ("nx", C.c_int32), ("vy", C.c_int32), ("vx", C.c_int32), ("gx", C.c_int32), ("ntiles", C.c_int32),
                ("pairs_per_channel", C.c_int32), ("pairs", C.c_int32), ("streams", C.c_int32), ("batch", C.c_int32),
                ("launches", C.c_int32), ("scratch_bytes", C.c_uint64)]


class Blit(C.Structure):  # r2f_blit: the uniform block of shaders/copy_to_int.wgsl
    _fields_ = [
        ("scale_x", C.c_float), ("scale_y", C.c_float), ("offset_x", C.c_float), ("offset_y", C.c_float),
        ("canvas_min_x", C.c_float), ("canvas_min_y", C.c_float), ("canvas_max_x", C.c_float), ("canvas_max_y", C.c_float),
        ("canvas_color", C.c_float * 3),
    ]


class JpegOpts(C.Structure):  # r2f_jpeg_opts (sampling: 0 4:4:4, 1 4:2:2, 2 4:2:0; progressive: 0 or 1; the rest 0: none)
    _fields_ = [("quality", C.c_int32), ("sampling", C.c_int32), ("optimize", C.c_int32), ("progressive", C.c_int32),
                ("restart_interval", C.c_int32), ("x_density", C.c_int32), ("y_density", C.c_int32)]


class TiffPlan(C.Structure):  # r2f_tiff_plan
    _fields_ = [("header_bytes", C.c_uint64), ("file_bytes", C.c_uint64), ("row_bytes", C.c_uint64), ("rows_per_strip", C.c_uint32),
                ("strips", C.c_uint32)]


class LensProfile(C.Structure):  # r2f_lens_profile (raw2film_amd.lens.LensProfile fills it)
    _fields_ = [("model", C.c_int32), ("n_coef", C.c_int32), ("coef", C.c_double * 3), ("has_vignetting", C.c_int32),
                ("auto_scale", C.c_int32), ("vignetting", C.c_double * 3), ("center", C.c_double * 2), ("scale", C.c_double),
                ("norm_radius_px", C.c_double)]


class LensParams(C.Structure):  # r2f_lens_params: the fp32 constants of one frame size
    _fields_ = [("model", C.c_int32), ("vignetting", C.c_int32), ("cx", C.c_float), ("cy", C.c_float), ("q", C.c_float),
                ("inv_scale", C.c_float), ("c0", C.c_float), ("k", C.c_float * 3), ("qv", C.c_float), ("v", C.c_float * 3),
                ("scale", C.c_double)]


class LensTca(C.Structure):  # r2f_lens_tca: (v, c, b) of red and of blue (raw2film_amd.lens.LensProfile.to_c_tca fills it)
    _fields_ = [("model", C.c_int32), ("n_coef", C.c_int32), ("red", C.c_double * 3), ("blue", C.c_double * 3)]


class LensTcaParams(C.Structure):  # r2f_lens_tca_params: the same constants in fp32
    _fields_ = [("model", C.c_int32), ("red", C.c_float * 3), ("blue", C.c_float * 3)]


class LensProjection(C.Structure):  # r2f_lens_projection (raw2film_amd.lens.LensProfile.to_c_projection fills it)
    _fields_ = [("type", C.c_int32), ("focal", C.c_double)]


class LensProjectionParams(C.Structure):  # r2f_lens_projection_params: the projection step's constant in fp32
    _fields_ = [("type", C.c_int32), ("inv_focal", C.c_float)]


class RawProfile(C.Structure):  # r2f_raw_profile (raw2film_amd.raw.RawProfile fills it)
    _fields_ = [("pattern", C.c_int32), ("half_size", C.c_int32), ("black", C.c_double * 4), ("mul", C.c_double * 4),
                ("matrix", C.c_double * 9)]


class DemosaicParams(C.Structure):  # r2f_demosaic_params: the constants of one frame size
    _fields_ = [("cfa", C.c_int32 * 4), ("black", C.c_int32 * 4), ("mul", C.c_float * 4), ("M", C.c_float * 9),
                ("half_size", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32)]


class XTransProfile(C.Structure):  # r2f_xtrans_profile (raw2film_amd.raw.XTransProfile fills it)
    _fields_ = [("pattern", C.c_int32 * 36), ("reduced", C.c_int32), ("black", C.c_double * 36), ("mul", C.c_double * 3),
                ("matrix", C.c_double * 9)]


class XTransParams(C.Structure):  # r2f_xtrans_params: the constants and per-phase tables of one frame size
    _fields_ = [("cfa", C.c_uint8 * 36), ("gap", C.c_uint8 * 4 * 36), ("taps", C.c_uint16 * 2 * 36), ("wsum", C.c_uint8 * 2 * 36),
                ("cell_count", C.c_uint8 * 3 * 4), ("recip", C.c_uint32 * 2 * 36), ("black", C.c_int32 * 36), ("mul", C.c_float * 3),
                ("M", C.c_float * 9), ("reduced", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32)]


class RawLevels(C.Structure):  # r2f_raw_levels (raw2film_amd.raw.RawLevels fills it)
    _fields_ = [("white_balance", C.c_double * 3), ("white_level", C.c_int32), ("adjust_maximum_thr", C.c_double)]


class RawScale(C.Structure):  # r2f_raw_scale: the multipliers of one frame, the maximum they scale to and whether it was the measured one
    _fields_ = [("mul", C.c_double * 3), ("maximum_used", C.c_int32), ("adjusted", C.c_int32)]


class Highlight(C.Structure):  # r2f_highlight: the highlight mode a scale was planned with, and mode 2's clip level
    _fields_ = [("mode", C.c_int32), ("clip", C.c_int32)]


class DenoiseParams(C.Structure):  # r2f_denoise_params (raw2film_amd.raw.WaveletDenoise.plan fills it)
    _fields_ = [("black", C.c_int32 * 4), ("shift", C.c_int32), ("threshold", C.c_float)]


class RepairParams(C.Structure):  # r2f_repair_params (raw2film_amd.raw.HotPixels.plan fills it)
    _fields_ = [("period", C.c_int32), ("black", C.c_int32 * 36), ("offset", C.c_int8 * 2 * 4 * 36), ("threshold", C.c_int32),
                ("q", C.c_int32), ("min_neighbours", C.c_int32)]


HIGHLIGHT_CLIP, HIGHLIGHT_UNCLIP, HIGHLIGHT_BLEND = 0, 1, 2  # R2F_HIGHLIGHT_*: LibRaw's highlight modes 0, 1 and 2
MEDIAN_MAX_PASSES = 4  # R2F_MEDIAN_MAX_PASSES: the most passes of step M (LibRaw's med_passes) the median kernels' LDS holds

_P = C.POINTER
_fp = C.c_void_p  # float* (host numpy or device) passed as an address

# The demosaic entry points of include/r2f.h.  All share the head (ctx, src_rows, src_gy0, src_nrows, src_pitch, H, W, params) and the
# tail (dst, y0, y1, stream); this table is the one place that says what each takes in between, in the header's order, and which
# options select it (demosaic_entry).  DEMOSAIC_ARGS: an argument's name here -> the C parameters it stands for.
DEMOSAIC_ARGS = {"orientation": (("orientation", C.c_int),), "clip": (("clip", C.c_int),), "passes": (("passes", C.c_int),),
                 "window": (("row0", C.c_int), ("col0", C.c_int), ("rows", C.c_int), ("cols", C.c_int)),
                 "decode": (("divisor", C.c_float), ("factor", C.c_float))}


class MosaicKind(NamedTuple):
    """A kind of mosaic, by its params struct (MOSAIC_KINDS)."""
    min_side: int  # the smallest side of such a mosaic
    reduced_field: str  # the params field that says "reduced"
    entries: dict  # (float epilogue, form) -> (entry point, the arguments between `params` and `dst`)

    def reduced(self, params) -> bool:
        return bool(getattr(params, self.reduced_field))


MOSAIC_KINDS = {
    DemosaicParams: MosaicKind(2, "half_size", {
        (False, "plain"): ("r2f_demosaic_u16", ()),
        (False, "oriented"): ("r2f_demosaic_oriented_u16", ("orientation",)),
        (False, "blend"): ("r2f_demosaic_blend_u16", ("orientation", "clip")),
        (False, "median"): ("r2f_demosaic_median_u16", ("orientation", "clip", "passes")),
        (True, "plain"): ("r2f_demosaic_f32", ("window", "decode")),
        (True, "blend"): ("r2f_demosaic_blend_f32", ("clip", "window", "decode")),
        (True, "median"): ("r2f_demosaic_median_f32", ("clip", "passes", "window", "decode")),
    }),
    XTransParams: MosaicKind(6, "reduced", {
        (False, "plain"): ("r2f_demosaic_xtrans_u16", ()),
        (False, "oriented"): ("r2f_demosaic_xtrans_oriented_u16", ("orientation",)),
        (False, "blend"): ("r2f_demosaic_xtrans_blend_u16", ("orientation", "clip")),
        (False, "median"): ("r2f_demosaic_xtrans_median_u16", ("orientation", "clip", "passes")),
    }),
}


def demosaic_entry(params_type, f32, orientation=0, clip=None, passes=0):
    """Which entry point a demosaic's options select -> (its name, the arguments it takes between `params` and `dst`).  passes > 0:
    the median form (a `clip` of None goes as 0); else a clip: the blend form (an orientation of 0 is passed along); else an
    orientation with the uint16 result: the oriented form; else the plain one.  ValueError for what has no entry point."""
    if f32 and orientation:
        raise ValueError(f"the float epilogue writes the upright frame: orientation {orientation!r} has no entry point")
    form = "median" if passes else "blend" if clip is not None else "oriented" if orientation else "plain"
    try:
        return MOSAIC_KINDS[params_type].entries[bool(f32), form]
    except KeyError:
        raise ValueError(f"no demosaic entry point takes {params_type.__name__} with the {'float' if f32 else 'uint16'} epilogue") from None


def _demosaic_signatures():
    head = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int]
    tail = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return {name: (C.c_int, head + [_P(params_type)] + [t for a in args for _, t in DEMOSAIC_ARGS[a]] + tail)
            for params_type, kind in MOSAIC_KINDS.items() for name, args in kind.entries.values()}


_SIGNATURES = {
    "r2f_version": (C.c_char_p, []),
    "r2f_create": (C.c_int, [C.c_int, _P(C.c_void_p)]),
    "r2f_destroy": (None, [C.c_void_p]),
    "r2f_last_error": (C.c_char_p, [C.c_void_p]),
    "r2f_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "r2f_set_matrix3x3": (C.c_int, [C.c_void_p, _fp]),
    "r2f_set_lut2d": (C.c_int, [C.c_void_p, _fp, C.c_int]),
    "r2f_set_curve1d": (C.c_int, [C.c_void_p, _fp, C.c_int]),
    "r2f_set_lut3d": (C.c_int, [C.c_void_p, _fp, C.c_int]),
    "r2f_set_grain_lut": (C.c_int, [C.c_void_p, _fp, C.c_int]),
    "r2f_set_kernel": (C.c_int, [C.c_void_p, C.c_int, _fp, C.c_int, C.c_int, C.c_int]),
    "r2f_workspace_bytes": (C.c_size_t, [_P(Params), C.c_int, C.c_int]),
    "r2f_render": (
        C.c_int,
        [C.c_void_p, _P(Params), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p],
    ),
    "r2f_stage_front": (
        C.c_int,
        [C.c_void_p, _P(Params), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _P(Planes), C.c_void_p, C.c_void_p,
         C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_stage_halation": (
        C.c_int,
        [C.c_void_p, _P(Params), _P(Planes), _P(Planes), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_stage_exposure_range": (C.c_int, [C.c_void_p, _P(Planes), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "r2f_stage_mtf": (
        C.c_int,
        [C.c_void_p, _P(Params), _P(Planes), _P(Planes), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_stage_tail": (
        C.c_int,
        [C.c_void_p, _P(Params), _P(Planes), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
         C.c_void_p],
    ),
    "r2f_stage_grain": (
        C.c_int,
        [C.c_void_p, _P(Params), _P(Planes), _P(Planes), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_stage_burn_sums": (
        C.c_int,
        [C.c_void_p, _P(Params), _P(Planes), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_stage_burn_map": (
        C.c_int,
        [C.c_void_p, _P(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_stage_chroma_nr_h": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _P(Planes), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_stage_chroma_nr_v": (
        C.c_int,
        [C.c_void_p, _P(Planes), _P(Planes), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_resize_area": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _P(Planes), C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_stage_noise": (
        C.c_int,
        [C.c_void_p, _P(Params), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_stage_stencil": (
        C.c_int,
        [C.c_void_p, C.c_int, _P(Planes), _P(Planes), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_warp_affine": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, _P(Planes), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_lens_plan": (C.c_int, [_P(LensProfile), C.c_int, C.c_int, _P(LensParams)]),
    "r2f_lens_phase_table": (C.c_int, [C.c_void_p]),
    "r2f_lens_correct": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _P(LensParams), _P(Planes), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_lens_plan_tca": (C.c_int, [_P(LensProfile), _P(LensTca), C.c_int, C.c_int, _P(LensParams), _P(LensTcaParams)]),
    "r2f_lens_correct_tca": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _P(LensParams), _P(LensTcaParams), _P(Planes), C.c_int, C.c_int, C.c_int,
         C.c_int, C.c_void_p],
    ),
    "r2f_lens_plan_projected": (
        C.c_int,
        [_P(LensProfile), _P(LensProjection), _P(LensTca), C.c_int, C.c_int, _P(LensParams), _P(LensProjectionParams), _P(LensTcaParams)],
    ),
    "r2f_lens_correct_projected": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _P(LensParams), _P(LensProjectionParams), _P(LensTcaParams), _P(Planes),
         C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_demosaic_plan": (C.c_int, [_P(RawProfile), C.c_int, C.c_int, _P(DemosaicParams)]),
    **_demosaic_signatures(),
    "r2f_xtrans_plan": (C.c_int, [_P(XTransProfile), C.c_int, C.c_int, _P(XTransParams)]),
    "r2f_raw_scale_plan": (C.c_int, [_P(RawLevels), _P(C.c_double), C.c_int, C.c_uint32, _P(RawScale)]),
    "r2f_raw_scale_plan_highlight": (
        C.c_int, [_P(RawLevels), _P(C.c_double), C.c_int, C.c_uint32, C.c_int, _P(RawScale), _P(Highlight)]),
    "r2f_mosaic_maximum": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, _P(C.c_int32), C.c_int, C.c_int, C.c_void_p,
         C.c_void_p],
    ),
    "r2f_mosaic_denoise_plan": (C.c_int, [C.c_double, C.c_int, _P(C.c_double), C.c_int, C.c_int, _P(DenoiseParams)]),
    "r2f_mosaic_denoise_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "r2f_mosaic_denoise": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, _P(DenoiseParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p],
    ),
    "r2f_mosaic_denoise_level": (
        C.c_int,
        [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, _P(DenoiseParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t,
         C.c_void_p],
    ),
    "r2f_mosaic_repair_plan": (
        C.c_int,
        [C.c_int, _P(C.c_int32), _P(C.c_double), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P(RepairParams)],
    ),
    "r2f_mosaic_repair": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, _P(RepairParams), C.c_void_p, C.c_int64, C.c_int, C.c_int,
         C.c_void_p, C.c_void_p],
    ),
    "r2f_resize_lanczos4_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "r2f_lanczos4_table": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "r2f_kernel_timing": (C.c_int, [C.c_void_p, C.c_int, _P(C.c_double), _P(C.c_int), _P(C.c_double)]),
    "r2f_stage_grain_field": (C.c_int, [C.c_void_p, _P(Params), _P(Planes), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "r2f_stage_tail_field": (
        C.c_int,
        [C.c_void_p, _P(Params), _P(Planes), _P(Planes), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_stencil_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "r2f_histogram_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "r2f_stage_front_split": (
        C.c_int,
        [C.c_void_p, _P(Params), C.c_void_p, C.c_int, C.c_int, C.c_int, _P(Planes), _P(Planes), C.c_int, C.c_int, C.c_int, C.c_int,
         _P(C.c_int), C.c_void_p],
    ),
    "r2f_resize_lanczos4_f32": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _P(Planes), C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_lanczos4_table_f32": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "r2f_resize_area_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "r2f_decode_u16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "r2f_exposure_rows": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p],
    ),
    "r2f_exposure_finish": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p]),
    "r2f_decode_u16_auto": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_float, C.c_void_p, C.c_void_p],
    ),
    "r2f_exposure_result": (C.c_int, [C.c_void_p, _P(C.c_double), _P(C.c_float)]),
    "r2f_blit_rgba8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, _P(Blit), C.c_void_p]),
    "r2f_plan_fft": (C.c_int, [C.c_int] * 11 + [_P(FftPlan)]),
    "r2f_plan_stencil": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "r2f_plan_tile_order": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "r2f_generation": (C.c_uint64, [C.c_void_p]),
    "r2f_render_stats": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "r2f_write_frame_params": (C.c_int, [C.c_void_p, _P(Params), C.c_void_p]),
    "r2f_frame_exposure_range": (C.c_int, [C.c_void_p, _P(C.c_float), _P(C.c_int), _P(C.c_int)]),
    "r2f_frame_scratch_choice": (C.c_int, [C.c_void_p, _P(C.c_int), _P(C.c_int)]),
    "r2f_frame_scratch_flags": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, _P(C.c_int)]),
    "r2f_stream_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "r2f_histogram_render": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    ),
    "r2f_jpeg_bound_bytes": (C.c_uint64, [C.c_int, C.c_int]),
    "r2f_jpeg_header": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, _P(C.c_size_t)]),
    "r2f_jpeg_encode": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p],
    ),
    "r2f_jpeg_rows_begin": (
        C.c_int,
        [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p],
    ),
    "r2f_jpeg_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "r2f_jpeg_bound_bytes_ex": (C.c_uint64, [C.c_int, C.c_int, C.c_int]),
    "r2f_jpeg_header_ex": (C.c_int, [_P(JpegOpts), C.c_int, C.c_int, C.c_void_p, C.c_size_t, _P(C.c_size_t)]),
    "r2f_jpeg_bound_bytes_opts": (C.c_uint64, [_P(JpegOpts), C.c_int, C.c_int]),
    "r2f_jpeg_optimal_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_int)]),
    "r2f_jpeg_encode_ex": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _P(JpegOpts), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p],
    ),
    "r2f_jpeg_rows_begin_ex": (
        C.c_int,
        [C.c_void_p, C.c_int, C.c_int, _P(JpegOpts), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p],
    ),
    "r2f_render16": (
        C.c_int,
        [C.c_void_p, _P(Params), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p],
    ),
    "r2f_stage_front16": (
        C.c_int,
        [C.c_void_p, _P(Params), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
         C.c_int, C.c_void_p],
    ),
    "r2f_stage_tail16": (
        C.c_int,
        [C.c_void_p, _P(Params), _P(Planes), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
         C.c_int, C.c_void_p],
    ),
    "r2f_stage_tail_field16": (
        C.c_int,
        [C.c_void_p, _P(Params), _P(Planes), _P(Planes), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
         C.c_int, C.c_void_p],
    ),
    "r2f_resize_lanczos4_u16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "r2f_resize_area_u16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "r2f_tiff_header": (
        C.c_int,
        [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, _P(C.c_size_t), _P(TiffPlan)],
    ),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def _bind(path: str) -> C.CDLL:
    # torch FIRST: its wheel ships a HIP runtime of its own (torch/lib/libamdhip64.so), and the dynamic loader keeps whichever
    # libamdhip64 a process met first.  Loaded before torch, this library would pull in the system's runtime (/opt/rocm/lib) and torch
    # would then run on that one instead of the one it was built against -- on the GPU box r2f_create then fails with R2F_EHIP
    # (found with `python __graft_entry__.py --smoke`, i.e. build() -- which binds the library -- and smoke() in ONE process).  The
    # Python layer needs torch anyway (device buffers, streams); a host that only wants the C ABI binds the .so itself.
    try:
        import torch  # noqa: F401
    except ImportError:  # (the plan-only entry points and the symbol tests work without it)
        pass
    lib = C.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return lib


def load(path: str | None = None) -> C.CDLL:
    """dlopen the in-tree library and bind every symbol of include/r2f.h; raises if absent.
    path: ANOTHER build of the library (a development variant, tools/build_variant.py) bound beside the in-tree one -- the
    library exports nothing but its C ABI, so two builds in one process do not interpose each other's internals."""
    global _lib
    if path is not None and os.path.abspath(path) != os.path.abspath(LIB_PATH):
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing")
        return _bind(os.path.abspath(path))
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m raw2film_amd.build` (hipcc, gfx950). "
            "raw2film_amd has no CPU fallback."
        )
    _lib = _bind(LIB_PATH)
    return _lib
