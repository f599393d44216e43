"""The one table of the demosaic entry points (raw2film_amd._lib.MOSAIC_KINDS) against include/r2f.h, and the rule by which a step's
options pick an entry point (_lib.demosaic_entry) against that rule written out here.  No GPU, no library: the header's text and
the table."""

import ctypes as C
import itertools
import os
import re

import pytest

from raw2film_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ["ctx", "src_rows", "src_gy0", "src_nrows", "src_pitch", "H", "W", "params"]
TAIL = ["y0", "y1", "stream"]  # behind the destination, whose name says its element type
C_TYPES = {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64}


def prototypes():
    """{name: [(type, parameter name)]} of the r2f_demosaic_* entry points the header declares (the planner is not one)."""
    text = open(os.path.join(ROOT, "include", "r2f.h")).read()
    found = {}
    for name, params in re.findall(r"R2F_API int (r2f_demosaic_\w+)\(([^;]*?)\);", text, re.S):
        if name == "r2f_demosaic_plan":
            continue
        found[name] = [tuple(" ".join(p.split()).rsplit(" ", 1)) for p in params.split(",")]
    return found


def table():
    """{name: (params struct, the argument names between `params` and `dst`)} of the table under test."""
    return {name: (params_type, args) for params_type, kind in _lib.MOSAIC_KINDS.items() for name, args in kind.entries.values()}


def test_the_table_names_the_headers_entry_points_and_their_arguments_in_its_order():
    header, entries = prototypes(), table()
    assert len(header) == 11 and set(header) == set(entries)
    assert sum(len(kind.entries) for kind in _lib.MOSAIC_KINDS.values()) == 11  # (no entry point under two keys)
    for name, params in header.items():
        params_type, args = entries[name]
        names = [n for _, n in params]
        assert names[:8] == HEAD and names[-3:] == TAIL and names[-4].startswith("dst_"), name
        struct = {"const r2f_demosaic_params*": _lib.DemosaicParams, "const r2f_xtrans_params*": _lib.XTransParams}[params[7][0]]
        assert struct is params_type, name
        expanded = [pair for a in args for pair in _lib.DEMOSAIC_ARGS[a]]
        assert names[8:-4] == [n for n, _ in expanded], name
        res, argtypes = _lib._SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == len(params), name
        assert argtypes[:8] == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(params_type)], name
        assert argtypes[8:-4] == [t for _, t in expanded] == [C_TYPES[t] for t, _ in params[8:-4]], name
        assert argtypes[-4:] == [C.c_void_p, C.c_int, C.c_int, C.c_void_p], name
        for (ctype, _), bound in zip(params[:7], argtypes[:7]):  # (a pointer goes as an address)
            assert bound is (C.c_void_p if ctype.endswith("*") else C_TYPES[ctype]), name


def test_each_kind_states_its_smallest_side_and_the_field_that_says_reduced():
    bayer, xtrans = _lib.MOSAIC_KINDS[_lib.DemosaicParams], _lib.MOSAIC_KINDS[_lib.XTransParams]
    assert (bayer.min_side, bayer.reduced_field) == (2, "half_size") and (xtrans.min_side, xtrans.reduced_field) == (6, "reduced")
    for kind, params_type in ((bayer, _lib.DemosaicParams), (xtrans, _lib.XTransParams)):
        p = params_type()
        assert kind.reduced(p) is False
        setattr(p, kind.reduced_field, 1)
        assert kind.reduced(p) is True


# the rule, written out: (X-Trans, float epilogue, form) -> (entry point, the arguments between `params` and `dst`)
WINDOW_DECODE = ("window", "decode")
RULE = {
    (False, False, "plain"): ("r2f_demosaic_u16", ()),
    (False, False, "oriented"): ("r2f_demosaic_oriented_u16", ("orientation",)),
    (False, False, "blend"): ("r2f_demosaic_blend_u16", ("orientation", "clip")),
    (False, False, "median"): ("r2f_demosaic_median_u16", ("orientation", "clip", "passes")),
    (False, True, "plain"): ("r2f_demosaic_f32", WINDOW_DECODE),
    (False, True, "blend"): ("r2f_demosaic_blend_f32", ("clip",) + WINDOW_DECODE),
    (False, True, "median"): ("r2f_demosaic_median_f32", ("clip", "passes") + WINDOW_DECODE),
    (True, False, "plain"): ("r2f_demosaic_xtrans_u16", ()),
    (True, False, "oriented"): ("r2f_demosaic_xtrans_oriented_u16", ("orientation",)),
    (True, False, "blend"): ("r2f_demosaic_xtrans_blend_u16", ("orientation", "clip")),
    (True, False, "median"): ("r2f_demosaic_xtrans_median_u16", ("orientation", "clip", "passes")),
}
PRODUCT = list(itertools.product((False, True), (False, True), (0, 5), (None, 1, 65535), (0, 1, 4)))


def test_the_product_of_options_selects_by_the_stated_rule():
    assert len(RULE) == 11 and len(PRODUCT) == 72
    reached = set()
    for xtrans, f32, orientation, clip, passes in PRODUCT:
        params_type = _lib.XTransParams if xtrans else _lib.DemosaicParams
        case = (xtrans, f32, orientation, clip, passes)
        if (xtrans and f32) or (f32 and orientation):  # no X-Trans float epilogue; the float epilogue is upright
            with pytest.raises(ValueError):
                _lib.demosaic_entry(params_type, f32, orientation, clip, passes)
            continue
        if passes > 0:
            form = "median"
        elif clip is not None:
            form = "blend"
        elif orientation and not f32:
            form = "oriented"
        else:
            form = "plain"
        assert _lib.demosaic_entry(params_type, f32, orientation, clip, passes) == RULE[xtrans, f32, form], case
        reached.add((xtrans, f32, form))
    assert reached == set(RULE)  # every entry point is some options' choice
