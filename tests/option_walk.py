"""The walk over r2f_set_option that tests/golden/option_walk.json records and tests/test_options_host.py /
tests/test_gpu_options.py repeat: every option name x VALUES, plus one unknown name, in this order on one context.

    python tests/option_walk.py path/to/libr2f_hip.so out.json

records the walk of THAT library (needs a GPU: it creates a context).  The committed file was recorded this way from the library
built at the commit before the option table replaced the strcmp chain, so it says what the chain did, not what the table does."""

import ctypes as C
import json
import sys

NAMES = [
    "stencil_variant", "render_graph", "stencil_lds_kb", "stencil_sym", "stencil_ablate", "kernel_timing", "stencil_fft",
    "stencil_fft_window", "stencil_fft_window_max", "stencil_fft_even_batches", "stencil_fixed", "grain_fixed", "front_fast",
    "grain_separable", "front_blocks_per_cu", "stencil_fft_window_rows", "stencil_fft_min_taps", "stencil_fft_streams",
    "stencil_fft_cols_walk", "stencil_fft_mixed_sign", "stencil_fft_real_spectrum", "stencil_fft_epilogue_lds",
    "stencil_fft_scratch96_auto", "stencil_fft_scratch96", "stencil_fft_scratch32", "stencil_fft_batch", "xcd_band", "xcd_remap",
]
UNKNOWN = "no_such_option"
VALUES = [-2, -1, 0, 1, 2, 7, 8, 64, 65, 160, 161, 256, 300, 512, 1024, 2**31 - 1]


def walk(lib):
    """[[name, value, return code, r2f_last_error text after the call, generation step of the call], ...] on a fresh context."""
    lib.r2f_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.r2f_destroy.argtypes = [C.c_void_p]
    lib.r2f_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.r2f_last_error.argtypes = [C.c_void_p]
    lib.r2f_last_error.restype = C.c_char_p
    lib.r2f_generation.argtypes = [C.c_void_p]
    lib.r2f_generation.restype = C.c_uint64
    h = C.c_void_p()
    assert lib.r2f_create(0, C.byref(h)) == 0
    rows = []
    try:
        for name in NAMES + [UNKNOWN]:
            for v in VALUES:
                g0 = lib.r2f_generation(h)
                rc = lib.r2f_set_option(h, name.encode(), v)
                rows.append([name, v, rc, lib.r2f_last_error(h).decode(), lib.r2f_generation(h) - g0])
    finally:
        lib.r2f_destroy(h)
    return rows


if __name__ == "__main__":
    rows = walk(C.CDLL(sys.argv[1]))
    header = ("r2f_set_option over every option name x a fixed value list (tests/option_walk.py), recorded by running the walk against "
              "the library built from the commit BEFORE the option table (the strcmp chain in r2f_set_option); not written from the table")
    with open(sys.argv[2], "w") as f:
        json.dump({"header": header, "columns": ["name", "value", "rc", "last_error", "generation_step"], "rows": rows}, f, indent=0)
    print(len(rows), "rows")
