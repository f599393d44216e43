"""A session across the RAW and lens options: one long-lived HipProcessor (frame cache on, graphs at their default) walks
tests/prepath_cases.py's session_walk -- mosaics of differing shapes and arrays and one decoded frame, one axis value changed at a
time, film sliders, repeated calls, in-place edits announced by `src_version`, every fifth step an export -- and after every step
its result equals that of a second processor that reloads everything (cache=False, render_graph 0), which in turn equals that
processor's render of the model's frame F for the step's settings.  `last_raw_scale` and `last_raw_denoise` agree on cache hits
as well: a cached frame keeps them; so do the stops of a step that measures its exposure on the device.  What is exercised are the context-owned buffers across calls: the denoise workspace, the mosaic
buffers, the Lanczos and lens tables, the device exposure record, and the frame cache keyed by the profiles.
Fixed seeds; R2F_PREPATH_SESSION_STEPS lengthens a run."""

import os

import pytest

import prepath_cases as pc
from helpers import stocks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STEPS = int(os.environ.get("R2F_PREPATH_SESSION_STEPS", "40"))


def call(proc, entry, src, case, film, mosaic, **extra):
    neg, prt, _ = stocks()
    kw = dict(pc.load_keywords(case), exposure=pc.exposure_of(case, mosaic), halation=False, sharpness=False, grain=0, color_masking=1.0,
              print_film=prt, seed=3, **film, **extra)
    if mosaic:
        kw["raw_profile"], kw["raw_denoise"] = pc.profiles(case)
    if entry == "jpeg":
        return proc.process_jpeg(src, neg, 6, 0.4, quality=90, **kw)
    if entry == "tiff":
        return proc.process_tiff(src, neg, 6, 0.4, output_bits=16, **kw)
    return proc.process(src, neg, 6, 0.4, **kw)


@pytest.mark.parametrize("seed", pc.SESSION_SEEDS)
def test_a_session_across_sources_and_options_equals_reloading_and_the_models_frame(seed):
    from raw2film_amd import HipProcessor

    sources = {name: pc.session_source(name) for name in pc.SESSION_SOURCES}
    frames = {}  # (source, version, the RAW-side values) -> model_frame's answer for the source's current content
    a, b = HipProcessor(cameras={}, lenses={}, device=0), HipProcessor(cameras={}, lenses={}, device=0)
    b.ctx.set_option("render_graph", 0)
    try:
        for i, step in enumerate(pc.session_walk(seed, STEPS)):
            name, case, film, entry = step["source"], step["case"], step["film"], step["entry"]
            src, mosaic = sources[name], name != "frame"
            if step["kind"] == "edit":
                pc.edit_in_place(src, step["version"])
            where = (seed, i, step)
            got = call(a, entry, src, case, film, mosaic, src_version=(name, step["version"]))
            records = (a.last_raw_scale, a.last_raw_denoise)
            stops = a.last_auto_exposure
            want = call(b, entry, src, case, film, mosaic, cache=False)
            assert pc.same(got, want), where
            assert records == (b.last_raw_scale, b.last_raw_denoise), where
            if case["exposure"] == "auto":  # the stops of the device's record are this frame's, on a cache hit as well
                assert stops is not None and stops == b.last_auto_exposure, (where, stops, b.last_auto_exposure)
            assert a.exposure_rejected == b.exposure_rejected, where
            if not mosaic:
                assert records == (None, None), where
                continue
            key = (name, step["version"], tuple(case[k] for k in pc.RAW_AXES))
            if key not in frames:
                frames[key] = pc.raw_model(src, case)
            F, scale, denoise = frames[key]
            assert records == (scale, denoise), where
            assert pc.same(want, call(b, entry, F, case, film, False, cache=False)), where
    finally:
        a.close()
        b.close()
