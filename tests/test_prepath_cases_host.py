"""tests/golden/prepath_pairs.json and tests/prepath_cases.py without a GPU: the list covers every admissible pair of axis values
and misses exactly the refused ones; no case is a refusal -- phase 1 runs for the mosaic and for the model's frame F, and the two
payloads agree on every resolution and window --; every refused combination raises the error `refusal` cites; the model frames
are no vacuous inputs (contrast, shape, the sibling's difference, blended pixels, the adjusted flag); and the session walk of
tests/test_gpu_prepath_session.py visits what it is there for."""

import re

import numpy as np
import pytest

import highlight_model as hm
import prepath_cases as pc

LIST = pc.load_list()
IDS = [pc.case_id(case) for case, _, _ in LIST]
RESOLUTIONS = ("final_resolution", "resize_to", "upscale_to", "output_resolution", "canvas_resolution", "pipeline_resolution")


def test_the_list_covers_every_admissible_pair_and_misses_exactly_the_refused_ones():
    assert len(LIST) <= pc.CAP and len(set(IDS)) == len(IDS)
    for case, _, _ in LIST:
        assert list(case) == list(pc.AXES) and all(case[a] in pc.AXES[a] for a in pc.AXES), case
    for axis, values in pc.AXES.items():
        assert {case[axis] for case, _, _ in LIST} == set(values), axis
    covered = set().union(*(pc.pairs_of(case) for case, _, _ in LIST))
    refused = pc.refused_pairs()
    assert len(pc.all_pairs()) == 1441 and len(refused) == 10
    assert pc.all_pairs() - covered == refused, sorted(pc.all_pairs() - covered - refused) + sorted(covered & refused)


def test_every_case_has_a_sibling_with_one_option_neutralised_and_every_option_serves_three_times():
    uses = dict.fromkeys(pc.NEUTRAL, 0)
    for case, option, sibling in LIST:
        axis, active, neutral = pc.NEUTRAL[option]
        assert active(case) and sibling == {**case, axis: neutral} and pc.admissible(sibling), (case, option)
        uses[option] += 1
    assert min(uses.values()) >= 3, uses


def _windows(payload):
    lens, warp = payload.get("lens"), payload.get("warp")
    return (None if lens is None else (lens["window"], lens["rotate_times"]),
            None if warp is None else (warp["window"], warp["rotate_times"], warp["m_dst_to_src"].tobytes()))


@pytest.mark.parametrize("row", LIST, ids=IDS)
def test_no_case_is_a_refusal_and_both_routes_plan_the_same_frame(row):
    case, option, sibling = row
    assert pc.admissible(case)
    mosaic = pc.mosaic_of(case)
    F, scale, denoise = pc.model_frame(case)
    profile, _ = pc.profiles(case)
    assert F.dtype == np.uint16 and F.shape == (*profile.oriented_shape(*mosaic.shape, case["half_size"]), 3)
    a, b = pc.phase1(case, mosaic, True), pc.phase1(case, F, False)
    for key in RESOLUTIONS:
        assert a[key] == b[key], key
    assert _windows(a) == _windows(b)
    assert a["image_array"].shape == mosaic.shape and set(a["demosaic"]) == pc.demosaic_keys(case)
    assert a["exposure_rejected"] is None and b["exposure_rejected"] is None
    # the inputs are no vacuous ones: contrast behind the crops, and the sibling's frame is another picture
    kept = pc.cropped(F, b)
    assert kept.std() > 1
    G = pc.model_frame(sibling)[0]
    other = pc.cropped(G, pc.phase1(sibling, G, False))
    if other.shape != kept.shape:  # only a sibling that undoes a transposing orientation frames another shape: its common corner is compared
        assert option == "orientation" and case["orientation"] & 4 and G.shape == (F.shape[1], F.shape[0], 3), (option, other.shape)
        h, w = min(kept.shape[0], other.shape[0]), min(kept.shape[1], other.shape[1])
        kept, other = kept[:h, :w], other[:h, :w]
    differing = float((other != kept).any(axis=-1).mean())
    assert kept.size >= 300 and differing >= 0.1, (option, differing)
    if case["highlight"] == "blend":
        stats = {}
        pc.raw_model(mosaic, case, stats)
        assert stats["blended"] >= hm.MIN_BLENDED * stats["pixels"], stats
    assert (scale is None) == (case["scale"] == "numeric") and (denoise is None) == (case["raw_denoise"] == "none")
    if scale is not None:
        assert scale["adjusted"] == (case["scale"] == "adjusted"), scale
    if denoise is not None:
        assert denoise["shift"] == (1 if case["raw_denoise"] == "fixed" else 2), denoise


@pytest.mark.parametrize("pair", sorted(pc.refused_pairs(), key=repr), ids=lambda p: f"{p[0][0]}={p[0][1]}+{p[1][0]}={p[1][1]}")
def test_a_refused_pair_raises_what_the_predicate_cites(pair):
    base = {**LIST[0][0], "array": "RGGB", "scale": "nominal", "highlight": "clip", "raw_denoise": "none", "exposure": "stops",
            "rotation": 0.0, "rotate_times": 0}
    assert pc.admissible(base)
    case = {**base, pair[0][0]: pair[0][1], pair[1][0]: pair[1][1]}
    error, text, _ = pc.refusal(case)
    with pytest.raises(error, match=re.escape(text)):
        pc.phase1(case, pc.mosaic_of(case), True)


def test_sixteen_bits_into_a_texture_is_refused_before_any_work():
    from raw2film_amd.hip_processor import check_output_bits

    with pytest.raises(ValueError, match="cannot be combined with dst_texture"):
        check_output_bits(16, dst_texture=object())


def test_the_module_needs_no_torch():
    import os
    import subprocess
    import sys

    code = ("import sys; sys.path.insert(0, 'tests'); import prepath_cases as pc; pc.model_frame(pc.load_list()[0][0]); "
            "assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_the_session_walks_together_visit_every_post_path():
    posts = {s["case"]["post"] for seed in pc.SESSION_SEEDS for s in pc.session_walk(seed, 40) if s["source"] != "frame" and s["entry"] == "process"}
    assert posts == set(pc.AXES["post"]), posts


@pytest.mark.parametrize("seed", pc.SESSION_SEEDS)
def test_the_session_walk_visits_what_it_is_there_for(seed):
    walk = pc.session_walk(seed, 40)
    assert walk == pc.session_walk(seed, 40) and len(walk) == 40
    kinds = [s["kind"] for s in walk]
    for kind in pc.STEP_KINDS:
        assert kinds.count(kind) >= 2, (kind, kinds)
    assert {s["source"] for s in walk} == set(pc.SESSION_SOURCES)
    bayer = [s["source"] for s in walk if s["source"].startswith("bayer")]
    assert sum(1 for p, q in zip(bayer, bayer[1:]) if p != q) >= 2, bayer  # the denoise and mosaic buffers shrink and grow
    # every RAW-side axis and the lens profile change between two process() calls on one mosaic: a cache key that missed one shows
    assert set(pc.RAW_AXES[1:] + ("lens_profile",)) <= pc.cache_changes(walk), pc.cache_changes(walk)
    # the device exposure record: exposure=None through process() on both Bayer shapes and the X-Trans mosaic, on a repeated call
    # (a cache hit) and behind an in-place edit; and a turned or rotated frame, which takes its exposure in stops
    assert {"bayer", "bayer2", "xtrans", "repeat", "edit"} <= pc.auto_exposure_visits(walk), pc.auto_exposure_visits(walk)
    on_mosaics = [s["case"] for s in walk if s["source"] != "frame"]
    assert any(c["rotation"] or c["rotate_times"] for c in on_mosaics)
    posts = {s["case"]["post"] for s in walk if s["source"] != "frame" and s["entry"] == "process"} - {"plain"}
    assert len(posts) >= 2, posts
    # most steps are a mosaic's, of several sets of RAW-side values: what the GPU test compares with the model's frame
    assert len(on_mosaics) >= 20
    assert len({(s["source"], s["version"], tuple(s["case"][a] for a in pc.RAW_AXES)) for s in walk if s["source"] != "frame"}) >= 5
    assert [s["entry"] for s in walk[4::5]] == ["jpeg", "tiff"] * 4 and all(s["entry"] == "process" for i, s in enumerate(walk) if i % 5 != 4)
    for prev, step in zip(walk, walk[1:]):
        assert pc.admissible(step["case"]) or step["source"] == "frame"
        changed = [a for a in step["case"] if a != "array" and step["case"][a] != prev["case"][a]]
        if step["kind"] == "axis":
            assert len(changed) == 1 and step["source"] == prev["source"] and step["film"] == prev["film"]
        elif step["kind"] == "source":
            assert step["source"] != prev["source"] and changed in ([], ["raw_denoise"])
        elif step["kind"] == "film":
            assert not changed and step["film"] != prev["film"]
        else:
            assert not changed and step["film"] == prev["film"] and step["source"] == prev["source"]
            assert step["version"] == prev["version"] + (step["kind"] == "edit")
    # every case of the walk on a mosaic source is one the processor takes: phase 1 does not refuse it
    for step in walk:
        if step["source"] != "frame":
            pc.phase1({**step["case"], "entry": "process8"}, pc._source(step["source"]), True)
