"""The sensor's orientation in the device demosaic, without a GPU: the index map (raw2film_amd/csrc/r2f_mosaic_math.h, namespace
orient) in a stand-alone program under AddressSanitizer / UBSan (tests/orient_check.cpp), the profiles' `orientation` field, the
payload of phase 1 (crop numbers are those of the oriented frame, an upright payload is key for key what it was) and the two
stream gates.  That the device writes the oriented frame's bytes is tests/test_gpu_orientation.py's."""

import dataclasses
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import demosaic_model as dm
import xtrans_model as xm
from raw2film_amd import _lib
from raw2film_amd.hip_processor import HipProcessor
from raw2film_amd.payload import host_stream_gate, mosaic_frame_samples, mosaic_rejection, stream_rejection
from raw2film_amd.raw import RawProfile, XTransProfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def orient(D, o):
    """The NumPy statement of include/r2f.h."""
    E = D
    if o & 2:
        E = E[::-1]
    if o & 1:
        E = E[:, ::-1]
    if o & 4:
        E = E.transpose(1, 0, 2)
    return E


# ---- the stand-alone program
def test_index_map_is_the_definition_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path / "orient_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           os.path.join(ROOT, "tests", "orient_check.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "cases ok" in res.stdout


def test_the_named_orientations_are_the_turns_they_are_called():
    D = np.arange(4 * 6 * 3).reshape(4, 6, 3)
    assert np.array_equal(orient(D, 0), D) and np.array_equal(orient(D, 3), np.rot90(D, 2))
    assert np.array_equal(orient(D, 5), np.rot90(D, 1)) and np.array_equal(orient(D, 6), np.rot90(D, -1))
    assert np.array_equal(orient(D, 4), D.transpose(1, 0, 2)) and np.array_equal(orient(D, 7), np.rot90(D, 2).transpose(1, 0, 2))
    # the pixel map of the header, element by element
    for o in range(8):
        O = orient(D, o)
        assert O.shape == ((6, 4, 3) if o & 4 else (4, 6, 3))
        for r in range(O.shape[0]):
            for c in range(O.shape[1]):
                a, b = (c, r) if o & 4 else (r, c)
                assert np.array_equal(O[r, c], D[4 - 1 - a if o & 2 else a, 6 - 1 - b if o & 1 else b])


def test_the_header_states_the_definition_and_the_library_exports_both_entry_points():
    text = open(os.path.join(ROOT, "include", "r2f.h")).read()
    definition = text[text.index("The sensor's orientation in the demosaic"):text.index("R2F_API int r2f_demosaic_oriented_u16")]
    assert "UNPINNED" in definition and "sizes.flip" in definition and "E.transpose(1, 0, 2)" in definition
    assert "r2f_demosaic_xtrans_oriented_u16" in text
    lib = _lib.load()
    for name in ("r2f_demosaic_oriented_u16", "r2f_demosaic_xtrans_oriented_u16"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert f"`{name}`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---- the profiles
@pytest.mark.parametrize("cls", [RawProfile, XTransProfile], ids=lambda c: c.__name__)
def test_orientation_is_a_validated_field_of_equality_hash_and_repr(cls):
    assert cls().orientation == 0 and cls() == cls(orientation=0) and hash(cls()) == hash(cls(orientation=0))
    assert dataclasses.fields(cls)[-1].name == "orientation"
    a, b = cls(orientation=5), cls(orientation=np.int64(5))
    assert a == b and hash(a) == hash(b) and type(b.orientation) is int and {a: 1}[b] == 1
    assert a != cls() and a != cls(orientation=6) and len({cls(orientation=o) for o in range(8)}) == 8
    assert "orientation=5" in repr(a) and "orientation=0" in repr(cls())
    with pytest.raises(Exception):
        a.orientation = 0
    for bad in (-1, 8, 1.0, "3", None, True, False, (1,)):
        with pytest.raises(ValueError, match=cls.__name__):
            cls(orientation=bad)
    assert not hasattr(cls(), "flip")  # (process(flip=) is the aspect's)


def test_oriented_shape():
    for o in range(8):
        turned = bool(o & 4)
        assert RawProfile(orientation=o).oriented_shape(96, 146) == ((146, 96) if turned else (96, 146))
        assert RawProfile(orientation=o).oriented_shape(96, 146, True) == ((73, 48) if turned else (48, 73))
        assert XTransProfile(orientation=o).oriented_shape(97, 146) == ((146, 97) if turned else (97, 146))
        assert XTransProfile(orientation=o).oriented_shape(97, 146, True) == ((48, 32) if turned else (32, 48))
        # ... the shape of the definition's O
        p = RawProfile(orientation=o).plan(96, 146, True)
        assert orient(np.zeros((p.out_h, p.out_w, 3)), o).shape[:2] == RawProfile(orientation=o).oriented_shape(96, 146, True)
    assert bytes(RawProfile(orientation=5).plan(96, 146)) == bytes(RawProfile().plan(96, 146))  # (the params know nothing of it)


# ---- phase 1 of the processor
@pytest.fixture
def proc():
    p = HipProcessor.__new__(HipProcessor)
    p.cameras = p.lenses = None
    p.payload_alpha = True
    return p


def _bayer():
    mosaic, prof = dm.fixture("random", "GRBG", 96, 146)
    return mosaic, prof, dm


def _xtrans():
    mosaic, prof = xm.fixture("random", xm.PATTERNS[1], 97, 146)
    return mosaic, prof, xm


CROP_KEYS = ("final_resolution", "output_resolution", "canvas_resolution", "pipeline_resolution", "resize_to", "upscale_to", "chroma_nr",
             "u16_factor", "u16_window", "exposure_root")


@pytest.mark.parametrize("source", [_bayer, _xtrans], ids=["bayer-96x146", "xtrans-97x146"])
@pytest.mark.parametrize("kw", [
    dict(exposure=0.5), dict(exposure=0.5, half_size=False), dict(exposure=-1.0, zoom=1.3, rotate_times=1), dict(exposure=0.0, rotation=3.5, zoom=1.2),
    dict(exposure="device", zoom=1.3), dict(exposure=None), dict(exposure=0.25, flip=True, frame_width=36, frame_height=36),
    dict(exposure=0.5, resolution=(30, 45), canvas_mode="Uniform white", canvas_scale=1.1),
])
def test_an_oriented_payload_has_the_crop_numbers_of_the_oriented_frame(proc, source, kw):
    """Orientation 5 (90 degrees counter-clockwise): every crop-derived number is that of extract_image_data_cpu on the oriented
    model frame, and the step's window and turns, applied to that frame, give the frame the plain call uploads."""
    mosaic, upright, model = source()
    prof = dataclasses.replace(upright, orientation=5)
    half = kw.get("half_size", True)
    D = model.demosaic(mosaic, upright, half_size=half)
    rgb = np.ascontiguousarray(orient(D, 5))
    assert rgb.shape[:2] == (D.shape[1], D.shape[0]) == prof.oriented_shape(*mosaic.shape, half) and rgb.shape[0] > rgb.shape[1]
    pay = proc.extract_image_data_cpu(mosaic, raw_profile=prof, **kw)
    plain = proc.extract_image_data_cpu(rgb, **dict(kw, exposure="device" if kw["exposure"] is None else kw["exposure"]))
    assert set(pay) == set(plain) | {"demosaic"} and pay["image_array"] is mosaic
    step = pay["demosaic"]
    assert set(step) == {"params", "window", "rotate_times", "orientation"} and step["orientation"] == 5
    assert (step["params"].out_h, step["params"].out_w) == D.shape[:2]  # (the params are the upright frame's)
    for k in CROP_KEYS:
        assert pay[k] == plain[k], k
    assert (pay["warp"] is None) == (plain["warp"] is None)
    if pay["warp"] is not None:
        assert pay["warp"]["window"] == plain["warp"]["window"] and pay["warp"]["rotate_times"] == plain["warp"]["rotate_times"]
    if plain["u16_window"] is None:
        r0, c0, nr, nc = step["window"]
        assert np.array_equal(np.rot90(rgb[r0:r0 + nr, c0:c0 + nc], k=step["rotate_times"]), plain["image_array"])
    else:
        assert step["window"] is None and step["rotate_times"] == 0 and plain["image_array"].shape == rgb.shape
    # ... and they are not the upright frame's: a 3 : 2 crop of a portrait frame is another one (a square crop has the same sides)
    up = proc.extract_image_data_cpu(mosaic, raw_profile=upright, **kw)
    assert (up["pipeline_resolution"] != pay["pipeline_resolution"]) == (kw.get("frame_height", 24) != kw.get("frame_width", 36))


@pytest.mark.parametrize("source", [_bayer, _xtrans], ids=["bayer", "xtrans"])
def test_an_upright_payload_is_key_for_key_what_it_was(proc, source):
    mosaic, upright, _ = source()
    for prof in (upright, dataclasses.replace(upright, orientation=0)):
        for kw in (dict(exposure=0.5), dict(exposure=None, half_size=False), dict(exposure=0.5, rotate_times=1)):
            step = proc.extract_image_data_cpu(mosaic, raw_profile=prof, **kw)["demosaic"]
            assert set(step) == {"params", "window", "rotate_times"}


def test_frame_samples_follow_the_orientation():
    """With bit 4 the crops see the demosaiced frame with its sides swapped: the samples are those of a mosaic of the transposed shape
    (the aspect crop matches the longer side, so a 3 : 2 frame keeps all of itself either way)."""
    for shape, zoom in (((6000, 9000), 1.0), ((6000, 8000), 1.0), ((97, 146), 1.3), ((101, 131), 1.0)):
        src, swapped = np.zeros(shape, np.uint16), np.zeros(shape[::-1], np.uint16)
        for o in range(8):
            for half, reduction in ((False, 2), (True, 3)):
                want = mosaic_frame_samples(swapped if o & 4 else src, half, 1.5, False, zoom, reduction)
                assert mosaic_frame_samples(src, half, 1.5, False, zoom, reduction, o) == want
                assert mosaic_frame_samples(src, half, 1.5, False, zoom, reduction, orientation=o) == want
    big = np.zeros((6000, 9000), np.uint16)
    assert mosaic_frame_samples(big, False, 1.5, False, 1.0, 2, 5) == 6000 * 9000 * 3 == mosaic_frame_samples(big, False, 1.5, False, 1.0)


def test_both_stream_gates_name_the_orientation_and_pass_the_same_upright_call(proc):
    big = np.zeros((1 << 13, 1 << 13), np.uint16)
    # (everything a Bayer mosaic needs in order to stream is there: stops, no turn, no lens step, a large window)
    assert host_stream_gate(big, 16, 0.0, 0, "No", 0.0, False, True, stops=True, frame_samples=3 << 26) is None
    assert host_stream_gate(big, 16, 0.0, 0, "No", 0.0, False, True, stops=True, frame_samples=3 << 26, orientation=0) is None
    for o in range(1, 8):
        for xtrans in (False, True):
            why = host_stream_gate(big, 16, 0.0, 0, "No", 0.0, False, True, stops=True, frame_samples=3 << 26, xtrans=xtrans, orientation=o)
            assert why is not None and "demosaic" in why and f"orientation = {o}" in why
    assert mosaic_rejection(True, 0, False, 3 << 26) is None and "orientation" in mosaic_rejection(True, 0, False, 3 << 26, False, 6)
    # the existing reasons and their order, for an upright mosaic
    assert "X-Trans" in mosaic_rejection(False, 1, True, None, True) and "not given in stops" in mosaic_rejection(False, 1, True, None)
    assert "rotate_times" in mosaic_rejection(True, 1, True, None) and "lens step" in mosaic_rejection(True, 0, True, None)
    assert "no window" in mosaic_rejection(True, 0, False, None) and "below 16.7 M" in mosaic_rejection(True, 0, False, 100)
    # the payload's gate
    mosaic, upright, _ = _bayer()
    pay = proc.extract_image_data_cpu(mosaic, raw_profile=dataclasses.replace(upright, orientation=6), exposure=0.5, half_size=False)
    why = stream_rejection(pay, (8192, 8192), "torch.int16", False, "gpu")
    assert why is not None and "demosaic" in why and "orientation = 6" in why
    pay = proc.extract_image_data_cpu(mosaic, raw_profile=upright, exposure=0.5, half_size=False)
    assert "orientation" not in stream_rejection(pay, (8192, 8192), "torch.int16", False, "gpu")  # (its window is small: that reason)
    # the processor's gate
    proc.stream_bands = 16
    settings = {k: p.default for k, p in inspect.signature(HipProcessor.process).parameters.items() if p.default is not inspect.Parameter.empty}
    assert proc._host_stream_gate(big, dict(settings, raw_profile=RawProfile("RGGB"), exposure=0.5, half_size=False)) is None
    for prof in (RawProfile("RGGB", orientation=3), XTransProfile(orientation=5)):
        why = proc._host_stream_gate(big, dict(settings, raw_profile=prof, exposure=0.5, half_size=False))
        assert why is not None and f"orientation = {prof.orientation}" in why


def test_an_orientation_is_part_of_the_image_cache_key(proc):
    uploads = []

    def prepare(payload):
        uploads.append(payload.get("demosaic"))
        proc._texture = ("frame", None, {})
        proc.image_param_dict = None

    proc.prepare_gpu_textures = prepare
    mosaic, upright, _ = _bayer()
    proc.load_image_texture(mosaic, raw_profile=upright, exposure=0.0)
    proc.load_image_texture(mosaic, raw_profile=dataclasses.replace(upright, orientation=0), exposure=0.0)
    assert len(uploads) == 1 and "orientation" not in uploads[0]
    proc.load_image_texture(mosaic, raw_profile=dataclasses.replace(upright, orientation=5), exposure=0.0)
    assert len(uploads) == 2 and uploads[1]["orientation"] == 5
    proc.load_image_texture(mosaic, raw_profile=dataclasses.replace(upright, orientation=5), exposure=0.0)
    assert len(uploads) == 2
