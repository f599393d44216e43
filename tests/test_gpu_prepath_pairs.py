"""The RAW and lens options of HipProcessor in pairs, end to end: over the pairwise list tests/golden/prepath_pairs.json every entry
point on a mosaic with the case's profiles returns, byte for byte, what the same entry point returns on the uint16 frame F that the
tests' models make of that mosaic (tests/prepath_cases.py: model_frame) -- both sides run the same kernels behind the demosaic but
take different crop routes (the demosaic step, the device decode or the lens step cuts on one side, the host on the other).
`last_raw_scale` and `last_raw_denoise` are the models' numbers, and a sibling case -- one RAW-side option neutralised -- renders
another picture, so that no equality holds vacuously.  No tolerance anywhere."""

import numpy as np
import pytest

import prepath_cases as pc
from helpers import stocks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LIST = pc.load_list()
FILM = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, seed=3)


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


def run(proc, case, src, mosaic):
    """The case's entry point on its mosaic (with its profiles) or on a decoded frame -> (the result, the payload or None)."""
    neg, prt, _ = stocks()
    load = dict(pc.load_keywords(case), exposure=pc.exposure_of(case, mosaic))
    if mosaic:
        load["raw_profile"], load["raw_denoise"] = pc.profiles(case)
    film = dict(FILM, print_film=prt)
    entry = case["entry"]
    if entry == "process8":
        return proc.process(src, neg, 6, 0.4, **load, **film), None
    if entry == "process16":
        return proc.process(src, neg, 6, 0.4, output_bits=16, **load, **film), None
    if entry == "jpeg":
        return proc.process_jpeg(src, neg, 6, 0.4, quality=90, **load, **film), None
    if entry == "tiff16":
        return proc.process_tiff(src, neg, 6, 0.4, output_bits=16, **load, **film), None
    if entry == "texture":
        dst = torch.zeros(pc.TEXTURE_SHAPE, dtype=torch.uint8, device="cuda")
        assert proc.process(src, neg, 6, 0.4, dst_texture=dst, **load, **film) is None
        return dst.cpu().numpy(), None
    payload = proc.extract_image_data_cpu(src, **load)
    rest = dict(film, **{k: load[k] for k in ("frame_width", "frame_height", "canvas_mode", "canvas_scale")})
    if entry == "two_phase":
        return proc.process_preloaded(payload, neg, 6, 0.4, final_scaling="cpu", **rest), payload
    assert entry == "submit"
    return proc.submit_preloaded(payload, neg, 6, 0.4, final_scaling="cpu", **rest).result(), payload


@pytest.mark.parametrize("row", LIST, ids=[pc.case_id(case) for case, _, _ in LIST])
def test_the_mosaic_renders_the_bytes_of_the_models_frame(proc, row):
    case, option, sibling = row
    mosaic = pc.mosaic_of(case)
    F, scale, denoise = pc.model_frame(case)
    got, payload = run(proc, case, mosaic, True)
    assert proc.last_raw_scale == scale and proc.last_raw_denoise == denoise
    assert proc.exposure_rejected is None
    if payload is not None:
        assert payload["image_array"].shape == mosaic.shape and set(payload["demosaic"]) == pc.demosaic_keys(case)
    want, _ = run(proc, case, F, False)
    assert proc.last_raw_scale is None and proc.last_raw_denoise is None and proc.exposure_rejected is None
    if isinstance(got, bytes):
        assert type(want) is bytes and np.frombuffer(got, dtype=np.uint8).std() > 1
    else:
        assert got.shape == want.shape and got.dtype == want.dtype and got.std() > 1
        assert got.dtype == (np.uint16 if case["entry"] == "process16" else np.uint8)
    assert pc.same(got, want), case["entry"] if isinstance(got, bytes) else int((got != want).sum())
    other, _ = run(proc, sibling, pc.mosaic_of(sibling), True)
    assert not pc.same(got, other), option  # (the option changed the picture: the equality above does not hold vacuously)
