"""The RAW and lens pre-path on the device against a simulated camera and lens (tests/camera_sim.py): a scene known in closed form,
exposed through a sensor and a lens that do the physical inverse of what each profile field claims to correct, must come back --
and under every named misreading of a field it must not.  The thresholds are those tools/make_camera_sim.py derived from the NumPy
models on the CPU (tests/golden/camera_sim.json; tests/test_camera_sim_host.py holds the models to them); nothing here runs a
model or an oracle, and nothing is measured into a bound.

Per step through HipContext (the order of the steps is this file's there), composed through HipProcessor (the order is the
processor's: extract_image_data_cpu, then the upload and _prepare_device_frame, the exposure factor divided out)."""

import json
import os

import numpy as np
import pytest

import camera_sim as cs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_sim.json")) as _f:
    GOLDEN = json.load(_f)["checks"]


class DeviceBackend:
    """camera_sim's backend over HipContext and HipProcessor."""

    def __init__(self, ctx, proc=None):
        self.ctx, self.proc = ctx, proc

    def develop(self, mosaic, profile, half_size=False, denoise=None, repair=None, keep_units=False):
        from raw2film_amd.raw import WaveletDenoise, XTransProfile

        ctx = self.ctx
        H, W = mosaic.shape
        m = torch.from_numpy(np.array(mosaic).view(np.int16)).cuda()  # (uint16 bits)
        if repair is not None:
            m = ctx.mosaic_repair(m, repair.plan(profile, H, W))
        resolved, scale = profile, None
        if profile.deferred:
            resolved, scale = profile.resolve_scale(ctx.mosaic_maximum(m, profile))
        if denoise is not None:
            dn = denoise.plan(resolved.black, H, W, denoise.maximum if denoise.maximum is not None else int(scale.maximum_used))
            m = ctx.mosaic_denoise(m, dn)
            resolved = WaveletDenoise.shifted(resolved, 0 if keep_units else dn.shift)
        params = resolved.plan(H, W, half_size)
        xtrans = isinstance(profile, XTransProfile)
        clip, passes, o = resolved.blend_clip, profile.median_passes, profile.orientation
        if passes:
            out = (ctx.demosaic_xtrans_median if xtrans else ctx.demosaic_median_u16)(m, params, passes, clip=clip, orientation=o)
        elif clip is not None:
            out = (ctx.demosaic_xtrans_blend if xtrans else ctx.demosaic_blend_u16)(m, params, clip, orientation=o)
        else:
            out = (ctx.demosaic_xtrans if xtrans else ctx.demosaic_u16)(m, params, orientation=o)
        return out.cpu().numpy().view(np.uint16)

    def lens(self, picture, profile):
        image = torch.from_numpy(np.array(picture, dtype=np.float32)).cuda()
        return self.ctx.lens_correct(image, profile).permute(1, 2, 0).cpu().numpy()

    def composed(self, mosaic, profile, denoise, repair, lens_profile, keywords):
        proc = self.proc
        payload = proc.extract_image_data_cpu(np.array(mosaic), raw_profile=profile, raw_denoise=denoise, raw_repair=repair,
                                              lens_profile=lens_profile, **keywords)
        proc.prepare_gpu_textures(payload)  # the upload and _prepare_device_frame
        frame, layout, _ = proc._texture
        assert layout == "chw"
        window = payload["lens"]["window"]
        assert tuple(frame.shape) == (3, window[2], window[3])
        return frame.permute(1, 2, 0).cpu().numpy().astype(np.float64) / float(payload["u16_factor"]), window[:2]


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def backend(proc):
    return DeviceBackend(proc.ctx, proc)


_MEASURED = {}


def measured(name, backend):
    """camera_sim.measure of a check on the device, once."""
    if name not in _MEASURED:
        _MEASURED[name] = cs.measure(name, backend)
        print(name, _MEASURED[name])
    return _MEASURED[name]


def holds(name, backend):
    """The scene comes back under the correct reading and under no misreading: the file's threshold lies between."""
    m, threshold = measured(name, backend), GOLDEN[name]["threshold"]
    assert set(m["misreadings"]) == set(GOLDEN[name]["misreadings"])  # (none dropped)
    assert m["correct"] < threshold, (name, m["correct"], threshold)
    for wrong, err in m["misreadings"].items():
        assert err > threshold, (name, wrong, err, threshold)
    return m


def test_the_frames_are_small_and_ragged_against_the_tiles():
    assert cs.BAYER_SHAPE == (98, 150) and cs.XTRANS_SHAPE == (97, 149) and cs.LENS_SHAPE == (128, 160)
    assert all(s % 2 == 0 and s >= 64 for s in cs.BAYER_SHAPE)  # the denoise admits it
    assert cs.BAYER_SHAPE[1] % 64 and cs.BAYER_SHAPE[0] % 32 and cs.XTRANS_SHAPE[1] % 64 and cs.XTRANS_SHAPE[0] % 32
    assert cs.LENS_SHAPE[1] % 64


@pytest.mark.parametrize("name", ["bayer_full", "bayer_half", "bayer_half_centres", "xtrans_full", "xtrans_third", "xtrans_third_centres"])
def test_demosaic_returns_the_scene_at_full_and_reduced_size(backend, name):
    holds(name, backend)


@pytest.mark.parametrize("name", ["bayer_colour", "xtrans_colour"])
def test_multipliers_black_levels_and_matrix_return_the_scene(backend, name):
    holds(name, backend)


@pytest.mark.parametrize("name", [f"orientation_{o}" for o in range(8)] + ["xtrans_orientation_5"])
def test_a_mounted_sensor_comes_back_upright(backend, name):
    holds(name, backend)


@pytest.mark.parametrize("name", ["levels_nominal", "levels_adjusted"])
def test_raw_levels_bring_the_sensors_white_to_full_scale(backend, name):
    holds(name, backend)


@pytest.mark.parametrize("name", ["unclip", "blend_unsaturated"])
def test_unclip_and_blend_return_the_scene_at_their_normalisation(backend, name):
    holds(name, backend)


def test_blend_lowers_the_error_inside_a_saturated_patch(backend):
    figures = measured("blend_patch", backend)["figures"]
    assert figures["blend"] < figures["clip"], figures


@pytest.mark.parametrize("name", ["median_1", "median_4"])
def test_the_scene_still_returns_behind_the_median(backend, name):
    holds(name, backend)


def test_the_median_does_not_grow_the_colour_difference_error_of_a_noisy_frame(backend):
    figures = measured("median_noise", backend)["figures"]
    assert figures["passes_1"] <= figures["passes_0"] and figures["passes_4"] <= figures["passes_0"], figures


def test_the_denoise_lowers_the_error_and_keeps_the_mean(backend):
    m = holds("denoise", backend)
    assert m["correct"] < m["noisy"], m
    assert abs(m["bias"]) < GOLDEN["denoise"]["bias_bound"], m


@pytest.mark.parametrize("name", ["repair_bayer", "repair_xtrans"])
def test_the_repair_brings_a_frame_with_stuck_samples_back(backend, name):
    m = holds(name, backend)
    assert set(m["misreadings"]) == {"not_repaired"}  # below the threshold with the repair, above it without


@pytest.mark.parametrize("name", [f"lens_{n}" for n in cs.LENS_PROFILES])
def test_the_lens_step_undoes_the_simulated_lens(backend, name):
    holds(name, backend)


@pytest.mark.parametrize("name", ["composed_bayer", "composed_xtrans"])
def test_the_composed_pre_path_returns_the_scene_and_no_single_misreading_does(backend, proc, name):
    m = holds(name, backend)
    assert set(m["misreadings"]) >= {"cfa", "orientation", "levels", "white_balance", "repair", "black", "matrix", "lens_distortion", "lens_tca",
                                     "lens_vignetting"}
    # the last run was a lens misreading with everything else in place: the processor reports what ran
    assert proc.last_raw_scale["adjusted"] and proc.last_raw_repair["repaired"] > 0
    assert (proc.last_raw_denoise is None) == (name == "composed_xtrans")
