"""bench.py's JSON line: the keys and types the driver and the judge read (the measurement contract), on the headline
configuration with a short CPU-baseline sample."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_bench_line_carries_the_contract_fields():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--cpu-seconds", "3", "--no-alone"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "exactly ONE JSON line on stdout"
    d = json.loads(lines[0])
    for key, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                     ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str),
                     ("config", dict), ("roofline", dict), ("cpu_baseline", dict)):
        assert isinstance(d[key], typ), key
    assert "vs_baseline" in d and d["vs_baseline"] is None  # BASELINE.md holds no published number for this metric
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 2 and d["unit"] == "MP/s" and d["higher_is_better"] is True
    assert "100MP" in d["metric"].replace(" ", "") or "100 MP" in d["metric"]
    assert d["config"]["workload"].startswith("cfg4_100mp") and "model" not in d["config"]
    # value = whole-job throughput: the frame's megapixels over the step time
    assert d["value"] == pytest.approx(12288 * 8192 / 1e6 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and "traffic" in r
    assert r["peak"] == 8000.0 and r["frac"] == pytest.approx(r["achieved"] / r["peak"])
    assert r["achieved"] == pytest.approx(24.0 * 12288 * 8192 / (d["ms_per_step"] * 1e-3) / 1e9, rel=1e-6)  # 24 B/px
    if r["traffic"] is not None:  # only from a capture of these very sources
        assert r["traffic_provenance"]["match"] is True and r["traffic"] > 24.0 * 12288 * 8192
    k = r["dominant_kernel"]
    assert k["bound"] == "hbm" and 0.0 < k["frac"] < 1.0 and k["kernel_ms"] > 0
    assert "fft_cols_walk_kernel" in k["kernel"] or "tail_kernel" in k["kernel"]  # (the largest per-step class of the two: run dependent)
    # the headline frame's exposure spans max / min = 1.4e5: beyond the 12-byte element's guard (6.2e4 with the stand-in Portra curve:
    # the searched constant) -- but the choice is made per WINDOW PAIR, and a window of the noise frame spans ~2e4: nearly every pair
    # takes the element; and the eager stage-by-stage steps behind the breakdown made the same choices from the same record
    e = r["halation_scratch_element"]
    assert e["armed"] and 0 < e["min"] < 1e-2 and 10 < e["max_abs"] < 1e3 and 3e4 < e["bound"] < 1e5
    assert e["max_abs"] > e["bound"] * max(e["min"], e["floor"])
    assert e["pairs"] > 500 and 0.9 * e["pairs"] <= e["packed_pairs"] <= e["pairs"]
    assert e["eager_breakdown_took_the_same_element"] is True
    if "fft_cols_walk_kernel" in k["kernel"]:
        assert "fft_cols_walk_kernel<32, 3>" in k["kernel"] or "fft_cols_walk_kernel<32, 1>" in k["kernel"]  # instances the timed steps launch
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "MP/s" and c["cores"] >= 1 and c["value"] > 0 and isinstance(c["sample"], str)
    assert d["value"] / c["value"] > 100  # a reported ratio, not the target -- but the GPU path must not be the CPU path


def test_dump_outputs_hold_the_last_timed_step_and_repeat(tmp_path):
    """--dump-outputs: rows of what the LAST timed step handed its caller, float32, within 64 MB, the same from run to run with the
    same arguments.  cfg3_45mp draws a new grain seed every frame, so the rows are checked against the frame rendered here with
    that step's seed (2 warm-up frames -- the graph is captured on the second -- then 2 timed ones: GRAIN_SEED + 4)."""
    import numpy as np
    import torch

    from raw2film_amd import HipProcessor, filmstock
    from raw2film_amd.synthetic import CONFIGS, synthetic_frame_device

    args = ["--config", "cfg3_45mp", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-breakdown", "--no-pcie", "--no-alone"]
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-2000:]
        assert sum(f.stat().st_size for f in d.glob("*.npy")) <= 64 << 20
        dumps.append({f.stem: np.load(f) for f in d.glob("*.npy")})
    assert sorted(dumps[0]) == sorted(dumps[1]) == ["output_rows", "output_rows_index"]
    for k in dumps[0]:
        np.testing.assert_array_equal(dumps[0][k], dumps[1][k])
    W, H = CONFIGS["cfg3_45mp"]
    rows, idx = dumps[0]["output_rows"], dumps[0]["output_rows_index"].astype(np.int64)
    assert rows.dtype == np.float32 and rows.shape == (len(idx), W, 3) and idx[0] == 0 and idx[-1] == H - 1 and len(idx) < H

    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    settings = dict(print_film=prt, frame_width=36, frame_height=24, exp_kelvin=6000, color_masking=1.0, halation=True, halation_size=1.0,
                    halation_green_factor=0.3, halation_intensity=1.0, sharpness=True, sharpening_strength=0.0, grain=2)  # bench.py's
    frame = synthetic_frame_device(H, W, seed=1234, device="cuda:0")
    proc = HipProcessor(device=0)
    want = proc.process_array(frame, neg, 6, 0.4, colorspace="linear-rec709", seed=20260630 + 4, return_float=True, output="device",
                              **settings)
    np.testing.assert_array_equal(rows, want[torch.as_tensor(idx, device=want.device)].cpu().numpy())
    proc.close()
