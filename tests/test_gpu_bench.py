"""bench.py end to end on one GPU, at a small size of configs[1] (1,500 points): a plain run prints the
headline line only and --dump-outputs writes the last timed step's arrays; --full adds the roofline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = 1500
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "cfg2", "--points", str(POINTS)]


def _bench(extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    d = tmp_path / "dump"
    res = _bench(["--dump-outputs", str(d)])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["dtype"] == "fp32" and res["unit"] == "points/s"
    assert res["higher_is_better"] is True and res["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: points of one step / time of one step
    assert res["value"] == pytest.approx(POINTS / (res["ms_per_step"] * 1e-3), rel=1e-3)
    for k in ("roofline", "bf16_mode", "cpu_baseline"):
        assert k not in res
    assert sorted(os.listdir(d)) == ["grads.npy", "loss.npy", "out.npy", "params.npy"]
    arr = {n: np.load(d / (n + ".npy")) for n in ("out", "loss", "grads", "params")}
    assert all(a.dtype == np.float32 and a.ndim == 1 and np.isfinite(a).all() for a in arr.values())
    assert arr["out"].shape == (POINTS,) and arr["loss"].shape == (1,) and arr["loss"][0] > 0
    assert arr["grads"].shape == arr["params"].shape and arr["grads"].size > 100000
    assert np.abs(arr["grads"]).max() > 0
    assert sum(a.nbytes for a in arr.values()) <= 64e6


@pytest.mark.gpu
def test_full_run_adds_the_roofline():
    res = _bench(["--full", "--fp32-only", "--no-cpu-baseline"])
    assert res["steps"] == 3 and res["ms_per_step"] > 0
    assert res["roofline"]["class"] in res["roofline"]["class_ms_per_step"] and res["roofline"]["launches"] > 0
