"""bench.py's plain run: the headline line and nothing else, and --dump-outputs, whose arrays must be the same from run to run (the
inputs depend on the arguments only, not on the number of steps)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("parity", "roofline", "cpu_baseline", "pcie_inclusive", "reads_per_s_incl_pcie", "one_step_at_a_time", "workloads", "extension")


def _plain(out_dir, steps=3):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--genome-mbp", "200",
           "--reads", "300000", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    j = _plain(a, steps=3)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in j
    assert j["steps"] == 3 and j["unit"] == "reads/s" and j["higher_is_better"] is True and j["value"] > 0
    assert abs(j["value"] - 300000 / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
    assert not any(k in j for k in FULL_ONLY)

    names = sorted(os.listdir(a))
    assert names == ["digest.npy", "mem_off.npy", "mems.npy", "read_ids.npy", "seed_off.npy", "seeds.npy", "totals.npy"]
    assert sum(os.path.getsize(a / n) for n in names) <= 64 << 20
    d = {n[:-4]: np.load(a / n) for n in names}
    assert all(x.dtype == np.float64 for x in d.values())
    assert d["totals"][0] == 300000 and d["totals"][1] > 0 and d["totals"][2] > 0
    n = d["read_ids"].size
    assert n > 1000 and d["mem_off"].size == n + 1 and d["mems"].shape == (int(d["mem_off"][-1]), 4)
    assert d["seed_off"].size == n + 1 and d["seeds"].shape == (int(d["seed_off"][-1]), 3)

    _plain(b, steps=2)   # another process, another number of steps: the same outputs
    assert [nm for nm in names if not np.array_equal(np.load(a / nm), np.load(b / nm))] == []


def test_steps_must_be_positive():
    """argument check, before anything touches a GPU"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr
