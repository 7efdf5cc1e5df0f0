"""The arithmetic of the backward kernels' single-child extension without a GPU (tests/cpp/occ_math_check.cpp over
compseed_amd/csrc/occ_math.hpp, which extend1b of fm_device.hpp calls): counting the bases of a 32-byte record up to every row against a
count made base by base, and child c of a bi-interval for every pair of positions k < l of a 192-row BWT, every child, both directions
and the sentinel at every position, with record counts that pass 2^32 inside the text, against the child assembled from naive Occ counts
by the cascade extend4 states.  About 30 million cases per seed, a few seconds."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "occ_math_check.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("occ_math") / "occ_math_check")
    c = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", out, SRC], capture_output=True, text=True)
    assert c.returncode == 0 and not c.stderr, c.stderr                      # (no warnings either)
    return out


def test_counting_equals_the_count_base_by_base(exe):
    r = subprocess.run([exe, "count"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok count"), r.stdout + r.stderr
    assert int(r.stdout.split()[2]) == 64 * 4004, r.stdout


@pytest.mark.parametrize("seed", [1, 2])
def test_child_equals_the_cascade_over_naive_counts(exe, seed):
    r = subprocess.run([exe, "child", str(seed)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok child"), r.stdout + r.stderr
    print(r.stdout.strip())
    assert int(r.stdout.split()[2]) > 25_000_000, r.stdout
