"""The lane sets of bwd_win_kernel's dispenser without a GPU (tests/cpp/lane_sets_check.cpp): the mask arithmetic of
compseed_amd/csrc/lane_sets.hpp -- the w lowest free lanes, a lane's rank in its set, the next higher member, release -- against naive
loops for every width and over full, empty, alternating, top-bits-only and random masks, and a lane-by-lane model of the dispenser as
smem_bwd.hpp writes it (one free mask, calls of 19..64 lanes in queue order, 64 slots a draw, lanes returned at a call's end or, with
early release, as soon as they cannot matter): every call placed once and in order, no lane in two calls, the free mask always the
complement of what the calls hold, and the wave reaches its exit."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "lane_sets_check.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lane_sets") / "lane_sets_check")
    c = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", out, SRC], capture_output=True, text=True)
    assert c.returncode == 0 and not c.stderr, c.stderr                      # (no warnings either)
    return out


def test_helpers_equal_the_naive_loops(exe):
    r = subprocess.run([exe, "helpers"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok helpers"), r.stdout + r.stderr


@pytest.mark.parametrize("early", [0, 1], ids=["release_at_end", "early_release"])
@pytest.mark.parametrize("seed,n_calls", [(1, 1), (2, 3), (3, 65), (4, 500), (5, 3000)])
def test_model_places_every_call_once(exe, seed, n_calls, early):
    r = subprocess.run([exe, "model", str(seed), str(n_calls), str(early)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok model"), r.stdout + r.stderr
    print(r.stdout.strip())
    if n_calls >= 500:                                                      # the sets do get packed: three calls or more share the wave
        assert int(r.stdout.split("up to ")[1].split()[0]) >= (3 if early else 2), r.stdout
