"""Settling an end of bwd_win_kernel's wave loop at the moment it stops (smem_bwd.hpp, CS_WIN_SETTLE), without a GPU
(tests/cpp/win_settle_check.cpp): the mask arithmetic compseed_amd/csrc/lane_sets.hpp adds for it -- the valid ends above a lane that stop
in this iteration, the lane it reads s from, who reports, who carries the s on, what returns to the free mask, when the lanes that wait to
report are flushed -- against naive loops over full, empty, alternating, top-only and random masks, and a lane-by-lane model of the wave
loop on synthetic calls (1..46 stored LEPs, random subsets of valid window ends, stop positions that never rise as the end gets shorter,
ties, equal-size stops, ends shorter than min_seed_len) that runs the same queue with the rule applied at the call's end and settled at
the stop: the same reports for every call, every lane back in the free mask exactly once, the free mask always the complement of what
calls and pending lanes hold, calls of 64 lanes placed, the wave at its exit, and more calls sharing the wave than before."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "win_settle_check.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("win_settle") / "win_settle_check")
    c = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", out, SRC], capture_output=True, text=True)
    assert c.returncode == 0 and not c.stderr, c.stderr                      # (no warnings either)
    return out


def test_helpers_equal_the_naive_loops(exe):
    r = subprocess.run([exe, "helpers"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok helpers"), r.stdout + r.stderr


@pytest.mark.parametrize("seed,n_calls", [(1, 1), (2, 3), (3, 65), (4, 500), (5, 3000)])
def test_settled_at_the_stop_reports_what_the_call_end_rule_reports(exe, seed, n_calls):
    r = subprocess.run([exe, "model", str(seed), str(n_calls)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok model"), r.stdout + r.stderr
    print(r.stdout.strip())
    if n_calls >= 65:                                                       # lanes come back sooner: fewer iterations, more calls a wave
        it0, it1 = map(int, re.search(r"iterations (\d+) -> (\d+)", r.stdout).groups())
        c0, c1 = map(float, re.search(r"calls per iteration ([\d.]+) -> ([\d.]+)", r.stdout).groups())
        assert it1 < it0 and c1 > c0, r.stdout
