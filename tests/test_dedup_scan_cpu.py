"""The per-read routine written for a device de-duplication pass (compseed_amd/csrc/dedup_scan.hpp: both sorts over (key, index) records,
the event scan, the strip-wise banded global alignment) as a plain C++ program without a GPU (tests/cpp/dedup_scan_check.cpp).  In its
one-lane instantiation over the seven ddp1 sets and the aln2 sets it must leave the reference's own regions (tests/golden/ddp1, aln2) --
and, byte for byte, what the host cs_dedup_regions leaves.  Its 64-lane and 8-lane instantiations run on threads in lockstep (a ballot or
a shuffle is an exchange between two barriers): lanes that part ways never finish, and the ballots, the strips of the alignment and the
carry between them must give the same bytes.  A wrong tie order, float expression, band edge or event rule shows here before any kernel runs."""
import os
import subprocess

import numpy as np
import pytest

import _aln2
import _data
from test_dedup import SETS, _load

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dedup_scan") / "dedup_scan_check")
    src = os.path.join(HERE, "cpp", "dedup_scan_check.cpp")
    c = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off", "-o", out, src], capture_output=True, text=True)
    assert c.returncode == 0 and not c.stderr, c.stderr                      # (no warnings either)
    return out


@pytest.fixture(scope="module")
def lanes_exe(tmp_path_factory):
    """the same program with its N-lane instantiation on N lockstep threads, N = 64 and 8"""
    out = {}
    for n in (64, 8):
        out[n] = str(tmp_path_factory.mktemp("dedup_scan_%d" % n) / "dedup_scan_check")
        c = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off", "-pthread", "-DCS_EMU_W=%d" % n, "-o", out[n],
                            os.path.join(HERE, "cpp", "dedup_scan_check.cpp")], capture_output=True, text=True)
        assert c.returncode == 0 and not c.stderr, c.stderr
    return out


def _l_pac():
    return int(open(_data.PREFIX + ".ann").read().split()[0])


def _run(exe, d, reg_off, regs, bases, off, ap, dp):
    import compseed_amd as ca
    assert regs.dtype == ca.ALNREG_DT and regs.dtype.itemsize == 56
    l_pac = _l_pac()
    meta = np.array([off.size - 1, regs.size, l_pac, ap.a, ap.b, ap.o_del, ap.e_del, ap.o_ins, ap.e_ins, ap.w, dp.max_chain_gap,
                     int(np.array([dp.mask_level_redun], np.float32).view(np.uint32)[0])], np.int64)
    pac = np.fromfile(_data.PREFIX + ".pac", np.uint8)[:(l_pac + 3) // 4]
    for name, arr in (("meta", meta), ("reg_off", reg_off.astype(np.uint64)), ("regs", regs), ("read_off", off.astype(np.uint64)), ("bases", bases), ("pac", pac)):
        np.ascontiguousarray(arr).tofile(os.path.join(d, name + ".bin"))
    r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rd = lambda n, dt: np.fromfile(os.path.join(d, n + ".bin"), dt)
    return dict(reg_off=rd("out_off", np.uint64), regs=rd("out_regs", ca.ALNREG_DT), n_comp=rd("out_nc", np.int32)), rd("out_stat", np.uint64)


def _check(got, zd, host, what):
    assert np.array_equal(got["reg_off"], zd["reg_off"]), what
    for f in FIELDS:
        assert np.array_equal(got["regs"][f], zd["reg_" + f]), (what, f)
    assert np.array_equal(got["regs"]["frac_rep"].view(np.uint32), zd["reg_frac_rep"].view(np.uint32)), what
    assert np.array_equal(got["n_comp"], zd["reg_n_comp"]), what
    for k in ("reg_off", "regs", "n_comp"):
        assert got[k].tobytes() == host[k].tobytes(), (what, k)


@pytest.mark.parametrize("name", sorted(SETS))
def test_one_lane_routine_leaves_the_references_regions(exe, tmp_path, name):
    import compseed_amd as ca
    reg_off, regs, bases, off, zd = _load(name)
    al = ca.Aligner(_data.PREFIX, -1)
    host = al.dedup_regions(reg_off, regs, bases, off)
    al.close()
    got, stat = _run(exe, tmp_path, reg_off, regs, bases, off, ca.AlnParams(), ca.DedupParams())
    _check(got, zd, host, name)
    merged = int((zd["reg_n_comp"] > 1).sum())
    assert stat[0] >= stat[1] >= merged and (merged == 0 or stat[1] > 0), (name, stat.tolist(), merged)
    if name in ("gap3k", "long90", "ragged"):
        assert stat[0] > 0, name                                            # the alignment ran


@pytest.mark.parametrize("name", _aln2.SETS)
def test_one_lane_routine_on_the_aln2_sets(exe, tmp_path, name):
    import compseed_amd as ca
    reg_off, regs = _aln2.regions(_aln2.npz(name, "aln"))
    zd = _aln2.npz(name, "ddp")
    bases, off = _aln2.reads(name)
    ap = _aln2.aln_params(name)
    al = ca.Aligner(_data.PREFIX, -1, ap)
    host = al.dedup_regions(reg_off, regs, bases, off)
    al.close()
    got, _ = _run(exe, tmp_path, reg_off, regs, bases, off, ap, ca.DedupParams())
    _check(got, zd, host, name)


@pytest.mark.parametrize("lanes,name", [(64, "main100"), (64, "sorted150"), (8, "sorted150"), (8, "ragged")])
def test_many_lane_routine_in_lockstep(exe, lanes_exe, tmp_path, lanes, name):
    """the wave's code path: several candidates per step and one ballot (main100, ragged: reads of up to 63 and 500 live regions), the
    patch alignment in strips with the carry between them (sorted150: one alignment, ragged: eight); the same bytes and the same
    alignment and merge counts as one lane"""
    import compseed_amd as ca
    reg_off, regs, bases, off, zd = _load(name)
    al = ca.Aligner(_data.PREFIX, -1)
    host = al.dedup_regions(reg_off, regs, bases, off)
    al.close()
    (tmp_path / "one").mkdir(); (tmp_path / "many").mkdir()
    one, stat1 = _run(exe, tmp_path / "one", reg_off, regs, bases, off, ca.AlnParams(), ca.DedupParams())
    got, stat = _run(lanes_exe[lanes], tmp_path / "many", reg_off, regs, bases, off, ca.AlnParams(), ca.DedupParams())
    _check(got, zd, host, (name, lanes))
    assert stat.tolist() == stat1.tolist() and (name == "main100" or stat[0] > 0), (name, lanes, stat.tolist(), stat1.tolist())
