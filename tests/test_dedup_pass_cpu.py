"""The whole device de-duplication pass without a GPU (tests/cpp/dedup_pass_check.cpp): the bodies that its kernels loop over
(compseed_amd/csrc/dedup_pass.hpp, compact.hpp; the kernels themselves are not in the library) driven by a plain
C++ program in the kernels' order -- check, light reads, heavy reads, keep flags, scan, scatter, offsets -- over batch-sized lists at the reads' input offsets and
with both placements of the patch alignment's rows.  Byte for byte the host cs_dedup_regions and the reference's goldens: one lane over
the seven ddp1 sets and the aln2 sets, 64 and 8 lanes on lockstep threads over the sets the existing lockstep test uses.  The check body
must refuse every class of inconsistent input before anything follows an offset (one hand-made case each, from sorted150)."""
import os
import subprocess

import numpy as np
import pytest

import _aln2
import _data
from test_dedup import SETS, _load
from test_dedup_scan_cpu import _check, _l_pac

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "dedup_pass_check.cpp")
MAX_READ_LEN = 65536


def _build(out, *defs):
    c = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off", "-pthread", *defs, "-o", out, SRC], capture_output=True, text=True)
    assert c.returncode == 0 and not c.stderr, c.stderr                      # (no warnings either)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("dedup_pass") / "dedup_pass_check"))


@pytest.fixture(scope="module")
def lanes_exe(tmp_path_factory):
    return {n: _build(str(tmp_path_factory.mktemp("dedup_pass_%d" % n) / "dedup_pass_check"), "-DCS_EMU_W=%d" % n) for n in (64, 8)}


def _write(d, reg_off, regs, bases, off, ap, dp):
    import compseed_amd as ca
    assert regs.dtype == ca.ALNREG_DT and regs.dtype.itemsize == 56
    l_pac = _l_pac()
    meta = np.array([off.size - 1, regs.size, l_pac, ap.a, ap.b, ap.o_del, ap.e_del, ap.o_ins, ap.e_ins, ap.w, dp.max_chain_gap,
                     int(np.array([dp.mask_level_redun], np.float32).view(np.uint32)[0])], np.int64)
    pac = np.fromfile(_data.PREFIX + ".pac", np.uint8)[:(l_pac + 3) // 4]
    for name, arr in (("meta", meta), ("reg_off", reg_off.astype(np.uint64)), ("regs", regs), ("read_off", off.astype(np.uint64)), ("bases", bases), ("pac", pac)):
        np.ascontiguousarray(arr).tofile(os.path.join(d, name + ".bin"))


def _run(exe, d, reg_off, regs, bases, off, ap, dp, lds_rows=None):
    import compseed_amd as ca
    os.makedirs(d, exist_ok=True)
    _write(d, reg_off, regs, bases, off, ap, dp)
    r = subprocess.run([exe, str(d)] + ([] if lds_rows is None else [str(lds_rows)]), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rd = lambda n, dt: np.fromfile(os.path.join(d, n + ".bin"), dt)
    return dict(reg_off=rd("out_off", np.uint64), regs=rd("out_regs", ca.ALNREG_DT), n_comp=rd("out_nc", np.int32)), rd("out_stat", np.uint64)


def _heavy_reads(reg_off, regs):
    live = np.concatenate([[0], np.cumsum(regs["qe"] > regs["qb"])])
    return int((live[reg_off[1:].astype(np.int64)] - live[reg_off[:-1].astype(np.int64)] >= 2).sum())


def _host(reg_off, regs, bases, off, ap=None):
    import compseed_amd as ca
    al = ca.Aligner(_data.PREFIX, -1, ap)
    host = al.dedup_regions(reg_off, regs, bases, off)
    al.close()
    return host


def _stat_ok(stat, zd, reg_off, regs, what):
    merged = int((zd["reg_n_comp"] > 1).sum())
    assert stat[0] >= stat[1] >= merged, (what, stat.tolist(), merged)
    assert stat[2] == _heavy_reads(reg_off, regs) and stat[3] == zd["reg_rb"].size, (what, stat.tolist())


@pytest.mark.parametrize("name", sorted(SETS))
def test_one_lane_pass_leaves_the_references_regions(exe, tmp_path, name):
    import compseed_amd as ca
    reg_off, regs, bases, off, zd = _load(name)
    got, stat = _run(exe, tmp_path, reg_off, regs, bases, off, ca.AlnParams(), ca.DedupParams())
    _check(got, zd, _host(reg_off, regs, bases, off), name)
    _stat_ok(stat, zd, reg_off, regs, name)


@pytest.mark.parametrize("name", _aln2.SETS)
def test_one_lane_pass_on_the_aln2_sets(exe, tmp_path, name):
    import compseed_amd as ca
    reg_off, regs = _aln2.regions(_aln2.npz(name, "aln"))
    zd = _aln2.npz(name, "ddp")
    bases, off = _aln2.reads(name)
    ap = _aln2.aln_params(name)
    got, stat = _run(exe, tmp_path, reg_off, regs, bases, off, ap, ca.DedupParams())
    _check(got, zd, _host(reg_off, regs, bases, off, ap), name)
    _stat_ok(stat, zd, reg_off, regs, name)


@pytest.mark.parametrize("name", ["long90", "ragged"])
def test_both_row_placements_give_the_same_bytes(exe, tmp_path, name):
    """long90's patches span 800 to 1,500 read bases and ragged's up to a few hundred: with 2 x 1,025 (the device's) resp. 2 x 200 words of
    small rows some alignments fit and some do not (gap3k's all go beyond 1,025: its test above covers that); with none (0) all go to
    the large rows"""
    import compseed_amd as ca
    reg_off, regs, bases, off, zd = _load(name)
    host = _host(reg_off, regs, bases, off)
    rows = {"long90": 1025, "ragged": 200}[name]
    got, stat = _run(exe, tmp_path / "mixed", reg_off, regs, bases, off, ca.AlnParams(), ca.DedupParams(), rows)
    _check(got, zd, host, (name, rows))
    assert stat[4] > 0 and stat[5] > 0, (name, stat.tolist())                # both placements occurred
    got0, stat0 = _run(exe, tmp_path / "hbm", reg_off, regs, bases, off, ca.AlnParams(), ca.DedupParams(), 0)
    _check(got0, zd, host, (name, 0))
    assert stat0[4] == 0 and stat0[5] > 0 and stat0[:4].tolist() == stat[:4].tolist(), (name, stat0.tolist(), stat.tolist())


@pytest.mark.parametrize("lanes,name", [(64, "main100"), (64, "sorted150"), (8, "ragged")])
def test_many_lane_pass_in_lockstep(exe, lanes_exe, tmp_path, lanes, name):
    """the wave kernel's instantiation on lockstep threads, inside the whole pass: the same bytes and the same counters as one lane"""
    import compseed_amd as ca
    reg_off, regs, bases, off, zd = _load(name)
    host = _host(reg_off, regs, bases, off)
    rows = 200 if name == "ragged" else None
    one, stat1 = _run(exe, tmp_path / "one", reg_off, regs, bases, off, ca.AlnParams(), ca.DedupParams(), rows)
    got, stat = _run(lanes_exe[lanes], tmp_path / "many", reg_off, regs, bases, off, ca.AlnParams(), ca.DedupParams(), rows)
    _check(got, zd, host, (name, lanes))
    assert stat.tolist() == stat1.tolist() and (name == "main100" or stat[0] > 0), (name, lanes, stat.tolist(), stat1.tolist())


def _bad_cases():
    """name -> a function that spoils (reg_off, regs, bases, off) of sorted150 in one way; l_pac is passed in"""
    def first_live(reg_off, regs):
        return int(np.flatnonzero(regs["qe"] > regs["qb"])[0])

    def reg(field, value):
        def f(reg_off, regs, bases, off, l_pac):
            g = first_live(reg_off, regs)
            regs[field][g] = value(regs[g], l_pac) if callable(value) else value
            return reg_off, regs, bases, off
        return f

    def offs(which, i, value):
        def f(reg_off, regs, bases, off, l_pac):
            arr = reg_off if which == "reg" else off
            arr[i] = value(arr) if callable(value) else value
            return reg_off, regs, bases, off
        return f

    def long_read(reg_off, regs, bases, off, l_pac):
        r = int(np.flatnonzero(np.diff(reg_off.astype(np.int64)) > 0)[-1])     # the last read with regions: 65,536 bases
        grow = MAX_READ_LEN - int(off[r + 1] - off[r])
        off[r + 1:] += np.uint64(grow)
        return reg_off, regs, np.concatenate([bases, np.zeros(grow, np.uint8)]), off

    mid = 40
    return {
        "reg_off_decreases": offs("reg", mid, lambda a: a[mid + 1] + np.uint64(1)),
        "reg_off_not_from_0": offs("reg", 0, 1),
        "reg_off_not_to_n_regs": offs("reg", -1, lambda a: a[-1] - np.uint64(1)),
        "reg_off_beyond_n_regs": offs("reg", -1, lambda a: a[-1] + np.uint64(1)),
        "read_off_not_from_0": offs("read", 0, 1),
        "read_off_decreases": offs("read", mid, lambda a: a[mid - 1] - np.uint64(1)),
        "read_of_65536_bases": long_read,
        "qb_negative": reg("qb", -1),
        "qe_beyond_the_read": reg("qe", 151),
        "rb_negative": reg("rb", -1),
        "re_not_beyond_rb": reg("re", lambda x, l_pac: x["rb"]),
        "re_beyond_the_reference": reg("re", lambda x, l_pac: 2 * l_pac + 1),
        "span_beyond_131072": reg("re", lambda x, l_pac: x["rb"] + 2 * MAX_READ_LEN + 1),
    }


@pytest.mark.parametrize("case", sorted(_bad_cases()))
def test_check_body_refuses_inconsistent_input(exe, tmp_path, case):
    import compseed_amd as ca
    reg_off, regs, bases, off, _ = _load("sorted150")
    assert np.diff(off.astype(np.int64)).max() == 150
    args = _bad_cases()[case](reg_off.astype(np.uint64).copy(), regs.copy(), bases.copy(), off.astype(np.uint64).copy(), _l_pac())
    _write(tmp_path, *args, ca.AlnParams(), ca.DedupParams())
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and "refused" in r.stderr, (case, r.returncode, r.stderr)
    assert not os.path.exists(os.path.join(tmp_path, "out_off.bin"))


def test_check_body_accepts_what_the_pass_drops(exe, tmp_path):
    """a purged region (qe <= qb) is dropped whatever it holds, and a read without regions may be of any length"""
    import compseed_amd as ca
    reg_off, regs, bases, off, zd = _load("sorted150")
    regs = regs.copy()
    dead = np.flatnonzero(regs["qe"] <= regs["qb"])
    assert dead.size
    regs["rb"][dead[0]] = -5; regs["re"][dead[0]] = -7
    got, _ = _run(exe, tmp_path, reg_off, regs, bases, off, ca.AlnParams(), ca.DedupParams())
    _check(got, zd, _host(reg_off, regs, bases, off), "sorted150")
