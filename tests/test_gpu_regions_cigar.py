"""cs_regions_cigar on the GPU: from regions to CIGAR, NM and MD (cigar_gpu.hip: the bodies of cigar_scan.hpp as kernels).  Over the
reference's own regions the result must be, byte for byte, what the plain C++ program (tests/cpp/cigar_scan_check.cpp, the same bodies on
one CPU lane) gives for every region -- which tests/test_cigar_scan_cpu.py holds against the reference's SAM, and which is checked against
it here again.  The sets are the smallest that reach each path: main100 (no-DP and small-band jobs, both strands), indel150_400 (every
job a DP, one strip), long90 (strips and the carry, H / E beyond the LDS rows: reads of up to 1,500 bases against 1,025 rows), gap3k (3-kb
spans, wide bands; again with the scratch budget forced small, so that the jobs take many chunks), ends (contig edges, the join, reverse
strand positions), params.odei / params.oied (asymmetric penalties, w of 7 and 5).  No golden set reaches a second try with a doubled
band (where the reference goes round again its band is 0 and stays 0), so the retries run on regions whose truesc is raised by hand:
there the only yardstick is the CPU program running the same next_try, which is a check of the kernels' plumbing (the flags, the second
and third pass, what a job keeps), not of the rule."""
import numpy as np
import pytest

import _cigar
import _data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _cigar.build(str(tmp_path_factory.mktemp("cigar_scan_gpu") / "cigar_scan_check"))


def _gpu(name, reg_off, regs, bases, off, flags=0):
    import compseed_amd as ca
    al = ca.Aligner(_data.PREFIX, 0, _cigar.aln_params(name))
    try:
        res = al.regions_cigar(reg_off, regs, bases, off, flags)
        st = al.cigar_stats()
    finally:
        al.close()
    return res, st


def _same(got, want, what, raw=True):
    if raw:
        for k in ("alns", "cigar", "md"):
            assert got[k].tobytes() == want[k].tobytes(), (what, k)
    assert _cigar.per_region(got) == _cigar.per_region(want), what


@pytest.mark.parametrize("name", ["main100", "indel150_400", "long90", "gap3k", "ends", "params.odei", "params.oied"])
def test_regions_cigar_is_the_cpu_programs_and_the_references(exe, tmp_path, name):
    reg_off, regs, bases, off, _ = _cigar.load(name)
    want = _cigar.run(exe, tmp_path, reg_off, regs, bases, off, _cigar.aln_params(name))
    got, st = _gpu(name, reg_off, regs, bases, off)
    _cigar.check_layout(got, regs.size)
    _same(got, want, name)
    _cigar.check_against_sam(name, got)
    w = want["stat"]
    assert (st["regions"], st["dp_jobs"], st["nodp_jobs"], st["retries"], st["rejected"], st["cells"]) == (regs.size, w["dp_jobs"], w["nodp_jobs"], w["retries"], 0, w["cells"]), (st, w)
    assert st["launches"] > 0 and st["kernel_ms"] > 0


def test_small_scratch_takes_many_chunks_and_changes_no_alignment(exe, tmp_path):
    import compseed_amd.binding as b
    reg_off, regs, bases, off, _ = _cigar.load("gap3k")
    want = _cigar.run(exe, tmp_path, reg_off, regs, bases, off, _cigar.aln_params("gap3k"), budget=64 << 10)
    assert want["stat"]["chunks"] > 10
    got, st = _gpu("gap3k", reg_off, regs, bases, off, b.CIGAR_SMALL_SCRATCH)
    _cigar.check_layout(got, regs.size)
    _same(got, want, "gap3k small scratch")
    plain, st0 = _gpu("gap3k", reg_off, regs, bases, off)
    assert st["launches"] > st0["launches"] + 20                             # three kernels a chunk
    _same(got, plain, "gap3k small scratch vs default", raw=False)


def test_retries_on_made_up_truesc_take_a_second_and_third_pass(exe, tmp_path):
    reg_off, regs, bases, off = _cigar.subset("params.odei", 1, 0, first_reads=17)
    regs["truesc"] += 60                                                     # the regions claim more than their alignment gives: the band doubles
    want = _cigar.run(exe, tmp_path, reg_off, regs, bases, off, _cigar.aln_params("params.odei"))
    got, st = _gpu("params.odei", reg_off, regs, bases, off)
    _same(got, want, "retries")
    assert st["retries"] > 0 and st["retries"] == want["stat"]["retries"] and got["alns"]["tries"].max() >= 2


def test_empty_results_rejection_and_errors(exe, tmp_path):
    import compseed_amd as ca
    reg_off, regs, bases, off, _ = _cigar.load("main100")
    l_pac, _ = _cigar.contigs()
    n = int(reg_off[40])
    regs = regs[:n].copy(); reg_off = reg_off[:41].copy(); bases = bases[:int(off[40])].copy(); off = off[:41].copy()
    al = ca.Aligner(_data.PREFIX, 0)
    try:
        first = al.regions_cigar(reg_off, regs, bases, off)
        want = _cigar.run(exe, tmp_path / "a", reg_off, regs, bases, off, ca.AlnParams())
        _same(first, want, "first call")
        _same(al.regions_cigar(reg_off, regs, bases, off), want, "second call")          # two calls in a row
        empty = al.regions_cigar(reg_off[:1], regs[:0], bases[:0], off[:1])
        assert empty["alns"].size == 0 and empty["cigar"].size == 0 and empty["md"].tobytes() == b"\0"
        none = al.regions_cigar(np.zeros(41, np.uint64), regs[:0], bases, off)               # reads without regions
        assert none["alns"].size == 0 and none["md"].tobytes() == b"\0"
        bad = regs.copy()
        bad["qe"][1] = bad["qb"][1]                                          # purged
        bad["rb"][2] = -1                                                    # unmapped
        bad["re"][3] = -5
        res = al.regions_cigar(reg_off, bad, bases, off)
        _same(res, _cigar.run(exe, tmp_path / "b", reg_off, bad, bases, off, ca.AlnParams()), "purged and unmapped")
        rows = _cigar.per_region(res)
        assert all(rows[g] == (-1, -1, 0, 0, 0, 0, 0, (), b"") for g in (1, 2, 3))
        fwd = int(np.flatnonzero(bad["re"] <= l_pac)[5])
        bad["rb"][fwd] = l_pac - 40; bad["re"][fwd] = l_pac - 40 + (bad["qe"][fwd] - bad["qb"][fwd])   # bridges the strands
        with pytest.raises(ca.CSError) as ei:
            al.regions_cigar(reg_off, bad, bases, off)
        assert ei.value.code == -1 and ei.value.result is not None           # CS_EINVAL after the others were delivered
        _same(ei.value.result, _cigar.run(exe, tmp_path / "c", reg_off, bad, bases, off, ca.AlnParams()), "rejected")
        assert _cigar.per_region(ei.value.result)[fwd] == (-1, -1, 0, 0, -1, 0, 0, (), b"")
        assert al.cigar_stats()["rejected"] == 1
        # the error list: unknown flags, inconsistent offsets, a region outside its read -- each found before any kernel follows an offset
        for args in ((reg_off, regs, bases, off, 2),):
            with pytest.raises(ca.CSError) as ei:
                al.regions_cigar(*args)
            assert ei.value.code == -1
        x = reg_off.copy(); x[5] = x[7]
        y = reg_off.copy(); y[-1] += 1
        z = off.copy(); z[9] = z[8] - 1
        far = regs.copy(); far["qe"][7] = 30000
        out = regs.copy(); out["re"][9] = 2 * l_pac + 5
        for ro, rg, of in ((x, regs, off), (y, regs, off), (reg_off, regs, z), (reg_off, far, off), (reg_off, out, off)):
            with pytest.raises(ca.CSError) as ei:
                al.regions_cigar(ro, rg, bases, of)
            assert ei.value.code == -1
        _same(al.regions_cigar(reg_off, regs, bases, off), want, "after the errors")      # the aligner is usable afterwards
    finally:
        al.close()
    host = ca.Aligner(_data.PREFIX, -1)
    try:
        with pytest.raises(ca.CSError) as ei:
            host.regions_cigar(reg_off, regs, bases, off)
        assert ei.value.code == -4                                           # CS_EDEVICE
        assert host.cigar_stats()["regions"] == 0
    finally:
        host.close()
