"""cs_regions_mark on the GPU: primary marking, MAPQ, SAM line selection and XA membership (mark_gpu.hip: the bodies of mark_scan.hpp as
kernels).  Over the reference's own regions the result must be, byte for byte, what the plain C++ program (tests/cpp/mark_scan_check.cpp,
the same bodies on one CPU lane) gives -- which tests/test_mark_scan_cpu.py holds against the reference's SAM lines, and which is held
against them here again.  The sets are the smallest that reach each path: main100 (the lane-per-read path: 3,000 reads of a few regions),
repeat100 (the wave path, lists in LDS, up to 501 regions a read), ragged (reads without regions, unmapped reads), long90 and ends (0x800
lines, the MAPQ cap), gap3k, params.a2 (T = 60, the sub_n threshold from a + b), params.oied (from o_ins + e_ins), alt.main100 (the ALT
branch, on an index with an .alt file).  A z of several ballot steps exists in no golden set: it runs on _mark.tiled_read's made-up read,
against the CPU program and the rule itself."""
import numpy as np
import pytest

import _cigar
import _data
import _mark

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _mark.build(str(tmp_path_factory.mktemp("mark_scan_gpu") / "mark_scan_check"))


@pytest.fixture(scope="module")
def alt_prefix(tmp_path_factory):
    return _mark.alt_prefix(tmp_path_factory.mktemp("alt_index"))


def _gpu(name, flags=0, arrays=None, prefix=None, **kw):
    import compseed_amd as ca
    reg_off, regs, off = arrays if arrays is not None else (_mark.load(name)[0], _mark.load(name)[1], _mark.load(name)[3])
    al = ca.Aligner(prefix or _data.PREFIX, 0, _cigar.aln_params(name) if name != _mark.ALT else None)
    try:
        res = al.regions_mark(reg_off, regs, off, ca.MarkParams(**_mark.mark_params(name)), flags=flags, **kw)
        st = al.mark_stats()
    finally:
        al.close()
    return res, st


@pytest.mark.parametrize("name,flags", [("main100", _mark.ALL), ("main100", 0), ("repeat100", _mark.ALL), ("repeat100", 0), ("long90", _mark.ALL), ("long90", 0), ("ragged", _mark.ALL),
                                        ("ends", _mark.ALL), ("gap3k", _mark.ALL), ("params.a2", _mark.ALL), ("params.oied", _mark.ALL), (_mark.ALT, _mark.ALL), (_mark.ALT, 0)])
def test_regions_mark_is_the_cpu_programs_and_the_references(exe, alt_prefix, tmp_path, name, flags):
    want = _mark.run(exe, tmp_path, name, flags)
    got, st = _gpu(name, flags, prefix=alt_prefix if name == _mark.ALT else None)
    _mark.same_bytes(got, want, (name, flags))
    _mark.check_properties(name, got)
    mode = "all" if flags & _mark.ALL else "def"
    assert _mark.check_lines(name, got, mode) == _mark.MANIFEST["sets"][name][mode]["mapped_lines"]
    if mode == "def":
        assert _mark.check_xa_counts(name, got)[0] == _mark.MANIFEST["sets"][name]["def"]["xa_entries"]
    reg_off, regs = _mark.load(name)[:2]
    w = want["stat"]
    assert (st["reads"], st["regions"], st["lines"], st["xa_members"], st["cigar_regions"]) == (reg_off.size - 1, regs.size, w["lines"], w["xa_members"], w["cigar_regions"]), (st, w)
    n = np.diff(reg_off.astype(np.int64))
    assert (st["light_reads"], st["wave_reads"], st["hbm_reads"]) == (int(((n > 0) & (n <= 8)).sum()), int((n > 8).sum()), int((n > 512).sum())), st
    assert st["launches"] > 0 and st["kernel_ms"] > 0


def test_sets_reach_both_paths():
    n = lambda name: np.diff(_mark.load(name)[0].astype(np.int64))
    assert ((n("main100") > 0) & (n("main100") <= 8)).sum() > 2800 and (n("main100") > 8).any()   # the lane path (2,899 reads), and 101 reads for the wave
    assert (n("repeat100") > 64).sum() >= 60 and n("repeat100").max() <= 512                       # lists of several strips, in LDS


@pytest.mark.parametrize("name", ["main100", "repeat100"])
def test_path_flags_change_no_byte(exe, tmp_path, name):
    want = _mark.run(exe, tmp_path, name, _mark.ALL)
    n = np.diff(_mark.load(name)[0].astype(np.int64))
    got, st = _gpu(name, _mark.ALL | _mark.NO_LIGHT_PATH)
    _mark.same_bytes(got, want, (name, "no light path"))
    assert st["light_reads"] == 0 and st["wave_reads"] == int((n > 0).sum()) and st["hbm_reads"] == 0
    got, st = _gpu(name, _mark.ALL | _mark.NO_LIGHT_PATH | _mark.FROM_HBM)
    _mark.same_bytes(got, want, (name, "from HBM"))
    assert st["light_reads"] == 0 and st["hbm_reads"] == st["wave_reads"] == int((n > 0).sum()) > 0


def test_a_z_of_several_ballot_steps_on_a_made_up_read(exe, tmp_path):
    """NOT a comparison with the reference (see _mark.tiled_read): 150 primaries, three ballot steps in the wave kernel's k loop"""
    arrays, tile_of = _mark.tiled_read()
    want = _mark.run(exe, tmp_path, "main100", 0, arrays=arrays)
    for flags in (0, _mark.FROM_HBM):
        got, st = _gpu("main100", flags, arrays=arrays)
        _mark.same_bytes(got, want, ("tiled", flags))
        _mark.check_tiled(got, arrays, tile_of)
        assert st["wave_reads"] == 1 and st["light_reads"] == 2 and st["hbm_reads"] == (1 if flags else 0)


def test_marks_feed_the_cigar_stage():
    import compseed_amd as ca
    name = "long90"
    reg_off, regs, bases, off, _ = _mark.load(name)
    al = ca.Aligner(_data.PREFIX, 0, _cigar.aln_params(name))
    try:
        res = al.regions_mark(reg_off, regs, off, ca.MarkParams(**_mark.mark_params(name)))
        alns = al.regions_cigar(res["cigar_reg_off"], res["cigar_regs"], bases, off)
        ms, cs = al.mark_stats(), al.cigar_stats()
    finally:
        al.close()
    n_x, n_l = _mark.check_cigars(name, res, alns)                          # every SAM line and XA entry of the fixture comes out
    assert n_x == _mark.MANIFEST["sets"][name]["def"]["xa_entries"] > 0 and n_l == _mark.MANIFEST["sets"][name]["def"]["mapped_lines"]
    assert cs["regions"] == ms["cigar_regions"] == res["cigar_regs"].size < regs.size


def test_empty_input_errors_and_reuse(exe, tmp_path):
    import compseed_amd as ca
    reg_off, regs, _, off, _ = _mark.load("main100")
    l_pac, _ = _cigar.contigs()
    n = int(reg_off[40])
    regs = regs[:n].copy(); reg_off = reg_off[:41].copy(); off = off[:41].copy()
    want = _mark.run(exe, tmp_path / "a", "main100", 0, arrays=(reg_off, regs, off))
    al = ca.Aligner(_data.PREFIX, 0)
    try:
        _mark.same_bytes(al.regions_mark(reg_off, regs, off), want, "first call")
        _mark.same_bytes(al.regions_mark(reg_off, regs, off), want, "second call")           # two calls in a row
        empty = al.regions_mark(reg_off[:1], regs[:0], off[:1])
        assert empty["marks"].size == 0 and empty["line_off"].tolist() == [0] and empty["cigar_reg_off"].tolist() == [0] and empty["cigar_regs"].size == 0
        none = al.regions_mark(np.zeros(41, np.uint64), regs[:0], off)                        # reads without regions
        assert none["marks"].size == 0 and none["line_off"].size == 41 and not none["line_off"].any() and not none["cigar_reg_off"].any()

        def fails(code, ro=reg_off, rg=regs, of=off, **kw):
            with pytest.raises(ca.CSError) as ei:
                al.regions_mark(ro, rg, of, **kw)
            assert ei.value.code == code, (ei.value.code, code, kw)

        def changed(k, **fields):
            bad = regs.copy()
            for f, v in fields.items():
                bad[f][k] = v
            return bad
        fails(-1, flags=8)                                                   # unknown flag bits
        fails(-1, flags=0x400)
        fails(-1, params=ca.MarkParams(mapq_coef_len=0))                     # that formula stays the caller's
        fails(-1, params=ca.MarkParams(mapq_coef_len=-3))
        fails(-5, params=ca.MarkParams(mapq_coef_len=200000))                # CS_ERANGE: beyond the table of logarithms
        # what check_read refuses, each found before any kernel follows an offset
        for bad in (changed(1, qe=regs["qb"][1]), changed(2, rb=-1), changed(3, re=-5), changed(4, qb=-1), changed(7, qe=30000), changed(9, re=2 * l_pac + 5), changed(5, rid=-1), changed(6, rid=2),
                    changed(8, score=-1)):
            fails(-1, rg=bad)
        x = reg_off.copy(); x[5] = x[7]
        y = reg_off.copy(); y[-1] += 1
        z = off.copy(); z[9] = z[8] - 1
        w = reg_off.copy(); w[0] = 1
        for ro, of in ((x, off), (y, off), (reg_off, z), (w, off)):
            fails(-1, ro=ro, of=of)
        fails(-5, rg=changed(10, rb=0, re=131073))                           # sizes: CS_ERANGE
        big = np.zeros(70000, ca.ALNREG_DT)
        big["qe"] = 50; big["rb"] = np.arange(70000); big["re"] = big["rb"] + 50; big["score"] = 50
        fails(-5, ro=np.array([0, 70000], np.uint64), rg=big, of=np.array([0, 100], np.uint64))
        _mark.same_bytes(al.regions_mark(reg_off, regs, off), want, "after the errors")      # the aligner is usable afterwards
    finally:
        al.close()
    host = ca.Aligner(_data.PREFIX, -1)
    try:
        with pytest.raises(ca.CSError) as ei:
            host.regions_mark(reg_off, regs, off)
        assert ei.value.code == -4                                           # CS_EDEVICE
        assert host.mark_stats()["regions"] == 0
    finally:
        host.close()
