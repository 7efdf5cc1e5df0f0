"""Primary marking, MAPQ, SAM line selection and XA membership without a GPU: the bodies of compseed_amd/csrc/mark_scan.hpp
(mem_mark_primary_se with its ALT branch, mem_approx_mapq_se, the loop of mem_reg2sam, mem_gen_alt's rule) driven in the kernels' order by
a plain C++ program (tests/cpp/mark_scan_check.cpp).  Over the reference's own regions (tests/golden/ddp1, aln2, mark1/alt.main100) the
lines of every read must be EXACTLY the lines the reference's program wrote for it (tests/golden/mark1: once with -a -Y, once with -Y), in
order: flag, MAPQ, AS, XS and the number of SA entries; the reads without a line exactly its unmapped ones; in default mode the XA lists
as long as its XA tags, and after the CIGAR stage (tests/cpp/cigar_scan_check.cpp over cigar_regs) entry by entry the same.  These are
equalities: nothing here is a cap.  The one-lane instantiation runs over all 15 sets in both modes.  The 8- and 64-lane instantiations
run on threads in lockstep over repeat100 (120 reads of up to 501 regions: lists of several strips), ragged, long90 and ends (the
0x800 lines and the MAPQ cap) and alt.main100 (the ALT branch), and must give the one-lane build's bytes.  No golden read has more
than a handful of primaries, so z never spans a second ballot step there: that case runs on a made-up read, against the rule itself."""
import numpy as np
import pytest

import _cigar
import _mark


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _mark.build(str(tmp_path_factory.mktemp("mark_scan") / "mark_scan_check"))


@pytest.fixture(scope="module")
def lanes_exe(tmp_path_factory):
    return {n: _mark.build(str(tmp_path_factory.mktemp("mark_scan_%d" % n) / "mark_scan_check"), n) for n in (64, 8)}


@pytest.fixture(scope="module")
def one_lane(exe, tmp_path_factory):
    """the one-lane result per (set, flags), computed once"""
    cache = {}

    def get(name, flags):
        if (name, flags) not in cache:
            cache[name, flags] = _mark.run(exe, tmp_path_factory.mktemp("one_%s_%d" % (name.replace(".", "_"), flags)), name, flags)
        return cache[name, flags]
    return get


@pytest.mark.parametrize("name", _mark.SETS)
def test_one_lane_pass_gives_exactly_the_references_lines(one_lane, name):
    for mode, flags in (("all", _mark.ALL), ("def", 0)):
        res = one_lane(name, flags)
        _mark.check_properties(name, res)
        n = _mark.check_lines(name, res, mode)
        assert n == _mark.MANIFEST["sets"][name][mode]["mapped_lines"]
        m = res["marks"]
        if mode == "all":
            assert (m["xa_of"] == -1).all() and res["stat"]["xa_members"] == 0
        else:
            entries, members = _mark.check_xa_counts(name, res)
            assert entries == _mark.MANIFEST["sets"][name]["def"]["xa_entries"]
            print("%s: %d lines, %d XA entries, %d regions with xa_of >= 0, %d of %d regions to the CIGAR stage" % (name, n, entries, members, res["stat"]["cigar_regions"], m.size))


def test_sets_reach_what_they_are_for(one_lane):
    rep = one_lane("repeat100", _mark.ALL)["marks"]
    ro = _mark.load("repeat100")[0].astype(np.int64)
    assert np.diff(ro).max() > 448 and (rep["sub_n"] > 64).any()             # lists of several strips at 64 lanes
    # every read of repeat100 lies inside the repeat: one primary each, so z never holds more than one entry there, and no golden set
    # has a read with more than a handful of primaries.  A z of several ballot steps is made by hand (_mark.tiled_read)
    assert max(int((rep["secondary"][ro[r]:ro[r + 1]] < 0).sum()) for r in range(ro.size - 1)) == 1
    alt = one_lane(_mark.ALT, 0)["marks"]
    assert (alt["is_alt"] == 1).any() and (alt["secondary"] == _mark.INT_MAX).any() and (alt["alt_sc"] > 0).any()
    assert ((alt["secondary_all"] >= 0) & (alt["secondary"] < 0)).any()      # a primary of the second round that the first one had under an ALT hit
    for name in ("long90", "ends"):
        m = one_lane(name, 0)["marks"]
        assert (m["flag"] & 0x800 != 0).sum() == _mark.MANIFEST["sets"][name]["def"]["supplementary_lines"] > 0
    # the MAPQ cap of a supplementary line (comp_seed.cpp:1103) is reached: without it some 0x800 line would carry more than its read's first line
    # (in `ends`; long90's supplementary lines all stay below their read's first line)
    m = one_lane("ends", _mark.KEEP_SUPP_MAPQ)["marks"]
    assert (m["mapq"] != one_lane("ends", 0)["marks"]["mapq"]).any()


@pytest.mark.parametrize("name", ["main100", "long90", "params.oied"])
def test_xa_entries_and_lines_after_the_cigar_stage(one_lane, tmp_path, name):
    res = one_lane(name, 0)
    _, _, bases, off, _ = _mark.load(name)
    cig = _cigar.build(str(tmp_path / "cigar_scan_check"))
    alns = _cigar.run(cig, tmp_path / "c", res["cigar_reg_off"], res["cigar_regs"], bases, off, _cigar.aln_params(name))
    assert _cigar.MANIFEST["sets"][name]["keep_every_kth_read"] == 1
    n_x, n_l = _mark.check_cigars(name, res, alns)
    assert n_x == _mark.MANIFEST["sets"][name]["def"]["xa_entries"] and n_l == _mark.MANIFEST["sets"][name]["def"]["mapped_lines"]
    assert res["cigar_regs"].size < _mark.load(name)[1].size                # fewer regions than a caller without marks has to align


LOCKSTEP = [("repeat100", _mark.ALL), ("ragged", _mark.ALL), ("long90", 0), ("ends", 0), (_mark.ALT, 0), (_mark.ALT, _mark.ALL)]


# (an emulated exchange is two barriers among the lanes' threads: repeat100 takes some seven seconds at 64 lanes, so its second mode --
# the same marking, another selection -- runs at 8 lanes only)
@pytest.mark.parametrize("lanes,name,flags", [(w, n, f) for w in (8, 64) for n, f in LOCKSTEP] + [(8, "repeat100", 0)])
def test_many_lane_pass_in_lockstep(one_lane, lanes_exe, tmp_path, lanes, name, flags):
    got = _mark.run(lanes_exe[lanes], tmp_path, name, flags)
    want = one_lane(name, flags)
    _mark.same_bytes(got, want, (name, lanes, flags))
    assert got["stat"] == want["stat"]


@pytest.mark.parametrize("lanes", [1, 8, 64])
def test_a_z_of_several_ballot_steps_on_a_made_up_read(exe, lanes_exe, tmp_path, lanes):
    """NOT a comparison with the reference (see _mark.tiled_read): 150 primaries, so the k loop takes 3 steps of 64 entries and 19 of 8, and
    the first hit is in any of them.  Asserted: what the rule gives for these regions, worked out from the regions alone, and the one-lane bytes."""
    arrays, tile_of = _mark.tiled_read()
    want = _mark.run(exe, tmp_path / "one", "main100", 0, arrays=arrays)
    _mark.check_properties("main100", want, arrays=arrays)
    _mark.check_tiled(want, arrays, tile_of)
    if lanes > 1:
        _mark.same_bytes(_mark.run(lanes_exe[lanes], tmp_path / "many", "main100", 0, arrays=arrays), want, lanes)


def test_no_multi_and_keep_supp_mapq(one_lane):
    base = one_lane("long90", 0)["marks"]
    nm = one_lane("long90", _mark.NO_MULTI)["marks"]
    supp = base["flag"] & 0x800 != 0
    assert supp.any()
    want = base.copy()
    want["flag"][supp] = (base["flag"][supp] & ~0x800) | 0x100
    assert nm.tobytes() == want.tobytes()                                   # every 0x800 becomes 0x100 and nothing else changes
    for k in ("line_off", "cigar_reg_off", "cigar_regs", "cigar_src"):
        assert one_lane("long90", _mark.NO_MULTI)[k].tobytes() == one_lane("long90", 0)[k].tobytes()
    for name in ("long90", "ends"):                                         # (the cap is reached in `ends` only)
        base, keep = one_lane(name, 0)["marks"], one_lane(name, _mark.KEEP_SUPP_MAPQ)["marks"]
        differ = keep["mapq"] != base["mapq"]
        assert differ.any() == (name == "ends")
        assert (keep["mapq"] >= base["mapq"]).all() and (base["flag"][differ] & 0x800 != 0).all()   # only MAPQs of 0x800 lines, and only upwards
        assert all((keep[f] == base[f]).all() for f in base.dtype.names if f != "mapq")


def test_the_hash_depends_on_the_reads_number(exe, tmp_path):
    """id_base shifts every read's hash_64 argument: ties between equal scores fall otherwise, the lines' scores stay"""
    a = _mark.run(exe, tmp_path / "a", "repeat100", _mark.ALL)
    b = _mark.run(exe, tmp_path / "b", "repeat100", _mark.ALL, id_base=1000)
    assert a["marks"]["reg"].tobytes() != b["marks"]["reg"].tobytes()
    _mark.check_properties("repeat100", b)
    assert a["line_off"].tobytes() == b["line_off"].tobytes()


def test_empty_input_and_what_the_checks_refuse(exe, tmp_path):
    reg_off, regs, _, off, _ = _mark.load("main100")
    l_pac, _ = _cigar.contigs()
    n = int(reg_off[40])
    regs = regs[:n].copy(); reg_off = reg_off[:41].copy(); off = off[:41].copy()
    first = _mark.run(exe, tmp_path / "a", "main100", 0, arrays=(reg_off, regs, off))
    _mark.check_properties("main100", first, arrays=(reg_off, regs))
    empty = _mark.run(exe, tmp_path / "b", "main100", 0, arrays=(reg_off[:1], regs[:0], off[:1]))
    assert empty["marks"].size == 0 and empty["line_off"].tolist() == [0] and empty["cigar_reg_off"].tolist() == [0]
    none = _mark.run(exe, tmp_path / "c", "main100", 0, arrays=(np.zeros(41, np.uint64), regs[:0], off))
    assert none["marks"].size == 0 and not none["line_off"].any() and none["line_off"].size == 41

    def refused(k, what, status=3, **fields):
        bad = regs.copy()
        for f, v in fields.items():
            bad[f][k] = v
        _mark.run(exe, tmp_path / what, "main100", 0, arrays=(reg_off, bad, off), expect=status)
    refused(1, "purged", qe=regs["qb"][1])
    refused(2, "unmapped_rb", rb=-1)
    refused(3, "unmapped_re", re=-5)
    refused(4, "qb", qb=-1)
    refused(7, "outside_read", qe=30000)
    refused(9, "outside_ref", re=2 * l_pac + 5)
    refused(5, "rid_low", rid=-1)
    refused(6, "rid_high", rid=2)
    refused(8, "score", score=-1)
    refused(10, "span", status=4, rb=0, re=131073)                           # a size: the library's CS_ERANGE
    x = reg_off.copy(); x[5] = x[7]
    y = reg_off.copy(); y[-1] += 1
    z = off.copy(); z[9] = z[8] - 1
    w = reg_off.copy(); w[0] = 1
    for k, (ro, of) in enumerate(((x, off), (y, off), (reg_off, z), (w, off))):
        _mark.run(exe, tmp_path / ("csr%d" % k), "main100", 0, arrays=(ro, regs, of), expect=3)


def test_a_read_of_70000_regions_is_out_of_range(exe, tmp_path):
    import compseed_amd as ca
    regs = np.zeros(70000, ca.ALNREG_DT)
    regs["qe"] = 50; regs["rb"] = np.arange(70000); regs["re"] = regs["rb"] + 50; regs["score"] = 50
    _mark.run(exe, tmp_path, "main100", 0, arrays=(np.array([0, 70000], np.uint64), regs, np.array([0, 100], np.uint64)), expect=4)
