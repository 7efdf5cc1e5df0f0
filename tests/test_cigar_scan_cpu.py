"""From regions to CIGAR, NM and MD without a GPU: the bodies of compseed_amd/csrc/cigar_scan.hpp (the band and its retries, the banded
global alignment with ksw_global2's backtrack matrix, the backtrack as a counting and a writing walk, NM / MD, the squeezed deletion, the
clips, the contig position) driven in the kernels' order by a plain C++ program (tests/cpp/cigar_scan_check.cpp).  Over the reference's
own regions (tests/golden/ddp1, aln2) every SAM line the reference's program wrote for a read (tests/golden/sam1: -a -Y) must be among
the results for that read's regions -- strand, contig, position, CIGAR, NM, MD, and AS = the region's score --, and at most 3 % of a
set's regions with score >= 30 may be left without a line (the reference's output filter drops some; gap3k's pieces are mostly dropped
secondaries, so it is compared for containment only, as the fixture's MANIFEST says).  The program itself fails if a job's fill score is
not banded_global_score's, if a walk leaves its band, or if the writing call counts otherwise than the counting call.  The one-lane
instantiation runs over every set.  The 64- and 8-lane instantiations run on threads in lockstep over a share of indel150_400, long90,
gap3k, params.odei and params.oied -- an emulated exchange is two barriers among up to 64 threads, about a millisecond and a half per
strip at 64 lanes, so whole sets would take hours (long90 alone: 1,201 jobs of some 6,000 strips) -- chosen job by job with the jobs
that have several strips a row first (_cigar.subset), and must give the one-lane build's bytes.  Over whole sets the 64-lane fill is
checked on the GPU only (tests/test_gpu_regions_cigar.py).
No golden set holds a region whose band doubles: where the reference goes round again (score < truesc - a) its band is 0 and stays 0.
The doubling of next_try is therefore tested on regions whose truesc is raised by hand, with nothing of the reference to compare
with: only the rule's own consequences are asserted there (test_retries_double_the_band_on_made_up_truesc)."""
import pytest

import _cigar


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _cigar.build(str(tmp_path_factory.mktemp("cigar_scan") / "cigar_scan_check"))


@pytest.fixture(scope="module")
def lanes_exe(tmp_path_factory):
    return {n: _cigar.build(str(tmp_path_factory.mktemp("cigar_scan_%d" % n) / "cigar_scan_check"), n) for n in (64, 8)}


@pytest.fixture(scope="module")
def one_lane(exe, tmp_path_factory):
    """the one-lane result per set, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            reg_off, regs, bases, off, _ = _cigar.load(name)
            cache[name] = _cigar.run(exe, tmp_path_factory.mktemp("one_" + name.replace(".", "_")), reg_off, regs, bases, off, _cigar.aln_params(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", _cigar.SETS)
def test_one_lane_pass_gives_the_references_alignments(one_lane, name):
    res = one_lane(name)
    reg_off, regs, _, _, _ = _cigar.load(name)
    _cigar.check_layout(res, regs.size)
    st = res["stat"]
    assert st["rejected"] == 0 and st["dp_jobs"] + st["nodp_jobs"] == regs.size, (name, st)   # the reference's regions are all live and inside a strand
    if "no_sam" in _cigar.MANIFEST["sets"][name]:
        return                                                               # cap64: the program's own checks (scores, bands, counts) only
    lines, regs30, unclaimed = _cigar.check_against_sam(name, res)
    print("%s: %d lines, %d regions with score >= 30, %d unclaimed (%.2f %%); %s" % (name, lines, regs30, unclaimed, 100. * unclaimed / regs30, st))


def test_sets_reach_what_they_are_for(one_lane):
    assert one_lane("main100")["stat"]["nodp_jobs"] > 0 and one_lane("main100")["stat"]["dp_jobs"] > 0
    assert one_lane("indel150_400")["stat"]["dp_jobs"] > 10000
    # (no golden set reaches a second try with a doubled band: where the reference goes round again its band is 0 and stays 0, which
    # next_try ends after one evaluation -- test_retries_double_the_band makes the case)
    assert all(one_lane(name)["stat"]["retries"] == 0 and (one_lane(name)["alns"]["tries"] == 1).all() for name in ("params.odei", "params.oied", "params.w10"))
    ops = lambda name: one_lane(name)["cigar"] & 15
    assert (ops("indel150_400") == 1).any() and (ops("indel150_400") == 2).any() and (ops("ends") == 3).any()
    assert (one_lane("ends")["alns"]["is_rev"] == 1).any() and (one_lane("ends")["alns"]["rid"] == 1).any()
    assert one_lane("gap3k")["alns"]["w"].max() >= 100                       # the long gaps: wide bands, 3-kb spans


@pytest.mark.parametrize("lanes,name", [(64, "indel150_400"), (64, "long90"), (64, "gap3k"), (8, "long90"), (8, "gap3k"), (64, "params.odei"), (8, "params.oied"),
                                        (8, "indel150_400"), (8, "params.odei"), (64, "params.oied")])
def test_many_lane_fill_in_lockstep(exe, lanes_exe, tmp_path, lanes, name):
    """the wave's fill: strips of 64 or 8 columns, F as a prefix maximum with the carry between strips; the same bytes as one lane (so
    the same scores, which the one-lane build holds against banded_global_score).  Each case gets the jobs that fit 7,000 strips at 64
    lanes or 70,000 at 8 (some ten seconds), those with several strips a row first: every job of the share at 8 lanes; at 64 lanes
    all but a few of indel150_400's, long90's and gap3k's -- params.odei and params.oied hold no job wider than 64 columns at all (bands
    of up to 14 and 10), so 64 lanes run their one-strip rows, where lanes beyond the band's end must stay out."""
    reg_off, regs, bases, off = _cigar.subset(name, lanes, 7000 if lanes == 64 else 70000)
    _, n_col = _cigar.bands(name, regs)
    wide = int((n_col > lanes).sum())
    assert wide >= (0 if lanes == 64 and name.startswith("params.") else 1), (name, lanes, wide, regs.size)
    print("%s, %d lanes: %d jobs, %d with several strips a row" % (name, lanes, regs.size, wide))
    want = _cigar.run(exe, tmp_path / "one", reg_off, regs, bases, off, _cigar.aln_params(name))
    got = _cigar.run(lanes_exe[lanes], tmp_path / "many", reg_off, regs, bases, off, _cigar.aln_params(name))
    assert want["stat"]["dp_jobs"] == int((n_col > 0).sum()) > 0, name        # (the sizing's band formulas are the header's)
    for k in ("alns", "cigar", "md"):
        assert got[k].tobytes() == want[k].tobytes(), (name, lanes, k)
    assert got["stat"] == want["stat"], (name, lanes)


def test_retries_double_the_band_on_made_up_truesc(exe, tmp_path):
    """NOT a comparison with the reference: no fixture holds a real retry with a doubled band.  Regions that claim 60 points more than their
    alignment can give (truesc raised by hand): the global score stays below truesc - a, so the band doubles until three tries are made,
    the score repeats or 4 w is reached (comp_seed.cpp:835-843), and the last try is the one kept.  Asserted: what follows from that
    rule and from a CIGAR's meaning, nothing else."""
    import numpy as np
    reg_off, regs, bases, off = _cigar.subset("params.odei", 1, 0, first_reads=17)
    regs["truesc"] += 60
    res = _cigar.run(exe, tmp_path, reg_off, regs, bases, off, _cigar.aln_params("params.odei"))
    _cigar.check_layout(res, regs.size)
    a = res["alns"]
    assert res["stat"]["retries"] > 0 and a["tries"].max() >= 2 and a["tries"].min() >= 1 and a["tries"].max() <= 3
    assert res["stat"]["retries"] == int((a["tries"] - 1).sum())
    assert (a["w"] <= 4 * 7).all() and (a["w"][a["tries"] == 3] % 4 == 0).all()        # doubled twice
    read_len = np.diff(off.astype(np.int64))[np.repeat(np.arange(off.size - 1), np.diff(reg_off.astype(np.int64)))]
    for g, (_, _, _, score, _, _, _, cg, _) in enumerate(_cigar.per_region(res)):
        assert sum(c >> 4 for c in cg if c & 15 in (0, 1, 3)) == read_len[g], g         # the CIGAR spans the read
        assert sum(c >> 4 for c in cg if c & 15 in (0, 2)) <= regs["re"][g] - regs["rb"][g], g


def test_small_budget_takes_many_chunks_and_changes_no_alignment(exe, one_lane, tmp_path):
    reg_off, regs, bases, off, _ = _cigar.load("gap3k")
    got = _cigar.run(exe, tmp_path, reg_off, regs, bases, off, _cigar.aln_params("gap3k"), budget=64 << 10)
    want = one_lane("gap3k")
    assert got["stat"]["chunks"] > want["stat"]["chunks"] and got["stat"]["chunks"] > 10
    _cigar.check_layout(got, regs.size)
    assert _cigar.per_region(got) == _cigar.per_region(want)


def test_empty_purged_unmapped_and_rejected_regions(exe, tmp_path):
    import numpy as np
    reg_off, regs, bases, off, _ = _cigar.load("main100")
    l_pac, _ = _cigar.contigs()
    n = int(reg_off[40])
    regs = regs[:n].copy(); reg_off = reg_off[:41].copy(); bases = bases[:int(off[40])]; off = off[:41].copy()
    want = _cigar.per_region(_cigar.run(exe, tmp_path / "a", reg_off, regs, bases, off, _cigar.aln_params("main100")))
    regs["qe"][1] = regs["qb"][1]                                            # purged
    regs["rb"][2] = -1                                                       # unmapped
    regs["re"][3] = -5
    fwd = int(np.flatnonzero(regs["re"] <= l_pac)[5])
    regs["rb"][fwd] = l_pac - 40; regs["re"][fwd] = l_pac - 40 + (regs["qe"][fwd] - regs["qb"][fwd])   # bridges the strands
    res = _cigar.run(exe, tmp_path / "b", reg_off, regs, bases, off, _cigar.aln_params("main100"))
    got = _cigar.per_region(res)
    assert res["stat"]["rejected"] == 1
    for g in range(n):
        if g in (1, 2, 3):
            assert got[g] == (-1, -1, 0, 0, 0, 0, 0, (), b""), g
        elif g == fwd:
            assert got[g] == (-1, -1, 0, 0, -1, 0, 0, (), b""), g
        else:
            assert got[g] == want[g], g
    empty = _cigar.run(exe, tmp_path / "c", reg_off[:1], regs[:0], bases[:0], off[:1], _cigar.aln_params("main100"))
    assert empty["alns"].size == 0 and empty["cigar"].size == 0 and empty["md"].tobytes() == b"\0"
    regs["qe"][7] = 30000                                                    # outside its read: the checks refuse the batch
    _cigar.run(exe, tmp_path / "d", reg_off, regs, bases, off, _cigar.aln_params("main100"), expect=3)
