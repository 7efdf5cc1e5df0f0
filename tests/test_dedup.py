"""cs_dedup_regions (dedup.cpp) = what the reference does with a read's alignment regions after the extension stage (comp_seed.cpp:2385-2395):
purged regions dropped, mem_sort_dedup_patch (comp_seed.cpp:629-687).  In: the regions the reference's extension stage left (tests/golden/aln1,
flt1, ddp1/gap3k.aln.npz); out must be what the reference's own mem_sort_dedup_patch left (tests/golden/ddp1/, oracle/_ref/ref_dump --dedup),
region by region in its order: two unstable sorts whose tie order is klib's, redundant regions removed, and -- gap3k: 3-kb reads with a
gap in the middle that the extension does not cross -- pairs of regions merged after a banded global alignment (ksw_global2's score).
tests/golden/aln2 (make_golden.py aln2) adds what those runs do not reach: scoring, band and Z-drop other than mem_opt_init's (the global alignment of
the patch reads them through the aligner's cs_aln_params_t), regions at the ends of the contigs, reads of exactly 63 to 65 regions.
Host code: runs without a GPU (an aligner created with device -1)."""
import os

import numpy as np
import pytest

import _aln2
import _data

G = os.path.dirname(_data.GOLD)
SETS = {"main100": ("aln1", _data.GOLD), "sorted150": ("aln1", _data.GOLD), "ragged": ("aln1", _data.GOLD), "repeat100": ("aln1", _data.GOLD),
        "indel150_400": ("aln1", os.path.join(G, "aln1")), "long90": ("flt1", os.path.join(G, "flt1")), "gap3k": ("ddp1", os.path.join(G, "ddp1"))}


def _load(name):
    import compseed_amd as ca
    adir, rdir = SETS[name]
    z = np.load(os.path.join(G, adir, name + ".aln.npz"))
    zd = np.load(os.path.join(G, "ddp1", name + ".ddp.npz"))
    raw = open(os.path.join(rdir, name + ".txt"), "rb").read()
    reads = raw.split(b"\n")[:-1] if raw.endswith(b"\n") else raw.split(b"\n")
    bases, off = _data.pack_reads(reads)
    regs = np.zeros(z["reg_rb"].size, dtype=ca.ALNREG_DT)
    for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep", "chain"):
        regs[f] = z["reg_" + f]
    return z["reg_off"], regs, bases, off, zd


@pytest.mark.parametrize("name", sorted(SETS))
def test_regions_after_dedup_are_the_references(name):
    import compseed_amd as ca
    reg_off, regs, bases, off, zd = _load(name)
    al = ca.Aligner(_data.PREFIX, -1)
    got = al.dedup_regions(reg_off, regs, bases, off)
    al.close()
    assert np.array_equal(got["reg_off"], zd["reg_off"]), name
    g = got["regs"]
    for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0"):
        assert np.array_equal(g[f], zd["reg_" + f]), (name, f, int((g[f] != zd["reg_" + f]).sum()))
    assert np.array_equal(g["frac_rep"].view(np.uint32), zd["reg_frac_rep"].view(np.uint32))
    assert np.array_equal(got["n_comp"], zd["reg_n_comp"])
    assert g.size < regs.size


def test_goldens_exercise_merges_and_ties():
    zd = np.load(os.path.join(G, "ddp1", "gap3k.ddp.npz"))
    assert (zd["reg_n_comp"] > 1).sum() > 100                 # regions the patch merged
    z = np.load(os.path.join(G, "ddp1", "repeat100.ddp.npz"))
    per_read = np.diff(z["reg_off"].astype(np.int64))
    assert per_read.max() > 100                                # hundreds of regions per read: equal scores and equal ends, the sorts' tie order decides


@pytest.mark.parametrize("name", _aln2.SETS)
def test_aln2_regions_after_dedup_are_the_references(name):
    """the aln2 sets, each with the cs_aln_params_t the reference ran with"""
    import compseed_amd as ca
    reg_off, regs = _aln2.regions(_aln2.npz(name, "aln"))
    zd = _aln2.npz(name, "ddp")
    bases, off = _aln2.reads(name)
    al = ca.Aligner(_data.PREFIX, -1, _aln2.aln_params(name))
    got = al.dedup_regions(reg_off, regs, bases, off)
    al.close()
    assert np.array_equal(got["reg_off"], zd["reg_off"]), name
    g = got["regs"]
    for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0"):
        assert np.array_equal(g[f], zd["reg_" + f]), (name, f, int((g[f] != zd["reg_" + f]).sum()))
    assert np.array_equal(g["frac_rep"].view(np.uint32), zd["reg_frac_rep"].view(np.uint32))
    assert np.array_equal(got["n_comp"], zd["reg_n_comp"])
    assert 0 < g.size < regs.size


def test_aln2_goldens_reach_what_they_are_for():
    """the committed aln2 files hold: reads of exactly 63, 64 and 65 regions (purge_kernel's limit and its all-lanes branch, the first read
    for purge_big_kernel); chains of 8 and 9 seeds (SMALL_CHAIN) under non-default parameters; live regions that begin or end at 0, at the
    contigs' join on either strand, at l_pac and at 2 * l_pac; in every params set regions at w and at 2w (a retry), except where the
    reference itself leaves none (recorded in the manifest); scores beyond 8 bits; at least five non-default parameter sets over at most
    200 reads"""
    M = _aln2.MANIFEST
    l_pac, join = M["l_pac"], M["join"]
    assert l_pac == int(open(_data.PREFIX + ".ann").read().split()[0])
    per_read, chain_n, max_score = [], [], 0
    edges = {0: 0, join: 0, l_pac: 0, 2 * l_pac - join: 0, 2 * l_pac: 0}
    for name in _aln2.SETS:
        z, info = _aln2.npz(name, "aln"), M["sets"][name]
        assert z["reg_rb"].size == z["cseed_rbeg"].size == info["regions"]
        live = z["reg_qe"] > z["reg_qb"]
        assert np.array_equal(~live, (z["reg_qb"] == -1) & (z["reg_qe"] == -1)) and int((~live).sum()) == info["purged"]
        per_read += np.diff(z["reg_off"].astype(np.int64)).tolist()
        for x in edges:
            edges[x] += int((z["reg_rb"][live] == x).sum() + (z["reg_re"][live] == x).sum())
        max_score = max(max_score, int(z["reg_score"].max()))
        if name in _aln2.PARAM_SETS:
            chain_n += z["chain_n"].tolist()
            w = info["aln_params"]["w"]
            ws = set(z["reg_w"][live].tolist())
            assert w in ws and (info["reference_leaves_no_2w"] or 2 * w in ws), (name, ws)
            assert info["reference_leaves_no_2w"] == (2 * w not in ws)
            assert info["n_reads"] <= 200 and info["aln_params"] != M["sets"]["ends"]["aln_params"]
    per_read, chain_n = np.array(per_read), np.array(chain_n)
    for k in (63, 64, 65):
        assert (per_read == k).sum() >= 5, k
    assert (chain_n == 8).sum() >= 5 and (chain_n == 9).sum() >= 5
    assert min(edges.values()) >= 5, edges
    assert max_score > 255
    assert len(_aln2.PARAM_SETS) >= 5 and [s for s in _aln2.PARAM_SETS if M["sets"][s]["reference_leaves_no_2w"]] == ["params.a2", "params.w3d0"]
    assert (per_read > 64).sum() > 0 and M["sets"]["params.w3d0"]["purged"] * 10 < M["sets"]["params.w3d0"]["regions"]   # the purge's cliff at w = 3, zdrop = 0


def test_host_only_aligner_refuses_to_extend():
    import compseed_amd as ca
    al = ca.Aligner(_data.PREFIX, -1)
    with pytest.raises(ca.CSError) as ei:
        al.extend_chains(np.zeros(1, np.uint64), np.zeros(0, ca.CHAIN_DT), np.zeros(1, np.uint64), np.zeros(0, ca.SEED_DT), np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert ei.value.code == -4
    al.close()
