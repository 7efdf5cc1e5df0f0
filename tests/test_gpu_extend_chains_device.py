"""The extension stage over device-resident chains (cs_extend_chains_device, compseed_amd/csrc/align_gpu.hip): the reference's own regions
on the seven golden sets from uploaded chains, with the purged regions kept (device flags 0: byte for byte cs_extend_chains' result) and
left behind on the device (CS_ALN_DEV_COMPACT); the whole chain seed_batch_device -> chain_device -> filter_device -> extend_chains_device
without a host array in between; cs_dedup_regions of the compacted result; the checking kernels; degenerate batches; host and device
calls on one aligner."""
import functools
import os

import numpy as np
import pytest

import _aln2
import _data
from test_gpu_align import DDP, _load
from test_gpu_chain_device import ENGINE_RUNS, _cp

gpu = pytest.mark.gpu
SETS = ["main100", "sorted150", "ragged", "repeat100", "indel150_400", "long90", "gap3k"]
FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "chain")
COUNTERS = ("reads", "regions", "pairs", "retries", "purged", "launches")
DEV_FLAGS = [0, 1]   # 0, CS_ALN_DEV_COMPACT


@functools.lru_cache(maxsize=None)
def _golden(name):
    """a golden set as cs_extend_chains takes it and as the reference left it: (chain_off, chains, cseed_off, cseeds, score), bases, off, reg_off, regs"""
    import compseed_amd as ca
    z, bases, off = _load(name)
    n_chains = z["chain_pos"].size
    chains = np.zeros(n_chains, dtype=ca.CHAIN_DT)
    chains["pos"], chains["rid"], chains["n_seeds"], chains["frac_rep"], chains["is_alt"] = z["chain_pos"], z["chain_rid"], z["chain_n"], z["chain_frac_rep"], z["chain_is_alt"]
    cseed_off = np.zeros(n_chains + 1, dtype=np.uint64); np.cumsum(z["chain_n"].astype(np.uint64), out=cseed_off[1:])
    cseeds = np.zeros(z["cseed_rbeg"].size, dtype=ca.SEED_DT)
    cseeds["rbeg"], cseeds["qbeg"], cseeds["len"] = z["cseed_rbeg"], z["cseed_qbeg"], z["cseed_len"]
    regs = np.zeros(z["reg_rb"].size, dtype=ca.ALNREG_DT)
    for f in FIELDS + ("frac_rep",):
        regs[f] = z["reg_" + f]
    batch = (z["chain_off"].astype(np.uint64), chains, cseed_off, cseeds, z["cseed_score"].astype(np.int32))
    return batch, bases, off, z["reg_off"].astype(np.uint64), regs


def _live(reg_off, regs):
    """what CS_ALN_DEV_COMPACT must leave of (reg_off, regs): each read's regions with qe > qb in unchanged order"""
    mask = regs["qe"] > regs["qb"]
    before = np.concatenate(([0], np.cumsum(mask))).astype(np.uint64)
    return before[reg_off.astype(np.int64)], regs[mask]


def _same_regs(got, reg_off, regs, what=None):
    assert got["reg_off"].dtype == np.uint64 and np.array_equal(got["reg_off"], reg_off), what
    g = got["regs"]
    assert g.size == regs.size, (what, g.size, regs.size)
    for f in FIELDS:
        assert np.array_equal(g[f], regs[f]), (what, f, int((g[f] != regs[f]).sum()))
    assert np.array_equal(g["frac_rep"].view(np.uint32), regs["frac_rep"].view(np.uint32)), what
    assert g.tobytes() == regs.tobytes(), what


class Dev:
    """host arrays in device memory through the engine's helpers, freed at the end of the test"""

    def __init__(self, eng):
        self.eng, self.ptrs = eng, []

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.eng.alloc(max(arr.nbytes, 8))
        if arr.nbytes:
            self.eng.upload(p, arr)
        self.ptrs.append(p)
        return p

    def chains(self, chain_off, chains, cseed_off, cseeds):
        return dict(n_reads=chain_off.size - 1, n_chains=chains.size, n_seeds=cseeds.size, chain_off=self.up(chain_off), chains=self.up(chains),
                    cseed_off=self.up(cseed_off), cseeds=self.up(cseeds))

    def free(self):
        for p in self.ptrs:
            self.eng.free(p)
        self.ptrs = []


@pytest.fixture(scope="module")
def eng():
    import compseed_amd as ca
    ix = ca.Index.load(_data.PREFIX)
    e = ca.Engine(ix, 0)
    yield e
    e.close()
    ix.close()


@pytest.fixture()
def dev(eng):
    d = Dev(eng)
    yield d
    d.free()


_HOST = {}


def _host_counters(name, aflags):
    """the counters one cs_extend_chains call over a golden set moves on a fresh aligner (computed once per set and aligner flags)"""
    import compseed_amd as ca
    if (name, aflags) not in _HOST:
        batch, bases, off, reg_off, regs = _golden(name)
        al = ca.Aligner(_data.PREFIX, 0, ca.AlnParams(flags=aflags))
        got = al.extend_chains(*batch[:4], bases, off, cseed_score=batch[4])
        st = al.stats()
        al.close()
        _same_regs(got, reg_off, regs, (name, "host call"))
        _HOST[(name, aflags)] = {k: st[k] for k in COUNTERS}
    return _HOST[(name, aflags)]


def test_goldens_reach_the_compactions_boundaries():
    """the seven sets hold reads whose regions are all purged or absent, reads with none purged and a read with more than 64 regions;
    over a quarter of the regions are purged"""
    empty = full = big = n_regs = n_live = 0
    for name in SETS:
        _, _, _, reg_off, regs = _golden(name)
        new_off, live = _live(reg_off, regs)
        per_read, per_read_live = np.diff(reg_off.astype(np.int64)), np.diff(new_off.astype(np.int64))
        empty += int((per_read_live == 0).sum()); full += int(((per_read_live == per_read) & (per_read > 0)).sum()); big += int((per_read > 64).sum())
        n_regs += regs.size; n_live += live.size
        assert regs.size > 4000 and regs.size - live.size > 1000, name
        assert np.array_equal(regs["qe"] > regs["qb"], ~((regs["qb"] == -1) & (regs["qe"] == -1))), name     # the purge's mark is the only way to qe <= qb here
    assert empty > 0 and full > 0 and big > 0, (empty, full, big)
    assert n_live < 0.75 * n_regs


@gpu
@pytest.mark.parametrize("dflags", DEV_FLAGS)
@pytest.mark.parametrize("aflags", [0, 3])
@pytest.mark.parametrize("name", SETS)
def test_uploaded_golden_chains_give_the_references_regions(eng, dev, name, aflags, dflags):
    import compseed_amd as ca
    batch, bases, off, reg_off, regs = _golden(name)
    want = _host_counters(name, aflags)
    d = dev.chains(*batch[:4])
    d_sc, d_b, d_o = dev.up(batch[4]), dev.up(bases), dev.up(off)
    al = ca.Aligner(_data.PREFIX, 0, ca.AlnParams(flags=aflags))
    r = al.extend_chains_device(d, d_b, d_o, d_cseed_score=d_sc, flags=dflags)
    st = al.stats()
    got = ca.download_regions(eng, r)
    al.close()
    assert r["n_reads"] == off.size - 1
    if dflags == 0:
        assert r["n_regs"] == regs.size
        _same_regs(got, reg_off, regs, name)
    else:
        new_off, live = _live(reg_off, regs)
        assert r["n_regs"] == live.size == int((regs["qe"] > regs["qb"]).sum())
        _same_regs(got, new_off, live, name)
    assert {k: st[k] for k in COUNTERS} == want and st["regions"] == regs.size and st["purged"] == int((regs["qe"] <= regs["qb"]).sum())


@gpu
@pytest.mark.parametrize("dflags", DEV_FLAGS)
@pytest.mark.parametrize("name", _aln2.SETS)
def test_uploaded_aln2_chains_give_the_references_regions(eng, dev, name, dflags):
    """tests/golden/aln2 (other scoring, band and Z-drop; the ends of the reference; reads of 63, 64 and 65 regions) through cs_extend_chains_device with the
    set's cs_aln_params_t: the reference's regions byte for byte, the purged ones kept or left behind, and the purge's counter"""
    import compseed_amd as ca
    z = _aln2.npz(name, "aln")
    bases, off = _aln2.reads(name)
    batch = _aln2.chains_in(z)
    reg_off, regs = _aln2.regions(z)
    d = dev.chains(*batch[:4])
    d_sc, d_b, d_o = dev.up(batch[4]), dev.up(bases), dev.up(off)
    al = ca.Aligner(_data.PREFIX, 0, _aln2.aln_params(name))
    r = al.extend_chains_device(d, d_b, d_o, d_cseed_score=d_sc, flags=dflags)
    st = al.stats()
    got = ca.download_regions(eng, r)
    al.close()
    assert r["n_reads"] == off.size - 1
    want = (reg_off, regs) if dflags == 0 else _live(reg_off, regs)
    assert r["n_regs"] == want[1].size
    _same_regs(got, *want, name)
    assert st["regions"] == regs.size and st["purged"] == int((regs["qe"] <= regs["qb"]).sum())


@gpu
@pytest.mark.parametrize("dflags", DEV_FLAGS)
def test_reads_to_regions_without_leaving_the_device(eng, dflags):
    """seed_batch_device -> chain_device -> filter_device -> extend_chains_device -> download_regions == cs_extend_chains of the downloaded
    filtered chains, byte for byte (and the aln1 golden for default seeding parameters); the filter's device output is left as it was and
    the result lies in buffers of the aligner's own"""
    import compseed_amd as ca
    chainer = ca.Chainer(_data.PREFIX, device=0)
    al, host = ca.Aligner(_data.PREFIX, 0), ca.Aligner(_data.PREFIX, 0)
    for name, pname in ENGINE_RUNS:
        z, kw = _data.load_golden(name, pname)
        bases, off = _data.load_reads(name)
        d_b, d_o = eng.alloc(bases.nbytes), eng.alloc(off.nbytes)
        eng.upload(d_b, bases); eng.upload(d_o, off)
        res = eng.seed_batch_device(d_b, d_o, off.size - 1, bases.size, ca.Params(**kw))
        fd = chainer.filter_device(chainer.chain_device(res, d_o, _cp(kw)), d_b, d_o)
        before = ca.download_chains(eng, fd)
        r = al.extend_chains_device(fd, d_b, d_o, flags=dflags)                      # (the scores are the dict's own)
        got = ca.download_regions(eng, r)
        after = ca.download_chains(eng, fd)
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), (name, pname, k)
        h = host.extend_chains(before["chain_off"], before["chains"], before["cseed_off"], before["cseeds"], bases, off, cseed_score=before["cseed_score"])
        want = (h["reg_off"], h["regs"]) if dflags == 0 else _live(h["reg_off"], h["regs"])
        _same_regs(got, *want, (name, pname))
        assert r["n_regs"] == want[1].size and h["regs"].size > 1000
        if pname == "default":
            g_off, g_regs = _golden(name)[3:]
            _same_regs(got, *((g_off, g_regs) if dflags == 0 else _live(g_off, g_regs)), (name, "golden"))
        ins = set(fd[k] for k in ("chain_off", "chains", "cseed_off", "cseeds", "cseed_score")) | {d_b, d_o}
        assert r["reg_off"] and r["regs"] and r["reg_off"] != r["regs"] and {r["reg_off"], r["regs"]}.isdisjoint(ins)
        eng.free(d_b); eng.free(d_o)
    al.close(); host.close(); chainer.close()


@gpu
@pytest.mark.parametrize("name", ["sorted150", "indel150_400", "long90", "gap3k"])
def test_dedup_of_the_compacted_regions_is_the_references(eng, dev, name):
    """cs_dedup_regions starts by the filter the compaction applies (dedup.cpp, comp_seed.cpp:2387-2393): the compacted result and the
    full one de-duplicate to the same regions, the reference's own (tests/golden/ddp1)"""
    import compseed_amd as ca
    batch, bases, off, _, _ = _golden(name)
    zd = np.load(os.path.join(DDP, name + ".ddp.npz"))
    d = dev.chains(*batch[:4])
    d_sc, d_b, d_o = dev.up(batch[4]), dev.up(bases), dev.up(off)
    al = ca.Aligner(_data.PREFIX, 0)
    full = ca.download_regions(eng, al.extend_chains_device(d, d_b, d_o, d_cseed_score=d_sc))
    compact = ca.download_regions(eng, al.extend_chains_device(d, d_b, d_o, d_cseed_score=d_sc, flags=ca.ALN_DEV_COMPACT))
    assert compact["regs"].size < full["regs"].size
    dd = al.dedup_regions(compact["reg_off"], compact["regs"], bases, off)
    df = al.dedup_regions(full["reg_off"], full["regs"], bases, off)
    al.close()
    assert np.array_equal(dd["reg_off"], zd["reg_off"]) and np.array_equal(dd["n_comp"], zd["reg_n_comp"])
    for f in FIELDS[:-1]:
        assert np.array_equal(dd["regs"][f], zd["reg_" + f]), (name, f)
    assert np.array_equal(dd["regs"]["frac_rep"].view(np.uint32), zd["reg_frac_rep"].view(np.uint32))
    for k in ("reg_off", "regs", "n_comp"):
        assert dd[k].tobytes() == df[k].tobytes(), (name, k)


def _two_chain_batch():
    """the first read of sorted150 with its first chain, once as it is and once emptied (tests/test_gpu_align.py: test_degenerate_inputs)"""
    import compseed_amd as ca
    batch, bases, off, _, _ = _golden("sorted150")
    n0 = int(batch[1]["n_seeds"][0])
    chains = np.zeros(2, dtype=ca.CHAIN_DT)
    chains[:] = batch[1][0]
    chains["n_seeds"] = [n0, 0]
    return (np.array([0, 2], np.uint64), chains, np.array([0, n0, n0], np.uint64), batch[3][:n0].copy(), batch[4][:n0].copy()), bases[:int(off[1])].copy(), off[:2].copy(), n0


def _ann_l_pac(prefix):
    return int(open(prefix + ".ann").read().split()[0])


@gpu
def test_checking_kernels_refuse_inconsistent_device_input(eng, dev):
    """each bad batch is one call that must return CS_EINVAL without following the bad value; the aligner serves the next call"""
    import compseed_amd as ca
    (chain_off, chains, cseed_off, cseeds, score), bases, off, n0 = _two_chain_batch()
    assert n0 >= 2
    al, host = ca.Aligner(_data.PREFIX, 0), ca.Aligner(_data.PREFIX, 0)
    good = host.extend_chains(chain_off, chains, cseed_off, cseeds, bases, off, cseed_score=score)
    assert good["regs"].size == n0
    d_b, d_sc, d_o = dev.up(bases), dev.up(score), dev.up(off)
    d_good = dev.chains(chain_off, chains, cseed_off, cseeds)
    five = chains.copy(); five["n_seeds"] = [n0, 5]
    far = cseeds.copy(); far["rbeg"][0] = 2 * _ann_l_pac(_data.PREFIX)

    def u64(*v):
        return np.array(v, np.uint64)

    bad = [("cseed_off that does not match n_seeds", dev.chains(chain_off, chains, u64(0, n0 - 1, n0), cseeds), d_o),
           ("chain_off decreasing", dev.chains(u64(2, 0), chains, cseed_off, cseeds), d_o),
           ("chain_off[n] above n_chains", dev.chains(u64(0, 3), chains, cseed_off, cseeds), d_o),
           ("cseed_off[n_chains] above n_seeds", dev.chains(chain_off, five, u64(0, n0, n0 + 5), cseeds), d_o),
           ("decreasing read_offsets", d_good, dev.up(u64(int(off[1]), 0))),
           ("read_offsets that do not start at 0", d_good, dev.up(u64(5, 5 + int(off[1])))),
           ("a read with chains of 65,536 bases", d_good, dev.up(u64(0, 65536))),
           ("a first seed at 2 * l_pac", dev.chains(chain_off, chains, cseed_off, far), d_o)]
    for what, d, d_off in bad:
        for dflags in DEV_FLAGS:
            with pytest.raises(ca.CSError) as ei:
                al.extend_chains_device(d, d_b, d_off, d_cseed_score=d_sc, flags=dflags)
            assert ei.value.code == -1, what
        _same_regs(ca.download_regions(eng, al.extend_chains_device(d_good, d_b, d_o, d_cseed_score=d_sc)), good["reg_off"], good["regs"], what)
    _same_regs(ca.download_regions(eng, al.extend_chains_device(d_good, d_b, d_o, d_cseed_score=d_sc, flags=1)), *_live(good["reg_off"], good["regs"]))
    al.close(); host.close()


@gpu
@pytest.mark.parametrize("dflags", DEV_FLAGS)
def test_degenerate_batches_give_the_host_calls_results(eng, dev, dflags):
    import compseed_amd as ca
    al, host = ca.Aligner(_data.PREFIX, 0), ca.Aligner(_data.PREFIX, 0)
    z = np.zeros

    def both(chain_off, chains, cseed_off, cseeds, bases, off, score, d=None):
        h = host.extend_chains(chain_off, chains, cseed_off, cseeds, bases, off, cseed_score=score)
        d = d or dev.chains(chain_off, chains, cseed_off, cseeds)
        r = al.extend_chains_device(d, dev.up(bases), dev.up(off), d_cseed_score=None if score is None else dev.up(score), flags=dflags)
        want = (h["reg_off"], h["regs"]) if dflags == 0 else _live(h["reg_off"], h["regs"])
        assert r["n_reads"] == off.size - 1 and r["n_regs"] == want[1].size
        _same_regs(ca.download_regions(eng, r), *want)
        return h

    # no reads: with device arrays of one offset each, and with no arrays at all
    h = both(z(1, np.uint64), z(0, ca.CHAIN_DT), z(1, np.uint64), z(0, ca.SEED_DT), z(0, np.uint8), z(1, np.uint64), None)
    assert h["reg_off"].tolist() == [0] and h["regs"].size == 0
    r = al.extend_chains_device(dict(n_reads=0, n_chains=0, n_seeds=0, chain_off=None, chains=None, cseed_off=None, cseeds=None), None, None, flags=dflags)
    assert (r["n_reads"], r["n_regs"]) == (0, 0) and ca.download_regions(eng, r)["reg_off"].tolist() == [0]
    # three reads without chains
    bases, off = _data.load_reads("sorted150")
    h = both(z(4, np.uint64), z(0, ca.CHAIN_DT), z(1, np.uint64), z(0, ca.SEED_DT), bases[:int(off[3])], off[:4], None)
    assert h["reg_off"].tolist() == [0, 0, 0, 0]
    # a chain the seed test left without seeds beside one that kept its own; then the same without scores (score = len)
    (chain_off, chains, cseed_off, cseeds, score), b1, o1, n0 = _two_chain_batch()
    h = both(chain_off, chains, cseed_off, cseeds, b1, o1, score)
    assert h["regs"].size == n0
    both(chain_off, chains, cseed_off, cseeds, b1, o1, None)
    st_d, st_h = al.stats(), host.stats()
    assert {k: st_d[k] for k in COUNTERS} == {k: st_h[k] for k in COUNTERS}
    al.close(); host.close()


@gpu
def test_host_and_device_calls_share_an_aligner(eng, dev):
    import compseed_amd as ca
    batch, bases, off, reg_off, regs = _golden("main100")
    b2, bases2, off2, reg_off2, regs2 = _golden("ragged")
    d = dev.chains(*batch[:4])
    d_sc, d_b, d_o = dev.up(batch[4]), dev.up(bases), dev.up(off)
    al = ca.Aligner(_data.PREFIX, 0)
    for dflags in DEV_FLAGS:
        want = (reg_off, regs) if dflags == 0 else _live(reg_off, regs)
        _same_regs(ca.download_regions(eng, al.extend_chains_device(d, d_b, d_o, d_cseed_score=d_sc, flags=dflags)), *want, "device first")
        _same_regs(al.extend_chains(*b2[:4], bases2, off2, cseed_score=b2[4]), reg_off2, regs2, "host after device")
        _same_regs(ca.download_regions(eng, al.extend_chains_device(d, d_b, d_o, d_cseed_score=d_sc, flags=dflags)), *want, "device after host")
    al.close()
