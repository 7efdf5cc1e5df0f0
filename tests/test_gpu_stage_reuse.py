"""One Chainer and one Aligner through a sequence of batches that no single stage test states: the largest golden run (the buffers
grow), an empty batch, the smallest run, a call the checking kernels refuse with CS_EINVAL, the first run again.  The device stages keep
their state in one shared layer (compseed_amd/csrc/dev_stage.hpp): a stream, timing events and pinned counter words that are destroyed
with the stage, and typed grow-only device buffers (DevBuf<T> members, grown by DevBuf::ensure, which frees before it allocates and keeps
no contents).  After every step each stage's result must be, byte for byte, what freshly created handles return for the same input.  The
chainer, the filter and the aligner's extension (chain_gpu.hip, chain_filter_gpu.hip, align_gpu.hip) are also held against the host calls
cs_chain_batch / cs_chain_filter, for the host-array forms and for the *_device forms chained on the device; then the handles close, and so
does a chainer whose filter state was never made.  The Extender (extend.hip) goes through a sequence of its own: its three host forms and
the device form on one handle.  The aligner's two later stages, cs_regions_mark (mark_gpu.hip) and cs_regions_cigar (cigar_gpu.hip), have a
leg each over the sets their own tests run, with the difference of the stage's statistics across every step compared as well."""
import functools

import numpy as np
import pytest

import _cigar
import _data
import _mark
import _oracle
from test_chain import golden_chains
from test_gpu_chain_device import _cp, _golden_in
from test_gpu_extend import TRACES, _random_pairs
from test_gpu_extend_chains_device import Dev, _same_regs

pytestmark = pytest.mark.gpu

CHAIN_KEYS = ("chain_off", "chains", "cseed_off", "cseeds")
FLT_KEYS = CHAIN_KEYS + ("cseed_score",)
BIG = ("repeat100", "default")            # the golden run with the most seeds and chains (120 reads)
SMALL = ("ragged", "default")              # a sixth of its chains, but 300 reads: the per-read buffers grow when the others need not
STEPS = [BIG, None, SMALL, "refused", BIG]                                           # None: the batch without reads


def _same(a, b, keys, what):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


@functools.lru_cache(maxsize=None)
def _batch(run):
    """-> (mem_off, mems, seed_off, seeds), bases, read offsets, chain parameters of a golden run, or of the batch without reads"""
    import compseed_amd as ca
    if run is None:
        z8 = np.zeros(1, np.uint64)
        return (z8, np.zeros(0, ca.INTV_DT), z8, np.zeros(0, ca.SEED_DT)), np.zeros(0, np.uint8), z8, ca.ChainParams()
    z, kw = _data.load_golden(*run)
    bases, off = _data.load_reads(run[0])
    mem_off, mems, seed_off, seeds = _golden_in(z)
    return (np.ascontiguousarray(mem_off, np.uint64), mems, np.ascontiguousarray(seed_off, np.uint64), seeds), bases, off, _cp(kw)


class _DevSeeds:
    """golden seeds in device memory, in the form Chainer.chain_device takes an on-device Result"""

    def __init__(self, dev, seeds_in, n_seeds=None):
        mem_off, mems, seed_off, seeds = seeds_in
        self.n_reads, self.n_mems, self.n_seeds = mem_off.size - 1, mems.size, seeds.size if n_seeds is None else n_seeds
        self.ptr = dict(mem_off=dev.up(mem_off), mems=dev.up(mems), seed_off=dev.up(seed_off), seeds=dev.up(seeds))


def _host_pass(chainer, al, run):
    """chain_gpu -> filter_gpu -> extend_chains over host arrays"""
    seeds_in, bases, off, cp = _batch(run)
    ch = chainer.chain_gpu(*seeds_in, off, cp)
    fl = chainer.filter_gpu(*(ch[k] for k in CHAIN_KEYS), bases, off)
    return ch, fl, al.extend_chains(*(fl[k] for k in CHAIN_KEYS), bases, off, cseed_score=fl["cseed_score"])


def _device_pass(eng, dev, chainer, al, run):
    """chain_device -> filter_device -> extend_chains_device, every stage reading the one before it in device memory"""
    import compseed_amd as ca
    seeds_in, bases, off, cp = _batch(run)
    d_b, d_o = dev.up(bases), dev.up(off)
    d = chainer.chain_device(_DevSeeds(dev, seeds_in), d_o, cp)
    ch = ca.download_chains(eng, d)
    fd = chainer.filter_device(d, d_b, d_o)
    fl = ca.download_chains(eng, fd)
    r = al.extend_chains_device(fd, d_b, d_o)
    assert (d["n_reads"], fd["n_reads"], r["n_reads"]) == (off.size - 1,) * 3 and r["n_regs"] == fl["cseeds"].size
    return ch, fl, ca.download_regions(eng, r)


@pytest.fixture(scope="module")
def eng():
    import compseed_amd as ca
    ix = ca.Index.load(_data.PREFIX)
    e = ca.Engine(ix, 0)
    yield e
    e.close()
    ix.close()


@pytest.fixture(scope="module")
def fresh(eng):
    """run -> the three results of fresh handles (host-array forms and device forms) and of the host calls; computed once per run"""
    import compseed_amd as ca
    cache = {}

    def get(run):
        if run not in cache:
            seeds_in, bases, off, cp = _batch(run)
            chainer, al = ca.Chainer(_data.PREFIX, device=0), ca.Aligner(_data.PREFIX, 0)
            by_host_arrays = _host_pass(chainer, al, run)
            host_ch = chainer.chain(*seeds_in, off, cp, threads=4)
            host_fl = chainer.filter(*(host_ch[k] for k in CHAIN_KEYS), bases, off, threads=4)
            chainer.close(); al.close()
            chainer, al, dev = ca.Chainer(_data.PREFIX, device=0), ca.Aligner(_data.PREFIX, 0), Dev(eng)
            by_device_arrays = _device_pass(eng, dev, chainer, al, run)
            dev.free(); chainer.close(); al.close()
            for got in (by_host_arrays, by_device_arrays):
                _same(got[0], host_ch, CHAIN_KEYS, (run, "fresh chainer against cs_chain_batch"))
                _same(got[1], host_fl, FLT_KEYS, (run, "fresh chainer against cs_chain_filter"))
            _same_regs(by_device_arrays[2], by_host_arrays[2]["reg_off"], by_host_arrays[2]["regs"], (run, "fresh aligners"))
            cache[run] = (host_ch, host_fl, by_host_arrays[2])
        return cache[run]
    return get


def _check(got, want, what):
    _same(got[0], want[0], CHAIN_KEYS, (what, "chains"))
    _same(got[1], want[1], FLT_KEYS, (what, "filtered chains"))
    _same_regs(got[2], want[2]["reg_off"], want[2]["regs"], (what, "regions"))


def _refused(call, what):
    import compseed_amd as ca
    with pytest.raises(ca.CSError) as ei:
        call()
    assert ei.value.code == -1, what


def _seed_off_decreasing(seed_off):
    """a copy in which one read's seeds end before they begin (the next read takes them: nothing reaches beyond n_seeds)"""
    bad = seed_off.copy()
    r = int(np.nonzero(bad[:-2] > 0)[0][0])
    bad[r + 1] = bad[r] - np.uint64(1)
    return bad


def _cseed_off_beyond(cseed_off):
    bad = cseed_off.copy()
    bad[-1] += np.uint64(1)                                   # the last chain ends one seed behind n_seeds
    return bad


def test_the_runs_differ_in_size():
    big, small = _batch(BIG), _batch(SMALL)
    assert BIG == max(_data.golden_runs(), key=lambda run: golden_chains(*run)["pos"].size)
    assert big[0][3].size > 2 * small[0][3].size and golden_chains(*BIG)["pos"].size > 2 * golden_chains(*SMALL)["pos"].size > 0
    assert big[2].size < small[2].size
    # ... and the later stages' sets: (reads, regions, most regions a read, longest read)
    shape = lambda x: (x[0].size - 1, x[1].size, int(np.diff(x[0].astype(np.int64)).max()), int(np.diff(x[3].astype(np.int64)).max()))
    assert shape(_regions("repeat100"))[:3] == (120, 30006, 501) and shape(_regions("main100"))[:2] == (3000, 4561)
    assert shape(_regions("gap3k"))[:2] == (120, 222) and shape(_regions("gap3k"))[3] == 3712 > 1024 > shape(_regions("main100"))[3]


def test_host_array_forms_on_reused_handles(fresh):
    import compseed_amd as ca
    chainer, al = ca.Chainer(_data.PREFIX, device=0), ca.Aligner(_data.PREFIX, 0)
    for i, run in enumerate(STEPS):
        if run == "refused":
            seeds_in, bases, off, cp = _batch(BIG)
            ch, fl, _ = fresh(BIG)
            _refused(lambda: chainer.chain_gpu(seeds_in[0], seeds_in[1], _seed_off_decreasing(seeds_in[2]), seeds_in[3], off, cp), "seed_off decreasing")
            _refused(lambda: chainer.filter_gpu(ch["chain_off"], ch["chains"], _cseed_off_beyond(ch["cseed_off"]), ch["cseeds"], bases, off), "cseed_off beyond n_seeds")
            _refused(lambda: al.extend_chains(fl["chain_off"], fl["chains"], _cseed_off_beyond(fl["cseed_off"]), fl["cseeds"], bases, off, cseed_score=fl["cseed_score"]),
                     "cseed_off beyond n_seeds")
            continue
        _check(_host_pass(chainer, al, run), fresh(run), (i, run))
    chainer.close(); al.close()
    assert not chainer._h


def test_device_forms_on_reused_handles(eng, fresh):
    import compseed_amd as ca
    chainer, al, dev = ca.Chainer(_data.PREFIX, device=0), ca.Aligner(_data.PREFIX, 0), Dev(eng)
    for i, run in enumerate(STEPS):
        if run == "refused":
            seeds_in, bases, off, cp = _batch(BIG)
            ch, fl, _ = fresh(BIG)
            d_b, d_o = dev.up(bases), dev.up(off)
            _refused(lambda: chainer.chain_device(_DevSeeds(dev, seeds_in, n_seeds=seeds_in[3].size - 1), d_o, cp), "n_seeds below seed_off[n_reads]")
            bad_ch = dev.chains(ch["chain_off"], ch["chains"], _cseed_off_beyond(ch["cseed_off"]), ch["cseeds"])
            _refused(lambda: chainer.filter_device(bad_ch, d_b, d_o), "cseed_off beyond n_seeds")
            bad_fl = dev.chains(fl["chain_off"], fl["chains"], _cseed_off_beyond(fl["cseed_off"]), fl["cseeds"])
            _refused(lambda: al.extend_chains_device(bad_fl, d_b, d_o, d_cseed_score=dev.up(fl["cseed_score"])), "cseed_off beyond n_seeds")
            continue
        _check(_device_pass(eng, dev, chainer, al, run), fresh(run), (i, run))
        dev.free()
    dev.free(); chainer.close(); al.close()


def test_a_chainer_without_filter_state_closes():
    import compseed_amd as ca
    seeds_in, _, off, cp = _batch(SMALL)
    chainer = ca.Chainer(_data.PREFIX, device=0)
    assert chainer.chain_gpu(*seeds_in, off, cp)["chains"].size > 0 and chainer.filter_stats()["reads"] == 0
    chainer.close()
    assert not chainer._h
    never_used = ca.Chainer(_data.PREFIX, device=0)
    never_used.close()


EXT_BIG, EXT_OTHER = "indel150.default", "sorted150.default"   # the recorded run with the most pairs and the most sequence bytes; one with other buffer sizes


def _ext_pairs(pairs):
    import compseed_amd as ca
    pr = np.zeros(pairs.size, dtype=ca.EXT_PAIR_DT)
    for f in ("q_off", "t_off", "qlen", "tlen", "h0"):
        pr[f] = pairs[f]
    return pr


def _ext_oracle(pairs, qbuf, tbuf, w):
    """the oracle under mem_opt_init's scoring (what Extender(0) computes) at band w"""
    import compseed_amd as ca
    P = ca.ExtParams()
    meta = np.tile(np.array([[0, w, P.zdrop, P.end_bonus, P.o_del, P.e_del, P.o_ins, P.e_ins] + [0] * 9], dtype=np.int32), (pairs.size, 1))
    fx = dict(mat=np.array(list(P.mat), dtype=np.int8), pairs=pairs, qbuf=qbuf, tbuf=tbuf, meta=meta)
    return _oracle.bsw_extend(fx, threads=8).astype(ca.EXT_RES_DT)


def _mixed_batch():
    """40 pairs of 1..300 columns (either side of the 160 columns the lane kernel takes) and three of 9,000..12,000 (beyond what the
    wave-per-pair kernel keeps in LDS: the band state goes to HBM)"""
    rng = np.random.default_rng(20)
    p0, q0, t0 = _random_pairs(rng, 40, 1, 300)
    p1, q1, t1 = _random_pairs(rng, 3, 9000, 12000)
    p1["q_off"] += q0.size; p1["t_off"] += t0.size
    pairs = np.concatenate([p0, p1])
    assert (pairs["qlen"] <= 160).any() and ((pairs["qlen"] > 160) & (pairs["qlen"] <= 300)).any() and (pairs["qlen"] >= 9000).sum() == 3
    return pairs, np.concatenate([q0, q1]), np.concatenate([t0, t1])


def test_the_extender_on_a_reused_handle(eng):
    """One Extender through: the biggest recorded run (the buffers grow), an empty batch, a small mixed batch whose three long queries bring
    the HBM band state onto a used handle, a batch with four bad pairs (CS_EINVAL, the others delivered, the bad ones zero), an upload and
    three resident pair lists (all pairs at w = 100, fifty at w = 13, all again), another run through extend() and then extend_resident()
    with NO upload in between, the device form, close.  Every result is, byte for byte, what a fresh Extender's extend() returns for the same
    input and what the recorded run or the oracle says.  The resident call without an upload pins the rule that a host-form call leaves
    its sequences resident (include/compseed_amd.h): it must run against the second run's buffers and their sizes, not the uploaded ones."""
    import compseed_amd as ca
    big, other = _oracle.bsw_fixture(EXT_BIG), _oracle.bsw_fixture(EXT_OTHER)
    assert all(big[k].size > _oracle.bsw_fixture(tag)[k].size for tag in TRACES if tag != EXT_BIG for k in ("pairs", "qbuf", "tbuf"))
    pr_big, pr_other = _ext_pairs(big["pairs"]), _ext_pairs(other["pairs"])
    want_big, want_other = big["want"].astype(ca.EXT_RES_DT), other["want"].astype(ca.EXT_RES_DT)
    x = ca.Extender(0)
    delivered = 0

    def step(what, call, args, want, fresh_args=None):
        """call(handle, *args) on the reused handle against extend(*fresh_args or args) on a fresh one, and against `want`"""
        nonlocal delivered
        got = call(x, *args)
        fresh = ca.Extender(0)
        ref = fresh.extend(*(fresh_args or args))
        fresh.close()
        assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes(), (what, "reused handle against a fresh one")
        assert np.array_equal(got, want), (what, int((got != want).sum()))
        delivered += got.size

    host = ca.Extender.extend
    resident = ca.Extender.extend_resident
    step("big host batch", host, (pr_big, big["qbuf"], big["tbuf"], 100), want_big)
    step("empty batch", host, (pr_big[:0], big["qbuf"], big["tbuf"], 100), want_big[:0])
    mixed, mq, mt = _mixed_batch()
    step("small mixed batch", host, (_ext_pairs(mixed), mq, mt, 100), _ext_oracle(mixed, mq, mt, 100))
    # the refused call of test_gpu_extend.test_device_variant_and_errors
    bad = pr_other[:50].copy()
    bad["q_off"][3] = other["qbuf"].size; bad["qlen"][7] = 0; bad["tlen"][11] = -1; bad["t_off"][13] = 2**40
    ok = np.ones(50, bool); ok[[3, 7, 11, 13]] = False
    fresh, outs = ca.Extender(0), []
    for h in (x, fresh):
        with pytest.raises(ca.CSError) as ei:
            h.extend(bad, other["qbuf"], other["tbuf"], 100)
        assert ei.value.code == -1 and "4 pair(s)" in str(ei.value)
        outs.append(h.last_out)
    fresh.close()
    assert outs[0].tobytes() == outs[1].tobytes(), "refused batch: reused handle against a fresh one"
    assert np.array_equal(outs[0][ok], want_other[:50][ok]) and (outs[0][~ok].view(np.int32) == 0).all()
    delivered += 50
    # upload, then three pair lists against the resident sequences
    x.upload(big["qbuf"], big["tbuf"])
    sub = np.arange(7, pr_big.size, pr_big.size // 50)[:50]
    want_sub = _ext_oracle(big["pairs"][sub], big["qbuf"], big["tbuf"], 13)
    step("resident, all pairs", resident, (pr_big, 100), want_big, (pr_big, big["qbuf"], big["tbuf"], 100))
    step("resident, 50 pairs at w = 13", resident, (pr_big[sub], 13), want_sub, (pr_big[sub], big["qbuf"], big["tbuf"], 13))
    step("resident, all pairs again", resident, (pr_big, 100), want_big, (pr_big, big["qbuf"], big["tbuf"], 100))
    # another run through the host form, then resident without an upload: the host form's sequences are the resident ones
    step("other host batch", host, (pr_other, other["qbuf"], other["tbuf"], 100), want_other)
    step("resident after a host batch, no upload", resident, (pr_other, 100), want_other, (pr_other, other["qbuf"], other["tbuf"], 100))
    # the device form on the same handle, the caller's arrays
    n = pr_big.size
    d_p, d_q, d_t, d_o = eng.alloc(pr_big.nbytes), eng.alloc(big["qbuf"].size), eng.alloc(big["tbuf"].size), eng.alloc(n * 24)
    eng.upload(d_p, pr_big); eng.upload(d_q, big["qbuf"]); eng.upload(d_t, big["tbuf"])
    x.extend_device(d_p, n, d_q, big["qbuf"].size, d_t, big["tbuf"].size, d_o, 100)
    got = eng.download(d_o, ca.EXT_RES_DT, n)
    for d in (d_p, d_q, d_t, d_o):
        eng.free(d)
    assert np.array_equal(got, want_big), "device form"
    delivered += n
    assert x.stats()["pairs"] == delivered == 4 * pr_big.size + 2 * pr_other.size + 43 + 50 + 50   # (the refused batch counts: its other results were delivered)
    x.close()
    assert not x.h
    never_used = ca.Extender(0)
    never_used.close()


# ---- the aligner's later stages: cs_regions_mark and cs_regions_cigar on one Aligner each, default parameters throughout
MARK_STEPS = ["repeat100", None, "main100", "refused", "repeat100"]   # per-region buffers and the wave path grow; then the per-read ones alone (3,000 reads of 4,561 regions)
CIGAR_STEPS = ["main100", None, "gap3k", "refused", "main100"]        # gap3k: few regions, but H / E rows beyond the LDS rows and the largest backtrack scratch


def _regions(name):
    """reg_off, regs, bases, read offsets of a set, or of the batch without reads"""
    if name is None:
        reg_off, regs, bases, off, _ = _cigar.load("main100")
        return reg_off[:1], regs[:0], bases[:0], off[:1]
    return _cigar.load(name)[:4]


def _reg_off_decreasing(reg_off):
    """a copy with one entry below its predecessor (the next read takes the regions: nothing reaches beyond n_regs)"""
    bad = reg_off.copy()
    r = int(np.nonzero(bad[:-2] > 0)[0][0])
    bad[r + 1] = bad[r] - np.uint64(1)
    return bad


def _stats_step(before, after):
    return {k: after[k] - before[k] for k in after if k != "kernel_ms"}   # (kernel_ms is a time)


def _later_stage_leg(steps, call, stats, same):
    """`steps` on one Aligner; after each the result and the step's share of the statistics are a fresh Aligner's"""
    import compseed_amd as ca
    al = ca.Aligner(_data.PREFIX, 0)
    try:
        for i, name in enumerate(steps):
            if name == "refused":
                reg_off, regs, bases, off = _regions(steps[0])
                _refused(lambda: call(al, _reg_off_decreasing(reg_off), regs, bases, off), "reg_off decreasing")
                continue
            before = stats(al)
            got = call(al, *_regions(name))
            fresh = ca.Aligner(_data.PREFIX, 0)
            try:
                want = call(fresh, *_regions(name))
                zero = dict.fromkeys(before, 0)                                   # (a stage that has not run reports zeroes)
                assert _stats_step(before, stats(al)) == _stats_step(zero, stats(fresh)), (i, name)
            finally:
                fresh.close()
            same(got, want, (i, name))
    finally:
        al.close()


def test_regions_mark_on_a_reused_aligner():
    _later_stage_leg(MARK_STEPS, lambda al, reg_off, regs, bases, off: al.regions_mark(reg_off, regs, off), lambda al: al.mark_stats(), _mark.same_bytes)


def test_regions_cigar_on_a_reused_aligner():
    def same(got, want, what):
        for k in ("alns", "cigar", "md"):
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)
    _later_stage_leg(CIGAR_STEPS, lambda al, reg_off, regs, bases, off: al.regions_cigar(reg_off, regs, bases, off), lambda al: al.cigar_stats(), same)
