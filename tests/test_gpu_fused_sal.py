"""The fused sort + SAL path (sort_expand16_kernel, sal_expand_heavy_kernel, the per-read seed counts taken while the mems are emitted)
against the oracle and against the same engine with `disable=fused_sal` (the two-pass sort, scan and sal_expand_kernel).

One small index: the golden tandem reference (tests/golden/g1: segmental copies, a 300-bp family, a 23-bp x 700 tandem array, a
homopolymer).  One batch of 2,007 reads (no multiple of 16), put together so that every path of the new kernels has reads to work on;
the classes are asserted from the oracle's output below.  The inputs come from numpy's PCG64 with a fixed seed, chosen with the oracle
on a CPU so that the classes hold.
"""
import numpy as np
import pytest

import _data
import _oracle

pytestmark = pytest.mark.gpu

N_READS = 2007
SEED = 20261018


def _make_reads():
    rng = np.random.default_rng(SEED)
    g = _data.load_pac_forward()
    reads = []

    def take(st, ln, p_sub=0.0, p_n=0.0, rc=False):
        q = g[st: st + ln].copy()
        if rc:
            q = (3 - q[::-1]).astype(np.uint8)
        if p_sub > 0:
            mut = rng.random(ln) < p_sub
            q[mut] = (q[mut] + rng.integers(1, 4, int(mut.sum()))).astype(np.uint8) % 4
        if p_n > 0:
            q[rng.random(ln) < p_n] = 4
        return q

    for j in range(1600):                                          # the bulk: 150 bp, 1 % substitutions, a few Ns
        reads.append(take(int(rng.integers(0, g.size - 150)), 150, 0.01, 0.002, bool(j & 1)))
    tandem = np.flatnonzero((g[:-23 * 3] == g[23:-23 * 2]) & (g[:-23 * 3] == g[23 * 2:-23]))  # inside the 23-bp array: x2 > max_occ
    t0, t1 = int(tandem[200]), int(tandem[-200])
    for j in range(120):
        reads.append(take(int(rng.integers(t0, t1 - 150)), 150, 0.01 if j % 3 else 0.0, 0.0, bool(j & 1)))
    for j in range(60):                                            # homopolymer / dinucleotide stretch: tens to hundreds of slots per mem
        reads.append(take(int(rng.integers(29900, 30300)), 150, 0.0, 0.0, bool(j & 1)))
    for j in range(100):                                           # 400-900 bp, exact: 17..64 mems (round 3 adds one every ~20 bases)
        ln = int(rng.integers(400, 901))
        reads.append(take(int(rng.integers(0, g.size - ln)), ln, 0.0, 0.0, bool(j & 1)))
    for j in range(24):                                            # 2-5 kbp, exact: more than 64 mems, mems beyond `cap`
        ln = int(rng.integers(2000, 5001))
        reads.append(take(int(rng.integers(0, g.size - ln)), ln, 0.0, 0.0, bool(j & 1)))
    for j in range(40):                                            # all-N reads
        reads.append(np.full(int(rng.integers(30, 200)), 4, np.uint8))
    while len(reads) < N_READS:                                    # random reads: no mem (or hardly any)
        reads.append(rng.integers(0, 4, 150).astype(np.uint8))
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    bases = np.frombuffer(b"ACGTN", np.uint8)[np.concatenate(reads)]
    off = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.uint64)
    return bases, off


@pytest.fixture(scope="module")
def world():
    import compseed_amd as ca
    ix = ca.Index.load(_data.PREFIX)
    eng = ca.Engine(ix, 0)
    o = _oracle.OracleIndex(_data.PREFIX)
    bases, off = _make_reads()
    want = {}

    def oracle(**kw):                                              # one oracle run per parameter set, shared by the tests
        key = tuple(sorted(kw.items()))
        if key not in want:
            want[key] = o.seed_batch(bases, off, _oracle.make_params(**kw), mode=1, threads=8)
        return want[key]

    yield dict(ca=ca, ix=ix, eng=eng, bases=bases, off=off, oracle=oracle)
    o.close(); eng.close(); ix.close()


def _same(got, want):
    assert np.array_equal(got.mem_off, want["mem_off"]) and np.array_equal(got.mems, want["mems"])
    assert np.array_equal(got.seed_off, want["seed_off"]) and np.array_equal(got.seeds, want["seeds"])


def test_input_has_a_read_in_every_class(world):
    """from the oracle's output at the defaults: what the new kernels branch on is all there"""
    assert world["off"].size - 1 == N_READS and N_READS % 16 != 0
    w = world["oracle"]()
    n = np.diff(w["mem_off"].astype(np.int64))
    assert (n == 0).any() and ((n >= 1) & (n <= 16)).any() and ((n >= 17) & (n <= 64)).any() and (n > 64).any()
    x2 = w["mems"]["x2"]
    assert (x2 > 500).any()                                        # step > 1
    assert ((x2 >= 5) & (x2 <= 16)).any()                          # expanded by the 16 lanes of its group, one step
    assert ((x2 > 16) & (x2 <= 500)).any()                         # ... several steps
    assert ((x2 >= 1) & (x2 <= 4)).any()                           # by its own lane
    heavy = np.repeat(n > 64, n)
    assert (x2[heavy] > 4).any() and (x2[heavy] <= 4).any()        # both kinds inside the reads sal_expand_heavy_kernel takes
    for c in (3, 1):
        assert (world["oracle"](c=c)["mems"]["x2"] > c).any()


@pytest.mark.parametrize("kw", [dict(), dict(c=3), dict(c=1), dict(c=4), dict(c=5), dict(c=16), dict(c=17)],
                         ids=lambda kw: "-".join("%s%s" % kv for kv in kw.items()) or "defaults")
def test_fused_sal_vs_oracle_and_two_pass_path(world, kw):
    """c=3, c=1: x2 > max_occ for many mems and step > 1; c=4 / c=5: slot counts at and across SAL_LIGHT; c=16 / c=17: one group step and two"""
    ca, eng = world["ca"], world["eng"]
    got = eng.seed_batch(world["bases"], world["off"], ca.Params(**kw))
    _same(got, world["oracle"](**kw))
    old = eng.seed_batch(world["bases"], world["off"], ca.Params(disable=ca.disable_mask("fused_sal"), **kw))
    _same(old, world["oracle"](**kw))


def test_want_sal_0_gives_the_same_mems(world):
    ca, eng = world["ca"], world["eng"]
    got = eng.seed_batch(world["bases"], world["off"], ca.Params(want_sal=0))
    w = world["oracle"]()
    assert np.array_equal(got.mem_off, w["mem_off"]) and np.array_equal(got.mems, w["mems"])
    assert got.seeds is None and got.seed_off is None


def test_device_pipeline_two_in_flight(world):
    """submit_device / collect_device with two batches in flight on the two pass contexts; every result is downloaded before the next
    submit (a collected result is valid until the second submit from then)"""
    ca, eng = world["ca"], world["eng"]
    bases, off = world["bases"], world["off"]
    w = world["oracle"]()
    d_b, d_o = eng.alloc(bases.nbytes), eng.alloc(off.nbytes)
    try:
        eng.upload(d_b, bases); eng.upload(d_o, off)
        n, nb = off.size - 1, int(off[-1])

        def check(r):
            assert (r.n_reads, r.n_mems, r.n_seeds) == (n, w["mems"].size, w["seeds"].size)
            assert np.array_equal(eng.download(r.ptr["mem_off"], "<u8", n + 1), w["mem_off"])
            assert np.array_equal(eng.download(r.ptr["mems"], ca.INTV_DT, r.n_mems), w["mems"])
            assert np.array_equal(eng.download(r.ptr["seed_off"], "<u8", n + 1), w["seed_off"])
            assert np.array_equal(eng.download(r.ptr["seeds"], ca.SEED_DT, r.n_seeds), w["seeds"])

        for par in (ca.Params(), ca.Params(disable=ca.disable_mask("fused_sal"))):
            eng.submit_device(d_b, d_o, n, nb, par); eng.submit_device(d_b, d_o, n, nb, par)
            for _ in range(3):
                check(eng.collect_device())
                eng.submit_device(d_b, d_o, n, nb, par)
            check(eng.collect_device()); check(eng.collect_device())
    finally:
        eng.sync()
        eng.free(d_b); eng.free(d_o)


@pytest.mark.parametrize("opts", [dict(max_raw_mb=1), dict(mem_cap=8)], ids=["two_sub_batches", "mem_cap8"])
def test_sub_batches_and_small_cap(world, opts):
    """max_raw_mb=1: the batch goes through the stage in two sub-batches (1,024 + 983 reads), the running seed total continues from one to
    the next and d_seeds grows with its contents kept; mem_cap=8: most reads have mems beyond `cap` and take the wave kernels"""
    ca = world["ca"]
    eng = ca.Engine(world["ix"], 0, **opts)
    try:
        for kw in (dict(), dict(c=3)):
            _same(eng.seed_batch(world["bases"], world["off"], ca.Params(**kw)), world["oracle"](**kw))
            _same(eng.seed_batch(world["bases"], world["off"], ca.Params(disable=ca.disable_mask("fused_sal"), **kw)), world["oracle"](**kw))
    finally:
        eng.close()


def _fallback_reads():
    """1,024 reads whose round-3 seeds run the overflow records of their sub-batch full (220 exact reads of 10 kbp: ~440 mems beyond `cap`
    each against 1,024 * 4 + 65,536 records), then 1,000 ordinary reads"""
    rng = np.random.default_rng(SEED + 1)
    g = _data.load_pac_forward()
    reads = [g[st: st + 10000].copy() for st in rng.integers(0, g.size - 10000, 220)]
    reads += [g[st: st + 150].copy() for st in rng.integers(0, g.size - 150, 1024 - 220 + 1000)]
    bases = np.frombuffer(b"ACGTN", np.uint8)[np.concatenate(reads)]
    off = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.uint64)
    return bases, off


def test_fallback_in_the_first_sub_batch_then_a_split_sub_batch(world):
    """max_raw_mb=1: sub-batches of 1,024 reads.  The first one overflows its records and is redone by the fused kernel, which ends the
    fused sort + SAL for the call; the second goes through the split kernels and the sort alone, run_sal makes all seeds.  A small call
    before it leaves the context a d_salcnt far shorter than the mems of the first sub-batch."""
    ca = world["ca"]
    bases, off = _fallback_reads()
    o = _oracle.OracleIndex(_data.PREFIX)
    want = o.seed_batch(bases, off, _oracle.make_params(), mode=1, threads=8)
    o.close()
    n = np.diff(want["mem_off"].astype(np.int64))
    assert int(np.maximum(n[:1024] - 64, 0).sum()) > 1024 * 4 + 65536           # the records of the first sub-batch run full
    eng = ca.Engine(world["ix"], 0, max_raw_mb=1)
    try:
        eng.seed_batch(bases[-16 * 150:], np.arange(17, dtype=np.uint64) * np.uint64(150), ca.Params(disable=ca.disable_mask("fused_sal")))
        eng.reset_stats()
        got = eng.seed_batch(bases, off, ca.Params())
        assert eng.stats()["overflow_kernel_launches"] > 0                      # the fused kernel's second pass ran: the fallback was taken
        _same(got, want)
    finally:
        eng.close()


def test_max_occ_beyond_the_32_bit_seed_count_is_refused(world):
    """a read has fewer than 2^22 mems, so max_occ <= 1024 keeps a read's seed count in 32 bits; beyond that the call returns CS_ERANGE"""
    ca, eng = world["ca"], world["eng"]
    with pytest.raises(ca.CSError) as err:
        eng.seed_batch(world["bases"][: int(world["off"][16])], world["off"][:17], ca.Params(c=1025))
    assert err.value.code == -5                                                 # CS_ERANGE
    got = eng.seed_batch(world["bases"], world["off"], ca.Params(c=1024))
    _same(got, world["oracle"](c=1024))
