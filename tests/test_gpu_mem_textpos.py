"""The text position of a unique mem in the spare bits of its raw record (fm_device.hpp MEM_POS_TAG) and in the side word of its
re-seeding call (smem_common.hpp AUX_POS): fwd0_kernel, fwd_kernel and r3text_kernel write it, r2text_kernel, r3text_kernel and
sort_expand16_kernel use it in the place of a suffix-array read, every other reader of raw records decodes it.  Results never depend on
it and no tagged word leaves the sort, so the specification is the reference's golden vectors and the oracle; `disable=mem_pos` is the
A/B inside one build."""
import numpy as np
import pytest

import _data
import _oracle
from test_gpu_parity import _check_against_golden, _expand_packed
from test_gpu_r3text_fused import _many_mem_reads

pytestmark = pytest.mark.gpu

ENGINES = {"isa32": dict(), "sa64": dict(sa64=1), "sa40": dict(sa40=1)}
TOP = np.uint64(63)


def _untagged(mems):
    assert not (mems["x2"] >> TOP).any()


def _same(got, want, sal=True):
    _untagged(got.mems)
    assert np.array_equal(got.mem_off, want["mem_off"]) and np.array_equal(got.mems, want["mems"])
    if sal:
        assert np.array_equal(got.seed_off, want["seed_off"]) and np.array_equal(got.seeds, want["seeds"])


@pytest.fixture(scope="module")
def ix():
    import compseed_amd as ca
    i = ca.Index.load(_data.PREFIX)
    yield i
    i.close()


@pytest.fixture(scope="module")
def eng(ix):
    import compseed_amd as ca
    e = ca.Engine(ix, 0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def many():
    """the batch of tests 3, 5 and 6 and the oracle's result, made once: reads of seven or eight unique pieces, so nearly every mem of
    rounds 1 and 3 is a unique one whose emitter holds its position"""
    bases, off, want = _many_mem_reads()
    x2 = want["mems"]["x2"]
    assert int((x2 == 1).sum()) * 10 > 9 * x2.size            # precondition: the batch is made of unique mems
    return bases, off, want


# ------------------------------------------------------------------------------------------------------------------ 1. goldens
@pytest.mark.parametrize("on", [True, False], ids=["mem_pos", "disabled"])
@pytest.mark.parametrize("kind", list(ENGINES))
def test_goldens_on_all_engines(ix, kind, on):
    """every golden run bit-exact, and no bit 63 in any mem array that leaves the engine: the host call, the packed form unpacked, the
    device result read through gather_reads, and want_sal = 0"""
    import compseed_amd as ca
    dis = 0 if on else ca.disable_mask("mem_pos")
    e = ca.Engine(ix, 0, **ENGINES[kind])
    try:
        for name, pname in _data.golden_runs():
            z, kw = _data.load_golden(name, pname)
            bases, off = _data.load_reads(name)
            n = off.size - 1
            zm = z["mems"]
            res = e.seed_batch(bases, off, ca.Params(disable=dis, **kw))
            _untagged(res.mems)
            _check_against_golden(res, z)
            p = e.seed_batch_packed(bases, off, ca.Params(disable=dis, **kw))
            mems, seeds = _expand_packed(p)
            _untagged(mems)
            assert np.array_equal(p["mem_off"], z["mem_off"]) and np.array_equal(p["seed_off"], z["seed_off"])
            assert np.array_equal(np.stack([mems["x0"], mems["x1"], mems["x2"], mems["info"]], axis=1), zm)
            assert np.array_equal(seeds["rbeg"], z["seed_rbeg"]) and np.array_equal(seeds["qbeg"], z["seed_qbeg"]) and np.array_equal(seeds["len"], z["seed_len"])
            d_b = e.alloc(bases.nbytes + 64); d_o = e.alloc(off.nbytes)
            try:
                e.upload(d_b, bases); e.upload(d_o, off)
                dev = e.seed_batch_device(d_b, d_o, n, bases.size, ca.Params(disable=dis, **kw))
                assert dev.n_mems == zm.shape[0] and dev.n_seeds == z["seed_rbeg"].size
                g = e.gather_reads(np.arange(n, dtype=np.uint64))
                _untagged(g.mems)
                _check_against_golden(g, z)
            finally:
                e.free(d_b); e.free(d_o)
            nos = e.seed_batch(bases, off, ca.Params(want_sal=0, disable=dis, **kw))
            _untagged(nos.mems)
            m = nos.mems
            assert nos.seeds is None and np.array_equal(nos.mem_off, z["mem_off"])
            assert np.array_equal(np.stack([m["x0"], m["x1"], m["x2"], m["info"]], axis=1), zm)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------ 2. digests
def test_digests_with_each_site_switched_off(eng):
    """main100 (3,000 fixture reads): the device-side digests of all four result arrays are the same with the tags on, off, under the literal
    algorithm, and with every kernel that writes or reads a tag switched off on its own while the others go on"""
    import compseed_amd as ca
    bases, off = _data.load_reads("main100")
    z, kw = _data.load_golden("main100", "default")
    _check_against_golden(eng.seed_batch(bases, off, ca.Params(**kw)), z)          # the digest below is the golden result's
    want = eng.result_digest()
    for par in (dict(disable=ca.disable_mask("mem_pos")), dict(sst_mode=0)):
        eng.seed_batch(bases, off, ca.Params(**kw, **par), copy=False)
        assert eng.result_digest() == want, par
    for site in ("text_mode", "text_sweep", "r2_text", "r3_text", "fwd0", "fused_sal"):
        eng.seed_batch(bases, off, ca.Params(disable=ca.disable_mask(site), **kw), copy=False)
        assert eng.result_digest() == want, site


# ------------------------------------------------------------------------------------------------------------------ 3. the other sort paths
def test_tagged_mems_as_overflow_records(ix, many):
    """mem_cap 8: the reads have more mems than that, so tagged mems of r3text_kernel and fwd_kernel travel as overflow records and are
    decoded by sort_compact_wave_kernel (mem_at); seeds by sal_expand_heavy_kernel, and by run_sal with the fused path off"""
    import compseed_amd as ca
    bases, off, want = many
    assert int(np.diff(want["mem_off"].astype(np.int64)).min()) > 8
    e = ca.Engine(ix, 0, mem_cap=8)
    try:
        e.reset_stats()
        _same(e.seed_batch(bases, off), want)
        assert e.stats()["overflow_mems"] > 0 and e.stats()["r3_text_seeds"] > 0
        _same(e.seed_batch(bases, off, ca.Params(disable=ca.disable_mask("fused_sal"))), want)
        _same(e.seed_batch(bases, off, ca.Params(want_sal=0)), want, sal=False)
    finally:
        e.close()


@pytest.fixture(scope="module")
def tandem():
    """24 reads of 1.5 to 2.5 kbp across an end of the fixture's 23-bp x 700 tandem array, either strand: a unique flank of 1,300 bases or
    more (a unique round-3 seed every twenty bases: tagged mems) and then the array -- more than 64 mems each; behind them the fixture's
    repeat100 reads (tandem array and low-complexity stretch, up to 64 mems).  With the oracle's result, made once."""
    g = _data.load_pac_forward()
    c = (g[:-46] == g[23:-23]) & (g[:-46] == g[46:])
    idx = np.flatnonzero(c)
    brk = np.flatnonzero(np.diff(idx) > 1)
    starts, ends = np.concatenate([[0], brk + 1]), np.concatenate([brk, [idx.size - 1]])
    k = int(np.argmax(ends - starts))
    t0, t1 = int(idx[starts[k]]), int(idx[ends[k]]) + 46          # the array
    assert t1 - t0 == 23 * 700
    rng = np.random.default_rng(64)
    reads = []
    for j in range(24):
        ln = int(rng.integers(1500, 2501))
        flank = int(rng.integers(1300, ln - 100))
        st = t0 - flank if j & 2 else t1 - (ln - flank)
        q = g[st: st + ln]
        reads.append((3 - q[::-1]).astype(np.uint8) if j & 1 else q)
    bases = np.frombuffer(b"ACGT", np.uint8)[np.concatenate(reads)]
    rb, ro = _data.load_reads("repeat100")
    off = np.concatenate([[0], np.cumsum([r.size for r in reads]), bases.size + ro[1:].astype(np.int64)]).astype(np.uint64)
    bases = np.concatenate([bases, rb])
    o = _oracle.OracleIndex(_data.PREFIX)
    want = o.seed_batch(bases, off, _oracle.make_params(), mode=0, threads=4)
    o.close()
    return bases, off, want


def test_reads_with_more_than_64_mems(eng, tandem):
    """sort_compact_wave_kernel and sal_expand_heavy_kernel on reads whose raw lists hold tagged mems"""
    bases, off, want = tandem
    n = np.diff(want["mem_off"].astype(np.int64))
    heavy = np.repeat(n > 64, n)
    assert int((n > 64).sum()) >= 24 and (want["mems"]["x2"][heavy] == 1).any()   # unique mems inside the reads the wave kernels take
    _same(eng.seed_batch(bases, off), want)


@pytest.mark.parametrize("how", ["want_sal0", "no_fused_sal"])
def test_sort_compact16_and_run_sal(eng, many, tandem, how):
    """sort_compact16_kernel decodes the tagged records it sorts; run_sal expands the decoded mems"""
    import compseed_amd as ca
    par = dict(want_sal=0) if how == "want_sal0" else dict(disable=ca.disable_mask("fused_sal"))
    for bases, off, want in (many, tandem):
        _same(eng.seed_batch(bases, off, ca.Params(**par)), want, sal=par.get("want_sal", 1) != 0)


# ------------------------------------------------------------------------------------------------------------------ 4. edges of the position
def test_edges_of_the_position():
    """a random genome of 5,000 bases: the first and the last 60 bases and their reverse complements (P = 0, l_pac - 60, l_pac, seq_len - 60:
    the tag may not depend on P != 0), and a read with one substitution in the middle -- a tagged SMEM from fwd0_kernel at its start and an
    untagged unique SMEM from a backward kernel behind the substitution"""
    import compseed_amd as ca
    rng = np.random.default_rng(5000)
    fwd = rng.integers(0, 4, 5000).astype(np.uint8)
    rc = lambda q: (3 - q[::-1]).astype(np.uint8)
    first, last = fwd[:60], fwd[-60:]
    sub = fwd[1000:1150].copy()
    sub[75] = (sub[75] + 1) & 3
    reads = [first, last, rc(first), rc(last), sub, rc(sub)]
    bases = np.frombuffer(b"ACGT", np.uint8)[np.concatenate(reads)]
    off = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.uint64)
    o = _oracle.OracleIndex.build(fwd)
    want = o.seed_batch(bases, off, _oracle.make_params(), mode=0, threads=2)
    o.close()
    mo = want["mem_off"].astype(np.int64)
    so = want["seed_off"].astype(np.int64)
    whole = np.uint64(60)
    for r, pos in enumerate((0, 5000 - 60, 10000 - 60, 5000)):           # precondition: one unique SMEM over the whole read, at the edge
        m = want["mems"][mo[r]:mo[r + 1]]
        k = np.flatnonzero((m["info"] == whole) & (m["x2"] == 1))
        assert k.size == 1 and pos in want["seeds"]["rbeg"][so[r]:so[r + 1]]
    m = want["mems"][mo[4]:mo[5]]
    beg = (m["info"] >> np.uint64(32)).astype(np.int64)
    assert ((m["x2"] == 1) & (beg == 0)).any() and ((m["x2"] == 1) & (beg > 0)).any()
    ix = ca.Index.build(fwd, 0)
    try:
        for opts in (dict(), dict(sa64=1), dict(sa40=1)):
            e = ca.Engine(ix, 0, jump_k=8, **opts)
            try:
                for dis in (0, ca.disable_mask("mem_pos")):
                    _same(e.seed_batch(bases, off, ca.Params(disable=dis)), want)
            finally:
                e.close()
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------------------------ 5. lists that are not final
@pytest.mark.parametrize("opts", [dict(), dict(sa64=1)], ids=["isa32", "sa64"])
def test_lists_that_are_not_final(ix, many, opts):
    """r3_text_iter 1: r3text_kernel starts after the first iteration and reads lists the kernels of rounds 1/2 still append tagged and
    untagged mems to (it only looks below its snapshot of the counts)"""
    import compseed_amd as ca
    bases, off, want = many
    e = ca.Engine(ix, 0, r3_text_iter=1, **opts)
    try:
        e.reset_stats()
        _same(e.seed_batch(bases, off), want)
        assert e.stats()["r3_text_seeds"] > 0
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------ 6. the path really runs
def test_the_tags_save_suffix_array_reads(eng, many):
    """a counting pass with and without the tags: fewer sa_entry events in r2text_kernel and r3text_kernel, the same work otherwise"""
    import compseed_amd as ca
    bases, off, want = many
    seen = {}
    for name, dis in (("on", 0), ("off", ca.disable_mask("mem_pos"))):
        eng.reset_stats()
        _same(eng.seed_batch(bases, off, ca.Params(count_traffic=1, disable=dis)), want)
        k = eng.traffic_model()["kernels"]
        seen[name] = ({kn: k.get(kn, {}).get("events", {}).get("sa_entry", 0) for kn in ("r2text_kernel", "r3text_kernel")}, eng.stats())
    (sa_on, st_on), (sa_off, st_off) = seen["on"], seen["off"]
    print("sa_entry events with tags", sa_on, "without", sa_off)
    for kn in ("r2text_kernel", "r3text_kernel"):
        assert sa_off[kn] > 0 and sa_on[kn] < sa_off[kn], (kn, sa_on, sa_off)
    for key in ("r3_text_seeds", "reseed_text_calls", "mems", "seeds"):
        assert st_on[key] == st_off[key] and st_on[key] > 0, key
