"""cs_engine_submit_device / cs_engine_collect_device as a pipeline uses them: every legal order of submits and collects, results checked
at the LATEST moment the contract allows ("valid until the second submit after its collect", include/compseed_amd.h), consumers that work
on batch n while n+2 is seeded, a want_sal = 0, a refused and an empty batch in the stream, digest / gather after a drain, the documented
two-thread model, and the memory report.  Batches are slices of the golden runs with their run's own -k/-r/-y/-c/-s; the expected output is
the same slice of the committed golden, and every comparison is of whole arrays: mem_off, the four mem words, seed_off, seed rbeg / qbeg /
len.  No verdict depends on timing: a check is placed where the contract says the result is still valid, and the schedules that drain the
stream first (... C C then S S) have the overwriting batch collected before the check."""
import functools
import itertools
import os
import threading

import numpy as np
import pytest

import _data
from test_chain import check_chains, golden_chains
from test_chain_filter import ALN, check_filtered
from test_gpu_chain_device import ENGINE_RUNS, _cp

pytestmark = pytest.mark.gpu

# (reads, params, first read, one past the last): eight batches that differ in n_reads, n_mems and n_seeds, listed largest first
SLICES = [("main100", "k14", 0, 3000), ("main100", "default", 100, 2500), ("sorted150", "r1.0", 0, 1500), ("shuffled100", "default", 0, 1000),
          ("ragged", "default", 20, 250), ("repeat100", "c50s20", 0, 120), ("main100", "k25r2.5y5", 500, 560), ("main100", "y0", 1000, 1040)]
ORDER_A = [0, 1, 2, 3, 4, 5, 6, 7]          # strictly shrinking: no buffer grows after batch 0
ORDER_B = [7, 0, 6, 2, 5, 1, 4, 3]          # 40 -> 3000 -> 60 -> 1500 -> 120 -> 2400 -> 230 -> 1000 reads: grows and shrinks
EINVAL = -1


@functools.lru_cache(maxsize=None)
def _slice(i):
    """-> dict(kw, bases, off, n, want = (mem_off, mems[:, 4], seed_off, rbeg, qbeg, len)) of SLICES[i]; computed once, never modified"""
    name, pname, k0, k1 = SLICES[i]
    z, kw = _data.load_golden(name, pname)
    bases, off = _data.load_reads(name)
    mo, so = z["mem_off"].astype(np.int64), z["seed_off"].astype(np.int64)
    want = ((mo[k0:k1 + 1] - mo[k0]).astype(np.uint64), z["mems"][mo[k0]:mo[k1]], (so[k0:k1 + 1] - so[k0]).astype(np.uint64),
            z["seed_rbeg"][so[k0]:so[k1]], z["seed_qbeg"][so[k0]:so[k1]], z["seed_len"][so[k0]:so[k1]])
    for a in want:
        a.setflags(write=False)
    return dict(kw=kw, bases=bases[int(off[k0]):int(off[k1])].copy(), off=(off[k0:k1 + 1] - off[k0]).astype(np.uint64), n=k1 - k0, want=want)


def test_the_batches_differ_and_the_orders_are_what_they_claim():
    counts = [(_slice(i)["n"], _slice(i)["want"][1].shape[0], _slice(i)["want"][3].size) for i in range(len(SLICES))]
    assert len(SLICES) == 8 and min(c[0] for c in counts) == 40 and max(c[0] for c in counts) == 3000
    for k in range(3):
        assert len(set(c[k] for c in counts)) == 8
        assert all(counts[ORDER_A[j]][k] > counts[ORDER_A[j + 1]][k] for j in range(7))          # strictly shrinking in every array
    nb = [counts[i][0] for i in ORDER_B]
    assert nb[:3] == [40, 3000, 60] and all((nb[j + 1] > nb[j]) != (nb[j + 2] > nb[j + 1]) for j in range(6))  # up, down, up, ...


class Dev:
    """an engine with the eight batches uploaded (inputs stay untouched and alive until close)"""

    def __init__(self, passes):
        import compseed_amd as ca
        self.ix = ca.Index.load(_data.PREFIX)
        self.e = ca.Engine(self.ix, 0, passes_in_flight=passes)
        self.n_ctx = passes
        self.bufs = {}
        for i in range(len(SLICES)):
            s = _slice(i)
            d_b, d_o = self.e.alloc(s["bases"].nbytes + 64), self.e.alloc(s["off"].nbytes)
            self.e.upload(d_b, s["bases"]); self.e.upload(d_o, s["off"])
            self.bufs[i] = (d_b, d_o)
        self.e.sync()

    def submit(self, i, **pkw):
        import compseed_amd as ca
        s = _slice(i)
        kw = dict(s["kw"]); kw.update(pkw)
        self.e.submit_device(self.bufs[i][0], self.bufs[i][1], s["n"], s["bases"].size, ca.Params(**kw))

    def close(self):
        for d_b, d_o in self.bufs.values():
            self.e.free(d_b); self.e.free(d_o)
        self.e.close(); self.ix.close()


@pytest.fixture(scope="module")
def dev2():
    d = Dev(2)
    yield d
    d.close()


def _get(e, ptr, dt, n):
    return e.download(ptr, dt, n) if n else np.zeros(0, dtype=dt)


def check_result(e, r, i, sal=True, tag=None):
    """downloads the arrays r points to and compares them, whole, with the golden slice i"""
    import compseed_amd as ca
    s = _slice(i)
    mo_w, mm_w, so_w, rb_w, qb_w, ln_w = s["want"]
    assert (r.n_reads, r.n_mems) == (s["n"], mm_w.shape[0]), tag
    mo = e.download(r.ptr["mem_off"], np.uint64, s["n"] + 1)
    mm = _get(e, r.ptr["mems"], ca.INTV_DT, r.n_mems)
    assert np.array_equal(mo, mo_w), tag
    for k, f in enumerate(("x0", "x1", "x2", "info")):
        assert np.array_equal(mm[f], mm_w[:, k]), (tag, f)
    if not sal:
        assert not r.ptr["seed_off"] and not r.ptr["seeds"] and r.n_seeds == 0, tag
        return
    assert r.n_seeds == rb_w.size, tag
    so = e.download(r.ptr["seed_off"], np.uint64, s["n"] + 1)
    ss = _get(e, r.ptr["seeds"], ca.SEED_DT, r.n_seeds)
    assert np.array_equal(so, so_w), tag
    assert np.array_equal(ss["rbeg"], rb_w) and np.array_equal(ss["qbeg"], qb_w) and np.array_equal(ss["len"], ln_w), tag


def schedules(n_ctx, n=6):
    """every sequence of n submits and n collects with 0 <= in flight <= n_ctx, as strings of S and C"""
    out = []
    for seq in itertools.product("SC", repeat=2 * n):
        f = ok = 0
        for ch in seq:
            f += 1 if ch == "S" else -1
            if f < 0 or f > n_ctx:
                break
        else:
            ok = f == 0
        if ok:
            out.append("".join(seq))
    return out


def run_schedule(d, sched, batches, tag=None):
    """Runs the schedule; batches[j] = (slice index, dict(want_sal=..) or "refused" spec, see below) is the j-th submit.  Every collected
    result is checked at the latest moment it is valid: immediately before the second submit after its collect, or at the end.  Returns
    the number of results that were checked after the batch that reused their pass context had itself been collected."""
    import compseed_amd as ca
    e = d.e
    held = []                     # [batch number, Result, submits since its collect]
    n_sub = n_col = late = 0

    def check(h):
        nonlocal late
        j, r, _ = h
        i, spec = batches[j]
        if i is None:             # the empty batch
            assert (r.n_reads, r.n_mems, r.n_seeds) == (0, 0, 0), (tag, j)
            assert e.download(r.ptr["mem_off"], np.uint64, 1).tolist() == [0] and e.download(r.ptr["seed_off"], np.uint64, 1).tolist() == [0], (tag, j)
        else:
            check_result(e, r, i, sal=spec.get("want_sal", 1) != 0, tag=(tag, j))
        late += n_col > j + d.n_ctx
    for ch in sched:
        if ch == "S":
            for h in [h for h in held if h[2] == 1]:
                check(h); held.remove(h)
            i, spec = batches[n_sub]
            if i is None:
                e.submit_device(0, d.bufs[0][1], 0, 0, ca.Params())
            elif "bad_off" in spec:
                e.submit_device(d.bufs[i][0], spec["bad_off"], _slice(i)["n"], _slice(i)["bases"].size, ca.Params(**_slice(i)["kw"]))
            else:
                d.submit(i, **spec)
            n_sub += 1
            for h in held:
                h[2] += 1
        else:
            i, spec = batches[n_col]
            if i is not None and "bad_off" in spec:
                with pytest.raises(ca.CSError) as ei:
                    e.collect_device()
                assert ei.value.code == EINVAL, (tag, n_col)
            else:
                held.append([n_col, e.collect_device(), 0])
            n_col += 1
    for h in held:
        check(h)
    return late


# ---------------------------------------------------------------------------------------------------------------- 1. every legal schedule
@pytest.mark.parametrize("passes", [2, 1])
def test_every_schedule_of_six_submits_and_collects(passes):
    """all 32 (passes_in_flight = 2) / the one (1) order of six submits and six collects on the growing-and-shrinking batches; the first
    schedule runs on a fresh engine (a buffer has no slack on its first allocation), the others reuse it and start one batch further on"""
    scheds = schedules(passes)
    assert len(scheds) == (32 if passes == 2 else 1)
    d = Dev(passes)
    try:
        late = []
        for k, sc in enumerate(scheds):
            batches = [(ORDER_B[(k + j) % 8], {}) for j in range(6)]
            late.append(run_schedule(d, sc, batches, tag=sc))
        # at least one schedule checks a result after the batch that reused its context was itself collected: nothing then runs on
        # that context, so the verdict does not depend on how far an overwriting pass has got
        assert any(late), scheds
        if passes == 2:
            assert late[scheds.index("SSCSCSCSCSCC")] >= 1       # r3: one submit after its collect, then both later batches collected
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------------------------- 2. lifetime, order A
@pytest.mark.parametrize("passes", [2, 1])
def test_result_outlives_the_next_batch_on_its_context(passes):
    """sub 0, sub 1, col 0, sub 2, col 1, col 2 (one context: sub 0, col 0, sub 1, col 1), THEN r0 is read: one submit has followed its
    collect, so it is valid, and the batch that ran on its context since has been collected, so nothing races the download.  The batches
    shrink, so no buffer is reallocated: an engine that left r0 in its context shows the next batch's values here (and nothing worse).
    Against the parent of the change that introduced the spare result set this test fails on a value mismatch in r0, for both values of
    `passes`."""
    d = Dev(passes)
    try:
        e = d.e
        if passes == 2:
            d.submit(ORDER_A[0]); d.submit(ORDER_A[1])
            r0 = e.collect_device()
            d.submit(ORDER_A[2])
            r1 = e.collect_device(); r2 = e.collect_device()
            check_result(e, r2, ORDER_A[2], tag="r2")
        else:
            d.submit(ORDER_A[0])
            r0 = e.collect_device()
            d.submit(ORDER_A[1])
            r1 = e.collect_device()
        check_result(e, r1, ORDER_A[1], tag="r1")
        check_result(e, r0, ORDER_A[0], tag="r0")
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------------------------- 3. consumers working late
def test_chainer_and_filter_work_on_batch_n_while_n_plus_2_is_seeded():
    """the five runs of test_gpu_chain_device, two in flight: chain_device(r_n) is called after submit(n + 2) has been issued, filter_device
    after it; both read the held pointers.  Chains == the golden chains; filtered chains == the aln1 golden for the default-parameter
    runs, == the host filter of the downloaded chains for the others"""
    import compseed_amd as ca
    ix = ca.Index.load(_data.PREFIX)
    eng = ca.Engine(ix, 0, passes_in_flight=2)
    chainer = ca.Chainer(_data.PREFIX, device=0)
    bufs = []
    for name, pname in ENGINE_RUNS:
        z, kw = _data.load_golden(name, pname)
        bases, off = _data.load_reads(name)
        d_b, d_o = eng.alloc(bases.nbytes + 64), eng.alloc(off.nbytes)
        eng.upload(d_b, bases); eng.upload(d_o, off)
        bufs.append((name, pname, kw, d_b, d_o, bases, off))
    eng.sync()

    def sub(j):
        _, _, kw, d_b, d_o, bases, off = bufs[j]
        eng.submit_device(d_b, d_o, off.size - 1, bases.size, ca.Params(**kw))
    try:
        sub(0); sub(1)
        for n in range(len(bufs)):
            r = eng.collect_device()
            if n + 2 < len(bufs):
                sub(n + 2)                                       # runs on r's pass context, now
            name, pname, kw, d_b, d_o, bases, off = bufs[n]
            d = chainer.chain_device(r, d_o, _cp(kw))
            got = ca.download_chains(eng, d)
            check_chains(got, golden_chains(name, pname))
            f = ca.download_chains(eng, chainer.filter_device(d, d_b, d_o))
            if pname == "default":
                check_filtered(f, np.load(os.path.join(ALN, name + ".aln.npz")))
            else:
                host = chainer.filter(got["chain_off"], got["chains"], got["cseed_off"], got["cseeds"], bases, off, threads=4)
                for k in ("chain_off", "chains", "cseed_off", "cseeds", "cseed_score"):
                    assert f[k].dtype == host[k].dtype and f[k].tobytes() == host[k].tobytes(), (name, pname, k)
    finally:
        for b in bufs:
            eng.free(b[3]); eng.free(b[4])
        chainer.close(); eng.close(); ix.close()


# ---------------------------------------------------------------------------------------------------------------- 4. want_sal = 0 in between
@pytest.mark.parametrize("sched", ["SSCSCSCSCC", "SSCCSSCCSC"])
def test_batch_without_seeds_between_batches_with_seeds(dev2, sched):
    """want_sal = 0 between want_sal = 1 batches: null seed_off / seeds and the golden mems for it; the seeds of its neighbours -- which
    share seed buffers with it through the spare set -- intact at the latest legal moment"""
    batches = [(ORDER_B[1], {}), (ORDER_B[2], {"want_sal": 0}), (ORDER_B[3], {}), (ORDER_B[0], {"want_sal": 0}), (ORDER_B[5], {})]
    run_schedule(dev2, sched, batches, tag=sched)


# ---------------------------------------------------------------------------------------------------------------- 5. a refused batch
def _bad_offsets(kind, off):
    if kind == "shifted":
        return off + np.uint64(1)
    if kind == "past_the_end":
        return np.concatenate([off[:-1], [off[-1] + np.uint64(4096)]]).astype(np.uint64)
    return np.concatenate([off[:5], [off[3]], off[6:]]).astype(np.uint64)       # not ascending


@pytest.mark.parametrize("kind", ["shifted", "past_the_end", "descending"])
def test_refused_batch_in_the_stream(dev2, kind):
    """offsets that do not tile [0, n_bases) (those of test_device_offsets_are_validated: refused by validation, never read out of bounds)
    between two good batches: its collect is CS_EINVAL and hands nothing out, the batch before it is still valid afterwards -- it is
    checked before the second submit after its own collect, which is after the refusal -- the batch after it is right, and the stream
    goes on for two more"""
    i_bad = ORDER_B[3]
    bad = _bad_offsets(kind, _slice(i_bad)["off"])
    d_bad = dev2.e.alloc(bad.nbytes); dev2.e.upload(d_bad, bad); dev2.e.sync()
    try:
        batches = [(ORDER_B[1], {}), (i_bad, {"bad_off": d_bad}), (ORDER_B[4], {}), (ORDER_B[5], {}), (ORDER_B[6], {})]
        # S0 S1 C0 C1(refused) S2 [r0 checked here, before S3, the second submit after its collect] S3 C2 C3 S4 C4
        run_schedule(dev2, "SSCCSSCCSC", batches, tag=kind)
        run_schedule(dev2, "SSCSCSCSCC", batches, tag=kind)      # steady order: the refused batch's successor is in flight at its collect
    finally:
        dev2.e.free(d_bad)


# ---------------------------------------------------------------------------------------------------------------- 6. an empty batch
@pytest.mark.parametrize("sched", ["SSCSCSCSCC", "SSCCSSCCSC"])
def test_empty_batch_in_the_stream(dev2, sched):
    batches = [(ORDER_B[1], {}), (None, {}), (ORDER_B[3], {}), (None, {}), (ORDER_B[5], {})]
    run_schedule(dev2, sched, batches, tag=sched)


# ---------------------------------------------------------------------------------------------------------------- 7. digest and gather
def test_digest_and_gather_follow_the_collected_result(dev2):
    """after a drain the "last result" is the batch collected last, in the arrays that were handed out (its context holds an older
    batch's by then): result_digest == the digest of a blocking seed_batch_device of the same batch == the host restatement over the
    golden arrays; gather_reads == the golden slice; both are an error code while a batch is in flight"""
    import compseed_amd as ca
    e = dev2.e
    i_last = ORDER_B[3]
    dev2.submit(ORDER_B[1]); dev2.submit(ORDER_B[2])
    for fn in (e.result_digest, lambda: e.gather_reads(np.arange(3, dtype=np.uint64))):
        with pytest.raises(ca.CSError) as ei:
            fn()
        assert ei.value.code == EINVAL
    e.collect_device()
    dev2.submit(i_last)
    e.collect_device()
    with pytest.raises(ca.CSError):
        e.result_digest()                                        # one still in flight
    r = e.collect_device()
    dg = e.result_digest()
    s = _slice(i_last)
    mo_w, mm_w, so_w, rb_w, qb_w, ln_w = s["want"]
    mems = np.zeros(mm_w.shape[0], dtype=ca.INTV_DT)
    mems["x0"], mems["x1"], mems["x2"], mems["info"] = mm_w[:, 0], mm_w[:, 1], mm_w[:, 2], mm_w[:, 3]
    seeds = np.zeros(rb_w.size, dtype=ca.SEED_DT)
    seeds["rbeg"], seeds["qbeg"], seeds["len"] = rb_w, qb_w, ln_w
    assert dg == tuple(ca.binding.digest_words(a) for a in (mo_w, mems, so_w, seeds))
    ids = np.array([s["n"] - 1, 0, 7, 7, 500, 1499, 1, 2, 1000, 33], dtype=np.uint64)
    g = e.gather_reads(ids)
    assert g.n_reads == ids.size == 10
    mo, so = mo_w.astype(np.int64), so_w.astype(np.int64)
    for j, rd in enumerate(ids.astype(int)):
        assert np.array_equal(g.mems[int(g.mem_off[j]):int(g.mem_off[j + 1])], mems[mo[rd]:mo[rd + 1]]), rd
        assert np.array_equal(g.seeds[int(g.seed_off[j]):int(g.seed_off[j + 1])], seeds[so[rd]:so[rd + 1]]), rd
    check_result(e, r, i_last, tag="after digest and gather")
    e.seed_batch_device(dev2.bufs[i_last][0], dev2.bufs[i_last][1], s["n"], s["bases"].size, ca.Params(**s["kw"]))
    assert e.result_digest() == dg


# ---------------------------------------------------------------------------------------------------------------- 8. two threads
@pytest.mark.parametrize("passes", [2, 1])
def test_one_submitting_and_one_collecting_thread(passes):
    """the documented thread model: a submitting and a collecting thread, a semaphore of n_ctx tokens between them; the collector
    verifies each result before it gives its token back.  24 batches; results in submission order, all golden"""
    d = Dev(passes)
    N = 24
    order = [ORDER_B[j % 8] for j in range(N)]
    tokens, submitted, stop = threading.Semaphore(passes), threading.Semaphore(0), threading.Event()
    errors, done = [], []

    def submitter():
        try:
            for j in range(N):
                if not tokens.acquire(timeout=60) or stop.is_set():
                    raise RuntimeError("no token for batch %d" % j)
                d.submit(order[j])
                submitted.release()
        except BaseException as ex:          # noqa: B902 -- reported by the test below
            errors.append(("submitter", ex)); stop.set(); submitted.release()

    def collector():
        try:
            for j in range(N):
                if not submitted.acquire(timeout=60) or stop.is_set():
                    raise RuntimeError("batch %d was never submitted" % j)
                r = d.e.collect_device()
                check_result(d.e, r, order[j], tag=("thread", j))
                done.append(j)
                tokens.release()
        except BaseException as ex:          # noqa: B902
            errors.append(("collector", ex)); stop.set(); tokens.release()
    ts = [threading.Thread(target=submitter, daemon=True), threading.Thread(target=collector, daemon=True)]
    try:
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in ts), "a thread did not return"
        assert not errors, errors
        assert done == list(range(N))
    finally:
        if not any(t.is_alive() for t in ts):
            d.close()


# ---------------------------------------------------------------------------------------------------------------- 9. memory report
def _result_bytes(i):
    import compseed_amd as ca
    s = _slice(i)
    return 2 * (s["n"] + 1) * 8 + s["want"][1].shape[0] * np.dtype(ca.INTV_DT).itemsize + s["want"][3].size * np.dtype(ca.SEED_DT).itemsize


def _sum_of_groups(m):
    return sum(m[k] for k in ("occ_bwt", "sampled_sa", "full_sa", "isa", "text", "lcp_rep", "jump_table", "kmer_filter")) + sum(m["pass_ctx"])


def test_memory_report_counts_the_spare_result_set():
    """after a stream with two in flight total == the sum of the groups and pass_ctx[] grew by at least one result set of the largest batch.
    Then the spare set on its own, one context, the same batch three times: blocking (its result sits in the context), streamed (a
    collect moves it into the spare set: same total), streamed again (the context has to make result buffers anew while the spare set
    still holds the previous result): pass_ctx[0] grows by at least one result set, which is the set the contract costs"""
    big = ORDER_A[0]
    d = Dev(2)
    try:
        m0 = d.e.memory()
        assert m0["total"] == _sum_of_groups(m0)
        run_schedule(d, "SSCSCSCSCSCSCSCC", [(i, {}) for i in ORDER_B], tag="memory")
        m1 = d.e.memory()
        assert m1["total"] == _sum_of_groups(m1) and m1["n_pass_ctx"] == 2 and m1["pass_ctx"][1] > 0
        assert sum(m1["pass_ctx"]) - sum(m0["pass_ctx"]) >= _result_bytes(big)
    finally:
        d.close()
    d = Dev(1)
    try:
        import compseed_amd as ca
        s = _slice(big)
        d.e.seed_batch_device(d.bufs[big][0], d.bufs[big][1], s["n"], s["bases"].size, ca.Params(**s["kw"]))
        ma = d.e.memory()
        d.submit(big); r = d.e.collect_device()
        mb = d.e.memory()
        assert mb["total"] == ma["total"] == _sum_of_groups(mb) and mb["pass_ctx"][1] == 0
        d.submit(big); r2 = d.e.collect_device()
        mc = d.e.memory()
        assert mc["total"] == _sum_of_groups(mc)
        assert mc["pass_ctx"][0] - ma["pass_ctx"][0] >= _result_bytes(big)
        check_result(d.e, r2, big, tag="second")
        assert r2.ptr["mems"] != r.ptr["mems"]                   # the first result was not overwritten in place
    finally:
        d.close()
