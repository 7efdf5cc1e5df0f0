"""Lean seeding results (cs_params_t.result_flags = CS_RESULT_LEAN): the caller reads no x0 / x1 of the mems.  Everything else -- mem_off,
x2, info, seed_off, the seeds in both forms, the counters -- is bit for bit the result of flags 0, which the other test files pin to the
reference's goldens and the oracle; x1 reads 0 wherever a mem is handed out, x0 reads 0 where mems travel as CS_MEM_LEAN8 (8 bytes
instead of 16 over PCIe), and the result does not depend on `disable`, `sst_mode` or engine options, down to the device digest."""
import gzip
import os

import numpy as np
import pytest

import _data
import _oracle
from test_chain import check_chains, golden_chains

pytestmark = pytest.mark.gpu

U32 = np.uint64(32)
LOW = np.uint64(0xffffffff)


def _lean(**kw):
    import compseed_amd as ca
    return ca.Params(result_flags=ca.RESULT_LEAN, **kw)


def _keep(p):
    """a packed result as copies (the views die with the engine's next call), seed_rbeg expanded"""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    out["seed_rbeg"] = None if p["seed_rbeg_lo"] is None else p["seed_rbeg"].copy()
    return out


def _same_packed(a, b):
    """two packed results, byte for byte: format, offsets, mems as they travel, both seed planes"""
    assert a["mem_format"] == b["mem_format"] and a["n_mems"] == b["n_mems"] and a["n_seeds"] == b["n_seeds"] and a["max_occ"] == b["max_occ"]
    assert a["mems"].dtype == b["mems"].dtype and a["mems"].tobytes() == b["mems"].tobytes()
    for k in ("mem_off", "seed_off", "seed_rbeg_lo", "seed_rbeg_hi"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or a[k].tobytes() == b[k].tobytes()), k


def _same_but_x(lean_mems, full_mems, x0_zero):
    """a lean mem array against the flags-0 one: x2 and info identical, x1 == 0, x0 zero or as computed"""
    assert lean_mems.size == full_mems.size
    assert np.array_equal(lean_mems["x2"], full_mems["x2"]) and np.array_equal(lean_mems["info"], full_mems["info"])
    assert not lean_mems["x1"].any()
    if x0_zero:
        assert not lean_mems["x0"].any()
    else:
        assert np.array_equal(lean_mems["x0"], full_mems["x0"])


def _download(eng, r, sal=True):
    import compseed_amd as ca
    def get(ptr, dt, n):
        return eng.download(ptr, dt, n) if n else np.zeros(0, dtype=dt)
    out = dict(mem_off=get(r.ptr["mem_off"], np.uint64, r.n_reads + 1), mems=get(r.ptr["mems"], ca.INTV_DT, r.n_mems))
    if sal:
        out["seed_off"] = get(r.ptr["seed_off"], np.uint64, r.n_reads + 1); out["seeds"] = get(r.ptr["seeds"], ca.SEED_DT, r.n_seeds)
    return out


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
def reads():
    """3,000 reads of 150 bases: the golden set sorted150 twice (results do not depend on the batch a read travels in)"""
    bases, off = _data.load_reads("sorted150")
    n = off.size - 1
    b2 = np.concatenate([bases, bases])
    o2 = np.concatenate([off, off[1:] + off[-1]]).astype(np.uint64)
    assert o2.size == 2 * n + 1 and int(o2[-1]) == b2.size
    return b2, o2


@pytest.fixture(scope="module")
def want(reads):
    """the oracle's result for the 3,000 reads, computed once"""
    o = _oracle.OracleIndex(_data.PREFIX)
    w = o.seed_batch(reads[0], reads[1], _oracle.make_params(), mode=0, threads=4)
    o.close()
    return w


@pytest.fixture(scope="module")
def packed(eng, reads):
    """test 1's two blocking packed calls on one engine, kept as copies: (flags 0, LEAN)"""
    import compseed_amd as ca
    full = _keep(eng.seed_batch_packed(reads[0], reads[1], ca.Params()))
    lean = _keep(eng.seed_batch_packed(reads[0], reads[1], _lean()))
    return full, lean


# ------------------------------------------------------------------------------------------------------------------ 1. packed, blocking
def test_packed_blocking(packed, want):
    import compseed_amd as ca
    full, lean = packed
    assert full["mem_format"] == ca.MEM_PACKED16 and lean["mem_format"] == ca.MEM_LEAN8
    assert lean["mems"].dtype == ca.MEM8_DT and lean["mems"].dtype.itemsize == 8 and lean["mems"].size == full["mems"].size == lean["n_mems"]
    for k in ("mem_off", "seed_off", "seed_rbeg_lo", "seed_rbeg_hi"):
        assert lean[k].tobytes() == full[k].tobytes(), k
    assert lean["n_seeds"] == full["n_seeds"] and lean["max_occ"] == full["max_occ"] and lean["seed_format"] == full["seed_format"]
    fm, lm = ca.unpack_mems16(full["mems"]), ca.unpack_mems8(lean["mems"])
    _same_but_x(lm, fm, x0_zero=True)
    assert np.array_equal(lm["x2"], want["mems"]["x2"]) and np.array_equal(lm["info"], want["mems"]["info"])
    assert np.array_equal(lean["mem_off"], want["mem_off"]) and np.array_equal(lean["seed_off"], want["seed_off"])
    assert np.array_equal(lean["seed_rbeg"], want["seeds"]["rbeg"])
    assert np.array_equal(fm, want["mems"])                                  # (the flags-0 run on the same engine is the oracle's)
    assert np.array_equal(ca.unpack_mems(lean), lm)


# ------------------------------------------------------------------------------------------------------------------ 2. expanded
def test_expanded(eng, reads, want):
    import compseed_amd as ca
    full = eng.seed_batch(reads[0], reads[1], ca.Params())
    lean = eng.seed_batch(reads[0], reads[1], _lean())
    assert np.array_equal(full.mems, want["mems"]) and np.array_equal(full.seeds, want["seeds"])
    assert lean.mem_off.tobytes() == full.mem_off.tobytes() and lean.seed_off.tobytes() == full.seed_off.tobytes()
    assert lean.seeds.tobytes() == full.seeds.tobytes()
    z = full.mems.copy(); z["x0"] = 0; z["x1"] = 0
    assert lean.mems.tobytes() == z.tobytes()


# ------------------------------------------------------------------------------------------------------------------ 3. sub-batches
@pytest.mark.parametrize("host_pack_threads", [8, 0])
def test_sub_batches(ix, reads, packed, host_pack_threads):
    """pipeline_reads = 700 over 3,000 reads: five sub-batches, four with a non-zero mem_base, placed in 8-byte elements"""
    import compseed_amd as ca
    e = ca.Engine(ix, 0, pipeline_reads=700, expand_threads=3, host_pack_threads=host_pack_threads)
    try:
        _same_packed(_keep(e.seed_batch_packed(reads[0], reads[1], _lean())), packed[1])
        _same_packed(_keep(e.seed_batch_packed(reads[0], reads[1], ca.Params())), packed[0])
        _same_packed(_keep(e.seed_batch_packed(reads[0], reads[1], _lean())), packed[1])
        x = e.seed_batch(reads[0], reads[1], _lean())
        _same_but_x(x.mems, ca.unpack_mems16(packed[0]["mems"]), x0_zero=True)
        assert np.array_equal(x.seeds["rbeg"], packed[0]["seed_rbeg"]) and np.array_equal(x.mem_off, packed[0]["mem_off"])
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------ 4. stream
def test_stream_mixes_formats(ix, reads):
    """batches of 1,000 / 3,000 / 500 reads with flags 0, LEAN, 0 through submit / collect_packed, then five more so that every pinned
    result slot (batch number mod 4) and both device pack slots are used again at the other element size; each batch comes back in its own
    format and equals its blocking call"""
    import compseed_amd as ca
    bases, off = reads
    def cut(r0, r1):
        b = ca.pinned_array(int(off[r1] - off[r0])); b[:] = bases[int(off[r0]):int(off[r1])]
        return b, (off[r0:r1 + 1] - off[r0]).astype(np.uint64)
    sets = [cut(0, 1000), cut(0, 3000), cut(2500, 3000)]
    flags = [0, 1, 0, 1, 1, 0, 1, 0]                         # batch i and batch i + 4 share a result slot and differ in format
    e = ca.Engine(ix, 0, pipeline_reads=900)
    try:
        blocking = {}
        for s in range(3):
            for f in (0, 1):
                blocking[s, f] = _keep(e.seed_batch_packed(sets[s][0], sets[s][1], ca.Params(result_flags=f)))
        n, depth, sub = len(flags), 3, 0
        for i in range(n):
            while sub < n and sub < i + depth:
                e.submit(sets[sub % 3][0], sets[sub % 3][1], ca.Params(result_flags=flags[sub])); sub += 1
            p = e.collect_packed()
            assert p["mem_format"] == (ca.MEM_LEAN8 if flags[i] else ca.MEM_PACKED16), i
            assert p["mems"].dtype.itemsize == (8 if flags[i] else 16)
            _same_packed(_keep(p), blocking[i % 3, flags[i]])
        lean, full = blocking[1, 1], blocking[1, 0]
        _same_but_x(ca.unpack_mems8(lean["mems"]), ca.unpack_mems16(full["mems"]), x0_zero=True)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------ 5. device
DISABLES = [(), ("r3_text",), ("text_mode", "r2_text", "text_sweep", "r3_text"), ("fused_sal",), ("mem_pos",), ("window",)]


def test_device_results_and_digests(eng, reads, want):
    import compseed_amd as ca
    bases, off = reads
    n = off.size - 1
    d_b = eng.alloc(bases.nbytes + 64); d_o = eng.alloc(off.nbytes)
    try:
        eng.upload(d_b, bases); eng.upload(d_o, off)
        full = _download(eng, eng.seed_batch_device(d_b, d_o, n, bases.size, ca.Params()))
        dig_full = eng.result_digest()
        assert np.array_equal(full["mems"], want["mems"]) and np.array_equal(full["seeds"], want["seeds"])
        r = eng.seed_batch_device(d_b, d_o, n, bases.size, _lean())
        lean = _download(eng, r)
        dig = eng.result_digest()
        for k in ("mem_off", "seed_off", "seeds"):
            assert lean[k].tobytes() == full[k].tobytes(), k
        _same_but_x(lean["mems"], full["mems"], x0_zero=False)           # device arrays: x0 as computed, x1 == 0
        z = full["mems"].copy(); z["x1"] = 0
        assert lean["mems"].tobytes() == z.tobytes()
        assert (dig[0], dig[2], dig[3]) == (dig_full[0], dig_full[2], dig_full[3]) and dig[1] != dig_full[1]
        assert dig[1] == ca.binding.digest_words(z)                       # the digest sees the arrays as they lie
        g = eng.gather_reads(np.array([5, 2999, 0, 1500], dtype=np.uint64))   # ... and so does gather_reads
        assert not g.mems["x1"].any() and g.mems["x0"].any()
        # lean results do not depend on the shortcuts: with round 3 on the index x1 is a real number before the sort stores 0
        for names in DISABLES:
            eng.seed_batch_device(d_b, d_o, n, bases.size, _lean(disable=ca.disable_mask(*names)))
            assert eng.result_digest() == dig, names
        eng.seed_batch_device(d_b, d_o, n, bases.size, _lean(sst_mode=0))
        assert eng.result_digest() == dig
        eng.seed_batch_device(d_b, d_o, n, bases.size, ca.Params(disable=ca.disable_mask("r3_text")))
        assert eng.result_digest() == dig_full                            # (flags 0 is untouched)
        # the device stream: one lean batch between two full ones, two in flight
        pars = [ca.Params(), _lean(), ca.Params()]
        eng.submit_device(d_b, d_o, n, bases.size, pars[0]); eng.submit_device(d_b, d_o, n, bases.size, pars[1])
        for i in range(3):
            got = _download(eng, eng.collect_device())
            if i == 0:
                eng.submit_device(d_b, d_o, n, bases.size, pars[2])
            ref = lean if i == 1 else full
            for k in ("mem_off", "mems", "seed_off", "seeds"):
                assert got[k].tobytes() == ref[k].tobytes(), (i, k)
    finally:
        eng.free(d_b); eng.free(d_o)


@pytest.mark.parametrize("opts", [dict(fused=1, mem_cap=6), dict(mem_cap=4), dict(sa64=1), dict(sa40=1), dict(text_arrays=0)],
                         ids=["fused_cap6", "mem_cap4", "sa64", "sa40", "no_text_arrays"])
def test_device_digest_on_other_engines(ix, eng, reads, opts):
    """the other kernels that write the final mems[]: the one-lane-per-read path of the `fused` engine option (sort_compact_kernel and
    its second pass over the reads with more than mem_cap mems), the wave sort behind overflow records (mem_cap 4), r3text_kernel's
    fused-entry instantiation (sa64), 40-bit entries, round 3 on the index alone; and sort-then-SAL instead of the fused pass on each"""
    import compseed_amd as ca
    bases, off = reads
    n = off.size - 1
    res = {}
    for name, e in (("default", eng), ("other", ca.Engine(ix, 0, **opts))):
        d_b = e.alloc(bases.nbytes + 64); d_o = e.alloc(off.nbytes)
        try:
            e.upload(d_b, bases); e.upload(d_o, off)
            e.seed_batch_device(d_b, d_o, n, bases.size, ca.Params())
            full = e.result_digest()
            r = e.seed_batch_device(d_b, d_o, n, bases.size, _lean())
            lean = e.result_digest()
            assert not e.download(r.ptr["mems"], ca.INTV_DT, r.n_mems)["x1"].any()
            e.seed_batch_device(d_b, d_o, n, bases.size, _lean(disable=ca.disable_mask("fused_sal", "r3_text")))
            assert e.result_digest() == lean
            res[name] = (full, lean)
        finally:
            e.free(d_b); e.free(d_o)
            if e is not eng:
                e.close()
    assert res["other"] == res["default"]


# ------------------------------------------------------------------------------------------------------------------ 6. the kernel path ran
@pytest.mark.parametrize("opts", [dict(), dict(sa64=1)], ids=["isa32_unfused", "sa64_fused"])
def test_r3text_skips_the_reverse_strand_loads(ix, reads, opts):
    """count_traffic = 1: r3text_kernel's inverse-SA events are strictly fewer under LEAN; every other kernel's row, every other event
    column and the counters are identical.

    One cell needs a correction before it can be compared: fwd_kernel's Occ-record events.  A bwt_extend query the on-device SST memo
    answers reads no Occ record, and which queries the memo answers depends on which workgroup takes which call -- cs_stats_t.bwt_calls
    (queries the memo did not answer) differs from pass to pass with identical parameters, as the header says of sst_mode.  Measured on
    an MI355X over 16 identical passes of this batch, flags alternating: fwd_kernel occ_record 25,660 .. 26,708, bwt_calls 56,497 ..
    57,021, every other cell of every kernel equal in all 16; and occ_record - 2 * bwt_calls == -87,334 in every pass (a query that
    misses the memo reads two records).  So that cell is compared as occ_record - 2 * bwt_calls, which is a function of the input alone."""
    import compseed_amd as ca
    e = ca.Engine(ix, 0, **opts)
    try:
        e.seed_batch(reads[0], reads[1], ca.Params(count_traffic=1), copy=False)       # (both measured runs start from the same warm engine)
        seen = {}
        for name, f in (("full", 0), ("lean", ca.RESULT_LEAN)):
            e.reset_stats()
            e.seed_batch(reads[0], reads[1], ca.Params(count_traffic=1, result_flags=f), copy=False)
            seen[name] = (e.traffic_model(), e.stats())
        (tf, sf), (tl, sl) = seen["full"], seen["lean"]
        kf, kl = tf["kernels"], tl["kernels"]
        print("r3text_kernel events: flags 0", kf["r3text_kernel"]["events"], "LEAN", kl["r3text_kernel"]["events"])
        print("other kernels: flags 0", {k: v["events"] for k, v in kf.items() if k != "r3text_kernel"})
        print("other kernels: LEAN   ", {k: v["events"] for k, v in kl.items() if k != "r3text_kernel"})
        print("stats: flags 0", sf, "LEAN", sl)
        isa_f, isa_l = kf["r3text_kernel"]["events"]["isa_entry"], kl["r3text_kernel"]["events"].get("isa_entry", 0)
        assert 0 < isa_l < isa_f
        assert set(kf) == set(kl)
        for kn in kf:
            ef, el = dict(kf[kn]["events"]), dict(kl[kn]["events"])
            if kn == "r3text_kernel":
                ef.pop("isa_entry"); el.pop("isa_entry", None)
            if kn == "fwd_kernel":                                           # (the memo's share taken out: docstring)
                ef["occ_record"] -= 2 * sf["bwt_calls"]; el["occ_record"] -= 2 * sl["bwt_calls"]
            assert ef == el, kn
        assert tf["event_bytes"] == tl["event_bytes"]
        for key in ("r3_text_seeds", "mems", "seeds"):
            assert sf[key] == sl[key] and sf[key] > 0, key
        for key in ("reads", "bases", "bwt_queries", "sal_queries", "sal_calls", "overflow_mems", "reseed_text_calls", "reseed_index_calls", "sweep_text_calls"):
            assert sf[key] == sl[key], key
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------ 7. downstream
def test_downstream_chains(eng):
    """chaining reads x2 and info of a mem only: the device chainer on a lean device result gives the chains of the full result byte for
    byte, the host chainer on the expanded lean result the chain golden of the set"""
    import compseed_amd as ca
    bases, off = _data.load_reads("sorted150")
    zc = golden_chains("sorted150", "default")
    n = off.size - 1
    ch = ca.Chainer(_data.PREFIX, device=0)
    d_b = eng.alloc(bases.nbytes + 64); d_o = eng.alloc(off.nbytes)
    try:
        eng.upload(d_b, bases); eng.upload(d_o, off)
        got = {}
        for name, par in (("full", ca.Params()), ("lean", _lean())):
            r = eng.seed_batch_device(d_b, d_o, n, bases.size, par)
            got[name] = ca.download_chains(eng, ch.chain_device(r, d_o, ca.ChainParams()))
        for k in ("chain_off", "chains", "cseed_off", "cseeds"):
            assert got["lean"][k].dtype == got["full"][k].dtype and got["lean"][k].tobytes() == got["full"][k].tobytes(), k
        check_chains(got["lean"], zc)
        x = eng.seed_batch(bases, off, _lean())
        assert not x.mems["x0"].any() and not x.mems["x1"].any()
        check_chains(ch.chain(x.mem_off, x.mems, x.seed_off, x.seeds, off, ca.ChainParams(), threads=4), zc)
    finally:
        eng.free(d_b); eng.free(d_o); ch.close()


# ------------------------------------------------------------------------------------------------------------------ 8. edges
def test_empty_batch_and_no_sal(eng, reads, packed):
    import compseed_amd as ca
    p = eng.seed_batch_packed(np.zeros(0, np.uint8), np.zeros(1, np.uint64), _lean())
    assert p["n_reads"] == 0 and p["n_mems"] == 0 and p["n_seeds"] == 0 and p["mem_format"] == ca.MEM_LEAN8 and list(p["mem_off"]) == [0]
    r = eng.seed_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64), _lean())
    assert r.n_reads == 0 and r.n_mems == 0 and r.n_seeds == 0
    d = eng.seed_batch_device(0, 0, 0, 0, _lean())
    assert d.n_reads == 0 and d.n_mems == 0 and d.n_seeds == 0
    # want_sal = 0
    nos = eng.seed_batch_packed(reads[0], reads[1], _lean(want_sal=0))
    assert nos["mem_format"] == ca.MEM_LEAN8 and nos["seed_off"] is None and nos["n_seeds"] == 0
    assert nos["mems"].tobytes() == packed[1]["mems"].tobytes() and nos["mem_off"].tobytes() == packed[1]["mem_off"].tobytes()
    x = eng.seed_batch(reads[0], reads[1], _lean(want_sal=0))
    assert x.seeds is None and np.array_equal(x.mems, ca.unpack_mems8(packed[1]["mems"]))
    d_b = eng.alloc(reads[0].nbytes + 64); d_o = eng.alloc(reads[1].nbytes)
    try:
        eng.upload(d_b, reads[0]); eng.upload(d_o, reads[1])
        r = eng.seed_batch_device(d_b, d_o, reads[1].size - 1, reads[0].size, _lean(want_sal=0))
        m = eng.download(r.ptr["mems"], ca.INTV_DT, r.n_mems)
        assert r.n_seeds == 0 and not m["x1"].any() and np.array_equal(m["x2"], ca.unpack_mems8(packed[1]["mems"])["x2"])
    finally:
        eng.free(d_b); eng.free(d_o)


def test_reads_shorter_than_the_seed_length(eng):
    import compseed_amd as ca
    bases, off = _data.pack_reads([b"ACGTACGTAC", b"TTGACCA", b"", b"GATTACAGATTACAGATT"])     # all shorter than min_seed_len 19
    for par in (ca.Params(), _lean()):
        p = eng.seed_batch_packed(bases, off, par)
        assert p["n_mems"] == 0 and p["n_seeds"] == 0 and list(p["mem_off"]) == [0] * 5 and list(p["seed_off"]) == [0] * 5
        assert p["mem_format"] == (ca.MEM_LEAN8 if par.result_flags else ca.MEM_PACKED16)
    r = eng.seed_batch(bases, off, _lean())
    assert r.n_mems == 0 and r.n_seeds == 0


def test_long_read_falls_back_to_full_records(eng):
    """a read of 33,000 bases does not fit the 15-bit query fields: CS_MEM_FULL32 with x1 == 0, x0 as computed, everything else as flags 0"""
    import compseed_amd as ca
    fa = gzip.open(os.path.join(_data.GOLD, "ref.fa.gz")).read().decode().split("\n")
    g = "".join(l for l in fa if not l.startswith(">")).replace("N", "A")
    bases, off = _data.pack_reads([g[2000:35000].encode(), g[50000:50150].encode()])
    full = _keep(eng.seed_batch_packed(bases, off, ca.Params()))
    lean = _keep(eng.seed_batch_packed(bases, off, _lean()))
    assert full["mem_format"] == lean["mem_format"] == ca.MEM_FULL32 and lean["mems"].dtype == ca.INTV_DT
    for k in ("mem_off", "seed_off", "seed_rbeg_lo", "seed_rbeg_hi"):
        assert lean[k].tobytes() == full[k].tobytes(), k
    _same_but_x(lean["mems"], full["mems"], x0_zero=False)
    assert full["mems"]["x1"].any() and int((full["mems"]["info"] & LOW).max()) >= 1 << 15
    x, xf = eng.seed_batch(bases, off, _lean()), eng.seed_batch(bases, off, ca.Params())
    _same_but_x(x.mems, xf.mems, x0_zero=False)
    assert x.seeds.tobytes() == xf.seeds.tobytes()
    o = _oracle.OracleIndex(_data.PREFIX)
    w = o.seed_batch(bases, off, _oracle.make_params(), mode=0, threads=2)
    o.close()
    assert np.array_equal(xf.mems, w["mems"]) and np.array_equal(xf.seeds, w["seeds"])


def test_unknown_flags_are_refused_everywhere(eng, reads, packed):
    """result_flags = 2 and reserved = 1: CS_EINVAL from the blocking, packed, submit and device entry points; nothing is left in flight
    and the engine works afterwards"""
    import compseed_amd as ca
    bases, off = reads
    n = off.size - 1
    bad2 = ca.Params(result_flags=2)
    bad3 = ca.Params(result_flags=3)
    badr = ca.Params(); badr.reserved = 1
    badl = _lean(); badl.reserved = 1
    pin = ca.pinned_array(bases.size); pin[:] = bases
    d_b = eng.alloc(bases.nbytes + 64); d_o = eng.alloc(off.nbytes)
    try:
        eng.upload(d_b, bases); eng.upload(d_o, off)
        for par in (bad2, bad3, badr, badl):
            for call in (lambda: eng.seed_batch(bases, off, par), lambda: eng.seed_batch_packed(bases, off, par), lambda: eng.submit(pin, off, par),
                         lambda: eng.seed_batch_device(d_b, d_o, n, bases.size, par), lambda: eng.submit_device(d_b, d_o, n, bases.size, par)):
                with pytest.raises(ca.CSError) as ei:
                    call()
                assert ei.value.code == -1, ei.value
            eng._inflight = []
            with pytest.raises(ca.CSError):
                eng.collect_packed()                                      # nothing was queued
            with pytest.raises(ca.CSError):
                eng.collect_device()
        _same_packed(_keep(eng.seed_batch_packed(bases, off, _lean())), packed[1])
        _same_packed(_keep(eng.seed_batch_packed(bases, off, ca.Params())), packed[0])
        r = eng.seed_batch_device(d_b, d_o, n, bases.size, _lean())
        assert r.n_mems == packed[1]["n_mems"] and r.n_seeds == packed[1]["n_seeds"]
    finally:
        eng.free(d_b); eng.free(d_o)
