"""Engine option `sa40` on the GPU: the full suffix array and the inverse suffix array as 40-bit entries, three to a 16-byte group.
Results never depend on the layout, so the specification is what the 4- and 8-byte engines are held to: the reference's golden vectors,
the oracle, cs_engine_check_index; plus cs_engine_memory, which is how the saving shows."""
import os
import sys
import time

import numpy as np
import pytest

import _data
import _oracle
from test_gpu_parity import _check_against_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

POISON = np.uint64(0xdeadbeefdeadbeef)
PAD = 128   # bytes a packed array may hold beyond its groups: the last group's unused entries (< 16) and four spare groups (64)


@pytest.fixture(scope="module")
def eng40():
    """40-bit entries on the small fixture index: the instantiation, exercised the way sa64 exercises the 8-byte one"""
    import compseed_amd as ca
    ix = ca.Index.load(_data.PREFIX)
    e = ca.Engine(ix, 0, sa40=1)
    yield e
    e.close()
    ix.close()


@pytest.mark.parametrize("name,pname", _data.golden_runs())
def test_golden_seeds_40bit_text_side(eng40, name, pname):
    """every reference golden through fsa40 / isa40 / lcp / rep, with every shortcut on and with sst_mode = 0"""
    import compseed_amd as ca
    z, kw = _data.load_golden(name, pname)
    bases, off = _data.load_reads(name)
    eng40.reset_stats()
    _check_against_golden(eng40.seed_batch(bases, off, ca.Params(**kw)), z)
    _check_against_golden(eng40.seed_batch(bases, off, ca.Params(sst_mode=0, **kw)), z)


def test_40bit_text_side_mechanisms_fire_and_sa_agrees(eng40):
    import compseed_amd as ca
    eng40.reset_stats()
    for name in ("main100", "sorted150"):
        bases, off = _data.load_reads(name)
        eng40.seed_batch(bases, off, ca.Params())
    st = eng40.stats()
    assert st["reseed_text_calls"] > 0 and st["sweep_text_calls"] > 0 and st["r3_text_seeds"] > 0
    n = int(eng40._index.view.seq_len)
    got = eng40.sa(np.arange(0, n + 1, dtype=np.uint64))          # sa_kernel poisons rows where fsa40 != the walk
    assert not (got == POISON).any()
    chk = eng40.check_index()                                     # ISA o SA = id, suffix order, BWT characters, sampled SA: every row
    assert chk["rows_checked"] == n
    assert all(chk[k] == 0 for k in ("order_violations", "isa_violations", "bwt_violations", "sampled_sa_violations", "undecided_rows")), chk


def test_sa40_without_full_sa_walks():
    """full_sa = 0: nothing to pack; SAL walks bwt_invPsi from the samples exactly as without the option"""
    import compseed_amd as ca
    ix = ca.Index.load(_data.PREFIX)
    e = ca.Engine(ix, 0, full_sa=0, sa40=1)
    for name, pname in _data.golden_runs():
        z, kw = _data.load_golden(name, pname)
        bases, off = _data.load_reads(name)
        _check_against_golden(e.seed_batch(bases, off, ca.Params(**kw)), z)
    m = e.memory()
    assert m["sa_entry_bits"] == 0 and m["full_sa"] == 0 and m["isa"] == 0 and m["text"] == 0 and m["lcp_rep"] == 0
    e.close(); ix.close()


def _sum_of_groups(m):
    return sum(m[k] for k in ("occ_bwt", "sampled_sa", "full_sa", "isa", "text", "lcp_rep", "jump_table", "kmer_filter")) + sum(m["pass_ctx"])


def test_memory_report(eng40):
    import compseed_amd as ca
    rows = int(eng40._index.view.seq_len) + 1
    m = eng40.memory()
    assert m["sa_entry_bits"] == 40
    assert 5 * rows <= m["full_sa"] <= 5.34 * rows + PAD and 5 * rows <= m["isa"] <= 5.34 * rows + PAD
    assert m["total"] == _sum_of_groups(m)
    ix = ca.Index.load(_data.PREFIX)
    e = ca.Engine(ix, 0)
    d = e.memory()
    assert d["sa_entry_bits"] == 32
    assert d["total"] == _sum_of_groups(d)
    assert 4 * rows <= d["full_sa"] <= 4 * rows + PAD and 4 * rows <= d["isa"] <= 4 * rows + PAD
    v = ix.view
    assert d["occ_bwt"] >= 4 * int(v.bwt_size) and d["sampled_sa"] >= 8 * int(v.n_sa) and d["text"] >= (rows - 1) // 4
    assert d["lcp_rep"] >= 2 * rows and d["jump_table"] == 16 << 30 and d["kmer_filter"] > 0
    assert d["n_pass_ctx"] == 1 and d["pass_ctx"][0] > 0 and d["pass_ctx"][1] == 0
    # everything but the two arrays is the same on both engines
    for k in ("occ_bwt", "sampled_sa", "text", "lcp_rep", "jump_table", "kmer_filter"):
        assert d[k] == m[k], k
    # a pass makes its context's buffers grow, and the report follows
    bases, off = _data.load_reads("sorted150")
    before = d["pass_ctx"][0]
    e.seed_batch(bases, off)
    a = e.memory()
    assert a["pass_ctx"][0] > before and a["total"] == _sum_of_groups(a)
    e8 = ca.Engine(ix, 0, sa64=1)
    assert e8.memory()["sa_entry_bits"] == 64 and e8.memory()["full_sa"] >= 8 * rows
    e8.close(); e.close(); ix.close()


def test_traffic_model_counts_five_bytes(eng40):
    import compseed_amd as ca
    eng40.reset_stats()
    bases, off = _data.load_reads("main100")
    eng40.seed_batch(bases, off, ca.Params(count_traffic=1))
    t = eng40.traffic_model()
    assert t["event_bytes"]["sa_entry"] == 5 and t["event_bytes"]["isa_entry"] == 5
    ev = {}
    for k in t["kernels"].values():
        for name, n in k["events"].items():
            ev[name] = ev.get(name, 0) + n
    assert ev.get("sa_entry", 0) > 0 and ev.get("isa_entry", 0) > 0      # ... and such events did occur
    eng40.reset_stats()


def test_sa40_at_full_size():
    """Only rows beyond 2^32 put anything into the fifth bytes: the hg19-size synthetic index of test_full_baseline_size_properties
    (same seed, same generator calls) through an sa40 engine.  cs_engine_check_index over all 6.2e9 rows (ISA o SA = id, suffix order
    decided on the text, BWT characters, sampled SA, recovered text == genome); 10 M x 150 bp reads, every shortcut on vs sst_mode = 0 by
    the device-side digests; the strided 100,000-read sample bit-exact against the oracle; and the two arrays at least 30 GB smaller
    than with 8-byte entries (derived: 2 x 6.2e9 x (8 - 5.33) = 33 GB)."""
    import torch
    import compseed_amd as ca
    import synth
    t0 = time.time()
    n = 10_000_000
    G = synth.make_genome(3_100_000_000, seed=20261003, device="cuda")
    ix = ca.Index.build(G.cpu().numpy(), 0)
    bases, off = synth.make_reads(G, n, 150, seed=777, p_sub=0.005, sort=True)
    assert ix.view.seq_len + 1 > 2**32
    rows = int(ix.view.seq_len) + 1
    t1 = time.time()
    eng = ca.Engine(ix, 0, sa40=1)
    t2 = time.time()
    m = eng.memory()
    print("memory():", m)
    assert m["sa_entry_bits"] == 40 and m["text"] > 0 and m["lcp_rep"] > 0
    chk = eng.check_index(G.data_ptr(), G.numel())
    t3 = time.time()
    print("index build %.1f s, engine creation %.1f s, check_index %.1f s" % (t1 - t0, t2 - t1, t3 - t2))
    assert chk["rows_checked"] == 2 * G.numel() and chk["text_checked"] == 1
    assert all(chk[k] == 0 for k in ("order_violations", "isa_violations", "bwt_violations", "sampled_sa_violations", "undecided_rows", "text_violations")), chk
    del G
    torch.cuda.empty_cache()
    assert m["full_sa"] <= 5.34 * rows + PAD and m["isa"] <= 5.34 * rows + PAD
    assert m["full_sa"] + m["isa"] <= 2 * 8 * rows - 30e9
    bw, sa = ix.arrays()
    v = ix.view
    o = _oracle.OracleIndex.from_arrays(v.primary, [v.L2[i] for i in range(1, 5)], bw, sa, 32)
    ids = np.arange(0, n, n // 100000, dtype=np.uint64)[:100000]               # every 100th read: 100,000 reads against the oracle
    sel = (ids[:, None].astype(np.int64) * 150 + np.arange(150)[None, :]).reshape(-1)
    hb = bases[torch.from_numpy(sel).to(bases.device)].cpu().numpy()
    ho = (np.arange(ids.size + 1, dtype=np.uint64) * np.uint64(150))
    torch.cuda.synchronize()
    r = eng.seed_batch_device(bases.data_ptr(), off.data_ptr(), n, bases.numel(), ca.Params())
    d_on = eng.result_digest()
    st = eng.stats()
    assert r.n_mems > 50_000_000
    assert st["reseed_text_calls"] > 0 and st["r3_text_seeds"] > 0 and st["sweep_text_calls"] > 0      # the shortcuts did run
    got = eng.gather_reads(ids)
    want = o.seed_batch(hb, ho, _oracle.make_params(), mode=1, threads=16)
    assert np.array_equal(got.mem_off, want["mem_off"]) and np.array_equal(got.mems, want["mems"])
    assert np.array_equal(got.seed_off, want["seed_off"]) and np.array_equal(got.seeds, want["seeds"])
    eng.reset_stats()
    eng.seed_batch_device(bases.data_ptr(), off.data_ptr(), n, bases.numel(), ca.Params(sst_mode=0))
    st0 = eng.stats()
    assert st0["reseed_text_calls"] == 0 and st0["r3_text_seeds"] == 0 and st0["bwt_calls"] == st0["bwt_queries"]
    assert eng.result_digest() == d_on                                         # all 10 M reads, all four arrays
    a = eng.memory()
    assert a["pass_ctx"][0] > m["pass_ctx"][0] and a["total"] == _sum_of_groups(a)
    print("memory() after the passes:", a)
    print("whole test %.1f s" % (time.time() - t0))
    o.close(); eng.close(); ix.close()
