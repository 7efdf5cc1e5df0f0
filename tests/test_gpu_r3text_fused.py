"""r3text_kernel on an index whose 8-byte inverse-SA entries carry rep[] (engine option sa64 on the fixture; the default at hg19 scale):
the fused instantiation, the register-held cover scan with more mems than it holds, the slots taken without atomics for complete reads
and with atomics for the others.  Results never depend on any of it, so the specification is the reference's golden vectors, the oracle
and cs_engine_check_index."""
import gzip
import os

import numpy as np
import pytest

import _data
import _oracle
from test_gpu_parity import _check_against_golden

pytestmark = pytest.mark.gpu

POISON = np.uint64(0xdeadbeefdeadbeef)
VIOLATIONS = ("order_violations", "isa_violations", "bwt_violations", "sampled_sa_violations", "undecided_rows")


@pytest.fixture(scope="module")
def ix():
    import compseed_amd as ca
    i = ca.Index.load(_data.PREFIX)
    yield i
    i.close()


@pytest.fixture(scope="module")
def eng_fused(ix):
    import compseed_amd as ca
    e = ca.Engine(ix, 0, sa64=1)
    yield e
    e.close()


def _goldens(e, runs=None, **pkw):
    import compseed_amd as ca
    for name, pname in (runs or _data.golden_runs()):
        z, kw = _data.load_golden(name, pname)
        bases, off = _data.load_reads(name)
        _check_against_golden(e.seed_batch(bases, off, ca.Params(**kw, **pkw)), z)


def test_every_golden_through_the_fused_path(eng_fused):
    eng_fused.reset_stats()
    _goldens(eng_fused)
    assert eng_fused.stats()["r3_text_seeds"] > 0          # round 3 did run from the text
    _goldens(eng_fused, sst_mode=0)


@pytest.mark.parametrize("opts", [dict(), dict(sa40=1)], ids=["isa32", "isa40"])
def test_every_golden_through_the_unfused_path(ix, opts):
    """4-byte and 40-bit inverse-SA entries have no spare byte: r3text_kernel<false>, which reads rep[] itself"""
    import compseed_amd as ca
    e = ca.Engine(ix, 0, **opts)
    _goldens(e)
    assert e.stats()["r3_text_seeds"] > 0
    _goldens(e, sst_mode=0)
    e.close()


def test_check_index_on_a_fused_engine(eng_fused):
    """isa_violations counts a row whose masked entry is not the rank, and a fused entry whose top byte is not rep[p]"""
    n = int(eng_fused._index.view.seq_len)
    chk = eng_fused.check_index()
    assert chk["rows_checked"] == n
    assert all(chk[k] == 0 for k in VIOLATIONS), chk
    got = eng_fused.sa(np.arange(0, n + 1, dtype=np.uint64))
    assert not (got == POISON).any()


PIECE = 29


def _many_mem_reads():
    """reads of seven or eight exact 29-base pieces from different places of the fixture genome, each unique in it (one SMEM of one
    occurrence when seeded on its own), the base after each piece substituted so that the match ends there: 209 and 239 bases"""
    rng = np.random.default_rng(29)
    fa = gzip.open(os.path.join(_data.GOLD, "ref.fa.gz")).read().decode().split("\n")
    g = "".join(l for l in fa if not l.startswith(">"))
    o = _oracle.OracleIndex(_data.PREFIX)
    cand = [int(p) for p in rng.integers(0, len(g) - PIECE - 1, 4000) if "N" not in g[int(p):int(p) + PIECE + 1]]
    bases, off = _data.pack_reads([g[p:p + PIECE].encode() for p in cand])
    w = o.seed_batch(bases, off, _oracle.make_params(), mode=0, threads=4)
    mo = w["mem_off"].astype(np.int64)
    whole = np.uint64(PIECE)                                   # info = begin << 32 | end
    uniq = [p for j, p in enumerate(cand)
            if any(int(m["x2"]) == 1 and m["info"] == whole for m in w["mems"][mo[j]:mo[j + 1]])]
    reads = []
    for i in range(240):
        npieces = 7 + (i & 1)
        parts = []
        for p in rng.choice(len(uniq), npieces, replace=False):
            p = uniq[int(p)]
            nxt = g[p + PIECE]
            parts.append(g[p:p + PIECE] + "ACGT"[("ACGT".index(nxt) + 1 + int(rng.integers(0, 3))) % 4])
        reads.append("".join(parts)[:-1].encode())
    bases, off = _data.pack_reads(reads)
    want = o.seed_batch(bases, off, _oracle.make_params(), mode=0, threads=4)
    o.close()
    return bases, off, want


def test_more_mems_than_the_register_scan_holds(eng_fused):
    bases, off, want = _many_mem_reads()
    assert 190 <= int(np.diff(off.astype(np.int64)).min()) and int(np.diff(off.astype(np.int64)).max()) <= 250
    mo = want["mem_off"].astype(np.int64)
    info = want["mems"]["info"]
    ln = (info & np.uint64(0xffffffff)).astype(np.int64) - (info >> np.uint64(32)).astype(np.int64)
    long_per_read = np.add.reduceat((ln >= 25).astype(np.int64), mo[:-1])
    long_per_read[mo[:-1] == mo[1:]] = 0
    assert int((long_per_read > 6).sum()) >= 100               # precondition: beyond any number of mems the kernel keeps in registers
    eng_fused.reset_stats()
    got = eng_fused.seed_batch(bases, off)
    assert eng_fused.stats()["r3_text_seeds"] > 0
    assert np.array_equal(got.mem_off, want["mem_off"]) and np.array_equal(got.mems, want["mems"])
    assert np.array_equal(got.seed_off, want["seed_off"]) and np.array_equal(got.seeds, want["seeds"])


def test_atomic_slots_and_overflow_records(ix):
    """mem_cap 8: a read with more than 8 mems is not `complete`, takes its slots with atomics and spills into the overflow records"""
    import compseed_amd as ca
    e = ca.Engine(ix, 0, sa64=1, mem_cap=8)
    e.reset_stats()
    res = []
    for name in ("main100", "sorted150"):
        z, kw = _data.load_golden(name, "default")
        bases, off = _data.load_reads(name)
        res.append((e.seed_batch(bases, off, ca.Params(**kw)), z))
    assert e.stats()["overflow_mems"] > 0
    for r, z in res:
        _check_against_golden(r, z)
    e.close()


@pytest.mark.parametrize("it", [1, 2, 5, 99])
def test_pending_reads_beside_the_kernel(ix, it):
    """r3_text_iter moves the launch: at 1 most reads still have calls queued (not complete), at 99 none has"""
    import compseed_amd as ca
    e = ca.Engine(ix, 0, sa64=1, r3_text_iter=it)
    _goldens(e, runs=[("main100", "default"), ("sorted150", "default"), ("repeat100", "default"), ("ragged", "k14")])
    assert e.stats()["r3_text_seeds"] > 0
    e.close()
