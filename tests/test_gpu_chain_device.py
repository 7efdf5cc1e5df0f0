"""The device chainer (cs_chain_batch_gpu / cs_chain_batch_device, compseed_amd/csrc/chain_gpu.hip) against the reference's own mem_chain
(the chain goldens) and against the host chainer cs_chain_batch, bit for bit, with flags 0 (sorted-array fast path, B-tree replay for reads
with equal keys) and with CS_CHAIN_TREE_ONLY (every read on the B-tree path)."""
import os
import shutil

import numpy as np
import pytest

import _data
from test_chain import check_chains, golden_chains

pytestmark = pytest.mark.gpu

FLAGS = [0, 1]   # 0, CS_CHAIN_TREE_ONLY
G = os.path.dirname(_data.GOLD)
ENGINE_RUNS = [("main100", "default"), ("repeat100", "default"), ("ragged", "k14"), ("sorted150", "r1.0"), ("main100", "c50s20")]


def _golden_in(z):
    import compseed_amd as ca
    mems = np.zeros(z["mems"].shape[0], dtype=ca.INTV_DT)
    mems["x0"], mems["x1"], mems["x2"], mems["info"] = z["mems"][:, 0], z["mems"][:, 1], z["mems"][:, 2], z["mems"][:, 3]
    seeds = np.zeros(z["seed_rbeg"].size, dtype=ca.SEED_DT)
    seeds["rbeg"], seeds["qbeg"], seeds["len"] = z["seed_rbeg"], z["seed_qbeg"], z["seed_len"]
    return z["mem_off"], mems, z["seed_off"], seeds


def _cp(kw):
    import compseed_amd as ca
    return ca.ChainParams(k=kw.get("k", 19), c=kw.get("c", 500))


def _same(a, b):
    for k in ("chain_off", "chains", "cseed_off", "cseeds"):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


@pytest.fixture(scope="module")
def chainer():
    import compseed_amd as ca
    c = ca.Chainer(_data.PREFIX, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def eng():
    import compseed_amd as ca
    ix = ca.Index.load(_data.PREFIX)
    e = ca.Engine(ix, 0)
    yield e
    e.close()
    ix.close()


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name,pname", _data.golden_runs())
def test_golden_runs_chain_like_the_reference(chainer, name, pname, flags):
    z, kw = _data.load_golden(name, pname)
    _, off = _data.load_reads(name)
    got = chainer.chain_gpu(*_golden_in(z), off, _cp(kw), flags=flags)
    check_chains(got, golden_chains(name, pname))
    host = chainer.chain(*_golden_in(z), off, _cp(kw), threads=4)
    _same(got, host)


@pytest.mark.parametrize("flags", FLAGS)
def test_alt_contigs(tmp_path, flags):
    import compseed_amd as ca
    shutil.copy(_data.PREFIX + ".ann", tmp_path / "ref.ann")
    shutil.copy(os.path.join(G, "alt1", "ref.alt"), tmp_path / "ref.alt")
    z, _ = _data.load_golden("main100", "default")
    zc = np.load(os.path.join(G, "alt1", "main100.default.chains.npz"))
    _, off = _data.load_reads("main100")
    c = ca.Chainer(str(tmp_path / "ref"), device=0)
    check_chains(c.chain_gpu(*_golden_in(z), off, ca.ChainParams(), flags=flags), zc)
    assert set(zc["is_alt"].tolist()) == {0, 1}
    c.close()


@pytest.mark.parametrize("flags", FLAGS)
def test_engine_device_output_chained_on_the_device(eng, chainer, flags):
    """seed_batch_device -> chain_device -> download == the golden chains, for the runs of test_gpu_parity's chain test"""
    import compseed_amd as ca
    for name, pname in ENGINE_RUNS:
        z, kw = _data.load_golden(name, pname)
        bases, off = _data.load_reads(name)
        d_b, d_o = eng.alloc(bases.nbytes), eng.alloc(off.nbytes)
        eng.upload(d_b, bases); eng.upload(d_o, off)
        r = eng.seed_batch_device(d_b, d_o, off.size - 1, bases.size, ca.Params(**kw))
        d = chainer.chain_device(r, d_o, _cp(kw), flags=flags)
        got = ca.download_chains(eng, d)
        check_chains(got, golden_chains(name, pname))
        assert d["n_chains"] == got["chains"].size and d["n_seeds"] == got["cseeds"].size
        eng.free(d_b); eng.free(d_o)


@pytest.mark.parametrize("flags", FLAGS)
def test_engine_device_stream_chained_between_submits(eng, chainer, flags):
    """submit_device / collect_device with two batches in flight; every collected batch is chained before the next submit"""
    import compseed_amd as ca
    bufs = []
    for name, pname in ENGINE_RUNS:
        z, kw = _data.load_golden(name, pname)
        bases, off = _data.load_reads(name)
        d_b, d_o = eng.alloc(bases.nbytes), eng.alloc(off.nbytes)
        eng.upload(d_b, bases); eng.upload(d_o, off)
        bufs.append((name, pname, kw, d_b, d_o, off, bases.size))
    eng.sync()
    submitted = 0
    for i in range(len(bufs)):
        while submitted < len(bufs) and submitted < i + 2:
            _, _, kw, d_b, d_o, off, nb = bufs[submitted]
            eng.submit_device(d_b, d_o, off.size - 1, nb, ca.Params(**kw))
            submitted += 1
        r = eng.collect_device()
        name, pname, kw, _, d_o, _, _ = bufs[i]
        got = ca.download_chains(eng, chainer.chain_device(r, d_o, _cp(kw), flags=flags))
        check_chains(got, golden_chains(name, pname))
    for b in bufs:
        eng.free(b[3]); eng.free(b[4])


@pytest.mark.parametrize("name,pname,n_tree", [("repeat100", "default", 5), ("main100", "default", 1), ("ragged", "k14", 0)])
def test_tree_path_coverage(chainer, name, pname, n_tree):
    """a read takes the tree path exactly when two of its final chains share a pos (counts read from the chain goldens)"""
    z, kw = _data.load_golden(name, pname)
    _, off = _data.load_reads(name)
    zc = golden_chains(name, pname)
    co = zc["chain_off"].astype(np.int64)
    dup = sum(np.unique(zc["pos"][co[r]:co[r + 1]]).size < co[r + 1] - co[r] for r in range(co.size - 1))
    assert dup == n_tree
    if name == "ragged":
        assert np.diff(co).max() > 1000      # the large-read (wave) variant of the fast path
    s0 = chainer.stats()
    check_chains(chainer.chain_gpu(*_golden_in(z), off, _cp(kw), flags=0), zc)
    s1 = chainer.stats()
    assert s1["tree_reads"] - s0["tree_reads"] == n_tree and s1["reads"] - s0["reads"] == off.size - 1
    check_chains(chainer.chain_gpu(*_golden_in(z), off, _cp(kw), flags=1), zc)
    s2 = chainer.stats()
    assert s2["tree_reads"] - s1["tree_reads"] == off.size - 1
    assert s2["chains"] - s1["chains"] == zc["pos"].size and s2["launches"] > s1["launches"] and s2["kernel_ms"] > s1["kernel_ms"]


def _ann_contigs(prefix):
    toks = open(prefix + ".ann").read().split("\n")
    l_pac, n = int(toks[0].split()[0]), int(toks[0].split()[1])
    offs = [int(toks[2 + 2 * i].split()[0]) for i in range(n)]
    return l_pac, offs


def _random_batch(n_reads, seed):
    """reads whose seeds come from a few positions (equal keys and node splits everywhere), seeds across a contig boundary and across the
    forward/reverse boundary, reads shorter than -k, reads without seeds, reads of more than 1,000 chains; mems with x2 above and below -c"""
    import compseed_amd as ca
    rng = np.random.default_rng(seed)
    l_pac, offs = _ann_contigs(_data.PREFIX)
    lens, seeds, mems, so, mo = [], [], [], [0], [0]
    for r in range(n_reads):
        L = int(rng.choice([12, 150, 150, 150, 400]))
        kind = rng.random()
        if kind < 0.05:
            ns = 0
        elif kind < 0.056:
            ns = int(rng.integers(1300, 1600))
        elif kind < 0.25:
            ns = int(rng.integers(65, 300))
        else:
            ns = int(rng.integers(1, 40))
        if ns > 1000:   # many distinct, scattered positions: one chain each
            rb = rng.integers(0, 2 * l_pac - 50, ns)
        else:
            base = rng.integers(0, 2 * l_pac - 2000, int(rng.integers(1, 6)))
            rb = base[rng.integers(0, base.size, ns)] + rng.choice([0, 0, 0, 1, 7, 60, 150, 300], ns)
        s = np.zeros(ns, dtype=ca.SEED_DT)
        s["rbeg"] = rb; s["qbeg"] = rng.integers(0, max(1, L - 19), ns); s["len"] = rng.integers(19, 45, ns)
        special = rng.random(ns)
        for i in np.nonzero(special < 0.03)[0]:
            s["rbeg"][i] = offs[int(rng.integers(1, len(offs)))] - int(rng.integers(1, 15)) if len(offs) > 1 else l_pac - 5
        for i in np.nonzero((special >= 0.03) & (special < 0.05))[0]:
            s["rbeg"][i] = l_pac - int(rng.integers(1, 15))
        seeds.append(s); so.append(so[-1] + ns); lens.append(L)
        nm = int(rng.integers(0, 5))
        b = np.sort(rng.integers(0, L, nm)); e = np.minimum(L, b + rng.integers(19, 80, nm))
        m = np.zeros(nm, dtype=ca.INTV_DT)
        m["x2"] = rng.choice([1, 3, 499, 500, 501, 2000], nm); m["info"] = (b.astype(np.uint64) << np.uint64(32)) | e.astype(np.uint64)
        mems.append(m); mo.append(mo[-1] + nm)
    off = np.zeros(n_reads + 1, dtype=np.uint64); np.cumsum(np.array(lens, dtype=np.uint64), out=off[1:])
    return (np.array(mo, dtype=np.uint64), np.concatenate(mems), np.array(so, dtype=np.uint64), np.concatenate(seeds)), off


@pytest.mark.parametrize("seed", [1, 2])
def test_random_reads_against_the_host_chainer(chainer, seed):
    import compseed_amd as ca
    batch, off = _random_batch(3000, seed)
    host = chainer.chain(*batch, off, ca.ChainParams(), threads=8)
    per_read = np.diff(host["chain_off"].astype(np.int64))
    assert per_read.max() > 1000 and (per_read == 0).sum() > 100
    pos, co = host["chains"]["pos"], host["chain_off"].astype(np.int64)
    dup = sum(np.unique(pos[co[r]:co[r + 1]]).size < co[r + 1] - co[r] for r in range(off.size - 1))
    assert dup > 200
    for flags in FLAGS:
        s0 = chainer.stats()
        _same(chainer.chain_gpu(*batch, off, ca.ChainParams(), flags=flags), host)
        s1 = chainer.stats()
        assert s1["tree_reads"] - s0["tree_reads"] == (dup if flags == 0 else off.size - 1)
    p2 = ca.ChainParams(w=30, max_chain_gap=400, k=25, c=60)
    _same(chainer.chain_gpu(*batch, off, p2), chainer.chain(*batch, off, p2, threads=8))


def _seed_reads(eng, path):
    import compseed_amd as ca
    reads = [l.encode() for l in open(path).read().split("\n") if l]
    bases, off = _data.pack_reads(reads)
    r = eng.seed_batch(bases, off, ca.Params())
    return (r.mem_off, r.mems, r.seed_off, r.seeds), off


def test_long_reads(eng, chainer):
    import compseed_amd as ca
    batch, off = _seed_reads(eng, os.path.join(G, "flt1", "long90.txt"))
    host = chainer.chain(*batch, off, ca.ChainParams(), threads=4)
    zc = np.load(os.path.join(G, "flt1", "long90.chains.npz"))
    check_chains(host, zc)
    assert np.diff(zc["chain_off"].astype(np.int64)).max() > 9000
    for flags in FLAGS:
        _same(chainer.chain_gpu(*batch, off, ca.ChainParams(), flags=flags), host)
    batch, off = _seed_reads(eng, os.path.join(G, "ddp1", "gap3k.txt"))
    host = chainer.chain(*batch, off, ca.ChainParams(), threads=4)
    assert host["chains"].size > 100
    for flags in FLAGS:
        _same(chainer.chain_gpu(*batch, off, ca.ChainParams(), flags=flags), host)


def test_edge_cases(eng, chainer):
    import ctypes
    import compseed_amd as ca
    # no reads: an empty result, on both entry points
    e = chainer.chain_gpu(np.zeros(1, np.uint64), np.zeros(0, ca.INTV_DT), np.zeros(1, np.uint64), np.zeros(0, ca.SEED_DT), np.zeros(1, np.uint64))
    assert e["chain_off"].tolist() == [0] and e["chains"].size == 0 and e["cseed_off"].tolist() == [0] and e["cseeds"].size == 0

    class Empty:
        n_reads = n_mems = n_seeds = 0
        ptr = dict(mem_off=None, mems=None, seed_off=None, seeds=None)
    d = chainer.chain_device(Empty(), 0)
    assert (d["n_reads"], d["n_chains"], d["n_seeds"]) == (0, 0, 0)
    assert ca.download_chains(eng, d)["chain_off"].tolist() == [0]
    # want_sal = 0: CS_EINVAL, and the chainer works afterwards
    bases, off = _data.load_reads("main100")
    d_b, d_o = eng.alloc(bases.nbytes), eng.alloc(off.nbytes)
    eng.upload(d_b, bases); eng.upload(d_o, off)
    r = eng.seed_batch_device(d_b, d_o, off.size - 1, bases.size, ca.Params(want_sal=0))
    with pytest.raises(ca.CSError) as ei:
        chainer.chain_device(r, d_o)
    assert ei.value.code == -1
    z, kw = _data.load_golden("main100", "default")
    mem_off, mems, _, _ = _golden_in(z)
    mem_off = np.ascontiguousarray(mem_off, dtype=np.uint64)
    res = ca.binding.CResult(off.size - 1, mems.size, 0, mem_off.ctypes.data, mems.ctypes.data, None, None)
    out = ca.binding.CChainResult()
    assert ca.load_library().cs_chain_batch_gpu(chainer._h, ctypes.byref(ca.ChainParams()), ctypes.byref(res), off.ctypes.data, 0, ctypes.byref(out)) == -1
    # a small batch, then a larger one: the buffers grow and the result is right
    n0 = 100
    zin = _golden_in(z)
    so = z["seed_off"].astype(np.int64); mo = z["mem_off"].astype(np.int64)
    small = (z["mem_off"][:n0 + 1], zin[1][:mo[n0]], z["seed_off"][:n0 + 1], zin[3][:so[n0]])
    _same(chainer.chain_gpu(*small, off[:n0 + 1]), chainer.chain(*small, off[:n0 + 1], threads=1))
    r = eng.seed_batch_device(d_b, d_o, off.size - 1, bases.size, ca.Params(**kw))
    check_chains(ca.download_chains(eng, chainer.chain_device(r, d_o)), golden_chains("main100", "default"))
    eng.free(d_b); eng.free(d_o)
