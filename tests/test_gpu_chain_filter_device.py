"""The device chain filter (cs_chain_filter_gpu / cs_chain_filter_device, compseed_amd/csrc/chain_filter_gpu.hip) against the reference's own
filtered chains (tests/golden/aln1, flt1) and against the host filter cs_chain_filter, byte for byte, with flags 0 (one lane per light
read, one wave per heavier one) and with CS_FLT_WAVE_ONLY (every read on the wave path)."""
import os

import numpy as np
import pytest

import _data
from test_chain import golden_chains
from test_chain_filter import ALN, FLT, _chains_in, _long_reads, check_filtered
from test_gpu_chain_device import ENGINE_RUNS, _ann_contigs, _cp

pytestmark = pytest.mark.gpu

FLAGS = [0, 1]   # 0, CS_FLT_WAVE_ONLY
KEYS = ("chain_off", "chains", "cseed_off", "cseeds", "cseed_score")
LIGHT_MAX, LDS_CAP = 16, 512     # chain_filter_gpu.hip: reads of more chains go one wave per read; lists of more chains do not fit the LDS
GOLDENS = ["main100", "repeat100", "sorted150", "ragged"]


def _same(a, b, keys=KEYS):
    for k in keys:
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


def test_goldens_cover_the_sort_and_both_paths():
    """kept chains per read in the four golden sets: 272 reads with 3..16 (the introsort's first partition runs, the rest is left to the
    insertion sort), 91 with more than 16 (the quicksort proper; the wave path), at most 502 (under the LDS cap)"""
    few = many = top = 0
    for name in GOLDENS:
        kept = np.diff(np.load(os.path.join(ALN, name + ".aln.npz"))["chain_off"].astype(np.int64))
        few += int(((kept >= 3) & (kept <= 16)).sum()); many += int((kept > 16).sum()); top = max(top, int(kept.max()))
    assert (few, many, top) == (272, 91, 502) and top <= LDS_CAP


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", GOLDENS)
def test_filtered_golden_chains_are_the_references(chainer, name, flags):
    zc = golden_chains(name, "default")
    z = np.load(os.path.join(ALN, name + ".aln.npz"))
    bases, off = _data.load_reads(name)
    s0 = chainer.filter_stats()
    got = chainer.filter_gpu(*_chains_in(zc), bases, off, flags=flags)
    s1 = chainer.filter_stats()
    check_filtered(got, z)
    _same(got, chainer.filter(*_chains_in(zc), bases, off, threads=4))
    per_read = np.diff(zc["chain_off"].astype(np.int64))
    wave = int((per_read > LIGHT_MAX).sum()) if flags == 0 else int((per_read > 0).sum())
    assert s1["wave_reads"] - s0["wave_reads"] == wave and s1["reads"] - s0["reads"] == off.size - 1
    if flags == 0:
        assert wave > 0 and int(((per_read > 0) & (per_read <= LIGHT_MAX)).sum()) > 0          # light and wave reads both occurred
    assert s1["chains_in"] - s0["chains_in"] == zc["pos"].size and s1["chains_out"] - s0["chains_out"] == got["chains"].size
    assert s1["seeds_out"] - s0["seeds_out"] == got["cseeds"].size
    assert s1["launches"] > s0["launches"] and s1["kernel_ms"] > s0["kernel_ms"]


@pytest.mark.parametrize("flags", FLAGS)
def test_long_reads_seed_test_is_the_references(chainer, flags):
    import compseed_amd as ca
    zc = np.load(os.path.join(FLT, "long90.chains.npz"))
    z = np.load(os.path.join(FLT, "long90.aln.npz"))
    bases, off = _long_reads()
    assert (zc["pos"].size, z["chain_pos"].size, zc["seed_rbeg"].size, z["cseed_rbeg"].size) == (42106, 39634, 61010, 57627)
    s0 = chainer.filter_stats()
    got = chainer.filter_gpu(*_chains_in(zc), bases, off, flags=flags)
    s1 = chainer.filter_stats()
    check_filtered(got, z)
    assert s1["sw_seeds"] - s0["sw_seeds"] > 1000 and s1["spill_reads"] > s0["spill_reads"]          # (reads of more than 9,000 chains)
    with pytest.raises(ca.CSError) as ei:
        chainer.filter_gpu(*_chains_in(zc), None, off, flags=flags)                                    # the seed test needs the reads
    assert ei.value.code == -1


@pytest.mark.parametrize("flags", FLAGS)
def test_engine_device_chains_filtered_on_the_device(eng, chainer, flags):
    """seed_batch_device -> chain_device -> filter_device -> download == the host filter of the downloaded chains (and the aln1 golden for
    default seeding parameters); the chainer's unfiltered device output is left as it was"""
    import compseed_amd as ca
    for name, pname in ENGINE_RUNS:
        z, kw = _data.load_golden(name, pname)
        bases, off = _data.load_reads(name)
        d_b, d_o = eng.alloc(bases.nbytes), eng.alloc(off.nbytes)
        eng.upload(d_b, bases); eng.upload(d_o, off)
        r = eng.seed_batch_device(d_b, d_o, off.size - 1, bases.size, ca.Params(**kw))
        d = chainer.chain_device(r, d_o, _cp(kw))
        before = ca.download_chains(eng, d)
        fd = chainer.filter_device(d, d_b, d_o, flags=flags)
        got = ca.download_chains(eng, fd)
        assert fd["n_chains"] == got["chains"].size and fd["n_seeds"] == got["cseeds"].size == got["cseed_score"].size
        _same(got, chainer.filter(before["chain_off"], before["chains"], before["cseed_off"], before["cseeds"], bases, off, threads=4))
        if pname == "default":
            check_filtered(got, np.load(os.path.join(ALN, name + ".aln.npz")))
        _same(ca.download_chains(eng, d), before, KEYS[:4])
        assert set(fd[k] for k in KEYS[:4]).isdisjoint(d[k] for k in KEYS[:4])                        # buffers of their own
        eng.free(d_b); eng.free(d_o)


COUNTS = [0, 1, 2, 3, 16, 17, 18, 33, 63, 64, 65, 200, LDS_CAP, LDS_CAP + 1]


def _random_chains(n_reads, seed):
    """150-base reads; chains per read from COUNTS; one seed per chain mostly, its length -- the chain's weight -- from four values, so
    that ties dominate; spans on the read overlap at random; is_alt mixed"""
    import compseed_amd as ca
    rng = np.random.default_rng(seed)
    per_read = np.array([COUNTS[r % len(COUNTS)] for r in range(n_reads)], dtype=np.int64)
    rng.shuffle(per_read)
    nc = int(per_read.sum())
    nseeds = rng.choice([1, 1, 1, 2, 3], nc)
    cseed_off = np.zeros(nc + 1, dtype=np.uint64); np.cumsum(nseeds.astype(np.uint64), out=cseed_off[1:])
    ns = int(cseed_off[-1])
    cseeds = np.zeros(ns, dtype=ca.SEED_DT)
    cseeds["len"] = rng.choice([19, 40, 60, 100], ns)
    first = np.repeat(cseed_off[:-1].astype(np.int64), nseeds)           # seeds after a chain's first continue it: shifted a little on both axes
    k_in = np.arange(ns) - first
    q0 = rng.integers(0, 150 - 19, nc); r0 = rng.integers(0, 400000, nc)
    cseeds["qbeg"] = np.minimum(np.repeat(q0, nseeds) + k_in * rng.integers(0, 12, ns), 150 - cseeds["len"])
    cseeds["rbeg"] = np.repeat(r0, nseeds) + k_in * rng.integers(0, 30, ns)
    chains = np.zeros(nc, dtype=ca.CHAIN_DT)
    chains["pos"] = r0; chains["rid"] = rng.integers(0, 2, nc); chains["n_seeds"] = nseeds
    chains["frac_rep"] = rng.random(nc).astype(np.float32); chains["is_alt"] = rng.random(nc) < 0.2
    chain_off = np.zeros(n_reads + 1, dtype=np.uint64); np.cumsum(per_read.astype(np.uint64), out=chain_off[1:])
    off = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(150)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 150 * n_reads)]
    return (chain_off, chains, cseed_off, cseeds), bases, off, per_read


@pytest.fixture(scope="module")
def random_batch():
    return _random_chains(294, 7)


PARAM_SETS = [dict(), dict(drop_ratio=0.0), dict(drop_ratio=0.9), dict(mask_level=0.1), dict(max_chain_extend=1), dict(max_chain_extend=2), dict(min_chain_weight=30)]


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kw", PARAM_SETS, ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()) or "default")
def test_random_chains_against_the_host_filter(chainer, random_batch, kw, flags):
    import compseed_amd as ca
    batch, bases, off, per_read = random_batch
    assert 200 < per_read.size < 1000 and 20000 < batch[1].size < 100000 and set(COUNTS) <= set(per_read.tolist())
    host = chainer.filter(*batch, bases, off, ca.FltParams(**kw), threads=8)
    assert 0 < host["chains"].size <= batch[1].size
    s0 = chainer.filter_stats()
    _same(chainer.filter_gpu(*batch, bases, off, ca.FltParams(**kw), flags=flags), host)
    s1 = chainer.filter_stats()
    assert s1["spill_reads"] - s0["spill_reads"] == int((per_read > LDS_CAP).sum()) >= 1
    assert s1["wave_reads"] - s0["wave_reads"] == int((per_read > (LIGHT_MAX if flags == 0 else 0)).sum())


def _edge_batch(seed):
    """1,000-base reads of random bases with hand-made chains whose seeds lie within 50 bases of position 0, of the boundary between the
    two contigs, of l_pac from either side and of 2 l_pac; seed lengths 19, 199 and 200 (`< 200` decides at 200) and three between (a window of 200
    or more is not scored: at the ends of a strand or of the read the clipped window of a longer seed still is).  Half of the seeds are
    copied from the reference into the read, so that scores on both sides of the threshold occur."""
    import compseed_amd as ca
    rng = np.random.default_rng(seed)
    l_pac, offs = _ann_contigs(_data.PREFIX)
    assert len(offs) == 2
    fwd = _data.load_pac_forward()
    both = np.concatenate([fwd, 3 - fwd[::-1]])
    L, n_reads = 1000, 6
    reads = rng.integers(0, 4, (n_reads, L)).astype(np.uint8)
    seeds, chains, per_read = [], [], []
    for r in range(n_reads):
        rows = []
        for ln in (19, 60, 99, 140, 199, 200):
            for at in (0, offs[1], l_pac, 2 * l_pac):
                for _ in range(2):
                    rb = int(np.clip(at + rng.integers(-50 - ln, 51), 0, 2 * l_pac - ln))
                    qb = int(rng.choice([0, int(rng.integers(0, L - ln + 1)), L - ln, int(rng.integers(0, 50)), L - ln - int(rng.integers(0, 50))]))
                    rows.append((rb, qb, ln))
                    if rng.random() < 0.5:
                        reads[r, qb:qb + ln] = both[rb:rb + ln]
        for rb, qb, ln in rows:
            seeds.append((rb, qb, ln)); chains.append((rb, 0, 1, 0.0, 0))
        per_read.append(len(rows))
    cseeds = np.array(seeds, dtype=ca.SEED_DT); ch = np.array(chains, dtype=ca.CHAIN_DT)
    chain_off = np.zeros(n_reads + 1, dtype=np.uint64); np.cumsum(np.array(per_read, dtype=np.uint64), out=chain_off[1:])
    cseed_off = np.arange(ch.size + 1, dtype=np.uint64)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[reads.reshape(-1)]
    return (chain_off, ch, cseed_off, cseeds), bases, np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(L)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kw", [dict(), dict(a=2, b=3, o_del=4, e_del=2, o_ins=5, e_ins=1), dict(a=400)], ids=["default", "scores", "a400"])
def test_long_read_edge_windows_against_the_host_filter(chainer, kw, flags):
    """a = 400: the host's score matrix is int8_t, a match scores (int8_t)400 = -112 there while min_hsp and the unscored seeds take 400"""
    import compseed_amd as ca
    batch, bases, off = _edge_batch(11)
    par = ca.FltParams(drop_ratio=0.0, **kw)          # (every chain kept: every hand-made seed is scored)
    host = chainer.filter(*batch, bases, off, par, threads=1)
    assert ((host["cseed_score"] != host["cseeds"]["len"] * par.a).sum() > 20 or par.a == 400) and 0 < host["cseeds"].size < batch[3].size
    s0 = chainer.filter_stats()
    _same(chainer.filter_gpu(*batch, bases, off, par, flags=flags), host)
    assert chainer.filter_stats()["sw_seeds"] - s0["sw_seeds"] > 50
    _same(chainer.filter_gpu(*batch, bases, off, ca.FltParams(**kw), flags=flags), chainer.filter(*batch, bases, off, ca.FltParams(**kw), threads=1))


def test_edge_cases(eng, chainer):
    import ctypes
    import compseed_amd as ca
    z8 = np.zeros(1, np.uint64)
    for flags in FLAGS:
        # no reads: an empty result, on both entry points
        e = chainer.filter_gpu(z8, np.zeros(0, ca.CHAIN_DT), z8, np.zeros(0, ca.SEED_DT), None, z8, flags=flags)
        assert e["chain_off"].tolist() == [0] and e["cseed_off"].tolist() == [0] and e["chains"].size == e["cseeds"].size == e["cseed_score"].size == 0
        d = chainer.filter_device(dict(n_reads=0, n_chains=0, n_seeds=0, chain_off=None, chains=None, cseed_off=None, cseeds=None), None, None, flags=flags)
        assert (d["n_reads"], d["n_chains"], d["n_seeds"]) == (0, 0, 0) and ca.download_chains(eng, d)["chain_off"].tolist() == [0]
        # reads, none with chains
        off = np.arange(6, dtype=np.uint64) * np.uint64(150)
        e = chainer.filter_gpu(np.zeros(6, np.uint64), np.zeros(0, ca.CHAIN_DT), z8, np.zeros(0, ca.SEED_DT), None, off, flags=flags)
        assert e["chain_off"].tolist() == [0] * 6 and e["cseed_off"].tolist() == [0] and e["chains"].size == 0
        # a read whose chains all fall below min_chain_weight, between two that keep theirs
        chains = np.zeros(5, ca.CHAIN_DT); chains["n_seeds"] = 1; chains["pos"] = np.arange(5)
        cseeds = np.zeros(5, ca.SEED_DT); cseeds["len"] = [50, 20, 25, 29, 60]; cseeds["rbeg"] = 1000 * np.arange(5)
        args = (np.array([0, 1, 4, 5], np.uint64), chains, np.arange(6, dtype=np.uint64), cseeds, None, np.array([0, 150, 300, 450], np.uint64))
        e = chainer.filter_gpu(*args, ca.FltParams(min_chain_weight=30), flags=flags)
        assert e["chain_off"].tolist() == [0, 1, 1, 2] and e["chains"]["pos"].tolist() == [0, 4]
        _same(e, chainer.filter(*args, ca.FltParams(min_chain_weight=30)))
        # a chain without seeds: CS_EINVAL, and the chainer works on the next call
        bad = np.array([0, 1, 2, 2, 4, 5], np.uint64)
        with pytest.raises(ca.CSError) as ei:
            chainer.filter_gpu(args[0], chains, bad, cseeds, None, args[5], flags=flags)
        assert ei.value.code == -1
        with pytest.raises(ca.CSError) as ei:                                                   # chain_off beyond n_chains
            chainer.filter_gpu(np.array([0, 1, 9, 5], np.uint64), chains, args[2], cseeds, None, args[5], flags=flags)
        assert ei.value.code == -1
        wrong = chains.copy(); wrong["n_seeds"][3] = 2
        with pytest.raises(ca.CSError) as ei:                                                   # n_seeds that is not what cseed_off says
            chainer.filter_gpu(args[0], wrong, args[2], cseeds, None, args[5], flags=flags)
        assert ei.value.code == -1
        _same(chainer.filter_gpu(*args, flags=flags), chainer.filter(*args))
        # a read of 65,536 bases: CS_ERANGE (65,535 is served: no seed test without chains)
        with pytest.raises(ca.CSError) as ei:
            chainer.filter_gpu(*args[:5], np.array([0, 150, 150 + 65536, 150 + 65536 + 150], np.uint64), flags=flags)
        assert ei.value.code == -5
        # unknown flags
        with pytest.raises(ca.CSError) as ei:
            chainer.filter_gpu(*args, flags=2)
        assert ei.value.code == -1
    # the call's own previous output as input: CS_EINVAL (device arrays, then host arrays)
    bases, off = _data.load_reads("main100")
    zc = golden_chains("main100", "default")
    d_b, d_o = eng.alloc(bases.nbytes), eng.alloc(off.nbytes)
    eng.upload(d_b, bases); eng.upload(d_o, off)
    r = eng.seed_batch_device(d_b, d_o, off.size - 1, bases.size, ca.Params())
    fd = chainer.filter_device(chainer.chain_device(r, d_o), None, d_o)                         # (short reads: the reads are not needed)
    with pytest.raises(ca.CSError) as ei:
        chainer.filter_device(fd, d_b, d_o)
    assert ei.value.code == -1
    check_filtered(ca.download_chains(eng, chainer.filter_device(chainer.chain_device(r, d_o), d_b, d_o)), np.load(os.path.join(ALN, "main100.aln.npz")))
    eng.free(d_b); eng.free(d_o)
    v = chainer.filter_gpu(*_chains_in(zc), bases, off, copy=False)
    cin = ca.binding.CChainResult(v["chain_off"].size - 1, v["chains"].size, v["cseeds"].size, v["chain_off"].ctypes.data, v["chains"].ctypes.data,
                                  v["cseed_off"].ctypes.data, v["cseeds"].ctypes.data)
    out = ca.binding.CChainResult(); sc = ctypes.c_void_p()
    assert ca.load_library().cs_chain_filter_gpu(chainer._h, ctypes.byref(ca.FltParams()), ctypes.byref(cin), bases.ctypes.data, off.ctypes.data, 0,
                                                 ctypes.byref(out), ctypes.byref(sc)) == -1
