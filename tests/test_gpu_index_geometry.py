"""Seeding parity across index geometries: small genomes built in the test, the engine against the oracle.

Every other GPU test of the seeding path runs on one of five indexes: five values of seq_len, five positions of `primary`, one
suffix-array sampling phase each.  Here the genome is chosen for its geometry -- where the text ends inside a file block / a device
record / a 40-bit group / a sampling interval, where the `$` row falls, how far lcp[] and rep[] saturate -- and the whole path is held
to oracle/cs_index_naive.c + oracle/cs_oracle.c (pinned byte for byte against bwaidx and the reference's goldens, tests/test_oracle.py):
the builder's arrays word for word, the primitives on every row, cs_engine_check_index, and mems and seeds of a batch of reads cut
from both strands, the join between them and both ends of the text, on every instantiation of the suffix-array entries.

Nothing is left out: no genome, read or seed is skipped or filtered.  Every class a genome or a batch stands for is asserted from the
oracle's index / output or the engine's counters at run time.
"""
import numpy as np
import pytest

import _oracle

pytestmark = pytest.mark.gpu

POISON = np.uint64(0xdeadbeefdeadbeef)
NONE64 = np.uint64(2**64 - 1)
ASCII = np.frombuffer(b"ACGTN", dtype=np.uint8)
JUMP_K = 8          # 4^8 entries, 1 MB (the default 4^15-entry table is 17 GB per engine and adds nothing on these genomes)
EXHAUSTIVE_N = 2048  # primitives on every row up to this text length; beyond it occ4 / sa on every row still, extend from a stride of rows


# ---------------------------------------------------------------------------------------------------------------------- genomes
def _random(l_pac, seed):
    return np.random.default_rng(seed).integers(0, 4, l_pac).astype(np.uint8)


def _runs3000():
    """700 random bases, 600 T, 300 random, a 23-mer thirty times, random to the end: repeats and mems longer than 255"""
    rng = np.random.default_rng(3000)
    unit = rng.integers(0, 4, 23)
    head = [rng.integers(0, 4, 700), np.full(600, 3), rng.integers(0, 4, 300), np.tile(unit, 30)]
    n_head = sum(p.size for p in head)
    return np.concatenate(head + [rng.integers(0, 4, 3000 - n_head)]).astype(np.uint8)


def _run_first(base, seed):
    """forty times `base`, then 960 random bases: suffix 0 is the largest (T) or the smallest (A) of a text that has all four bases"""
    return np.concatenate([np.full(40, base), np.random.default_rng(seed).integers(0, 4, 960)]).astype(np.uint8)


P0_SEED = 1470  # the first seed whose 1000-base genome has primary % 128 == 0 (searched from 1000 on, one CPU build per try)

# name -> (genome, checks of its class on the oracle's index: each a (description, predicate of (primary, n, n_sa)))
def _size_class(l_pac, *extra):
    return [("seq_len == 2 * l_pac", lambda p, n, s, l=l_pac: n == 2 * l), ("n_sa", lambda p, n, s: s == (n + 32) // 32)] + list(extra)


GENOMES = {
    "r32": (lambda: _random(32, 7032), _size_class(32, ("one device record", lambda p, n, s: (n + 63) // 64 == 1))),
    "r33": (lambda: _random(33, 7033), _size_class(33, ("two device records, one file block", lambda p, n, s: (n + 63) // 64 == 2 and (n + 127) // 128 == 1))),
    "r64": (lambda: _random(64, 7064), _size_class(64, ("exactly one file block", lambda p, n, s: n == 128))),
    "r96": (lambda: _random(96, 7096), _size_class(96, ("last block holds exactly 64 rows", lambda p, n, s: n % 128 == 64))),
    "r97": (lambda: _random(97, 7097), _size_class(97, ("last block holds 66 rows", lambda p, n, s: n % 128 == 66))),
    "r128": (lambda: _random(128, 7128), _size_class(128, ("two full file blocks", lambda p, n, s: n == 256))),
    "r1000": (lambda: _random(1000, 8000), _size_class(1000, ("n % 32 == 16", lambda p, n, s: n % 32 == 16))),
    "r1008": (lambda: _random(1008, 8008), _size_class(1008, ("n % 32 == 0, n % 128 == 96", lambda p, n, s: n % 32 == 0 and n % 128 == 96))),
    "r1024": (lambda: _random(1024, 8024), _size_class(1024, ("n % 32 == 0, n % 128 == 0", lambda p, n, s: n % 32 == 0 and n % 128 == 0))),
    "r20000": (lambda: _random(20000, 20000), _size_class(20000)),
    # `primary` on the first / last row of a 64-row record and of a 128-row block (the seeds were found by search on the CPU)
    "p64": (lambda: _random(1000, 1053), _size_class(1000, ("primary % 128 == 64", lambda p, n, s: p % 128 == 64))),
    "p63": (lambda: _random(1000, 1167), _size_class(1000, ("primary % 128 == 63", lambda p, n, s: p % 128 == 63))),
    "p127": (lambda: _random(1000, 1170), _size_class(1000, ("primary % 128 == 127", lambda p, n, s: p % 128 == 127))),
    "p0": (lambda: _random(1000, P0_SEED), _size_class(1000, ("primary % 128 == 0", lambda p, n, s: p % 128 == 0))),
    # the extremes: the `$` row last (all T) and first (all A); also the widest intervals a small index has
    "allT100": (lambda: np.full(100, 3, np.uint8), _size_class(100, ("primary == seq_len", lambda p, n, s: p == n))),
    "allT1024": (lambda: np.full(1024, 3, np.uint8), _size_class(1024, ("primary == seq_len, % 64 == 0", lambda p, n, s: p == n and p % 64 == 0))),
    "allA100": (lambda: np.zeros(100, np.uint8), _size_class(100, ("primary == 1", lambda p, n, s: p == 1))),
    # the same two extremes on a text that holds every base (the three above lack C and G, and round 3 of such an index stays on the index)
    "tfirst": (lambda: _run_first(3, 4003), _size_class(1000, ("primary == seq_len", lambda p, n, s: p == n))),
    "afirst": (lambda: _run_first(0, 4000), _size_class(1000, ("primary == 1", lambda p, n, s: p == 1))),
    "runs3000": (_runs3000, _size_class(3000)),
}
LACKS_A_BASE = ("allT100", "allT1024", "allA100")  # T^n A^n: no C, no G (asserted from the oracle's L2)
FORCE_64BIT = ("r33", "p0", "runs3000")          # the builder's 64-bit instantiation as well
OTHER_JUMP = ("r20000", "runs3000")               # also seeded with the default jump table and with none
SIZES = ("r32", "r33", "r64", "r96", "r97", "r128", "r1000", "r1008", "r1024", "r20000")

# parameter sets (cs_params_t / cso_params_t): the defaults; k = 10 < the window scheme's range and c = 3 (round 3 still starts from
# the 8-mer table; nearly every mem is sampled); k = 19 with every long SMEM re-seeded and round 3 down to pairs
PARAM_SETS = {"default": dict(), "k10c3": dict(k=10, c=3), "k19r1y2": dict(k=19, r=1.0, y=2)}
ENGINES = {"default": dict(), "sa64": dict(sa64=1), "sa40": dict(sa40=1), "nofsa": dict(full_sa=0), "notext": dict(text_arrays=0)}
READ_LENGTHS = (20, 31, 32, 33, 47, 64, 65, 100, 150, 300)


def _sub(read, rng):
    r = read.copy()
    p = int(rng.integers(0, r.size))
    r[p] = (r[p] + int(rng.integers(1, 4))) & 3
    return r


def make_reads(fwd, seed=99):
    """the batch of a genome: reads cut from T = fwd ++ revcomp(fwd) at both ends of the text, across the join of the strands and at
    random; each exact, with one substitution and (from 47 bases on) with an N in the middle; ten random 60-mers; one all-N read"""
    rng = np.random.default_rng(seed)
    l_pac = fwd.size
    T = np.concatenate([fwd, 3 - fwd[::-1]]).astype(np.uint8)
    n = T.size
    reads = []
    for ln in READ_LENGTHS:
        if ln > n:
            continue
        fixed = [0, 1, n - ln, n - ln - 1, l_pac - ln // 2 - 1, l_pac - ln // 2, l_pac - ln // 2 + 1, l_pac - ln, l_pac]
        starts = []
        for s in fixed + [int(x) for x in rng.integers(0, n - ln + 1, 12)]:
            if 0 <= s <= n - ln and s not in starts:
                starts.append(s)
        for s in starts:
            exact = T[s:s + ln]
            reads.append(exact)
            reads.append(_sub(exact, rng))
            if ln >= 47:
                withn = exact.copy()
                withn[ln // 2] = 4
                reads.append(withn)
    for _ in range(10):
        reads.append(rng.integers(0, 4, 60).astype(np.uint8))
    reads.append(np.full(50, 4, np.uint8))
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([r.size for r in reads], out=off[1:])
    return ASCII[np.concatenate(reads)], off


class Genome:
    """CPU side of one genome, made once and shared: the genome, the oracle's index, the batch and the oracle's results"""

    def __init__(self, name):
        make, self.classes = GENOMES[name]
        self.name = name
        self.fwd = make()
        self.l_pac = int(self.fwd.size)
        self.o = _oracle.OracleIndex.build(self.fwd)
        i = self.o.idx
        self.primary, self.n, self.n_sa = int(i.primary), int(i.seq_len), int(i.n_sa)
        self.every_base = all(int(i.L2[b + 1]) > int(i.L2[b]) for b in range(4))
        self.bases, self.off = make_reads(self.fwd)
        self._want = {}

    def want(self, pname, want_sal=True):
        key = (pname, want_sal)
        if key not in self._want:
            self._want[key] = self.o.seed_batch(self.bases, self.off, _oracle.make_params(**PARAM_SETS[pname]), mode=0, want_sal=want_sal, threads=4)
        return self._want[key]


_GENOMES = {}


def genome(name):
    if name not in _GENOMES:
        _GENOMES[name] = Genome(name)
    return _GENOMES[name]


class Geo:
    """one genome on the GPU: the index from the engine's builder and engines made on request, closed together"""

    def __init__(self, name):
        import compseed_amd as ca
        self.ca = ca
        self.g = genome(name)
        self.ix = ca.Index.build(self.g.fwd, 0)
        self._eng = {}

    def engine(self, kind):
        if kind not in self._eng:
            self._eng[kind] = self.ca.Engine(self.ix, 0, jump_k=JUMP_K, **ENGINES[kind])
        return self._eng[kind]

    def close(self):
        for e in self._eng.values():
            e.close()
        self._eng = {}
        self.ix.close()


@pytest.fixture(scope="module", params=list(GENOMES))
def geo(request):
    c = Geo(request.param)
    yield c
    c.close()


def _same_result(got, want, what, sal=True):
    assert np.array_equal(got.mem_off, want["mem_off"]), what
    assert np.array_equal(got.mems, want["mems"]), what
    if sal:
        assert np.array_equal(got.seed_off, want["seed_off"]), what
        assert np.array_equal(got.seeds, want["seeds"]), what


# ------------------------------------------------------------------------------------------------- what the genomes stand for
def test_genome_classes(geo):
    """the geometry each genome is here for, from the oracle's index; between them rows % 3 takes every value"""
    g = geo.g
    for what, holds in g.classes:
        assert holds(g.primary, g.n, g.n_sa), (g.name, what, g.primary, g.n, g.n_sa)
    assert 1 <= g.primary <= g.n
    assert g.every_base == (g.name not in LACKS_A_BASE)
    assert {(genome(k).n + 1) % 3 for k in SIZES} == {0, 1, 2}        # how full the last 40-bit group of three entries is


def test_read_classes(geo):
    """the batch holds what it was cut for, by the oracle's seeds: matches that start the text, that end it and that cross the join of
    the strands; on runs3000 also seeds and intervals beyond what a byte of lcp[] / rep[] holds"""
    g = geo.g
    s = g.want("default")["seeds"]
    end = s["rbeg"] + s["len"]
    at_start, at_end, across = int((s["rbeg"] == 0).sum()), int((end == g.n).sum()), int(((s["rbeg"] < g.l_pac) & (end > g.l_pac)).sum())
    print(g.name, "seeds at the start / at the end / across the join:", at_start, at_end, across)
    assert at_end > 0 and across > 0, (g.name, at_start, at_end, across)
    # T^1024 A^1024: a run of T's from the batch occurs more than max_occ times and position 0 is the LAST row of its interval, which the
    # sampling (slots x0 + k * step, k < max_occ) never reaches, at c = 3 no more than at 500; every other genome has such seeds
    assert at_start > 0 or g.name == "allT1024", (g.name, at_start)
    assert g.name != "allT1024" or int((g.want("k10c3")["seeds"]["rbeg"] == 0).sum()) == 0
    if g.name == "runs3000":
        m = g.want("default")["mems"]
        assert int(s["len"].max()) > 255 and int(m["x2"].max()) > 255
    if g.name == "allT1024":
        assert int(g.want("default")["mems"]["x2"].max()) > 500    # x2 > max_occ at the defaults: sampled slots


# ------------------------------------------------------------------------------------------------------------------- 1. builder
def _same_index(ix, g):
    v = ix.view
    i = g.o.idx
    assert int(v.primary) == g.primary and int(v.seq_len) == g.n and int(v.n_sa) == g.n_sa and int(v.bwt_size) == int(i.bwt_size)
    assert [int(x) for x in v.L2] == [int(x) for x in i.L2]
    bw, sa = ix.arrays()
    obw, osa = g.o.arrays()
    assert np.array_equal(bw, obw)            # every word: the counts, the bases, the trailing count record
    assert np.array_equal(sa, osa)


def test_builder_equals_the_oracle(geo):
    _same_index(geo.ix, geo.g)
    if geo.g.name in FORCE_64BIT:
        ix = geo.ca.Index.build(geo.g.fwd, 0, force_64bit=True)
        try:
            _same_index(ix, geo.g)
        finally:
            ix.close()


# ---------------------------------------------------------------------------------------------------------------- 2. primitives
def test_occ4_on_every_row(geo):
    g = geo.g
    k = np.concatenate([[NONE64], np.arange(0, g.n + 1, dtype=np.uint64)])      # never beyond n: cs_engine_occ4 does not range-check
    got = geo.engine("default").occ4(k)
    want = np.array([g.o.occ4(int(x)) for x in k], dtype=np.uint64)
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0][:10]


@pytest.mark.parametrize("kind", ["default", "nofsa"])
def test_sa_on_every_row(geo, kind):
    """with the full suffix array resident sa_kernel also compares it with the walk and poisons a mismatch; full_sa = 0 walks only"""
    g = geo.g
    rows = np.arange(0, g.n + 1, dtype=np.uint64)
    got = geo.engine(kind).sa(rows)
    assert not (got == POISON).any(), np.nonzero(got == POISON)[0][:10]
    want = np.array([g.o.sa(int(r)) for r in rows], dtype=np.uint64)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]


def test_extend_from_every_row(geo):
    """bwt_extend, both directions, all four children, from intervals that start on every row: one and two rows, around a record's 64
    rows and a block's 128, and up to the last row"""
    g = geo.g
    n = g.n
    x0s = np.arange(1, n + 1) if n <= EXHAUSTIVE_N else np.unique(np.concatenate([np.arange(1, n + 1, 37), np.arange(max(1, g.primary - 130), min(n, g.primary + 130) + 1),
                                                                                       np.arange(n - 300, n + 1), np.arange(1, 300)]))
    iv = []
    for x0 in x0s:
        for x2 in {1, 2, 63, 64, 65, 128, n + 1 - int(x0)}:
            if x2 >= 1 and x0 + x2 <= n + 1:
                iv.append((int(x0), int(x2)))
    ik = np.zeros(2 * len(iv), dtype=geo.ca.INTV_DT)
    ik["x0"] = np.tile([a for a, _ in iv], 2); ik["x2"] = np.tile([b for _, b in iv], 2); ik["x1"] = 1
    back = np.repeat(np.array([1, 0], np.uint8), len(iv))
    # forward extension searches x1 = 1: rows 0 .. x2 <= n (never an interval beyond n)
    got = geo.engine("default").extend(ik, back)
    want = np.array([g.o.extend(int(a["x0"]), 1, int(a["x2"]), int(b)) for a, b in zip(ik, back)], dtype=np.uint64)   # [i, child, (x0, x1, x2)]
    for f, name in enumerate(("x0", "x1", "x2")):
        bad = np.nonzero((got[name] != want[:, :, f]).any(axis=1))[0]
        assert bad.size == 0, (name, [(int(ik["x0"][i]), int(ik["x2"][i]), int(back[i])) for i in bad[:5]])
    assert not got["info"].any()               # the single-child forms the search uses agree with the four-child one


# --------------------------------------------------------------------------------------------------------------- 3. check_index
@pytest.mark.parametrize("kind", ["default", "sa64", "sa40"])
def test_check_index_with_the_genome(geo, kind):
    g = geo.g
    e = geo.engine(kind)
    d = e.alloc(g.l_pac + 64)
    try:
        e.upload(d, g.fwd)
        chk = e.check_index(d, g.l_pac)
    finally:
        e.free(d)
    assert chk["rows_checked"] == g.n and chk["text_checked"] == 1, chk
    for k in ("order_violations", "isa_violations", "bwt_violations", "sampled_sa_violations", "undecided_rows", "text_violations"):
        assert chk[k] == 0, (k, chk)
    assert e.memory()["sa_entry_bits"] == {"default": 32, "sa64": 64, "sa40": 40}[kind]


# ------------------------------------------------------------------------------------------------------------------- 4. seeding
def _seed_all_sets(ca, g, e, what, extra=()):
    """every parameter set with every shortcut on and with sst_mode = 0 (plus `extra` keyword sets on the defaults): mem_off, mems,
    seed_off and seeds equal the oracle's; returns the counters of the runs with the shortcuts on"""
    e.reset_stats()
    for pname, kw in PARAM_SETS.items():
        _same_result(e.seed_batch(g.bases, g.off, ca.Params(**kw)), g.want(pname), (g.name, what, pname))
    st = e.stats()
    for pname, kw in PARAM_SETS.items():
        _same_result(e.seed_batch(g.bases, g.off, ca.Params(sst_mode=0, **kw)), g.want(pname), (g.name, what, pname, "sst_mode=0"))
    for kw in extra:
        _same_result(e.seed_batch(g.bases, g.off, ca.Params(**kw)), g.want("default"), (g.name, what, kw))
    return st


@pytest.mark.parametrize("kind", list(ENGINES))
def test_seeding_equals_the_oracle(geo, kind):
    ca = geo.ca
    g = geo.g
    e = geo.engine(kind)
    extra = [dict(disable=ca.binding.disable_mask("fused_sal"))] if kind == "default" else []
    st = _seed_all_sets(ca, g, e, kind, extra)
    m = e.memory()
    assert m["sa_entry_bits"] == {"default": 32, "sa64": 64, "sa40": 40, "nofsa": 0, "notext": 32}[kind]
    assert (m["lcp_rep"] > 0) == (kind in ("default", "sa64", "sa40")) and (m["text"] > 0) == (kind != "nofsa")
    print(g.name, kind, {k: st[k] for k in ("reseed_text_calls", "reseed_index_calls", "sweep_text_calls", "r3_text_seeds", "overflow_mems")})
    if kind in ("default", "sa64", "sa40") and g.l_pac >= 1000:
        # the text side did answer: re-seeding calls, backward sweeps and round-3 seeds
        assert st["reseed_text_calls"] > 0 and st["sweep_text_calls"] > 0, st
        # ... round 3 only where every mem is an occurrence: a text that lacks a base gives empty mems (a call whose pivot is that base),
        # and the engine keeps the round 3 of such an index on the index (seed_pass.hip, run_smem_split)
        assert (st["r3_text_seeds"] > 0) == g.every_base, st
    if kind == "nofsa":
        assert st["reseed_text_calls"] == 0 and st["sweep_text_calls"] == 0 and st["r3_text_seeds"] == 0, st


@pytest.mark.parametrize("name", OTHER_JUMP)
@pytest.mark.parametrize("opts", [dict(), dict(jump_k=0, kmer_filter=0)], ids=["jump15", "nojump"])
def test_seeding_with_other_jump_tables(name, opts):
    """the default table of every 15-mer, of which a genome of a few kbp holds next to none, and no table and no k-mer filter at all"""
    import compseed_amd as ca
    g = genome(name)
    ix = ca.Index.build(g.fwd, 0)
    e = ca.Engine(ix, 0, **opts)
    try:
        st = _seed_all_sets(ca, g, e, str(opts))
        assert st["reseed_text_calls"] > 0 and st["sweep_text_calls"] > 0 and st["r3_text_seeds"] > 0, st
        mem = e.memory()
        assert (mem["jump_table"] == 16 << 30) if not opts else (mem["jump_table"] == 0 and mem["kmer_filter"] == 0)
    finally:
        e.close(); ix.close()


# ---------------------------------------------------------------------------------------------------------------- 5. want_sal=0
def test_mems_without_sal(geo):
    """want_sal = 0 (no seeds wanted: another path through the sort): the same mems, on the widest intervals too (the all-T genomes)"""
    g = geo.g
    got = geo.engine("default").seed_batch(g.bases, g.off, geo.ca.Params(want_sal=0))
    _same_result(got, g.want("default"), (g.name, "want_sal=0"), sal=False)
