"""bwd_win_kernel settles every end in the iteration in which it stops and frees its lane at once (smem_bwd.hpp, CS_WIN_SETTLE): a lane
carries the stop position of the nearest valid end above it that has left, an end that reports waits as "pending" for a common flush, and
the call's successor is pushed at placement.  A small genome built here holds what that can get wrong, and every case compares, on ALL
its reads and with exact equality of mem_off, mems, seed_off and seeds, the default path with the oracle, with the sst_mode = 0 pass and
with disable = window (the literal sweep, which never enters this kernel) -- with jump_k 10 and 15, and once with disable = kmer_filter.

The genome (about 33 kbp, numpy's PCG64) is random background with
  * mosaics: for a random read R, copies of intervals R[l:t) framed by bases that differ from R[l - 1] and R[t].  What a call at pivot x
    sees is then known: the forward pass ends where the last copy that holds [x, ..) ends, it stores an LEP where a copy drops out, and
    the end t walks left as far as the copies that hold [x, t) agree with the read.
      stair    copies [0,50) [46,150) [40,130) [30,110) [20,90) [6,70): the call at pivot 50 has five LEPs that stop at 45, 39, 29, 19
               and 5 -- the longer to the right, the shorter to the left --, every one reported, 40 clock steps between the first and
               the last, the window ends tie with the last.  Its forward pass reaches the read's end: no successor.
      stair_n  the same shape with the longest copy ending at 140 and an ambiguous base there: the successor skips it.
      tiling   copies [0,60) [35,66) [52,150) [50,68): at pivot 60 one LEP that stops at 51, window ends 71..78 that tie with it, window
               ends 61..66 that walk on to 34 (66 reported), and between them -- with the k-mer filter off -- the ends 67 and 68, which
               stop alone at 49 with 17 and 18 bases: consulted by the ends below, never reported.
      reseed   a 150-base segment twice in full and once as [0,100): the read's SMEM [0,150) has two occurrences, its re-seeding call
               (pivot 75, min_intv 3) stores the LEP [75,100) and walks to the read start.
  * families F(3) and F(46) and 2-copy segments as tests/test_gpu_bwd_lane_sets.py builds them: calls whose ends all stop in one
    iteration (at the junk base; only the longest reported) and the narrow calls (one LEP, 19 lanes); and decoys that put a read's
    second pivot on the first base of F(46) with genuine sequence in front of it: the call of 46 LEPs and 18 passing window ends that
    needs all 64 lanes, in one batch with the narrow calls that share its draws.

How the input was checked on the CPU: call() below restates a call by counting occurrences in the text of both strands -- the forward
pass (stored LEPs, next pivot), the window ends that pass, the position at which every end stops, and who reports by the first-survivor
rule.  test_input_holds_the_classes asserts the classes above from it without a GPU call; it was run on a CPU-only machine when the
test was written.
"""
import numpy as np
import pytest

import _oracle

pytestmark = pytest.mark.gpu

ASCII = np.frombuffer(b"ACGTN", dtype=np.uint8)
K = 19                       # min_seed_len (the default)
WIN = K - 1
CORE, STEP = 40, 3
FAMILIES = (3, 46)
N_DUP, DUP_LEN = 8, 400
LEAD = 3
MOSAICS = {
    "stair": [(0, 50), (46, 150), (40, 130), (30, 110), (20, 90), (6, 70)],
    "stair_n": [(0, 50), (46, 140), (40, 130), (30, 110), (20, 90), (6, 70)],
    "tiling": [(0, 60), (35, 66), (52, 150), (50, 68)],
    "reseed": [(0, 150), (0, 150), (0, 100)],
}


class Data:
    """the genome, the reads by set and the oracle's results, made once"""

    def __init__(self):
        rng = np.random.default_rng(20263)
        parts = [rng.integers(0, 4, 3000)]
        self.mosaic = {}
        for name, copies in MOSAICS.items():
            R = rng.integers(0, 4, 150)
            self.mosaic[name] = R
            for l, t in copies:
                left = rng.integers(0, 4, 40)
                right = rng.integers(0, 4, 40)
                if l > 0:
                    left[-1] = (R[l - 1] + 1 + rng.integers(0, 3)) & 3
                if t < R.size:
                    right[0] = (R[t] + 1 + rng.integers(0, 3)) & 3
                parts += [left, R[l:t], right]
        self.fam = {}
        for N in FAMILIES:
            core, ext = rng.integers(0, 4, CORE), rng.integers(0, 4, STEP * (N - 1) + 1)
            full = np.concatenate([core, ext[:STEP * (N - 1)]])
            copies = [np.concatenate([core, ext[:STEP * j], [(ext[STEP * j] + 1 + rng.integers(0, 3)) & 3]]) for j in range(N - 1)] + [full, full]
            self.fam[N] = dict(full=full, lead=[])
            for c in rng.permutation(len(copies)):
                lead = rng.integers(0, 4, 60)
                lead[-1] = LEAD
                if copies[c] is copies[0]:
                    self.fam[N]["lead"] = lead[-30:]                   # genuine sequence in front of the shortest copy
                parts += [lead, copies[c], rng.integers(0, 4, 30)]
        # decoys: a random head + the 18 bases in front of F(46)'s shortest copy + a base that is not the core's first.  A read "head + those
        # 18 bases + F(46)" matches its decoy up to the core and gets its second pivot there: 46 LEPs, and 18 window ends whose k-mers
        # all occur (in front of the shortest copy)
        self.heads = [rng.integers(0, 4, 12) for _ in range(10)]
        lead18, core0 = self.fam[46]["lead"][-WIN:], self.fam[46]["full"][0]
        for Q in self.heads:
            parts += [rng.integers(0, 4, 40), Q, lead18, [(core0 + 1 + rng.integers(0, 3)) & 3], rng.integers(0, 4, 40)]
        self.dups = []
        for _ in range(N_DUP):
            seg = rng.integers(0, 4, DUP_LEN)
            self.dups.append(seg)
            parts += [seg, rng.integers(0, 4, 500), seg, rng.integers(0, 4, 300)]
        parts.append(rng.integers(0, 4, 3000))
        self.fwd = np.concatenate(parts).astype(np.uint8)
        self.T = np.concatenate([self.fwd, 3 - self.fwd[::-1]]).astype(np.uint8)
        self.o = _oracle.OracleIndex.build(self.fwd)
        # the reads (codes 0..3, 4 = ambiguous)
        self.reads = {name: R.astype(np.uint8).copy() for name, R in self.mosaic.items()}
        self.reads["stair_n"][140] = 4
        fam_reads, pass_reads, dup_reads = [], [], []
        for N in FAMILIES:
            full = self.fam[N]["full"]
            for _ in range(200):
                junk = rng.integers(0, 4, int(rng.integers(8, 13)))
                junk[-1] = (LEAD + 1 + rng.integers(0, 3)) & 3
                fam_reads.append(np.concatenate([junk, full]).astype(np.uint8))
        for Q in self.heads:
            pass_reads.append(np.concatenate([Q, lead18, self.fam[46]["full"]]).astype(np.uint8))
        for q in range(1000):
            seg = self.dups[q % N_DUP]
            s = int(rng.integers(0, DUP_LEN - 150))
            rd = seg[s:s + 150].copy()
            p = int(rng.integers(30, 60))
            rd[p] = (rd[p] + 1 + rng.integers(0, 3)) & 3
            dup_reads.append(rd.astype(np.uint8))
        self.fam_reads, self.pass_reads, self.dup_reads = fam_reads, pass_reads, dup_reads
        mixed = fam_reads + dup_reads + pass_reads * 20 + [self.reads[n] for n in MOSAICS] * 100
        order = rng.permutation(len(mixed))
        self.sets = {"all": [mixed[k] for k in order]}
        self.sets["one"] = [self.reads["stair"]]
        self.sets["three"] = [self.reads["stair"], self.reads["tiling"], self.reads["reseed"]]
        self.sets["sixty_five"] = [self.reads[n] for n in MOSAICS] * 4 + pass_reads + dup_reads[:20] + fam_reads[:19]
        assert len(self.sets["sixty_five"]) == 65
        self._batch, self._want = {}, {}

    def batch(self, name):
        if name not in self._batch:
            reads = self.sets[name]
            off = np.zeros(len(reads) + 1, dtype=np.uint64)
            np.cumsum([r.size for r in reads], out=off[1:])
            self._batch[name] = (ASCII[np.concatenate(reads)], off)
        return self._batch[name]

    def want(self, name):
        if name not in self._want:
            bases, off = self.batch(name)
            self._want[name] = self.o.seed_batch(bases, off, _oracle.make_params(), mode=0, want_sal=True, threads=4)
        return self._want[name]

    # ---- a call by counting in the text
    def _occ(self, s):
        """start positions in T of the string s (no ambiguous base in it)"""
        T = self.T
        pos = np.flatnonzero(T[:T.size - s.size + 1] == s[0])
        for k in range(1, s.size):
            pos = pos[T[pos + k] == s[k]]
        return pos

    def _stop(self, read, a, t, min_intv):
        """the end t, known to match from a on: the position f at which [f, t) no longer has min_intv occurrences (read start: -1)"""
        pos, c = self._occ(read[a:t]), a - 1
        while c >= 0 and read[c] < 4:
            pos = pos[pos > 0] - 1
            pos = pos[self.T[pos] == read[c]]
            if pos.size < min_intv:
                break
            c -= 1
        return c

    def call(self, read, x, min_intv=1, jump_k=10, kmer_filter=True):
        """the call at pivot x: dict(n, ret, ends = [(t, f, is_lep)] from the longest end down, reported = [(f + 1, t)])"""
        i, leps, size = x + 1, [], self._occ(read[x:x + 1]).size
        while i < read.size and read[i] < 4:
            nxt = self._occ(read[x:i + 1]).size
            if nxt != size:
                if nxt < min_intv:
                    break
                leps.append(i)
            size = nxt
            i += 1
        leps.append(i)
        ret = i
        leps = [t for t in leps if x != 0 and t - x >= K]              # what the forward pass stores under the window scheme
        ends = [(t, self._stop(read, x, t, min_intv), True) for t in leps]
        if leps:
            for te in range(x + 1, x + K):
                if te > ret or te - K < 0 or (read[te - K:te] > 3).any():
                    continue
                if kmer_filter and self._occ(read[te - K:te]).size == 0:
                    continue
                if self._occ(read[te - jump_k:te]).size < min_intv:
                    continue
                ends.append((te, self._stop(read, te - jump_k, te, min_intv), False))
        ends.sort(reverse=True)
        reported, above = [], None
        for t, f, _ in ends:                                            # the first-survivor rule and the length filter
            if (above is None or f < above) and t - (f + 1) >= K:
                reported.append((f + 1, t))
            above = f
        return dict(n=len(leps), ret=ret, ends=ends, reported=reported)

    def chain(self, read):
        """the pivots of the read's round-1 calls"""
        x, piv = 0, []
        while x < read.size:
            piv.append(x)
            x = self.call(read, x)["ret"]
            while x < read.size and read[x] > 3:
                x += 1
        return piv


_DATA = []


def data():
    if not _DATA:
        _DATA.append(Data())
    return _DATA[0]


@pytest.fixture(scope="module", params=[10, 15], ids=["jump10", "jump15"])
def gpu(request):
    import compseed_amd as ca
    d = data()
    ix = ca.Index.build(d.fwd, 0)
    e = ca.Engine(ix, 0, jump_k=request.param)
    yield ca, e
    e.close(); ix.close()


def _same(got, want, what):
    assert np.array_equal(got.mem_off, want["mem_off"]), what
    assert np.array_equal(got.mems, want["mems"]), what
    assert np.array_equal(got.seed_off, want["seed_off"]), what
    assert np.array_equal(got.seeds, want["seeds"]), what


def _same_runs(a, b, what):
    for k in ("mem_off", "mems", "seed_off", "seeds"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), (what, k)


def test_input_holds_the_classes():
    """no GPU call: what the reads stand for, from call()"""
    d = data()
    # stair: four ends or more stop valid in different iterations, 30 clock steps or more apart, two or more reported; no successor
    R = d.reads["stair"]
    assert d.chain(R)[:2] == [0, 50], d.chain(R)
    c = d.call(R, 50)
    stops = sorted({f for _, f, _ in c["ends"]}, reverse=True)
    assert c["n"] == 5 and stops == [45, 39, 29, 19, 5], (c["n"], stops)
    assert stops[0] - stops[-1] >= 30 and len(c["reported"]) == 5 and c["ret"] == R.size
    assert sum(not lep for _, _, lep in c["ends"]) == WIN and all(f == 5 for _, f, lep in c["ends"] if not lep)
    # stair_n: the same call, and its successor skips an ambiguous base
    R = d.reads["stair_n"]
    c = d.call(R, 50)
    assert c["n"] == 5 and c["ret"] == 140 and R[140] == 4 and d.chain(R)[:3] == [0, 50, 141], (c["n"], c["ret"], d.chain(R))
    # tiling: with the filter off, an end that stops short of min_seed_len, alone in its iteration, between a longer end that left
    # before it and a shorter one that walks on and reports
    R = d.reads["tiling"]
    assert d.chain(R)[:2] == [0, 60], d.chain(R)
    c = d.call(R, 60)
    assert c["n"] == 1 and c["reported"] == [(52, 150), (35, 66)], (c["n"], c["reported"])
    c = d.call(R, 60, kmer_filter=False)
    f_of = {t: f for t, f, _ in c["ends"]}
    assert f_of[150] == 51 and f_of[68] == 49 and f_of[67] == 49 and f_of[66] == 34 and 68 - 50 < K, f_of
    assert c["reported"] == [(52, 150), (35, 66)], c["reported"]
    # reseed: the SMEM [0, 150) occurs twice; its re-seeding call (min_intv 3, pivot 75) has a stored LEP and walks to the read start
    R = d.reads["reseed"]
    assert d._occ(R).size == 2 and d._occ(R[:100]).size == 3
    c = d.call(R, 75, min_intv=3)
    assert c["n"] == 1 and c["reported"] == [(0, 100)] and min(f for _, f, _ in c["ends"]) == -1, c
    # families: every end stops in the same iteration, only the longest is reported; F(46) from genuine sequence: 46 LEPs and 18
    # window ends that pass, the call that needs all 64 lanes
    for R in (d.fam_reads[0], d.fam_reads[200]):
        calls = [d.call(R, x) for x in d.chain(R)[1:]]
        c = max(calls, key=lambda q: q["n"])
        assert c["n"] in FAMILIES and len({f for _, f, _ in c["ends"]}) == 1 and len(c["reported"]) == 1, (c["n"], c["reported"])
    wide = 0
    for R in d.pass_reads:
        wide += any(q["n"] == 46 and sum(not lep for _, _, lep in q["ends"]) == WIN for q in (d.call(R, x) for x in d.chain(R)[1:]))
    assert wide >= 9, wide                                             # of 10
    # ... and the narrow calls beside it: one stored LEP, 19 lanes
    narrow = 0
    for R in d.dup_reads[:20]:
        narrow += any(d.call(R, x)["n"] == 1 for x in d.chain(R)[1:])
    assert narrow >= 18, narrow
    assert [len(d.sets[k]) for k in ("one", "three", "sixty_five")] == [1, 3, 65] and len(d.sets["all"]) == 2000


@pytest.mark.parametrize("name", ["one", "three", "sixty_five", "all"])
def test_default_path_equals_oracle_sst0_and_no_window(gpu, name):
    ca, e = gpu
    d = data()
    bases, off = d.batch(name)
    got = e.seed_batch(bases, off, ca.Params())
    _same(got, d.want(name), (name, "oracle"))
    _same_runs(got, e.seed_batch(bases, off, ca.Params(sst_mode=0)), (name, "sst_mode=0"))
    _same_runs(got, e.seed_batch(bases, off, ca.Params(disable=ca.binding.disable_mask("window"))), (name, "disable=window"))
    assert got.n_mems > 0


def test_without_the_kmer_filter(gpu):
    """every window end without an ambiguous base goes to the jump table: ends that stop short of min_seed_len are consulted"""
    ca, e = gpu
    d = data()
    for name in ("three", "all"):
        bases, off = d.batch(name)
        _same(e.seed_batch(bases, off, ca.Params(disable=ca.binding.disable_mask("kmer_filter"))), d.want(name), (name, "disable=kmer_filter"))
