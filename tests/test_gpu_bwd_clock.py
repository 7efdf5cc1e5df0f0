"""The backward kernels extend through extend1b (fm_device.hpp, occ_math.hpp) and bwd_win_kernel keeps its loop's bookkeeping in lane masks
and its per-lane state narrow (smem_bwd.hpp: a stopped lane's position doubles as its f, rank 0 is a bit of the kind, the pivot and the
forward end share a word).  A genome of about 30 kbp built here holds what such changes, and any change to when a call's clock starts,
can get wrong; with jump_k 10 and 15 (min_seed_len 19) every case compares, on ALL its reads and with exact equality of mem_off, mems,
seed_off and seeds, the default path with the oracle, with the sst_mode = 0 pass and with disable = window.

The genome (numpy's PCG64): random background with
  * families F(N), N in FAMILIES, as in test_gpu_bwd_lane_sets.py: N + 1 copies of a 40-base core followed by a common extension, copy j
    leaves the extension after 2 j bases and two copies hold all of it, so a read "junk + core + extension" gets a call with n = N stored
    LEPs at the pivot behind the junk.  One full copy of F(46) IS THE START OF THE GENOME: the text's first suffix, whose row is
    `primary`, then lies inside the suffix-array interval of every prefix of that copy, and the LEP lanes of such a read, which hold
    exactly those prefixes when the pivot falls on the copy's start, extend an interval that contains `primary` in their first step
    (the `head` reads: a dozen genuine bases from elsewhere in front of the copy, so that the pass from the read start ends there);
  * 2-copy segments of 400 bases (reads with a substitution: calls with n = 1, and with n = 0 behind a substitution near the read's end);
  * junctions "L1 U | b Z": U (18 bases) occurs twice, once behind L1 and once in front of b; "b Z" lies in a 2-copy segment.  A read
    L1 U b Z gets its pivot on b, and the ONLY window end whose 19-mer occurs is the first one (U b); with junk instead of Z the call has
    no stored LEP and that 19-mer, which exists, dies one base further left.

The classes the batch must hold are asserted by test_input_holds_the_classes from a census of the text made on the CPU -- no GPU call; it
was run on a CPU-only machine when the test was written.  census() restates fwd_kernel's forward pass of a round-1 call by counting
occurrences in the text of both strands (an ambiguous base matches nothing and moves the pivot behind it), as test_gpu_bwd_lane_sets.py
does, and names a window end VALID when it lies inside the read and the forward match, its 19-mer holds no ambiguous base and occurs in
the text: the criterion of the k-mer filter the default path runs with (without the filter more ends pass the jump table and die before
they reach 19 bases).  The classes:
  * calls with no valid window end, with n = 1 and with n = 46 (the lanes of the stored LEPs are the only ones that step);
  * calls whose highest valid window end is rank 17, and calls whose only valid window end is rank 0;
  * calls with no stored LEP and a valid window end (its 19-mer exists and dies within the next bases): bwd_win0_kernel's walk;
  * pivots within 18 bases of the read start where the clock reaches -1.  A round-1 pivot cannot do that (the pass that ended on it
    proves that no match from the read start crosses it), a re-seeding pivot can: reads that start with 34 bases of a family's extension
    (5 copies; the first 19 of them 13 copies) get the SMEM [0, 34), which is re-seeded at pivot 17 with min_intv 6, and the window end
    19 walks to the read start;
  * pivots within 18 bases of the read end (window ends beyond the forward match, te > ret);
  * an ambiguous base inside the window, and one right in front of the pivot;
  * walks whose interval straddles `primary` and a record boundary in the same step (from the oracle's index: asserted for a stored LEP
    of a read whose pivot falls on the start of the genome's first copy).
"""
import numpy as np
import pytest

import _oracle

ASCII = np.frombuffer(b"ACGTN", dtype=np.uint8)
K = 19                       # min_seed_len (the default)
CORE, STEP = 40, 2
FAMILIES = (1, 13, 46)
HEAD = 46                    # the family whose full copy starts the genome
N_DUP, DUP_LEN = 8, 400
N_JUNC = 8
LEAD = 3                     # the base in front of every copy (T); a read's junk ends in another one
RESEED_A, RESEED_LEN = 89, 34


def _other(rng, b):
    return (int(b) + 1 + int(rng.integers(0, 3))) & 3


class Data:
    """the genome, the reads by set and the oracle's results, made once"""

    def __init__(self):
        rng = np.random.default_rng(20262)
        self.fam = {}
        parts = []
        for N in FAMILIES:
            core, ext = rng.integers(0, 4, CORE), rng.integers(0, 4, STEP * (N - 1) + 1)
            full = np.concatenate([core, ext[:STEP * (N - 1)]])
            copies = [np.concatenate([core, ext[:STEP * j], [_other(rng, ext[STEP * j])]]) for j in range(N - 1)] + [full, full]
            self.fam[N] = dict(full=full, lead=[])
            order = list(rng.permutation(len(copies)))
            if N == HEAD:                                                   # a full copy first, with nothing in front of it
                order.remove(len(copies) - 1)
                parts = [copies[-1], rng.integers(0, 4, 30)] + parts
            for c in order:
                lead = rng.integers(0, 4, 60)
                lead[-1] = LEAD
                if c == 0 and N > 1:
                    self.fam[N]["lead"] = lead[-30:]                        # genuine sequence in front of the shortest copy
                parts += [lead, copies[c], rng.integers(0, 4, 30)]
        self.dups = []
        for _ in range(N_DUP):
            seg = rng.integers(0, 4, DUP_LEN)
            self.dups.append(seg)
            parts += [seg, rng.integers(0, 4, 500), seg, rng.integers(0, 4, 300)]
        self.junc = []
        for q in range(N_JUNC):
            D, j = self.dups[q % N_DUP], 100 + 7 * q
            U, L1, L2 = rng.integers(0, 4, 18), rng.integers(0, 4, 30), rng.integers(0, 4, 30)
            U[-1] = _other(rng, D[j - 1]); L2[-1] = _other(rng, L1[-1])
            self.junc.append((L1, U, D, j))
            parts += [rng.integers(0, 4, 40), L1, U, [_other(rng, D[j])], rng.integers(0, 4, 40), L2, U, [D[j]], [_other(rng, D[j + 1])], rng.integers(0, 4, 40)]
        parts.append(rng.integers(0, 4, 3000))
        self.fwd = np.concatenate([np.asarray(p) for p in parts]).astype(np.uint8)
        self.T = np.concatenate([self.fwd, 3 - self.fwd[::-1]]).astype(np.uint8)
        code = np.zeros(self.T.size - K + 1, dtype=np.int64)
        for k in range(K):
            code = code << 2 | self.T[k:k + code.size]
        self.kmers = set(code.tolist())                                     # every 19-mer of the text, both strands
        self.o = _oracle.OracleIndex.build(self.fwd)
        sets = {}

        def junk(lo, hi):
            j = rng.integers(0, 4, int(rng.integers(lo, hi)))
            j[-1] = _other(rng, LEAD)
            return j

        def read150(*pieces):                                               # (a random tail where the pieces are shorter)
            return np.concatenate(list(pieces) + [rng.integers(0, 4, 150)])[:150]
        sets["families"] = [read150(junk(8, 13), self.fam[N]["full"]) for N in FAMILIES for _ in range(200)]
        head = []                                                           # genuine bases in front: the pass from 0 ends exactly on the copy's start
        while len(head) < 200:
            L, u = int(rng.integers(10, 15)), int(rng.integers(self.fwd.size - 2900, self.fwd.size - 100))
            if self.fwd[u + L - 1] != LEAD and self.fwd[u + L] != self.fam[HEAD]["full"][0]:
                head.append(read150(self.fwd[u:u + L], self.fam[HEAD]["full"]))
        sets["head"] = head
        sets["passes"] = [read150(self.fam[N]["lead"][cut % 10:], self.fam[N]["full"]) for N in FAMILIES if N >= 13 for cut in range(20)]
        dup, dup_end = [], []
        for q in range(900):
            seg = self.dups[q % N_DUP]
            s = int(rng.integers(0, DUP_LEN - 150))
            rd = seg[s:s + 150].copy()
            p = int(rng.integers(30, 60)) if q % 3 else int(rng.integers(133, 148))
            rd[p] = _other(rng, rd[p])
            (dup if q % 3 else dup_end).append(rd)
        sets["dups"], sets["dup_ends"] = dup, dup_end
        only0, only0_short = [], []
        for L1, U, D, j in self.junc:
            for cut in range(10):
                only0.append(np.concatenate([L1[-25 + cut:], U, D[j:j + 107 + cut]]))
                only0_short.append(np.concatenate([L1[-25 + cut:], U, D[j:j + 12], rng.integers(0, 4, 95 + cut)]))
        sets["only0"], sets["only0_short"] = only0, only0_short
        full = self.fam[HEAD]["full"]
        sets["reseed"] = [np.concatenate([full[RESEED_A:RESEED_A + RESEED_LEN], [_other(rng, full[RESEED_A + RESEED_LEN])], rng.integers(0, 4, 150 - RESEED_LEN - 1)])
                          for _ in range(40)]
        amb_front, amb_inside = [], []
        for N in (1, 46):
            for _ in range(40):
                amb_front.append(read150(junk(8, 13), [4], self.fam[N]["full"]))
                amb_inside.append(read150(junk(3, 5), [4], junk(8, 11), self.fam[N]["full"]))
        sets["amb_front"], sets["amb_inside"] = amb_front, amb_inside
        for name, reads in sets.items():
            assert all(r.size == 150 for r in reads), name
        mixed = [r for name in sorted(sets) for r in sets[name]]
        sets["all"] = [mixed[k] for k in rng.permutation(len(mixed))]
        sets["one"] = sets["head"][:1]
        self.sets = sets
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

    def count(self, s):
        """occurrences of s in the text of both strands (an ambiguous base matches nothing)"""
        if s.size == 0 or (s > 3).any():
            return 0 if s.size else self.T.size
        pos = np.flatnonzero(self.T[:self.T.size - s.size + 1] == s[0])
        for k in range(1, s.size):
            pos = pos[self.T[pos + k] == s[k]]
        return pos.size

    def has_kmer(self, s):
        c = 0
        for b in s:
            if b > 3:
                return False
            c = c << 2 | int(b)
        return c in self.kmers

    # ---- fwd_kernel's forward pass of a round-1 call at pivot x, by counting in the text: (n stored under the window scheme, next pivot)
    def forward_call(self, read, x):
        if read[x] > 3:
            return 0, x + 1
        T = self.T
        pos = np.flatnonzero(T == read[x])
        i, n = x + 1, 0
        while i < read.size:
            nxt = pos[pos + (i - x) < T.size]
            nxt = nxt[T[nxt + (i - x)] == read[i]]
            if nxt.size != pos.size:
                if nxt.size == 0:
                    break                                              # fin: the size changed and fell below min_intv = 1
                if x != 0 and i - x >= K:
                    n += 1
            pos = nxt
            i += 1
        if x != 0 and i - x >= K:
            n += 1
        return n, i

    def census(self, read):
        """the read's round-1 calls in launch order: (pivot, n, forward end, ranks of the valid window ends)"""
        x, calls = 0, []
        while x < read.size:
            n, ret = self.forward_call(read, x)
            if read[x] <= 3 and x != 0:
                valid = [g for g in range(K - 1) if x + 1 + g <= ret and x + 1 + g - K >= 0 and self.has_kmer(read[x + 1 + g - K:x + 1 + g])]
                calls.append((x, n, ret, valid))
            x = ret
        return calls

    def interval(self, s):
        """(x0, x2) of string s from the oracle's index, by backward search"""
        L2 = [int(v) for v in self.o.idx.L2]
        c = int(s[-1])
        x0, x1, x2 = L2[c] + 1, L2[3 - c] + 1, L2[c + 1] - L2[c]
        for b in s[-2::-1]:
            x0, x1, x2 = self.o.extend(x0, x1, x2, True)[int(b)]
        return x0, x2


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
    """no GPU call: what the batch stands for, from the census (a strided sample of the big sets: the reads of a set differ in their junk only)"""
    d = data()
    assert 2000 <= len(d.sets["all"]) <= 5000 and 20000 <= d.fwd.size <= 99000
    # no valid window end, n = 1 and n = 46
    bare = set()
    for read in d.sets["families"][::8]:
        bare.update(n for _, n, _, valid in d.census(read) if n and not valid)
    assert {1, 46} <= bare, sorted(bare)
    # the highest valid window end is rank 17 / the only valid one is rank 0 / no stored LEP and a valid end
    top17 = sum(any(n and valid and valid[-1] == K - 2 for _, n, _, valid in d.census(r)) for r in d.sets["passes"][::4])
    assert top17 >= 8, top17                                           # of 10
    only0 = sum(any(n and valid == [0] for _, n, _, valid in d.census(r)) for r in d.sets["only0"][::5])
    assert only0 >= 14, only0                                          # of 16
    short = sum(any(n == 0 and valid == [0] for _, n, _, valid in d.census(r)) for r in d.sets["only0_short"][::5])
    assert short >= 14, short
    # a pivot within 18 bases of the read end: window ends beyond the forward match
    late = sum(any(x + K - 1 > ret for x, _, ret, _ in d.census(r)) for r in d.sets["dup_ends"][::10])
    assert late >= 18, late                                            # of 20
    # the re-seeded SMEM [0, 34): at most split_width = 10 occurrences and at least int(1.5 * 19 + .499) = 28 bases, so it is re-seeded at
    # pivot 17 with min_intv = occurrences + 1, and the window end 19 (rank 1) has that many: it walks to the read start, the clock to -1
    for r in d.sets["reseed"][::8]:
        n0, ret0 = d.forward_call(r, 0)
        occ = d.count(r[:RESEED_LEN])
        assert ret0 == RESEED_LEN and 2 <= occ <= 10 and RESEED_LEN >= 28 and (0 + RESEED_LEN) // 2 == 17, (ret0, occ)
        assert d.count(r[:K]) >= occ + 1 and K - 17 - 1 == 1, d.count(r[:K])
    # an ambiguous base right in front of the pivot (every window end holds it) and inside the window, n = 1 and n = 46
    front, inside = set(), set()
    for r in d.sets["amb_front"][::4]:
        front.update(n for x, n, _, valid in d.census(r) if n and r[x - 1] > 3 and not valid)
    for r in d.sets["amb_inside"][::4]:
        inside.update(n for x, n, _, _ in d.census(r) if n and x >= 3 and (r[max(0, x - K + 1):x - 1] > 3).any())
    assert {1, 46} <= front and {1, 46} <= inside, (sorted(front), sorted(inside))
    # `primary` lies inside the head family: the genome starts with its full copy ...
    full = d.fam[HEAD]["full"]
    assert np.array_equal(d.fwd[:full.size], full)
    primary = int(d.o.idx.primary)
    x0, x2 = d.interval(full[:CORE])
    assert x2 == HEAD + 1 and x0 - 1 < primary <= x0 - 1 + x2, (x0, x2, primary)
    # ... and a read whose pivot falls on the copy's start holds, as a stored LEP, a prefix whose interval straddles primary AND whose two
    # rows lie in different 64-row records: the step that prepends the junk's last base reads two records and adds the primary flag
    both = 0
    for r in d.sets["head"][::10]:
        for x, n, ret, _ in d.census(r):
            if n == HEAD and np.array_equal(r[x:x + CORE], full[:CORE]):
                sizes = [d.count(r[x:t]) for t in range(x + K, ret + 1)]
                for q, t in enumerate(range(x + K, ret + 1)):
                    if t == ret or sizes[q + 1] != sizes[q]:               # a stored LEP: the size changes behind it, or the match ends
                        a, w = d.interval(r[x:t])
                        k, l = a - 1, a - 1 + w
                        if k < primary <= l and ((k - (k >= primary)) >> 6) != ((l - (l >= primary)) >> 6):
                            both += 1
    assert both >= 1, both


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["all", "one"])
def test_default_path_equals_oracle_sst0_and_no_window(gpu, name):
    ca, e = gpu
    d = data()
    bases, off = d.batch(name)
    got = e.seed_batch(bases, off, ca.Params())
    _same(got, d.want(name), (name, "oracle"))
    _same_runs(got, e.seed_batch(bases, off, ca.Params(sst_mode=0)), (name, "sst_mode=0"))
    _same_runs(got, e.seed_batch(bases, off, ca.Params(disable=ca.binding.disable_mask("window"))), (name, "disable=window"))
    assert got.n_mems > 0
