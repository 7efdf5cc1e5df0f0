"""bwd_win_kernel hands a wave's lanes out as sets (smem_bwd.hpp, lane_sets.hpp): a call with n stored LEPs takes 18 + n lanes, any
free ones.  A small genome built here holds what the dispenser can get wrong, and every case compares, on ALL its reads and with exact
equality of mem_off, mems, seed_off and seeds, the default path with the oracle, with the sst_mode = 0 pass and with
disable = window (the literal sweep, which never enters this kernel).

The genome (about 52 kbp, numpy's PCG64): random background with
  * families F(N), N in FAMILIES: N + 1 copies of a 40-base core followed by a common extension; copy j leaves the extension after
    3 j bases and two copies hold all of it.  A read "junk + core + extension" whose junk does not continue into any copy gets, at the
    pivot behind the junk, a forward pass whose interval size falls N + 1, N, ..., 2: N - 1 stored LEPs and the last one, n = N.
    The size never reaches 1, so the call never leaves the index for the text and always goes to the backward kernel;
  * 2-copy segments: exact duplications of 400 bases.  A read from one with a substitution gets a call with n = 1 a few bases
    behind the substitution (18 + 1 = 19 lanes: three such calls fit a wave), whose window ends mostly cover the substituted base.

How the input was checked on the CPU: census() below restates fwd_kernel's forward pass of a round-1 call (smem_fwd.hpp: the LEPs it
stores under the window scheme and the next pivot) by counting occurrences in the text of both strands, and follows every read's chain
of pivots.  test_input_holds_the_classes asserts from it, without a GPU call, that the batch holds calls with n of 1, 13, 14, 15
(the boundary between the former 32- and 64-lane classes), 45 and 46 (the call that needs all 64 lanes), a read set whose window ends
mostly fail the k-mer filter and one where all pass.  It was run on a CPU-only machine when the test was written.  Three or more calls
in one wave cannot be observed from outside the kernel; the `dup` reads are there for it: in the third launch nearly every one of them
has a call of 19 lanes (asserted), a wave draws 64 consecutive slots of that launch's queue, and the first placement of a wave with 64
free lanes takes as many calls from the head of its draw as fit -- three of 19.
"""
import numpy as np
import pytest

import _oracle

pytestmark = pytest.mark.gpu

ASCII = np.frombuffer(b"ACGTN", dtype=np.uint8)
K = 19                       # min_seed_len (the default)
JUMP_K = 10                  # 4^10 entries, 16 MB
CORE, STEP = 40, 3
FAMILIES = (1, 2, 3, 13, 14, 15, 45, 46)
N_DUP, DUP_LEN = 12, 400
LEAD = 3                     # the base in front of every copy (T); a read's junk ends in another one


class Data:
    """the genome, the reads by set and the oracle's results, made once"""

    def __init__(self):
        rng = np.random.default_rng(20261)
        parts = [rng.integers(0, 4, 3000)]
        self.fam = {}
        for N in FAMILIES:
            core, ext = rng.integers(0, 4, CORE), rng.integers(0, 4, STEP * (N - 1) + 1)
            full = np.concatenate([core, ext[:STEP * (N - 1)]])
            copies = [np.concatenate([core, ext[:STEP * j], [(ext[STEP * j] + 1 + rng.integers(0, 3)) & 3]]) for j in range(N - 1)] + [full, full]
            self.fam[N] = dict(full=full, lead=[])
            for c in rng.permutation(len(copies)):
                lead = rng.integers(0, 4, 60)
                lead[-1] = LEAD
                if copies[c] is copies[0] and N > 1:
                    self.fam[N]["lead"] = lead[-30:]                   # genuine sequence in front of the shortest copy
                parts += [lead, copies[c], rng.integers(0, 4, 30)]
        self.dups = []
        for _ in range(N_DUP):
            seg = rng.integers(0, 4, DUP_LEN)
            self.dups.append(seg)
            parts += [seg, rng.integers(0, 4, 500), seg, rng.integers(0, 4, 300)]
        parts.append(rng.integers(0, 4, 3000))
        self.fwd = np.concatenate(parts).astype(np.uint8)
        self.T = np.concatenate([self.fwd, 3 - self.fwd[::-1]]).astype(np.uint8)
        self.o = _oracle.OracleIndex.build(self.fwd)
        # the read sets
        fam_reads, pass_reads, dup_reads = [], [], []
        for N in FAMILIES:
            full = self.fam[N]["full"]
            for _ in range(250):
                junk = rng.integers(0, 4, int(rng.integers(8, 13)))
                junk[-1] = (LEAD + 1 + rng.integers(0, 3)) & 3
                fam_reads.append((N, np.concatenate([junk, full])))
            if N >= 13:                                                # the read runs from genuine sequence into the family: the second
                for cut in range(20):                                  # call's pivot lies inside `full`, and so do all its windows
                    pass_reads.append((N, np.concatenate([self.fam[N]["lead"][cut % 10:], full])))
        for q in range(1200):
            seg = self.dups[q % N_DUP]
            s = int(rng.integers(0, DUP_LEN - 150))
            rd = seg[s:s + 150].copy()
            p = int(rng.integers(30, 60))
            rd[p] = (rd[p] + 1 + rng.integers(0, 3)) & 3
            dup_reads.append((0, rd))
        mixed = fam_reads + dup_reads
        order = rng.permutation(len(mixed))
        self.sets = {"families": [mixed[k] for k in order], "filter_fails": dup_reads[:400], "filter_passes": pass_reads}
        self.sets["one"] = [r for r in fam_reads if r[0] == 46][:1]
        self.sets["three"] = [fam_reads[0], [r for r in fam_reads if r[0] == 15][0], dup_reads[0]]
        self.sets["sixty_five"] = self.sets["families"][:65]
        self._batch, self._want = {}, {}

    def batch(self, name):
        if name not in self._batch:
            reads = [r for _, r in self.sets[name]]
            off = np.zeros(len(reads) + 1, dtype=np.uint64)
            np.cumsum([r.size for r in reads], out=off[1:])
            self._batch[name] = (ASCII[np.concatenate(reads)], off)
        return self._batch[name]

    def want(self, name):
        if name not in self._want:
            bases, off = self.batch(name)
            self._want[name] = self.o.seed_batch(bases, off, _oracle.make_params(), mode=0, want_sal=True, threads=4)
        return self._want[name]

    # ---- fwd_kernel's forward pass of a round-1 call at pivot x, by counting in the text: (n stored under the window scheme, next pivot)
    def forward_call(self, read, x):
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

    def occurs(self, s):
        pos = np.flatnonzero(self.T[:self.T.size - s.size + 1] == s[0])
        for k in range(1, s.size):
            pos = pos[self.T[pos + k] == s[k]]
        return pos.size > 0

    def census(self, read):
        """the read's round-1 calls in launch order: (pivot, n, window ends that could pass, window ends whose K-mer occurs)"""
        x, calls = 0, []
        while x < read.size:
            n, ret = self.forward_call(read, x)
            ends = [te for te in range(x + 1, x + K) if te <= ret and te - K >= 0]
            calls.append((x, n, len(ends), sum(self.occurs(read[te - K:te]) for te in ends) if n else 0))
            x = ret
        return calls


_DATA = []


def data():
    if not _DATA:
        _DATA.append(Data())
    return _DATA[0]


@pytest.fixture(scope="module")
def gpu():
    import compseed_amd as ca
    d = data()
    ix = ca.Index.build(d.fwd, 0)
    e = ca.Engine(ix, 0, jump_k=JUMP_K)
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
    """no GPU call: what the batches stand for, from the census (a strided sample of the big sets: the reads of a family differ in their junk only)"""
    d = data()
    seen = set()
    for N, read in d.sets["families"][::20]:
        ns = [n for _, n, _, _ in d.census(read)]
        seen.update(ns)
        if N:
            assert N in ns, (N, ns)                                    # the family's call has exactly N stored LEPs
    assert {1, 13, 14, 15, 45, 46} <= seen, sorted(seen)
    assert max(seen) <= 46                                             # nothing here belongs to bwd_wide_kernel
    # the dup reads: the third launch's call takes 19 lanes, and its window ends mostly fail the filter
    third, cand, occ = 0, 0, 0
    for _, read in d.sets["filter_fails"][::20]:
        calls = d.census(read)
        third += len(calls) >= 3 and calls[2][1] == 1
        cand += sum(c[2] for c in calls if c[1]); occ += sum(c[3] for c in calls if c[1])
    assert third >= 18, third                                          # of 20
    assert cand > 0 and occ < 0.5 * cand, (occ, cand)
    # ... and the reads that run from genuine sequence into a family: a call with stored LEPs whose 18 window ends all pass
    full_windows = 0
    sample = d.sets["filter_passes"][::4]
    for _, read in sample:
        full_windows += any(n and c == K - 1 and o == c for _, n, c, o in d.census(read)[1:])
    assert full_windows >= 0.9 * len(sample), (full_windows, len(sample))


@pytest.mark.parametrize("name", ["families", "one", "three", "sixty_five", "filter_fails", "filter_passes"])
def test_default_path_equals_oracle_sst0_and_no_window(gpu, name):
    ca, e = gpu
    d = data()
    bases, off = d.batch(name)
    got = e.seed_batch(bases, off, ca.Params())
    _same(got, d.want(name), (name, "oracle"))
    _same_runs(got, e.seed_batch(bases, off, ca.Params(sst_mode=0)), (name, "sst_mode=0"))
    _same_runs(got, e.seed_batch(bases, off, ca.Params(disable=ca.binding.disable_mask("window"))), (name, "disable=window"))
    assert got.n_mems > 0
