// smem_text.hpp -- the text side of the split SMEM path: the fill of the k-mer filter, re-seeding calls answered from rep[] / lcp[]
// (r2text_kernel) and round 3 from the text (r3text_kernel).  Overview: smem_common.hpp.
#pragma once
#include "smem_common.hpp"

namespace csd {

// fills the k-mer filter (smem_common.hpp, kmer_filter_has) from the text
__global__ void kmer_filter_fill_kernel(const DevIndex ix, int k, uint64_t *bloom, uint32_t bits)
{
	const uint64_t n = ix.seq_len >= (uint64_t)k ? ix.seq_len - (uint64_t)k + 1 : 0;
	const uint64_t mask = k >= 32 ? ~0ull : ((1ull << (2 * k)) - 1ull);
	for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t h = kmer_hash(text_win(ix, p) & mask);
		atomicOr((unsigned long long *)&bloom[h >> (64u - bits)], (1ull << (h & 63u)) | (1ull << ((h >> 6) & 63u)));
	}
}

// Re-seeding from the text.
//
// A round-1 SMEM [beg, end) with a single occurrence triggers bwt_smem1a(pivot = (beg+end)/2, min_intv = 2)
// (bwamem.c:241-249): all maximal substrings through the pivot that occur at least twice.  On the FM index that is a
// forward pass plus a triangular backward sweep, ~150 extensions, and for most reads it finds nothing of min_seed_len.
// But inside [beg, end) the read IS the text at the SMEM's position P = SA[x0], and "occurs at least twice" is a property
// of the text alone: the substring of length l at text position p is repeated iff l <= rep[p] (fm_device.hpp).  So with
// e(q) = q + rep[q] the sweep of bwt.c:303-345 reads off directly:
//   * forward pass from the pivot p: longest match with >= 2 occurrences ends at e(p);
//   * backward step to start q: the longest surviving end is e(q) (never larger than e(q+1));
//   * [q, e(q)) is reported when it does not survive the next step, e(q-1) < e(q), i.e. rep[q-1] <= rep[q];
//   * the sweep is over when e(q) <= p.
// The bi-interval of a reported substring comes from the inverse suffix array and a short walk over lcp[] to the ends of
// its suffix-array interval (forward strand and reverse-complement strand).
// This only holds while the substrings stay inside [beg, end), where read and text agree: if a candidate reaches either
// end of the SMEM, a capped value (255) turns up, or an interval walk gets long, nothing is emitted and the call stays
// in the queue for fwd_kernel / bwd_all_kernel.  So the result is the reference's either way; only the cost differs.
// per-lane event counts of the text-side kernels, handed to the kernel's WaveCtr at the end
struct LaneCtr { uint32_t sa, isa, rep, lcp, mem; };
__device__ __forceinline__ void lc_flush(LaneCtr c, WaveCtr &W)
{
	W.addn(EV_SA, c.sa); W.addn(EV_ISA, c.isa); W.addn(EV_REP, c.rep); W.addn(EV_LCP, c.lcp); W.addn(EV_MEM, c.mem);
}
struct RepReader { // rep[] / lcp[] bytes around a moving position, one aligned 8-byte load per 8 positions (the arrays are padded)
	const uint8_t *base; uint64_t wk, w; uint32_t loads;
	__device__ __forceinline__ uint32_t at(uint64_t pos)
	{
		uint64_t k = pos >> 3;
		if (k != wk) { wk = k; w = *reinterpret_cast<const uint64_t *>(base + (k << 3)); ++loads; }
		return (uint32_t)(w >> ((pos & 7) << 3)) & 0xffu;
	}
};
struct LcpReader : RepReader { static constexpr uint32_t BYTES = 8; };
// bi-interval of the repeated substring of length v at text position pos (v <= 254, so the capped lcp[] decides exactly)
__device__ __forceinline__ bool text_interval(const DevIndex &ix, uint64_t pos, uint32_t v, Intv &out, LaneCtr &C, int MAX_WALK = 48)
{
	if (v == 0 || pos + v > ix.seq_len) return false; // (cannot happen for a substring of a mem; a walk must never leave the arrays)
	uint64_t lo = isa_direct(ix, pos), hi = lo, lo2 = isa_direct(ix, ix.seq_len - (pos + v));
	int steps = 0;
	C.isa += 2;
	LcpReader Lr = {ix.lcp, ~0ull, 0, 0}; // a walk is a chain of dependent loads: eight rows per load instead of one
	struct Tally { LcpReader &R; LaneCtr &C; __device__ ~Tally() { C.lcp += LcpReader::BYTES * R.loads; } } tally = {Lr, C};
	while (lo > 0 && Lr.at(lo) >= v) { --lo; if (++steps > MAX_WALK) return false; }
	while (hi < ix.seq_len && Lr.at(hi + 1) >= v) { ++hi; if (++steps > MAX_WALK) return false; }
	while (lo2 > 0 && Lr.at(lo2) >= v) { --lo2; if (++steps > 2 * MAX_WALK) return false; }
	out.x0 = lo; out.x1 = lo2; out.x2 = hi - lo + 1;
	return true;
}
// (r2_quick_rep, smem_common.hpp, is the test on rep[] itself: fwd0_kernel asks it too.)  0: answered; 1: needs the sweep; 2: the text cannot tell.
// a: the call's side word (emit_smem).  With AUX_POS its low bits ARE the SMEM's text position and the chain task -> aux -> rep[] has no
// suffix-array read in it; otherwise they are x0 and P = SA[x0] as before.
__device__ __forceinline__ int r2_quick(const SplitArgs &A, uint64_t a, int beg, int end, int pivot, uint64_t &P, LaneCtr &C)
{
	const DevIndex &ix = A.ix;
	const int len = end - beg, po = pivot - beg, k = A.min_seed_len;
	if (k < 2 || po > 4096) return 2;
	if (a & AUX_POS) P = a & AUX_LOW;
	else { P = sa_direct(ix, a & AUX_LOW); ++C.sa; }
	if (P >= ix.seq_len || P + (uint64_t)len > ix.seq_len) return 2; // (an SMEM lies inside the text)
	uint32_t nw = 0;
	const int q = r2_quick_rep(ix, P, len, po, k, nw);
	C.rep += nw;
	return q;
}
__device__ __forceinline__ bool r2_by_text(const SplitArgs &A, uint32_t r, uint64_t P, int beg, int end, int pivot, LaneCtr &C)
{
	const DevIndex &ix = A.ix;
	const int len = end - beg, po = pivot - beg, k = A.min_seed_len;
	// Where the SMEM touches an end of the READ the sweep cannot run past it either (bwt.c:303 stops the forward pass at
	// the last base, bwt.c:326 the backward sweep in front of the first), so there the text still tells everything: ends
	// are clipped to the read end, and a match that is still alive at the first base is reported there.
	const bool at_start = beg == 0, at_end = (uint64_t)end == A.off[r + 1] - A.off[r];
	// rep[] of the SMEM's bases, eight per aligned load; the window covers the offsets [wo, wo + 8) of the SMEM (32-bit arithmetic:
	// the walk is this kernel's inner loop, and a wave runs as long as its longest walk)
	const uint8_t *rp = ix.rep + P;
	int wo = po - (int)((P + (uint64_t)po) & 7ull);
	uint64_t w = *reinterpret_cast<const uint64_t *>(rp + wo);
	uint32_t loads = 1;
	struct Tally { uint32_t &n; LaneCtr &C; __device__ ~Tally() { C.rep += n; } } tally = {loads, C};
	constexpr int MAXC = 8;               // reported substrings per call; more (tandem arrays): leave it to the index
	int co[MAXC], cv[MAXC], ne = 0;
	auto eff = [&](int o, int &v) -> bool { // repeat length at offset o (inside the window) as far as it matters; false: the text cannot tell
		v = (int)((uint32_t)(w >> ((uint32_t)(o - wo) << 3)) & 0xffu);
		if (v == 0) return false;
		if (o + v >= len) { if (!at_end) return false; v = len - o; return true; } // (a capped 255 that reaches the end is as good as the true value)
		return v != 255;
	};
	int o = po, v = 0;
	if (!eff(o, v)) return false;
	for (;;) {
		if (o + v <= po) break;                               // no longer through the pivot: the sweep is over
		if (o == 0) {                                         // alive at the SMEM's first base
			if (!at_start) return false;                      // ... which is not the read's: the match may extend beyond it
			if (v >= k) { if (ne == MAXC) return false; co[ne] = 0; cv[ne] = v; ++ne; }
			break;
		}
		if (o == wo) { wo -= 8; w = *reinterpret_cast<const uint64_t *>(rp + wo); ++loads; } // (P + wo >= 0: an aligned address below P + o)
		int vp = 0;
		if (!eff(o - 1, vp)) return false;
		if (vp <= v && v >= k) { if (ne == MAXC) return false; co[ne] = o; cv[ne] = v; ++ne; }
		--o; v = vp;
	}
	Intv ci[MAXC];
	for (int j = 0; j < ne; ++j) if (!text_interval(ix, P + (uint64_t)co[j], (uint32_t)cv[j], ci[j], C, 192)) return false;
	for (int j = 0; j < ne; ++j) emit_mem(A, r, ci[j], (uint32_t)(beg + co[j]), (uint32_t)(beg + co[j] + cv[j]));
	return true;
}
// One lane per slot of the next forward queue.  Calls that are answered drop out; everything else is copied, without the
// no-op padding, to `fq_out` (the queue the finished iteration has consumed), so the next launches see a dense queue.
#ifndef CS_R2_WAVES
#define CS_R2_WAVES 6
#endif
__global__ __launch_bounds__(256, CS_R2_WAVES) void r2text_kernel(const SplitArgs A, const uint64_t *fq, const uint64_t *aux, const unsigned long long *n_ptr,
                                                     unsigned long long *n_done, unsigned long long *n_left, uint64_t *fq_out, unsigned long long *n_out)
{
	uint64_t n = *n_ptr; if (n > A.fq_cap) n = A.fq_cap;
	const uint32_t lane = threadIdx.x & 63u;
	unsigned long long done = 0, left = 0;
	LaneCtr C = {0, 0, 0, 0, 0};
	// a wave takes 256 consecutive slots at a time (one atomic on the output counter per 256 slots).  The quick test settles
	// most candidates; the others are gathered (LDS) and swept together on full waves afterwards -- the sweep is a loop of up
	// to a few dozen steps, and a wave runs as long as its longest.
	__shared__ uint64_t slow_P[256 / 64][256];
	__shared__ uint8_t slow_src[256 / 64][256], slow_ok[256 / 64][256];
	const uint32_t wv = threadIdx.x >> 6;
	const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
	for (uint64_t t0 = wave * 256; t0 < n; t0 += n_waves * 256) { // wave-uniform
		uint64_t task[4]; uint64_t km[4]; uint32_t total = 0, nslow = 0, slowm = 0;
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const uint64_t t = t0 + (uint64_t)(64 * j) + lane;
			task[j] = t < n ? fq[t] : FTASK_NONE;
			bool slow = false; uint64_t P = 0;
			if ((uint32_t)(task[j] >> 62) == TK_ROUND2 && ((task[j] >> 48) & 0x3fffu) == 2u) {
				const uint64_t a = aux[t];
				const int pivot = (int)((task[j] >> 32) & 0xffffu);
				const int beg = (int)((a >> 37) & 0xffffu), end = 2 * pivot + (int)((a >> 53) & 1u) - beg;
				const int q = r2_quick(A, a, beg, end, pivot, P, C);
				if (q == 0) { task[j] = FTASK_NONE; ++done; } else if (q == 1) slow = true; else ++left;
			}
			const uint64_t sm = __ballot(slow);
			if (slow) { const uint32_t i = nslow + (uint32_t)__popcll(sm & ((1ull << lane) - 1ull)); slow_P[wv][i] = P; slow_src[wv][i] = (uint8_t)(64 * j + (int)lane); slowm |= 1u << j; }
			nslow += (uint32_t)__popcll(sm);
		}
		__builtin_amdgcn_wave_barrier();
		for (uint32_t c = 0; c < nslow; c += 64) { // wave-uniform
			const uint32_t i = c + lane;
			if (i < nslow) {
				const uint32_t src = slow_src[wv][i];
				const uint64_t t = t0 + src, tk = fq[t], a = aux[t];
				const int pivot = (int)((tk >> 32) & 0xffffu);
				const int beg = (int)((a >> 37) & 0xffffu), end = 2 * pivot + (int)((a >> 53) & 1u) - beg;
				slow_ok[wv][src] = r2_by_text(A, (uint32_t)tk, slow_P[wv][i], beg, end, pivot, C) ? 1 : 0;
			}
		}
		__builtin_amdgcn_wave_barrier();
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			if (slowm & (1u << j)) { if (slow_ok[wv][64 * j + (int)lane]) { task[j] = FTASK_NONE; ++done; } else ++left; }
			km[j] = __ballot(task[j] != FTASK_NONE);
			total += (uint32_t)__popcll(km[j]);
		}
		__builtin_amdgcn_wave_barrier();
		if (total) {
			unsigned long long base = 0;
			if (lane == 0) base = atomicAdd(n_out, (unsigned long long)total);
			base = __shfl(base, 0);
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				if (task[j] != FTASK_NONE) fq_out[base + (uint64_t)__popcll(km[j] & ((1ull << lane) - 1ull))] = task[j];
				base += (uint64_t)__popcll(km[j]);
			}
		}
	}
	for (int o = 32; o > 0; o >>= 1) { done += __shfl_xor(done, o); left += __shfl_xor(left, o); }
	if (lane == 0) { if (done) atomicAdd(n_done, done); if (left) atomicAdd(n_left, left); }
	WaveCtr W; // (these two kernels have registers to spare: they always count)
	lc_flush(C, W);
	wc_flush(W, A.evc, KID_R2TEXT);
}

// ------------------------------------------------------------------------------------------------------------------
// Round 3 (bwt_seed_strategy1, bwt.c:357-381; the loop of bwamem.c:253-262) after rounds 1 and 2, one lane per read.
//
// A round-3 seed starting at x is the shortest prefix [x, x+L), L >= min_seed_len + 1, with fewer than max_mem_intv
// occurrences.  Where the read lies inside one of its own mems of rounds 1 and 2, [beg, end) -- an exact match of the text at
// P = SA[x0], whichever of its occurrences that row is -- the read IS the text, and for L = min_seed_len + 1 the answer is in the text arrays: rep[p] < L means the L-mer at p is
// unique (bi-interval = two inverse-suffix-array reads), otherwise a short walk over lcp[] counts its occurrences.  Only
// where that does not apply (the seed would leave the SMEM, 20 or more occurrences, repeats without a unique SMEM) the
// seed is computed on the FM index as before (jump table + extensions).  Same seeds, a fraction of the index reads:
// on the bench workload round 3 was the largest single consumer of HBM traffic.
// Length of the round-3 seed that starts at text position p: the smallest L >= k1 for which the L-mer at p has fewer than
// max_intv occurrences (bwt.c:370).  The suffixes that share a prefix with suffix p sit around row ISA[p]; going outwards,
// the running minimum of lcp[] on each side is the length shared with the j-th neighbour, non-increasing.  The L-mer has
// 1 + #{neighbours sharing >= L} occurrences, so L = 1 + the (max_intv - 1)-th largest shared length (or k1 if fewer than
// that many neighbours share k1 bases).  At most max_intv - 1 bytes of lcp[] on either side: two cache lines instead of the
// dozens of bwt_extend calls such a seed costs in a repeat.  False when a capped value (255) would decide.
// 0: the arrays cannot tell; 1: L; 2: max_intv - 1 neighbours share 255 bases or more (every prefix of up to 254 bases has max_intv occurrences)
// HAVE_ISA: the caller holds ISA[p] already (isa_p, from the fused entry it loaded for rep[p]); otherwise it is read here
template <bool HAVE_ISA>
__device__ __forceinline__ int r3_text_len(const DevIndex &ix, uint64_t p, uint64_t isa_p, int k1, uint32_t max_intv, int &L, LaneCtr &C)
{
	if (max_intv < 2 || max_intv > 41) return 0;
	const uint32_t m = max_intv - 1;
	if (p >= ix.seq_len) return 0;
	uint64_t up = isa_p;
	if (!HAVE_ISA) { up = isa_direct(ix, p); ++C.isa; }
	uint64_t dn = up + 1;
	LcpReader Lu = {ix.lcp, ~0ull, 0, 0}, Ld = {ix.lcp, ~0ull, 0, 0}; // one window per side: ~3 dependent loads instead of up to 19
	struct Tally { LcpReader &A, &B; LaneCtr &C; __device__ ~Tally() { C.lcp += LcpReader::BYTES * (A.loads + B.loads); } } tally = {Lu, Ld, C};
	uint32_t mu = Lu.at(up), md = Ld.at(dn), val = 0;
	for (uint32_t t = 0; t < m; ++t) {
		val = mu > md ? mu : md;
		if (val < (uint32_t)k1) { L = k1; return 1; }      // fewer than max_intv occurrences already at k1 bases
		if (mu >= md) { if (up == 0) return 0; --up; const uint32_t c = Lu.at(up); mu = c < mu ? c : mu; }
		else { if (dn > ix.seq_len) return 0; ++dn; const uint32_t c = Ld.at(dn); md = c < md ? c : md; }
	}
	if (val >= 255u) return 2;                              // the true shared length is not known
	L = (int)val + 1;
	return 1;
}

// cnt_snap: the per-read mem counts at a moment when every entry below them was complete (a copy taken between launches):
// the kernel may run beside the last, thin iterations of rounds 1/2, which keep appending to the same lists.  A read that is
// still being worked on simply finds fewer covering mems and takes more of its seeds from the index.
#ifndef CS_R3_WAVES
#define CS_R3_WAVES 5
#endif
// reads that still have calls of rounds 1/2 in the queue when r3text_kernel starts: their mem lists are not final
__global__ void mark_pending_kernel(const uint64_t *fq, const unsigned long long *n_ptr, uint64_t cap, int64_t n_reads, uint8_t *pending)
{
	uint64_t n = *n_ptr; if (n > cap) n = cap;
	for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t task = fq[t];
		if ((uint32_t)(task >> 62) != TK_NOP && (int64_t)(uint32_t)task < n_reads) pending[(uint32_t)task] = 1;
	}
}
// `pending[r] == 0` and no more than `cap` mems: every SMEM of the read is in its list.  Then the text answers everything: the mem that
// covers [x, x + k1) and reaches furthest to the right ends where the longest match from x ends (a longer one would sit in an SMEM of
// its own, which would be in the list), and if no mem covers it the k1-mer does not occur at all.
//
// What the kernel waits for is the chain of dependent round trips per read, at 5 waves/SIMD, so:
//   * FUSED (DevIndex::isa_fused): rep[p] comes with ISA[p] in one 8-byte entry, so "unique? then its rank" is one round trip, not two
//     dependent ones.  Chosen per instantiation; isa32 / isa40 indexes run the <false> one, which reads rep[] itself.
//   * the [begin, end) of the read's first R3_REG (two) mems of rounds 1/2 are loaded once per read and kept in registers (16 bits each:
//     reads are shorter than 65535 bases); the cover searches scan those and go to memory only for mems beyond them.  Measured at 0, 2, 4
//     and 6: 2 is fastest, more come back as spills.
//   * a `complete` read has no other writer of its mem list while this kernel runs, so its slots come from a lane-local counter that
//     starts at the snapshot count, and out_cnt[r] is stored once at the end; other reads take their slots with atomics as before
//     (the thin iterations beside the kernel may append to their lists).  One lane emits a read's seeds in order either way.
//     The SA slots of the seeds (SplitArgs::out_scnt) add up in a register and go out as one add per read, beside the count.
//   * LEAN (CS_RESULT_LEAN): the caller reads no x1, and the reverse-strand rank ISA[seq_len - (p + k1)] of a unique k1-mer is read
//     for nothing else, so those loads are not issued and a1 is 0 (the sort stores x1 = 0 whatever a kernel left there); C.isa counts
//     what was asked for.
template <bool FUSED, bool LEAN>
__global__ __launch_bounds__(256, CS_R3_WAVES) void r3text_kernel(const SplitArgs A, const uint32_t *cnt_snap, unsigned long long *n_text_seeds, const uint8_t *pending)
{
	const DevIndex &ix = A.ix;
	const int k1 = A.min_seed_len + 1;
	const int jk = (A.jump && A.jump_k <= A.min_seed_len) ? A.jump_k : 0;
	constexpr uint32_t R3_REG = 2; // mems of rounds 1/2 held in registers (measured at 0, 2, 4, 6: DESIGN 4.3)
	unsigned long long my_q = 0, my_hits = 0, my_text = 0;
	LaneCtr C = {0, 0, 0, 0, 0};
	WaveCtr W;
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < A.n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		const uint64_t rb = A.off[r]; const int len = (int)(A.off[r + 1] - rb);
		const uint32_t cs = cnt_snap[r], nm0 = cs < A.cap ? cs : A.cap; // the mems of rounds 1 and 2 known to be complete
		const bool complete = pending[r] == 0 && cs <= A.cap;
		const OutMem *mine = A.out + (size_t)r * A.cap;
		uint32_t mreg[R3_REG]; // begin << 16 | end of mems 0 .. R3_REG - 1 (0: none, covers nothing)
#pragma unroll
		for (uint32_t a = 0; a < R3_REG; ++a) {
			mreg[a] = 0;
			if (a < nm0) { const uint64_t info = mine[a].info; mreg[a] = (uint32_t)(info >> 32) << 16 | ((uint32_t)info & 0xffffu); }
		}
		C.mem += nm0 < R3_REG ? nm0 : R3_REG;
		// text position of mem `best`.  Its x2 word is loaded with x0, two loads in one round trip: a tagged mem (fm_device.hpp, MEM_POS_TAG)
		// brings the position, and only an untagged one costs the dependent trip mem record -> x0 -> SA
		auto pos_of = [&](int best) -> uint64_t {
			const uint64_t x0 = mine[best].x0, w = mine[best].x2;
			if (w & MEM_POS_TAG) return mem_pos(w);
			++C.sa;
			return sa_direct(ix, x0);
		};
		uint32_t next_slot = cs; // complete reads: the next free slot of the read's list
		int cb = 0, ce = 0; uint64_t cp = 0; // the mem the cursor is in: [cb, ce) at text position cp
		bool covered = false;
		int x = 0;
		PackedReader rd; rd.start(A.seqp, rb, (uint32_t)r, 0);
		// the mem that covers [x, x + k1) and reaches beyond `ce` furthest (the first of them in list order; any occurrence of it will do)
		auto cover = [&](int x, int &cb, int &ce) -> int {
			int best = -1;
#pragma unroll
			for (uint32_t a = 0; a < R3_REG; ++a) {
				const int mb = (int)(mreg[a] >> 16), me = (int)(mreg[a] & 0xffffu);
				if (x >= mb && x + k1 <= me && me > ce) { best = (int)a; cb = mb; ce = me; }
			}
			for (uint32_t a = R3_REG; a < nm0; ++a) {
				const uint64_t info = mine[a].info; const int mb = (int)(info >> 32), me = (int)(uint32_t)info;
				++C.mem;
				if (x >= mb && x + k1 <= me && me > ce) { best = (int)a; cb = mb; ce = me; }
			}
			return best;
		};
		auto take = [&](uint32_t n) -> uint32_t {
			if (complete) { const uint32_t k0 = next_slot; next_slot += n; return k0; }
			return atomicAdd(&A.out_cnt[r], n);
		};
		uint32_t my_slots = 0; // SA slots of the seeds this lane emits for the read: one add where the count is stored
		// pos: the seed's text position where it is unique and was taken from the text (it is SA[m.x0]: m.x0 is that position's rank), as for emit_mem
		auto put = [&](uint32_t kk, OutMem m, uint64_t pos = POS_NONE) {
			my_slots += sal_slots(m.x2, A.max_occ);
			if (m.x2 == 1 && pos != POS_NONE && (A.text_sweep & TS_MEM_POS)) m.x2 = MEM_POS_TAG | pos;
			if (kk < A.cap) A.out[(size_t)r * A.cap + kk] = m;
			else {
				unsigned long long sl = atomicAdd(A.ovf_cnt, 1ull);
				if (sl < A.ovf_cap) { OvfRec o = {m, (uint32_t)r, 0}; A.ovf[sl] = o; } else atomicMax(A.err, 1ull);
			}
		};
		while (x < len) {
			if (rd.at(x) > 3) { ++x; continue; }
			if (!(x >= cb && x + k1 <= ce)) { // look for a mem that covers [x, x + k1)
				cb = ce = 0;
				const int best = cover(x, cb, ce);
				covered = best >= 0;
				if (covered) {
					cp = pos_of(best);
					if (cp >= ix.seq_len || cp + (uint64_t)(ce - cb) > ix.seq_len) cb = ce = 0; // (a mem lies inside the text)
				}
			}
			if (complete && !covered) { // [x, x + k1) does not occur (or is cut short by an ambiguous base or the read's end): bwt.c:366-377
				uint32_t badw; const int nb = len - x < k1 ? len - x : k1;   // walks on to x + k1, the ambiguous base or the end, reports nothing
				(void)rd.window(x, nb, badw);
				const int fb = badw ? __ffs((int)badw) - 1 : 32;
				int nx = fb < k1 ? x + fb + 1 : x + k1;
				if (nx > len) nx = len;
				my_q += (unsigned)(nx - x - 1); my_hits += (unsigned)(nx - x - 1);
				x = nx;
				continue;
			}
			if (x >= cb && x + k1 <= ce && ix.rep) {
				const uint64_t p = cp + (uint64_t)(x - cb);
				// Inside a mem the next seeds start k1 apart as long as each k1-mer is unique, so up to four of them are resolved
				// at once, one counter update for the four mems.  Unfused: four rep[] bytes, then two inverse-SA reads for each of
				// the leading unique ones.  FUSED: the four entries bring the rep bytes and the forward ranks, and the four
				// reverse-strand ranks are asked for in the same round trip, before it is known which of them are needed -- the
				// kernel waits for dependent round trips, it is not short of requests, so a few wasted entries
				// (about one in five) are cheaper than a second trip.
				constexpr int SPEC = 4;
				int ns = (ce - x) / k1; if (ns > SPEC) ns = SPEC; // (>= 1: the mem covers [x, x + k1))
				uint32_t vj[SPEC]; uint64_t a0[SPEC], a1[SPEC];
#pragma unroll
				for (int j = 0; j < SPEC; ++j) {
					vj[j] = 255u; a0[j] = a1[j] = 0;
					if (j < ns) {
						const uint64_t pj = p + (uint64_t)(j * k1);
						if (FUSED) { a0[j] = isa_rep_direct(ix, pj, vj[j]); if (!LEAN) a1[j] = isa_direct(ix, ix.seq_len - (pj + (uint64_t)k1)); } // (pj + k1 <= cp + ce - cb <= seq_len)
						else vj[j] = (uint32_t)ix.rep[pj];
					}
				}
				if (FUSED) C.isa += (LEAN ? 1u : 2u) * (uint32_t)ns; else C.rep += (uint32_t)ns; // (single entries, one line apiece: a byte of rep[] is counted like the 8-byte loads of r2text_kernel)
				int nu = 0; // leading unique k1-mers
#pragma unroll
				for (int j = 0; j < SPEC; ++j) if (nu == j && vj[j] < (uint32_t)k1) nu = j + 1;
				if (nu > 0) {
					if (!FUSED) {
#pragma unroll
						for (int j = 0; j < SPEC; ++j) {
							const uint64_t pj = p + (uint64_t)(j * k1);
							a0[j] = j < nu ? isa_direct(ix, pj) : 0; a1[j] = !LEAN && j < nu ? isa_direct(ix, ix.seq_len - (pj + (uint64_t)k1)) : 0;
						}
						C.isa += (LEAN ? 1u : 2u) * (uint32_t)nu;
					}
					const uint32_t k0 = take((uint32_t)nu);
#pragma unroll
					for (int j = 0; j < SPEC; ++j) {
						if (j < nu) {
							OutMem m = {a0[j], a1[j], 1, (uint64_t)(uint32_t)(x + j * k1) << 32 | (uint32_t)(x + (j + 1) * k1)};
							put(k0 + (uint32_t)j, m, p + (uint64_t)(j * k1));
						}
					}
					my_q += (unsigned)(nu * (k1 - 1)); my_hits += (unsigned)(nu * (k1 - 1)); my_text += (unsigned)nu;
					x += nu * k1;
					continue;
				}
				// the k1-mer at p is repeated (vj[0] >= k1): a short walk over lcp[] counts its occurrences
				Intv iv = {0, 0, 0}; bool ok = false;
				int L = k1;
				if (k1 < 255) {
					const int st = r3_text_len<FUSED>(ix, p, a0[0], k1, (uint32_t)(A.max_mem_intv > 0xffffffffull ? 0xffffffffull : A.max_mem_intv), L, C);
					if (st == 1 && x + L <= ce) ok = text_interval(ix, p, (uint32_t)L, iv, C) && iv.x2 < A.max_mem_intv;
					else if (ce == len && ((st == 1 && x + L > ce) || (st == 2 && ce - x <= 254))) {
						// Every prefix of [x, len) has max_mem_intv occurrences or more (the mem reaches the read's end, so the read is the
						// text all the way): bwt.c:366-377 walks to the end without reporting -- reads from tandem arrays and young
						// duplications, each such walk a chain of a hundred extensions.  Round 3 is over for this read.
						my_q += (unsigned)(len - x - 1); my_hits += (unsigned)(len - x - 1);
						x = len;
						continue;
					} else if (complete && ((st == 1 && x + L > ce) || (st == 2 && ce - x <= 254))) {
						// ... and where the mem ends inside the read, the longest match from x ends with it -- if no other mem covers x
						// and reaches further (this one was picked for an earlier x): one base more and nothing is left, which is below
						// max_mem_intv but reports nothing either (bwt.c:370-371)
						int bmb = cb, bme = ce;
						const int best = cover(x, bmb, bme);
						if (best < 0) {
							my_q += (unsigned)(ce - x); my_hits += (unsigned)(ce - x);
							x = ce + 1;
							continue;
						}
						cb = bmb; ce = bme; cp = pos_of(best);
						if (!(cp >= ix.seq_len || cp + (uint64_t)(ce - cb) > ix.seq_len)) continue; // the same question again, inside that mem
						cb = ce = 0;                                                                // (cannot happen; then the index answers)
					}
				}
				if (ok) {
					const OutMem m = {iv.x0, iv.x1, iv.x2, (uint64_t)(uint32_t)x << 32 | (uint32_t)(x + L)};
					put(take(1u), m);
					my_q += (unsigned)(L - 1); my_hits += (unsigned)(L - 1); ++my_text;
					x += L;
					continue;
				}
			}
			// bwt_seed_strategy1 on the index -- unless the min_seed_len-mer at x does not occur at all (the filter of the window
			// scheme; typically a seed across a mismatch): then the interval runs empty before the seed may end, the reference walks on
			// to min_seed_len + 1 bases reporting nothing (bwt.c:369-371), and the next seed starts there
			if (A.bloom && x + A.min_seed_len <= len) {
				uint32_t badw; const uint64_t w = rd.window(x, A.min_seed_len, badw); wc_add(W, EV_BLOOM);
				if (!(badw & ((1u << A.min_seed_len) - 1u)) && !kmer_filter_has(A.bloom, A.bloom_bits, w & ((1ull << (2 * A.min_seed_len)) - 1ull))) {
					my_q += (unsigned)(A.min_seed_len - 1); my_hits += (unsigned)(A.min_seed_len - 1);
					x = x + k1 < len ? x + k1 : len;
					continue;
				}
			}
			Intv ik; int i; bool jumped = false;
			if (jk && x + jk <= len) {
				uint32_t bad; const uint32_t code = rd.kmer(x, jk, bad);
				if (bad <= 3) { uint32_t dummy; unpack_lep(A.jump[code], ik, dummy); wc_add(W, EV_JUMP); i = x + jk; jumped = true; my_q += (unsigned)(jk - 1); my_hits += (unsigned)(jk - 1); }
			}
			if (!jumped) { ik = set_intv(ix, (int)rd.at(x)); i = x + 1; }
			int nx = len;
			bool dead = ik.x2 == 0; // an empty interval stays empty (bwt.c:369 keeps extending it): no more index reads, the
			                        // reference still walks on to the first ambiguous base or to min_seed_len bases and reports nothing
			for (; i < len; ++i) {
				const uint32_t b = rd.at(i);
				if (b > 3) { nx = i + 1; break; }
				if (dead) { if (i - x >= A.min_seed_len) { nx = i + 1; break; } continue; }
				const Intv y = extend1<false>(ix, ik, 3 - (int)b, W); ++my_q;
				if (y.x2 < A.max_mem_intv && i - x >= A.min_seed_len) {
					if (y.x2 > 0) { const OutMem m = {y.x0, y.x1, y.x2, (uint64_t)(uint32_t)x << 32 | (uint32_t)(i + 1)}; put(take(1u), m); }
					nx = i + 1; break;
				}
				ik = y; dead = y.x2 == 0;
			}
			x = nx;
		}
		if (complete && next_slot != cs) A.out_cnt[r] = next_slot;
		if (A.out_scnt && my_slots) atomicAdd(&A.out_scnt[r], my_slots);
	}
	for (int o = 32; o > 0; o >>= 1) { my_q += __shfl_xor(my_q, o); my_hits += __shfl_xor(my_hits, o); my_text += __shfl_xor(my_text, o); }
	if ((threadIdx.x & 63u) == 0) { atomicAdd(A.n_queries, my_q); if (my_hits) atomicAdd(A.n_sst_hits, my_hits); if (my_text) atomicAdd(n_text_seeds, my_text); }
	lc_flush(C, W);
	wc_flush(W, A.evc, KID_R3TEXT);
}

} // namespace csd
