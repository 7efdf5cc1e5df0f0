// smem_bwd.hpp -- the backward sweeps of the split SMEM path: the literal sweep in groups of lanes (bwd_all_kernel) and the window
// scheme (bwd_win0_kernel, bwd_win_kernel, bwd_wide_kernel).  Overview: smem_common.hpp.
#pragma once
#include "smem_common.hpp"
#include "lane_sets.hpp"

namespace csd {

// bwd_win_kernel, bwd_wide_kernel and bwd_all_kernel extend through extend1b (fm_device.hpp, occ_math.hpp), which wants L2[c] + 1 in LDS:
// each fills a four-entry table once per workgroup.  CS_OCC_LEAN = 0 builds them on extend1<true> as before (the table is then unused).
// bwd_win0_kernel stays on extend1<true>: with extend1b it was no faster and spilled more.
#ifndef CS_OCC_LEAN
#define CS_OCC_LEAN 1
#endif
__device__ __forceinline__ void bwd_l2_table(const DevIndex &ix, uint64_t *l2p1) // every thread of the workgroup must call it
{
	if (threadIdx.x < 4) l2p1[threadIdx.x] = (threadIdx.x == 0 ? ix.L2[0] : threadIdx.x == 1 ? ix.L2[1] : threadIdx.x == 2 ? ix.L2[2] : ix.L2[3]) + 1ull;
	__syncthreads();
}
template <class WC>
__device__ __forceinline__ Intv bwd_extend(const DevIndex &ix, const uint64_t *l2p1, const Intv &e, int c, WC &W)
{
#if CS_OCC_LEAN
	return extend1b(ix, l2p1, e, c, W);
#else
	return extend1<true>(ix, e, c, W);
#endif
}

template <int G, class WC>
__device__ __forceinline__ void bwd_groups_run(const SplitArgs &A, const BTask *bq, uint64_t n_tasks, unsigned long long *ctr, WaveOut &O,
                                               unsigned long long &my_q, unsigned long long &my_hits, uint4 *sst, const uint64_t *l2p1, WC &W)
{
	const bool use_sst = A.sst != 0;
	int slen = SST2_K; uint32_t scode = 0; // this lane's match as a string, while it is short enough for the SST
	constexpr uint32_t MYCLS = G == 16 ? 0u : G == 32 ? 1u : 2u;
	const DevIndex &ix = A.ix;
	const uint32_t lane = threadIdx.x & 63u, gl = lane % G, gbase = lane - gl; // group = G consecutive lanes of a wave
	const uint64_t gmask = (G >= 64) ? ~0ull : (((1ull << (G & 63)) - 1ull) << gbase);
	bool active = false, live = false;
	uint32_t r = 0, kind = 0, min_intv = 1, pend = 0;
	int i = 0, ret = 0, nm = 0, last_start = 0, xp = 0;
	Intv e = {0, 0, 0};
	PackedReader rd;

	// Every lane of the wave stays in the loop until the whole wave is done, and every lane executes the dispenser code at
	// the top and the bottom of each iteration, so its wave-uniform state stays identical in all lanes.
	//
	// Task acquisition: the backward tasks sit in the forward tasks' slots, each tagged with its size class.  A wave takes
	// 64 consecutive slots with one atomic, its 64 lanes read the 64 tags in one coalesced load, and a ballot gives the mask
	// of slots that belong to this kernel's class; idle groups then pop slots off that mask.  Skipping foreign slots costs
	// nothing per slot, so every size class can scan the whole queue.
	uint64_t batch_base = 0, avail_m = 0; bool exhausted = false;
	for (;;) {
		uint64_t idle_m = __ballot(!active && gl == 0);
		if (idle_m != 0 && avail_m == 0 && !exhausted) {
			int src = __ffsll((long long)idle_m) - 1;
			unsigned long long base = 0;
			if ((int)lane == src) base = atomicAdd(ctr, 64ull);
			base = __shfl(base, src);
			if (base >= n_tasks) exhausted = true;
			else {
				uint64_t slot = base + lane;
				uint32_t cls = slot < n_tasks ? bq[slot].cls : 0xffffffffu;
				avail_m = __ballot(cls == MYCLS);
				batch_base = base;
			}
		}
		if (idle_m != 0 && avail_m != 0) {
			// the k-th idle group (in lane order) takes the k-th set bit of avail_m
			int k = __popcll(idle_m & ((1ull << gbase) - 1ull));
			uint64_t m = avail_m;
			for (int q = 0; q < k; ++q) m &= m - 1;
			bool mine = !active && m != 0;
			uint64_t t = batch_base + (uint64_t)(__ffsll((long long)m) - 1);
			int taken = __popcll(idle_m), have = __popcll(avail_m);
			if (taken > have) taken = have;
			for (int q = 0; q < taken; ++q) avail_m &= avail_m - 1;
			if (mine) {
				BTask bt = bq[t];
				r = bt.r; kind = bt.mi_kind >> 14; min_intv = bt.mi_kind & 0x3fffu; ret = bt.ret;
				int x = bt.x, n = bt.n; xp = x;
				live = (int)gl < n;
				if (live) { unpack_lep(A.lep[(size_t)t * A.lep_stride + (n - 1 - (int)gl)], e, pend); wc_add(W, EV_LEP); }
				uint64_t rb = A.off[r];
				rd.start(A.seqp, rb, r, x - 1);
				i = x - 1; nm = 0; last_start = 0;
				slen = SST2_K; scode = 0;
				if (use_sst && live && (int)pend - x < SST2_K) { // a short LEP: spell it, the SST is keyed by the string
					slen = (int)pend - x;
					for (int q = 0; q < slen; ++q) scode = scode << 2 | rd.at(x + q);
				}
				active = true;
			}
		}
		if (exhausted && avail_m == 0 && __ballot(active) == 0) break; // wave-uniform exit
		uint64_t push0 = FTASK_NONE, push1 = FTASK_NONE, aux0 = AUX_NONE; // forward tasks this lane spawns in this step
		if (active) {
			uint32_t b = i < 0 ? 4u : rd.at(i);
			uint64_t live_m = __ballot(live) & gmask;
			int first = __ffsll((long long)live_m) - 1; // the longest live match of the group
			bool end_call = false;
			if (b > 3) { // read start or ambiguous base (bwt.c:326): every live match stops; only the longest can be new
				if ((int)lane == first && (nm == 0 || i + 1 < last_start)) push0 = emit_smem(A, r, kind, e, i + 1, pend, aux0);
				end_call = true;
			} else {
				Intv y = e;
				bool cacheable = use_sst && live && slen < SST2_K, cached = false;
				uint32_t ccode = b << (2 * slen) | scode;       // read base b in front of the string
				if (cacheable) cached = sst_get(sst, A.sst2, slen + 1, ccode, y);
				if (live) {
					++my_q;
					if (cached) ++my_hits;
					else { y = bwd_extend(ix, l2p1, e, (int)b, W); if (cacheable) sst_put(sst, A.sst2, slen + 1, ccode, y); }
					if (slen < SST2_K) { scode = ccode; ++slen; }
				}
				bool stop = live && y.x2 < min_intv, cand = live && !stop;
				uint64_t cand_m = __ballot(cand) & gmask;
				// bwt.c:328-336: the first live match is an SMEM if it stops here (nothing longer survived) and is not contained
				bool first_stops = !((cand_m >> first) & 1ull);
				if (first_stops && (nm == 0 || i + 1 < last_start)) {
					if ((int)lane == first) push0 = emit_smem(A, r, kind, e, i + 1, pend, aux0);
					++nm; last_start = i + 1;
				}
				// bwt.c:337-340: keep a surviving match unless its size equals that of the previous surviving one
				uint64_t before = cand_m & ((1ull << lane) - 1ull);
				int prev = before ? 63 - __clzll((long long)before) : (int)lane;
				uint64_t prev_x2 = __shfl(y.x2, prev);
				bool keep = cand && (before == 0 || y.x2 != prev_x2);
				live = keep; e = y;
				if (cand_m == 0) end_call = true; else --i; // the first surviving match is always kept
			}
			if (end_call) {
				if (kind == TK_ROUND1 && gl == 0) push1 = chain_round1(rd, r, (int)(A.off[r + 1] - A.off[r]), ret, xp);
				active = false;
			}
		}
		wave_push<32>(O, push0 != FTASK_NONE, push0, A, aux0);
		wave_push<32>(O, push1 != FTASK_NONE, push1, A);
	}
}

// ------------------------------------------------------------------------------------------------------------------
// The backward sweep without the triangle ("window scheme").
//
// bwt.c:325-345 carries every LEP of the forward pass backward in lockstep: with ~16 LEPs that die after ~16 steps that
// is ~136 extensions per call, almost all of them spent on matches that never reach min_seed_len and are thrown away by
// the length filter (bwamem.c:232,246).  What the sweep reports can be stated per match END t (x < t <= ret):
//   let f(t) = the first position, going left from the pivot, at which [f, t) no longer has min_intv occurrences (or the
//   read start / an ambiguous base); f is monotone in t (a longer end dies no later);
//   the LEP ending at t is reported, as [f(t)+1, t), iff every longer LEP died strictly earlier, i.e. f(t) < f(t') for
//   the nearest longer end t' (the first-survivor rule of bwt.c:328-336; LEPs dropped by the equal-size rule of
//   bwt.c:337-340 have the same occurrences as a longer one, hence the same f, and are never reported either way).
// Only reports of at least min_seed_len bases are kept, and a bi-interval is a function of the string alone.  So an end
// t < x + min_seed_len matters only if the min_seed_len-mer [t - min_seed_len, t) occurs at all, and that is looked up
// directly: the jump table gives the bi-interval of its last jump_k bases, min_seed_len - jump_k backward extensions
// decide (a random 19-mer occurs in a 6 Gbp text with probability 2 %).  A lane that survives walks on alone to its f(t).
// Ends that are not looked at die inside their window, i.e. later than any reported shorter end, so the rule above can
// be evaluated over the lanes that did survive.  Ends t >= x + min_seed_len are the LEPs the forward pass stored (it
// stores no others under this scheme); each walks alone from the pivot.  ~16 table reads + ~40 extensions, 5 deep,
// replace 136 extensions, 17 deep; results identical.
//
// A set of lanes per call: its first 18 lanes take the ends x+1 .. x+18, the following ones the stored LEPs in ascending order.
// in two halves: the filter (does the end's min_seed_len-mer occur at all? -> its jump-table code), and the table lookup
template <class WC>
__device__ __forceinline__ bool win_lane_filter(const SplitArgs &A, PackedReader &rd, uint32_t gl, int x, int ret, uint32_t &code, WC &W)
{
	const int k = A.min_seed_len, jk = A.jump_k; // jk <= k <= 24 (the window scheme's range)
	const int te = x + 1 + (int)gl;
	if ((int)gl >= k - 1 || te > ret || te - k < 0) return false;
	uint32_t badw;
	const uint64_t w = rd.window(te - k, k, badw); // the k-mer [te - k, te): its last jk bases are the jump-table code
	if (badw & ((1u << k) - 1u)) return false;     // an ambiguous base inside the window: this end cannot reach min_seed_len
	if (A.bloom) { // does the min_seed_len-mer [te - k, te) occur at all?
		wc_add(W, EV_BLOOM);
		if (!kmer_filter_has(A.bloom, A.bloom_bits, w & ((1ull << (2 * k)) - 1ull))) return false;
	}
	code = __brev((uint32_t)(w >> (2 * (k - jk))));                // group q at 2(15-q), its two bits swapped
	code = (((code & 0xAAAAAAAAu) >> 1) | ((code & 0x55555555u) << 1)) >> (32 - 2 * jk);
	return true;
}
template <class WC>
__device__ __forceinline__ bool win_lane_jump(const SplitArgs &A, uint32_t code, int te, uint32_t min_intv,
                                              Intv &e, uint32_t &pend, int &s, unsigned long long &my_q, unsigned long long &my_hits, WC &W)
{
	const int jk = A.jump_k;
	uint32_t dummy; unpack_lep(A.jump[code], e, dummy); wc_add(W, EV_JUMP);
	my_q += (unsigned)(jk - 1); my_hits += (unsigned)(jk - 1);
	if (e.x2 < min_intv) return false;
	pend = (uint32_t)te; s = te - jk - 1;
	return true;
}
template <class WC>
__device__ __forceinline__ bool win_lane_init(const SplitArgs &A, PackedReader &rd, uint32_t gl, int x, int ret, uint32_t min_intv,
                                              Intv &e, uint32_t &pend, int &s, unsigned long long &my_q, unsigned long long &my_hits, WC &W)
{
	uint32_t code;
	return win_lane_filter(A, rd, gl, x, ret, code, W) && win_lane_jump(A, code, x + 1 + (int)gl, min_intv, e, pend, s, my_q, my_hits, W);
}

// Lanes by need, not by group: a call with n stored LEPs takes 18 + n lanes, any free ones (lane_sets.hpp).  The wave keeps a
// wave-uniform mask F of the lanes that belong to no call; a lane keeps the lane set of its call (gmask, 0: free) and finds its place
// by its rank in that set -- ranks 0..17 are the window lanes, rank 18 + j is LEP j.  The loop below addresses a call only through
// gmask-masked ballots and the next higher member of a ballot, so the lanes of a call need not be contiguous or aligned.  Calls are
// taken in queue order (both classes, 4 and 5, from one slot counter: one scan of the queue); the next call waits until F holds 18 + n
// lanes, which an empty wave always does.  Placement is tried at loop entry and in iterations after F changed, never on the common path.
// CS_WIN_RELEASE: lanes that cannot matter any more (valid == false: the filter or the jump lookup failed, or the equal-size rule
// stopped them) go back to F at once, all but the call's rank 0, which pushes the call's successor at its end.  A lane that stopped
// with valid == true holds f and e for the first-survivor rule and stays to the end of its call.
#ifndef CS_WIN_RELEASE
#define CS_WIN_RELEASE 1
#endif
// CS_WIN_SETTLE: every end is settled in the iteration in which it stops, and its lane goes back to F at once (lane_sets.hpp, "settling
// an end").  The ends of a call stop from the top of its set downward -- all walking lanes of a call extend [clk, end) on one clock, a
// longer end has at most the occurrences of a shorter one, window lanes join top-down and cannot die before the LEP lanes have joined
// (their strings are substrings of every stored LEP until then), and a stopped lane's s never changes -- so when a lane stops, the
// nearest valid end above it either stops in the same iteration or stopped earlier, and a lane needs to carry one value, fup, the s of
// the nearest valid end above it that has left.  An end that reports stays as "pending" -- out of its call's set, so nothing consults it,
// holding e, s, pend, r and kind -- until the wave flushes all pending lanes in one block (emit_smem + wave_push off the common
// iteration): when CS_WIN_PEND of them have gathered, when a placement is short of the lanes they hold, and before the exit.  The call's
// successor (chain_round1: a function of the task record alone) is pushed at placement by the top lane of the new set, so no lane has to
// stay to a call's end and a call has no end event: it is over when its set is empty.  Lanes whose filter or jump lookup fails leave at
// placement.  0: the loop as it was (rule applied at the call's end, rank 0 kept for the successor), for A/B builds
// (make variant DEFS=-DCS_WIN_SETTLE=0); CS_WIN_RELEASE applies to that form only.  Both forms keep their bookkeeping in lane masks;
// the older copy of the loop that went through 0/1 registers (CS_WIN_BOOK = 0) is gone.
#ifndef CS_WIN_SETTLE
#define CS_WIN_SETTLE 1
#endif
#ifndef CS_WIN_PEND
#define CS_WIN_PEND 8
#endif
__device__ __forceinline__ uint64_t lane_mask(bool p) { return __builtin_amdgcn_ballot_w64(p); } // __ballot without the trip through a 0/1 register
template <class WC>
__device__ __forceinline__ void bwd_win_run(const SplitArgs &A, const BTask *bq, uint64_t n_tasks, unsigned long long *ctr, WaveOut &O,
                                            unsigned long long &my_q, unsigned long long &my_hits, uint8_t *slot_w, const uint64_t *l2p1, WC &W)
{
	const DevIndex &ix = A.ix;
	const uint32_t lane = threadIdx.x & 63u;
	uint64_t gmask = 0;
	bool walking = false, valid = false;
	// Per-lane state is kept narrow (the kernel runs at the register limit of its six waves per SIMD): a lane that stops keeps its position
	// in s (a stopped lane's s is the f of the scheme above: nothing moves it any more), and the extensions and jump-table credits are
	// counted in 32 bits and added to the kernel's 64-bit counters once, at the end.
#if CS_WIN_SETTLE
	int fup = csls::FUP_NONE;  // the s of the nearest valid end above this lane that has left its set
	uint64_t P = 0;            // wave-uniform: the lanes that wait to report
	uint32_t r = 0, kind = 0, min_intv = 1, pend = 0, nq = 0, nh = 0;
#else
	// The call's pivot and forward end share a word (both 16 bits), and the kind carries in bit 2 whether this lane is NOT its call's rank 0
	// (WIN_TAIL) -- early release never takes a call's rank 0, so that is the same lane from placement to the call's end, whatever left the
	// set in between.
	constexpr uint32_t WIN_TAIL = 4u;
	uint32_t r = 0, kind = 0, min_intv = 1, pend = 0, retx = 0, nq = 0, nh = 0;
#endif
	int s = 0, clk = 0;
	Intv e = {0, 0, 0};
	PackedReader rd;
	// wave-uniform: the free lanes, the 64 slots drawn last and which of them still wait, and the lanes the next placement needs
	// (18 + n of the call at the head once known, 19 before -- no call takes fewer --, 65 when the queue is used up)
	uint64_t F = ~0ull, batch_base = 0, avail_m = 0; bool exhausted = false, place = true; uint32_t need = WIN_LANES + 1;
	for (;;) {
		while (place) { // wave-uniform; repeats only after lanes came back to F inside it (duds of a placement, a flush)
			place = false;
			if (csls::count(F) >= need) {
				bool fresh = false; uint64_t t = 0;
				for (;;) {
					if (avail_m == 0) {
						if (exhausted) { need = 65; break; }
						unsigned long long base = 0;
						if (lane == 0) base = atomicAdd(ctr, 64ull);
						base = (unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)base) | (unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32;
						if (base >= n_tasks) { exhausted = true; need = 65; break; }
						const uint64_t slot = base + lane;
						uint32_t cls = 0xffffffffu, n = 0;
						if (slot < n_tasks) { cls = bq[slot].cls; n = bq[slot].n; }
						avail_m = __ballot(cls == 4u || cls == 5u);  // (n <= WIN_G64_LEPS: 18 + n <= 64)
						batch_base = base;
						__builtin_amdgcn_wave_barrier();             // (the previous draw's widths have all been read)
						slot_w[lane] = (uint8_t)(WIN_LANES + n);
						__builtin_amdgcn_wave_barrier();
						continue;
					}
					const int k = __ffsll((long long)avail_m) - 1;
					const uint32_t w = __builtin_amdgcn_readfirstlane((uint32_t)slot_w[k]);
					if (csls::count(F) < w) { need = w; break; } // the head of the queue waits for lanes; nothing overtakes it
					const bool join = csls::takes(F, lane, w);
					const uint64_t take = __ballot(join);
					if (join) { gmask = take; t = batch_base + (uint64_t)k; fresh = true; }
					F = csls::release(F, take); avail_m &= avail_m - 1; need = WIN_LANES + 1;
				}
#if CS_WIN_SETTLE
				uint64_t push1 = FTASK_NONE;
#endif
				if (fresh) {
					const uint32_t gl = csls::rank_in(gmask, lane);
					BTask bt = bq[t];
					const int xp = bt.x, ret = bt.ret;
					r = bt.r; min_intv = bt.mi_kind & 0x3fffu;
					const uint64_t rb = A.off[r];
#if CS_WIN_SETTLE
					kind = (uint32_t)(bt.mi_kind >> 14); fup = csls::FUP_NONE;
					if (kind == TK_ROUND1 && (gmask & csls::above(lane)) == 0) { // the set's top lane (always an LEP lane) pushes the call's successor
						rd.start(A.seqp, rb, r, ret);
						push1 = chain_round1(rd, r, (int)(A.off[r + 1] - rb), ret, xp);
					}
#else
					kind = (uint32_t)(bt.mi_kind >> 14) | (gl ? WIN_TAIL : 0u); retx = (uint32_t)ret | (uint32_t)xp << 16;
#endif
					rd.start(A.seqp, rb, r, xp);
					if (gl < (uint32_t)WIN_LANES) {
						unsigned long long q0 = 0, h0 = 0;
						valid = win_lane_init(A, rd, gl, xp, ret, min_intv, e, pend, s, q0, h0, W);
						nq += (uint32_t)q0; nh += (uint32_t)h0;
					} else { // (the set has exactly 18 + n members: every rank from 18 on has its LEP)
						unpack_lep(A.lep[(size_t)t * A.lep_stride + ((int)gl - WIN_LANES)], e, pend); s = xp - 1; wc_add(W, EV_LEP);
						valid = true;
					}
					walking = valid;
					clk = xp + WIN_LANES - A.jump_k - 1; // the base in front of the last window lane, the first to join
					if (clk < xp - 1) clk = xp - 1;        // (the LEP lanes join at the pivot)
				}
#if CS_WIN_SETTLE
				wave_push<32>(O, push1 != FTASK_NONE, push1, A);
				const uint64_t dud = lane_mask(fresh && !valid); // window lanes whose filter or jump lookup failed never walk: back to F
				if (dud) { F |= dud; gmask = csls::settle_set(gmask, dud, lane); place = true; }
#endif
			}
#if CS_WIN_SETTLE
			if (csls::settle_flush(F, P, need, CS_WIN_PEND)) { // the lanes that wait to report, all at once
				uint64_t push0 = FTASK_NONE, aux0 = AUX_NONE;
				if (csls::has(P, lane)) push0 = emit_smem(A, r, kind, e, s + 1, pend, aux0);
				wave_push<32>(O, push0 != FTASK_NONE, push0, A, aux0);
				F |= P; P = 0; place = true;
			}
#endif
		}
		if (exhausted && avail_m == 0 && F == ~0ull) break; // wave-uniform exit
#ifdef CS_STEP_HIST
		W.steps((uint32_t)__popcll(__ballot(gmask != 0 && walking && s == clk)));
#endif
#ifdef CS_WIN_CENSUS
#if CS_WIN_SETTLE
		W.census(F, __ballot(walking && s == clk), __ballot(walking && s != clk), P, 0ull);
#else
		W.census(F, __ballot(gmask != 0 && walking && s == clk), __ballot(gmask != 0 && walking && s != clk), __ballot(gmask != 0 && !walking && valid),
		         __ballot(gmask != 0 && !valid && kind < WIN_TAIL));
#endif
#endif
		// One clock per call: position clk is the read base every walking lane prepends in this iteration.  A lane joins when the clock
		// reaches the base in front of its match (the window lanes start staggered, the LEPs at the pivot), so all lanes that walk hold
		// matches with the SAME start, and the equal-size rule of bwt.c:337-340 applies to them as it stands: a match with as many
		// occurrences as the next longer walking one has the same occurrences, shares its fate from here on and is never reported -- it
		// stops.  In repeats that is most lanes.
		// The kernel is bound by the VALU instructions of this loop, so its bookkeeping is kept out of the vector ALU where it can be: a
		// lane that walks belongs to a call (walking implies gmask != 0), so the step needs no test of gmask -- free lanes carry a stale clk
		// and take part in the ballots below with false --, "the lanes above me in this ballot" is made once per use, and the defaults of
		// the pushes exist only in the iteration in which some call ends.
		const bool step = walking && s == clk;
		if (step) {
			uint32_t b = s < 0 ? 4u : rd.at(s);
			if (b > 3) walking = false;
			else {
				Intv y = bwd_extend(ix, l2p1, e, (int)b, W); ++nq;
				if (y.x2 < min_intv) walking = false; else { e = y; --s; }
			}
		}
#if CS_WIN_SETTLE
		bool stopv = step && !walking; // stopped in this iteration with valid == true (a lane that walks is valid)
		if ((clk & 3) == 0) { // (every fourth step is enough: a lane that could have stopped earlier only repeats a few extensions)
			const bool surv = step && walking;
			const uint64_t hi = lane_mask(surv) & gmask & csls::above(lane);
			const uint32_t ax2 = __shfl(e.x2, hi ? (int)__builtin_ctzll(hi) : (int)lane);
			if (surv && hi != 0 && ax2 == e.x2) walking = false; // (not valid any more: it leaves below without a word)
		}
		--clk;
		const uint64_t out = lane_mask(step && !walking); // the lanes that stopped in this iteration: every one of them leaves its set now
		if (out) { // (some lane of the wave stops in one iteration of a few: the rule and the masks stay off the common path)
			const uint64_t stopm = lane_mask(stopv);
			bool reports = false;
			if (stopm) {
				const uint64_t hi = csls::stops_above(stopm, gmask, lane);
				const int fn = csls::settle_fn(hi, __shfl(s, (int)csls::settle_src(hi, lane)), fup);
				reports = stopv && csls::settle_reports(s, fn, pend, A.min_seed_len);
				fup = csls::settle_carry(stopv, hi, fn, fup);
			}
			const uint64_t pm = lane_mask(reports);
			P |= pm; F |= csls::settle_freed(out, pm); place = true;
			gmask = csls::settle_set(gmask, out, lane);
		}
#else
		if ((clk & 3) == 0) { // (every fourth step is enough: a lane that could have stopped earlier only repeats a few extensions)
			const bool surv = step && walking;
			const uint64_t hi = lane_mask(surv) & gmask & csls::above(lane);
			const uint32_t ax2 = __shfl(e.x2, hi ? (int)__builtin_ctzll(hi) : (int)lane);
			if (surv && hi != 0 && ax2 == e.x2) { walking = false; valid = false; }
		}
		--clk;
		const bool ending = gmask != 0 && (lane_mask(walking) & gmask) == 0; // all ends of this lane's call are settled
		if (lane_mask(ending)) { // (a call ends once in ~20 iterations: the first-survivor rule and the dispenser stay off the common path)
			uint64_t push0 = FTASK_NONE, push1 = FTASK_NONE, aux0 = AUX_NONE;
			if (ending) {
				const uint64_t hi = lane_mask(valid) & gmask & csls::above(lane);
				const int fn = __shfl(s, hi ? (int)__builtin_ctzll(hi) : (int)lane);
				if (valid && (hi == 0 || s < fn)) push0 = emit_smem(A, r, kind & 3u, e, s + 1, pend, aux0);
				if (kind == TK_ROUND1) push1 = chain_round1(rd, r, (int)(A.off[r + 1] - A.off[r]), (int)(retx & 0xffffu), (int)(retx >> 16)); // (rank 0 only: no WIN_TAIL)
				valid = false;
			}
			wave_push<32>(O, push0 != FTASK_NONE, push0, A, aux0);
			wave_push<32>(O, push1 != FTASK_NONE, push1, A);
		}
		// lanes that go back to F: those of the calls that ended, and (CS_WIN_RELEASE) those that can no longer matter
#if CS_WIN_RELEASE
		const uint64_t gone = lane_mask(gmask != 0 && !valid && (ending || kind >= WIN_TAIL));
#else
		const uint64_t gone = lane_mask(ending);
#endif
		if (gone) {
			F |= gone; place = true;
			gmask = csls::has(gone, lane) ? 0ull : csls::release(gmask, gone);
		}
#endif
	}
	my_q += nq; my_hits += nh;
}

// Calls with more than 64 LEPs (tandem arrays, very long reads): one WAVE per call, the list stays in HBM and every step
// of the sweep streams the live part through the wave 64 entries at a time, longest first, compacting it in place (the
// write index never passes below the chunk being processed).  Same rules as above; the "previous surviving size" is
// carried from chunk to chunk.
template <class WC>
__device__ __forceinline__ void bwd_wide_run(const SplitArgs &A, const BTask *bq, uint64_t n_tasks, unsigned long long *ctr, WaveOut &O,
                                             unsigned long long &my_q, const uint64_t *l2p1, WC &W)
{
	const DevIndex &ix = A.ix;
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t lt_mask = (1ull << lane) - 1ull;
	uint64_t batch_base = 0, avail_m = 0;
	for (;;) {
		if (avail_m == 0) { // wave-uniform acquisition, as in bwd_groups_run
			unsigned long long base = 0;
			if (lane == 0) base = atomicAdd(ctr, 64ull);
			base = __shfl(base, 0);
			if (base >= n_tasks) break;
			uint64_t slot = base + lane;
			uint32_t cls = slot < n_tasks ? bq[slot].cls : 0xffffffffu;
			avail_m = __ballot(cls == 3u);
			batch_base = base;
			if (avail_m == 0) continue;
		}
		uint64_t t = batch_base + (uint64_t)(__ffsll((long long)avail_m) - 1);
		avail_m &= avail_m - 1;
		BTask bt = bq[t];
		uint32_t r = bt.r, kind = bt.mi_kind >> 14, min_intv = bt.mi_kind & 0x3fffu;
		uint4 *lep = A.lep + (size_t)t * A.lep_stride;
		PackedReader rd; rd.start(A.seqp, A.off[r], r, (int)bt.x - 1);
		int n = bt.n, lo = 0, nm = 0, last_start = 0, f_long = 0x7fffffff;
		if (n <= 64) { // the whole list fits the wave: lane g holds LEP n-1-g in registers, nothing is streamed (same rules; no compaction:
			// the longest live match is the lowest live lane, the previous survivor the nearest surviving lane below)
			bool live = (int)lane < n;
			Intv p = {0, 0, 0}; uint32_t pend = 0;
			if (live) { unpack_lep(lep[n - 1 - (int)lane], p, pend); wc_add(W, EV_LEP); }
			for (int i = (int)bt.x - 1; i >= -1; --i) {
				const uint32_t b = i < 0 ? 4u : rd.at(i);
				Intv y = p;
				if (live && b <= 3) { y = bwd_extend(ix, l2p1, p, (int)b, W); ++my_q; }
				const bool cand = live && b <= 3 && y.x2 >= min_intv;
				const uint64_t live_m = __ballot(live), cand_m = __ballot(cand);
				const int first = __ffsll((long long)live_m) - 1;
				uint64_t push0 = FTASK_NONE, aux0 = AUX_NONE;
				if (!((cand_m >> first) & 1ull) && (nm == 0 || i + 1 < last_start)) { // the longest live match stops here (bwt.c:328-336)
					if ((int)lane == first) push0 = emit_smem(A, r, kind, p, i + 1, pend, aux0);
					++nm; last_start = i + 1;
				}
				const uint64_t before = cand_m & lt_mask;
				const int prev = before ? 63 - __clzll((long long)before) : (int)lane;
				const uint64_t px2 = __shfl(y.x2, prev);
				live = cand && (!before || y.x2 != px2); // bwt.c:337-340
				if (live) p = y;
				wave_push<32>(O, push0 != FTASK_NONE, push0, A, aux0);
				f_long = i;
				if (__ballot(live) == 0) break;
			}
			n = 0; // (skips the streamed form below)
		}
		for (int i = (int)bt.x - 1; n > 0 && i >= -1; --i) {
			uint32_t b = i < 0 ? 4u : rd.at(i);
			int w = n; bool first_done = false, have_prev = false; uint64_t prev_carry = 0, push0 = FTASK_NONE, aux0 = AUX_NONE;
			for (int top = n; top > lo; top -= 64) {
				int j = top - 1 - (int)lane; bool valid = j >= lo;
				Intv p = {0, 0, 0}; uint32_t pend = 0;
				if (valid) { unpack_lep(lep[j], p, pend); wc_add(W, EV_LEP); }
				Intv y = p;
				if (valid && b <= 3) { y = bwd_extend(ix, l2p1, p, (int)b, W); ++my_q; }
				bool cand = valid && b <= 3 && y.x2 >= min_intv;
				uint64_t cand_m = __ballot(cand);
				if (!first_done) { // lane 0 of the first chunk holds the longest live match (bwt.c:328-336)
					first_done = true;
					if (!(cand_m & 1ull) && (nm == 0 || i + 1 < last_start)) {
						if (lane == 0) push0 = emit_smem(A, r, kind, p, i + 1, pend, aux0);
						++nm; last_start = i + 1;
					}
				}
				uint64_t before = cand_m & lt_mask;
				int prev = before ? 63 - __clzll((long long)before) : (int)lane;
				uint64_t px2 = __shfl(y.x2, prev);
				if (!before) px2 = prev_carry;
				bool keep = cand && ((!before && !have_prev) || y.x2 != px2); // bwt.c:337-340
				uint64_t keep_m = __ballot(keep);
				if (keep) { lep[w - 1 - __popcll(keep_m & lt_mask)] = pack_lep(y, pend); wc_add(W, EV_LEP); }
				w -= __popcll(keep_m);
				if (cand_m) { have_prev = true; prev_carry = __shfl(y.x2, 63 - __clzll((long long)cand_m)); }
			}
			__threadfence_block(); // the compacted list is read back by other lanes of this wave in the next step
			wave_push<32>(O, push0 != FTASK_NONE, push0, A, aux0);
			f_long = i;            // the step at which the last stored LEP died, if this is the last step
			if (w == n) break;
			lo = w;
		}
		if (A.win) { // window scheme: the forward pass stored only the LEPs of min_seed_len bases or more; the short ends are
			// settled here by lanes 0..17 (bwd_win_run), the nearest longer end of the longest of them being the list above
			Intv e = {0, 0, 0}; uint32_t pend = 0; int s = 0, f = 0x7fffffff;
			unsigned long long hits = 0;
			bool valid = lane < (uint32_t)WIN_LANES && win_lane_init(A, rd, lane, (int)bt.x, (int)bt.ret, min_intv, e, pend, s, my_q, hits, W);
			bool walking = valid;
			while (__ballot(walking)) {
				if (walking) {
					uint32_t b = s < 0 ? 4u : rd.at(s);
					if (b > 3) { f = s; walking = false; }
					else {
						Intv y = bwd_extend(ix, l2p1, e, (int)b, W); ++my_q;
						if (y.x2 < min_intv) { f = s; walking = false; } else { e = y; --s; }
					}
				}
			}
			uint64_t vm = __ballot(valid);
			uint64_t higher = vm & ~((2ull << lane) - 1ull);
			int src = higher ? __ffsll((long long)higher) - 1 : (int)lane;
			int fn = __shfl(f, src);
			if (!higher) fn = f_long;
			uint64_t pushw = FTASK_NONE, auxw = AUX_NONE;
			if (valid && f < fn) pushw = emit_smem(A, r, kind, e, f + 1, pend, auxw);
			wave_push<32>(O, pushw != FTASK_NONE, pushw, A, auxw);
		}
		uint64_t push1 = (kind == TK_ROUND1 && lane == 0) ? chain_round1(rd, r, (int)(A.off[r + 1] - A.off[r]), bt.ret, bt.x) : FTASK_NONE;
		wave_push<32>(O, push1 != FTASK_NONE, push1, A);
	}
}

// All cooperative backward work of one forward launch in ONE kernel: every wave works through the three size classes,
// starting with a different one depending on its workgroup, so all classes progress at once and a wave whose class runs
// dry moves on to the next instead of idling through that class's tail.  The three orders are written out (a loop over a
// class index costs 35 more VGPRs and one wave per SIMD).  ctrs[c] is the slot counter of class c.
template <int BLOCK, bool COUNT>
__global__ __launch_bounds__(BLOCK, 5) void bwd_all_kernel(const SplitArgs A, const BTask *bq, uint64_t n_tasks, unsigned long long *ctrs)
{
	if (*A.n_btasks == 0) return; // e.g. the first launch of a batch: every call sits at pivot 0 and needs no sweep
	WaveOut O = {0, 0};
	unsigned long long my_q = 0, my_hits = 0;
	__shared__ uint4 sst[SST_ENTRIES];
	__shared__ uint64_t l2p1[4];
	sst_clear(sst);
	bwd_l2_table(A.ix, l2p1);
	WaveCtrT<COUNT> W;
	const uint32_t role = blockIdx.x & 7u; // 5/8 of the workgroups start on the <=16 class, 2/8 on <=32, 1/8 on <=64
	if (role < 5) {
		bwd_groups_run<16>(A, bq, n_tasks, ctrs + 0, O, my_q, my_hits, sst, l2p1, W);
		bwd_groups_run<32>(A, bq, n_tasks, ctrs + 1, O, my_q, my_hits, sst, l2p1, W);
		bwd_groups_run<64>(A, bq, n_tasks, ctrs + 2, O, my_q, my_hits, sst, l2p1, W);
	} else if (role < 7) {
		bwd_groups_run<32>(A, bq, n_tasks, ctrs + 1, O, my_q, my_hits, sst, l2p1, W);
		bwd_groups_run<64>(A, bq, n_tasks, ctrs + 2, O, my_q, my_hits, sst, l2p1, W);
		bwd_groups_run<16>(A, bq, n_tasks, ctrs + 0, O, my_q, my_hits, sst, l2p1, W);
	} else {
		bwd_groups_run<64>(A, bq, n_tasks, ctrs + 2, O, my_q, my_hits, sst, l2p1, W);
		bwd_groups_run<16>(A, bq, n_tasks, ctrs + 0, O, my_q, my_hits, sst, l2p1, W);
		bwd_groups_run<32>(A, bq, n_tasks, ctrs + 1, O, my_q, my_hits, sst, l2p1, W);
	}
	wave_push_finish(O, A);
	atomicAdd(A.n_queries, my_q);
	if (my_hits) atomicAdd(A.n_sst_hits, my_hits);
	wc_flush(W, A.evc, KID_BWD_ALL);
}

// Calls without any stored LEP (the forward match is shorter than min_seed_len: typically the call at a mismatch, whose
// matches are all chance matches) are the bulk, and all their work is the 18 window lookups, of which 97 % end at the
// filter.  They get a kernel of their own that packs three calls into a wave (54 of 64 lanes busy) instead of one call per
// 32-lane group: a wave owns 64 consecutive slots, finds this class by ballot and works through it three at a time.  A round
// is the filter alone; the ends that pass it are PARKED in LDS (16 bytes: read, end, jump-table code, call key), and only
// when 64 of them have gathered does the wave look them up in the jump table, extend them to min_seed_len in lockstep,
// walk the survivors on to their ends -- all of that on full waves instead of one or two lanes out of 64 -- and apply the
// first-survivor rule per call (the lanes of a call found by their key).  The kernel is VALU-bound: that is the point.
// No dispenser and no atomics on the task side.
struct WinPark { uint32_t r, code; int32_t te; uint16_t mk, key; };             // an end that passed the filter; key: 64-slot batch (10 bits) | slot (6)
#ifndef CS_WIN_WAVES
#define CS_WIN_WAVES 6
#endif
#ifndef CS_WIN0_WAVES
#define CS_WIN0_WAVES 6
#endif
template <int BLOCK, bool COUNT>
__global__ __launch_bounds__(BLOCK, CS_WIN0_WAVES) void bwd_win0_kernel(const SplitArgs A, const BTask *bq, uint64_t n_tasks)
{
	if (*A.n_btasks == 0) return;
	constexpr int PARK = 64;
	constexpr int32_t F_DEAD = (int32_t)0x80000000;
	__shared__ uint8_t rank2lane[BLOCK / 64][64];
	__shared__ WinPark park[BLOCK / 64][PARK];
	__shared__ int32_t park_f[BLOCK / 64][PARK];
	const DevIndex &ix = A.ix;
	const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
	const uint32_t seg = lane / WIN_LANES, gl = lane - seg * WIN_LANES;      // three segments of 18 lanes; lanes 54..63 idle
	const int kx = A.min_seed_len - A.jump_k;                                // extensions from the jump_k-mer to min_seed_len
	WaveOut O = {0, 0};
	WaveCtrT<COUNT> W;
	unsigned long long my_q = 0, my_hits = 0;
	int npark = 0; uint32_t park_seq0 = 0; // wave-uniform: parked ends, batch number of the oldest of them
	auto flush = [&]() {
		__builtin_amdgcn_wave_barrier();
		const bool mine = (int)lane < npark;
		Intv e = {0, 0, 0}; uint32_t pend = 0, r = 0, mk = 0, key = 0; int s = 0, f = 0x7fffffff, te = 0;
		PackedReader rd;
		bool alive = false;
		if (mine) {
			const WinPark p = park[wv][lane];
			r = p.r; mk = p.mk; key = p.key; te = p.te;
			alive = win_lane_jump(A, p.code, te, mk & 0x3fffu, e, pend, s, my_q, my_hits, W);
			if (alive) rd.start(A.seqp, A.off[r], r, s);
		}
		const uint32_t kind = mk >> 14, min_intv = mk & 0x3fffu;
		for (int st = 0; st < kx; ++st) { // wave-uniform: the jump_k-mer grows to min_seed_len bases, or the lane drops out
			if (alive) {
				const uint32_t b = rd.at(s);                                   // s >= 0: the window starts inside the read
				if (b > 3) alive = false;
				else {
					Intv y = extend1<true>(ix, e, (int)b, W); ++my_q;
					if (y.x2 < min_intv) alive = false; else { e = y; --s; }
				}
			}
		}
		bool walking = alive;
		while (__ballot(walking)) {
			if (walking) {
				uint32_t b = s < 0 ? 4u : rd.at(s);
				if (b > 3) { f = s; walking = false; }
				else {
					Intv y = extend1<true>(ix, e, (int)b, W); ++my_q;
					if (y.x2 < min_intv) { f = s; walking = false; } else { e = y; --s; }
				}
			}
		}
		if (mine) park_f[wv][lane] = alive ? f : F_DEAD;
		__builtin_amdgcn_wave_barrier();
		bool emit = alive;
		if (alive) { // the nearest longer match of the same call among the parked ones that reached min_seed_len
			int best_te = 0x7fffffff, best_f = 0;
			for (int q = 0; q < npark; ++q) {
				const int tq = park[wv][q].te, fq2 = park_f[wv][q];
				if (park[wv][q].key == key && fq2 != F_DEAD && tq > te && tq < best_te) { best_te = tq; best_f = fq2; }
			}
			emit = best_te == 0x7fffffff || f < best_f;
		}
		uint64_t push0 = FTASK_NONE, aux0 = AUX_NONE;
		if (emit) push0 = emit_smem(A, r, kind, e, f + 1, pend, aux0);
		wave_push<64>(O, push0 != FTASK_NONE, push0, A, aux0);
		__builtin_amdgcn_wave_barrier();
		npark = 0;
	};
	const uint64_t n_batches = (n_tasks + 63) / 64, wstride = (uint64_t)gridDim.x * (BLOCK / 64);
	const int k = A.min_seed_len, jk = A.jump_k;
	uint32_t bseq = 0;
	for (uint64_t bch = (uint64_t)blockIdx.x * (BLOCK / 64) + wv; bch < n_batches; bch += wstride, ++bseq) { // wave-uniform
		const uint64_t slot = bch * 64 + lane;
		BTask bt = {0, 0, 0, 0, 0, 0xffffffffu};
		if (slot < n_tasks) bt = bq[slot];
		const bool is = bt.cls == 6u;
		const uint64_t m = __ballot(is);
		const int cnt = __popcll(m);
		if (cnt == 0) continue;
		if (npark && bseq - park_seq0 >= 1000u) flush(); // (keys carry ten bits of the batch number)
		// Per slot, all calls of the batch at once: the bases every window of the call can touch, [x + 1 - k, x + 18), as one
		// 96-bit string + ambiguity bits (three records at most), and the call's successor.  The rounds below then need no
		// memory access but the filter word itself.
		uint64_t cw0 = 0, cbad = ~0ull; uint32_t cw1 = 0; uint64_t push1 = FTASK_NONE;
		if (is) {
			const uint64_t rb = A.off[bt.r]; const int len = (int)(A.off[bt.r + 1] - rb);
			PackedReader rd; rd.rec = A.seqp + (rb >> 5) + bt.r;
			const int c0 = (int)bt.x + 1 - k, start = c0 < 0 ? 0 : c0;
			const uint32_t sh = (uint32_t)(start - c0), j0 = (uint32_t)start & 31u;
			const int i0 = start >> 5, imax = len >> 5;           // (record imax exists and ends the read)
			const uint4 none = {0u, 0u, ~0u, 0u};
			const uint4 q0 = rd.rec[i0], q1 = i0 + 1 <= imax ? rd.rec[i0 + 1] : none, q2 = i0 + 2 <= imax ? rd.rec[i0 + 2] : none;
			const uint64_t b0 = (uint64_t)q0.x | (uint64_t)q0.y << 32, b1 = (uint64_t)q1.x | (uint64_t)q1.y << 32, b2 = (uint64_t)q2.x | (uint64_t)q2.y << 32;
			uint64_t wa = b0 >> (j0 << 1), wb = b1 >> (j0 << 1);      // bases start .. start+31 and start+32 .. start+63
			uint64_t bad = ((uint64_t)q1.z << 32 | q0.z) >> j0;         // their ambiguity bits (64 - j0 of them; the rest from q2)
			if (j0) { wa |= b1 << ((32u - j0) << 1); wb |= b2 << ((32u - j0) << 1); bad |= (uint64_t)q2.z << (64u - j0); }
			if (sh) { wb = wb << (sh << 1) | wa >> (64u - (sh << 1)); wa <<= sh << 1; bad = bad << sh | ((1ull << sh) - 1ull); } // the read starts inside the range
			cw0 = wa; cw1 = (uint32_t)wb; cbad = bad;
			if ((bt.mi_kind >> 14) == TK_ROUND1) { rd.wk = i0; rd.bases = b0; rd.bad = q0.z; push1 = chain_round1(rd, bt.r, len, (int)bt.ret, (int)bt.x); }
			rank2lane[wv][__popcll(m & ((1ull << lane) - 1ull))] = (uint8_t)lane;
		}
		wave_push<64>(O, push1 != FTASK_NONE, push1, A);
		__builtin_amdgcn_wave_barrier();
		for (int r0 = 0; r0 < cnt; r0 += 3) { // wave-uniform
			const int rank = r0 + (int)seg;
			const bool job = seg < 3 && rank < cnt;
			const int src = job ? (int)rank2lane[wv][rank] : (int)lane;
			const uint32_t r = __shfl(bt.r, src), mk = __shfl((uint32_t)bt.mi_kind, src);
			const int x = __shfl((int)bt.x, src), ret = __shfl((int)bt.ret, src);
			const uint64_t c0w = __shfl(cw0, src), cb = __shfl(cbad, src); const uint32_t c1w = __shfl(cw1, src);
			const int te = x + 1 + (int)gl;
			bool pass = job && (int)gl < k - 1 && te <= ret && te - k >= 0;
			uint32_t code = 0;
			if (pass) {
				const uint32_t g2 = gl << 1;
				const uint64_t w = gl ? c0w >> g2 | (uint64_t)c1w << (64u - g2) : c0w; // the k-mer [te - k, te)
				pass = ((uint32_t)(cb >> gl) & ((1u << k) - 1u)) == 0;              // no ambiguous base in it
				if (pass && A.bloom) { wc_add(W, EV_BLOOM); pass = kmer_filter_has(A.bloom, A.bloom_bits, w & ((1ull << (2 * k)) - 1ull)); }
				code = __brev((uint32_t)(w >> (2 * (k - jk))));
				code = (((code & 0xAAAAAAAAu) >> 1) | ((code & 0x55555555u) << 1)) >> (32 - 2 * jk);
			}
			const uint64_t am = __ballot(pass);
			if (npark + __popcll(am) > PARK) flush();
			if (npark == 0) park_seq0 = bseq;
			if (pass) {
				WinPark p; p.r = r; p.code = code; p.te = te; p.mk = (uint16_t)mk; p.key = (uint16_t)((bseq & 0x3ffu) << 6 | (uint32_t)src);
				park[wv][npark + __popcll(am & ((1ull << lane) - 1ull))] = p;
			}
			npark += __popcll(am);
		}
		__builtin_amdgcn_wave_barrier();
	}
	if (npark) flush();
	wave_push_finish(O, A);
	atomicAdd(A.n_queries, my_q);
	if (my_hits) atomicAdd(A.n_sst_hits, my_hits);
	wc_flush(W, A.evc, KID_BWD_WIN0);
}

// window scheme: the calls with 1 to 46 stored LEPs, all from the one slot counter ctrs[0]
template <int BLOCK, bool COUNT>
__global__ __launch_bounds__(BLOCK, CS_WIN_WAVES) void bwd_win_kernel(const SplitArgs A, const BTask *bq, uint64_t n_tasks, unsigned long long *ctrs)
{
	if (*A.n_btasks == 0) return;
	__shared__ uint8_t slot_w[BLOCK / 64][64]; // per wave: the lanes each of the 64 slots drawn last needs
	__shared__ uint64_t l2p1[4];
	WaveOut O = {0, 0};
	WaveCtrT<COUNT> W;
	unsigned long long my_q = 0, my_hits = 0;
	bwd_l2_table(A.ix, l2p1);
	bwd_win_run(A, bq, n_tasks, ctrs, O, my_q, my_hits, slot_w[threadIdx.x >> 6], l2p1, W);
	wave_push_finish(O, A);
	atomicAdd(A.n_queries, my_q);
	if (my_hits) atomicAdd(A.n_sst_hits, my_hits);
	wc_flush(W, A.evc, KID_BWD_WIN);
}

// the calls with more than 64 LEPs, one wave each; rare, so it runs beside bwd_all_kernel on its own stream
#ifndef CS_WIDE_BLOCKS
#define CS_WIDE_BLOCKS 6
#endif
template <bool COUNT>
__global__ __launch_bounds__(256, CS_WIDE_BLOCKS) void bwd_wide_kernel(const SplitArgs A, const BTask *bq, uint64_t n_tasks, unsigned long long *ctr)
{
	if (*A.n_btasks == 0) return;
	WaveOut O = {0, 0};
	WaveCtrT<COUNT> W;
	unsigned long long my_q = 0;
	__shared__ uint64_t l2p1[4];
	bwd_l2_table(A.ix, l2p1);
	bwd_wide_run(A, bq, n_tasks, ctr, O, my_q, l2p1, W);
	wave_push_finish(O, A);
	atomicAdd(A.n_queries, my_q);
	wc_flush(W, A.evc, KID_BWD_WIDE);
}

} // namespace csd
