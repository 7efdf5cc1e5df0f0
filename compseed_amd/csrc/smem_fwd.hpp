// smem_fwd.hpp -- the forward side of the split SMEM path: the initial tasks, fwd_kernel (one lane per call) and fwd0_kernel (the
// calls at the first base of each read).  Overview: smem_common.hpp.
#pragma once
#include "smem_common.hpp"

namespace csd {

// initial tasks: round-1 call at the first unambiguous base, and the round-3 chain (bwamem.c:226, 253)
__global__ void init_tasks_kernel(const SplitArgs A, uint64_t *fq, uint64_t *fq_r3)
{
	int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= A.n_reads) return;
	uint64_t b = A.off[r]; int len = (int)(A.off[r + 1] - b), x = 0;
	PackedReader rd; rd.start(A.seqp, b, (uint32_t)r, 0);
	while (x < len && rd.at(x) > 3) ++x;
	// the round-3 chains get a queue of their own: they depend on nothing and run on a second stream (engine.hip)
	fq[r] = x < len ? ftask_pack((uint32_t)r, (uint32_t)x, 1, TK_ROUND1) : ftask_pack((uint32_t)r, 0, 0, TK_NOP);
	fq_r3[r] = (len > 0 && A.max_mem_intv > 0) ? ftask_pack((uint32_t)r, 0, 0, TK_ROUND3) : ftask_pack((uint32_t)r, 0, 0, TK_NOP);
}

template <int BLOCK, bool COUNT>
__global__ __launch_bounds__(BLOCK, 6) void fwd_kernel(const SplitArgs A)
{
	const DevIndex &ix = A.ix;
	bool active = false;
	uint64_t tslot = 0; uint32_t r = 0, kind = 0, min_intv = 1, dprev = 0;
	int len = 0, x = 0, i = 0, n = 0;
	Intv ik = {0, 0, 0};
	PackedReader rd;
	uint4 *lep = nullptr;
	uint32_t my_q = 0, my_hits = 0, my_sw = 0; // per-lane counters (a lane sees a few thousand extensions at most); bit 31 of my_sw: created a backward task
	WavePool P = {0, 0, false};
	WaveOut O = {0, 0};
	WaveCtrT<COUNT> W;
	__shared__ uint4 sst[SST_ENTRIES];
	sst_clear(sst);
	const bool use_sst = A.sst != 0;
	int slen = 0; uint32_t scode = 0; // the string matched so far, while it is short enough for the SST
	// Text mode.  Once the forward match of an SMEM call occurs exactly once, every further bwt_extend only re-ranks that one
	// occurrence: its size stays 1 until the read and the text disagree (bwt.c:309-316 pushes nothing in between).  So the
	// lane looks the occurrence's text position up in the suffix array once, compares the read against the 2-bit text eight
	// bases per iteration without touching the index, and at the end takes the reverse-strand coordinate from the inverse
	// suffix array (the forward coordinate of a unique match does not move).  Two random reads replace ~80 per read.
	const bool text_on = use_sst && ix.text2 != nullptr;
	// (text mode is kind == TK_TEXT; the text cursor lives in ik.x1)
	const int jump_k = (use_sst && A.jump && A.jump_k <= A.min_seed_len) ? A.jump_k : 0;
	// start a round-3 segment at x: through the jump table when the next jump_k bases are all A/C/G/T, else base by base
	auto r3_start = [&]() -> bool { // true: the jump table was used
		if (jump_k && x + jump_k <= len) {
			uint32_t bad; const uint32_t code = rd.kmer(x, jump_k, bad);
			if (bad == 0) {
				uint32_t e; unpack_lep(A.jump[code], ik, e); wc_add(W, EV_JUMP);
				i = x + jump_k; slen = jump_k; scode = 0;
				my_q += (unsigned)(jump_k - 1); my_hits += (unsigned)(jump_k - 1);
				return true;
			}
		}
		scode = rd.at(x); slen = 1;
		ik = set_intv(ix, (int)scode); i = x + 1;
		return false;
	};
	for (;;) {
		uint64_t t_id = 0;
		bool got = pool_take<256>(P, !active, A.task_ctr, A.n_f, t_id);
		if (!active && got) {
			tslot = t_id;
			uint64_t t = A.fq[tslot];
			kind = (uint32_t)(t >> 62);
			r = (uint32_t)t; x = (int)((t >> 32) & 0xffffu); min_intv = (uint32_t)((t >> 48) & 0x3fffu);
			dprev = 0;
			if (kind == TK_ROUND1) { dprev = min_intv - 1; min_intv = 1; } // see chain_round1
			if (kind != TK_NOP && (int64_t)r < A.n_reads) {
				uint64_t rb = A.off[r]; len = (int)(A.off[r + 1] - rb);
				if (x < len) {
					rd.start(A.seqp, rb, r, x);
					lep = A.lep + tslot * A.lep_stride; n = 0;
					if (kind == TK_ROUND3) while (x < len && rd.at(x) > 3) ++x; // first start (bwamem.c:255-256)
					if (x < len) {
						if (kind == TK_ROUND3) r3_start();
						else {
							// A round-1 call at pivot 0 keeps no LEPs (below), so its first jump_k steps can come from the
							// jump table too, provided the jump_k-mer occurs at all (otherwise: step by step, to find where it stops)
							// (the same holds for every call under the window scheme: LEPs shorter than min_seed_len are not stored)
							bool start = true;
							if (((x == 0 && kind == TK_ROUND1) || A.win) && jump_k) {
								start = false;
								if (r3_start() && ik.x2 < min_intv) { my_q -= (unsigned)(jump_k - 1); my_hits -= (unsigned)(jump_k - 1); start = true; }
							}
							if (start) { scode = rd.at(x); slen = 1; ik = set_intv(ix, (int)scode); i = x + 1; }
						}
						active = true;
					}
				}
			}
		}
		if (P.exhausted && __ballot(active) == 0) break; // wave-uniform exit
		uint64_t push0 = FTASK_NONE, push1 = FTASK_NONE, aux0 = AUX_NONE; // forward tasks this lane spawns in this step
		if (active) {
			bool fin = false; // the forward pass of an SMEM call ends in this iteration with ik = [x, i)
			uint64_t fpos = POS_NONE; // text position of read base x, where the match ended in text mode (as in fwd0_kernel)
			if (kind == TK_TEXT) {
				uint64_t tpos = ik.x1;
				fin = text_step(ix, rd, i, tpos, my_q, my_hits, W);        // up to 32 bases against the text
				ik.x1 = tpos;
				if (fin) {
					fpos = tpos - (uint64_t)(i - x);
					ik.x1 = isa_direct(ix, ix.seq_len - tpos); kind = TK_ROUND1; // rank of the reverse complement of [x, i)
					wc_add(W, EV_ISA);
					// The sweep of this call cannot pass the previous pivot x - dprev (chain_round1), and while the unique
					// match keeps agreeing with the text in front of it, it stays the longest survivor and nothing else is
					// reported (bwt.c:328-336).  So if the dprev - 1 bases between the pivots agree, the whole sweep reports
					// exactly one SMEM, [x - dprev + 1, i), and its bi-interval comes from the inverse suffix array.
					if (dprev > 0 && (A.text_sweep & TS_SWEEP)) {
						const int nb = (int)dprev - 1;
						const uint64_t px = fpos;
						bool same = px >= (uint64_t)nb;
						for (int done = 0; same && done < nb;) { // read [x - nb, x) against the text in front of px, a record at a time
							const int p = x - nb + done;
							rd.seek(p);
							const uint32_t j = (uint32_t)p & 31u, room = 32u - j, n = (uint32_t)(nb - done) < room ? (uint32_t)(nb - done) : room;
							const uint64_t dx = (rd.bases >> (j << 1)) ^ text_win(ix, px - (uint64_t)(nb - done)); wc_add(W, EV_TEXT, 4u);
							const uint64_t keep = n >= 32u ? ~0ull : (1ull << (n << 1)) - 1ull;
							same = (dx & keep) == 0 && ((rd.bad >> j) & (uint32_t)(n >= 32u ? ~0u : (1u << n) - 1u)) == 0;
							done += (int)n;
						}
						if (same) {
							Intv m = {isa_direct(ix, px - (uint64_t)nb), ik.x1, 1}; wc_add(W, EV_ISA);
							push0 = emit_smem(A, r, TK_ROUND1, m, x - nb, (uint32_t)i, aux0, px - (uint64_t)nb); // (m.x0 is the rank of that position)
							push1 = chain_round1(rd, r, len, i, x);
							++my_sw; active = false; fin = false;
						}
					}
				}
			} else {
				// ---- the one extension site: forward by read base i (bwt.c:309-311 / 368-369)
				uint32_t b = i < len ? rd.at(i) : 4u;
				Intv y = ik;
				bool cached = false, cacheable = use_sst && b <= 3 && slen < SST2_K;
				uint32_t ccode = scode << 2 | b;                    // the string extended by read base b
				if (cacheable) cached = sst_get(sst, A.sst2, slen + 1, ccode, y);
				if (b <= 3) {
					++my_q;
					if (cached) ++my_hits;
					else { y = extend1<false>(ix, ik, 3 - (int)b, W); if (cacheable) sst_put(sst, A.sst2, slen + 1, ccode, y); }
					scode = ccode; ++slen;                          // slen keeps counting; only values < SST2_K are looked at
				}
				if (kind == TK_ROUND3) { // bwt_seed_strategy1, bwt.c:366-377
					if (b <= 3 && !(y.x2 < A.max_mem_intv && i - x >= A.min_seed_len)) { ik = y; ++i; }
					else if (b > 3 && i >= len) active = false;
					else {
						if (b <= 3 && y.x2 > 0) emit_mem(A, r, y, (uint32_t)x, (uint32_t)(i + 1));
						x = i + 1; // restart behind the seed / the ambiguous base
						while (x < len && rd.at(x) > 3) ++x;
						if (x >= len) active = false; else r3_start();
					}
				} else { // ---- forward pass of an SMEM call, bwt.c:303-320
					const bool changed = b > 3 || y.x2 != ik.x2;            // read end (i == len), ambiguous base, or size change
					fin = b > 3 || (y.x2 != ik.x2 && y.x2 < min_intv);
					if (changed && !fin && x != 0 && (!A.win || i - x >= A.min_seed_len)) { lep[n++] = pack_lep(ik, (uint32_t)i); wc_add(W, EV_LEP); }
					if (!fin) {
						ik = y; ++i;
						if (text_on && ik.x2 == 1 && kind == TK_ROUND1) { // unique from here on: continue on the text
							const uint64_t tp = sa_direct(ix, ik.x0) + (uint64_t)(i - x); // text cursor: the base that has to equal read base i
							wc_add(W, EV_SA);
							if (tp <= ix.seq_len) { kind = TK_TEXT; ik.x1 = tp; }  // (always: the match lies inside the text)
						}
					}
				}
			}
			if (fin) { // ik = the longest forward match [x, i): the last LEP (bwt.c:307/315/320)
				// A call at pivot 0 has a trivial backward sweep (bwt.c:325 starts at i = -1): its only SMEM is the longest
				// forward match, so it needs no LEP list, no backward task, and finishes right here.
				if (x == 0) {
					push0 = emit_smem(A, r, kind, ik, 0, (uint32_t)i, aux0, fpos); // (fpos: a call that ended in text mode; ik.x0 has not moved since SA[ik.x0] was read)
					if (kind == TK_ROUND1) push1 = chain_round1(rd, r, len, i, x);
				} else { // hand the list to the backward kernel of its size class; ret = end of the longest match = next pivot
					if (!A.win || i - x >= A.min_seed_len) { lep[n++] = pack_lep(ik, (uint32_t)i); wc_add(W, EV_LEP); }
					uint32_t cls = n <= 16 ? 0u : n <= 32 ? 1u : n <= 64 ? 2u : 3u;
					if (A.win) cls = n == 0 ? 6u : n <= WIN_G32_LEPS ? 4u : n <= WIN_G64_LEPS ? 5u : 3u;
					BTask bt = {r, (uint16_t)x, (uint16_t)(min_intv | kind << 14), (uint16_t)n, (uint16_t)i, cls};
					A.bq[tslot] = bt;
					my_sw |= 0x80000000u;
				}
				active = false;
			}
		}
		wave_push<64>(O, push0 != FTASK_NONE, push0, A, aux0);
		wave_push<64>(O, push1 != FTASK_NONE, push1, A);
	}
	wave_push_finish(O, A);
	atomicAdd(A.n_queries, (unsigned long long)my_q);
	if (my_hits) atomicAdd(A.n_sst_hits, (unsigned long long)my_hits);
	if (my_sw & 0x80000000u) atomicAdd(A.n_btasks, 1ull);
	if (my_sw & 0x7fffffffu) atomicAdd(A.n_text_sweeps, (unsigned long long)(my_sw & 0x7fffffffu));
	wc_flush(W, A.evc, KID_FWD);
}


// The first launch of a batch: every call is a round-1 call at the read's first base, and almost all of them go jump table
// -> a few extensions until the match is unique -> text mode -> one SMEM, the next pivot, a re-seeding candidate.  None of
// that needs LEPs, backward tasks, the SST or round 3, so these calls get a kernel without them: half the registers of
// fwd_kernel (the calls are latency-bound, so resident waves are what counts).  It takes the calls it can start from the
// jump table and replaces them by no-ops in the queue; whatever is left (reads that begin with an ambiguous base, are
// shorter than jump_k, or whose first jump_k-mer does not occur) is fwd_kernel's, launched over the same queue afterwards.
template <int BLOCK, bool COUNT>
__global__ __launch_bounds__(BLOCK, 8) void fwd0_kernel(const SplitArgs A, uint64_t *fq)
{
	const DevIndex &ix = A.ix;
	const int jk = A.jump_k;
	bool active = false, textm = false;
	uint32_t r = 0;
	int len = 0, i = 0;
	Intv ik = {0, 0, 0};
	PackedReader rd;
	uint32_t my_q = 0, my_hits = 0, my_r2 = 0;
	WavePool P = {0, 0, false};
	WaveOut O = {0, 0};
	WaveCtrT<COUNT> W;
	for (;;) {
		uint64_t t_id = 0;
		bool got = pool_take<256>(P, !active, A.task_ctr, A.n_f, t_id);
		if (!active && got) {
			const uint64_t t = fq[t_id];
			r = (uint32_t)t;
			if ((uint32_t)(t >> 62) == TK_ROUND1 && ((t >> 32) & 0xffffu) == 0 && (int64_t)r < A.n_reads) {
				const uint64_t rb = A.off[r]; len = (int)(A.off[r + 1] - rb);
				if (len >= jk) {
					rd.start(A.seqp, rb, r, 0);
					uint32_t bad; const uint32_t code = rd.kmer(0, jk, bad);
					uint32_t e; unpack_lep(A.jump[code], ik, e); wc_add(W, EV_JUMP);
					if (bad <= 3 && ik.x2 > 0) {
						fq[t_id] = FTASK_NONE;                       // ours
						i = jk; textm = false; active = true;
						my_q += (unsigned)(jk - 1); my_hits += (unsigned)(jk - 1);
					}
				}
			}
		}
		if (P.exhausted && __ballot(active) == 0) break; // wave-uniform exit
		uint64_t push0 = FTASK_NONE, push1 = FTASK_NONE, aux0 = AUX_NONE;
		if (active) {
			bool fin = false;
			uint64_t fpos = POS_NONE; // text position of the read's first base, where the match ended in text mode
			if (textm) { // as in fwd_kernel: the unique match against the 2-bit text, cursor in ik.x1
				uint64_t tpos = ik.x1;
				fin = text_step(ix, rd, i, tpos, my_q, my_hits, W);
				ik.x1 = tpos;
				if (fin) { fpos = tpos - (uint64_t)i; ik.x1 = isa_direct(ix, ix.seq_len - tpos); wc_add(W, EV_ISA); }
			} else {
				uint32_t b = i < len ? rd.at(i) : 4u;
				if (b > 3) fin = true;
				else {
					++my_q;
					const Intv y = extend1<false>(ix, ik, 3 - (int)b, W);
					if (y.x2 == 0) fin = true;                       // bwt.c:313-315 with min_intv = 1
					else {
						ik = y; ++i;
						if (ik.x2 == 1) {
							const uint64_t tp = sa_direct(ix, ik.x0) + (uint64_t)i;
							wc_add(W, EV_SA);
							if (tp <= ix.seq_len) { textm = true; ik.x1 = tp; } // (always: the match lies inside the text)
						}
					}
				}
			}
			if (fin) { // the call's only SMEM is its longest forward match (bwt.c:325 starts the sweep at -1)
				push0 = emit_smem(A, r, TK_ROUND1, ik, 0, (uint32_t)i, aux0, fpos);
				if (push0 != FTASK_NONE && aux0 != AUX_NONE && fpos != POS_NONE && ix.rep) { // its re-seeding call, if rep[] settles it right here
					uint32_t nw = 0; const int pv = i >> 1;                                    // (emit_smem: pivot = (beg + end) / 2, beg = 0)
					if (A.min_seed_len >= 2 && fpos + (uint64_t)i <= ix.seq_len && pv <= 4096 && r2_quick_rep(ix, fpos, i, pv, A.min_seed_len, nw) == 0) { push0 = FTASK_NONE; ++my_r2; }
					wc_add(W, EV_REP, nw);
				}
				push1 = chain_round1(rd, r, len, i, 0);
				active = false;
			}
		}
		if (__ballot((push0 & push1) != FTASK_NONE)) {
			wave_push<64>(O, push0 != FTASK_NONE, push0, A, aux0);
			wave_push<64>(O, push1 != FTASK_NONE, push1, A);
		}
	}
	wave_push_finish(O, A);
	atomicAdd(A.n_queries, (unsigned long long)my_q);
	if (my_hits) atomicAdd(A.n_sst_hits, (unsigned long long)my_hits);
	if (my_r2) atomicAdd(A.n_r2_quick, (unsigned long long)my_r2);
	wc_flush(W, A.evc, KID_FWD0);
}

} // namespace csd
