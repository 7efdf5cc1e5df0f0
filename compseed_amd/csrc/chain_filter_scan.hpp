// chain_filter_scan.hpp -- mem_chain_flt + mem_flt_chained_seeds (mapping/comp_seed.cpp:297-412) as bodies that the kernels of
// chain_filter_gpu.hip and a plain C++ program (tests/cpp/chain_filter_scan_check.cpp: W = 1 over the goldens, W = 8 / 64 on threads in
// lockstep) run alike, each indexed by chain, read, seed or lane.  chain_filter.cpp stays the specification and does not include this
// header.  No body does an atomic: where one can go wrong or has something to count it returns a verdict or a count, and the kernel (or
// the program's loop) adds it up.  The lanes are wave_lanes.hpp's.  In the order of the pass:
//   chain_weight_of  a chain: checked against n_seeds / cseed_off (false: inconsistent), its weight (chain_weight of chain_filter.cpp, both
//                    sweeps, the cap at 2^30 - 1) and its span on the read
//   classify_read    a read: chain_off and the read's length are checked, the threshold table says whether the read is long enough for the
//                    seed test, reads of more than LIGHT_MAX chains (all reads with chains under CS_FLT_WAVE_ONLY) are the wave's: V_ bits.
//                    Nothing below runs on input that any read or chain refused.
//   filter_read<W>   a read by W lanes: mem_chain_flt, the lists being the caller's.  Lane 0 sorts; the scan tests W kept chains per step
//                    and one ballot finds the first that stops it.  With one lane the ballots are the lane's own booleans and the routine
//                    is the sequential one.
//   seed_owner, seed_sw_score   a seed of a kept chain of a long read: mem_seed_sw's window, bns_fetch_seq's clip and striped_sw_score's
//                    recurrence with its two quirks; H, E and the query's codes at a stride (the wave's lanes interleave them in LDS)
//   compact_read     a read, behind two exclusive sums over the per-read counts of kept chains and kept seeds: chain_off is there, chains
//                    (n_seeds after the seed test), cseed_off, cseeds and the scores are written
// The sort is klib's introsort as klib_sort.hpp restates it: among equal weights its order decides which chain is kept and which is
// shadowed, and it is not stable for any n but 2 (the first partition runs whatever n is).  The float compares of the scan are the
// host's expressions; the units that include this are compiled without fast-math and with -ffp-contract=off.
#pragma once
#include "band_align.hpp"
#include "klib_sort.hpp"
#include "wave_lanes.hpp"

#include <climits>
#include <cmath>

namespace csf {
using csdd::lanes_below; using csdd::wballot; using csdd::wcount; using csdd::wsum; using csdd::wsync; using csdd::sc_mat;
constexpr int LIGHT_MAX = 16;               // reads of more chains go one wave per read
constexpr int LDS_CAP = 512;                // chains of a read whose lists fit the wave kernel's LDS (26 bytes per chain: 13 KB, 12 waves per CU)
constexpr uint64_t MAX_READ_LEN = 65536;    // the engine's own limit; the threshold table has one entry per length below it
constexpr int32_t NO_SW = INT32_MIN;        // table entry: no seed test for reads of this length (otherwise: min_hsp)
constexpr int32_t DROPPED = INT32_MIN;      // sscore entry: the seed test dropped this seed
constexpr int SW_MAX = 199;                 // both sequences of the seed test are shorter than 200 (MEM_SHORT_LEN)
enum { V_BAD = 1, V_LONG = 2, V_SW = 4, V_WAVE = 8 };   // classify_read: inconsistent offsets, 65,536 bases or more, needs the seed test, the wave's

struct WRec { int32_t w, idx; };
struct Heavier { CS_HD bool operator()(const WRec &a, const WRec &b) const { return a.w > b.w; } };   // flt_lt: descending weight
struct alignas(8) Iv { int32_t x, y; };     // a chain's span on the read (one 8-byte access)

struct Args {
	const uint64_t *chain_off, *cseed_off, *read_off; const cs_chain_t *chains; const cs_seed_t *cseeds; const uint8_t *bases;
	int64_t n_reads; uint64_t n_chains, n_seeds; uint32_t flags; cs_flt_params_t o;
	int64_t l_pac; const int64_t *ctg_off; const int32_t *ctg_len; int32_t n_ctg; const uint8_t *pac;
	const int32_t *tab;                                            // per read length: min_hsp, or NO_SW
	int32_t *w, *cb, *ce, *cns; uint8_t *kflag;                    // per input chain: weight, span on the read, seeds left, kept
	WRec *srt; Iv *span; int32_t *ki, *kfirst; uint8_t *alt, *keptv;     // per chain slot: a read's lists when they are not in LDS
	uint32_t *ord;                                                 // per chain slot: the read's kept chains in output order
	int32_t *sscore;                                               // per input seed: the seed test's score, or DROPPED
	uint64_t *nch, *nsd; uint32_t *wave_list;                      // per read: counts (n + 1, the last 0), scanned into chain_off / sbase
	unsigned long long *ctr;   // [0] wave reads [1] spill reads [2] inconsistent input [3] reads too long [4] the seed test is needed [5] seeds scored
	uint64_t *o_chain_off, *sbase, *o_cseed_off; cs_chain_t *o_chains; cs_seed_t *o_cseeds; int32_t *o_score;
};

// min_hsp and the seed_sw decision per read length below MAX_READ_LEN, with the very expressions of filter_range (chain_filter.cpp): the
// device's log is not asked.  Depends on a and min_chain_weight alone.
inline void fill_table(const cs_flt_params_t &o, int32_t *tab)
{
	for (int l_query = 0; l_query < (int)MAX_READ_LEN; ++l_query) {
		const double min_l = o.min_chain_weight ? 1.1f * (float)o.min_chain_weight : 5.5f * std::log((double)l_query);   // MEM_HSP_COEF, MEM_MINSC_COEF
		const bool seed_sw = !(min_l > 0.05f * (float)l_query) && l_query > 0;                                          // MEM_SEEDSW_COEF
		tab[l_query] = seed_sw ? ((l_query > 0 || o.min_chain_weight) ? (int)(o.a * min_l + .499) : 0) : NO_SW;
	}
}

CS_HD inline bool chain_weight_of(const Args &A, uint64_t c)
{
	const uint64_t s0 = A.cseed_off[c], s1 = A.cseed_off[c + 1];
	A.kflag[c] = 0;
	if (s1 <= s0 || s1 > A.n_seeds || s1 - s0 != (uint64_t)(int64_t)A.chains[c].n_seeds) { A.w[c] = INT32_MIN; A.cb[c] = A.ce[c] = 0; A.cns[c] = 0; return false; }
	const cs_seed_t *sd = A.cseeds + s0; const int n = (int)(s1 - s0);
	int64_t end = 0; int wq = 0, wr = 0;   // chain_weight of chain_filter.cpp (mem_chain_weight, comp_seed.cpp:205-224)
	for (int j = 0; j < n; ++j) {
		const int64_t b = sd[j].qbeg, e = b + sd[j].len;
		if (b >= end) wq += sd[j].len; else if (e > end) wq += (int)(e - end);
		end = std::max(end, e);
	}
	end = 0;
	for (int j = 0; j < n; ++j) {
		const int64_t b = sd[j].rbeg, e = b + sd[j].len;
		if (b >= end) wr += sd[j].len; else if (e > end) wr += (int)(e - end);
		end = std::max(end, e);
	}
	const int w = std::min(wq, wr);
	A.w[c] = w < (1 << 30) ? w : (1 << 30) - 1;
	A.cb[c] = sd[0].qbeg; A.ce[c] = sd[n - 1].qbeg + sd[n - 1].len; A.cns[c] = n;
	return true;
}

CS_HD inline int classify_read(const Args &A, int64_t r)
{
	const uint64_t c0 = A.chain_off[r], c1 = A.chain_off[r + 1], l = A.read_off[r + 1] - A.read_off[r];
	A.nch[r] = 0; A.nsd[r] = 0;
	int v = l >= MAX_READ_LEN ? V_LONG : 0;
	if (c1 < c0 || c1 > A.n_chains) return v | V_BAD;
	if (l >= MAX_READ_LEN || c1 == c0) return v;
	if (A.tab[l] != NO_SW) v |= V_SW;
	if ((A.flags & CS_FLT_WAVE_ONLY) || c1 - c0 > (uint64_t)LIGHT_MAX) v |= V_WAVE;
	return v;
}

// sig_overlap / much_lighter of chain_filter.cpp, operand for operand (a multiply, then a compare: nothing to contract)
CS_HD inline bool sig_overlap(const cs_flt_params_t &o, int bj, int ej, bool aj, int bi, int ei, bool ai)
{
	const int b_max = bj > bi ? bj : bi, e_min = ej < ei ? ej : ei;
	if (!(e_min > b_max && (!aj || ai))) return false;
	const int li = ei - bi, lj = ej - bj, min_l = li < lj ? li : lj;
	return (float)(e_min - b_max) >= (float)min_l * o.mask_level && min_l < o.max_chain_gap;
}
CS_HD inline bool much_lighter(const cs_flt_params_t &o, int wi, int wj) { return (float)wi < (float)wj * o.drop_ratio && wj - wi >= (o.min_seed_len << 1); }

// mem_chain_flt for read r, by W lanes (1 or 64); the lists are the caller's: LDS, or HBM at the read's chain slots
template <int W> CS_HD inline void filter_read(const Args &A, int64_t r, int lane, WRec *srt, Iv *span, uint8_t *alt, int32_t *ki, int32_t *kfirst, uint8_t *keptv)
{
	const uint64_t c0 = A.chain_off[r];
	const int nc = (int)(A.chain_off[r + 1] - c0);
	const uint64_t below = lanes_below(lane);
	int n = 0;                                                    // the chains of at least min_chain_weight, in input order
	for (int base = 0; base < nc; base += W) {
		const int j = base + lane; int w = 0;
		const bool ok = j < nc && (w = A.w[c0 + j]) >= A.o.min_chain_weight;
		const uint64_t m = wballot<W>(ok);
		if (ok) srt[n + wcount(m & below)] = {w, j};
		n += wcount(m);
	}
	wsync<W>();
	uint32_t n_out = 0; unsigned long long s_out = 0;
	if (n > 0) {
		if (lane == 0) cs_klib_introsort((size_t)n, srt, Heavier());
		wsync<W>();
		for (int i = lane; i < n; i += W) {
			const uint64_t c = c0 + (uint64_t)srt[i].idx;
			span[i] = {A.cb[c], A.ce[c]}; alt[i] = A.chains[c].is_alt != 0; keptv[i] = 0;
		}
		if (lane == 0) { ki[0] = 0; kfirst[0] = -1; }
		wsync<W>();
		if (lane == 0) keptv[0] = 3;
		// the overlap scan (overlap_scan_plain of chain_filter.cpp): chain i against the chains kept so far, in the order they were kept
		int nk = 1;
		for (int i = 1; i < n; ++i) {
			const Iv si = span[i]; const int wi = srt[i].w; const bool ai = alt[i] != 0;
			bool large = false, stopped = false;
			for (int base = 0; base < nk; base += W) {
				const int k = base + lane;
				bool ov = false, ml = false;
				if (k < nk) {
					const int j = ki[k]; const Iv sj = span[j];
					ov = sig_overlap(A.o, sj.x, sj.y, alt[j] != 0, si.x, si.y, ai);
					ml = ov && much_lighter(A.o, wi, srt[j].w);
				}
				const uint64_t ovm = wballot<W>(ov), stm = wballot<W>(ml);
				if (stm) {   // the scan stops at the first much heavier overlapping chain: the overlapping ones up to it take i as their shadow
					const int s = __builtin_ffsll((long long)stm) - 1;
					if (ov && lane <= s && kfirst[k] < 0) kfirst[k] = i;
					stopped = true;
					break;
				}
				if (ov && kfirst[k] < 0) kfirst[k] = i;
				large = large || ovm != 0;
			}
			if (!stopped) {
				if (lane == 0) { ki[nk] = i; kfirst[nk] = -1; keptv[i] = large ? 2 : 3; }
				++nk;
			}
			wsync<W>();
		}
		// the first chain shadowed by each kept one survives, at most max_chain_extend such extras (comp_seed.cpp:337-349)
		for (int k = lane; k < nk; k += W) { const int f = kfirst[k]; if (f >= 0) keptv[f] = 1; }
		wsync<W>();
		if (lane == 0) {
			int i = 0, extras = 0;
			for (; i < n; ++i) { const int kv = keptv[i]; if (kv == 0 || kv == 3) continue; if (++extras >= A.o.max_chain_extend) break; }
			for (; i < n; ++i) if (keptv[i] < 3) keptv[i] = 0;
		}
		wsync<W>();
		for (int base = 0; base < n; base += W) {                    // the kept chains in sorted order
			const int i = base + lane;
			const bool k = i < n && keptv[i] != 0;
			const uint64_t m = wballot<W>(k);
			if (k) { const int idx = srt[i].idx; A.ord[c0 + n_out + wcount(m & below)] = (uint32_t)idx; A.kflag[c0 + idx] = 1; s_out += (unsigned long long)A.cns[c0 + idx]; }
			n_out += wcount(m);
		}
		s_out = wsum<W>(s_out);
	}
	if (lane == 0) { A.nch[r] = n_out; A.nsd[r] = s_out; }
}

// ---- mem_flt_chained_seeds: the seeds that belong to a kept chain of a long read do the work
// the number of entries <= key in the ascending a[0..n), minus one
CS_HD inline int64_t holder_of(const uint64_t *a, int64_t n, uint64_t key)
{
	int64_t lo = 0, hi = n;
	while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a[mid] <= key) lo = mid + 1; else hi = mid; }
	return lo - 1;
}
// true: seed s is tested; its chain, its read and the read's min_hsp (seeds before cseed_off[0] or behind the last chain's belong to no chain)
CS_HD inline bool seed_owner(const Args &A, uint64_t s, int64_t *c_out, int64_t *r_out, int *min_hsp)
{
	const int64_t c = holder_of(A.cseed_off, (int64_t)A.n_chains + 1, s);
	if (!(c >= 0 && c < (int64_t)A.n_chains && A.kflag[c] != 0)) return false;
	const int64_t r = holder_of(A.chain_off, A.n_reads + 1, (uint64_t)c);
	if (!(r >= 0 && r < A.n_reads)) return false;
	*c_out = c; *r_out = r;
	*min_hsp = A.tab[A.read_off[r + 1] - A.read_off[r]];
	return *min_hsp != NO_SW;
}
// Seed s of read r: what sscore[s] gets -- the local score of the seed's neighbourhood, DROPPED below min_hsp, len * a where mem_seed_sw
// does not align (a long seed or a long window); *ran: it aligned.  H and E are the 16-bit halves of he[j * stride], the query's codes
// qs[j * stride], j < SW_MAX: sc_mat's scores are int8_t, so no score exceeds 127 * 199.
CS_HD inline int32_t seed_sw_score(const Args &A, int64_t r, uint64_t s, int min_hsp, uint32_t *he, uint8_t *qs, int stride, bool *ran)
{
	const cs_flt_params_t &o = A.o;
	const int64_t l_pac = A.l_pac;
	const int l_query = (int)(A.read_off[r + 1] - A.read_off[r]);
	const cs_seed_t sd = A.cseeds[s];
	int sw = -1; bool run = false;
	int qb = 0, qlen = 0, tlen = 0; int64_t rb = 0;
	if (sd.len < 200) {   // mem_seed_sw (comp_seed.cpp:367-391) as chain_filter.cpp states it
		qb = std::max(sd.qbeg - 50, 0); const int qe = std::min(sd.qbeg + sd.len + 50, l_query);
		rb = std::max((int64_t)sd.rbeg - 50, (int64_t)0); int64_t re = std::min((int64_t)sd.rbeg + sd.len + 50, l_pac << 1);
		const int64_t mid = (sd.rbeg + sd.rbeg + sd.len) >> 1;
		if (rb < l_pac && l_pac < re) { if (mid < l_pac) re = l_pac; else rb = l_pac; }
		if (!(qe - qb >= 200 || re - rb >= 200)) {
			const bool rev = mid >= l_pac;   // bns_fetch_seq: clip to the contig that holds `mid`, on the strand of `mid`
			const int64_t mid_f = rev ? (l_pac << 1) - 1 - mid : mid;
			int lo = 0, hi = A.n_ctg;
			while (lo < hi) { const int m = (lo + hi) >> 1; if (A.ctg_off[m] <= mid_f) lo = m + 1; else hi = m; }
			const int rid = std::max(lo - 1, 0);
			int64_t far_b = A.ctg_off[rid], far_e = far_b + A.ctg_len[rid];
			if (rev) { const int64_t tmp = far_b; far_b = (l_pac << 1) - far_e; far_e = (l_pac << 1) - tmp; }
			rb = std::max(rb, far_b); re = std::min(re, far_e);
			tlen = (int)std::max(re - rb, (int64_t)0); qlen = qe - qb; run = true;
		}
	}
	if (run) {
		sw = 0;
		if (qlen > 0 && tlen > 0) {   // striped_sw_score of chain_filter.cpp: H in place behind a carried diagonal, E beside it
			const uint8_t *q = A.bases + A.read_off[r] + (uint64_t)qb;
			for (int j = 0; j < qlen; ++j) {
				qs[j * stride] = cs_base_code_(q[j]);
				he[j * stride] = 0;
			}
			const int slen = (qlen + 7) / 8, oe_del = o.o_del + o.e_del, oe_ins = o.o_ins + o.e_ins;
			int best = 0;
			for (int i = 0; i < tlen; ++i) {
				const int64_t p = rb + i;
				const int tb = p >= l_pac ? 3 - cs_pac_base_(A.pac, (l_pac << 1) - 1 - p) : cs_pac_base_(A.pac, p);
				int f = 0, rowmax = 0, diag = 0, seg = 0;
				for (int j = 0; j < qlen; ++j) {   // the main loop: F only from inside the position's own segment
					if (seg == 0) f = 0;
					if (++seg == slen) seg = 0;
					const uint32_t x = he[j * stride];
					const int h_old = (int)(x & 0xffffu); int e = (int)(x >> 16);
					int h = diag + sc_mat(o.a, o.b, tb, qs[j * stride]);
					h = std::max(h, e); h = std::max(h, f);
					diag = h_old; rowmax = std::max(rowmax, h);
					e = std::max(std::max(e - o.e_del, 0), std::max(h - oe_del, 0));
					f = std::max(std::max(f - o.e_ins, 0), std::max(h - oe_ins, 0));
					he[j * stride] = (uint32_t)h | ((uint32_t)e << 16);
				}
				f = 0;
				for (int j = 0; j < qlen; ++j) {   // the lazy-F loop: insertions that cross segment boundaries reach H, not E
					const uint32_t x = he[j * stride];
					const int h = std::max((int)(x & 0xffffu), f);
					he[j * stride] = (x & 0xffff0000u) | (uint32_t)h;
					f = std::max(std::max(f - o.e_ins, 0), std::max(h - oe_ins, 0));
				}
				best = std::max(best, rowmax);
			}
			sw = best;
		}
	}
	*ran = run;
	if (!(sw < 0 || sw >= min_hsp)) return DROPPED;   // a short seed in a poor neighbourhood
	return sw < 0 ? sd.len * o.a : sw;
}

CS_HD inline void compact_read(const Args &A, int64_t r)
{
	const int64_t n = A.n_reads;
	const uint64_t c0 = A.chain_off[r], co = A.o_chain_off[r], nc = A.o_chain_off[r + 1] - co;
	uint64_t so = A.sbase[r];
	if (nc) {
		const bool tested = A.tab[A.read_off[r + 1] - A.read_off[r]] != NO_SW;
		for (uint64_t k = 0; k < nc; ++k) {
			const uint64_t c = c0 + A.ord[c0 + k];
			cs_chain_t ch = A.chains[c];
			A.o_cseed_off[co + k] = so;
			int kept = 0;
			for (uint64_t s = A.cseed_off[c]; s < A.cseed_off[c + 1]; ++s) {
				const cs_seed_t sd = A.cseeds[s];
				int score = sd.len;                  // what mem_chain leaves when the seed test does not run
				if (tested) { score = A.sscore[s]; if (score == DROPPED) continue; }
				A.o_cseeds[so] = sd; A.o_score[so] = score; ++so; ++kept;
			}
			ch.n_seeds = kept;
			A.o_chains[co + k] = ch;
		}
	}
	if (r == 0) A.o_cseed_off[A.o_chain_off[n]] = A.sbase[n];
}
} // namespace csf
