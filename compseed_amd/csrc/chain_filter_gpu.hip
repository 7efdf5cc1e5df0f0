// chain_filter_gpu.hip -- cs_chain_filter_device / cs_chain_filter_gpu: mem_chain_flt + mem_flt_chained_seeds of the reference
// (mapping/comp_seed.cpp:297-412) on the GPU, byte for byte what cs_chain_filter (chain_filter.cpp) returns, which stays the specification.
// A read's work is sequential over its chains (the sort, then the scan down the sorted list), so a read is one lane or one wave:
//   weight_kernel    one lane per input chain: the chain is checked against n_seeds / cseed_off (ctr[2] counts what is inconsistent), its
//                    weight (chain_weight of chain_filter.cpp, both sweeps, the cap at 2^30 - 1) and its span on the read are written.
//   classify_kernel  one lane per read: chain_off and the read's length are checked (ctr[2], ctr[3]), the threshold table says whether the
//                    read is long enough for the seed test (ctr[4]), reads of more than LIGHT_MAX chains go to the wave list (all reads
//                    with chains under CS_FLT_WAVE_ONLY).  The host waits for the counters: nothing below runs on inconsistent input.
//   light_kernel     reads of up to LIGHT_MAX chains, one lane each, lists in HBM scratch at the read's own chain slots.
//   wave_kernel      one wave per read of the wave list, lists in LDS up to LDS_CAP chains, else the same code on the HBM scratch
//                    (ctr[1]).  Lane 0 sorts; the scan tests 64 kept chains per step and one ballot finds the first that stops it.
//   sw_kernel        (only if ctr[4]) one lane per seed of a kept chain of a long read: mem_seed_sw's window, bns_fetch_seq's clip and
//                    striped_sw_score's recurrence with its two quirks, H and E rows interleaved in LDS across the lanes.
//   compact_kernel   two exclusive scans over the per-read counts of kept chains and kept seeds, then one lane per read writes chain_off,
//                    chains (n_seeds after the seed test), cseed_off, cseeds and the scores.
// The sort is klib's introsort as klib_sort.hpp restates it, compiled for the device: among equal weights its order decides which chain
// is kept and which is shadowed, and it is not stable for any n but 2 (the first partition runs whatever n is).  The float compares of the
// scan are the host's expressions; the unit is compiled without fast-math and with -ffp-contract=off like the rest.
#include "dev_stage.hpp"
#include "klib_sort.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

namespace csf {
constexpr int LIGHT_MAX = 16;               // reads of more chains go one wave per read
constexpr int LDS_CAP = 512;                // chains of a read whose lists fit the wave kernel's LDS (26 bytes per chain: 13 KB, 12 waves per CU)
constexpr uint64_t MAX_READ_LEN = 65536;    // the engine's own limit; the threshold table has one entry per length below it
constexpr int32_t NO_SW = INT32_MIN;        // table entry: no seed test for reads of this length (otherwise: min_hsp)
constexpr int32_t DROPPED = INT32_MIN;      // sscore entry: the seed test dropped this seed
constexpr int SW_MAX = 199;                 // both sequences of the seed test are shorter than 200 (MEM_SHORT_LEN)

struct WRec { int32_t w, idx; };
struct Heavier { __host__ __device__ bool operator()(const WRec &a, const WRec &b) const { return a.w > b.w; } };   // flt_lt: descending weight

struct Args {
	const uint64_t *chain_off, *cseed_off, *read_off; const cs_chain_t *chains; const cs_seed_t *cseeds; const uint8_t *bases;
	int64_t n_reads; uint64_t n_chains, n_seeds; uint32_t flags; cs_flt_params_t o;
	int64_t l_pac; const int64_t *ctg_off; const int32_t *ctg_len; int32_t n_ctg; const uint8_t *pac;
	const int32_t *tab;                                            // per read length: min_hsp, or NO_SW
	int32_t *w, *cb, *ce, *cns; uint8_t *kflag;                    // per input chain: weight, span on the read, seeds left, kept
	WRec *srt; int2 *span; int32_t *ki, *kfirst; uint8_t *alt, *keptv;   // per chain slot: a read's lists when they are not in LDS
	uint32_t *ord;                                                 // per chain slot: the read's kept chains in output order
	int32_t *sscore;                                               // per input seed: the seed test's score, or DROPPED
	uint64_t *nch, *nsd; uint32_t *wave_list;                      // per read: counts (n + 1, the last 0), scanned into chain_off / sbase
	unsigned long long *ctr;   // [0] wave reads [1] spill reads [2] inconsistent input [3] reads too long [4] the seed test is needed [5] seeds scored
	uint64_t *o_chain_off, *sbase, *o_cseed_off; cs_chain_t *o_chains; cs_seed_t *o_cseeds; int32_t *o_score;
};

__global__ void __launch_bounds__(256) weight_kernel(Args A)
{
	for (uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; c < A.n_chains; c += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t s0 = A.cseed_off[c], s1 = A.cseed_off[c + 1];
		A.kflag[c] = 0;
		if (s1 <= s0 || s1 > A.n_seeds || s1 - s0 != (uint64_t)(int64_t)A.chains[c].n_seeds) { atomicAdd(A.ctr + 2, 1ull); A.w[c] = INT32_MIN; A.cb[c] = A.ce[c] = 0; A.cns[c] = 0; continue; }
		const cs_seed_t *sd = A.cseeds + s0; const int n = (int)(s1 - s0);
		int64_t end = 0; int wq = 0, wr = 0;   // chain_weight of chain_filter.cpp (mem_chain_weight, comp_seed.cpp:205-224)
		for (int j = 0; j < n; ++j) {
			const int64_t b = sd[j].qbeg, e = b + sd[j].len;
			if (b >= end) wq += sd[j].len; else if (e > end) wq += (int)(e - end);
			end = max(end, e);
		}
		end = 0;
		for (int j = 0; j < n; ++j) {
			const int64_t b = sd[j].rbeg, e = b + sd[j].len;
			if (b >= end) wr += sd[j].len; else if (e > end) wr += (int)(e - end);
			end = max(end, e);
		}
		const int w = min(wq, wr);
		A.w[c] = w < (1 << 30) ? w : (1 << 30) - 1;
		A.cb[c] = sd[0].qbeg; A.ce[c] = sd[n - 1].qbeg + sd[n - 1].len; A.cns[c] = n;
	}
}

__global__ void __launch_bounds__(256) classify_kernel(Args A)
{
	for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < A.n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		const uint64_t c0 = A.chain_off[r], c1 = A.chain_off[r + 1], l = A.read_off[r + 1] - A.read_off[r];
		A.nch[r] = 0; A.nsd[r] = 0;
		if (l >= MAX_READ_LEN) atomicAdd(A.ctr + 3, 1ull);
		if (c1 < c0 || c1 > A.n_chains) { atomicAdd(A.ctr + 2, 1ull); continue; }
		if (l >= MAX_READ_LEN || c1 == c0) continue;
		if (A.tab[l] != NO_SW) atomicOr(A.ctr + 4, 1ull);
		if ((A.flags & CS_FLT_WAVE_ONLY) || c1 - c0 > (uint64_t)LIGHT_MAX) A.wave_list[atomicAdd(A.ctr + 0, 1ull)] = (uint32_t)r;
	}
}

// sig_overlap / much_lighter of chain_filter.cpp, operand for operand (a multiply, then a compare: nothing to contract)
__device__ __forceinline__ bool sig_overlap(const cs_flt_params_t &o, int bj, int ej, bool aj, int bi, int ei, bool ai)
{
	const int b_max = max(bj, bi), e_min = min(ej, ei);
	if (!(e_min > b_max && (!aj || ai))) return false;
	const int li = ei - bi, lj = ej - bj, min_l = min(li, lj);
	return (float)(e_min - b_max) >= (float)min_l * o.mask_level && min_l < o.max_chain_gap;
}
__device__ __forceinline__ bool much_lighter(const cs_flt_params_t &o, int wi, int wj) { return (float)wi < (float)wj * o.drop_ratio && wj - wi >= (o.min_seed_len << 1); }

// mem_chain_flt for read r, by W lanes (1 or 64); the lists are the caller's: LDS, or HBM at the read's chain slots
template <int W> __device__ __forceinline__ void filter_read(const Args &A, int64_t r, int lane, WRec *srt, int2 *span, uint8_t *alt, int32_t *ki, int32_t *kfirst, uint8_t *keptv)
{
	const uint64_t c0 = A.chain_off[r];
	const int nc = (int)(A.chain_off[r + 1] - c0);
	const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
	// the chains of at least min_chain_weight, in input order
	int n = 0;
	if constexpr (W == 1) {
		for (int j = 0; j < nc; ++j) { const int w = A.w[c0 + j]; if (w >= A.o.min_chain_weight) srt[n++] = {w, j}; }
	} else {
		for (int base = 0; base < nc; base += W) {
			const int j = base + lane; int w = 0;
			const bool ok = j < nc && (w = A.w[c0 + j]) >= A.o.min_chain_weight;
			const uint64_t m = __ballot(ok);
			if (ok) srt[n + __popcll(m & below)] = {w, j};
			n += __popcll(m);
		}
		__syncthreads();
	}
	uint32_t n_out = 0; unsigned long long s_out = 0;
	if (n > 0) {
		if (lane == 0) cs_klib_introsort((size_t)n, srt, Heavier());
		if constexpr (W > 1) __syncthreads();
		for (int i = lane; i < n; i += W) {
			const uint64_t c = c0 + (uint64_t)srt[i].idx;
			span[i] = make_int2(A.cb[c], A.ce[c]); alt[i] = A.chains[c].is_alt != 0; keptv[i] = 0;
		}
		if (lane == 0) { ki[0] = 0; kfirst[0] = -1; }
		if constexpr (W > 1) __syncthreads();
		if (lane == 0) keptv[0] = 3;
		// the overlap scan (overlap_scan_plain of chain_filter.cpp): chain i against the chains kept so far, in the order they were kept
		int nk = 1;
		for (int i = 1; i < n; ++i) {
			const int2 si = span[i]; const int wi = srt[i].w; const bool ai = alt[i] != 0;
			bool large = false, stopped = false;
			if constexpr (W == 1) {
				for (int k = 0; k < nk; ++k) {
					const int j = ki[k]; const int2 sj = span[j];
					if (sig_overlap(A.o, sj.x, sj.y, alt[j] != 0, si.x, si.y, ai)) {
						large = true;
						if (kfirst[k] < 0) kfirst[k] = i;
						if (much_lighter(A.o, wi, srt[j].w)) { stopped = true; break; }
					}
				}
			} else {
				for (int base = 0; base < nk; base += W) {
					const int k = base + lane;
					bool ov = false, ml = false;
					if (k < nk) {
						const int j = ki[k]; const int2 sj = span[j];
						ov = sig_overlap(A.o, sj.x, sj.y, alt[j] != 0, si.x, si.y, ai);
						ml = ov && much_lighter(A.o, wi, srt[j].w);
					}
					const uint64_t ovm = __ballot(ov), stm = __ballot(ml);
					if (stm) {   // the scan stops at the first much heavier overlapping chain: the overlapping ones up to it take i as their shadow
						const int s = __ffsll((unsigned long long)stm) - 1;
						if (ov && lane <= s && kfirst[k] < 0) kfirst[k] = i;
						stopped = true;
						break;
					}
					if (ov && kfirst[k] < 0) kfirst[k] = i;
					large = large || ovm != 0;
				}
			}
			if (!stopped) {
				if (lane == 0) { ki[nk] = i; kfirst[nk] = -1; keptv[i] = large ? 2 : 3; }
				++nk;
			}
			if constexpr (W > 1) __syncthreads();
		}
		// the first chain shadowed by each kept one survives, at most max_chain_extend such extras (comp_seed.cpp:337-349)
		for (int k = lane; k < nk; k += W) { const int f = kfirst[k]; if (f >= 0) keptv[f] = 1; }
		if constexpr (W > 1) __syncthreads();
		if (lane == 0) {
			int i = 0, extras = 0;
			for (; i < n; ++i) { const int kv = keptv[i]; if (kv == 0 || kv == 3) continue; if (++extras >= A.o.max_chain_extend) break; }
			for (; i < n; ++i) if (keptv[i] < 3) keptv[i] = 0;
		}
		if constexpr (W > 1) __syncthreads();
		// the kept chains in sorted order
		if constexpr (W == 1) {
			for (int i = 0; i < n; ++i) if (keptv[i]) { const int idx = srt[i].idx; A.ord[c0 + n_out++] = (uint32_t)idx; A.kflag[c0 + idx] = 1; s_out += (unsigned long long)A.cns[c0 + idx]; }
		} else {
			for (int base = 0; base < n; base += W) {
				const int i = base + lane;
				const bool k = i < n && keptv[i] != 0;
				const uint64_t m = __ballot(k);
				if (k) { const int idx = srt[i].idx; A.ord[c0 + n_out + __popcll(m & below)] = (uint32_t)idx; A.kflag[c0 + idx] = 1; s_out += (unsigned long long)A.cns[c0 + idx]; }
				n_out += __popcll(m);
			}
			for (int d = 32; d > 0; d >>= 1) s_out += __shfl_xor(s_out, d);
		}
	}
	if (lane == 0) { A.nch[r] = n_out; A.nsd[r] = s_out; }
}

__global__ void __launch_bounds__(256) light_kernel(Args A)
{
	if (A.flags & CS_FLT_WAVE_ONLY) return;
	for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < A.n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		const uint64_t c0 = A.chain_off[r], nc = A.chain_off[r + 1] - c0;
		if (nc == 0 || nc > (uint64_t)LIGHT_MAX) continue;
		filter_read<1>(A, r, 0, A.srt + c0, A.span + c0, A.alt + c0, A.ki + c0, A.kfirst + c0, A.keptv + c0);
	}
}

__global__ void __launch_bounds__(64) wave_kernel(Args A)
{
	__shared__ WRec s_srt[LDS_CAP]; __shared__ int2 s_span[LDS_CAP]; __shared__ int32_t s_ki[LDS_CAP], s_kfirst[LDS_CAP]; __shared__ uint8_t s_alt[LDS_CAP], s_keptv[LDS_CAP];
	const unsigned long long n = A.ctr[0];
	const int lane = threadIdx.x;
	for (unsigned long long w = blockIdx.x; w < n; w += gridDim.x) {
		const int64_t r = A.wave_list[w];
		const uint64_t c0 = A.chain_off[r], nc = A.chain_off[r + 1] - c0;
		if (nc <= (uint64_t)LDS_CAP) filter_read<64>(A, r, lane, s_srt, s_span, s_alt, s_ki, s_kfirst, s_keptv);
		else {
			if (lane == 0) atomicAdd(A.ctr + 1, 1ull);
			filter_read<64>(A, r, lane, A.srt + c0, A.span + c0, A.alt + c0, A.ki + c0, A.kfirst + c0, A.keptv + c0);
		}
		__syncthreads();
	}
}

// ---- mem_flt_chained_seeds: one lane per input seed; the lanes whose seed belongs to a kept chain of a long read do the work
// the number of entries <= key in the ascending a[0..n), minus one
__device__ __forceinline__ int64_t holder_of(const uint64_t *a, int64_t n, uint64_t key)
{
	int64_t lo = 0, hi = n;
	while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a[mid] <= key) lo = mid + 1; else hi = mid; }
	return lo - 1;
}
// entry t * 5 + q of bwa_fill_scmat's 5 x 5 matrix of int8_t, as the host fills it: a and -b pass through int8_t (a = 400 scores -112), and
// the host indexes the flat array with the query's code, which can be 5 for '-'.  So no score exceeds 127 * 199: H and E fit 16 bits.
__device__ __forceinline__ int sc_mat(const cs_flt_params_t &o, int t, int q) { const int x = t * 5 + q, i = x / 5, j = x - i * 5; return (i == 4 || j == 4) ? -1 : i == j ? (int)(int8_t)o.a : (int)(int8_t)-o.b; }

// H and E as the 16-bit halves of one LDS word per query position, the query's codes beside them, all interleaved across the wave's lanes
__global__ void __launch_bounds__(64) sw_kernel(Args A)
{
	__shared__ uint32_t he[SW_MAX * 64];
	__shared__ uint8_t qs[SW_MAX * 64];
	const int lane = threadIdx.x;
	const cs_flt_params_t &o = A.o;
	const int64_t l_pac = A.l_pac;
	for (uint64_t s0 = (uint64_t)blockIdx.x * 64; s0 < A.n_seeds; s0 += (uint64_t)gridDim.x * 64) {
		const uint64_t s = s0 + lane;
		bool active = s < A.n_seeds;
		int64_t c = 0, r = 0; int min_hsp = 0, l_query = 0;
		if (active) { c = holder_of(A.cseed_off, (int64_t)A.n_chains + 1, s); active = c >= 0 && c < (int64_t)A.n_chains && A.kflag[c] != 0; }   // (seeds before cseed_off[0] or behind the last chain's belong to no chain)
		if (active) { r = holder_of(A.chain_off, A.n_reads + 1, (uint64_t)c); active = r >= 0 && r < A.n_reads; }
		if (active) {
			l_query = (int)(A.read_off[r + 1] - A.read_off[r]);
			min_hsp = A.tab[l_query]; active = min_hsp != NO_SW;
		}
		if (active) {
			const cs_seed_t sd = A.cseeds[s];
			int sw = -1; bool run = false;
			int qb = 0, qlen = 0, tlen = 0; int64_t rb = 0;
			if (sd.len < 200) {   // mem_seed_sw (comp_seed.cpp:367-391) as chain_filter.cpp states it
				qb = max(sd.qbeg - 50, 0); const int qe = min(sd.qbeg + sd.len + 50, l_query);
				rb = max((int64_t)sd.rbeg - 50, (int64_t)0); int64_t re = min((int64_t)sd.rbeg + sd.len + 50, l_pac << 1);
				const int64_t mid = (sd.rbeg + sd.rbeg + sd.len) >> 1;
				if (rb < l_pac && l_pac < re) { if (mid < l_pac) re = l_pac; else rb = l_pac; }
				if (!(qe - qb >= 200 || re - rb >= 200)) {
					const bool rev = mid >= l_pac;   // bns_fetch_seq: clip to the contig that holds `mid`, on the strand of `mid`
					const int64_t mid_f = rev ? (l_pac << 1) - 1 - mid : mid;
					int lo = 0, hi = A.n_ctg;
					while (lo < hi) { const int m = (lo + hi) >> 1; if (A.ctg_off[m] <= mid_f) lo = m + 1; else hi = m; }
					const int rid = max(lo - 1, 0);
					int64_t far_b = A.ctg_off[rid], far_e = far_b + A.ctg_len[rid];
					if (rev) { const int64_t tmp = far_b; far_b = (l_pac << 1) - far_e; far_e = (l_pac << 1) - tmp; }
					rb = max(rb, far_b); re = min(re, far_e);
					tlen = (int)max(re - rb, (int64_t)0); qlen = qe - qb; run = true;
				}
			}
			if (run) {
				sw = 0;
				if (qlen > 0 && tlen > 0) {   // striped_sw_score of chain_filter.cpp: H in place behind a carried diagonal, E beside it
					const uint8_t *q = A.bases + A.read_off[r] + (uint64_t)qb;
					for (int j = 0; j < qlen; ++j) {
						qs[j * 64 + lane] = cs_base_code_(q[j]);
						he[j * 64 + lane] = 0;
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
							const uint32_t x = he[j * 64 + lane];
							const int h_old = (int)(x & 0xffffu); int e = (int)(x >> 16);
							int h = diag + sc_mat(o, tb, qs[j * 64 + lane]);
							h = max(h, e); h = max(h, f);
							diag = h_old; rowmax = max(rowmax, h);
							e = max(max(e - o.e_del, 0), max(h - oe_del, 0));
							f = max(max(f - o.e_ins, 0), max(h - oe_ins, 0));
							he[j * 64 + lane] = (uint32_t)h | ((uint32_t)e << 16);
						}
						f = 0;
						for (int j = 0; j < qlen; ++j) {   // the lazy-F loop: insertions that cross segment boundaries reach H, not E
							const uint32_t x = he[j * 64 + lane];
							const int h = max((int)(x & 0xffffu), f);
							he[j * 64 + lane] = (x & 0xffff0000u) | (uint32_t)h;
							f = max(max(f - o.e_ins, 0), max(h - oe_ins, 0));
						}
						best = max(best, rowmax);
					}
					sw = best;
				}
			}
			if (!(sw < 0 || sw >= min_hsp)) {   // a short seed in a poor neighbourhood: dropped
				A.sscore[s] = DROPPED;
				atomicAdd((unsigned long long *)A.nsd + r, ~0ull);
				atomicSub(A.cns + c, 1);
			} else A.sscore[s] = sw < 0 ? sd.len * o.a : sw;
			if (run) atomicAdd(A.ctr + 5, 1ull);
		}
	}
}

__global__ void __launch_bounds__(256) compact_kernel(Args A)
{
	const int64_t n = A.n_reads;
	for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
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
}
} // namespace csf

namespace {
enum { B_CTG_OFF, B_CTG_LEN, B_PAC, B_TAB, B_W, B_CB, B_CE, B_CNS, B_KFLAG, B_SRT, B_SPAN, B_KI, B_KFIRST, B_ALT, B_KEPTV, B_ORD, B_SSCORE, B_NCH, B_NSD, B_WAVE,
       B_CTR, B_SCAN, B_O_CHAIN_OFF, B_SBASE, B_O_CSEED_OFF, B_O_CHAINS, B_O_CSEEDS, B_O_SCORE,
       B_IN_CHAIN_OFF, B_IN_CHAINS, B_IN_CSEED_OFF, B_IN_CSEEDS, B_IN_BASES, B_IN_READ_OFF, B_COUNT };   // B_IN_*: cs_chain_filter_gpu's uploads
} // namespace

struct cs_chainer_flt_gpu : cs_dev_stage<B_COUNT> {
	int n_ctg = 0; cs_flt_stats_t st = {};
	bool tab_uploaded = false, have_pac = false; int32_t tab_a = 0, tab_mcw = 0; std::vector<int32_t> tab;
	std::vector<cs_chain_t> h_chains; std::vector<uint64_t> h_chain_off, h_cseed_off; std::vector<cs_seed_t> h_cseeds; std::vector<int32_t> h_score;   // cs_chain_filter_gpu's result
};

void cs_chainer_flt_gpu_release_(cs_chainer_flt_gpu *g)
{
	if (!g) return;
	g->release();
	delete g;
}

namespace {
int flt_init(cs_chainer *c)
{
	if (c->flt) return CS_OK;
	cs_chainer_flt_gpu *g = new cs_chainer_flt_gpu();
	if (int rc = g->init(cs_chainer_gpu_device_(c->gpu), true)) { cs_chainer_flt_gpu_release_(g); return rc; }
	c->flt = g;   // (released with the chainer, whatever fails below)
	const cs_refseq_view &R = c->ref;   // contig offsets and lengths, once
	g->n_ctg = (int)R.offset.size();
	if (int rc = g->ensure(B_CTG_OFF, R.offset.size() * 8 + 8)) return rc;
	if (int rc = g->ensure(B_CTG_LEN, R.len.size() * 4 + 4)) return rc;
	HIP_TRY(hipMemcpy(g->b[B_CTG_OFF].p, R.offset.data(), R.offset.size() * 8, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(g->b[B_CTG_LEN].p, R.len.data(), R.len.size() * 4, hipMemcpyHostToDevice));
	return CS_OK;
}

// min_hsp and the seed_sw decision per read length, with the very expressions of filter_range (chain_filter.cpp): the device's log is not
// asked.  Rebuilt when a or min_chain_weight change.
void build_table(cs_chainer_flt_gpu &G, const cs_flt_params_t &o)
{
	if (!G.tab.empty() && G.tab_a == o.a && G.tab_mcw == o.min_chain_weight) return;
	G.tab.resize((size_t)csf::MAX_READ_LEN);
	for (int l_query = 0; l_query < (int)csf::MAX_READ_LEN; ++l_query) {
		const double min_l = o.min_chain_weight ? 1.1f * (float)o.min_chain_weight : 5.5f * std::log((double)l_query);   // MEM_HSP_COEF, MEM_MINSC_COEF
		const bool seed_sw = !(min_l > 0.05f * (float)l_query) && l_query > 0;                                          // MEM_SEEDSW_COEF
		G.tab[(size_t)l_query] = seed_sw ? ((l_query > 0 || o.min_chain_weight) ? (int)(o.a * min_l + .499) : 0) : csf::NO_SW;
	}
	G.tab_uploaded = false; G.tab_a = o.a; G.tab_mcw = o.min_chain_weight;   // (filter_device_ uploads it)
}

int check_call(const char *what, cs_chainer_t *c, const cs_flt_params_t *par, const cs_chain_result_t *in, const uint64_t *read_offsets, uint32_t flags, const cs_chain_result_t *out)
{
	if (!c || !par || !in || !out) return cs_fail_(CS_EINVAL, std::string(what) + ": null argument");
	if (!c->gpu) return cs_fail_(CS_EINVAL, std::string(what) + ": this chainer has no device (create it with cs_chainer_create_device)");
	if (flags & ~CS_FLT_WAVE_ONLY) return cs_fail_(CS_EINVAL, std::string(what) + ": unknown flags");
	if (in->n_reads < 0 || (in->n_reads > 0 && (!in->chain_off || !read_offsets)) || (in->n_chains > 0 && (!in->chains || !in->cseed_off)) || (in->n_seeds > 0 && !in->cseeds))
		return cs_fail_(CS_EINVAL, std::string(what) + ": bad argument");
	if (par->a < 1 || par->b < 0 || par->e_del < 1 || par->e_ins < 1 || par->o_del < 0 || par->o_ins < 0 || par->max_chain_extend < 1) return cs_fail_(CS_EINVAL, std::string(what) + ": bad parameters");
	if (in->n_reads >= 0xffffffffll || in->n_chains >= 0x7fffffffull) return cs_fail_(CS_ERANGE, std::string(what) + ": more than 2^32 reads or 2^31 chains in one call");
	return CS_OK;
}

// both filters over a device-resident batch; the result stays in the filter state's device buffers
int filter_device_(cs_chainer *c, const cs_flt_params_t &o, const cs_chain_result_t &in, const uint8_t *d_bases, const uint64_t *d_ro, uint32_t flags, cs_chain_result_t &out,
                   const int32_t **d_score)
{
	if (int rc = flt_init(c)) return rc;
	cs_chainer_flt_gpu &G = *c->flt;
	constexpr int N_CTR = cs_chainer_flt_gpu::N_CTR;
	HIP_TRY(hipSetDevice(G.device));
	hipStream_t s = G.s;
	const int64_t n = in.n_reads;
	const uint64_t nc = in.n_chains, ns = in.n_seeds;
	if (nc && in.chains == G.at<cs_chain_t>(B_O_CHAINS)) return cs_fail_(CS_EINVAL, "cs_chain_filter_device: the input is this function's own previous output");
	const size_t per_chain = (size_t)nc + 1, per_seed = (size_t)ns + 1, per_read = (size_t)n + 1;
	struct { int which; size_t bytes; } need[] = {
		{B_TAB, (size_t)csf::MAX_READ_LEN * 4}, {B_W, per_chain * 4}, {B_CB, per_chain * 4}, {B_CE, per_chain * 4}, {B_CNS, per_chain * 4}, {B_KFLAG, per_chain},
		{B_SRT, per_chain * sizeof(csf::WRec)}, {B_SPAN, per_chain * sizeof(int2)}, {B_KI, per_chain * 4}, {B_KFIRST, per_chain * 4}, {B_ALT, per_chain}, {B_KEPTV, per_chain},
		{B_ORD, per_chain * 4}, {B_NCH, per_read * 8}, {B_NSD, per_read * 8}, {B_WAVE, per_read * 4}, {B_CTR, N_CTR * 8},
		{B_O_CHAIN_OFF, per_read * 8}, {B_SBASE, per_read * 8}, {B_O_CSEED_OFF, per_chain * 8}, {B_O_CHAINS, per_chain * sizeof(cs_chain_t)},
		{B_O_CSEEDS, per_seed * sizeof(cs_seed_t)}, {B_O_SCORE, per_seed * 4}};
	for (auto &q : need) if (int rc = G.ensure(q.which, q.bytes)) return rc;
	build_table(G, o);
	if (!G.tab_uploaded) { HIP_TRY(hipMemcpy(G.b[B_TAB].p, G.tab.data(), (size_t)csf::MAX_READ_LEN * 4, hipMemcpyHostToDevice)); G.tab_uploaded = true; }
	csf::Args A;
	A.chain_off = in.chain_off; A.cseed_off = in.cseed_off; A.read_off = d_ro; A.chains = in.chains; A.cseeds = in.cseeds; A.bases = d_bases;
	A.n_reads = n; A.n_chains = nc; A.n_seeds = ns; A.flags = flags; A.o = o;
	A.l_pac = c->ref.l_pac; A.ctg_off = G.at<int64_t>(B_CTG_OFF); A.ctg_len = G.at<int32_t>(B_CTG_LEN); A.n_ctg = G.n_ctg; A.pac = G.at<uint8_t>(B_PAC);
	A.tab = G.at<int32_t>(B_TAB);
	A.w = G.at<int32_t>(B_W); A.cb = G.at<int32_t>(B_CB); A.ce = G.at<int32_t>(B_CE); A.cns = G.at<int32_t>(B_CNS); A.kflag = G.at<uint8_t>(B_KFLAG);
	A.srt = G.at<csf::WRec>(B_SRT); A.span = G.at<int2>(B_SPAN); A.ki = G.at<int32_t>(B_KI); A.kfirst = G.at<int32_t>(B_KFIRST);
	A.alt = G.at<uint8_t>(B_ALT); A.keptv = G.at<uint8_t>(B_KEPTV); A.ord = G.at<uint32_t>(B_ORD); A.sscore = nullptr;
	A.nch = G.at<uint64_t>(B_NCH); A.nsd = G.at<uint64_t>(B_NSD); A.wave_list = G.at<uint32_t>(B_WAVE); A.ctr = G.at<unsigned long long>(B_CTR);
	A.o_chain_off = G.at<uint64_t>(B_O_CHAIN_OFF); A.sbase = G.at<uint64_t>(B_SBASE); A.o_cseed_off = G.at<uint64_t>(B_O_CSEED_OFF);
	A.o_chains = G.at<cs_chain_t>(B_O_CHAINS); A.o_cseeds = G.at<cs_seed_t>(B_O_CSEEDS); A.o_score = G.at<int32_t>(B_O_SCORE);
	out.n_reads = n; out.n_chains = 0; out.n_seeds = 0;
	out.chain_off = A.o_chain_off; out.chains = A.o_chains; out.cseed_off = A.o_cseed_off; out.cseeds = A.o_cseeds;
	if (d_score) *d_score = A.o_score;
	if (n == 0) return G.empty_csr(A.o_chain_off, A.o_cseed_off);
	HIP_TRY(hipMemsetAsync(A.ctr, 0, N_CTR * 8, s));
	HIP_TRY(hipMemsetAsync(A.nch + n, 0, 8, s));
	HIP_TRY(hipMemsetAsync(A.nsd + n, 0, 8, s));
	HIP_TRY(hipEventRecord(G.ev[0], s));
	unsigned launches = 1;
	if (nc) { hipLaunchKernelGGL(csf::weight_kernel, G.grid((int64_t)nc, 256), dim3(256), 0, s, A); ++launches; }
	hipLaunchKernelGGL(csf::classify_kernel, G.grid(n, 256), dim3(256), 0, s, A);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(G.ev[1], s));
	HIP_TRY(hipMemcpyAsync(G.h_ctr, A.ctr, N_CTR * 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if (G.h_ctr[2]) return cs_fail_(CS_EINVAL, "cs_chain_filter_device: a chain without seeds, offsets that are not a CSR, or n_seeds that disagrees with cseed_off");
	if (G.h_ctr[3]) return cs_fail_(CS_ERANGE, "cs_chain_filter_device: a read of 65,536 bases or more");
	const uint64_t n_wave = G.h_ctr[0];
	const bool need_sw = G.h_ctr[4] != 0;
	if (need_sw) {   // the seed test reads the reads and the reference
		if (!d_bases) return cs_fail_(CS_EINVAL, "cs_chain_filter_device: the reads are needed for the seed test of long reads");
		if (!G.have_pac) {
			if (c->pac.empty()) { const int rc = cs_load_pac_(c->prefix.c_str(), c->ref.l_pac, c->pac); if (rc != CS_OK) { c->pac.clear(); return rc; } }
			if (int rc = G.ensure(B_PAC, c->pac.size())) return rc;
			HIP_TRY(hipMemcpy(G.b[B_PAC].p, c->pac.data(), c->pac.size(), hipMemcpyHostToDevice));
			G.have_pac = true;
		}
		A.pac = G.at<uint8_t>(B_PAC);
		if (int rc = G.ensure(B_SSCORE, per_seed * 4)) return rc;
		A.sscore = G.at<int32_t>(B_SSCORE);
	}
	HIP_TRY(hipEventRecord(G.ev[2], s));
	if (!(flags & CS_FLT_WAVE_ONLY)) { hipLaunchKernelGGL(csf::light_kernel, G.grid(n, 256), dim3(256), 0, s, A); ++launches; }
	if (n_wave) { hipLaunchKernelGGL(csf::wave_kernel, dim3((unsigned)std::min<uint64_t>(n_wave, (uint64_t)G.n_cu * 12)), dim3(64), 0, s, A); ++launches; }
	if (need_sw && ns) {
		hipLaunchKernelGGL(csf::sw_kernel, dim3((unsigned)std::min<uint64_t>((ns + 63) / 64, (uint64_t)G.n_cu * 64)), dim3(64), 0, s, A);
		++launches;
	}
	HIP_TRY(hipGetLastError());
	// chain_off and the per-read seed bases: exclusive scans over n + 1 counts (the last one 0: the totals)
	if (int rc = G.scan<uint64_t>(B_SCAN, A.nch, A.o_chain_off, A.nsd, A.sbase, (size_t)n + 1, 0)) return rc;
	hipLaunchKernelGGL(csf::compact_kernel, G.grid(n, 256), dim3(256), 0, s, A);
	HIP_TRY(hipGetLastError());
	launches += 3;
	HIP_TRY(hipEventRecord(G.ev[3], s));
	HIP_TRY(hipMemcpyAsync(G.h_ctr, A.o_chain_off + n, 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(G.h_ctr + 2, A.sbase + n, 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(G.h_ctr + 1, A.ctr + 1, 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(G.h_ctr + 5, A.ctr + 5, 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	out.n_chains = G.h_ctr[0]; out.n_seeds = G.h_ctr[2];
	G.add_kernel_ms(G.st.kernel_ms);
	G.st.reads += (uint64_t)n; G.st.chains_in += nc; G.st.chains_out += out.n_chains; G.st.seeds_in += ns; G.st.seeds_out += out.n_seeds;
	G.st.wave_reads += n_wave; G.st.spill_reads += G.h_ctr[1]; G.st.sw_seeds += G.h_ctr[5]; G.st.launches += launches;
	return CS_OK;
}
} // namespace

extern "C" int cs_chain_filter_device(cs_chainer_t *c, const cs_flt_params_t *par, const cs_chain_result_t *d_in, const uint8_t *d_bases, const uint64_t *d_read_offsets,
                                      uint32_t flags, cs_chain_result_t *d_out, const int32_t **d_cseed_score)
{
	if (int rc = check_call("cs_chain_filter_device", c, par, d_in, d_read_offsets, flags, d_out)) return rc;
	return filter_device_(c, *par, *d_in, d_bases, d_read_offsets, flags, *d_out, d_cseed_score);
}

extern "C" int cs_chain_filter_gpu(cs_chainer_t *c, const cs_flt_params_t *par, const cs_chain_result_t *in, const uint8_t *bases, const uint64_t *read_offsets, uint32_t flags,
                                   cs_chain_result_t *out, const int32_t **cseed_score)
{
	if (int rc = check_call("cs_chain_filter_gpu", c, par, in, read_offsets, flags, out)) return rc;
	if (int rc = flt_init(c)) return rc;
	cs_chainer_flt_gpu &G = *c->flt;
	HIP_TRY(hipSetDevice(G.device));
	const int64_t n = in->n_reads;
	if (in->n_chains && in->chains == G.h_chains.data()) return cs_fail_(CS_EINVAL, "cs_chain_filter_gpu: the input is this function's own previous output");
	// the reads are uploaded only when some read with chains is long enough for the seed test (the table is the device's own)
	build_table(G, *par);
	bool need_bases = false;
	for (int64_t r = 0; r < n && !need_bases; ++r) {
		const uint64_t l = read_offsets[r + 1] - read_offsets[r];
		need_bases = l < csf::MAX_READ_LEN && in->chain_off[r + 1] > in->chain_off[r] && G.tab[(size_t)l] != csf::NO_SW;
	}
	if (need_bases && !bases) return cs_fail_(CS_EINVAL, "cs_chain_filter_gpu: the reads are needed for the seed test of long reads");
	cs_chain_result_t d = *in;
	if (n > 0) {
		if (int rc = G.up(B_IN_CHAIN_OFF, in->chain_off, ((size_t)n + 1) * 8)) return rc;
		if (int rc = G.up(B_IN_READ_OFF, read_offsets, ((size_t)n + 1) * 8)) return rc;
		if (in->n_chains) {
			if (int rc = G.up(B_IN_CHAINS, in->chains, (size_t)in->n_chains * sizeof(cs_chain_t))) return rc;
			if (int rc = G.up(B_IN_CSEED_OFF, in->cseed_off, ((size_t)in->n_chains + 1) * 8)) return rc;
		}
		if (in->n_seeds) { if (int rc = G.up(B_IN_CSEEDS, in->cseeds, (size_t)in->n_seeds * sizeof(cs_seed_t))) return rc; }
		if (need_bases) { if (int rc = G.up(B_IN_BASES, bases, (size_t)read_offsets[n])) return rc; }
		HIP_TRY(hipStreamSynchronize(G.s));
		d.chain_off = G.at<uint64_t>(B_IN_CHAIN_OFF); d.chains = G.at<cs_chain_t>(B_IN_CHAINS);
		d.cseed_off = G.at<uint64_t>(B_IN_CSEED_OFF); d.cseeds = G.at<cs_seed_t>(B_IN_CSEEDS);
	}
	cs_chain_result_t dr; const int32_t *d_sc = nullptr;
	if (int rc = filter_device_(c, *par, d, need_bases ? G.at<uint8_t>(B_IN_BASES) : nullptr, n > 0 ? G.at<uint64_t>(B_IN_READ_OFF) : nullptr, flags, dr, &d_sc)) return rc;
	if (int rc = cs_download_chains_(G.s, dr, d_sc, G.h_chain_off, G.h_chains, G.h_cseed_off, G.h_cseeds, &G.h_score, out)) return rc;
	if (cseed_score) *cseed_score = G.h_score.data();
	return CS_OK;
}

extern "C" int cs_chain_filter_stats(const cs_chainer_t *c, cs_flt_stats_t *st)
{
	if (!c || !st) return cs_fail_(CS_EINVAL, "cs_chain_filter_stats: null argument");
	if (c->flt) *st = c->flt->st; else memset(st, 0, sizeof *st);
	return CS_OK;
}
