// mark_scan.hpp -- what the reference decides about a read's regions between mem_sort_dedup_patch and mem_reg2aln: mem_mark_primary_se
// (comp_seed.cpp:711-774), mem_approx_mapq_se (:686-709), the selection loop of mem_reg2sam (:1089-1106) and the membership rule of
// mem_gen_alt (:1026-1054), as bodies a device pass (mark_gpu.hip) and a plain C++ program (tests/cpp/mark_scan_check.cpp: W = 1 over the
// goldens, W = 8 / 64 on threads in lockstep) run alike.  The lane primitives are wave_lanes.hpp's.  In the order of the pass:
//   check_read      a lane per read: the offsets are CSR arrays; every region is live and mapped, lies inside its read and inside
//                   [0, 2 l_pac), names a contig of the table and scores >= 0 (C_BAD otherwise); fewer than MAX_REGS regions, each
//                   spanning at most MAX_SPAN bases on either side (C_RANGE otherwise).  The lane compares its own entries BEFORE it
//                   walks [reg_off[r], reg_off[r + 1]); nothing else follows an offset before the host has seen the verdict, and
//                   every later loop's trip count is a region count or a z length that this function bounded by MAX_REGS.
//   mark_read<W>    W lanes per read over the read's Work lists (n entries each: lane-private, LDS, or HBM scratch):
//                   the sort by alnreg_hlt, mem_mark_primary_se_core, secondary_all / alt_sc and the ALT branch.
//                   alnreg_hlt and alnreg_hlt2 (comp_seed.cpp:590-593) are strict total orders -- hash_64 is a bijection and a read's
//                   ids differ -- so ANY correct sort gives the reference's order: the first sort is a rank sort (an entry's rank is
//                   the number of entries before it, n^2 / W compares, no exchange between lanes), and the second one is the stable
//                   partition of the first order by is_alt, which is what alnreg_hlt2 asks of a list that alnreg_hlt has sorted.
//                   In the core the i loop is sequential (z grows); the k loop tests W entries of z per step and takes the first hit
//                   by ballot; only that j gets sub / sub_n written.
//   mapq_of         mem_approx_mapq_se for mapQ_coef_len > 0, in double as the reference has it; the three logarithms come from a table
//                   of the host's std::log(k), k in [0, LOG_N), so that no device libm stands before (int)(x + .499)
//   select_read<W>  per region in rank order: its cs_mark_t (line, flag, MAPQ with the supplementary cap, XS, xa_of), the region itself
//                   in rank order (the CIGAR stage's input before compaction) and need_cigar; per read the number of lines.  The
//                   per-region part is spread over the lanes; the part that carries state along the ranks (the line counter, the first
//                   line's MAPQ, mem_gen_alt's counts) is one lane's, n steps.
// No body waits for another lane's memory except through the wave's own barrier (wsync).  Float and double expressions are the
// reference's, operand for operand; the units that include this are compiled with -ffp-contract=off.
#pragma once
#include "wave_lanes.hpp"

#include <climits>

namespace csmk {
using csdd::lanes_below; using csdd::wballot; using csdd::wsync;
constexpr uint64_t MAX_REGS = 65536;                                   // a read has fewer regions than this: ranks and z fit 16 bits, 2 sub_n + 1 < LOG_N
constexpr int64_t MAX_SPAN = 131072;                                   // mem_approx_mapq_se's l is at most this
constexpr int LOG_N = 131073;                                          // the table of logarithms: k in [0, LOG_N)
enum { V_OK = 0, V_BAD = 1, V_RANGE = 2 };                             // check_read's verdict

struct In { const uint64_t *reg_off, *read_off; const cs_alnreg_t *regs; int64_t n_reads; uint64_t n_regs; };
struct Ref { int64_t l_pac; const uint8_t *ctg_alt; int n_ctg; const double *logtab; };   // ctg_alt: bntann1_t.is_alt per contig
struct Par { cs_mark_params_t p; int a, b, o_del, e_del, o_ins, e_ins; uint32_t flags; int64_t id_base; };
// a read's lists, n entries each.  key: input order, (score << 1 | !is_alt); ord: rank -> input index; rk: key in rank order;
// key doubles as the old -> new position map and z as the staging list of the ALT branch's reordering
struct Work { uint32_t *key, *rk; int32_t *ord, *qb, *qe, *z, *sec, *sall, *sub, *subn; };
constexpr int WORK_LISTS = 10;
CS_HD inline Work work_at(int32_t *base, uint64_t stride, uint64_t at)   // ten lists of `stride` entries, this read's part at `at`
{
	int32_t *p = base + at;
	const Work w = {(uint32_t *)p, (uint32_t *)(p + stride), p + 2 * stride, p + 3 * stride, p + 4 * stride, p + 5 * stride, p + 6 * stride, p + 7 * stride, p + 8 * stride, p + 9 * stride};
	return w;
}

CS_HD inline int check_read(const In &D, const Ref &R, int64_t r)
{
	const uint64_t c0 = D.reg_off[r], c1 = D.reg_off[r + 1], b0 = D.read_off[r], b1 = D.read_off[r + 1];
	if (c1 < c0 || c1 > D.n_regs || b1 < b0 || (r == 0 && (b0 != 0 || c0 != 0)) || (r == D.n_reads - 1 && c1 != D.n_regs)) return V_BAD;
	if (c1 - c0 >= MAX_REGS) return V_RANGE;
	const uint64_t l = b1 - b0;
	int v = V_OK;
	for (uint64_t g = c0; g < c1; ++g) {                              // (c0 <= c1 <= n_regs: inside the array)
		const cs_alnreg_t x = D.regs[g];
		if (x.qb < 0 || x.qe <= x.qb || (uint64_t)x.qe > l || x.rb < 0 || x.re <= x.rb || x.re > (R.l_pac << 1) || x.rid < 0 || x.rid >= R.n_ctg || x.score < 0) return V_BAD;
		if (x.qe - x.qb > MAX_SPAN || x.re - x.rb > MAX_SPAN) v = V_RANGE;
	}
	return v;
}

CS_HD inline uint64_t hash_64(uint64_t key)                               // bwalib/utils.h:99-110
{
	key += ~(key << 32); key ^= key >> 22; key += ~(key << 13); key ^= key >> 8;
	key += key << 3; key ^= key >> 15; key += ~(key << 27); key ^= key >> 31;
	return key;
}
CS_HD inline int rk_score(uint32_t k) { return (int)(k >> 1); }
CS_HD inline int rk_alt(uint32_t k) { return (int)(~k & 1u); }

// mem_mark_primary_se_core over the first m entries in their current order.  sub_n is not reset: the second pass of the ALT branch adds to it.
template <int W> CS_HD inline void mark_core(const Par &P, int m, const Work &K, int lane)
{
	int tmp = P.a + P.b;
	tmp = P.o_del + P.e_del > tmp ? P.o_del + P.e_del : tmp;
	tmp = P.o_ins + P.e_ins > tmp ? P.o_ins + P.e_ins : tmp;
	int zn = 1;                                                       // (m >= 1)
	if (lane == 0) K.z[0] = 0;
	wsync<W>();
	for (int i = 1; i < m; ++i) {
		const int qbi = K.qb[i], qei = K.qe[i], sci = rk_score(K.rk[i]), alti = rk_alt(K.rk[i]);
		int hit = -1;
		for (int k0 = 0; k0 < zn; k0 += W) {                           // (zn <= i < m < MAX_REGS)
			const int k = k0 + lane;
			bool ok = false;
			if (k < zn) {
				const int j = K.z[k];
				const int b_max = K.qb[j] > qbi ? K.qb[j] : qbi, e_min = K.qe[j] < qei ? K.qe[j] : qei;
				if (e_min > b_max) {
					const int min_l = qei - qbi < K.qe[j] - K.qb[j] ? qei - qbi : K.qe[j] - K.qb[j];
					ok = e_min - b_max >= min_l * P.p.mask_level;
				}
			}
			const uint64_t mk = wballot<W>(ok);
			if (mk) { hit = k0 + __builtin_ctzll(mk); break; }
		}
		if (lane == 0) {
			if (hit < 0) K.z[zn] = i;
			else {
				const int j = K.z[hit];
				if (K.sub[j] == 0) K.sub[j] = sci;
				if (rk_score(K.rk[j]) - sci <= tmp && (rk_alt(K.rk[j]) || !alti)) ++K.subn[j];
				K.sec[i] = j;
			}
		}
		if (hit < 0) ++zn;
		wsync<W>();
	}
}

// mem_mark_primary_se for the read's n >= 1 regions x[0, n); id: the read's number (id_base + read).  Returns n_pri.
// Afterwards, per final rank p: ord[p] the region, rk[p] its score and is_alt, sec / sall / sub / subn[p] the reference's fields.
template <int W> CS_HD inline int mark_read(const Par &P, const Ref &R, const cs_alnreg_t *x, int n, uint64_t id, const Work &K, int lane)
{
	for (int i = lane; i < n; i += W) K.key[i] = (uint32_t)x[i].score << 1 | (R.ctg_alt[x[i].rid] ? 0u : 1u);
	wsync<W>();
	// the sort by alnreg_hlt: the greater key first, the smaller hash among equal keys
	for (int i = lane; i < n; i += W) {
		const uint32_t ki = K.key[i];
		const uint64_t hi = hash_64(id + (uint64_t)i);
		int rank = 0;
		for (int j = 0; j < n; ++j) {
			const uint32_t kj = K.key[j];
			if (kj > ki || (kj == ki && j != i && hash_64(id + (uint64_t)j) < hi)) ++rank;
		}
		K.ord[rank] = i;
	}
	wsync<W>();
	int n_pri = 0;
	for (int p = lane; p < n; p += W) {
		const cs_alnreg_t &y = x[K.ord[p]];
		K.rk[p] = K.key[K.ord[p]]; K.qb[p] = y.qb; K.qe[p] = y.qe; K.sec[p] = -1; K.sub[p] = 0; K.subn[p] = 0;
	}
	wsync<W>();
	for (int p0 = 0; p0 < n; p0 += W) n_pri += (int)csdd::wcount(wballot<W>(p0 + lane < n && !rk_alt(K.rk[p0 + lane])));
	mark_core<W>(P, n, K, lane);
	if (n_pri == n) {
		for (int p = lane; p < n; p += W) K.sall[p] = K.sec[p];
		wsync<W>();
		return n_pri;
	}
	// the ALT branch (comp_seed.cpp:754-768).  key[old rank] = the position after the sort by alnreg_hlt2: the entries off the ALT contigs
	// first, either group in the order it has
	int pri = 0;
	for (int p0 = 0; p0 < n; p0 += W) {
		const int p = p0 + lane;
		const bool in = p < n, alt = in && rk_alt(K.rk[p]);
		const uint64_t mp = wballot<W>(in && !alt), ma = wballot<W>(alt);
		if (in) K.key[p] = n_pri > 0 ? (uint32_t)(alt ? n_pri + (p0 - pri) + (int)csdd::wcount(ma & lanes_below(lane)) : pri + (int)csdd::wcount(mp & lanes_below(lane))) : (uint32_t)p;
		pri += (int)csdd::wcount(mp);
	}
	wsync<W>();
	for (int p = lane; p < n; p += W) {                               // (by old rank; the lists move below)
		const int s = K.sec[p];
		K.sall[p] = s >= 0 ? (int32_t)K.key[s] : -1;
		if (s >= 0 && rk_alt(K.rk[p])) K.sec[p] = INT_MAX;
	}
	wsync<W>();
	if (n_pri > 0) {
		int32_t *const lists[7] = {K.ord, (int32_t *)K.rk, K.qb, K.qe, K.sec, K.sall, K.sub};
		for (int t = 0; t < 8; ++t) {                                 // every list to its new order, staged in z
			int32_t *const a = t < 7 ? lists[t] : K.subn;
			for (int p = lane; p < n; p += W) K.z[K.key[p]] = a[p];
			wsync<W>();
			for (int p = lane; p < n; p += W) a[p] = K.z[p];
			wsync<W>();
		}
		for (int p = lane; p < n_pri; p += W) { K.sub[p] = 0; K.sec[p] = -1; }
		wsync<W>();
		mark_core<W>(P, n_pri, K, lane);
	}
	return n_pri;
}

// mem_approx_mapq_se (csub is 0 in this reference: only ever merged from zero-initialised regions)
CS_HD inline int mapq_of(const Par &P, const Ref &R, const cs_alnreg_t &x, int sub_, int sub_n)
{
	const int sub = sub_ ? sub_ : P.p.min_seed_len * P.a;
	if (sub >= x.score) return 0;
	const int l = x.qe - x.qb > (int)(x.re - x.rb) ? x.qe - x.qb : (int)(x.re - x.rb);
	const double identity = 1. - (double)(l * P.a - x.score) / (P.a + P.b) / l;
	int mapq;
	if (x.score == 0) mapq = 0;
	else {
		// mem_opt_t keeps mapQ_coef_fac = log(mapQ_coef_len) in an int (comp_seed.h:68): 3 for the default 50, and that is what divides
		double tmp = l < P.p.mapq_coef_len ? 1. : (int)R.logtab[P.p.mapq_coef_len] / R.logtab[l];
		tmp *= identity * identity;
		mapq = (int)(6.02 * (x.score - sub) / P.a * tmp * tmp + .499);
	}
	if (sub_n > 0) mapq -= (int)(4.343 * R.logtab[sub_n + 1] + .499);
	if (mapq > 60) mapq = 60;
	if (mapq < 0) mapq = 0;
	return (int)(mapq * (1. - x.frac_rep) + .499);
}

// After mark_read (n >= 1): the read's marks m[0, n) and its regions in rank order ranked[0, n), need[0, n) = "the CIGAR stage wants it";
// returns the number of lines; *n_xa: the regions with xa_of >= 0.
template <int W> CS_HD inline int select_read(const Par &P, const Ref &R, const cs_alnreg_t *x, int n, const Work &K, cs_mark_t *m, cs_alnreg_t *ranked, uint32_t *need, int *n_xa, int lane)
{
	const bool all = (P.flags & CS_MARK_ALL) != 0;
	for (int p = lane; p < n; p += W) {
		const cs_alnreg_t y = x[K.ord[p]];
		const int sec = K.sec[p], sa = K.sall[p], alt = rk_alt(K.rk[p]);
		cs_mark_t o;
		o.reg = K.ord[p]; o.is_alt = alt; o.secondary = sec; o.secondary_all = sa; o.sub = K.sub[p]; o.sub_n = K.subn[p];
		o.alt_sc = !alt && sa >= 0 && rk_alt(K.rk[sa]) ? rk_score(K.rk[sa]) : 0;   // (the first round's secondary, where it stands now)
		bool line = y.score >= P.p.T && !(sec >= 0 && (alt || !all));   // comp_seed.cpp:1092-1094
		if (line && sec >= 0 && sec < INT_MAX && y.score < rk_score(K.rk[sec]) * P.p.drop_ratio) line = false;
		o.line = line ? 0 : -1;
		o.mapq = sec < 0 ? mapq_of(P, R, y, o.sub, o.sub_n) : 0;
		o.xs = sec < 0 ? o.sub : -1;
		o.flag = (y.rb >= R.l_pac ? 0x10 : 0) | (sec >= 0 ? 0x100 : 0);
		o.xa_of = !all && sa >= 0 && y.score >= rk_score(K.rk[sa]) * (double)P.p.xa_drop_ratio ? sa : -1;   // get_pri_idx
		m[p] = o; ranked[p] = y; K.z[p] = 0;
	}
	wsync<W>();
	int l = 0, xa = 0;
	if (lane == 0) {
		int mapq0 = 0;
		for (int p = 0; p < n; ++p) {
			if (m[p].line < 0) continue;
			if (l && m[p].secondary < 0) m[p].flag |= (P.flags & CS_MARK_NO_MULTI) ? 0x100 : 0x800;
			if (l == 0) mapq0 = m[p].mapq;
			else if (!(P.flags & CS_MARK_KEEP_SUPP_MAPQ) && !m[p].is_alt && m[p].mapq > mapq0) m[p].mapq = mapq0;
			m[p].line = l++;
		}
		// mem_gen_alt: z[r] = members of r's list, bit 30 = an ALT one among them (n < MAX_REGS)
		if (!all) {
			for (int p = 0; p < n; ++p) if (m[p].xa_of >= 0) K.z[m[p].xa_of] = (K.z[m[p].xa_of] + 1) | (m[p].is_alt ? 1 << 30 : 0);
			for (int p = 0; p < n; ++p) {
				if (m[p].xa_of < 0) continue;
				const int c = K.z[m[p].xa_of] & ~(1 << 30), has_alt = K.z[m[p].xa_of] >> 30;
				if (c > P.p.max_xa_hits_alt || (!has_alt && c > P.p.max_xa_hits)) m[p].xa_of = -1; else ++xa;
			}
		}
		for (int p = 0; p < n; ++p) need[p] = m[p].line >= 0 || m[p].xa_of >= 0 ? 1u : 0u;   // need_cigar
	}
	wsync<W>();
	*n_xa = xa;
	return l;                                                         // (lane 0's; the other lanes' values are not used)
}
} // namespace csmk
