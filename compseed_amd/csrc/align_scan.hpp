// align_scan.hpp -- the extension stage, mem_chain2aln_across_reads_V2 (mapping/comp_seed.cpp:1319-2237), as bodies that the kernels of
// align_gpu.hip and a plain C++ program (tests/cpp/align_scan_check.cpp: W = 1 over the goldens, W = 8 / 64 on threads in lockstep) run
// alike, each indexed by read, base, chain, pair, region or lane.  No body does an atomic or appends to a list: where one has something
// to count, to refuse or to send on it returns a count or a verdict, and where a wave needs slots it asks a callable of the caller's; the
// kernel (or the program's loop) does the rest.  The lanes are wave_lanes.hpp's.  In the order of the pass:
//   check_read, check_chain   cs_extend_chains_device only: a lane reads its own two entries of an offset array and compares them with each
//                    other and with the host's counts (true: refused).  Nothing below runs on input that any read or chain refused.
//   chain_read       a read: its number into the slots of its chains
//   read_of_base, query_codes   a base: its read by a search in the offsets; its code into the forward and the reversed copy of the read
//   chain_window     a chain: the reference window its seeds can reach with the gap they can afford (affordable_gap = cal_max_gap), clipped
//                    to the strand and to the contig of the first seed (bns_fetch_seq) -> w0, 2 x length; false: that seed lies outside
//                    the reference.  An exclusive sum of the caller's gives every window its place.
//   fill_window<W>   a chain by W lanes: the window's bases from the packed reference, forward and reversed
//   seed_rank, chain_ctx, emit_region   a seed's place in the order of extension; what a chain's regions share; one region and its (at
//                    most two) pairs at the slots the caller reserved
//   count_pairs, emit_chain   a chain of up to SMALL_CHAIN seeds by one lane: how many pairs each side gets; its regions from its slot bases
//   chain_regions<W> a longer chain by W lanes, W seeds at a time; `reserve(counter, n)` is called by lane 0 and returns the first of n slots
//   apply_result     a pair's extension into its region: clipped or to the end of the read, truesc, the band used; true: the band may
//                    have cut the alignment and a try is left, the pair goes on the retry list (the band-retry rule, MAX_BAND_TRY 2).
//                    The region is the caller's copy, loaded before and stored after the append, as apply_kernel always did it.
//   right_h0         a right pair starts from the score the left side reached
//   seed_coverage    a region: the chain's seeds that lie inside it on both axes
//   purge_around, purge_rival, purge_load   the two tests of the redundancy purge (comp_seed.cpp:2141-2232) and a region as they read it
//   purge_read_regs<W>   a read of at most W regions by W lanes: a region per lane, which ones are still there is a mask
//   purge_read_mem<W>    a read of any size by W lanes: flags in memory, W earlier regions per step; with one lane the reference's loop
// Both purge walks add the number purged to lane 0's accumulator.  purge_big_kernel, the third walk (a workgroup of eight waves per
// read, the read staged in LDS, a double-buffered vote per step), stays in align_gpu.hip and is NOT run on the CPU: the lockstep lanes stand for one wave, not
// for waves that meet at a workgroup barrier with LDS between them.  It is built from purge_around, purge_rival and purge_load, and
// hands the reads beyond its LDS to purge_read_mem<64>; the GPU tests hold it against the same goldens (flags 0 and 1 against 2 and 3).
// The arithmetic is the host driver's that these kernels replaced, operand for operand: the divisions of affordable_gap are in double
// precision, as are .1 * l_query and * .95; the units that include this are compiled without fast-math and with -ffp-contract=off.
#pragma once
#include "cs_internal.hpp"
#include "wave_lanes.hpp"

#include <cstring>

namespace csa {
constexpr int32_t UNSET = -99;            // the reference's H0_ (mapping/macro.h:44): a coordinate that has not been set yet
constexpr int SMALL_CHAIN = 8;            // chains of up to this many seeds (nearly all) are a lane's
constexpr int PURGE_CAP = 3000, PURGE_GAPS = 1024;   // purge_big_kernel: regions of a read that fit its LDS; entries of its table of affordable gaps
constexpr uint64_t MAX_READ_LEN = 65536;

// The counter words: pairs on the left / right list, pairs sent back for the wider band, chains whose first seed lies outside the reference,
// purged regions, chains on the list of region_big_kernel, reads on the list of purge_big_kernel and that kernel's ticket.  Two words serve
// twice in cs_extend_chains_device: its checks count into the first two before the core clears the block, and the long chains' count has
// served when the compaction writes the number of live regions in its place.
enum { C_LEFT, C_RIGHT, C_RETRY, C_BAD_CHAIN, C_PURGED, C_BIG_CHAINS, C_BIG_READS, C_TICKET, C_COUNT,
       C_REFUSED = C_LEFT, C_N_BASES = C_RIGHT, C_LIVE = C_BIG_CHAINS };

struct Args {
	const uint64_t *chain_off, *cseed_off, *read_off; const cs_chain_t *chains; const cs_seed_t *cseeds; const int32_t *score; const uint8_t *bases;
	int64_t n_reads, n_chains, n_seeds, l_pac; uint64_t n_bases;
	const uint8_t *pac; const int64_t *ctg_off; const int32_t *ctg_len; int32_t n_ctg;
	cs_aln_params_t o;
	uint32_t *chain_read; int64_t *w0; uint64_t *wlen2, *tb0;   // per chain: window start, 2 x length (scanned into tb0)
	uint8_t *qbuf, *tbuf; uint32_t *ord; cs_alnreg_t *regs; uint32_t *reg_ci;
	cs_ext_pair_t *lp, *rp;
	int32_t small_chain, light_max, purge_cap;   // SMALL_CHAIN / 64 / PURGE_CAP unless cs_aln_params_t.flags says otherwise (A/B tests)
	uint32_t *big, *big_reads;             // chains of more than SMALL_CHAIN seeds / reads of more than 64 regions: lists for the *_big kernels
	unsigned long long *ctr;               // the C_* words
};

// ---- cs_extend_chains_device.  The caller's arrays are device memory that no host loop has seen, so what cs_extend_chains' host loops
// refuse is counted by two bodies that follow no offset themselves.  Beyond the host's conditions: read_off starts at 0 and does not
// decrease (read_of_base's search and read lengths rest on it), a read with chains is shorter than MAX_READ_LEN, and both offset arrays
// run from 0 to their count -- a chain no read owns has no chain_read entry, a seed no chain owns no region, and the bodies below read both.
struct DevIn { const uint64_t *chain_off, *cseed_off, *read_off; const cs_chain_t *chains; int64_t n_reads; uint64_t n_chains, n_seeds; };
CS_HD inline bool check_read(const DevIn &D, int64_t r)
{
	const uint64_t c0 = D.chain_off[r], c1 = D.chain_off[r + 1], b0 = D.read_off[r], b1 = D.read_off[r + 1];
	return c1 < c0 || c1 > D.n_chains || b1 < b0 || (r == 0 && (b0 != 0 || c0 != 0)) || (r == D.n_reads - 1 && c1 != D.n_chains) || (c1 > c0 && b1 - b0 >= MAX_READ_LEN);
}
CS_HD inline bool check_chain(const DevIn &D, uint64_t c)
{
	const uint64_t s0 = D.cseed_off[c], s1 = D.cseed_off[c + 1];
	return s1 < s0 || s1 > D.n_seeds || (int64_t)(s1 - s0) != (int64_t)D.chains[c].n_seeds || (c == 0 && s0 != 0) || (c == D.n_chains - 1 && s1 != D.n_seeds);
}

CS_HD inline int affordable_gap(const cs_aln_params_t &o, int qlen) // cal_max_gap (comp_seed.cpp:415-421)
{
	const int l_del = (int)((double)(qlen * o.a - o.o_del) / o.e_del + 1.), l_ins = (int)((double)(qlen * o.a - o.o_ins) / o.e_ins + 1.);
	int l = l_del > l_ins ? l_del : l_ins;
	l = l > 1 ? l : 1;
	return l < (o.w << 1) ? l : (o.w << 1);
}

CS_HD inline void chain_read(const Args &A, int64_t r)
{
	for (uint64_t ci = A.chain_off[r]; ci < A.chain_off[r + 1]; ++ci) A.chain_read[ci] = (uint32_t)r;
}
CS_HD inline int64_t read_of_base(const Args &A, uint64_t b) // binary search in the offsets
{
	int64_t lo = 0, hi = A.n_reads;
	while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (A.read_off[mid] <= b) lo = mid; else hi = mid; }
	return lo;
}
CS_HD inline void query_codes(const Args &A, uint64_t b) // every read as codes, forward and reversed (a left extension reads the reversed prefix, comp_seed.cpp:1525)
{
	const int64_t lo = read_of_base(A, b);
	const uint64_t b0 = A.read_off[lo], len = A.read_off[lo + 1] - b0, j = b - b0;
	const uint8_t c = cs_base_code_(A.bases[b]);
	A.qbuf[b] = c; A.qbuf[A.n_bases + b0 + (len - 1 - j)] = c;
}
CS_HD inline bool chain_window(const Args &A, int64_t ci)
{
	const cs_aln_params_t &o = A.o;
	const cs_seed_t *sd = A.cseeds + A.cseed_off[ci];
	const int ns = (int)(A.cseed_off[ci + 1] - A.cseed_off[ci]);
	A.w0[ci] = 0; A.wlen2[ci] = 0;
	if (ns <= 0) return true;
	const uint32_t r = A.chain_read[ci];
	const int l_query = (int)(A.read_off[r + 1] - A.read_off[r]);
	const int64_t l_pac = A.l_pac;
	int64_t w0 = l_pac << 1, w1 = 0;
	for (int i = 0; i < ns; ++i) {
		const cs_seed_t s = sd[i];
		const int64_t b = s.rbeg - (s.qbeg + affordable_gap(o, s.qbeg));
		const int tail = l_query - s.qbeg - s.len;
		const int64_t e = s.rbeg + s.len + (tail + affordable_gap(o, tail));
		w0 = w0 < b ? w0 : b; w1 = w1 > e ? w1 : e;
	}
	w0 = w0 > 0 ? w0 : 0; w1 = w1 < (l_pac << 1) ? w1 : (l_pac << 1);
	const int64_t mid = sd[0].rbeg;
	if (w0 < l_pac && l_pac < w1) { if (mid < l_pac) w1 = l_pac; else w0 = l_pac; } // never across the strands
	// clip to the contig of the first seed (bns_fetch_seq, bntseq.c:426-451)
	const bool rev = mid >= l_pac;
	const int64_t mid_f = rev ? (l_pac << 1) - 1 - mid : mid;
	int lo = 0, hi = A.n_ctg;                                         // last contig whose offset is <= mid_f
	while (hi - lo > 1) { const int m = (lo + hi) >> 1; if (A.ctg_off[m] <= mid_f) lo = m; else hi = m; }
	if (mid_f < 0 || mid_f >= l_pac || !(w0 <= mid && mid < w1)) return false;
	int64_t far_b = A.ctg_off[lo], far_e = far_b + A.ctg_len[lo];
	if (rev) { const int64_t x = far_b; far_b = (l_pac << 1) - far_e; far_e = (l_pac << 1) - x; }
	w0 = w0 > far_b ? w0 : far_b; w1 = w1 < far_e ? w1 : far_e;
	A.w0[ci] = w0; A.wlen2[ci] = w1 > w0 ? (uint64_t)(w1 - w0) * 2 : 0;
	return true;
}
// the window's bases, forward strand as stored, reverse strand complemented from the mirror position; then reversed
template <int W> CS_HD inline void fill_window(const Args &A, int64_t ci, int lane)
{
	const int64_t L = (int64_t)(A.wlen2[ci] >> 1), w0 = A.w0[ci];
	uint8_t *t = A.tbuf + A.tb0[ci];
	for (int64_t k = lane; k < L; k += W) {
		const int64_t p = w0 + k;
		const uint8_t b = (uint8_t)(p < A.l_pac ? cs_pac_base_(A.pac, p) : 3 - cs_pac_base_(A.pac, (A.l_pac << 1) - 1 - p));
		t[k] = b; t[L + (L - 1 - k)] = b;
	}
}

// ---- regions.  A chain's seeds are extended in the order of their scores, highest first, later ones first among equals (comp_seed.cpp:1406-1411,
// 1440-1458); that order is total, so a seed's place is the number of seeds that rank before it and every seed can be placed on its own.
CS_HD inline int seed_rank(const cs_seed_t *sd, const int32_t *sc, int ns, int i)
{
	const int si = sc ? sc[i] : sd[i].len;
	int rk = 0;
	for (int y = 0; y < ns; ++y) { const int sy = sc ? sc[y] : sd[y].len; rk += (sy > si || (sy == si && y > i)) ? 1 : 0; }
	return rk;
}
struct ChainCtx { int64_t ci, w0, L, tb0; uint64_t s0, rb0; int32_t l_query, rid, chain; float frac_rep; };
CS_HD inline ChainCtx chain_ctx(const Args &A, int64_t ci)
{
	ChainCtx X;
	const cs_chain_t c = A.chains[ci];
	const uint32_t r = A.chain_read[ci];
	X.ci = ci; X.s0 = A.cseed_off[ci]; X.rb0 = A.read_off[r]; X.l_query = (int32_t)(A.read_off[r + 1] - X.rb0);
	X.w0 = A.w0[ci]; X.L = (int64_t)(A.wlen2[ci] >> 1); X.tb0 = (int64_t)A.tb0[ci];
	X.rid = c.rid; X.frac_rep = c.frac_rep; X.chain = (int32_t)(ci - (int64_t)A.chain_off[r]);
	return X;
}
// seed i of the chain, k-th in the order of extension: its region and its (at most two) pairs, at the slots the caller reserved (a pair's
// `reserved` word = its region)
CS_HD inline void emit_region(const Args &A, const ChainCtx &X, const cs_seed_t &s, int i, int k, bool left, bool right, uint64_t lslot, uint64_t rslot)
{
	const cs_aln_params_t &o = A.o;
	const uint64_t g = X.s0 + (uint64_t)k;
	cs_alnreg_t a; memset(&a, 0, sizeof a);
	a.w = o.w; a.score = a.truesc = -1; a.rid = X.rid; a.frac_rep = X.frac_rep; a.seedlen0 = s.len; a.chain = X.chain;
	a.rb = a.re = UNSET; a.qb = a.qe = UNSET;
	if (left) { // reversed read prefix against the reversed window in front of the seed
		const int64_t tl = s.rbeg - X.w0;
		const cs_ext_pair_t p = {(uint64_t)(A.n_bases + X.rb0 + (uint64_t)(X.l_query - s.qbeg)), (uint64_t)(X.tb0 + X.L + (X.L - tl)), s.qbeg, (int32_t)tl, s.len * o.a, (int32_t)g};
		A.lp[lslot] = p;
		a.qb = s.qbeg; a.rb = s.rbeg;
	} else { a.score = a.truesc = s.len * o.a; a.qb = 0; a.rb = s.rbeg; }
	if (right) { // the rest of the read against the window behind the seed
		const int qe = s.qbeg + s.len; const int64_t re = s.rbeg + s.len - X.w0;
		const cs_ext_pair_t p = {(uint64_t)(X.rb0 + (uint64_t)qe), (uint64_t)(X.tb0 + re), X.l_query - qe, (int32_t)(X.L - re), 0, (int32_t)g};
		A.rp[rslot] = p;
		a.qe = qe; a.re = X.w0 + re;
	} else { a.qe = X.l_query; a.re = s.rbeg + s.len; }
	A.regs[g] = a; A.reg_ci[g] = (uint32_t)X.ci; A.ord[g] = (uint32_t)i;
}
// a chain by one lane: the pairs its seeds put on either list, then -- the caller has reserved that many slots from ls / rs on -- its regions
CS_HD inline void count_pairs(const ChainCtx &X, const cs_seed_t *sd, int ns, uint32_t &nl, uint32_t &nr)
{
	for (int i = 0; i < ns; ++i) { const cs_seed_t s = sd[i]; nl += s.qbeg != 0; nr += s.qbeg + s.len != X.l_query; }
}
CS_HD inline void emit_chain(const Args &A, const ChainCtx &X, const cs_seed_t *sd, int ns, uint64_t ls, uint64_t rs)
{
	const int32_t *sc = A.score ? A.score + X.s0 : nullptr;
	for (int i = 0; i < ns; ++i) {
		const cs_seed_t s = sd[i];
		const bool left = s.qbeg != 0, right = s.qbeg + s.len != X.l_query;
		emit_region(A, X, s, i, seed_rank(sd, sc, ns, i), left, right, ls, rs);
		ls += left; rs += right;
	}
}
// a long chain (a repeat's hundreds of seeds on one diagonal band) by W lanes: a seed per lane, W at a time
template <int W, class Reserve> CS_HD inline void chain_regions(const Args &A, int64_t ci, int lane, Reserve reserve)
{
	const uint64_t lt = (1ull << lane) - 1ull;
	const ChainCtx X = chain_ctx(A, ci);
	const cs_seed_t *sd = A.cseeds + X.s0;
	const int32_t *sc = A.score ? A.score + X.s0 : nullptr;
	const int ns = (int)(A.cseed_off[ci + 1] - X.s0);
	for (int i0 = 0; i0 < ns; i0 += W) {
		const int i = i0 + lane;
		cs_seed_t s = {0, 0, 0}; int k = 0; bool left = false, right = false;
		if (i < ns) { s = sd[i]; k = seed_rank(sd, sc, ns, i); left = s.qbeg != 0; right = s.qbeg + s.len != X.l_query; }
		const uint64_t ml = csdd::wballot<W>(left), mr = csdd::wballot<W>(right);
		unsigned long long bl = 0, br = 0;
		if (lane == 0) { if (ml) bl = reserve(C_LEFT, csdd::wcount(ml)); if (mr) br = reserve(C_RIGHT, csdd::wcount(mr)); }
		bl = csdd::wbcast64<W>(bl, 0); br = csdd::wbcast64<W>(br, 0);
		if (i < ns) emit_region(A, X, s, i, k, left, right, bl + (uint64_t)csdd::wcount(ml & lt), br + (uint64_t)csdd::wcount(mr & lt));
	}
}

// ---- the results of a side.  settled unless the band may have cut the alignment: same score as before, the path stayed within 3/4 of the
// band, or no try left
CS_HD inline bool apply_result(const Args &A, cs_alnreg_t &a, const cs_ext_pair_t &pr, const cs_ext_result_t &x, int w, int attempt, int is_left, int pen_clip)
{
	const int prev = a.score;
	a.score = x.score;
	if (a.score == prev || x.max_off < (w >> 1) + (w >> 2) || attempt == 1) {
		const bool local = x.gscore <= 0 || x.gscore <= a.score - pen_clip;   // clipping beats reaching the end of the read
		if (is_left) {
			if (local) { a.qb -= x.qle; a.rb -= x.tle; a.truesc = a.score; }
			else { a.qb = 0; a.rb -= x.gtle; a.truesc = x.gscore; }
		} else {
			if (local) { a.qe += x.qle; a.re += x.tle; a.truesc += a.score - pr.h0; }
			else { const uint32_t r = A.chain_read[A.reg_ci[(uint32_t)pr.reserved]]; a.qe = (int32_t)(A.read_off[r + 1] - A.read_off[r]); a.re += x.gtle; a.truesc += x.gscore - pr.h0; }
		}
		a.w = a.w > w ? a.w : w;
	} else return true;
	return false;
}
CS_HD inline void right_h0(cs_ext_pair_t &p, const cs_alnreg_t *regs) { p.h0 = regs[(uint32_t)p.reserved].score; } // comp_seed.cpp:1917-1922
CS_HD inline void seed_coverage(const Args &A, int64_t g) // comp_seed.cpp:1758-1766
{
	const uint32_t ci = A.reg_ci[g];
	const cs_seed_t *sd = A.cseeds + A.cseed_off[ci];
	const int ns = (int)(A.cseed_off[ci + 1] - A.cseed_off[ci]);
	cs_alnreg_t a = A.regs[g];
	int cov = 0;
	for (int i = 0; i < ns; ++i) { const cs_seed_t t = sd[i]; if (t.qbeg >= a.qb && t.qbeg + t.len <= a.qe && t.rbeg >= a.rb && t.rbeg + t.len <= a.re) cov += t.len; }
	A.regs[g].seedcov = cov;
}

// ---- the purge, comp_seed.cpp:2141-2232: walking a read's seeds in the order they were extended, a seed that lies inside an earlier,
// surviving region of the read, is not much longer than that region's seed and sits within the band of its diagonal at either end is
// redundant -- unless a higher-ranked seed of its chain that is still in play overlaps it on another diagonal.  Its region is marked
// qb = qe = -1.  The walk over a read's regions is sequential (a region's fate decides about the later ones), but both tests are "is there
// one among the earlier ...": the lanes hold the earlier regions / the higher-ranked seeds and a ballot answers.
struct PReg { int64_t rb, re; int32_t qb, qe, seedlen0, w; };
template <class GapF> // gap_of(x) = affordable_gap(o, x); x is a distance inside the read here, 0 .. l_query
CS_HD inline bool purge_around(const cs_seed_t &s, const PReg &p, int l_query, GapF gap_of)
{
	if (s.rbeg < p.rb || s.rbeg + s.len > p.re || s.qbeg < p.qb || s.qbeg + s.len > p.qe) return false;
	if (s.len - p.seedlen0 > .1 * l_query) return false;
	int qd = s.qbeg - p.qb; int64_t rd = s.rbeg - p.rb;
	int gap = gap_of((int)(qd < rd ? qd : rd)), w = gap < p.w ? gap : p.w;
	if (qd - rd < w && rd - qd < w) return true;
	qd = p.qe - (s.qbeg + s.len); rd = p.re - (s.rbeg + s.len);
	gap = gap_of((int)(qd < rd ? qd : rd)); w = gap < p.w ? gap : p.w;
	return qd - rd < w && rd - qd < w;
}
CS_HD inline bool purge_rival(const cs_seed_t &s, const cs_seed_t &t) // t: a seed ranked above s in its chain
{
	if (t.len < s.len * .95) return false;
	if (s.qbeg <= t.qbeg && s.qbeg + s.len - t.qbeg >= s.len >> 2 && t.qbeg - s.qbeg != t.rbeg - s.rbeg) return true;
	return t.qbeg <= s.qbeg && t.qbeg + t.len - s.qbeg >= s.len >> 2 && s.qbeg - t.qbeg != s.rbeg - t.rbeg;
}
CS_HD inline void purge_load(const Args &A, uint64_t g0, uint64_t g, PReg &p, cs_seed_t &s, int &first)
{
	const uint64_t s0 = A.cseed_off[A.reg_ci[g]];
	first = (int)(s0 - g0);                                         // the read's regions [first, g) are the higher-ranked seeds of g's chain
	s = A.cseeds[s0 + A.ord[g]];
	const cs_alnreg_t a = A.regs[g];
	p.rb = a.rb; p.re = a.re; p.qb = a.qb; p.qe = a.qe; p.seedlen0 = a.seedlen0; p.w = a.w;
}
// a read of 2 .. W regions (with 64 lanes all but a few in a thousand): a region per lane, everything in registers -- the seed in question
// comes from its lane by a shuffle, which regions are still there is a mask
template <int W> CS_HD inline void purge_read_regs(const Args &A, int64_t r, int lane, unsigned long long &purged)
{
	const cs_aln_params_t &o = A.o;
	const uint64_t g0 = A.cseed_off[A.chain_off[r]], g1 = A.cseed_off[A.chain_off[r + 1]];
	const int G = (int)(g1 - g0), l_query = (int)(A.read_off[r + 1] - A.read_off[r]);
	PReg p = {0, 0, 0, 0, 0, 0}; cs_seed_t s = {0, 0, 0}; int first = 0;
	if (lane < G) purge_load(A, g0, g0 + (uint64_t)lane, p, s, first);
	const uint64_t all = G == 64 ? ~0ull : (1ull << G) - 1ull;
	uint64_t alive = all;
	for (int g = 1; g < G; ++g) {
		cs_seed_t sg; sg.rbeg = (int64_t)csdd::wbcast64<W>((unsigned long long)s.rbeg, g); sg.qbeg = csdd::wbcast<W>(s.qbeg, g); sg.len = csdd::wbcast<W>(s.len, g);
		const int fg = csdd::wbcast<W>(first, g);
		const bool before = lane < g && ((alive >> lane) & 1ull);
		if (csdd::wballot<W>(before && purge_around(sg, p, l_query, [&](int x) { return affordable_gap(o, x); })) == 0) continue;
		if (csdd::wballot<W>(before && lane >= fg && purge_rival(sg, s)) != 0) continue;
		alive &= ~(1ull << g);
	}
	const uint64_t gone = all & ~alive;
	if ((gone >> lane) & 1ull) { A.regs[g0 + (uint64_t)lane].qb = -1; A.regs[g0 + (uint64_t)lane].qe = -1; }
	if (lane == 0) purged += (unsigned long long)csdd::wcount(gone);
}
// a read of any size straight from memory (the fallback of purge_big_kernel): which regions are purged so far is a byte array that is
// read around the L1 (volatile) -- lane 0 writes, all lanes read in the next step.  On the device every step is a chain of HBM round trips.
// The number purged is added to lane 0's `purged` (an accumulator of the caller's, not a return value: purge_big_kernel's device code stays
// instruction for instruction what it was only this way).
template <int W> CS_HD inline void purge_read_mem(const Args &A, int64_t r, uint8_t *pflag, int lane, unsigned long long &purged)
{
	const cs_aln_params_t &o = A.o;
	volatile uint8_t *pf = pflag;
	const int l_query = (int)(A.read_off[r + 1] - A.read_off[r]);
	const uint64_t g0 = A.cseed_off[A.chain_off[r]];
	uint64_t g = g0;
	for (uint64_t ci = A.chain_off[r]; ci < A.chain_off[r + 1]; ++ci) {
		const uint64_t s0 = A.cseed_off[ci];
		const cs_seed_t *sd = A.cseeds + s0;
		const uint32_t *ord = A.ord + s0;
		const int ns = (int)(A.cseed_off[ci + 1] - s0);
		for (int k = 0; k < ns; ++k, ++g) {
			const cs_seed_t s = sd[ord[k]];
			bool around = false;
			for (uint64_t base = g0; base < g && !around; base += W) {
				const uint64_t i = base + (uint64_t)lane;
				bool hit = false;
				if (i < g && !pf[i]) { const cs_alnreg_t a = A.regs[i]; const PReg p = {a.rb, a.re, a.qb, a.qe, a.seedlen0, a.w}; hit = purge_around(s, p, l_query, [&](int x) { return affordable_gap(o, x); }); }
				around = csdd::wballot<W>(hit) != 0;
			}
			if (!around) continue;
			bool rival = false;
			for (int base = 0; base < k && !rival; base += W) {
				const int v = base + lane;
				const bool hit = v < k && !pf[s0 + (uint64_t)v] && purge_rival(s, sd[ord[v]]);
				rival = csdd::wballot<W>(hit) != 0;
			}
			if (rival) continue;
			if (lane == 0) { pf[g] = 1; A.regs[g].qb = -1; A.regs[g].qe = -1; ++purged; }
			csdd::wfence<W>();
		}
	}
}
} // namespace csa
