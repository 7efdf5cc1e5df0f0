// dedup_scan.hpp -- mem_sort_dedup_patch for ONE read, by W lanes (1 or 64): what dedup_range of dedup.cpp does between a read's live
// regions and its surviving ones, written for a device pass in which a light read is one lane and a heavy one a wave (DESIGN.md section
// 10-2: that pass is not in the library yet, and NO kernel includes this header) and for a plain C++ program: tests/cpp/dedup_scan_check.cpp
// runs W = 1 over the goldens, and W = 8 / 64 on threads in lockstep, without a GPU.  dedup.cpp stays the specification and does not
// include this header.
//   * the two sorts are klib's introsort (klib_sort.hpp) over (key, index) records, run by lane 0: its moves depend on comparisons only,
//     so the permutation is the one sorting the whole records gives;
//   * the scan: `i` is sequential; for one `i` the `j` loop is evaluated W candidates per step against the current `p`, and a ballot
//     finds the first `j` in loop order whose outcome is an EVENT -- the loop's end condition failing, the `break` of the redundant
//     branch, or a patch candidate (every cheap test of patch_score passed).  Every `j` before the event that is redundant with
//     p.score >= q.score gets q.qe = q.qb; the event is handled and the step restarts at j - 1 with the possibly merged `p` (a merge
//     moves p.rb, so the end condition is evaluated per candidate against the current p, never cached).  Between two events `p` is
//     constant and each `j` writes only its own `q`: that is the host's order;
//   * the global alignment of a patch is banded_global_score of band_align.hpp, a column per lane in strips of W; the lanes themselves --
//     wsync, wballot, wbcast, wsum, wprefix_max, lanes_below and the CSD_ macros under them -- are wave_lanes.hpp's.  Both headers were
//     split out of this one, which keeps what belongs to de-duplication; they keep its namespace.
// Float and double expressions are the host's, operand for operand; the units that include this are compiled with -ffp-contract=off.
#pragma once
#include "band_align.hpp"
#include "klib_sort.hpp"
#include "wave_lanes.hpp"

namespace csdd {
struct Par { cs_aln_params_t o; cs_dedup_params_t d; int64_t l_pac; const uint8_t *pac; };
struct SRec { int64_t k0; int32_t k1, k2, idx; };                 // first sort: k0 = re; second: k0 = rb, k1 = score, k2 = qb
struct ByEnd { CS_HD bool operator()(const SRec &x, const SRec &y) const { return x.k0 < y.k0; } };                                                   // alnreg_slt2
struct ByScore { CS_HD bool operator()(const SRec &x, const SRec &y) const { return x.k1 > y.k1 || (x.k1 == y.k1 && (x.k0 < y.k0 || (x.k0 == y.k0 && x.k2 < y.k2))); } };   // alnreg_slt
// the alignment's rows: `lds` holds 2 * lds_rows words (0: none), `hbm` 2 * (the read's length + 1)
struct Work { int32_t *lds; int lds_rows; int32_t *hbm; };
struct Stat { uint32_t aligns = 0, merges = 0; };

// global_span_score of dedup.cpp (bwa_gen_cigar2 without the CIGAR); false = no alignment, *score untouched
template <int W> CS_HD bool global_span_score(const Par &P, int w_, int l_query, const uint8_t *bases, int q0, int64_t rb, int64_t re, int *score, const Work &wk, int lane)
{
	const int64_t l_pac = P.l_pac;
	if (l_query <= 0 || rb >= re || (rb < l_pac && re > l_pac)) return false;
	int64_t b = rb, e = re;                                       // bns_get_seq (bntseq.c:403-424)
	if (e > (l_pac << 1)) e = l_pac << 1;
	if (b < 0) b = 0;
	if (!(b >= l_pac || e <= l_pac)) return false;
	const int64_t rlen = e - b;
	if (re - rb != rlen) return false;
	const Span S = {bases, q0, l_query, rb >= l_pac, b, e, l_pac, P.pac};
	if (l_query == re - rb && w_ == 0) {
		int sc = 0;
		for (int i = lane; i < l_query; i += W) sc += sc_mat(P.o.a, P.o.b, span_t(S, i), span_q(S, i));
		*score = wsum<W>(sc);
		return true;
	}
	const int mat0 = (int)(int8_t)P.o.a;
	const int max_ins = (int)((double)(((l_query + 1) >> 1) * mat0 - P.o.o_ins) / P.o.e_ins + 1.);
	const int max_del = (int)((double)(((l_query + 1) >> 1) * mat0 - P.o.o_del) / P.o.e_del + 1.);
	int max_gap = max_ins > max_del ? max_ins : max_del;
	max_gap = max_gap > 1 ? max_gap : 1;
	const int dl = (int)rlen - l_query, adl = dl < 0 ? -dl : dl;
	int w = (max_gap + adl + 1) >> 1;
	w = w < w_ ? w : w_;
	const int min_w = adl + 3;
	w = w > min_w ? w : min_w;
	int32_t *H = l_query + 1 <= wk.lds_rows ? wk.lds : wk.hbm;
	*score = banded_global_score<W>(S, (int)rlen, P.o, w, H, H + l_query + 1, lane);
	return true;
}

// mem_patch_reg (comp_seed.cpp:599-627) in two halves.  patch_cheap: every test of patch_score before the alignment, and the band it asks for
CS_HD inline bool patch_cheap(const Par &P, const cs_alnreg_t &a, const cs_alnreg_t &b, int *w_out)
{
	const int64_t l_pac = P.l_pac;
	if (a.rb < l_pac && b.rb >= l_pac) return false;               // on different strands
	if (a.qb >= b.qb || a.qe >= b.qe || a.re >= b.re) return false; // not colinear
	int w = (int)((a.re - b.rb) - (a.qe - b.qb));                  // the diagonal shift between the two
	w = w > 0 ? w : -w;
	double r = (double)(a.re - b.rb) / (double)(b.re - a.rb) - (double)(a.qe - b.qb) / (double)(b.qe - a.qb);
	r = r > 0. ? r : -r;
	if (a.re < b.rb || a.qe < b.qb) { if (w > P.o.w << 1 || r >= 0.05f) return false; }   // PATCH_MAX_R_BW
	else if (w > P.o.w << 2 || r >= 0.05f * 2) return false;
	w += a.w + b.w;
	w = w < P.o.w << 2 ? w : P.o.w << 2;
	*w_out = w;
	return true;
}
// ... and the rest: the alignment over both and the 0.9 test; returns the score (0: no merge)
template <int W> CS_HD int patch_finish(const Par &P, const uint8_t *bases, const cs_alnreg_t &a, const cs_alnreg_t &b, int w, const Work &wk, int lane)
{
	int score = 0;
	global_span_score<W>(P, w, b.qe - a.qb, bases, a.qb, a.rb, b.re, &score, wk, lane);   // (a failed fetch leaves the score at 0)
	const int q_s = (int)((double)(b.qe - a.qb) / ((b.qe - b.qb) + (a.qe - a.qb)) * (b.score + a.score) + .499);
	const int r_s = (int)((double)(b.re - a.rb) / ((b.re - b.rb) + (a.re - a.rb)) * (b.score + a.score) + .499);
	if ((double)score / (q_s > r_s ? q_s : r_s) < 0.90f) return 0;                        // PATCH_MIN_SC_RATIO
	return score;
}

enum { K_NONE = 0, K_KILLQ = 1, K_STOP = 2, K_BREAK = 3, K_PATCH = 4 };   // a candidate's outcome; from K_STOP on: an event
constexpr int BAILED = -1;

// One read: `in[0, n_in)` its regions as the extension stage left them (purged ones, qe <= qb, are dropped), `bases` its first base.
// a / nc / srt: room for the read's live regions (the caller's: private, LDS or HBM).  The survivors go to out / out_nc in the host's
// order; returns their number -- or BAILED, with nothing written to out, at the first patch candidate when may_align is false.
template <int W> CS_HD int dedup_read(const Par &P, const cs_alnreg_t *in, int n_in, const uint8_t *bases, int lane, cs_alnreg_t *a, int32_t *nc, SRec *srt,
                                      const Work &wk, bool may_align, cs_alnreg_t *out, int32_t *out_nc, Stat &st)
{
	const uint64_t below = lanes_below(lane);
	int n = 0;                                                    // the live regions in input order (comp_seed.cpp:2387-2393)
	for (int base = 0; base < n_in; base += W) {
		const int j = base + lane;
		const bool live = j < n_in && in[j].qe > in[j].qb;
		const uint64_t m = wballot<W>(live);
		if (live) { const SRec s = {in[j].re, 0, 0, j}; srt[n + __builtin_popcountll(m & below)] = s; }
		n += __builtin_popcountll(m);
	}
	wsync<W>();
	if (n == 0) return 0;
	if (n == 1) {                                                 // a read's only region keeps n_comp = 0: the reference's function returns before it sets it
		if (lane == 0) { out[0] = in[srt[0].idx]; out_nc[0] = 0; }
		wsync<W>();
		return 1;
	}
	if (lane == 0) cs_klib_introsort((size_t)n, srt, ByEnd());
	wsync<W>();
	for (int i = lane; i < n; i += W) { a[i] = in[srt[i].idx]; nc[i] = 1; }
	wsync<W>();
	const int64_t gap = P.d.max_chain_gap; const float mlr = P.d.mask_level_redun;
	for (int i = 1; i < n; ++i) {
		cs_alnreg_t p = a[i]; int pnc = nc[i];
		{ const cs_alnreg_t &pv = a[i - 1]; if (p.rid != pv.rid || p.rb >= pv.re + gap) continue; }
		int j = i - 1;
		while (j >= 0) {
			const int jj = j - lane;
			int kind = K_STOP;
			if (jj >= 0) {
				const cs_alnreg_t q = a[jj];
				if (!(p.rid == q.rid && p.rb < q.re + gap)) kind = K_STOP;
				else if (q.qe == q.qb) kind = K_NONE;                 // excluded before
				else {
					const int64_t o_r = q.re - p.rb;
					const int64_t o_q = q.qb < p.qb ? q.qe - p.qb : p.qe - q.qb;
					const int64_t m_r = q.re - q.rb < p.re - p.rb ? q.re - q.rb : p.re - p.rb;
					const int64_t m_q = q.qe - q.qb < p.qe - p.qb ? q.qe - q.qb : p.qe - p.qb;
					int w;
					if ((float)o_r > mlr * (float)m_r && (float)o_q > mlr * (float)m_q) kind = p.score < q.score ? K_BREAK : K_KILLQ;   // one of the two is redundant
					else kind = q.rb < p.rb && patch_cheap(P, q, p, &w) ? K_PATCH : K_NONE;
				}
			}
			const uint64_t evm = wballot<W>(kind >= K_STOP);
			const int first = evm ? __builtin_ffsll((long long)evm) - 1 : W;
			if (kind == K_KILLQ && lane < first) a[jj].qe = a[jj].qb;
			if (!evm) { j -= W; continue; }
			const int ev = wbcast<W>(kind, first);
			if (ev == K_STOP) break;
			if (ev == K_BREAK) { p.qe = p.qb; break; }
			if (!may_align) return BAILED;                            // (uniform: every lane sees the same event)
			const int je = j - first;                                 // merge q = a[je] into p?
			const cs_alnreg_t q = a[je];
			int w = 0;
			patch_cheap(P, q, p, &w);
			++st.aligns;
			const int score = patch_finish<W>(P, bases, q, p, w, wk, lane);
			if (score > 0) {
				++st.merges;
				pnc += nc[je] + 1;
				p.seedcov = p.seedcov > q.seedcov ? p.seedcov : q.seedcov;
				p.qb = q.qb; p.rb = q.rb;
				p.truesc = p.score = score;
				p.w = w;
				if (lane == 0) a[je].qb = a[je].qe;
			}
			j = je - 1;
		}
		if (lane == 0) { a[i] = p; nc[i] = pnc; }
		wsync<W>();
	}
	int m = 0;                                                    // the survivors in this order, then by score / start / read start (alnreg_slt)
	for (int base = 0; base < n; base += W) {
		const int i = base + lane;
		const bool live = i < n && a[i].qe > a[i].qb;
		const uint64_t mk = wballot<W>(live);
		if (live) { const SRec s = {a[i].rb, a[i].score, a[i].qb, i}; srt[m + __builtin_popcountll(mk & below)] = s; }
		m += __builtin_popcountll(mk);
	}
	wsync<W>();
	if (m == 0) return 0;
	if (lane == 0) cs_klib_introsort((size_t)m, srt, ByScore());
	wsync<W>();
	int n_out = 0;                                                // identical neighbours dropped
	for (int base = 0; base < m; base += W) {
		const int i = base + lane;
		bool keep = i < m;
		if (keep && i > 0) { const SRec x = srt[i], y = srt[i - 1]; keep = !(x.k1 == y.k1 && x.k0 == y.k0 && x.k2 == y.k2); }
		const uint64_t mk = wballot<W>(keep);
		if (keep) { const int o = n_out + __builtin_popcountll(mk & below), k = srt[i].idx; out[o] = a[k]; out_nc[o] = nc[k]; }
		n_out += __builtin_popcountll(mk);
	}
	wsync<W>();
	return n_out;
}
} // namespace csdd
