// band_align.hpp -- what the alignments behind the extension stage share: bwa_fill_scmat's matrix as a function, the two sequences of a
// global alignment (Span: the read forward or reversed, the packed reference on either strand) and banded_global_score, ksw_global2's
// score by W lanes (1 or 64; wave_lanes.hpp).  dedup_scan.hpp scores its patches with it; cigar_scan.hpp's global_fill is the same
// recurrence with the backtrack matrix beside it and is held against it by tests/cpp/cigar_scan_check.cpp; chain_filter_scan.hpp takes
// sc_mat alone.
//   banded_global_score of dedup.cpp: rows = reference, in place in H and E as the host keeps them, a column per lane in strips of W.
//   Gaps open from the diagonal move only, so within a row neither E nor F depends on the row's own H:
//   F(j) = max(NEG - e_ins (j - beg), max_{k<j} m(k) - oe_ins - e_ins (j - 1 - k)) is a prefix maximum of m(k) + e_ins k over the row,
//   carried from strip to strip -- integer maxima, exact in any order.  The band's clipping, H[end] = h1, E[end] = NEG, the first column
//   only while beg == 0 and the first row up to w are the host's.  Bases come from the read and from the packed reference on the fly
//   (3 - base of the mirrored position on the reverse strand; both reversed when rb >= l_pac).
#pragma once
#include "wave_lanes.hpp"

namespace csdd {
constexpr int32_t NEG = -0x40000000;          // MINUS_INF (ksw.c:490)

// entry t * 5 + q of bwa_fill_scmat's 5 x 5 matrix of int8_t, as the host fills it: a and -b pass through int8_t (a = 400 scores -112), and
// the flat array is indexed with the query's code, which can be 5 for '-' (t <= 3: within the 25).  So no score exceeds 127.
CS_HD inline int sc_mat(int a, int b, int t, int q) { const int x = t * 5 + q, i = x / 5, j = x - i * 5; return (i == 4 || j == 4) ? -1 : i == j ? (int)(int8_t)a : (int)(int8_t)-b; }

// the two sequences of a patch as global_span_score lays them out: query[0, qlen) from the read at q0, the reference span [b, e)
struct Span { const uint8_t *bases; int q0, qlen; bool rev; int64_t b, e, l_pac; const uint8_t *pac; };
CS_HD inline int span_q(const Span &S, int j) { return cs_base_code_(S.bases[S.q0 + (S.rev ? S.qlen - 1 - j : j)]); }
CS_HD inline int span_t(const Span &S, int64_t i)
{
	const int64_t p = S.rev ? S.e - 1 - i : S.b + i;
	return p >= S.l_pac ? 3 - cs_pac_base_(S.pac, (S.l_pac << 1) - 1 - p) : cs_pac_base_(S.pac, p);
}

// banded_global_score of dedup.cpp (ksw_global2's score, ksw.c:504-587).  H and E hold qlen + 1 words each.
template <int W> CS_HD int banded_global_score(const Span &S, int tlen, const cs_aln_params_t &o, int w, int32_t *H, int32_t *E, int lane)
{
	const int qlen = S.qlen, o_del = o.o_del, e_del = o.e_del, o_ins = o.o_ins, e_ins = o.e_ins;
	const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
	for (int j = lane; j <= qlen; j += W) { H[j] = j == 0 ? 0 : j <= w ? -(o_ins + e_ins * j) : NEG; E[j] = NEG; }
	wsync<W>();
	for (int i = 0; i < tlen; ++i) {
		const int tb = span_t(S, i);
		const int beg = i > w ? i - w : 0, end = i + w + 1 < qlen ? i + w + 1 : qlen;
		const int32_t h1_0 = beg == 0 ? -(o_del + e_del * (i + 1)) : NEG;
		if (beg >= end) {                                              // no column of this row inside the band: the host's H[end] = h1, E[end] = NEG
			if (lane == 0) { H[end] = h1_0; E[end] = NEG; }
			wsync<W>();
			continue;
		}
		int64_t carry = NO_G;
		int32_t next_h = 0;                                            // H[s + W] as the row before left it: the strip's last lane writes over it
		for (int s = beg; s < end; s += W) {
			const int j = s + lane;
			const bool in = j < end;
			int32_t m = NEG, e = NEG;
			if (in) { m = (lane == 0 && s > beg ? next_h : H[j]) + sc_mat(o.a, o.b, tb, span_q(S, j)); e = E[j]; }
			if (s + W < end) next_h = H[s + W];
			const int64_t g = in ? (int64_t)m + (int64_t)e_ins * j : NO_G;
			const int64_t gx = wprefix_max<W>(g, lane, carry);
			wsync<W>();                                                // every lane has read its H[j] before a neighbour stores H[j + 1]
			if (in) {
				const int64_t f0 = (int64_t)NEG - (int64_t)e_ins * (j - beg), f1 = gx - oe_ins - (int64_t)e_ins * (j - 1);
				const int32_t f = (int32_t)(f0 > f1 ? f0 : f1);
				int32_t h = m >= e ? m : e;
				h = h >= f ? h : f;
				const int32_t x = m - oe_del;
				e -= e_del; e = e > x ? e : x;
				E[j] = e;
				if (j == beg) H[beg] = h1_0;
				H[j + 1] = h;
				if (j + 1 == end) E[end] = NEG;
			}
		}
		wsync<W>();
	}
	const int score = H[qlen];
	wsync<W>();
	return score;
}
} // namespace csdd
