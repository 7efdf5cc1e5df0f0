// cigar_scan.hpp -- mem_reg2aln for ONE region (comp_seed.cpp:811-880: the band and its retries, bwa_gen_cigar2 of bwalib/bwa.c:147-233,
// ksw_global2 of bwalib/ksw.c:504-606 with its backtrack, NM and MD, the squeezed deletion, the clips, the contig-relative position), as
// bodies a device pass (cigar_gpu.hip) and a plain C++ program (tests/cpp/cigar_scan_check.cpp: W = 1 over the goldens, W = 8 / 64 on
// threads in lockstep) run alike.  The lane primitives are wave_lanes.hpp's; Span / span_q / span_t, sc_mat and banded_global_score,
// which global_fill restates with the backtrack matrix beside it, are band_align.hpp's.  In the order of the pass:
//   check_read     a lane per read: the offsets are CSR arrays, a read with regions is shorter than MAX_READ_LEN, a live mapped region lies
//                  inside its read and inside [0, 2 l_pac) and spans at most 2 MAX_READ_LEN of the reference; rd[g] = the region's read.
//                  The lane compares its own entries BEFORE it walks [reg_off[r], reg_off[r + 1]); nothing else follows an offset before
//                  the host has seen the verdict.
//   classify       a lane per region: empty (purged: qe <= qb; unmapped: rb < 0 or re < 0), rejected (bwa_gen_cigar2 returns nothing:
//                  the region bridges the strands, or its clamped span is not re - rb), or a job with its first band (first_band)
//   job_bytes      the backtrack matrix of a job's current try: n_col * tlen bytes, 0 without DP (bwa.c:167-175)
//   global_fill<W> W lanes per job: banded_global_score with the byte of ksw.c:551-565 per cell; sum_score<W>: the no-DP sum
//   next_try       the do ... while of mem_reg2aln as a function of (region, this try's score, the score before, the try's number):
//                  done, or the next band.  A band of 0 doubles to 0, and the reference's second try then ends by score == last_sc with
//                  the first try's result: such a job is done after ONE evaluation
//   count_aln      one lane per job: ONE walk over the backtrack matrix (global_backtrack) gives the counts -- CIGAR operations, MD bytes,
//                  NM -- without memory for the CIGAR: the runs come last one first, and so do MD's pieces
//   finish_aln     one lane per job: the same walk again, now writing the runs at their places, then NM and MD forward as bwa.c:195-225
//                  has them, the position, the clips.  It writes inside the ranges the counts gave it, whatever it finds.
// No body waits for another lane's memory: order comes from the kernel boundaries (or from the wave's own barrier inside global_fill).
// Float and double expressions are the reference's, operand for operand; the units that include this are compiled with -ffp-contract=off.
#pragma once
#include "band_align.hpp"
#include "wave_lanes.hpp"

namespace cscg {
using csdd::NEG; using csdd::NO_G; using csdd::Span; using csdd::sc_mat; using csdd::span_q; using csdd::span_t; using csdd::wprefix_max; using csdd::wsum; using csdd::wsync;
constexpr uint64_t MAX_READ_LEN = 65536;                               // as in the extension stage (align_gpu.hip)
enum { J_EMPTY = 0, J_REJECT = 1, J_JOB = 2 };                         // a region's class

struct In { const uint64_t *reg_off, *read_off; const cs_alnreg_t *regs; const uint8_t *bases; int64_t n_reads; uint64_t n_regs; };
struct Ref { int64_t l_pac; const uint8_t *pac; const int64_t *ctg_off; int n_ctg; };
// per region: its read, its class, the band of the current try (mem_reg2aln's w2), the tries evaluated, this try's score and the one before
struct State { uint32_t *rd; uint8_t *cls; int32_t *w2, *tries, *score, *last_sc; };
// what the counting call learns of a job: the result's CIGAR operations and MD bytes (NUL included), the raw CIGAR's runs, whether its first
// (with its length) or else its last is a deletion that is dropped, NM, and whether the walk left its band
struct Counts { uint32_t n_cigar, md_bytes, n_raw, lead_len; int32_t nm; uint8_t lead, trail, flagged; };

// true: the read's entries are consistent; *len: its length if it has regions (0 otherwise)
CS_HD inline bool check_read(const In &D, int64_t l_pac, int64_t r, uint32_t *rd, uint64_t *len)
{
	*len = 0;
	const uint64_t c0 = D.reg_off[r], c1 = D.reg_off[r + 1], b0 = D.read_off[r], b1 = D.read_off[r + 1];
	if (c1 < c0 || c1 > D.n_regs || b1 < b0 || (r == 0 && (b0 != 0 || c0 != 0)) || (r == D.n_reads - 1 && c1 != D.n_regs)) return false;
	if (c1 == c0) return true;
	const uint64_t l = b1 - b0;
	if (l >= MAX_READ_LEN) return false;
	*len = l;
	bool ok = true;
	for (uint64_t g = c0; g < c1; ++g) {                              // (c0 <= c1 <= n_regs: inside the arrays)
		rd[g] = (uint32_t)r;
		const cs_alnreg_t x = D.regs[g];
		if (x.qe <= x.qb || x.rb < 0 || x.re < 0) continue;           // purged or unmapped: an empty result, whatever else it holds
		if (x.qb < 0 || (uint64_t)x.qe > l || x.rb >= x.re || x.re > (l_pac << 1) || x.re - x.rb > (int64_t)(2 * MAX_READ_LEN)) ok = false;
	}
	return ok;
}

CS_HD inline int infer_bw(int l1, int l2, int score, int a, int q, int r)   // comp_seed.cpp:803-809
{
	if (l1 == l2 && l1 * a - score < (q + r - a) << 1) return 0;
	int w = (int)((double)((l1 < l2 ? l1 : l2) * a - score - q) / r + 2.);
	const int d = l1 - l2, ad = d < 0 ? -d : d;
	if (w < ad) w = ad;
	return w;
}
// the band of the first try (comp_seed.cpp:829-833, and the clamp of line 837)
CS_HD inline int first_band(const cs_aln_params_t &o, const cs_alnreg_t &x)
{
	const int tmp = infer_bw(x.qe - x.qb, (int)(x.re - x.rb), x.truesc, o.a, o.o_del, o.e_del);
	int w2 = infer_bw(x.qe - x.qb, (int)(x.re - x.rb), x.truesc, o.a, o.o_ins, o.e_ins);
	w2 = w2 > tmp ? w2 : tmp;
	if (w2 > o.w) w2 = w2 < x.w ? w2 : x.w;
	return w2 < o.w << 2 ? w2 : o.w << 2;
}
// after try number `i` (0, 1, 2) with band w2 scored `score` (last_sc: the try before, -(1 << 30) for none): true = done, or *next = the next band
CS_HD inline bool next_try(const cs_aln_params_t &o, const cs_alnreg_t &x, int w2, int score, int last_sc, int i, int *next)
{
	if (score == last_sc || w2 == o.w << 2) return true;              // comp_seed.cpp:840
	int n = w2 << 1;
	if (!(i + 1 < 3 && score < x.truesc - o.a)) return true;          // line 843
	n = n < o.w << 2 ? n : o.w << 2;                                  // line 837 of the next round
	if (n == w2) return true;                                         // 0 stays 0: the next try is this one again and ends by score == last_sc
	*next = n;
	return false;
}

CS_HD inline int classify(const Ref &R, const cs_aln_params_t &o, const cs_alnreg_t &x, int *w2)
{
	if (x.qe <= x.qb || x.rb < 0 || x.re < 0) return J_EMPTY;
	const int64_t l_pac = R.l_pac;
	if (x.rb >= x.re || (x.rb < l_pac && x.re > l_pac)) return J_REJECT;   // bwa.c:160
	int64_t b = x.rb, e = x.re;                                       // bns_get_seq (bntseq.c:403-424)
	if (e > (l_pac << 1)) e = l_pac << 1;
	if (b < 0) b = 0;
	if (!(b >= l_pac || e <= l_pac) || x.re - x.rb != e - b) return J_REJECT;
	*w2 = first_band(o, x);
	return J_JOB;
}

CS_HD inline Span job_span(const Ref &R, const cs_alnreg_t &x, const uint8_t *read) { const Span S = {read, x.qb, x.qe - x.qb, x.rb >= R.l_pac, x.rb, x.re, R.l_pac, R.pac}; return S; }
CS_HD inline bool job_nodp(const cs_alnreg_t &x, int w2) { return (int64_t)(x.qe - x.qb) == x.re - x.rb && w2 == 0; }   // bwa.c:167
// ksw_global2's band for bwa_gen_cigar2's w_ (bwa.c:178-187)
CS_HD inline int job_band(const cs_aln_params_t &o, const cs_alnreg_t &x, int w_)
{
	const int l_query = x.qe - x.qb, rlen = (int)(x.re - x.rb);
	const int mat0 = (int)(int8_t)o.a;
	const int max_ins = (int)((double)(((l_query + 1) >> 1) * mat0 - o.o_ins) / o.e_ins + 1.);
	const int max_del = (int)((double)(((l_query + 1) >> 1) * mat0 - o.o_del) / o.e_del + 1.);
	int max_gap = max_ins > max_del ? max_ins : max_del;
	max_gap = max_gap > 1 ? max_gap : 1;
	const int dl = rlen - l_query, adl = dl < 0 ? -dl : dl;
	int w = (max_gap + adl + 1) >> 1;
	w = w < w_ ? w : w_;
	const int min_w = adl + 3;
	return w > min_w ? w : min_w;
}
CS_HD inline int job_ncol(int qlen, int w) { return qlen < 2 * w + 1 ? qlen : 2 * w + 1; }   // ksw.c:512
CS_HD inline uint64_t job_bytes(const cs_aln_params_t &o, const cs_alnreg_t &x, int w2)
{
	if (job_nodp(x, w2)) return 0;
	return (uint64_t)job_ncol(x.qe - x.qb, job_band(o, x, w2)) * (uint64_t)(x.re - x.rb);
}

template <int W> CS_HD int sum_score(const Span &S, const cs_aln_params_t &o, int lane)   // bwa.c:174-175
{
	int sc = 0;
	for (int i = lane; i < S.qlen; i += W) sc += sc_mat(o.a, o.b, span_t(S, i), span_q(S, i));
	return wsum<W>(sc);
}

// banded_global_score (band_align.hpp) with ksw_global2's backtrack matrix: row i holds n_col bytes at z + i * n_col, column j at j - beg.
// The byte is the reference's (ksw.c:551-565): bits 0-1 the direction of H, bit 2 "E continues", bit 5 "F continues"; `f` is the F the
// cell itself used, which the prefix maximum gives every lane at once.  H and E hold qlen + 1 words each.
template <int W> CS_HD int global_fill(const Span &S, int tlen, const cs_aln_params_t &o, int w, int32_t *H, int32_t *E, uint8_t *z, int lane)
{
	const int qlen = S.qlen, o_del = o.o_del, e_del = o.e_del, o_ins = o.o_ins, e_ins = o.e_ins;
	const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins, n_col = job_ncol(qlen, w);
	for (int j = lane; j <= qlen; j += W) { H[j] = j == 0 ? 0 : j <= w ? -(o_ins + e_ins * j) : NEG; E[j] = NEG; }
	wsync<W>();
	for (int i = 0; i < tlen; ++i) {
		const int tb = span_t(S, i);
		const int beg = i > w ? i - w : 0, end = i + w + 1 < qlen ? i + w + 1 : qlen;
		const int32_t h1_0 = beg == 0 ? -(o_del + e_del * (i + 1)) : NEG;
		uint8_t *zi = z + (uint64_t)i * (uint64_t)n_col;
		if (beg >= end) {                                              // no column of this row inside the band
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
				uint8_t d = m >= e ? 0 : 1;
				int32_t h = m >= e ? m : e;
				d = h >= f ? d : 2;
				h = h >= f ? h : f;
				const int32_t x = m - oe_del;
				e -= e_del;
				d |= e > x ? 1 << 2 : 0;
				e = e > x ? e : x;
				E[j] = e;
				d |= f - e_ins > m - oe_ins ? 2 << 4 : 0;
				zi[j - beg] = d;
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

// ksw_global2's backtrack (ksw.c:589-602) as one walk that hands every finished run to emit(index in walk order, op, len): the runs come
// out last one first, push_cigar's merge rule applied, the two leftovers included.  Returns the number of runs; *bad: the walk would have
// read outside its row's [beg, end) and stopped.
template <class Emit> CS_HD inline int global_backtrack(const uint8_t *z, int tlen, int qlen, int w, bool *bad, Emit emit)
{
	const int n_col = job_ncol(qlen, w);
	int i = tlen - 1, k = (i + w + 1 < qlen ? i + w + 1 : qlen) - 1, which = 0, n = 0, op = -1; uint32_t len = 0;
	auto push = [&](int o2, uint32_t l2) { if (o2 == op) { len += l2; return; } if (op >= 0) emit(n++, op, len); op = o2; len = l2; };
	*bad = false;
	while (i >= 0 && k >= 0) {
		const int beg = i > w ? i - w : 0, end = i + w + 1 < qlen ? i + w + 1 : qlen;
		if (k < beg || k >= end) { *bad = true; break; }
		which = z[(uint64_t)i * (uint64_t)n_col + (uint64_t)(k - beg)] >> (which << 1) & 3;
		if (which == 0) { push(0, 1); --i; --k; }
		else if (which == 1) { push(2, 1); --i; }
		else { push(1, 1); --k; }
	}
	if (!*bad) {
		if (i >= 0) push(2, (uint32_t)(i + 1));
		if (k >= 0) push(1, (uint32_t)(k + 1));
	}
	if (op >= 0) emit(n++, op, len);
	return n;
}

CS_HD inline int pos2rid(const Ref &R, int64_t pos_f)                  // bns_pos2rid (bntseq.c:354-368)
{
	if (pos_f >= R.l_pac) return -1;
	int left = 0, mid = 0, right = R.n_ctg;
	while (left < right) {
		mid = (left + right) >> 1;
		if (pos_f >= R.ctg_off[mid]) {
			if (mid == R.n_ctg - 1) break;
			if (pos_f < R.ctg_off[mid + 1]) break;
			left = mid + 1;
		} else right = mid;
	}
	return mid;
}


// One walk, counting.  MD is c0 B1 c1 ... Bn cn NUL: breaks B (a mismatch's base; ^ and an inner deletion's bases) and the counts c of equal
// bases between them.  Walking backward, `tail` is the count that FOLLOWS the next break met; the last one left is c0.  A deletion is
// inner unless it is the raw CIGAR's first or last run (bwa.c:211), and whether a run is the first is known when the walk ends: one
// deletion waits in `pend` until the next run comes.
CS_HD inline Counts count_aln(const Ref &R, const cs_aln_params_t &o, const cs_alnreg_t &x, const uint8_t *read, int l_read, int w2, const uint8_t *z)
{
	const Span S = job_span(R, x, read);
	const int l_query = S.qlen, tlen = (int)(x.re - x.rb);
	const bool is_rev = x.rb >= R.l_pac;
	Counts c = {0, 0, 1, 0, 0, 0, 0, 0};
	int tail = 0, n_mm = 0, n_gap = 0; uint32_t bytes = 0;
	auto digits = [](int v) { int d = 1; while (v >= 10) { v /= 10; ++d; } return d; };
	auto match_run = [&](int xe, int ye, int len) {                   // query [xe - len, xe) against text [ye - len, ye), last base first
		for (int i = 1; i <= len; ++i) {
			if (span_q(S, xe - i) != span_t(S, ye - i)) { bytes += (uint32_t)digits(tail) + 1; tail = 0; ++n_mm; } else ++tail;
		}
	};
	if (job_nodp(x, w2)) match_run(l_query, tlen, l_query);
	else {
		int xe = l_query, ye = tlen, op_first = 0, op_last = 0; uint32_t len_first = 0, pend = 0; bool bad = false;
		c.n_raw = (uint32_t)global_backtrack(z, tlen, l_query, job_band(o, x, w2), &bad, [&](int r, int op, uint32_t len) {
			if (pend) { bytes += (uint32_t)digits(tail) + 1 + pend; tail = 0; n_gap += (int)pend; pend = 0; }   // the deletion before this run was an inner one
			if (r == 0) op_last = op;
			op_first = op; len_first = len;
			if (op == 0) { match_run(xe, ye, (int)len); xe -= (int)len; ye -= (int)len; }
			else if (op == 2) { if (r > 0) pend = len; ye -= (int)len; }
			else { xe -= (int)len; n_gap += (int)len; }
		});
		c.flagged = bad ? 1 : 0;
		c.lead = c.n_raw > 0 && op_first == 2 ? 1 : 0;
		c.trail = !c.lead && c.n_raw > 0 && op_last == 2 ? 1 : 0;
		c.lead_len = c.lead ? len_first : 0;
	}
	const int clip5 = is_rev ? l_read - x.qe : x.qb, clip3 = is_rev ? x.qb : l_read - x.qe;
	c.n_cigar = c.n_raw - c.lead - c.trail + (clip5 ? 1 : 0) + (clip3 ? 1 : 0);
	c.md_bytes = bytes + (uint32_t)digits(tail) + 1;
	c.nm = n_mm + n_gap;
	return c;
}

struct Sink { char *p; uint32_t n, cap; CS_HD void put(char ch) { if (n < cap) p[n] = ch; ++n; } };
CS_HD inline void put_num(Sink &s, int u)                              // kputw of a count
{
	char t[12]; int l = 0;
	do { t[l++] = (char)('0' + u % 10); u /= 10; } while (u);
	while (l) s.put(t[--l]);
}

// The job's result: cigar[0, c.n_cigar) and md[0, c.md_bytes) are its own ranges, *out gets every field but the two offsets.  The raw
// CIGAR's dropped deletion (the first with pos += len, or else the last: comp_seed.cpp:848-857) is not stored; NM and MD go forward over the
// kept runs, run k being the raw CIGAR's k + lead.  Returns false if it counted otherwise than `c` says (nothing was written outside).
CS_HD inline bool finish_aln(const Ref &R, const cs_aln_params_t &o, const cs_alnreg_t &x, const uint8_t *read, int l_read, int w2, int score, int tries, const uint8_t *z,
                             const Counts &c, uint32_t *cigar, char *md, cs_aln_t *out)
{
	const Span S = job_span(R, x, read);
	const int l_query = S.qlen, tlen = (int)(x.re - x.rb);
	const bool is_rev = x.rb >= R.l_pac;
	const int clip5 = is_rev ? l_read - x.qe : x.qb, clip3 = is_rev ? x.qb : l_read - x.qe;
	const int c5 = clip5 ? 1 : 0, c3 = clip3 ? 1 : 0, n_raw = (int)c.n_raw, lead = c.lead, n_kept = n_raw - lead - c.trail;
	bool same = (int)c.n_cigar == n_kept + c5 + c3 && n_kept >= 0;
	if (!same) return false;
	uint32_t *kept = cigar + c5;
	if (job_nodp(x, w2)) { if (n_kept == 1) kept[0] = (uint32_t)l_query << 4; else same = false; }
	else {
		bool bad;
		const int n = global_backtrack(z, tlen, l_query, job_band(o, x, w2), &bad, [&](int r, int op, uint32_t len) { const int k = n_raw - 1 - r - lead; if (k >= 0 && k < n_kept) kept[k] = len << 4 | (uint32_t)op; });
		same = n == n_raw;
	}
	if (!same) return false;
	if (c5) cigar[0] = (uint32_t)clip5 << 4 | 3;
	if (c3) cigar[c5 + n_kept] = (uint32_t)clip3 << 4 | 3;
	const char *int2base = is_rev ? "TGCAN" : "ACGTN";                // bwa.c:195-225
	Sink sk = {md, 0, c.md_bytes};
	int xq = 0, y = (int)c.lead_len, u = 0, n_mm = 0, n_gap = 0;
	for (int k = 0; k < n_kept; ++k) {
		const int op = (int)(kept[k] & 0xf), len = (int)(kept[k] >> 4), raw_k = k + lead;
		if (op == 0) {
			if (xq + len > l_query || y + len > tlen) { same = false; break; }
			for (int i = 0; i < len; ++i) {
				const int tb = span_t(S, y + i);
				if (span_q(S, xq + i) != tb) { put_num(sk, u); sk.put(int2base[tb]); ++n_mm; u = 0; } else ++u;
			}
			xq += len; y += len;
		} else if (op == 2) {
			if (y + len > tlen) { same = false; break; }
			if (raw_k > 0 && raw_k < n_raw - 1) {
				put_num(sk, u); sk.put('^');
				for (int i = 0; i < len; ++i) sk.put(int2base[span_t(S, y + i)]);
				u = 0; n_gap += len;
			}
			y += len;
		} else { xq += len; n_gap += len; }
	}
	put_num(sk, u); sk.put(0);
	int64_t pos = is_rev ? (R.l_pac << 1) - 1 - (x.re - 1) : x.rb;    // bns_depos of rb, or of re - 1 on the reverse strand
	pos += c.lead_len;
	const int rid = pos2rid(R, pos);
	out->rid = rid; out->pos = rid >= 0 ? pos - R.ctg_off[rid] : pos; out->is_rev = is_rev ? 1 : 0;
	out->score = score; out->nm = n_mm + n_gap; out->n_cigar = (int32_t)c.n_cigar; out->w = w2; out->tries = tries;
	return same && sk.n == c.md_bytes && out->nm == c.nm;
}
} // namespace cscg
