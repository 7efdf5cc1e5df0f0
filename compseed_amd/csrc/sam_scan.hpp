// sam_scan.hpp -- the SAM text of a batch: what mem_aln2sam (comp_seed.cpp:904-1024), the string part of mem_gen_alt (:1056-1067) and the
// unmapped record of mem_reg2sam (:1107-1117) write for single-end reads, from cs_regions_mark's marks and cs_regions_cigar's alignments
// over marks->cigar_regs, as bodies a device pass (sam_gpu.hip) and a plain C++ program (tests/cpp/sam_scan_check.cpp: W = 1, and
// W = 8 / 64 on threads in lockstep) run alike.  The lane primitives are wave_lanes.hpp's.  An "entry" is an entry of cigar_regs: the
// regions with a line or an XA membership, per read in rank order, entry e with its mark ent_src[e] and its alignment alns[e].
// In the order of the pass:
//   check_read      a lane per read: every CSR array starts at 0 and does not decrease, marks / entries / lines end at their counts; the
//                   read is shorter than MAX_READ; the read's marks number their lines 0, 1, 2 ... in rank order and as many as line_off
//                   says; xa_of is -1 or a rank of the read; the entries name exactly the read's marks with line >= 0 or xa_of >= 0, in
//                   order; every entry's alignment has a contig, a position, a score, a CIGAR inside the array whose clips fit the read.
//                   The lane compares its own offsets BEFORE it walks them.
//   check_ent       a lane per entry: CIGAR range and op codes (at most 4), md_off inside the array with a NUL behind it (md_len[e] = the
//                   string's length: no later loop looks for a NUL), rid inside the contig table.
//                   Nothing else follows an offset before the host has seen the verdict; every later loop's trip count is a count that
//                   these two bounded.
//   index_read      a lane per read: line_ent[line_off[r] + l] = the entry of line l, line_read = r; n_pri[r] = lines that are not real secondaries
//                   (mark.secondary < 0: a -M supplementary prints 0x100 but is none); n_xa[r] = members of an XA list that is printed
//   emit_line / emit_unmapped / emit_read<W, STORE>   a line's record, the record of a read without lines, all records of a read (the size
//                   pass, which also notes where each line starts: line_pos), field by field in mem_aln2sam's order, through a Sink that counts
//                   (STORE = false: the size pass) or stores (the writing pass): ONE routine, so the two cannot drift apart.  All W lanes
//                   walk the same fields with the same position; byte runs (name, SEQ, QUAL, MD, RG, comment, contig names) are stored W
//                   bytes a step with reversal and complement done in the index; a CIGAR's runs are stored by the lanes that own them,
//                   64 runs a step, at offsets from a prefix sum over the runs' widths; a number or a literal of a few bytes is lane 0's.
//                   The members of an SA or XA list are found W candidates a step by ballot.  A store outside the record's range
//                   [Sink.lo, Sink.hi) is not made and reported, as is an end position other than hi.
// No body waits for another lane's memory: the lanes only meet in shuffles and ballots.
#pragma once
#include "wave_lanes.hpp"

namespace cssm {
using csdd::wballot;
constexpr uint64_t MAX_READ = 65536;                                   // a read is shorter than this
enum { V_OK = 0, V_BAD = 1 };

struct In {
	int64_t n_reads; uint64_t n_marks, n_lines, n_ents, n_cigar, md_bytes;
	const uint64_t *mark_off, *line_off, *ent_off, *read_off, *name_off, *comment_off;   // n_reads + 1 each; comment_off may be null
	const cs_mark_t *marks; const uint32_t *ent_src; const cs_alnreg_t *ent_regs; const cs_aln_t *alns; const uint32_t *cigar; const char *md;
	const uint8_t *bases, *quals; const char *names, *comments;       // quals / comments may be null
	const char *ctg_names; const uint32_t *ctg_name_off; const uint8_t *ctg_alt; int n_ctg;   // the contig table: names as a CSR
	const char *rg; int rg_len; uint32_t flags;                        // the RG tag's value (rg_len 0: no tag), CS_SAM_*
};
struct Index { uint32_t *md_len, *line_ent, *line_read, *n_pri, *n_xa; uint64_t *line_pos; };   // md_len: per entry; line_ent / line_read / line_pos: per line; n_pri / n_xa: per read

CS_HD inline bool csr_ok(const uint64_t *off, int64_t r) { return off[r + 1] >= off[r] && (r != 0 || off[0] == 0); }

CS_HD inline int check_read(const In &D, int64_t r)
{
	if (!csr_ok(D.mark_off, r) || !csr_ok(D.line_off, r) || !csr_ok(D.ent_off, r) || !csr_ok(D.read_off, r) || !csr_ok(D.name_off, r) || (D.comment_off && !csr_ok(D.comment_off, r))) return V_BAD;
	const uint64_t m0 = D.mark_off[r], m1 = D.mark_off[r + 1], e0 = D.ent_off[r], e1 = D.ent_off[r + 1], L = D.line_off[r + 1] - D.line_off[r];
	if (m1 > D.n_marks || e1 > D.n_ents || D.line_off[r + 1] > D.n_lines) return V_BAD;
	if (r == D.n_reads - 1 && (m1 != D.n_marks || e1 != D.n_ents || D.line_off[r + 1] != D.n_lines)) return V_BAD;
	const uint64_t len = D.read_off[r + 1] - D.read_off[r], nm = m1 - m0;
	if (len >= MAX_READ || L > nm || e1 - e0 > nm || nm > 0x7fffffffull) return V_BAD;
	uint64_t lines = 0, need = 0;
	for (uint64_t g = m0; g < m1; ++g) {                               // (m0 <= m1 <= n_marks: inside the array)
		const int line = D.marks[g].line, xa = D.marks[g].xa_of;
		if (line >= 0 ? (uint64_t)line != lines : line != -1) return V_BAD;
		if (xa < -1 || (xa >= 0 && (uint64_t)xa >= nm)) return V_BAD;
		if (line >= 0) ++lines;
		if (line >= 0 || xa >= 0) ++need;
	}
	if (lines != L || need != e1 - e0) return V_BAD;
	uint64_t prev = 0;
	for (uint64_t e = e0; e < e1; ++e) {                               // (inside the array as well)
		const uint64_t g = D.ent_src[e];
		if (g < m0 || g >= m1 || (e > e0 && g <= prev)) return V_BAD;
		prev = g;
		if (D.marks[g].line < 0 && D.marks[g].xa_of < 0) return V_BAD;   // as many entries as marks that need one, each another such mark: all of them
		const cs_aln_t a = D.alns[e];
		if (a.rid < 0 || a.pos < 0 || a.nm < 0 || a.n_cigar <= 0 || a.cigar_off > D.n_cigar || (uint64_t)a.n_cigar > D.n_cigar - a.cigar_off) return V_BAD;
		if (D.ent_regs[e].score < 0 || D.marks[g].mapq < 0) return V_BAD;
		const uint32_t c5 = D.cigar[a.cigar_off], c3 = D.cigar[a.cigar_off + (uint64_t)a.n_cigar - 1];
		uint64_t clip = (c5 & 15) >= 3 ? c5 >> 4 : 0;
		if (a.n_cigar > 1 && (c3 & 15) >= 3) clip += c3 >> 4;
		if (clip > len) return V_BAD;
	}
	return V_OK;
}
CS_HD inline int check_ent(const In &D, uint64_t e, uint32_t *md_len)
{
	const cs_aln_t a = D.alns[e];
	if (a.rid < 0 || a.rid >= D.n_ctg || a.n_cigar < 0 || a.cigar_off > D.n_cigar || (uint64_t)a.n_cigar > D.n_cigar - a.cigar_off || a.md_off >= D.md_bytes) return V_BAD;
	for (uint64_t k = a.cigar_off; k < a.cigar_off + (uint64_t)a.n_cigar; ++k) if ((D.cigar[k] & 15) > 4) return V_BAD;
	uint64_t k = a.md_off;
	while (k < D.md_bytes && D.md[k]) ++k;
	if (k == D.md_bytes || k - a.md_off > 0xffffffffull) return V_BAD;
	md_len[e] = (uint32_t)(k - a.md_off);
	return V_OK;
}

CS_HD inline bool is_real_secondary(const cs_mark_t &m) { return m.secondary >= 0; }   // never by the printed 0x100: -M gives it to supplementary lines

CS_HD inline void index_read(const In &D, const Index &X, int64_t r)
{
	const uint64_t m0 = D.mark_off[r], l0 = D.line_off[r];
	uint32_t pri = 0, xa = 0;
	for (uint64_t e = D.ent_off[r]; e < D.ent_off[r + 1]; ++e) {
		const cs_mark_t &m = D.marks[D.ent_src[e]];
		if (m.line >= 0) { X.line_ent[l0 + (uint64_t)m.line] = (uint32_t)e; X.line_read[l0 + (uint64_t)m.line] = (uint32_t)r; if (!is_real_secondary(m)) ++pri; }
		if (m.xa_of >= 0 && D.marks[m0 + (uint64_t)m.xa_of].line >= 0) ++xa;
	}
	X.n_pri[r] = pri; X.n_xa[r] = xa;
}
// (double)score / alt_sc in thousandths, rounded as glibc's "%.3f" rounds it: the EXACT binary value half-to-even, by integer arithmetic
// on the mantissa (score >= 0, alt_sc > 0: the value is below 2^31, its exponent negative)
CS_HD inline uint64_t pa_milli(int score, int alt_sc)
{
	const double v = (double)score / alt_sc;
	const uint64_t bits = __builtin_bit_cast(uint64_t, v);
	const int ex = (int)(bits >> 52 & 0x7ff);
	if (ex == 0) return 0;                                            // 0 (a denormal cannot come out of two ints)
	const uint64_t p = ((bits & ((1ull << 52) - 1)) | 1ull << 52) * 1000;   // v * 1000 = p * 2^(ex - 1075), p < 2^63
	const int s = 1075 - ex;
	if (s <= 0) return p << -s;
	if (s >= 64) return 0;
	uint64_t q = p >> s;
	const uint64_t rem = p & ((1ull << s) - 1), half = 1ull << (s - 1);
	if (rem > half || (rem == half && (q & 1))) ++q;
	return q;
}

CS_HD inline int ndig(uint64_t v) { int n = 1; while (v >= 10) { v /= 10; ++n; } return n; }

// the exclusive prefix sum of v over the lanes; total: the sum
template <int W> CS_HD inline int wscan_excl(int v, int lane, int &total)
{
#ifdef CSD_SYNC
	if constexpr (W > 1) {
		int x = v;
		for (int d = 1; d < W; d <<= 1) { const int y = CSD_SHFL_UP(x, d, W); if (lane >= d) x += y; }
		total = CSD_SHFL(x, W - 1, W);
		return x - v;
	}
#endif
	(void)lane;
	total = v;
	return 0;
}

template <int W, bool STORE> struct Sink {
	char *text; uint64_t lo, hi, pos; int lane; bool bad;
	CS_HD void put(uint64_t at, char c) { if (at >= lo && at < hi) text[at] = c; else bad = true; }
	CS_HD void ch(char c) { if (STORE && lane == 0) put(pos, c); ++pos; }
	CS_HD void num(uint64_t v)
	{
		const int n = ndig(v);
		if (STORE && lane == 0) { uint64_t at = pos + (uint64_t)n; do { put(--at, (char)('0' + v % 10)); v /= 10; } while (v); }
		pos += (uint64_t)n;
	}
	template <int N> CS_HD void lit(const char (&s)[N])
	{
		if (STORE && lane == 0) for (int i = 0; i < N - 1; ++i) put(pos + (uint64_t)i, s[i]);
		pos += (uint64_t)(N - 1);
	}
	template <class F> CS_HD void bytes(uint64_t len, F f)                // byte i of the run is f(i): W bytes a step
	{
		if (STORE) for (uint64_t i = (uint64_t)lane; i < len; i += W) put(pos + i, f(i));
		pos += len;
	}
	CS_HD void run(const char *s, uint64_t len) { bytes(len, [=](uint64_t i) { return s[i]; }); }
	// n runs as <length><letter of tab>; hard: a clip is written H (add_cigar, comp_seed.cpp:897-898)
	CS_HD void cigar(const uint32_t *c, int n, const char *tab, bool hard)
	{
		for (int k0 = 0; k0 < n; k0 += W) {
			const int k = k0 + lane;
			uint32_t x = 0; int w = 0;
			if (k < n) { x = c[k]; w = ndig(x >> 4) + 1; }
			int total;
			const int before = wscan_excl<W>(w, lane, total);
			if (STORE && k < n) {
				int op = (int)(x & 15);
				if (hard && (op == 3 || op == 4)) op = 4;
				uint64_t at = pos + (uint64_t)(before + w - 1), v = x >> 4;
				put(at, tab[op]);
				do { put(--at, (char)('0' + v % 10)); v /= 10; } while (v);
			}
			pos += (uint64_t)total;
		}
	}
};

// the j in [0, n) with test(j), in order, W candidates a step: body(j) runs on all lanes alike
template <int W, class T, class B> CS_HD inline void each_hit(uint64_t n, int lane, T test, B body)
{
	for (uint64_t j0 = 0; j0 < n; j0 += W) {
		uint64_t m = wballot<W>(j0 + (uint64_t)lane < n && test(j0 + (uint64_t)lane));
		while (m) { const int b = __builtin_ctzll(m); m &= m - 1; body(j0 + (uint64_t)b); }
	}
}

template <int W, bool STORE> CS_HD inline void emit_ctg(const In &D, Sink<W, STORE> &S, int rid)
{
	S.run(D.ctg_names + D.ctg_name_off[rid], D.ctg_name_off[rid + 1] - D.ctg_name_off[rid]);
}
// SEQ, a tab, QUAL: the read's bases [qb, qe), forward or reversed and complemented, and its qualities alike
template <int W, bool STORE> CS_HD inline void emit_seq_qual(const In &D, Sink<W, STORE> &S, uint64_t b0, uint64_t qb, uint64_t qe, bool rev)
{
	const uint8_t *bs = D.bases + b0;
	if (!rev) S.bytes(qe - qb, [=](uint64_t i) { const uint8_t c = cs_base_code_(bs[qb + i]); return "ACGTN"[c > 4 ? 4 : c]; });
	else S.bytes(qe - qb, [=](uint64_t i) { const uint8_t c = cs_base_code_(bs[qe - 1 - i]); return "TGCAN"[c > 4 ? 4 : c]; });
	S.ch('\t');
	if (!D.quals) { S.ch('*'); return; }
	const uint8_t *q = D.quals + b0;
	if (!rev) S.bytes(qe - qb, [=](uint64_t i) { return (char)q[qb + i]; });
	else S.bytes(qe - qb, [=](uint64_t i) { return (char)q[qe - 1 - i]; });
}

// what every record ends in
template <int W, bool STORE> CS_HD inline void emit_tail(const In &D, int64_t r, Sink<W, STORE> &S)
{
	if (D.comment_off) { S.ch('\t'); S.run(D.comments + D.comment_off[r], D.comment_off[r + 1] - D.comment_off[r]); }
	S.ch('\n');
}
// the record of a read without lines (mem_reg2aln of no region: flag 4, score 0, sub 0), from S.pos on
template <int W, bool STORE> CS_HD inline void emit_unmapped(const In &D, int64_t r, Sink<W, STORE> &S)
{
	const uint64_t b0 = D.read_off[r];
	S.run(D.names + D.name_off[r], D.name_off[r + 1] - D.name_off[r]);
	S.lit("\t4\t*\t0\t0\t*\t*\t0\t0\t");
	emit_seq_qual(D, S, b0, 0, D.read_off[r + 1] - b0, false);
	S.lit("\tAS:i:0\tXS:i:0");
	if (D.rg_len) { S.lit("\tRG:Z:"); S.run(D.rg, (uint64_t)D.rg_len); }
	emit_tail(D, r, S);
}
// the record of line `which` of read r, from S.pos on
template <int W, bool STORE> CS_HD inline void emit_line(const In &D, const Index &X, int64_t r, uint64_t which, Sink<W, STORE> &S)
{
	const int lane = S.lane;
	const uint64_t b0 = D.read_off[r], len = D.read_off[r + 1] - b0, l0 = D.line_off[r], L = D.line_off[r + 1] - l0, m0 = D.mark_off[r], e0 = D.ent_off[r], ne = D.ent_off[r + 1] - e0;
	const bool several = X.n_pri[r] >= 2, xa_any = X.n_xa[r] != 0;
	const uint64_t e = X.line_ent[l0 + which];
	const uint64_t g = D.ent_src[e];
	const cs_mark_t mk = D.marks[g];
	const cs_aln_t a = D.alns[e];
	const uint32_t *cg = D.cigar + a.cigar_off;
	const bool sec = is_real_secondary(mk);
	const bool hard = which > 0 && !(D.flags & CS_SAM_SOFTCLIP) && !mk.is_alt;
	S.run(D.names + D.name_off[r], D.name_off[r + 1] - D.name_off[r]); S.ch('\t');
	S.num((uint64_t)((mk.flag | (a.is_rev ? 0x10 : 0)) & 0xffff)); S.ch('\t');
	emit_ctg(D, S, a.rid); S.ch('\t');
	S.num((uint64_t)a.pos + 1); S.ch('\t');
	S.num((uint64_t)mk.mapq); S.ch('\t');
	S.cigar(cg, a.n_cigar, "MIDSH", hard);
	S.lit("\t*\t0\t0\t");
	if (sec) S.lit("*\t*");
	else {
		uint64_t qb = 0, qe = len;
		if (hard) {                                                   // cut exactly where the CIGAR got H; on the reverse strand the leading clip cuts the read's end
			const uint32_t c5 = cg[0], c3 = cg[a.n_cigar - 1];
			const uint64_t lead = (c5 & 15) >= 3 ? c5 >> 4 : 0, trail = (c3 & 15) >= 3 ? c3 >> 4 : 0;
			if (!a.is_rev) { qb += lead; qe -= trail; } else { qe -= lead; qb += trail; }
			if (qe < qb) { S.bad = true; qe = qb; }                   // (a CIGAR of one clip: check_read counts it once)
		}
		emit_seq_qual(D, S, b0, qb, qe, a.is_rev != 0);
	}
	S.lit("\tNM:i:"); S.num((uint64_t)a.nm);
	S.lit("\tMD:Z:"); S.run(D.md + a.md_off, X.md_len[e]);
	S.lit("\tAS:i:"); S.num((uint64_t)D.ent_regs[e].score);
	if (mk.xs >= 0) { S.lit("\tXS:i:"); S.num((uint64_t)mk.xs); }
	if (D.rg_len) { S.lit("\tRG:Z:"); S.run(D.rg, (uint64_t)D.rg_len); }
	if (!sec) {
		if (several) {                                                // the read's other lines that are not real secondaries, in line order
			S.lit("\tSA:Z:");
			each_hit<W>(L, lane, [&](uint64_t j) { return j != which && !is_real_secondary(D.marks[D.ent_src[X.line_ent[l0 + j]]]); }, [&](uint64_t j) {
				const uint64_t f = X.line_ent[l0 + j];
				const cs_aln_t o = D.alns[f];
				emit_ctg(D, S, o.rid); S.ch(',');
				S.num((uint64_t)o.pos + 1); S.ch(',');
				S.ch("+-"[o.is_rev ? 1 : 0]); S.ch(',');
				S.cigar(D.cigar + o.cigar_off, o.n_cigar, "MIDSH", false);
				S.ch(','); S.num((uint64_t)D.marks[D.ent_src[f]].mapq);
				S.ch(','); S.num((uint64_t)o.nm);
				S.ch(';');
			});
		}
		if (mk.alt_sc > 0) {
			const uint64_t q = pa_milli(D.ent_regs[e].score, mk.alt_sc);
			S.lit("\tpa:f:"); S.num(q / 1000); S.ch('.');
			S.ch((char)('0' + q / 100 % 10)); S.ch((char)('0' + q / 10 % 10)); S.ch((char)('0' + q % 10));
		}
	}
	if (xa_any) {                                                      // the regions whose xa_of names this line's rank, in rank order
		const int rank = (int)(g - m0);
		bool first = true;
		each_hit<W>(ne, lane, [&](uint64_t j) { return D.marks[D.ent_src[e0 + j]].xa_of == rank; }, [&](uint64_t j) {
			const cs_aln_t o = D.alns[e0 + j];
			if (first) { S.lit("\tXA:Z:"); first = false; }
			emit_ctg(D, S, o.rid); S.ch(',');
			S.ch("+-"[o.is_rev ? 1 : 0]); S.num((uint64_t)o.pos + 1); S.ch(',');
			S.cigar(D.cigar + o.cigar_off, o.n_cigar, "MIDSHN", false);
			S.ch(','); S.num((uint64_t)o.nm);
			S.ch(';');
		});
	}
	emit_tail(D, r, S);
}
// all records of read r, from S.pos on; line_pos (the size pass): where each line starts, counted from the read's first byte
template <int W, bool STORE> CS_HD inline void emit_read(const In &D, const Index &X, int64_t r, Sink<W, STORE> &S, uint64_t *line_pos = nullptr)
{
	const uint64_t l0 = D.line_off[r], L = D.line_off[r + 1] - l0, start = S.pos;
	if (L == 0) { emit_unmapped(D, r, S); return; }
	for (uint64_t which = 0; which < L; ++which) {
		if (line_pos && S.lane == 0) line_pos[l0 + which] = S.pos - start;
		emit_line(D, X, r, which, S);
	}
}
} // namespace cssm
