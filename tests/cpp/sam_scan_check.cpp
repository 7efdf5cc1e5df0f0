// sam_scan_check.cpp -- the bodies of compseed_amd/csrc/sam_scan.hpp (the SAM text of a batch: what cs_regions_sam runs as kernels) driven
// in the kernels' order as a plain C++ program: check (a lane per read, a lane per entry), index, the size pass (emit_read counting, with
// each line's start), an exclusive sum, the writing pass (emit_line / emit_unmapped storing, record by record).  tests/test_sam_scan_cpu.py chains it behind mark_scan_check and cigar_scan_check:
// it writes their results and the reads, names, qualities and comments as flat binary files into a directory, runs this over them and
// compares the text with the reference program's own output (tests/golden/samtext1).  No GPU and no Python in the process: it can be
// built with -fsanitize=address,undefined and run as it is.
// Built with -DCS_EMU_W=N (lockstep.hpp) the writing pass runs its N-lane instantiation -- the wave kernel's -- on N threads in lockstep;
// the size pass is the one-lane instantiation in every build, as in the device pass.
// Every read's text is also made by straight(), a routine of this file that formats with snprintf and std::string and shares no code
// with the header: the two must agree byte for byte.
//   sam_scan_check DIR [THREADS REPEAT]     (THREADS > 0: the one-lane writing pass over the batch on that many threads, REPEAT times; prints the best ms)
//   sam_scan_check --pa                     pa_milli against snprintf("%.3f") for every score, alt_sc in 1 .. 400
//   in:  meta.bin (int64: n_reads flags), reg_off.bin, marks.bin, line_off.bin, cig_off.bin, cig_src.bin, cig_regs.bin (mark_scan_check's
//        files), alns.bin, cigar.bin, md.bin (cigar_scan_check's), read_off.bin, bases.bin, name_off.bin, names.bin, ctg_names.bin (one
//        name a line), ctg_alt.bin, rg.bin (the RG id, may be empty); optional: quals.bin, comment_off.bin + comments.bin
//   out: text_off.bin (uint64), text.bin, stat.bin (uint64: lines unmapped bytes xa_entries sa_entries)
//   exit status 3: the input fails the checks (the library's CS_EINVAL); 1: a writer left its range or disagreed with its count
//   (the library's CS_EDEVICE); 5: the text differs from straight()'s
#include "lockstep.hpp"
#include "../../compseed_amd/csrc/sam_scan.hpp"

#include <chrono>
#include <cstring>
#include <thread>

static bool exists(const std::string &p) { FILE *f = fopen(p.c_str(), "rb"); if (f) fclose(f); return f != nullptr; }

static int pa_sweep()
{
	long bad = 0;
	for (int s = 1; s <= 400; ++s) for (int a = 1; a <= 400; ++a) {
		char want[64], got[64];
		snprintf(want, sizeof want, "%.3f", (double)s / a);
		const uint64_t q = cssm::pa_milli(s, a);
		snprintf(got, sizeof got, "%llu.%03llu", (unsigned long long)(q / 1000), (unsigned long long)(q % 1000));
		if (strcmp(want, got)) { if (!bad++) fprintf(stderr, "%d / %d: %s, not %s\n", s, a, got, want); }
	}
	printf("pa sweep: 160000 cases, %ld differ\n", bad);
	return bad ? 1 : 0;
}

// a read's records as the reference's functions make them, straight down, with snprintf: no Sink, no lanes, no prefix sums
static std::string straight(const cssm::In &D, int64_t r)
{
	auto num = [](long long v) { char b[32]; snprintf(b, sizeof b, "%lld", v); return std::string(b); };
	auto cig = [&](const cs_aln_t &a, const char *tab, bool hard) {
		std::string s;
		for (int k = 0; k < a.n_cigar; ++k) { int c = D.cigar[a.cigar_off + k] & 15; if (hard && (c == 3 || c == 4)) c = 4; s += num(D.cigar[a.cigar_off + k] >> 4) + tab[c]; }
		return s;
	};
	auto ctg = [&](int rid) { return std::string(D.ctg_names + D.ctg_name_off[rid], D.ctg_names + D.ctg_name_off[rid + 1]); };
	const std::string name(D.names + D.name_off[r], D.names + D.name_off[r + 1]);
	const std::string rg = D.rg_len ? "\tRG:Z:" + std::string(D.rg, D.rg + D.rg_len) : "";
	const std::string cm = D.comment_off ? "\t" + std::string(D.comments + D.comment_off[r], D.comments + D.comment_off[r + 1]) : "";
	const int len = (int)(D.read_off[r + 1] - D.read_off[r]);
	std::string seq, qual;
	for (int i = 0; i < len; ++i) { const uint8_t c = cs_base_code_(D.bases[D.read_off[r] + i]); seq += "ACGTN"[c > 4 ? 4 : c]; if (D.quals) qual += (char)D.quals[D.read_off[r] + i]; }
	std::vector<uint64_t> lines;                                      // the entries with a line, in rank order
	for (uint64_t e = D.ent_off[r]; e < D.ent_off[r + 1]; ++e) if (D.marks[D.ent_src[e]].line >= 0) lines.push_back(e);
	if (lines.empty()) return name + "\t4\t*\t0\t0\t*\t*\t0\t0\t" + seq + "\t" + (D.quals ? qual : "*") + "\tAS:i:0\tXS:i:0" + rg + cm + "\n";
	std::string out;
	for (size_t w = 0; w < lines.size(); ++w) {
		const uint64_t e = lines[w];
		const cs_mark_t &m = D.marks[D.ent_src[e]];
		const cs_aln_t &a = D.alns[e];
		const bool hard = w > 0 && !(D.flags & CS_SAM_SOFTCLIP) && !m.is_alt, sec = m.secondary >= 0;
		out += name + "\t" + num(m.flag | (a.is_rev ? 16 : 0)) + "\t" + ctg(a.rid) + "\t" + num(a.pos + 1) + "\t" + num(m.mapq) + "\t" + cig(a, "MIDSH", hard) + "\t*\t0\t0\t";
		if (sec) out += "*\t*";
		else {
			int qb = 0, qe = len;
			const uint32_t c5 = D.cigar[a.cigar_off], c3 = D.cigar[a.cigar_off + a.n_cigar - 1];
			if (hard) {
				if ((c5 & 15) >= 3) (a.is_rev ? qe : qb) += a.is_rev ? -(int)(c5 >> 4) : (int)(c5 >> 4);
				if ((c3 & 15) >= 3) (a.is_rev ? qb : qe) += a.is_rev ? (int)(c3 >> 4) : -(int)(c3 >> 4);
			}
			std::string s = seq.substr(qb, qe - qb), q = D.quals ? qual.substr(qb, qe - qb) : "*";
			if (a.is_rev) {
				std::string t(s.rbegin(), s.rend());
				for (char &c : t) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
				s = t;
				if (D.quals) q = std::string(q.rbegin(), q.rend());
			}
			out += s + "\t" + q;
		}
		out += "\tNM:i:" + num(a.nm) + "\tMD:Z:" + std::string(D.md + a.md_off) + "\tAS:i:" + num(D.ent_regs[e].score);
		if (m.xs >= 0) out += "\tXS:i:" + num(m.xs);
		out += rg;
		if (!sec) {
			std::string sa;
			for (size_t j = 0; j < lines.size(); ++j) {
				const cs_mark_t &mj = D.marks[D.ent_src[lines[j]]];
				const cs_aln_t &o = D.alns[lines[j]];
				if (j == w || mj.secondary >= 0) continue;
				sa += ctg(o.rid) + "," + num(o.pos + 1) + "," + (o.is_rev ? "-" : "+") + "," + cig(o, "MIDSH", false) + "," + num(mj.mapq) + "," + num(o.nm) + ";";
			}
			if (!sa.empty()) out += "\tSA:Z:" + sa;
			if (m.alt_sc > 0) { char b[64]; snprintf(b, sizeof b, "\tpa:f:%.3f", (double)D.ent_regs[e].score / m.alt_sc); out += b; }
		}
		std::string xa;
		for (uint64_t f = D.ent_off[r]; f < D.ent_off[r + 1]; ++f) {
			const cs_aln_t &o = D.alns[f];
			if (D.marks[D.ent_src[f]].xa_of < 0 || D.mark_off[r] + (uint64_t)D.marks[D.ent_src[f]].xa_of != D.ent_src[e]) continue;
			xa += ctg(o.rid) + "," + (o.is_rev ? "-" : "+") + num(o.pos + 1) + "," + cig(o, "MIDSHN", false) + "," + num(o.nm) + ";";
		}
		if (!xa.empty()) out += "\tXA:Z:" + xa;
		out += cm + "\n";
	}
	return out;
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "--pa")) return pa_sweep();
	if (argc != 2 && argc != 4) { fprintf(stderr, "usage: sam_scan_check DIR [THREADS REPEAT] | --pa\n"); return 2; }
	const std::string d = std::string(argv[1]) + "/";
	const int threads = argc == 4 ? atoi(argv[2]) : 0, repeat = argc == 4 ? atoi(argv[3]) : 0;
	std::vector<int64_t> meta; std::vector<uint64_t> mark_off, line_off, ent_off, read_off, name_off, comment_off; std::vector<cs_mark_t> marks; std::vector<uint32_t> ent_src, cigar;
	std::vector<cs_alnreg_t> ent_regs; std::vector<cs_aln_t> alns; std::vector<char> md, names, comments, ctg_text, rg; std::vector<uint8_t> bases, quals, ctg_alt;
	if (!slurp(d + "meta.bin", meta) || !slurp(d + "reg_off.bin", mark_off) || !slurp(d + "marks.bin", marks) || !slurp(d + "line_off.bin", line_off) || !slurp(d + "cig_off.bin", ent_off) ||
	    !slurp(d + "cig_src.bin", ent_src) || !slurp(d + "cig_regs.bin", ent_regs) || !slurp(d + "alns.bin", alns) || !slurp(d + "cigar.bin", cigar) || !slurp(d + "md.bin", md) ||
	    !slurp(d + "read_off.bin", read_off) || !slurp(d + "bases.bin", bases) || !slurp(d + "name_off.bin", name_off) || !slurp(d + "names.bin", names) || !slurp(d + "ctg_names.bin", ctg_text) ||
	    !slurp(d + "ctg_alt.bin", ctg_alt) || !slurp(d + "rg.bin", rg))
		return 2;
	const bool has_q = exists(d + "quals.bin"), has_c = exists(d + "comment_off.bin");
	if ((has_q && !slurp(d + "quals.bin", quals)) || (has_c && (!slurp(d + "comment_off.bin", comment_off) || !slurp(d + "comments.bin", comments)))) return 2;
	if (meta.size() != 2) { fprintf(stderr, "meta.bin: 2 words expected\n"); return 2; }
	const int64_t n = meta[0];
	const size_t per_read = (size_t)n + 1;
	std::vector<uint32_t> ctg_name_off(1, 0); std::vector<char> ctg_names;
	for (char c : ctg_text) { if (c == '\n') ctg_name_off.push_back((uint32_t)ctg_names.size()); else ctg_names.push_back(c); }
	// what the library's host side refuses before any kernel runs
	if (n < 0 || mark_off.size() != per_read || line_off.size() != per_read || ent_off.size() != per_read || read_off.size() != per_read || name_off.size() != per_read ||
	    (has_c && comment_off.size() != per_read) || ent_regs.size() != ent_src.size() || alns.size() != ent_src.size() || ctg_name_off.size() != ctg_alt.size() + 1 || ctg_alt.empty() ||
	    (has_q && quals.size() != bases.size())) {
		fprintf(stderr, "inconsistent input\n");
		return 3;
	}
	ctg_names.push_back(0); names.push_back(0); comments.push_back(0); rg.push_back(0); cigar.push_back(0); bases.push_back(0); quals.push_back(0);   // (no null data() for an empty array)
	cssm::In D;
	memset(&D, 0, sizeof D);
	D.n_reads = n; D.n_marks = marks.size(); D.n_lines = n ? line_off[(size_t)n] : 0; D.n_ents = ent_src.size(); D.n_cigar = cigar.size() - 1; D.md_bytes = md.size();
	D.mark_off = mark_off.data(); D.line_off = line_off.data(); D.ent_off = ent_off.data(); D.read_off = read_off.data(); D.name_off = name_off.data(); D.comment_off = has_c ? comment_off.data() : nullptr;
	D.marks = marks.data(); D.ent_src = ent_src.data(); D.ent_regs = ent_regs.data(); D.alns = alns.data(); D.cigar = cigar.data(); D.md = md.data();
	D.bases = bases.data(); D.quals = has_q ? quals.data() : nullptr; D.names = names.data(); D.comments = has_c ? comments.data() : nullptr;
	D.ctg_names = ctg_names.data(); D.ctg_name_off = ctg_name_off.data(); D.ctg_alt = ctg_alt.data(); D.n_ctg = (int)ctg_alt.size();
	D.rg = rg.data(); D.rg_len = (int)rg.size() - 1; D.flags = (uint32_t)meta[1];
	// the totals the host knows: the last offsets must lie inside the arrays it uploads
	if (n && (read_off[(size_t)n] > bases.size() - 1 || name_off[(size_t)n] > names.size() - 1 || (has_c && comment_off[(size_t)n] > comments.size() - 1))) { fprintf(stderr, "offsets beyond the arrays\n"); return 3; }

	// check: a lane per read, a lane per entry
	std::vector<uint32_t> md_len(D.n_ents + 1, 0), line_ent(D.n_lines + 1, 0), line_read(D.n_lines + 1, 0), n_pri(per_read, 0), n_xa(per_read, 0);
	std::vector<uint64_t> line_pos(D.n_lines + 1, 0);
	bool bad = n == 0 && (D.n_marks || D.n_ents);
	for (int64_t r = 0; r < n; ++r) bad |= cssm::check_read(D, r) != cssm::V_OK;
	// (check_read accepted e1 <= n_ents for every read before check_ent's lanes are believed; on the device both run in one launch and
	// neither follows the other's arrays)
	for (uint64_t e = 0; e < D.n_ents; ++e) bad |= cssm::check_ent(D, e, md_len.data()) != cssm::V_OK;
	if (bad) { fprintf(stderr, "the input fails the checks\n"); return 3; }
	const cssm::Index X = {md_len.data(), line_ent.data(), line_read.data(), n_pri.data(), n_xa.data(), line_pos.data()};
	for (int64_t r = 0; r < n; ++r) cssm::index_read(D, X, r);

	// the size pass and the exclusive sum
	std::vector<uint64_t> text_off(per_read, 0), stat(5, 0);
	for (int64_t r = 0; r < n; ++r) {
		cssm::Sink<1, false> S = {nullptr, 0, 0, 0, 0, false};
		cssm::emit_read<1, false>(D, X, r, S, line_pos.data());
		text_off[(size_t)r + 1] = text_off[(size_t)r] + S.pos;
		const uint64_t L = line_off[(size_t)r + 1] - line_off[(size_t)r];
		stat[0] += L; stat[1] += L == 0; stat[3] += n_xa[(size_t)r]; stat[4] += n_pri[(size_t)r] >= 2 ? (uint64_t)n_pri[(size_t)r] * (n_pri[(size_t)r] - 1) : 0;
	}
	stat[2] = text_off[(size_t)n];
	std::vector<char> text(text_off[(size_t)n] + 1, '#');

	// the writing pass: LANES lanes per record, the lines and then the reads without lines, as the device pass takes them
	std::vector<int> broken(64, 0);
	if (!run_lanes([&](int lane) {
		for (uint64_t t = 0; t < D.n_lines + (uint64_t)n; ++t) {
			const bool line = t < D.n_lines;
			const int64_t r = line ? (int64_t)line_read[t] : (int64_t)(t - D.n_lines);
			const uint64_t l0 = line_off[(size_t)r], l1 = line_off[(size_t)r + 1], t0 = text_off[(size_t)r];
			if (!line && l1 != l0) continue;
			const uint64_t lo = line ? t0 + line_pos[t] : t0, hi = line && t + 1 < l1 ? t0 + line_pos[t + 1] : text_off[(size_t)r + 1];
			cssm::Sink<LANES, true> S = {text.data(), lo, hi, lo, lane, false};
			if (line) cssm::emit_line<LANES, true>(D, X, r, t - l0, S); else cssm::emit_unmapped<LANES, true>(D, r, S);
			if (S.bad || S.pos != S.hi) broken[(size_t)lane] = 1;
		}
	})) return 2;
	for (int b : broken) if (b) { fprintf(stderr, "a writer left its range or disagreed with its count\n"); return 1; }
	if (text[text_off[(size_t)n]] != '#') { fprintf(stderr, "a store behind the text\n"); return 1; }
	text.pop_back();
	for (int64_t r = 0; r < n; ++r) {
		const std::string want = straight(D, r);
		if (want.size() != text_off[(size_t)r + 1] - text_off[(size_t)r] || memcmp(want.data(), text.data() + text_off[(size_t)r], want.size())) {
			fprintf(stderr, "read %lld differs from the straight routine:\n%s%.*s", (long long)r, want.c_str(), (int)(text_off[(size_t)r + 1] - text_off[(size_t)r]), text.data() + text_off[(size_t)r]);
			return 5;
		}
	}
	if (threads > 0) {                                                 // the figure a device pass is held against: the same text on host threads
		double best = 1e30;
		for (int k = 0; k < repeat; ++k) {
			const auto t0 = std::chrono::steady_clock::now();
			std::vector<std::thread> th;
			for (int t = 0; t < threads; ++t) th.emplace_back([&, t]() {
				for (int64_t r = n * t / threads; r < n * (t + 1) / threads; ++r) {
					cssm::Sink<1, true> S = {text.data(), text_off[(size_t)r], text_off[(size_t)r + 1], text_off[(size_t)r], 0, false};
					cssm::emit_read<1, true>(D, X, r, S);
				}
			});
			for (std::thread &t : th) t.join();
			best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
		}
		printf("host_write_ms %.4f threads %d reads %lld bytes %llu\n", best, threads, (long long)n, (unsigned long long)text.size());
	}
	if (!spill(d + "text_off.bin", text_off) || !spill(d + "text.bin", text) || !spill(d + "stat.bin", stat)) return 2;
	return 0;
}
