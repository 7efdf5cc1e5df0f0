// mark_scan_check.cpp -- the bodies of compseed_amd/csrc/mark_scan.hpp (primary marking, MAPQ, SAM line selection and XA membership: what
// cs_regions_mark runs as kernels) driven in the kernels' order as a plain C++ program: check, then per read the marking and the
// selection over batch-sized lists at the read's offset (the wave kernel's HBM placement), an exclusive sum of the reads' line counts,
// one of the need_cigar flags, and compact.hpp's move of the flagged regions in rank order.
// tests/test_mark_scan_cpu.py writes a set's regions, read offsets and the contigs' ALT flags as flat binary files into a directory, runs
// this over them and compares what it writes with the reference's own SAM lines (tests/golden/mark1).  No GPU and no Python in the
// process: it can be built with -fsanitize=address,undefined and run as it is.
// Built with -DCS_EMU_W=N (lockstep.hpp) every read runs the N-lane instantiations -- the wave kernel's -- on N threads in lockstep.
//   mark_scan_check DIR
//   in:  meta.bin (int64: n_reads n_regs l_pac n_ctg a b o_del e_del o_ins e_ins T mapq_coef_len max_xa_hits max_xa_hits_alt min_seed_len
//        flags id_base), fpar.bin (float: mask_level drop_ratio xa_drop_ratio), reg_off.bin, regs.bin, read_off.bin, ctg_alt.bin (uint8)
//   out: marks.bin (cs_mark_t), line_off.bin, cig_off.bin (uint64), cig_regs.bin (cs_alnreg_t), cig_src.bin (uint32),
//        stat.bin (uint64: lines xa_members cigar_regions)
//   exit status 3: the input fails check_read (the library's CS_EINVAL); 4: a size is out of range (CS_ERANGE)
#include "lockstep.hpp"
#include "../../compseed_amd/csrc/mark_scan.hpp"
#include "../../compseed_amd/csrc/compact.hpp"

#include <cmath>
#include <cstring>

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: mark_scan_check DIR\n"); return 2; }
	const std::string d = std::string(argv[1]) + "/";
	std::vector<int64_t> meta; std::vector<float> fpar; std::vector<uint64_t> reg_off, read_off; std::vector<cs_alnreg_t> regs; std::vector<uint8_t> ctg_alt;
	if (!slurp(d + "meta.bin", meta) || !slurp(d + "fpar.bin", fpar) || !slurp(d + "reg_off.bin", reg_off) || !slurp(d + "regs.bin", regs) || !slurp(d + "read_off.bin", read_off) ||
	    !slurp(d + "ctg_alt.bin", ctg_alt))
		return 2;
	if (meta.size() != 17 || fpar.size() != 3) { fprintf(stderr, "meta.bin: 17 words, fpar.bin: 3 words expected\n"); return 2; }
	const int64_t n = meta[0];
	const uint64_t n_regs = (uint64_t)meta[1];
	if (n < 0 || reg_off.size() != (size_t)n + 1 || read_off.size() != (size_t)n + 1 || regs.size() != n_regs || (int64_t)ctg_alt.size() != meta[3] || ctg_alt.empty()) {
		fprintf(stderr, "inconsistent input\n");
		return 2;
	}
	csmk::Par P;
	memset(&P, 0, sizeof P);
	P.a = (int)meta[4]; P.b = (int)meta[5]; P.o_del = (int)meta[6]; P.e_del = (int)meta[7]; P.o_ins = (int)meta[8]; P.e_ins = (int)meta[9];
	P.p.T = (int32_t)meta[10]; P.p.mapq_coef_len = (int32_t)meta[11]; P.p.max_xa_hits = (int32_t)meta[12]; P.p.max_xa_hits_alt = (int32_t)meta[13]; P.p.min_seed_len = (int32_t)meta[14];
	P.p.mask_level = fpar[0]; P.p.drop_ratio = fpar[1]; P.p.xa_drop_ratio = fpar[2];
	P.flags = (uint32_t)meta[15]; P.id_base = meta[16];
	if (P.p.mapq_coef_len <= 0 || P.p.mapq_coef_len >= csmk::LOG_N) { fprintf(stderr, "mapq_coef_len out of range\n"); return 2; }
	std::vector<double> logtab((size_t)csmk::LOG_N);
	for (int k = 0; k < csmk::LOG_N; ++k) logtab[(size_t)k] = std::log((double)k);
	const csmk::Ref R = {meta[2], ctg_alt.data(), (int)ctg_alt.size(), logtab.data()};
	const csmk::In D = {reg_off.data(), read_off.data(), regs.data(), n, n_regs};

	// check: a lane per read
	bool bad = n == 0 && (n_regs || reg_off[0]), range = false;
	for (int64_t r = 0; r < n; ++r) { const int v = csmk::check_read(D, R, r); bad |= v == csmk::V_BAD; range |= v == csmk::V_RANGE; }
	if (bad) { fprintf(stderr, "the input fails the checks\n"); return 3; }
	if (range) { fprintf(stderr, "a read has 65,536 regions or more, or a region spans more than 131,072 bases\n"); return 4; }

	// marking and selection: LANES lanes per read, read after read
	std::vector<int32_t> lists((size_t)csmk::WORK_LISTS * n_regs + 1, -7);
	std::vector<cs_mark_t> marks(n_regs); std::vector<cs_alnreg_t> ranked(n_regs); std::vector<uint32_t> need(n_regs + 1, 0);
	std::vector<uint64_t> nl((size_t)n + 1, 0);
	std::vector<uint64_t> stat(3, 0);
	if (!run_lanes([&](int lane) {
		for (int64_t r = 0; r < n; ++r) {
			const uint64_t c0 = reg_off[r];
			const int m = (int)(reg_off[r + 1] - c0);
			if (m == 0) continue;
			const csmk::Work K = csmk::work_at(lists.data(), n_regs, c0);
			csmk::mark_read<LANES>(P, R, regs.data() + c0, m, (uint64_t)(P.id_base + r), K, lane);
			int xa = 0;
			const int l = csmk::select_read<LANES>(P, R, regs.data() + c0, m, K, marks.data() + c0, ranked.data() + c0, need.data() + c0, &xa, lane);
			if (lane == 0) { nl[r] = (uint64_t)l; stat[1] += (uint64_t)xa; }
		}
	})) return 2;

	// the exclusive sums and the compaction
	std::vector<uint64_t> line_off((size_t)n + 1, 0), cig_off((size_t)n + 1, 0);
	for (int64_t r = 0; r < n; ++r) line_off[r + 1] = line_off[r] + nl[r];
	std::vector<uint32_t> nslot(n_regs + 1, 0);
	for (uint64_t g = 0; g < n_regs; ++g) nslot[g + 1] = nslot[g] + need[g];
	const uint64_t n_cig = nslot[n_regs];
	std::vector<cs_alnreg_t> cig_regs(n_cig); std::vector<uint32_t> cig_src(n_cig);
	for (uint64_t t = 0; t < n_regs * csa::REG_WORDS; ++t) csa::move_word((const uint64_t *)ranked.data(), need.data(), nslot.data(), t, (uint64_t *)cig_regs.data());
	for (uint64_t g = 0; g < n_regs; ++g) if (need[g]) cig_src[nslot[g]] = (uint32_t)g;
	for (int64_t r = 0; r <= n; ++r) cig_off[r] = nslot[reg_off[r]];
	stat[0] = line_off[n]; stat[2] = n_cig;
	if (!spill(d + "marks.bin", marks) || !spill(d + "line_off.bin", line_off) || !spill(d + "cig_off.bin", cig_off) || !spill(d + "cig_regs.bin", cig_regs) || !spill(d + "cig_src.bin", cig_src) ||
	    !spill(d + "stat.bin", stat))
		return 2;
	return 0;
}
