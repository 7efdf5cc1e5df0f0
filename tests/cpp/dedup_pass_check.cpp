// dedup_pass_check.cpp -- the WHOLE device de-duplication pass (its kernels are not in the library) as a plain C++
// program: the bodies of compseed_amd/csrc/dedup_pass.hpp and compact.hpp in the order kernels would run them -- check, light reads, heavy reads, keep flags, scan,
// scatter of regions and n_comp, offsets -- with a plain exclusive sum where the device calls rocPRIM, over batch-sized lists at the
// reads' input offsets as the device keeps them, and with the patch alignment's rows in a small array ("LDS", 2 * LDS_ROWS words) when they
// fit and in a large one ("HBM", 2 * (longest read + 1) words) otherwise.  tests/test_dedup_pass_cpu.py writes the inputs (the files of
// dedup_scan_check.cpp) and compares the outputs with the host call and the reference's goldens.  No GPU and no Python in the process:
// it can be built with -fsanitize=address,undefined and run as it is.  -DCS_EMU_W=N (lockstep.hpp): the heavy reads by N lanes on N
// lockstep threads.
//   dedup_pass_check DIR [LDS_ROWS]          (LDS_ROWS: default csdp::LDS_ROWS; 0: every alignment's rows in the large array)
//   in:  meta.bin, reg_off.bin, regs.bin, read_off.bin, bases.bin, pac.bin   (see dedup_scan_check.cpp)
//   out: out_off.bin, out_regs.bin, out_nc.bin, out_stat.bin (uint64: alignments, merges, heavy reads, regions out, heavy reads whose
//        alignments used the small rows, ... the large rows)
//   exit status 3: the check body refused the input (nothing followed an offset)
#include "lockstep.hpp"
#include "../../compseed_amd/csrc/dedup_pass.hpp"

#include <cstdlib>
#include <cstring>

constexpr int32_t SENTINEL = 0x7f7f7f7f;                              // in word 0 of both row arrays before a heavy read: an alignment leaves H[0] <= 0 there

struct Heavy {
	const csdp::In *D; const csdd::Par *P; const csdp::Lists *S; std::vector<int32_t> *lds, *hbm; int lds_rows;
	csdd::Stat st[64]; uint64_t used_lds = 0, used_hbm = 0;
};
static void before_read(Heavy &H) { if (!H.lds->empty()) (*H.lds)[0] = SENTINEL; (*H.hbm)[0] = SENTINEL; }
static void after_read(Heavy &H) { if (!H.lds->empty() && (*H.lds)[0] != SENTINEL) ++H.used_lds; if ((*H.hbm)[0] != SENTINEL) ++H.used_hbm; }

int main(int argc, char **argv)
{
	if (argc != 2 && argc != 3) { fprintf(stderr, "usage: dedup_pass_check DIR [LDS_ROWS]\n"); return 2; }
	const std::string d = std::string(argv[1]) + "/";
	const int lds_rows = argc == 3 ? atoi(argv[2]) : csdp::LDS_ROWS;
	std::vector<int64_t> meta; std::vector<uint64_t> reg_off, read_off; std::vector<cs_alnreg_t> regs; std::vector<uint8_t> bases, pac;
	if (!slurp(d + "meta.bin", meta) || !slurp(d + "reg_off.bin", reg_off) || !slurp(d + "regs.bin", regs) || !slurp(d + "read_off.bin", read_off) ||
	    !slurp(d + "bases.bin", bases) || !slurp(d + "pac.bin", pac))
		return 2;
	if (meta.size() != 12 || lds_rows < 0) { fprintf(stderr, "meta.bin: 12 words expected\n"); return 2; }
	const int64_t n = meta[0];
	// only the arrays' sizes are the program's to check (the device call has them from the host); what they hold is check_read's
	if (n < 1 || reg_off.size() != (size_t)n + 1 || read_off.size() != (size_t)n + 1 || regs.size() != (size_t)meta[1] || regs.empty()) { fprintf(stderr, "array sizes do not match meta.bin\n"); return 2; }
	pac.resize(pac.size() + 8, 0);
	csdd::Par P;
	memset(&P, 0, sizeof P);
	P.l_pac = meta[2]; P.pac = pac.data();
	P.o.a = (int32_t)meta[3]; P.o.b = (int32_t)meta[4]; P.o.o_del = (int32_t)meta[5]; P.o.e_del = (int32_t)meta[6]; P.o.o_ins = (int32_t)meta[7]; P.o.e_ins = (int32_t)meta[8];
	P.o.w = (int32_t)meta[9]; P.d.max_chain_gap = (int32_t)meta[10];
	const uint32_t bits = (uint32_t)meta[11];
	memcpy(&P.d.mask_level_redun, &bits, 4);
	if ((size_t)((P.l_pac + 3) / 4) > pac.size()) { fprintf(stderr, "pac.bin is shorter than l_pac\n"); return 2; }

	const uint64_t ng = regs.size();
	const csdp::In D = {reg_off.data(), read_off.data(), regs.data(), bases.data(), n, ng};
	// ---- dd_check_kernel
	uint64_t ctr[csdp::C_COUNT] = {};
	for (int64_t r = 0; r < n; ++r) {
		uint64_t len;
		if (!csdp::check_read(D, P.l_pac, r, &len)) ++ctr[csdp::C_BAD];
		else if (len > ctr[csdp::C_LONGEST]) ctr[csdp::C_LONGEST] = len;
	}
	ctr[csdp::C_NBASES] = read_off[(size_t)n];
	if (ctr[csdp::C_BAD]) { fprintf(stderr, "refused: %llu reads with inconsistent input\n", (unsigned long long)ctr[csdp::C_BAD]); return 3; }
	if (bases.size() < ctr[csdp::C_NBASES]) { fprintf(stderr, "bases.bin is shorter than read_off says\n"); return 2; }   // (the caller's buffer, not the pass's to check)
	const uint64_t longest = ctr[csdp::C_LONGEST];
	// ---- buffers, as the device call makes them
	std::vector<cs_alnreg_t> a(ng), stage(ng), o_regs(ng); std::vector<int32_t> nc(ng), stage_nc(ng), o_nc(ng); std::vector<csdd::SRec> srt(ng);
	std::vector<uint32_t> cnt((size_t)n), keep(ng + 1, 0xffffffffu), kscan(ng + 1); std::vector<uint8_t> heavy((size_t)n);
	std::vector<int32_t> lds((size_t)lds_rows * 2), hbm((size_t)(longest + 1) * 2);
	std::vector<uint64_t> o_off((size_t)n + 1);
	const csdp::Lists S = {a.data(), nc.data(), srt.data(), stage.data(), stage_nc.data(), cnt.data(), heavy.data()};
	// ---- dd_light_kernel
	for (int64_t r = 0; r < n; ++r) ctr[csdp::C_HEAVY] += (uint64_t)csdp::light_read(D, S, r);
	// ---- dd_wave_kernel
	Heavy H = {&D, &P, &S, &lds, &hbm, lds_rows, {}, 0, 0};
#ifdef CS_EMU_W
	constexpr int W = LANES;
	auto body = [&H](int lane) {
		const csdd::Work wk = {H.lds->data(), H.lds_rows, H.hbm->data()};
		for (int64_t r = 0; r < H.D->n_reads; ++r) {
			if (!H.S->heavy[r]) continue;
			if (lane == 0) before_read(H);
			emu::sync();
			csdp::heavy_read<W>(*H.D, *H.P, *H.S, r, lane, wk, H.st[lane]);
			emu::sync();
			if (lane == 0) after_read(H);
		}
	};
	if (!run_lanes(body)) return 2;
	for (int x = 1; x < W; ++x) if (H.st[x].aligns != H.st[0].aligns || H.st[x].merges != H.st[0].merges) { fprintf(stderr, "the lanes count different events\n"); return 1; }
#else
	{
		const csdd::Work wk = {lds.data(), lds_rows, hbm.data()};
		for (int64_t r = 0; r < n; ++r) {
			if (!heavy[(size_t)r]) continue;
			before_read(H);
			csdp::heavy_read<1>(D, P, S, r, 0, wk, H.st[0]);
			after_read(H);
		}
	}
#endif
	ctr[csdp::C_ALIGNS] = H.st[0].aligns; ctr[csdp::C_MERGES] = H.st[0].merges;
	for (int64_t r = 0; r < n; ++r) if (cnt[(size_t)r] > reg_off[(size_t)r + 1] - reg_off[(size_t)r]) { fprintf(stderr, "read %lld: more survivors than regions\n", (long long)r); return 1; }
	// ---- dd_keep_kernel, the scan, scatter_kernel, dd_nc_kernel, reg_off_live_kernel
	for (int64_t r = 0; r < n; ++r) csdp::keep_flags(D, cnt.data(), r, keep.data());
	{ uint32_t sum = 0; for (uint64_t g = 0; g <= ng; ++g) { kscan[g] = sum; sum += keep[g]; } }
	for (uint64_t t = 0; t < ng * csa::REG_WORDS; ++t) csa::move_word((const uint64_t *)stage.data(), keep.data(), kscan.data(), t, (uint64_t *)o_regs.data());
	for (uint64_t g = 0; g < ng; ++g) csdp::move_nc(stage_nc.data(), keep.data(), kscan.data(), g, o_nc.data());
	o_off = reg_off;
	for (int64_t r = 0; r <= n; ++r) csa::off_live(o_off.data(), kscan.data(), r);
	ctr[csdp::C_OUT] = kscan[ng];
	o_regs.resize((size_t)ctr[csdp::C_OUT]); o_nc.resize((size_t)ctr[csdp::C_OUT]);
	const std::vector<uint64_t> stat = {ctr[csdp::C_ALIGNS], ctr[csdp::C_MERGES], ctr[csdp::C_HEAVY], ctr[csdp::C_OUT], H.used_lds, H.used_hbm};
	if (!spill(d + "out_off.bin", o_off) || !spill(d + "out_regs.bin", o_regs) || !spill(d + "out_nc.bin", o_nc) || !spill(d + "out_stat.bin", stat)) return 2;
	return 0;
}
