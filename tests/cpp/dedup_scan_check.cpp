// dedup_scan_check.cpp -- the one-lane instantiation of compseed_amd/csrc/dedup_scan.hpp (the per-read routine written for a device pass
// that runs a lane or a wave per read) as a plain C++ program: tests/test_dedup_scan_cpu.py writes a set's regions, reads and the packed reference as
// flat binary files into a directory, runs this over them and compares what it writes with the reference's own regions (tests/golden/ddp1,
// aln2).  No GPU and no Python in the process: it can be built with -fsanitize=address,undefined and run as it is.
// Built with -DCS_EMU_W=N (lockstep.hpp) the program runs the N-lane instantiation -- the wave kernel's -- on N threads in lockstep.
//   dedup_scan_check DIR
//   in:  meta.bin (int64: n_reads n_regs l_pac a b o_del e_del o_ins e_ins w max_chain_gap, then the bits of mask_level_redun),
//        reg_off.bin, regs.bin, read_off.bin, bases.bin, pac.bin
//   out: out_off.bin (uint64, n_reads + 1), out_regs.bin (cs_alnreg_t), out_nc.bin (int32), out_stat.bin (uint64: alignments, merges)
#include "lockstep.hpp"
#include "../../compseed_amd/csrc/dedup_scan.hpp"

#include <cstring>

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: dedup_scan_check DIR\n"); return 2; }
	const std::string d = std::string(argv[1]) + "/";
	std::vector<int64_t> meta; std::vector<uint64_t> reg_off, read_off; std::vector<cs_alnreg_t> regs; std::vector<uint8_t> bases, pac;
	if (!slurp(d + "meta.bin", meta) || !slurp(d + "reg_off.bin", reg_off) || !slurp(d + "regs.bin", regs) || !slurp(d + "read_off.bin", read_off) ||
	    !slurp(d + "bases.bin", bases) || !slurp(d + "pac.bin", pac))
		return 2;
	if (meta.size() != 12) { fprintf(stderr, "meta.bin: 12 words expected\n"); return 2; }
	const int64_t n = meta[0];
	if (n < 0 || reg_off.size() != (size_t)n + 1 || read_off.size() != (size_t)n + 1 || regs.size() != (size_t)meta[1] || reg_off[(size_t)n] != regs.size() || read_off[(size_t)n] != bases.size()) {
		fprintf(stderr, "inconsistent input\n");
		return 2;
	}
	pac.resize(pac.size() + 8, 0);
	csdd::Par P;
	memset(&P, 0, sizeof P);
	P.l_pac = meta[2]; P.pac = pac.data();
	P.o.a = (int32_t)meta[3]; P.o.b = (int32_t)meta[4]; P.o.o_del = (int32_t)meta[5]; P.o.e_del = (int32_t)meta[6]; P.o.o_ins = (int32_t)meta[7]; P.o.e_ins = (int32_t)meta[8];
	P.o.w = (int32_t)meta[9]; P.d.max_chain_gap = (int32_t)meta[10];
	const uint32_t bits = (uint32_t)meta[11];
	memcpy(&P.d.mask_level_redun, &bits, 4);

	std::vector<uint64_t> out_off((size_t)n + 1, 0), stat(2, 0); std::vector<cs_alnreg_t> out_regs; std::vector<int32_t> out_nc;
	std::vector<cs_alnreg_t> a, o; std::vector<int32_t> nc, onc, ws; std::vector<csdd::SRec> srt;
	csdd::Stat st;
#ifdef CS_EMU_W
	constexpr int W = LANES;
	struct Shared { const csdd::Par *P; const std::vector<uint64_t> *reg_off, *read_off; const std::vector<cs_alnreg_t> *regs; const std::vector<uint8_t> *bases;
	                std::vector<cs_alnreg_t> *a, *o, *out_regs; std::vector<int32_t> *nc, *onc, *ws, *out_nc; std::vector<csdd::SRec> *srt; std::vector<uint64_t> *out_off;
	                int64_t n; int k[64]; csdd::Stat st[64]; int bad; } S = {&P, &reg_off, &read_off, &regs, &bases, &a, &o, &out_regs, &nc, &onc, &ws, &out_nc, &srt, &out_off, n, {}, {}, 0};
	auto body = [&S](int lane) {
		for (int64_t r = 0; r < S.n; ++r) {
			const uint64_t g0 = (*S.reg_off)[(size_t)r], g1 = (*S.reg_off)[(size_t)r + 1];
			const size_t cnt = (size_t)(g1 - g0), l_query = (size_t)((*S.read_off)[(size_t)r + 1] - (*S.read_off)[(size_t)r]);
			if (lane == 0) {
				S.a->assign(cnt + 1, cs_alnreg_t()); S.o->assign(cnt + 1, cs_alnreg_t()); S.nc->assign(cnt + 1, 0); S.onc->assign(cnt + 1, 0); S.srt->assign(cnt + 1, csdd::SRec());
				S.ws->assign((l_query + 1) * 2, 0);
			}
			emu::sync();
			const csdd::Work wk = {nullptr, 0, S.ws->data()};
			S.k[lane] = csdd::dedup_read<W>(*S.P, S.regs->data() + g0, (int)cnt, S.bases->data() + (*S.read_off)[(size_t)r], lane, S.a->data(), S.nc->data(), S.srt->data(), wk, true,
			                                  S.o->data(), S.onc->data(), S.st[lane]);
			emu::sync();
			if (lane == 0) {
				const int k = S.k[0];
				for (int x = 1; x < W; ++x) if (S.k[x] != k) S.bad = 1;          // (every lane returns the read's count)
				if (k < 0 || (size_t)k > cnt) { S.bad = 1; } else { S.out_regs->insert(S.out_regs->end(), S.o->begin(), S.o->begin() + k); S.out_nc->insert(S.out_nc->end(), S.onc->begin(), S.onc->begin() + k); }
				(*S.out_off)[(size_t)r + 1] = S.out_regs->size();
			}
			emu::sync();
		}
	};
	if (!run_lanes(body)) return 2;
	for (int x = 1; x < W; ++x) if (S.st[x].aligns != S.st[0].aligns || S.st[x].merges != S.st[0].merges) S.bad = 1;   // (... and counts the same events)
	if (S.bad) { fprintf(stderr, "the lanes disagree, or a read came back with an impossible count\n"); return 1; }
	st = S.st[0];
#else
	for (int64_t r = 0; r < n; ++r) {
		const uint64_t g0 = reg_off[(size_t)r], g1 = reg_off[(size_t)r + 1];
		const size_t cnt = (size_t)(g1 - g0), l_query = (size_t)(read_off[(size_t)r + 1] - read_off[(size_t)r]);
		a.assign(cnt + 1, cs_alnreg_t()); o.assign(cnt + 1, cs_alnreg_t()); nc.assign(cnt + 1, 0); onc.assign(cnt + 1, 0); srt.assign(cnt + 1, csdd::SRec());
		ws.assign((l_query + 1) * 2, 0);
		const csdd::Work wk = {nullptr, 0, ws.data()};
		const int k = csdd::dedup_read<1>(P, regs.data() + g0, (int)cnt, bases.data() + read_off[(size_t)r], 0, a.data(), nc.data(), srt.data(), wk, true, o.data(), onc.data(), st);
		if (k < 0 || (size_t)k > cnt) { fprintf(stderr, "read %lld: %d regions out of %zu\n", (long long)r, k, cnt); return 1; }
		out_regs.insert(out_regs.end(), o.begin(), o.begin() + k);
		out_nc.insert(out_nc.end(), onc.begin(), onc.begin() + k);
		out_off[(size_t)r + 1] = out_regs.size();
	}
#endif
	stat[0] = st.aligns; stat[1] = st.merges;
	if (!spill(d + "out_off.bin", out_off) || !spill(d + "out_regs.bin", out_regs) || !spill(d + "out_nc.bin", out_nc) || !spill(d + "out_stat.bin", stat)) return 2;
	return 0;
}
