// chain_filter_scan_check.cpp -- the bodies of compseed_amd/csrc/chain_filter_scan.hpp (mem_chain_flt + mem_flt_chained_seeds: what
// cs_chain_filter_device runs as kernels) driven in the kernels' order as a plain C++ program: the weight body per chain, the classify body
// per read (exit status 3 if any verdict is bad), the per-read filter, the seed test per seed where the threshold table asks for it, two
// exclusive sums, the compact body per read.  tests/test_chain_filter_scan_cpu.py writes a set's unfiltered chains, reads, packed
// reference and contigs as flat binary files into a directory, runs this over them and compares what it writes with the host call and the
// reference's filtered chains.  No GPU and no Python in the process: it can be built with -fsanitize=address,undefined and run as it is.
// The one-lane build takes reads by LIGHT_MAX as the kernels do: filter_read<1> over lists at the read's own chain slots up to LIGHT_MAX
// chains, above it the wave kernel's placement (lists of LDS_CAP entries, else the slots).  Built with -DCS_EMU_W=N (lockstep.hpp) every
// read with chains goes through filter_read<N> on N threads in lockstep: the CS_FLT_WAVE_ONLY case.
//   chain_filter_scan_check DIR
//   in:  meta.bin (int64: n_reads n_chains n_seeds l_pac), par.bin (cs_flt_params_t), chain_off.bin, chains.bin, cseed_off.bin, cseeds.bin,
//        read_off.bin, bases.bin, pac.bin, ctg_off.bin (int64), ctg_len.bin (int32)
//   out: out_chain_off.bin, out_chains.bin, out_cseed_off.bin, out_cseeds.bin, out_score.bin,
//        out_stat.bin (uint64: wave reads, reads whose lists went to the slots, seeds scored, chains out, seeds out)
//   exit status 3: a body refused the input (the library's CS_EINVAL / CS_ERANGE); nothing followed an offset
#include "lockstep.hpp"
#include "../../compseed_amd/csrc/chain_filter_scan.hpp"

#include <cstring>

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: chain_filter_scan_check DIR\n"); return 2; }
	const std::string d = std::string(argv[1]) + "/";
	std::vector<int64_t> meta, ctg_off; std::vector<int32_t> ctg_len; std::vector<uint64_t> chain_off, cseed_off, read_off; std::vector<cs_chain_t> chains;
	std::vector<cs_seed_t> cseeds; std::vector<uint8_t> bases, pac, par;
	if (!slurp(d + "meta.bin", meta) || !slurp(d + "par.bin", par) || !slurp(d + "chain_off.bin", chain_off) || !slurp(d + "chains.bin", chains) || !slurp(d + "cseed_off.bin", cseed_off) ||
	    !slurp(d + "cseeds.bin", cseeds) || !slurp(d + "read_off.bin", read_off) || !slurp(d + "bases.bin", bases) || !slurp(d + "pac.bin", pac) || !slurp(d + "ctg_off.bin", ctg_off) ||
	    !slurp(d + "ctg_len.bin", ctg_len))
		return 2;
	if (meta.size() != 4 || par.size() != sizeof(cs_flt_params_t)) { fprintf(stderr, "meta.bin: 4 words, par.bin: a cs_flt_params_t expected\n"); return 2; }
	const int64_t n = meta[0];
	const uint64_t nc = (uint64_t)meta[1], ns = (uint64_t)meta[2];
	// only the arrays' sizes are the program's to check (the device call has them from the host); what they hold is the bodies'
	if (n < 1 || chain_off.size() != (size_t)n + 1 || read_off.size() != (size_t)n + 1 || chains.size() != nc || cseed_off.size() != nc + 1 || cseeds.size() != ns || ctg_off.empty() ||
	    ctg_off.size() != ctg_len.size() || (size_t)((meta[3] + 3) / 4) > pac.size()) {
		fprintf(stderr, "array sizes do not match meta.bin\n");
		return 2;
	}
	// ---- buffers, as the device call makes them
	const size_t per_chain = (size_t)nc + 1, per_seed = (size_t)ns + 1, per_read = (size_t)n + 1;
	std::vector<int32_t> tab((size_t)csf::MAX_READ_LEN), w(per_chain), cb(per_chain), ce(per_chain), cns(per_chain), ki(per_chain), kfirst(per_chain), sscore(per_seed), o_score(per_seed);
	std::vector<uint8_t> kflag(per_chain), alt(per_chain), keptv(per_chain); std::vector<csf::WRec> srt(per_chain); std::vector<csf::Iv> span(per_chain);
	std::vector<uint32_t> ord(per_chain), wave_list(per_read); std::vector<uint64_t> nch(per_read, 0), nsd(per_read, 0), o_chain_off(per_read), sbase(per_read), o_cseed_off(per_chain);
	std::vector<cs_chain_t> o_chains(per_chain); std::vector<cs_seed_t> o_cseeds(per_seed);
	unsigned long long ctr[6] = {};
	csf::Args A;
	memset(&A, 0, sizeof A);
	memcpy(&A.o, par.data(), sizeof A.o);
	csf::fill_table(A.o, tab.data());
	A.chain_off = chain_off.data(); A.cseed_off = cseed_off.data(); A.read_off = read_off.data(); A.chains = chains.data(); A.cseeds = cseeds.data(); A.bases = bases.data();
	A.n_reads = n; A.n_chains = nc; A.n_seeds = ns; A.flags = LANES > 1 ? CS_FLT_WAVE_ONLY : 0;
	A.l_pac = meta[3]; A.ctg_off = ctg_off.data(); A.ctg_len = ctg_len.data(); A.n_ctg = (int32_t)ctg_off.size(); A.pac = pac.data();
	A.tab = tab.data(); A.w = w.data(); A.cb = cb.data(); A.ce = ce.data(); A.cns = cns.data(); A.kflag = kflag.data();
	A.srt = srt.data(); A.span = span.data(); A.ki = ki.data(); A.kfirst = kfirst.data(); A.alt = alt.data(); A.keptv = keptv.data(); A.ord = ord.data(); A.sscore = sscore.data();
	A.nch = nch.data(); A.nsd = nsd.data(); A.wave_list = wave_list.data(); A.ctr = ctr;
	A.o_chain_off = o_chain_off.data(); A.sbase = sbase.data(); A.o_cseed_off = o_cseed_off.data(); A.o_chains = o_chains.data(); A.o_cseeds = o_cseeds.data(); A.o_score = o_score.data();
	// ---- weight_kernel, classify_kernel; the host's look at the counters
	for (uint64_t c = 0; c < nc; ++c) if (!csf::chain_weight_of(A, c)) ++ctr[2];
	for (int64_t r = 0; r < n; ++r) {
		const int v = csf::classify_read(A, r);
		if (v & csf::V_LONG) ++ctr[3];
		if (v & csf::V_BAD) ++ctr[2];
		if (v & csf::V_SW) ctr[4] |= 1;
		if (v & csf::V_WAVE) wave_list[ctr[0]++] = (uint32_t)r;
	}
	if (ctr[2] || ctr[3]) { fprintf(stderr, "refused: %llu inconsistent chains or reads, %llu reads of 65,536 bases or more\n", ctr[2], ctr[3]); return 3; }
	if (bases.size() < read_off[(size_t)n]) { fprintf(stderr, "bases.bin is shorter than read_off says\n"); return 2; }   // (the caller's buffer, not the pass's to check)
	// ---- light_kernel (the one-lane build only), wave_kernel
	if (LANES == 1)
		for (int64_t r = 0; r < n; ++r) {
			const uint64_t c0 = chain_off[(size_t)r], k = chain_off[(size_t)r + 1] - c0;
			if (k == 0 || k > (uint64_t)csf::LIGHT_MAX) continue;
			csf::filter_read<1>(A, r, 0, A.srt + c0, A.span + c0, A.alt + c0, A.ki + c0, A.kfirst + c0, A.keptv + c0);
		}
	std::vector<csf::WRec> s_srt(csf::LDS_CAP); std::vector<csf::Iv> s_span(csf::LDS_CAP); std::vector<int32_t> s_ki(csf::LDS_CAP), s_kfirst(csf::LDS_CAP); std::vector<uint8_t> s_alt(csf::LDS_CAP), s_keptv(csf::LDS_CAP);
	const bool started = run_lanes([&](int lane) {
		for (unsigned long long t = 0; t < ctr[0]; ++t) {
			const int64_t r = wave_list[t];
			const uint64_t c0 = chain_off[(size_t)r], k = chain_off[(size_t)r + 1] - c0;
			if (k <= (uint64_t)csf::LDS_CAP) csf::filter_read<LANES>(A, r, lane, s_srt.data(), s_span.data(), s_alt.data(), s_ki.data(), s_kfirst.data(), s_keptv.data());
			else {
				if (lane == 0) ++ctr[1];
				csf::filter_read<LANES>(A, r, lane, A.srt + c0, A.span + c0, A.alt + c0, A.ki + c0, A.kfirst + c0, A.keptv + c0);
			}
			csdd::wsync<LANES>();
		}
	});
	if (!started) return 2;
	// ---- sw_kernel (only if some read is long enough): a lane per input seed, rows of its own (stride 1)
	if (ctr[4]) {
		std::vector<uint32_t> he(csf::SW_MAX); std::vector<uint8_t> qs(csf::SW_MAX);
		for (uint64_t s = 0; s < ns; ++s) {
			int64_t c = 0, r = 0; int min_hsp = 0;
			if (!csf::seed_owner(A, s, &c, &r, &min_hsp)) continue;
			bool ran;
			sscore[s] = csf::seed_sw_score(A, r, s, min_hsp, he.data(), qs.data(), 1, &ran);
			if (sscore[s] == csf::DROPPED) { --nsd[(size_t)r]; --cns[(size_t)c]; }
			if (ran) ++ctr[5];
		}
	}
	// ---- the two exclusive sums over n + 1 counts (the last one 0: the totals), compact_kernel
	{ uint64_t a = 0, b = 0; for (size_t r = 0; r <= (size_t)n; ++r) { o_chain_off[r] = a; sbase[r] = b; a += nch[r]; b += nsd[r]; } }
	for (int64_t r = 0; r < n; ++r) csf::compact_read(A, r);
	const uint64_t nco = o_chain_off[(size_t)n], nso = sbase[(size_t)n];
	if (nco > nc || nso > ns) { fprintf(stderr, "more chains or seeds out than in\n"); return 1; }
	o_cseed_off.resize((size_t)nco + 1); o_chains.resize((size_t)nco); o_cseeds.resize((size_t)nso); o_score.resize((size_t)nso);
	const std::vector<uint64_t> stat = {ctr[0], ctr[1], ctr[5], nco, nso};
	if (!spill(d + "out_chain_off.bin", o_chain_off) || !spill(d + "out_chains.bin", o_chains) || !spill(d + "out_cseed_off.bin", o_cseed_off) || !spill(d + "out_cseeds.bin", o_cseeds) ||
	    !spill(d + "out_score.bin", o_score) || !spill(d + "out_stat.bin", stat))
		return 2;
	return 0;
}
