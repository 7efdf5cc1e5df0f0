// align_scan_check.cpp -- the bodies of compseed_amd/csrc/align_scan.hpp (mem_chain2aln_across_reads_V2: what cs_extend_chains and
// cs_extend_chains_device run as kernels) driven in the order extend_core_ launches the kernels, as a plain C++ program: the two check
// bodies per read and per chain (exit status 3 if either refuses), chain_read, the queries, the windows (exit status 3 for a first seed
// outside the reference), an exclusive sum, fill, regions, the left side with its second try at 2w, right_h0, the right side likewise,
// seed coverage, the purge.  tests/test_align_scan_cpu.py writes a set's filtered chains, reads, packed reference and contigs as flat
// binary files into a directory, runs this over them and compares what it writes with the reference's regions.  The dynamic programming is
// not this program's subject: a pair is extended by the CPU restatement of the reference's extension (cso_extend_pair_rule of
// oracle/cs_bsw_oracle.c, linked in by the test) under the rule extend.hip applies with CS_EXT_VECTOR_ZDROP -- 3 for the pairs of the
// reference's vector class, else 0 --, on host threads; every other phase runs on the lanes.  No GPU and no Python in the process: it can
// be built with -fsanitize=address,undefined and run as it is.
// The one-lane build takes chains of up to small_chain seeds through count_pairs / emit_chain and longer ones through chain_regions<1>,
// and every read through purge_read_mem<1>, the reference's sequential loop.  Built with -DCS_EMU_W=N (lockstep.hpp) the small chains go
// a chain per lane (slots from wexcl_sum<N>, as region_kernel reserves them), long chains through chain_regions<N>, reads of up to
// min(N, light_max) regions through purge_read_regs<N> and the others through purge_read_mem<N>.  CS_ALN_NO_LIGHT_PATHS in the
// parameters' flags sets small_chain 0 and light_max 1 as extend_core_ does; CS_ALN_PURGE_FROM_HBM sets purge_cap 0, which only moves
// reads between the two last counts below -- purge_big_kernel's LDS walk is not run here (align_scan.hpp says why), its reads take
// purge_read_mem like the ones beyond its LDS.
//   align_scan_check DIR
//   in:  meta.bin (int64: n_reads n_chains n_seeds l_pac), par.bin (cs_aln_params_t), chain_off.bin, chains.bin, cseed_off.bin, cseeds.bin,
//        score.bin (int32 per seed, or empty: the seeds' lengths), read_off.bin, bases.bin, pac.bin, ctg_off.bin (int64), ctg_len.bin (int32)
//   out: out_reg_off.bin, out_regs.bin (cs_alnreg_t), out_stat.bin (uint64: left pairs, right pairs, retries, purged, long chains, reads
//        purged by purge_read_regs, by purge_read_mem, and of the latter those within purge_cap: the device's LDS walk)
//   exit status 3: a body refused the input (the library's CS_EINVAL); nothing followed an offset it had not checked
#include "lockstep.hpp"
#include "../../compseed_amd/csrc/align_scan.hpp"
#include "../../oracle/cs_oracle.h"   // (extern "C" inside)

#include <algorithm>
#include <cstring>

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: align_scan_check DIR\n"); return 2; }
	const std::string d = std::string(argv[1]) + "/";
	std::vector<int64_t> meta, ctg_off; std::vector<int32_t> ctg_len, score; std::vector<uint64_t> chain_off, cseed_off, read_off; std::vector<cs_chain_t> chains;
	std::vector<cs_seed_t> cseeds; std::vector<uint8_t> bases, pac, par;
	if (!slurp(d + "meta.bin", meta) || !slurp(d + "par.bin", par) || !slurp(d + "chain_off.bin", chain_off) || !slurp(d + "chains.bin", chains) || !slurp(d + "cseed_off.bin", cseed_off) ||
	    !slurp(d + "cseeds.bin", cseeds) || !slurp(d + "score.bin", score) || !slurp(d + "read_off.bin", read_off) || !slurp(d + "bases.bin", bases) || !slurp(d + "pac.bin", pac) ||
	    !slurp(d + "ctg_off.bin", ctg_off) || !slurp(d + "ctg_len.bin", ctg_len))
		return 2;
	if (meta.size() != 4 || par.size() != sizeof(cs_aln_params_t)) { fprintf(stderr, "meta.bin: 4 words, par.bin: a cs_aln_params_t expected\n"); return 2; }
	const int64_t n = meta[0], nc = meta[1], ns = meta[2];
	// only the arrays' sizes are the program's to check (the device call has them from the host); what they hold is the bodies'
	if (n < 1 || nc < 1 || ns < 1 || chain_off.size() != (size_t)n + 1 || read_off.size() != (size_t)n + 1 || chains.size() != (size_t)nc || cseed_off.size() != (size_t)nc + 1 ||
	    cseeds.size() != (size_t)ns || (!score.empty() && score.size() != (size_t)ns) || ctg_off.empty() || ctg_off.size() != ctg_len.size() || (size_t)((meta[3] + 3) / 4) > pac.size()) {
		fprintf(stderr, "array sizes do not match meta.bin\n");
		return 2;
	}
	cs_aln_params_t o;
	memcpy(&o, par.data(), sizeof o);
	// ---- check_reads_kernel, check_chains_kernel; the host's look at the counter
	const csa::DevIn D = {chain_off.data(), cseed_off.data(), read_off.data(), chains.data(), n, (uint64_t)nc, (uint64_t)ns};
	unsigned long long ctr[csa::C_COUNT] = {};
	for (int64_t r = 0; r < n; ++r) if (csa::check_read(D, r)) ++ctr[csa::C_REFUSED];
	for (int64_t c = 0; c < nc; ++c) if (csa::check_chain(D, (uint64_t)c)) ++ctr[csa::C_REFUSED];
	if (ctr[csa::C_REFUSED]) { fprintf(stderr, "refused: %llu reads or chains with inconsistent offsets or 65,536 bases or more\n", ctr[csa::C_REFUSED]); return 3; }
	const uint64_t n_bases = read_off[(size_t)n];
	if (bases.size() < n_bases) { fprintf(stderr, "bases.bin is shorter than read_off says\n"); return 2; }   // (the caller's buffer, not the pass's to check)
	memset(ctr, 0, sizeof ctr);
	// ---- buffers and arguments, as extend_core_ makes them
	std::vector<uint64_t> reg_off((size_t)n + 1), wlen2((size_t)nc + 1, 0), tb0((size_t)nc + 1);
	for (int64_t r = 0; r <= n; ++r) reg_off[(size_t)r] = cseed_off[chain_off[(size_t)r]];   // reg_off_kernel
	std::vector<uint32_t> chain_read((size_t)nc), big((size_t)nc), ord((size_t)ns), reg_ci((size_t)ns); std::vector<int64_t> w0((size_t)nc + 1);
	std::vector<uint8_t> qbuf((size_t)n_bases * 2 + 1), tbuf, pflag((size_t)ns, 0); std::vector<cs_alnreg_t> regs((size_t)ns);
	std::vector<cs_ext_pair_t> lp((size_t)ns), rp((size_t)ns), retry((size_t)ns); std::vector<cs_ext_result_t> res((size_t)ns);
	csa::Args A;
	memset(&A, 0, sizeof A);
	A.chain_off = chain_off.data(); A.cseed_off = cseed_off.data(); A.read_off = read_off.data(); A.chains = chains.data(); A.cseeds = cseeds.data();
	A.score = score.empty() ? nullptr : score.data(); A.bases = bases.data(); A.n_reads = n; A.n_chains = nc; A.n_seeds = ns; A.l_pac = meta[3]; A.n_bases = n_bases;
	A.pac = pac.data(); A.ctg_off = ctg_off.data(); A.ctg_len = ctg_len.data(); A.n_ctg = (int32_t)ctg_off.size(); A.o = o;
	A.chain_read = chain_read.data(); A.w0 = w0.data(); A.wlen2 = wlen2.data(); A.tb0 = tb0.data(); A.qbuf = qbuf.data(); A.ord = ord.data(); A.regs = regs.data(); A.reg_ci = reg_ci.data();
	A.lp = lp.data(); A.rp = rp.data(); A.ctr = ctr; A.big = big.data();
	A.small_chain = (o.flags & CS_ALN_NO_LIGHT_PATHS) ? 0 : csa::SMALL_CHAIN; A.light_max = (o.flags & CS_ALN_NO_LIGHT_PATHS) ? 1 : 64;
	A.purge_cap = (o.flags & CS_ALN_PURGE_FROM_HBM) ? 0 : csa::PURGE_CAP;
	// ---- chain_read_kernel, query_kernel, window_kernel; the scan; the host's look at the bad chains
	for (int64_t r = 0; r < n; ++r) csa::chain_read(A, r);
	for (uint64_t b = 0; b < n_bases; ++b) csa::query_codes(A, b);
	for (int64_t ci = 0; ci < nc; ++ci) if (!csa::chain_window(A, ci)) ++ctr[csa::C_BAD_CHAIN];
	if (ctr[csa::C_BAD_CHAIN]) { fprintf(stderr, "refused: the first seed of %llu chains lies outside the reference\n", ctr[csa::C_BAD_CHAIN]); return 3; }
	{ uint64_t a = 0; for (int64_t ci = 0; ci <= nc; ++ci) { tb0[(size_t)ci] = a; a += wlen2[(size_t)ci]; } }
	const uint64_t t_bytes = tb0[(size_t)nc];
	tbuf.resize((size_t)t_bytes + 1);
	A.tbuf = tbuf.data();
	// ---- fill_kernel, region_kernel, region_big_kernel (the long chains' list is made first: the lanes here have no atomics)
	for (int64_t ci = 0; ci < nc; ++ci) if ((int64_t)(cseed_off[(size_t)ci + 1] - cseed_off[(size_t)ci]) > A.small_chain) big[ctr[csa::C_BIG_CHAINS]++] = (uint32_t)ci;
	const unsigned long long n_big = ctr[csa::C_BIG_CHAINS];
	auto reserve = [&](int c, unsigned cnt) { const unsigned long long b = ctr[c]; ctr[c] += cnt; return b; };
	bool started = run_lanes([&](int lane) {
		for (int64_t ci = 0; ci < nc; ++ci) csa::fill_window<LANES>(A, ci, lane);
		for (int64_t base = 0; base < nc; base += LANES) {
			const int64_t ci = base + lane;
			int k = 0; bool mine = false; uint32_t nl = 0, nr = 0;
			csa::ChainCtx X = {}; const cs_seed_t *sd = nullptr;
			if (ci < nc) {
				const uint64_t s0 = cseed_off[(size_t)ci];
				k = (int)(cseed_off[(size_t)ci + 1] - s0);
				if (k > 0 && k <= A.small_chain) { mine = true; X = csa::chain_ctx(A, ci); sd = A.cseeds + s0; csa::count_pairs(X, sd, k, nl, nr); }
			}
			uint32_t tl, tr;
			const uint32_t el = csdd::wexcl_sum<LANES>(nl, lane, tl), er = csdd::wexcl_sum<LANES>(nr, lane, tr);
			unsigned long long bl = 0, br = 0;
			if (lane == 0) { if (tl) bl = reserve(csa::C_LEFT, tl); if (tr) br = reserve(csa::C_RIGHT, tr); }
			bl = csdd::wbcast64<LANES>(bl, 0); br = csdd::wbcast64<LANES>(br, 0);
			if (mine) csa::emit_chain(A, X, sd, k, bl + el, br + er);
		}
		for (unsigned long long e = 0; e < n_big; ++e) csa::chain_regions<LANES>(A, (int64_t)big[e], lane, reserve);
	});
	if (!started) return 2;
	const uint64_t n_left = ctr[csa::C_LEFT], n_right = ctr[csa::C_RIGHT];
	if (n_left > (uint64_t)ns || n_right > (uint64_t)ns) { fprintf(stderr, "more pairs than seeds\n"); return 1; }
	// ---- the dynamic programming, each side: band w, then 2w for the pairs apply_kernel sends back.  Matrix and end bonus as cs_aligner_create
	// builds them; the rule is extend.hip's under CS_EXT_VECTOR_ZDROP.
	cso_bsw_params_t P;
	for (int i = 0, k = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) P.mat[k++] = (int8_t)(i == 4 || j == 4 ? -1 : i == j ? o.a : -o.b);
	P.o_del = o.o_del; P.e_del = o.e_del; P.o_ins = o.o_ins; P.e_ins = o.e_ins; P.zdrop = o.zdrop; P.end_bonus = o.pen_clip5;
	const int T = std::max(1, std::min(16, o.threads));
	uint64_t retries = 0; std::atomic<bool> dp_ok{true};
	auto run_side = [&](cs_ext_pair_t *pairs, uint64_t cnt, int is_left, int pen_clip) {
		cs_ext_pair_t *cur = pairs, *nxt = retry.data();
		for (int attempt = 0; attempt < 2 && cnt; ++attempt) {
			const int w = o.w << attempt;
			const int64_t chunk = 256, n_chunks = ((int64_t)cnt + chunk - 1) / chunk;
			cs_for_chunks_(T, n_chunks, [&](int64_t c) {
				for (uint64_t i = (uint64_t)(c * chunk); i < std::min<uint64_t>(cnt, (uint64_t)((c + 1) * chunk)); ++i) {
					const cs_ext_pair_t &p = cur[i];
					cso_bsw_result_t x;
					if (p.qlen < 1 || p.tlen < 0 || p.q_off + (uint64_t)p.qlen > n_bases * 2 || p.t_off + (uint64_t)p.tlen > t_bytes ||
					    cso_extend_pair_rule(&P, cso_bsw_uses_vec_rule(&P, p.qlen, p.tlen, p.h0) ? 3 : 0, p.qlen, A.qbuf + p.q_off, p.tlen, A.tbuf + p.t_off, w, p.h0, &x)) { dp_ok = false; continue; }
					const cs_ext_result_t y = {x.score, x.qle, x.tle, x.gtle, x.gscore, x.max_off};
					res[i] = y;
				}
			});
			uint64_t n_retry = 0;
			for (uint64_t i = 0; i < cnt; ++i) {   // apply_kernel
				const cs_ext_pair_t pr = cur[i];
				const uint32_t g = (uint32_t)pr.reserved;
				cs_alnreg_t a = A.regs[g];
				if (csa::apply_result(A, a, pr, res[i], w, attempt, is_left, pen_clip)) nxt[n_retry++] = pr;
				A.regs[g] = a;
			}
			cnt = n_retry; retries += cnt;
			std::swap(cur, nxt);
		}
	};
	run_side(A.lp, n_left, 1, o.pen_clip5);
	for (uint64_t i = 0; i < n_right; ++i) csa::right_h0(A.rp[i], A.regs);
	run_side(A.rp, n_right, 0, o.pen_clip3);
	if (!dp_ok) { fprintf(stderr, "a pair leaves the buffers or could not be extended\n"); return 1; }
	// ---- seedcov_kernel, purge_kernel, purge_big_kernel's reads
	for (int64_t g = 0; g < ns; ++g) csa::seed_coverage(A, g);
	const uint64_t regs_max = LANES > 1 ? (uint64_t)std::min<int>(LANES, A.light_max) : 0;
	unsigned long long purged = 0, by_regs = 0, by_mem = 0, in_cap = 0;
	started = run_lanes([&](int lane) {
		unsigned long long my = 0;
		for (int64_t r = 0; r < n; ++r) {
			const uint64_t G = reg_off[(size_t)r + 1] - reg_off[(size_t)r];
			if (G < 2) continue;                                     // (a read's first region has nothing in front of it)
			if (G <= regs_max) { csa::purge_read_regs<LANES>(A, r, lane, my); if (lane == 0) ++by_regs; }
			else { csa::purge_read_mem<LANES>(A, r, pflag.data(), lane, my); if (lane == 0) { ++by_mem; in_cap += G <= (uint64_t)A.purge_cap; } }
		}
		if (lane == 0) purged = my;
	});
	if (!started) return 2;
	const std::vector<uint64_t> stat = {n_left, n_right, retries, purged, n_big, by_regs, by_mem, in_cap};
	if (!spill(d + "out_reg_off.bin", reg_off) || !spill(d + "out_regs.bin", regs) || !spill(d + "out_stat.bin", stat)) return 2;
	return 0;
}
