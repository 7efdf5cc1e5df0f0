// align_gpu.hip -- cs_extend_chains = mem_chain2aln_across_reads_V2 (mapping/comp_seed.cpp:1319-2237) with everything per chain, per seed
// and per read on the GPU.  The first version of this driver built the reference windows, the regions and the job lists on host threads
// around the extension kernels (30 M extensions: 0.8 s of kernels inside 6 s of host work); here the chains and the
// reads go up once, and what comes back are the regions:
//   chain_read_kernel   which read a chain belongs to
//   query_kernel        every read as codes, forward and reversed (a left extension reads the reversed prefix, comp_seed.cpp:1525)
//   window_kernel       per chain the reference window its seeds can reach with the gap they can afford (cal_max_gap), clipped to the
//                       strand and to the contig of the first seed (bns_fetch_seq) -> w0, length; a scan gives every window its place
//   fill_kernel         the window's bases from the 2-bit packed reference, forward and reversed (one wave per chain)
//   region_kernel       per chain: its seeds ranked by score (highest first, later ones first among equals: comp_seed.cpp:1440-1458), one
//                       region per seed, its left / right extension appended to the pair lists (a pair's `reserved` word = its region)
//   cs_extend_batch_device  the dynamic programming (extend.hip), band w, then 2w for the pairs apply_kernel sends back (MAX_BAND_TRY 2)
//   apply_kernel        a side's results into the regions: clipped or to the end of the read, truesc, the band used; retry list
//   seedcov_kernel, purge_kernel   comp_seed.cpp:1758-1766 and :2141-2232 (one thread per read walks its regions in extension order)
// Same results as the host driver it replaces, field by field (tests/test_gpu_align.py against the reference's own regions).
// The bodies are align_scan.hpp's, which tests/cpp/align_scan_check.cpp runs in this order on the CPU, one lane and 8 / 64 lanes in
// lockstep; a kernel here is a grid-stride, wave-stride or block-stride loop around a body and does the atomics and the list appends for
// what the body returns.  purge_big_kernel alone keeps its walk here (eight waves around a workgroup barrier: not run on the CPU).
#include "dev_stage.hpp"
#include "align_scan.hpp"
#include "compact.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

namespace csa {
using csdd::wexcl_sum; using csdd::wbcast64;

__global__ void chain_read_kernel(const Args A)
{
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < A.n_reads; r += (int64_t)gridDim.x * blockDim.x) chain_read(A, r);
}
__global__ void query_kernel(const Args A)
{
	for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < A.n_bases; b += (uint64_t)gridDim.x * blockDim.x) query_codes(A, b);
}
__global__ void window_kernel(const Args A)
{
	for (int64_t ci = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ci < A.n_chains; ci += (int64_t)gridDim.x * blockDim.x)
		if (!chain_window(A, ci)) atomicAdd(A.ctr + C_BAD_CHAIN, 1ull);
}
__global__ void fill_kernel(const Args A) // one wave per chain
{
	const int lane = threadIdx.x & 63;
	const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
	for (int64_t ci = wave; ci < A.n_chains; ci += n_waves) fill_window<64>(A, ci, lane);
}
// a chain per lane for the chains of up to SMALL_CHAIN seeds (nearly all); the pair slots of a wave's 64 chains come from one atomic per
// side (one per pair made the two counters the kernel's clock); longer chains go on a list for region_big_kernel
__global__ void region_kernel(const Args A)
{
	const int lane = threadIdx.x & 63;
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < A.n_chains; base += stride) {
		const int64_t ci = base + lane;
		int ns = 0; bool mine = false; uint32_t nl = 0, nr = 0;
		ChainCtx X; const cs_seed_t *sd = nullptr;
		if (ci < A.n_chains) {
			const uint64_t s0 = A.cseed_off[ci];
			ns = (int)(A.cseed_off[ci + 1] - s0);
			if (ns > A.small_chain) A.big[atomicAdd(A.ctr + C_BIG_CHAINS, 1ull)] = (uint32_t)ci;
			else if (ns > 0) { mine = true; X = chain_ctx(A, ci); sd = A.cseeds + s0; count_pairs(X, sd, ns, nl, nr); }
		}
		uint32_t tl, tr;
		const uint32_t el = wexcl_sum<64>(nl, lane, tl), er = wexcl_sum<64>(nr, lane, tr);
		unsigned long long bl = 0, br = 0;
		if (lane == 0) { if (tl) bl = atomicAdd(A.ctr + C_LEFT, (unsigned long long)tl); if (tr) br = atomicAdd(A.ctr + C_RIGHT, (unsigned long long)tr); }
		bl = wbcast64<64>(bl, 0); br = wbcast64<64>(br, 0);
		if (mine) emit_chain(A, X, sd, ns, bl + el, br + er);
	}
}
__global__ void region_big_kernel(const Args A) // one wave per long chain
{
	const int lane = threadIdx.x & 63;
	const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
	const uint64_t n_big = A.ctr[C_BIG_CHAINS];
	for (uint64_t e = wave; e < n_big; e += n_waves)
		chain_regions<64>(A, (int64_t)A.big[e], lane, [&](int c, unsigned n) { return atomicAdd(A.ctr + c, (unsigned long long)n); });
}
__global__ void right_h0_kernel(cs_ext_pair_t *rp, uint64_t n, const cs_alnreg_t *regs)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) right_h0(rp[i], regs);
}
// a side's results into the regions; pairs whose alignment may have been cut by the band go to `retry` (same pair, next try)
__global__ void apply_kernel(const Args A, const cs_ext_pair_t *pairs, const cs_ext_result_t *res, uint64_t n, int w, int attempt, int is_left, int pen_clip, cs_ext_pair_t *retry)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const cs_ext_pair_t pr = pairs[i];
		const uint32_t g = (uint32_t)pr.reserved;
		cs_alnreg_t a = A.regs[g];
		const cs_ext_result_t x = res[i];
		if (apply_result(A, a, pr, x, w, attempt, is_left, pen_clip)) retry[atomicAdd(A.ctr + C_RETRY, 1ull)] = pr;
		A.regs[g] = a;
	}
}
__global__ void seedcov_kernel(const Args A)
{
	for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < A.n_seeds; g += (int64_t)gridDim.x * blockDim.x) seed_coverage(A, g);
}
// reads of up to 64 regions: a wave per read.  Longer reads go on a list for purge_big_kernel.
__global__ void purge_kernel(const Args A)
{
	const int lane = threadIdx.x & 63;
	const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
	unsigned long long my = 0;
	for (int64_t r = wave; r < A.n_reads; r += n_waves) {
		const uint64_t g0 = A.cseed_off[A.chain_off[r]], g1 = A.cseed_off[A.chain_off[r + 1]];
		if (g1 - g0 < 2) continue;                                  // (a read's first region has nothing in front of it)
		if (g1 - g0 > (uint64_t)A.light_max) { if (lane == 0) A.big_reads[atomicAdd(A.ctr + C_BIG_READS, 1ull)] = (uint32_t)r; continue; }
		purge_read_regs<64>(A, r, lane, my);
	}
	if (lane == 0 && my) atomicAdd(A.ctr + C_PURGED, my);
}
// the reads with more than 64 regions (reads inside repeats: hundreds to thousands of regions, and the walk is quadratic): a workgroup of eight
// waves per read, the read's regions and seeds staged in the LDS -- a step of the walk costs LDS round trips instead of HBM ones, 512 earlier
// regions are looked at per round, the affordable gap (two divisions in double precision) comes from a table over the read's length, both
// tests of a step are answered with ONE barrier (every wave casts its two votes, double-buffered), and the reads are handed out by a ticket
// counter (a few reads of 2,000 regions are most of the work).  All 160 KB of a CU's LDS: one read per CU at a time.  A read beyond
// PURGE_CAP regions is the first wave's, from HBM (purge_read_mem).  This walk is the one the CPU program does not run (align_scan.hpp).
#ifndef CS_PURGE_THREADS
#define CS_PURGE_THREADS 512
#endif
constexpr int PB = CS_PURGE_THREADS;   // threads of purge_big_kernel's workgroup
__global__ __launch_bounds__(PB) void purge_big_kernel(const Args A, uint8_t *pflag)
{
	__shared__ PReg l_reg[PURGE_CAP];
	__shared__ cs_seed_t l_seed[PURGE_CAP];
	__shared__ int32_t l_first[PURGE_CAP];
	__shared__ uint8_t l_alive[PURGE_CAP];
	__shared__ int32_t l_gap[PURGE_GAPS];
	__shared__ unsigned long long l_ticket;
	__shared__ uint32_t l_vote[2][PB / 64];
	const cs_aln_params_t &o = A.o;
	const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const uint64_t n_big = A.ctr[C_BIG_READS];
	unsigned long long my = 0;
	for (int x = tid; x < PURGE_GAPS; x += PB) l_gap[x] = affordable_gap(o, x);
	for (;;) {
		__syncthreads();                                            // (the previous read's last LDS reads are done)
		if (tid == 0) l_ticket = atomicAdd(A.ctr + C_TICKET, 1ull);
		__syncthreads();
		const uint64_t e = l_ticket;
		if (e >= n_big) break;
		const int64_t r = (int64_t)A.big_reads[e];
		const uint64_t g0 = A.cseed_off[A.chain_off[r]], g1 = A.cseed_off[A.chain_off[r + 1]];
		if (g1 - g0 > (uint64_t)A.purge_cap) { if (tid < 64) purge_read_mem<64>(A, r, pflag, lane, my); continue; }
		const int G = (int)(g1 - g0), l_query = (int)(A.read_off[r + 1] - A.read_off[r]);
		auto gap_of = [&](int x) { return (unsigned)x < (unsigned)PURGE_GAPS ? l_gap[x] : affordable_gap(o, x); };
		for (int i = tid; i < G; i += PB) { PReg p; cs_seed_t s; int first; purge_load(A, g0, g0 + (uint64_t)i, p, s, first); l_reg[i] = p; l_seed[i] = s; l_first[i] = first; l_alive[i] = 1; }
		__syncthreads();
		for (int g = 1; g < G; ++g) {
			const cs_seed_t sg = l_seed[g];
			bool around = false, rival = false;
			for (int i = tid; i < g && !around; i += PB) around = l_alive[i] && purge_around(sg, l_reg[i], l_query, gap_of);
			for (int v = l_first[g] + tid; v < g && !rival; v += PB) rival = l_alive[v] && purge_rival(sg, l_seed[v]);
			const uint32_t vote = (__ballot(around) ? 1u : 0u) | (__ballot(rival) ? 2u : 0u);
			if (lane == 0) l_vote[g & 1][wv] = vote;
			__syncthreads();
			uint32_t all = 0;
			for (int w = 0; w < PB / 64; ++w) all |= l_vote[g & 1][w];
			if (all != 1u) continue;                                // not inside an earlier region, or defended by a rival
			if (lane == 0) l_alive[g] = 0;                          // (every wave for itself: its own later reads follow its own write)
			if (tid == 0) ++my;
		}
		for (int i = tid; i < G; i += PB) if (!l_alive[i]) { A.regs[g0 + (uint64_t)i].qb = -1; A.regs[g0 + (uint64_t)i].qe = -1; }
	}
	if (lane == 0 && my) atomicAdd(A.ctr + C_PURGED, my);
}

// ---- cs_extend_chains_device: the host waits for the checks' counter, and only then do reg_off_kernel and the kernels above index one
// array by another (the way chain_filter_gpu.hip goes about it)
__global__ void check_reads_kernel(const DevIn D, unsigned long long *bad)
{
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < D.n_reads; r += (int64_t)gridDim.x * blockDim.x) if (check_read(D, r)) atomicAdd(bad, 1ull);
}
__global__ void check_chains_kernel(const DevIn D, unsigned long long *bad)
{
	for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < D.n_chains; c += (uint64_t)gridDim.x * blockDim.x) if (check_chain(D, c)) atomicAdd(bad, 1ull);
}
__global__ void reg_off_kernel(const DevIn D, uint64_t *reg_off) // a read's regions start where its first chain's seeds start; entry n_reads: the total
{
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= D.n_reads; r += (int64_t)gridDim.x * blockDim.x) reg_off[r] = D.cseed_off[D.chain_off[r]];
}
// CS_ALN_DEV_COMPACT: the regions the purge marked (qe <= qb: what comp_seed.cpp:2387-2393 drops) stay behind.  live_kernel, an exclusive
// scan, scatter_kernel and reg_off_live_kernel are compact.hpp's (a device de-duplication would compact its survivors the same way: dedup_pass.hpp).
} // namespace csa

struct cs_aligner_gpu : cs_dev_stage {
	DevBuf<uint8_t> pac; DevBuf<int64_t> ctg_off; DevBuf<int32_t> ctg_len;                   // the packed reference and the contig table: once
	DevBuf<uint64_t> chain_off, cseed_off, read_off; DevBuf<cs_chain_t> chains; DevBuf<cs_seed_t> cseeds; DevBuf<int32_t> score; DevBuf<uint8_t> bases;   // cs_extend_chains' uploads
	DevBuf<uint32_t> chain_read, big, big_reads; DevBuf<int64_t> w0; DevBuf<uint64_t> wlen2, tb0; DevBuf<uint8_t> qbuf, tbuf, pflag;
	DevBuf<uint32_t> ord, reg_ci; DevBuf<cs_alnreg_t> regs; DevBuf<cs_ext_pair_t> lp, rp, retry; DevBuf<cs_ext_result_t> res; DevBuf<unsigned long long> ctr;
	DevBuf<uint64_t> o_reg_off; DevBuf<cs_alnreg_t> o_regs; DevBuf<uint32_t> live, lscan;     // cs_extend_chains_device: reg_off, the compacted regions, the live flags and their scan
};
static_assert(csa::C_COUNT <= cs_aligner_gpu::N_CTR, "the stage's pinned counter block holds the pass's counters");

void cs_aligner_gpu_release_(cs_aligner_gpu *g) { cs_dev_stage_delete_(g); }

namespace {
// -DCS_ALIGN_TIMING: the laps of a call on stderr (each one waits for the stream)
struct Lap {
#ifdef CS_ALIGN_TIMING
	hipStream_t s; const char *who; std::chrono::steady_clock::time_point t_last;
	Lap(hipStream_t s_, const char *who_) : s(s_), who(who_), t_last(std::chrono::steady_clock::now()) {}
	void operator()(const char *what) { (void)hipStreamSynchronize(s); const auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[%s] %-28s %8.1f ms\n", who, what, std::chrono::duration<double, std::milli>(t - t_last).count()); t_last = t; }
#else
	Lap(hipStream_t, const char *) {}
	void operator()(const char *) {}
#endif
};

// the aligner's device state, made by its first call; the packed reference and the contig table go up once
int gpu_state_(cs_aligner_gpu **gp, int device, const cs_refseq_view &R, const std::vector<uint8_t> &pac)
{
	if (int rc = cs_dev_stage_make_(gp, device, false, [&](cs_aligner_gpu &g) {
		if (int rc = g.up(g.pac, pac.data(), pac.size())) return rc;
		if (int rc = g.up(g.ctg_off, R.offset.data(), R.offset.size())) return rc;
		if (int rc = g.up(g.ctg_len, R.len.data(), R.len.size())) return rc;
		HIP_TRY(hipStreamSynchronize(g.s));          // (a failed copy is this call's error, not a later one's)
		return CS_OK;
	})) return rc;
	HIP_TRY(hipSetDevice((*gp)->device));
	return CS_OK;
}

// a batch in device memory: the aligner's own uploads (cs_extend_chains) or the caller's arrays (cs_extend_chains_device)
struct DevBatch { const uint64_t *chain_off, *cseed_off, *read_off; const cs_chain_t *chains; const cs_seed_t *cseeds; const int32_t *score; const uint8_t *bases;
                  int64_t n, nc, ns; uint64_t n_bases; };

// The stage itself, device pointers in: windows, regions, both sides' extensions, seed coverage, purge.  On return the regions lie in
// G.regs in the reference's order (the purge kernels may still be running on the stream) and C_PURGED counts the purged ones; the offsets
// were found consistent by the caller (host loops or checking kernels) and ns > 0.
int extend_core_(cs_aligner_gpu &G, cs_extender_t *ext, const cs_refseq_view &R, const cs_aln_params_t &o, const DevBatch &in, cs_aln_stats_t &st, Lap &lap, const char *who)
{
	hipStream_t s = G.s;
	const int64_t n = in.n, nc = in.nc, ns = in.ns;
	const uint64_t n_bases = in.n_bases;
	if (int rc = cs_ensure_each_((size_t)nc, 64, G.chain_read, G.big)) return rc;
	if (int rc = G.big_reads.ensure((size_t)n, 64)) return rc;
	if (int rc = cs_ensure_each_((size_t)nc + 1, 64, G.w0, G.wlen2, G.tb0)) return rc;
	if (int rc = G.qbuf.ensure((size_t)n_bases * 2, 64)) return rc;
	if (int rc = cs_ensure_each_((size_t)ns, 64, G.ord, G.reg_ci, G.regs, G.lp, G.rp, G.retry, G.res)) return rc;
	if (int rc = G.ctr.ensure(G.N_CTR)) return rc;
	unsigned long long *h = G.h_ctr.p;
	HIP_TRY(hipMemsetAsync(G.ctr.p, 0, G.N_CTR * sizeof *G.ctr.p, s));

	csa::Args A;
	A.chain_off = in.chain_off; A.cseed_off = in.cseed_off; A.read_off = in.read_off;
	A.chains = in.chains; A.cseeds = in.cseeds; A.score = in.score;
	A.bases = in.bases; A.n_reads = n; A.n_chains = nc; A.n_seeds = ns; A.l_pac = R.l_pac; A.n_bases = n_bases;
	A.pac = G.pac.p; A.ctg_off = G.ctg_off.p; A.ctg_len = G.ctg_len.p; A.n_ctg = (int32_t)R.offset.size();
	A.o = o;
	A.chain_read = G.chain_read.p; A.w0 = G.w0.p; A.wlen2 = G.wlen2.p; A.tb0 = G.tb0.p;
	A.qbuf = G.qbuf.p; A.tbuf = nullptr; A.ord = G.ord.p; A.regs = G.regs.p; A.reg_ci = G.reg_ci.p;
	A.lp = G.lp.p; A.rp = G.rp.p; A.ctr = G.ctr.p;
	A.big = G.big.p; A.big_reads = G.big_reads.p;
	A.small_chain = (o.flags & CS_ALN_NO_LIGHT_PATHS) ? 0 : csa::SMALL_CHAIN; A.light_max = (o.flags & CS_ALN_NO_LIGHT_PATHS) ? 1 : 64;
	A.purge_cap = (o.flags & CS_ALN_PURGE_FROM_HBM) ? 0 : csa::PURGE_CAP;

	lap("buffers");
	hipLaunchKernelGGL(csa::chain_read_kernel, G.grid(n), dim3(256), 0, s, A);
	hipLaunchKernelGGL(csa::query_kernel, G.grid((int64_t)n_bases), dim3(256), 0, s, A);
	hipLaunchKernelGGL(csa::window_kernel, G.grid(nc), dim3(256), 0, s, A);
	HIP_TRY(hipGetLastError());
	{ // every window's place in the target buffer: exclusive scan of 2 x length (one element more: the total)
		HIP_TRY(hipMemsetAsync(A.wlen2 + nc, 0, sizeof *A.wlen2, s));
		if (int rc = G.scan<uint64_t>(A.wlen2, A.tb0, (size_t)nc + 1, 0)) return rc;
	}
	HIP_TRY(hipMemcpyAsync(h, A.tb0 + nc, sizeof *h, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h + 1, A.ctr + csa::C_BAD_CHAIN, sizeof *h, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const uint64_t t_bytes = h[0], n_bad_chains = h[1];
	if (n_bad_chains) return cs_fail_(CS_EINVAL, std::string(who) + ": a chain's first seed lies outside the reference");
	lap("queries, windows, scan");
	if (int rc = G.tbuf.ensure((size_t)t_bytes, 64)) return rc;
	A.tbuf = G.tbuf.p;
	hipLaunchKernelGGL(csa::fill_kernel, G.grid(nc * 64), dim3(256), 0, s, A);
	lap("fill");
	hipLaunchKernelGGL(csa::region_kernel, G.grid(nc), dim3(256), 0, s, A);
	hipLaunchKernelGGL(csa::region_big_kernel, dim3((unsigned)G.n_cu * 8), dim3(256), 0, s, A);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(h, A.ctr, 2 * sizeof *h, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const uint64_t n_left = h[csa::C_LEFT], n_right = h[csa::C_RIGHT];
	lap("regions");

	// ---- the dynamic programming (extend.hip), each side: band w, then 2w for the pairs whose path came close to the band's edge
	auto run_side = [&](cs_ext_pair_t *pairs, uint64_t cnt, bool is_left, int pen_clip) -> int {
		cs_ext_pair_t *cur = pairs, *nxt = G.retry.p;
		for (int attempt = 0; attempt < 2 && cnt; ++attempt) { // MAX_BAND_TRY (comp_seed.cpp:423)
			const int w = o.w << attempt;
			const int rc = cs_extend_batch_device(ext, (int64_t)cnt, cur, A.qbuf, n_bases * 2, A.tbuf, t_bytes, w, G.res.p);
			if (rc != CS_OK) return rc;
			st.pairs += cnt; st.launches++;
			HIP_TRY(hipMemsetAsync(A.ctr + csa::C_RETRY, 0, sizeof *A.ctr, s));
			hipLaunchKernelGGL(csa::apply_kernel, G.grid((int64_t)cnt), dim3(256), 0, s, A, (const cs_ext_pair_t *)cur, (const cs_ext_result_t *)G.res.p, cnt, w, attempt, is_left ? 1 : 0, pen_clip, nxt);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(h, A.ctr + csa::C_RETRY, sizeof *h, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
			cnt = h[0]; st.retries += cnt;
			std::swap(cur, nxt);
		}
		return CS_OK;
	};
	if (int rc = run_side(A.lp, n_left, true, o.pen_clip5)) return rc;
	lap("left side");
	if (n_right) { hipLaunchKernelGGL(csa::right_h0_kernel, G.grid((int64_t)n_right), dim3(256), 0, s, A.rp, n_right, (const cs_alnreg_t *)A.regs); HIP_TRY(hipGetLastError()); HIP_TRY(hipStreamSynchronize(s)); }
	if (int rc = run_side(A.rp, n_right, false, o.pen_clip3)) return rc;

	lap("right side");
	hipLaunchKernelGGL(csa::seedcov_kernel, G.grid(ns), dim3(256), 0, s, A);
	lap("seedcov");
	if (int rc = G.pflag.ensure((size_t)ns, 64)) return rc;
	HIP_TRY(hipMemsetAsync(G.pflag.p, 0, (size_t)ns, s));
	hipLaunchKernelGGL(csa::purge_kernel, G.grid(n * 64), dim3(256), 0, s, A);
	lap("purge, light reads");
	hipLaunchKernelGGL(csa::purge_big_kernel, dim3((unsigned)G.n_cu), dim3(csa::PB), 0, s, A, G.pflag.p);
	HIP_TRY(hipGetLastError());
	lap("purge");
	return CS_OK;
}
} // namespace

// cs_extend_chains: host arrays (checked by align.cpp's loops) up, the core, every region down
int cs_extend_chains_gpu_(cs_aligner_gpu **gp, int device, cs_extender_t *ext, const cs_refseq_view &R, const std::vector<uint8_t> &pac, const cs_aln_params_t &o,
                          const cs_chain_result_t *chains, const int32_t *cseed_score, const uint8_t *bases, const uint64_t *read_offsets,
                          std::vector<uint64_t> &reg_off, std::vector<cs_alnreg_t> &regs, cs_aln_stats_t &st)
{
	if (int rc = gpu_state_(gp, device, R, pac)) return rc;
	cs_aligner_gpu &G = **gp;
	hipStream_t s = G.s;
	Lap lap(s, "cs_extend_chains");
	const int64_t n = chains->n_reads, nc = (int64_t)chains->n_chains, ns = (int64_t)chains->n_seeds;
	reg_off.assign((size_t)n + 1, 0);                              // (regs keeps its size from call to call: growing a vector by 200 MB of zeroes took 6 ms per million reads)
	for (int64_t r = 0; r < n; ++r) reg_off[(size_t)r + 1] = chains->cseed_off[chains->chain_off[r + 1]];
	st.reads += (uint64_t)n;
	if (ns == 0) { regs.clear(); return CS_OK; }
	if (ns >= 0x7fffffffll || nc >= 0xffffffffll) return cs_fail_(CS_ERANGE, "cs_extend_chains: more than 2^31 regions in one call");
	const uint64_t n_bases = read_offsets[n];
	if (int rc = G.up(G.chain_off, chains->chain_off, (size_t)n + 1)) return rc;
	if (int rc = G.up(G.cseed_off, chains->cseed_off, (size_t)nc + 1)) return rc;
	if (int rc = G.up(G.read_off, read_offsets, (size_t)n + 1)) return rc;
	if (int rc = G.up(G.chains, chains->chains, (size_t)nc)) return rc;
	if (int rc = G.up(G.cseeds, chains->cseeds, (size_t)ns)) return rc;
	if (cseed_score) { if (int rc = G.up(G.score, cseed_score, (size_t)ns)) return rc; }
	if (int rc = G.up(G.bases, bases, (size_t)n_bases)) return rc;
	lap("uploads");
	const DevBatch in = {G.chain_off.p, G.cseed_off.p, G.read_off.p, G.chains.p, G.cseeds.p, cseed_score ? G.score.p : nullptr, G.bases.p, n, nc, ns, n_bases};
	if (int rc = extend_core_(G, ext, R, o, in, st, lap, "cs_extend_chains")) return rc;
	regs.resize((size_t)ns);
	lap("host resize");
	HIP_TRY(hipMemcpyAsync(regs.data(), G.regs.p, (size_t)ns * sizeof(cs_alnreg_t), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(G.h_ctr.p, G.ctr.p + csa::C_PURGED, sizeof *G.ctr.p, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const uint64_t n_purged = G.h_ctr.p[0];
	lap("download");
	st.purged += n_purged; st.regions += (uint64_t)ns;
	return CS_OK;
}

// cs_extend_chains_device: the caller's device arrays, checked by kernels; the core; reg_off and (CS_ALN_DEV_COMPACT) the live regions
// made on the device.  Host round trips of its own: the checks' counter with n_bases, and at the end the purge counter with n_regs.
int cs_extend_chains_device_gpu_(cs_aligner_gpu **gp, int device, cs_extender_t *ext, const cs_refseq_view &R, const std::vector<uint8_t> &pac, const cs_aln_params_t &o,
                                 const cs_chain_result_t *d_chains, const int32_t *d_cseed_score, const uint8_t *d_bases, const uint64_t *d_read_offsets, uint32_t flags,
                                 cs_aln_result_t *d_out, cs_aln_stats_t &st)
{
	if (int rc = gpu_state_(gp, device, R, pac)) return rc;
	cs_aligner_gpu &G = **gp;
	hipStream_t s = G.s;
	Lap lap(s, "cs_extend_chains_device");
	const int64_t n = d_chains->n_reads, nc = (int64_t)d_chains->n_chains, ns = (int64_t)d_chains->n_seeds;
	if (int rc = G.o_reg_off.ensure((size_t)n + 1)) return rc;
	if (int rc = G.ctr.ensure(G.N_CTR)) return rc;
	unsigned long long *ctr = G.ctr.p, *h = G.h_ctr.p;
	uint64_t *reg_off = G.o_reg_off.p;
	if ((n == 0 && nc > 0) || (nc == 0 && ns > 0)) return cs_fail_(CS_EINVAL, "cs_extend_chains_device: chains without reads or seeds without chains");
	const csa::DevIn D = {d_chains->chain_off, d_chains->cseed_off, d_read_offsets, d_chains->chains, n, (uint64_t)nc, (uint64_t)ns};
	// C_REFUSED: what the checks refuse, C_N_BASES: read_offsets[n_reads]; one small copy, one wait
	HIP_TRY(hipMemsetAsync(ctr, 0, G.N_CTR * sizeof *ctr, s));
	if (n > 0) hipLaunchKernelGGL(csa::check_reads_kernel, G.grid(n), dim3(256), 0, s, D, ctr + csa::C_REFUSED);
	if (nc > 0) hipLaunchKernelGGL(csa::check_chains_kernel, G.grid(nc), dim3(256), 0, s, D, ctr + csa::C_REFUSED);
	HIP_TRY(hipGetLastError());
	if (n > 0) HIP_TRY(hipMemcpyAsync(ctr + csa::C_N_BASES, d_read_offsets + n, sizeof *ctr, hipMemcpyDeviceToDevice, s));
	HIP_TRY(hipMemcpyAsync(h, ctr, 2 * sizeof *ctr, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const uint64_t n_refused = h[csa::C_REFUSED], n_bases = h[csa::C_N_BASES];
	if (n_refused) return cs_fail_(CS_EINVAL, "cs_extend_chains_device: chain_off / cseed_off are not CSR offset arrays from 0 to n_chains / n_seeds that match the chains' seed counts, read_offsets do not start at 0 or decrease, or a read with chains has 65,536 bases or more");
	lap("checks");
	if (n > 0 && nc > 0) { hipLaunchKernelGGL(csa::reg_off_kernel, G.grid(n + 1), dim3(256), 0, s, D, reg_off); HIP_TRY(hipGetLastError()); }
	else HIP_TRY(hipMemsetAsync(reg_off, 0, ((size_t)n + 1) * sizeof *reg_off, s));
	st.reads += (uint64_t)n;
	d_out->n_reads = n; d_out->n_regs = 0; d_out->reg_off = reg_off; d_out->regs = G.regs.p;
	if (ns == 0) { HIP_TRY(hipStreamSynchronize(s)); return CS_OK; }
	const DevBatch in = {d_chains->chain_off, d_chains->cseed_off, d_read_offsets, d_chains->chains, d_chains->cseeds, d_cseed_score, d_bases, n, nc, ns, n_bases};
	if (int rc = extend_core_(G, ext, R, o, in, st, lap, "cs_extend_chains_device")) return rc;
	const cs_alnreg_t *regs = G.regs.p;
	if (flags & CS_ALN_DEV_COMPACT) {
		if (int rc = cs_ensure_each_((size_t)ns + 1, 0, G.live, G.lscan)) return rc;
		if (int rc = G.o_regs.ensure((size_t)ns)) return rc;
		uint32_t *live = G.live.p, *scan = G.lscan.p;
		hipLaunchKernelGGL(csa::live_kernel, G.grid(ns + 1), dim3(256), 0, s, regs, (uint64_t)ns, live);
		HIP_TRY(hipGetLastError());
		if (int rc = G.scan<uint32_t>(live, scan, (size_t)ns + 1, 0)) return rc;
		hipLaunchKernelGGL(csa::scatter_kernel, G.grid(ns * csa::REG_WORDS), dim3(256), 0, s, (const uint64_t *)regs, (uint64_t)ns, (const uint32_t *)live, (const uint32_t *)scan, (uint64_t *)G.o_regs.p);
		hipLaunchKernelGGL(csa::reg_off_live_kernel, G.grid(n + 1), dim3(256), 0, s, reg_off, n, (const uint32_t *)scan, (uint64_t)ns, ctr + csa::C_LIVE);   // (the long chains' count, the same word, has served)
		HIP_TRY(hipGetLastError());
		lap("compaction");
	}
	static_assert(csa::C_LIVE == csa::C_PURGED + 1, "one copy fetches both");
	HIP_TRY(hipMemcpyAsync(h, ctr + csa::C_PURGED, 2 * sizeof *ctr, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const uint64_t n_purged = h[0], n_live = h[1];
	lap("counters");
	st.purged += n_purged; st.regions += (uint64_t)ns;
	if (flags & CS_ALN_DEV_COMPACT) { d_out->n_regs = n_live; d_out->regs = G.o_regs.p; }
	else { d_out->n_regs = (uint64_t)ns; d_out->regs = regs; }
	return CS_OK;
}
