// chain_filter_gpu.hip -- cs_chain_filter_device / cs_chain_filter_gpu: mem_chain_flt + mem_flt_chained_seeds of the reference
// (mapping/comp_seed.cpp:297-412) on the GPU, byte for byte what cs_chain_filter (chain_filter.cpp) returns, which stays the specification.
// A read's work is sequential over its chains (the sort, then the scan down the sorted list), so a read is one lane or one wave:
//   weight_kernel    one lane per input chain: the chain is checked against n_seeds / cseed_off (C_BAD counts what is inconsistent), its
//                    weight (chain_weight of chain_filter.cpp, both sweeps, the cap at 2^30 - 1) and its span on the read are written.
//   classify_kernel  one lane per read: chain_off and the read's length are checked (C_BAD, C_LONG), the threshold table says whether the
//                    read is long enough for the seed test (C_SW), reads of more than LIGHT_MAX chains go to the wave list (all reads
//                    with chains under CS_FLT_WAVE_ONLY).  The host waits for the counters: nothing below runs on inconsistent input.
//   light_kernel     reads of up to LIGHT_MAX chains, one lane each, lists in HBM scratch at the read's own chain slots.
//   wave_kernel      one wave per read of the wave list, lists in LDS up to LDS_CAP chains, else the same code on the HBM scratch
//                    (C_SPILL).  Lane 0 sorts; the scan tests 64 kept chains per step and one ballot finds the first that stops it.
//   sw_kernel        (only if C_SW) one lane per seed of a kept chain of a long read: mem_seed_sw's window, bns_fetch_seq's clip and
//                    striped_sw_score's recurrence with its two quirks, H and E rows interleaved in LDS across the lanes.
//   compact_kernel   two exclusive scans over the per-read counts of kept chains and kept seeds, then one lane per read writes chain_off,
//                    chains (n_seeds after the seed test), cseed_off, cseeds and the scores.
// The sort is klib's introsort as klib_sort.hpp restates it, compiled for the device: among equal weights its order decides which chain
// is kept and which is shadowed, and it is not stable for any n but 2 (the first partition runs whatever n is).  The float compares of the
// scan are the host's expressions; the unit is compiled without fast-math and with -ffp-contract=off like the rest.
// The bodies are chain_filter_scan.hpp's, which tests/cpp/chain_filter_scan_check.cpp runs in this order on the CPU, one lane and 8 / 64
// lanes in lockstep; a kernel here is a grid-stride loop around a body and does the atomics for what the body returns.
#include "dev_stage.hpp"
#include "chain_filter_scan.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

namespace csf {
// the counter words: reads on the wave list, of those the ones with their lists in HBM, inconsistent chains or reads, reads too long, "some
// read needs the seed test", seeds the test scored
enum { C_WAVE, C_SPILL, C_BAD, C_LONG, C_SW, C_SW_SEEDS, C_COUNT };

__global__ void __launch_bounds__(256) weight_kernel(Args A)
{
	for (uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; c < A.n_chains; c += (uint64_t)gridDim.x * blockDim.x)
		if (!chain_weight_of(A, c)) atomicAdd(A.ctr + C_BAD, 1ull);
}

__global__ void __launch_bounds__(256) classify_kernel(Args A)
{
	for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < A.n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		const int v = classify_read(A, r);
		if (v & V_LONG) atomicAdd(A.ctr + C_LONG, 1ull);
		if (v & V_BAD) atomicAdd(A.ctr + C_BAD, 1ull);
		if (v & V_SW) atomicOr(A.ctr + C_SW, 1ull);
		if (v & V_WAVE) A.wave_list[atomicAdd(A.ctr + C_WAVE, 1ull)] = (uint32_t)r;
	}
}

__global__ void __launch_bounds__(256) light_kernel(Args A)
{
	if (A.flags & CS_FLT_WAVE_ONLY) return;
	for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < A.n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		const uint64_t c0 = A.chain_off[r], nc = A.chain_off[r + 1] - c0;
		if (nc == 0 || nc > (uint64_t)LIGHT_MAX) continue;
		filter_read<1>(A, r, 0, A.srt + c0, A.span + c0, A.alt + c0, A.ki + c0, A.kfirst + c0, A.keptv + c0);
	}
}

__global__ void __launch_bounds__(64) wave_kernel(Args A)
{
	__shared__ WRec s_srt[LDS_CAP]; __shared__ Iv s_span[LDS_CAP]; __shared__ int32_t s_ki[LDS_CAP], s_kfirst[LDS_CAP]; __shared__ uint8_t s_alt[LDS_CAP], s_keptv[LDS_CAP];
	const unsigned long long n = A.ctr[C_WAVE];
	const int lane = threadIdx.x;
	for (unsigned long long w = blockIdx.x; w < n; w += gridDim.x) {
		const int64_t r = A.wave_list[w];
		const uint64_t c0 = A.chain_off[r], nc = A.chain_off[r + 1] - c0;
		if (nc <= (uint64_t)LDS_CAP) filter_read<64>(A, r, lane, s_srt, s_span, s_alt, s_ki, s_kfirst, s_keptv);
		else {
			if (lane == 0) atomicAdd(A.ctr + C_SPILL, 1ull);
			filter_read<64>(A, r, lane, A.srt + c0, A.span + c0, A.alt + c0, A.ki + c0, A.kfirst + c0, A.keptv + c0);
		}
		__syncthreads();
	}
}

// one lane per input seed; H and E as the 16-bit halves of one LDS word per query position, the query's codes beside them, all interleaved
// across the wave's lanes
__global__ void __launch_bounds__(64) sw_kernel(Args A)
{
	__shared__ uint32_t he[SW_MAX * 64];
	__shared__ uint8_t qs[SW_MAX * 64];
	const int lane = threadIdx.x;
	for (uint64_t s0 = (uint64_t)blockIdx.x * 64; s0 < A.n_seeds; s0 += (uint64_t)gridDim.x * 64) {
		const uint64_t s = s0 + lane;
		int64_t c = 0, r = 0; int min_hsp = 0;
		if (s < A.n_seeds && seed_owner(A, s, &c, &r, &min_hsp)) {
			bool ran;
			const int32_t score = seed_sw_score(A, r, s, min_hsp, he + lane, qs + lane, 64, &ran);
			A.sscore[s] = score;
			if (score == DROPPED) {
				atomicAdd((unsigned long long *)A.nsd + r, ~0ull);
				atomicSub(A.cns + c, 1);
			}
			if (ran) atomicAdd(A.ctr + C_SW_SEEDS, 1ull);
		}
	}
}

__global__ void __launch_bounds__(256) compact_kernel(Args A)
{
	for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < A.n_reads; r += (int64_t)gridDim.x * blockDim.x) compact_read(A, r);
}
} // namespace csf

struct cs_chainer_flt_gpu : cs_dev_stage {
	int n_ctg = 0; cs_flt_stats_t st = {};
	bool tab_uploaded = false, have_pac = false; int32_t tab_a = 0, tab_mcw = 0; std::vector<int32_t> tab;
	std::vector<cs_chain_t> h_chains; std::vector<uint64_t> h_chain_off, h_cseed_off; std::vector<cs_seed_t> h_cseeds; std::vector<int32_t> h_score;   // cs_chain_filter_gpu's result
	DevBuf<int64_t> ctg_off; DevBuf<int32_t> ctg_len, d_tab; DevBuf<uint8_t> pac;              // contig table: once; the threshold table; the reference when a seed test needs it
	DevBuf<int32_t> w, cb, ce, cns, ki, kfirst; DevBuf<uint8_t> kflag, alt, keptv; DevBuf<csf::WRec> srt; DevBuf<csf::Iv> span; DevBuf<uint32_t> ord;   // per chain
	DevBuf<uint64_t> o_cseed_off; DevBuf<cs_chain_t> o_chains;                                // ... and the result's
	DevBuf<uint64_t> nch, nsd, o_chain_off, sbase; DevBuf<uint32_t> wave_list;                // per read
	DevBuf<int32_t> sscore, o_score; DevBuf<cs_seed_t> o_cseeds; DevBuf<unsigned long long> ctr;   // per seed; the counters
	DevBuf<uint64_t> in_chain_off, in_cseed_off, in_read_off; DevBuf<cs_chain_t> in_chains; DevBuf<cs_seed_t> in_cseeds; DevBuf<uint8_t> in_bases;   // cs_chain_filter_gpu's uploads
};
static_assert(csf::C_COUNT <= cs_chainer_flt_gpu::N_CTR, "the stage's pinned counter block holds the pass's counters");

void cs_chainer_flt_gpu_release_(cs_chainer_flt_gpu *g) { cs_dev_stage_delete_(g); }

namespace {
int flt_init(cs_chainer *c)
{
	return cs_dev_stage_make_(&c->flt, cs_chainer_gpu_device_(c->gpu), true, [&](cs_chainer_flt_gpu &g) {
		const cs_refseq_view &R = c->ref;   // contig offsets and lengths, once
		g.n_ctg = (int)R.offset.size();
		if (int rc = g.ctg_off.ensure(R.offset.size(), 8)) return rc;
		if (int rc = g.ctg_len.ensure(R.len.size(), 4)) return rc;
		HIP_TRY(hipMemcpy(g.ctg_off.p, R.offset.data(), R.offset.size() * sizeof(int64_t), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(g.ctg_len.p, R.len.data(), R.len.size() * sizeof(int32_t), hipMemcpyHostToDevice));
		return CS_OK;
	});
}

// the threshold table (csf::fill_table), rebuilt when a or min_chain_weight change
void build_table(cs_chainer_flt_gpu &G, const cs_flt_params_t &o)
{
	if (!G.tab.empty() && G.tab_a == o.a && G.tab_mcw == o.min_chain_weight) return;
	G.tab.resize((size_t)csf::MAX_READ_LEN);
	csf::fill_table(o, G.tab.data());
	G.tab_uploaded = false; G.tab_a = o.a; G.tab_mcw = o.min_chain_weight;   // (filter_device_ uploads it)
}

int check_call(const char *what, cs_chainer_t *c, const cs_flt_params_t *par, const cs_chain_result_t *in, const uint64_t *read_offsets, uint32_t flags, const cs_chain_result_t *out)
{
	if (!c || !par || !in || !out) return cs_fail_(CS_EINVAL, std::string(what) + ": null argument");
	if (!c->gpu) return cs_fail_(CS_EINVAL, std::string(what) + ": this chainer has no device (create it with cs_chainer_create_device)");
	if (flags & ~CS_FLT_WAVE_ONLY) return cs_fail_(CS_EINVAL, std::string(what) + ": unknown flags");
	if (in->n_reads < 0 || (in->n_reads > 0 && (!in->chain_off || !read_offsets)) || (in->n_chains > 0 && (!in->chains || !in->cseed_off)) || (in->n_seeds > 0 && !in->cseeds))
		return cs_fail_(CS_EINVAL, std::string(what) + ": bad argument");
	if (par->a < 1 || par->b < 0 || par->e_del < 1 || par->e_ins < 1 || par->o_del < 0 || par->o_ins < 0 || par->max_chain_extend < 1) return cs_fail_(CS_EINVAL, std::string(what) + ": bad parameters");
	if (in->n_reads >= 0xffffffffll || in->n_chains >= 0x7fffffffull) return cs_fail_(CS_ERANGE, std::string(what) + ": more than 2^32 reads or 2^31 chains in one call");
	return CS_OK;
}

// both filters over a device-resident batch; the result stays in the filter state's device buffers
int filter_device_(cs_chainer *c, const cs_flt_params_t &o, const cs_chain_result_t &in, const uint8_t *d_bases, const uint64_t *d_ro, uint32_t flags, cs_chain_result_t &out,
                   const int32_t **d_score)
{
	if (int rc = flt_init(c)) return rc;
	cs_chainer_flt_gpu &G = *c->flt;
	HIP_TRY(hipSetDevice(G.device));
	hipStream_t s = G.s;
	const int64_t n = in.n_reads;
	const uint64_t nc = in.n_chains, ns = in.n_seeds;
	if (nc && in.chains == G.o_chains.p) return cs_fail_(CS_EINVAL, "cs_chain_filter_device: the input is this function's own previous output");
	const size_t per_chain = (size_t)nc + 1, per_seed = (size_t)ns + 1, per_read = (size_t)n + 1;
	if (int rc = G.d_tab.ensure((size_t)csf::MAX_READ_LEN)) return rc;
	if (int rc = cs_ensure_each_(per_chain, 0, G.w, G.cb, G.ce, G.cns, G.kflag, G.srt, G.span, G.ki, G.kfirst, G.alt, G.keptv, G.ord, G.o_cseed_off, G.o_chains)) return rc;
	if (int rc = cs_ensure_each_(per_read, 0, G.nch, G.nsd, G.wave_list, G.o_chain_off, G.sbase)) return rc;
	if (int rc = cs_ensure_each_(per_seed, 0, G.o_cseeds, G.o_score)) return rc;
	if (int rc = G.ctr.ensure(G.N_CTR)) return rc;
	build_table(G, o);
	if (!G.tab_uploaded) { HIP_TRY(hipMemcpy(G.d_tab.p, G.tab.data(), (size_t)csf::MAX_READ_LEN * sizeof(int32_t), hipMemcpyHostToDevice)); G.tab_uploaded = true; }
	csf::Args A;
	A.chain_off = in.chain_off; A.cseed_off = in.cseed_off; A.read_off = d_ro; A.chains = in.chains; A.cseeds = in.cseeds; A.bases = d_bases;
	A.n_reads = n; A.n_chains = nc; A.n_seeds = ns; A.flags = flags; A.o = o;
	A.l_pac = c->ref.l_pac; A.ctg_off = G.ctg_off.p; A.ctg_len = G.ctg_len.p; A.n_ctg = G.n_ctg; A.pac = G.pac.p;
	A.tab = G.d_tab.p;
	A.w = G.w.p; A.cb = G.cb.p; A.ce = G.ce.p; A.cns = G.cns.p; A.kflag = G.kflag.p;
	A.srt = G.srt.p; A.span = G.span.p; A.ki = G.ki.p; A.kfirst = G.kfirst.p;
	A.alt = G.alt.p; A.keptv = G.keptv.p; A.ord = G.ord.p; A.sscore = nullptr;
	A.nch = G.nch.p; A.nsd = G.nsd.p; A.wave_list = G.wave_list.p; A.ctr = G.ctr.p;
	A.o_chain_off = G.o_chain_off.p; A.sbase = G.sbase.p; A.o_cseed_off = G.o_cseed_off.p;
	A.o_chains = G.o_chains.p; A.o_cseeds = G.o_cseeds.p; A.o_score = G.o_score.p;
	unsigned long long *h = G.h_ctr.p;
	out.n_reads = n; out.n_chains = 0; out.n_seeds = 0;
	out.chain_off = A.o_chain_off; out.chains = A.o_chains; out.cseed_off = A.o_cseed_off; out.cseeds = A.o_cseeds;
	if (d_score) *d_score = A.o_score;
	if (n == 0) return G.empty_csr(A.o_chain_off, A.o_cseed_off);
	HIP_TRY(hipMemsetAsync(A.ctr, 0, G.N_CTR * sizeof *A.ctr, s));
	HIP_TRY(hipMemsetAsync(A.nch + n, 0, sizeof *A.nch, s));
	HIP_TRY(hipMemsetAsync(A.nsd + n, 0, sizeof *A.nsd, s));
	HIP_TRY(hipEventRecord(G.ev[0], s));
	unsigned launches = 1;
	if (nc) { hipLaunchKernelGGL(csf::weight_kernel, G.grid((int64_t)nc, 256), dim3(256), 0, s, A); ++launches; }
	hipLaunchKernelGGL(csf::classify_kernel, G.grid(n, 256), dim3(256), 0, s, A);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(G.ev[1], s));
	HIP_TRY(hipMemcpyAsync(h, A.ctr, G.N_CTR * sizeof *A.ctr, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const uint64_t n_bad = h[csf::C_BAD], n_long = h[csf::C_LONG], n_wave = h[csf::C_WAVE];
	const bool need_sw = h[csf::C_SW] != 0;
	if (n_bad) return cs_fail_(CS_EINVAL, "cs_chain_filter_device: a chain without seeds, offsets that are not a CSR, or n_seeds that disagrees with cseed_off");
	if (n_long) return cs_fail_(CS_ERANGE, "cs_chain_filter_device: a read of 65,536 bases or more");
	if (need_sw) {   // the seed test reads the reads and the reference
		if (!d_bases) return cs_fail_(CS_EINVAL, "cs_chain_filter_device: the reads are needed for the seed test of long reads");
		if (!G.have_pac) {
			if (c->pac.empty()) { const int rc = cs_load_pac_(c->prefix.c_str(), c->ref.l_pac, c->pac); if (rc != CS_OK) { c->pac.clear(); return rc; } }
			if (int rc = G.pac.ensure(c->pac.size())) return rc;
			HIP_TRY(hipMemcpy(G.pac.p, c->pac.data(), c->pac.size(), hipMemcpyHostToDevice));
			G.have_pac = true;
		}
		A.pac = G.pac.p;
		if (int rc = G.sscore.ensure(per_seed)) return rc;
		A.sscore = G.sscore.p;
	}
	HIP_TRY(hipEventRecord(G.ev[2], s));
	if (!(flags & CS_FLT_WAVE_ONLY)) { hipLaunchKernelGGL(csf::light_kernel, G.grid(n, 256), dim3(256), 0, s, A); ++launches; }
	if (n_wave) { hipLaunchKernelGGL(csf::wave_kernel, dim3((unsigned)std::min<uint64_t>(n_wave, (uint64_t)G.n_cu * 12)), dim3(64), 0, s, A); ++launches; }
	if (need_sw && ns) {
		hipLaunchKernelGGL(csf::sw_kernel, dim3((unsigned)std::min<uint64_t>((ns + 63) / 64, (uint64_t)G.n_cu * 64)), dim3(64), 0, s, A);
		++launches;
	}
	HIP_TRY(hipGetLastError());
	// chain_off and the per-read seed bases: exclusive scans over n + 1 counts (the last one 0: the totals)
	if (int rc = G.scan<uint64_t>(A.nch, A.o_chain_off, A.nsd, A.sbase, (size_t)n + 1, 0)) return rc;
	hipLaunchKernelGGL(csf::compact_kernel, G.grid(n, 256), dim3(256), 0, s, A);
	HIP_TRY(hipGetLastError());
	launches += 3;
	HIP_TRY(hipEventRecord(G.ev[3], s));
	HIP_TRY(hipMemcpyAsync(h, A.o_chain_off + n, sizeof *h, hipMemcpyDeviceToHost, s));   // four totals into the first pinned words
	HIP_TRY(hipMemcpyAsync(h + 1, A.sbase + n, sizeof *h, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h + 2, A.ctr + csf::C_SPILL, sizeof *h, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h + 3, A.ctr + csf::C_SW_SEEDS, sizeof *h, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const uint64_t n_chains_out = h[0], n_seeds_out = h[1], n_spill = h[2], n_sw_seeds = h[3];
	out.n_chains = n_chains_out; out.n_seeds = n_seeds_out;
	G.add_kernel_ms(G.st.kernel_ms);
	G.st.reads += (uint64_t)n; G.st.chains_in += nc; G.st.chains_out += out.n_chains; G.st.seeds_in += ns; G.st.seeds_out += out.n_seeds;
	G.st.wave_reads += n_wave; G.st.spill_reads += n_spill; G.st.sw_seeds += n_sw_seeds; G.st.launches += launches;
	return CS_OK;
}
} // namespace

extern "C" int cs_chain_filter_device(cs_chainer_t *c, const cs_flt_params_t *par, const cs_chain_result_t *d_in, const uint8_t *d_bases, const uint64_t *d_read_offsets,
                                      uint32_t flags, cs_chain_result_t *d_out, const int32_t **d_cseed_score)
{
	if (int rc = check_call("cs_chain_filter_device", c, par, d_in, d_read_offsets, flags, d_out)) return rc;
	return filter_device_(c, *par, *d_in, d_bases, d_read_offsets, flags, *d_out, d_cseed_score);
}

extern "C" int cs_chain_filter_gpu(cs_chainer_t *c, const cs_flt_params_t *par, const cs_chain_result_t *in, const uint8_t *bases, const uint64_t *read_offsets, uint32_t flags,
                                   cs_chain_result_t *out, const int32_t **cseed_score)
{
	if (int rc = check_call("cs_chain_filter_gpu", c, par, in, read_offsets, flags, out)) return rc;
	if (int rc = flt_init(c)) return rc;
	cs_chainer_flt_gpu &G = *c->flt;
	HIP_TRY(hipSetDevice(G.device));
	const int64_t n = in->n_reads;
	if (in->n_chains && in->chains == G.h_chains.data()) return cs_fail_(CS_EINVAL, "cs_chain_filter_gpu: the input is this function's own previous output");
	// the reads are uploaded only when some read with chains is long enough for the seed test (the table is the device's own)
	build_table(G, *par);
	bool need_bases = false;
	for (int64_t r = 0; r < n && !need_bases; ++r) {
		const uint64_t l = read_offsets[r + 1] - read_offsets[r];
		need_bases = l < csf::MAX_READ_LEN && in->chain_off[r + 1] > in->chain_off[r] && G.tab[(size_t)l] != csf::NO_SW;
	}
	if (need_bases && !bases) return cs_fail_(CS_EINVAL, "cs_chain_filter_gpu: the reads are needed for the seed test of long reads");
	cs_chain_result_t d = *in;
	if (n > 0) {
		if (int rc = G.up(G.in_chain_off, in->chain_off, (size_t)n + 1)) return rc;
		if (int rc = G.up(G.in_read_off, read_offsets, (size_t)n + 1)) return rc;
		if (in->n_chains) {
			if (int rc = G.up(G.in_chains, in->chains, (size_t)in->n_chains)) return rc;
			if (int rc = G.up(G.in_cseed_off, in->cseed_off, (size_t)in->n_chains + 1)) return rc;
		}
		if (in->n_seeds) { if (int rc = G.up(G.in_cseeds, in->cseeds, (size_t)in->n_seeds)) return rc; }
		if (need_bases) { if (int rc = G.up(G.in_bases, bases, (size_t)read_offsets[n])) return rc; }
		HIP_TRY(hipStreamSynchronize(G.s));
		d.chain_off = G.in_chain_off.p; d.chains = G.in_chains.p;
		d.cseed_off = G.in_cseed_off.p; d.cseeds = G.in_cseeds.p;
	}
	cs_chain_result_t dr; const int32_t *d_sc = nullptr;
	if (int rc = filter_device_(c, *par, d, need_bases ? G.in_bases.p : nullptr, n > 0 ? G.in_read_off.p : nullptr, flags, dr, &d_sc)) return rc;
	if (int rc = cs_download_chains_(G.s, dr, d_sc, G.h_chain_off, G.h_chains, G.h_cseed_off, G.h_cseeds, &G.h_score, out)) return rc;
	if (cseed_score) *cseed_score = G.h_score.data();
	return CS_OK;
}

extern "C" int cs_chain_filter_stats(const cs_chainer_t *c, cs_flt_stats_t *st)
{
	if (!c || !st) return cs_fail_(CS_EINVAL, "cs_chain_filter_stats: null argument");
	return cs_dev_stage_stats_(c->flt, st);
}
