// mark_gpu.hip -- cs_regions_mark: primary marking, MAPQ, SAM line selection and XA membership for de-duplicated regions on the GPU
// (mem_mark_primary_se, mem_approx_mapq_se, the loop of mem_reg2sam, mem_gen_alt's rule).  The bodies are mark_scan.hpp's, CPU-tested in
// this order by tests/cpp/mark_scan_check.cpp; a kernel here is a grid-stride loop around them.  Kernel boundaries give all ordering: no
// kernel waits for another wave or block, and every loop's trip count follows from what check_read accepted.  Per call:
//   check_kernel      a lane per read: offsets, the regions' bounds, the counts.  The host waits for the verdict.
//   classify_kernel   a lane per read: light (1 .. LIGHT_MAX regions), or heavy (flag[r] = 1); the counters of the paths
//   an exclusive scan of the flags, list_kernel: the heavy reads in order
//   light_kernel      a lane per light read: mark_read<1> and select_read<1> over lists in the lane's own scratch
//   wave_kernel       one one-wave block per heavy read, block-stride: mark_read<64> and select_read<64>; the read's lists in LDS where
//                     it has at most LDS_REGS regions, otherwise (or under CS_MARK_FROM_HBM) in a batch-sized HBM buffer at the read's offset
//   an exclusive scan of the reads' line counts (line_off) and one of the need_cigar flags; compact.hpp's scatter of the regions in
//   rank order, cigar_kernel: the compacted reg_off and each compacted region's index into marks
#include "dev_stage.hpp"
#include "mark_scan.hpp"
#include "compact.hpp"

#include <cmath>

namespace csmk {
constexpr int LIGHT_MAX = 8;                                           // (unmeasured; the chain filter's light path takes 8 chains)
constexpr int LDS_REGS = 512;                                          // ten lists of 512 entries: 20,480 bytes of LDS a block (unmeasured)
enum { C_BAD, C_RANGE, C_LIGHT, C_WAVE, C_HBM, C_XA, C_COUNT };

struct Args {
	In D; Ref R; Par P; unsigned long long *ctr;
	cs_mark_t *marks; cs_alnreg_t *ranked; uint32_t *need, *nslot; uint64_t *nl, *line_off;   // need / nslot: n_regs + 1; nl / line_off: n_reads + 1
	uint32_t *flag, *slot, *heavy; uint64_t n_heavy; int32_t *hbm;
	uint64_t *cig_off; uint32_t *cig_src;
};

__global__ void check_kernel(Args A)
{
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < A.D.n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		const int v = check_read(A.D, A.R, r);
		if (v == V_BAD) atomicOr(&A.ctr[C_BAD], 1ull);
		if (v == V_RANGE) atomicOr(&A.ctr[C_RANGE], 1ull);
	}
}
__global__ void classify_kernel(Args A)
{
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= A.D.n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		if (r == A.D.n_reads) { A.flag[r] = 0; A.nl[r] = 0; A.need[A.D.n_regs] = 0; continue; }   // the scans' totals
		const uint64_t n = A.D.reg_off[r + 1] - A.D.reg_off[r];
		const bool heavy = n > (uint64_t)LIGHT_MAX || (n > 0 && (A.P.flags & CS_MARK_NO_LIGHT_PATH));
		A.flag[r] = heavy ? 1u : 0u;
		if (n == 0) A.nl[r] = 0;
		else if (!heavy) atomicAdd(&A.ctr[C_LIGHT], 1ull);
		else {
			atomicAdd(&A.ctr[C_WAVE], 1ull);
			if (n > (uint64_t)LDS_REGS || (A.P.flags & CS_MARK_FROM_HBM)) atomicAdd(&A.ctr[C_HBM], 1ull);
		}
	}
}
__global__ void list_kernel(Args A)
{
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < A.D.n_reads; r += (int64_t)gridDim.x * blockDim.x)
		if (A.flag[r]) A.heavy[A.slot[r]] = (uint32_t)r;
}
__global__ void light_kernel(Args A)
{
	int32_t lists[WORK_LISTS * LIGHT_MAX];
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < A.D.n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		const uint64_t c0 = A.D.reg_off[r];
		const int n = (int)(A.D.reg_off[r + 1] - c0);
		if (n == 0 || A.flag[r]) continue;                                // (n <= LIGHT_MAX)
		const Work K = work_at(lists, LIGHT_MAX, 0);
		mark_read<1>(A.P, A.R, A.D.regs + c0, n, (uint64_t)(A.P.id_base + r), K, 0);
		int xa = 0;
		A.nl[r] = (uint64_t)select_read<1>(A.P, A.R, A.D.regs + c0, n, K, A.marks + c0, A.ranked + c0, A.need + c0, &xa, 0);
		if (xa) atomicAdd(&A.ctr[C_XA], (unsigned long long)xa);
	}
}
__global__ void __launch_bounds__(64) wave_kernel(Args A)
{
	__shared__ int32_t lds[WORK_LISTS * LDS_REGS];
	const int lane = (int)threadIdx.x;
	for (uint64_t t = blockIdx.x; t < A.n_heavy; t += gridDim.x) {
		const int64_t r = A.heavy[t];
		const uint64_t c0 = A.D.reg_off[r];
		const int n = (int)(A.D.reg_off[r + 1] - c0);                     // (1 <= n < MAX_REGS)
		const Work K = n <= LDS_REGS && !(A.P.flags & CS_MARK_FROM_HBM) ? work_at(lds, LDS_REGS, 0) : work_at(A.hbm, A.D.n_regs, c0);
		mark_read<64>(A.P, A.R, A.D.regs + c0, n, (uint64_t)(A.P.id_base + r), K, lane);
		int xa = 0;
		const int l = select_read<64>(A.P, A.R, A.D.regs + c0, n, K, A.marks + c0, A.ranked + c0, A.need + c0, &xa, lane);
		if (lane == 0) { A.nl[r] = (uint64_t)l; if (xa) atomicAdd(&A.ctr[C_XA], (unsigned long long)xa); }
	}
}
__global__ void cigar_kernel(Args A)
{
	for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < A.D.n_regs + (uint64_t)A.D.n_reads + 1; g += (uint64_t)gridDim.x * blockDim.x) {
		if (g < A.D.n_regs) { if (A.need[g]) A.cig_src[A.nslot[g]] = (uint32_t)g; }
		else { const uint64_t r = g - A.D.n_regs; A.cig_off[r] = A.nslot[A.D.reg_off[r]]; }   // (reg_off[r] <= n_regs: checked)
	}
}
} // namespace csmk

struct cs_mark_gpu : cs_dev_stage {
	cs_mark_stats_t st = {};
	std::vector<cs_mark_t> marks; std::vector<uint64_t> line_off, cig_off; std::vector<cs_alnreg_t> cig_regs; std::vector<uint32_t> cig_src;   // the result
	DevBuf<uint8_t> alt; DevBuf<double> logtab;                                              // the ALT flags and the host's logarithms: once
	DevBuf<uint64_t> reg_off, read_off; DevBuf<cs_alnreg_t> regs; DevBuf<unsigned long long> ctr;   // the call's input, the counters
	DevBuf<cs_mark_t> d_marks; DevBuf<cs_alnreg_t> ranked, d_cig_regs; DevBuf<uint32_t> need, nslot, d_cig_src; DevBuf<int32_t> hbm;   // per region
	DevBuf<uint64_t> nl, d_line_off, d_cig_off; DevBuf<uint32_t> flag, slot, heavy;          // per read
};
static_assert(csmk::C_COUNT <= cs_mark_gpu::N_CTR, "the stage's pinned counter block holds the pass's counters");
static_assert(sizeof(cs_mark_t) == 48, "cs_mark_t is twelve 4-byte words");

void cs_mark_gpu_release_(cs_mark_gpu *g) { cs_dev_stage_delete_(g); }
int cs_mark_gpu_stats_(const cs_mark_gpu *g, cs_mark_stats_t *st) { return cs_dev_stage_stats_(g, st); }

int cs_regions_mark_gpu_(cs_mark_gpu **gp, int device, const cs_refseq_view &R, const cs_aln_params_t &o, const cs_mark_params_t &par, const cs_aln_result_t *regs,
                         const uint64_t *read_offsets, int64_t id_base, uint32_t flags, cs_mark_result_t *out)
{
	using namespace csmk;
	if (int rc = cs_dev_stage_make_(gp, device, true, [&](cs_mark_gpu &g) {
		std::vector<double> logs((size_t)LOG_N);                          // the host's logarithms: what the reference's libm calls return
		for (int k = 0; k < LOG_N; ++k) logs[(size_t)k] = std::log((double)k);
		if (int rc = g.alt.ensure(R.is_alt.size(), 64)) return rc;
		if (int rc = g.logtab.ensure(logs.size())) return rc;
		HIP_TRY(hipMemcpy(g.alt.p, R.is_alt.data(), R.is_alt.size(), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(g.logtab.p, logs.data(), logs.size() * sizeof(double), hipMemcpyHostToDevice));
		return CS_OK;
	})) return rc;
	cs_mark_gpu &G = **gp;
	HIP_TRY(hipSetDevice(G.device));
	hipStream_t s = G.s;
	const int64_t n = regs->n_reads;
	const uint64_t n_regs = regs->n_regs;
	G.marks.clear(); G.line_off.assign((size_t)n + 1, 0); G.cig_off.assign((size_t)n + 1, 0); G.cig_regs.clear(); G.cig_src.clear();
	auto deliver = [&]() {
		out->n_reads = n; out->n_regs = G.marks.size(); out->n_lines = G.line_off[(size_t)n]; out->marks = G.marks.data(); out->line_off = G.line_off.data();
		out->cigar_regs.n_reads = n; out->cigar_regs.n_regs = G.cig_regs.size(); out->cigar_regs.reg_off = G.cig_off.data(); out->cigar_regs.regs = G.cig_regs.data();
		out->cigar_src = G.cig_src.data();
	};
	deliver();
	if (n == 0 || n_regs == 0) {
		if (int rc = cs_check_no_regions_("cs_regions_mark", regs, read_offsets)) return rc;
		G.st.reads += (uint64_t)n;
		return CS_OK;
	}
	const size_t per_reg = (size_t)n_regs + 1, per_read = (size_t)n + 1;
	if (int rc = G.ctr.ensure(cs_mark_gpu::N_CTR)) return rc;
	if (int rc = cs_ensure_each_(per_reg, 0, G.d_marks, G.ranked, G.need, G.nslot, G.d_cig_src, G.d_cig_regs)) return rc;
	if (int rc = cs_ensure_each_(per_read, 0, G.nl, G.d_line_off, G.flag, G.slot, G.heavy, G.d_cig_off)) return rc;
	if (int rc = G.up(G.reg_off, regs->reg_off, per_read)) return rc;
	if (int rc = G.up(G.read_off, read_offsets, per_read)) return rc;
	if (int rc = G.up(G.regs, regs->regs, (size_t)n_regs)) return rc;
	Args A = {};
	A.D = {G.reg_off.p, G.read_off.p, G.regs.p, n, n_regs};
	A.R = {R.l_pac, G.alt.p, (int)R.offset.size(), G.logtab.p};
	A.P = {par, o.a, o.b, o.o_del, o.e_del, o.o_ins, o.e_ins, flags, id_base};
	A.ctr = G.ctr.p;
	A.marks = G.d_marks.p; A.ranked = G.ranked.p; A.need = G.need.p; A.nslot = G.nslot.p;
	A.nl = G.nl.p; A.line_off = G.d_line_off.p; A.flag = G.flag.p; A.slot = G.slot.p; A.heavy = G.heavy.p;
	A.cig_off = G.d_cig_off.p; A.cig_src = G.d_cig_src.p;
	unsigned long long *h = G.h_ctr.p;
	uint64_t launches = 0;
	HIP_TRY(hipMemsetAsync(A.ctr, 0, cs_mark_gpu::N_CTR * sizeof *A.ctr, s));
	HIP_TRY(hipEventRecord(G.ev[0], s));
	hipLaunchKernelGGL(check_kernel, G.grid(n, 256), dim3(256), 0, s, A); ++launches;
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(h, A.ctr, cs_mark_gpu::N_CTR * sizeof *A.ctr, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));                                  // the verdict, before any kernel follows an offset
	if (h[C_BAD]) return cs_fail_(CS_EINVAL, "cs_regions_mark: reg_off / read_offsets are not CSR offset arrays from 0, or a region is purged, unmapped, outside its read or the reference, names no contig or scores below 0");
	if (h[C_RANGE]) return cs_fail_(CS_ERANGE, "cs_regions_mark: a read has 65,536 regions or more, or a region spans more than 131,072 bases");
	hipLaunchKernelGGL(classify_kernel, G.grid(n + 1, 256), dim3(256), 0, s, A); ++launches;
	HIP_TRY(hipGetLastError());
	if (int rc = G.scan<uint32_t>(A.flag, A.slot, per_read, 0u)) return rc;
	HIP_TRY(hipMemcpyAsync(h, A.ctr, cs_mark_gpu::N_CTR * sizeof *A.ctr, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const uint64_t n_light = h[C_LIGHT], n_heavy = h[C_WAVE], n_hbm = h[C_HBM];
	if (n_light) {
		hipLaunchKernelGGL(light_kernel, G.grid(n, 64), dim3(64), 0, s, A); ++launches;
		HIP_TRY(hipGetLastError());
	}
	if (n_heavy) {
		if (n_hbm) { if (int rc = G.hbm.ensure((size_t)WORK_LISTS * (size_t)n_regs, 64)) return rc; }
		A.hbm = G.hbm.p; A.n_heavy = n_heavy;
		hipLaunchKernelGGL(list_kernel, G.grid(n, 256), dim3(256), 0, s, A);
		hipLaunchKernelGGL(wave_kernel, dim3((unsigned)std::min<uint64_t>(n_heavy, (uint64_t)G.n_cu * 8)), dim3(64), 0, s, A); launches += 2;
		HIP_TRY(hipGetLastError());
	}
	if (int rc = G.scan<uint64_t>(A.nl, A.line_off, per_read, 0ull)) return rc;
	if (int rc = G.scan<uint32_t>(A.need, A.nslot, per_reg, 0u)) return rc;
	hipLaunchKernelGGL(csa::scatter_kernel, G.grid((int64_t)n_regs * csa::REG_WORDS, 256), dim3(256), 0, s, (const uint64_t *)A.ranked, n_regs, A.need, A.nslot, (uint64_t *)G.d_cig_regs.p);
	hipLaunchKernelGGL(cigar_kernel, G.grid((int64_t)n_regs + n + 1, 256), dim3(256), 0, s, A); launches += 2;
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(G.ev[1], s));
	HIP_TRY(hipMemcpyAsync(h, A.nslot + n_regs, sizeof *A.nslot, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h + 1, A.ctr + C_XA, sizeof *h, hipMemcpyDeviceToHost, s));
	G.marks.resize((size_t)n_regs);
	HIP_TRY(hipMemcpyAsync(G.marks.data(), A.marks, (size_t)n_regs * sizeof(cs_mark_t), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(G.line_off.data(), A.line_off, per_read * sizeof *A.line_off, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(G.cig_off.data(), A.cig_off, per_read * sizeof *A.cig_off, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const uint64_t n_cig = *(const uint32_t *)h, n_xa = h[1];
	G.cig_regs.resize((size_t)n_cig); G.cig_src.resize((size_t)n_cig);
	if (n_cig) {
		HIP_TRY(hipMemcpyAsync(G.cig_regs.data(), G.d_cig_regs.p, (size_t)n_cig * sizeof(cs_alnreg_t), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemcpyAsync(G.cig_src.data(), A.cig_src, (size_t)n_cig * sizeof *A.cig_src, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
	}
	deliver();
	float ms = 0.f;
	if (hipEventElapsedTime(&ms, G.ev[0], G.ev[1]) == hipSuccess) G.st.kernel_ms += ms; else (void)hipGetLastError();
	G.st.reads += (uint64_t)n; G.st.regions += n_regs; G.st.lines += G.line_off[(size_t)n]; G.st.xa_members += n_xa; G.st.cigar_regions += n_cig;
	G.st.light_reads += n_light; G.st.wave_reads += n_heavy; G.st.hbm_reads += n_hbm; G.st.launches += launches;
	return CS_OK;
}
