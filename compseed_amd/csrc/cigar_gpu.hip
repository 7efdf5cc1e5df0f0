// cigar_gpu.hip -- cs_regions_cigar: from regions to CIGAR, NM and MD on the GPU (mem_reg2aln, comp_seed.cpp:811-880, without primary marking,
// MAPQ and SAM text).  The bodies are cigar_scan.hpp's, CPU-tested in this order by tests/cpp/cigar_scan_check.cpp; a kernel here is a
// grid-stride loop around one of them.  Kernel boundaries give all ordering: no kernel waits for another wave or block.  Per call:
//   check_kernel      a lane per read: offsets, lengths, the regions' bounds; rd[g] = the region's read.  The host waits for the verdict.
//   classify_kernel   a lane per region: the empty result, the class, the first band, flag[g] = "a job"
//   per try (at most three): an exclusive scan of the flags, list_kernel (the active regions in order, their backtrack-matrix bytes), a scan
//   of the bytes, which the host reads to cut the jobs into chunks under the scratch budget (SCRATCH_BUDGET: an unmeasured choice; a job
//   above it gets a chunk of its own); per chunk:
//     fill_kernel     one wave per job, block-stride: global_fill<64> into the chunk's scratch (sum_score<64> without DP); H and E in LDS
//                     where the job's qlen + 1 <= LDS_ROWS, otherwise in the block's own rows of an HBM buffer sized by the longest read
//     count_kernel    a lane per job: next_try -- a job that goes round again keeps nothing of this try -- or count_aln; flag[g] = "again"
//     two scans, then finish_kernel, a lane per job: finish_aln into the chunk's CIGAR / MD buffers, which the host appends to the result
// so the CIGARs lie in the order the jobs finished; cs_aln_t's offsets say where.
#include "dev_stage.hpp"
#include "cigar_scan.hpp"

namespace cscg {
constexpr int LDS_ROWS = 1025;                                         // H and E of up to 1,024 read bases: 8,200 bytes of LDS a block (unmeasured)
constexpr uint64_t SCRATCH_BUDGET = 256ull << 20, SMALL_BUDGET = 64ull << 10;
// the counter words; C_BROKEN: walks that left their band and jobs written otherwise than counted (neither may happen: CS_EDEVICE)
enum { C_BAD, C_LONGEST, C_REJECT, C_BROKEN, C_CELLS, C_DP, C_NODP, C_RETRY, C_COUNT };

struct Args {
	In D; Ref R; cs_aln_params_t o; State S; cs_aln_t *alns; unsigned long long *ctr;
	uint32_t *flag, *slot, *jobs; uint64_t *zb, *zoff;                // per try: flag / slot over the regions, the rest over the jobs
	uint64_t a, b; uint8_t *z; int32_t *hbm; int64_t rows;            // the chunk [a, b) of the jobs, its scratch, the blocks' H / E rows
	Counts *cnt; uint64_t *nc, *nmd, *coff, *moff; uint32_t *cigar; char *md; uint64_t c0, m0;
};

__global__ void check_kernel(Args A)
{
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < A.D.n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		uint64_t len;
		if (!check_read(A.D, A.R.l_pac, r, A.S.rd, &len)) atomicOr(&A.ctr[C_BAD], 1ull);
		if (len) atomicMax(&A.ctr[C_LONGEST], (unsigned long long)len);
	}
}
__global__ void classify_kernel(Args A)
{
	for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g <= A.D.n_regs; g += (uint64_t)gridDim.x * blockDim.x) {
		if (g == A.D.n_regs) { A.flag[g] = 0; continue; }             // the scan's total
		int w = 0;
		const int c = classify(A.R, A.o, A.D.regs[g], &w);
		A.S.cls[g] = (uint8_t)c; A.S.w2[g] = w; A.S.tries[g] = 0; A.S.score[g] = 0; A.S.last_sc[g] = -(1 << 30);
		cs_aln_t e; memset(&e, 0, sizeof e);
		e.pos = -1; e.rid = -1; e.nm = c == J_REJECT ? -1 : 0;
		uint64_t *dst = (uint64_t *)&A.alns[g]; const uint64_t *src = (const uint64_t *)&e;   // (the padding too: the records compare as bytes)
		for (int k = 0; k < (int)(sizeof(cs_aln_t) / 8); ++k) dst[k] = src[k];
		A.flag[g] = c == J_JOB ? 1u : 0u;
		if (c == J_REJECT) atomicAdd(&A.ctr[C_REJECT], 1ull);
	}
}
__global__ void list_kernel(Args A)
{
	for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < A.D.n_regs; g += (uint64_t)gridDim.x * blockDim.x)
		if (A.flag[g]) { const uint32_t t = A.slot[g]; A.jobs[t] = (uint32_t)g; A.zb[t] = job_bytes(A.o, A.D.regs[g], A.S.w2[g]); }
}
__global__ void __launch_bounds__(64) fill_kernel(Args A)
{
	__shared__ int32_t lds[2 * LDS_ROWS];
	const int lane = (int)threadIdx.x;
	for (uint64_t t = A.a + blockIdx.x; t < A.b; t += gridDim.x) {
		const uint32_t g = A.jobs[t];
		const cs_alnreg_t x = A.D.regs[g];
		const int w2 = A.S.w2[g];
		const Span S = job_span(A.R, x, A.D.bases + A.D.read_off[A.S.rd[g]]);
		int score;
		if (job_nodp(x, w2)) score = sum_score<64>(S, A.o, lane);
		else {
			const int w = job_band(A.o, x, w2), tlen = (int)(x.re - x.rb);
			int32_t *H = S.qlen + 1 <= LDS_ROWS ? lds : A.hbm + (uint64_t)blockIdx.x * 2 * (uint64_t)A.rows;
			score = global_fill<64>(S, tlen, A.o, w, H, H + S.qlen + 1, A.z + (A.zoff[t] - A.zoff[A.a]), lane);
			if (lane == 0) atomicAdd(&A.ctr[C_CELLS], (unsigned long long)tlen * (unsigned long long)job_ncol(S.qlen, w));
		}
		if (lane == 0) A.S.score[g] = score;
	}
}
__global__ void count_kernel(Args A)
{
	for (uint64_t t = A.a + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < A.b; t += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t g = A.jobs[t];
		const cs_alnreg_t x = A.D.regs[g];
		const int w2 = A.S.w2[g], score = A.S.score[g];
		Counts c = {};
		int nw = 0;
		if (!next_try(A.o, x, w2, score, A.S.last_sc[g], A.S.tries[g], &nw)) {
			A.S.last_sc[g] = score; A.S.w2[g] = nw; A.S.tries[g] += 1; A.flag[g] = 1;
			atomicAdd(&A.ctr[C_RETRY], 1ull);
		} else {
			A.S.tries[g] += 1; A.flag[g] = 0;
			const uint64_t r = A.S.rd[g];
			c = count_aln(A.R, A.o, x, A.D.bases + A.D.read_off[r], (int)(A.D.read_off[r + 1] - A.D.read_off[r]), w2, A.z + (A.zoff[t] - A.zoff[A.a]));
			atomicAdd(&A.ctr[job_nodp(x, w2) ? C_NODP : C_DP], 1ull);
			if (c.flagged) atomicAdd(&A.ctr[C_BROKEN], 1ull);
		}
		A.cnt[t - A.a] = c; A.nc[t - A.a] = A.flag[g] ? 0 : c.n_cigar; A.nmd[t - A.a] = A.flag[g] ? 0 : c.md_bytes;
	}
}
__global__ void finish_kernel(Args A)
{
	for (uint64_t t = A.a + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < A.b; t += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t g = A.jobs[t];
		if (A.flag[g]) continue;                                      // goes round again
		const uint64_t r = A.S.rd[g], co = A.coff[t - A.a], mo = A.moff[t - A.a];
		cs_aln_t out; memset(&out, 0, sizeof out);
		out.cigar_off = A.c0 + co; out.md_off = A.m0 + mo;
		if (!finish_aln(A.R, A.o, A.D.regs[g], A.D.bases + A.D.read_off[r], (int)(A.D.read_off[r + 1] - A.D.read_off[r]), A.S.w2[g], A.S.score[g], A.S.tries[g],
		                A.z + (A.zoff[t] - A.zoff[A.a]), A.cnt[t - A.a], A.cigar + co, A.md + mo, &out))
			atomicAdd(&A.ctr[C_BROKEN], 1ull);
		uint64_t *dst = (uint64_t *)&A.alns[g]; const uint64_t *src = (const uint64_t *)&out;
		for (int k = 0; k < (int)(sizeof(cs_aln_t) / 8); ++k) dst[k] = src[k];
	}
}
} // namespace cscg

static_assert(sizeof(cs_aln_t) == 56 && sizeof(cs_aln_t) % 8 == 0, "cs_aln_t is seven 8-byte words");

struct cs_cigar_gpu : cs_dev_stage {
	cs_cigar_stats_t st = {};
	std::vector<cs_aln_t> alns; std::vector<uint32_t> cigar; std::vector<char> md; std::vector<uint64_t> zoff;   // the result, and a try's matrix offsets
	DevBuf<uint8_t> pac; DevBuf<int64_t> ctg;                                                  // the packed reference and the contig offsets: once
	DevBuf<uint64_t> reg_off, read_off; DevBuf<cs_alnreg_t> regs; DevBuf<uint8_t> bases;      // the call's input
	DevBuf<uint32_t> rd; DevBuf<uint8_t> cls; DevBuf<int32_t> w2, tries, score, last_sc; DevBuf<cs_aln_t> d_alns; DevBuf<unsigned long long> ctr;   // per region
	DevBuf<uint32_t> flag, slot, jobs; DevBuf<uint64_t> zb, d_zoff;                            // per try
	DevBuf<uint8_t> z; DevBuf<int32_t> hbm; DevBuf<cscg::Counts> cnt; DevBuf<uint64_t> nc, nmd, coff, moff; DevBuf<uint32_t> d_cigar; DevBuf<char> d_md;   // per chunk
};
constexpr int N_CTRW = cs_cigar_gpu::N_CTR;
static_assert(cscg::C_COUNT <= N_CTRW, "the stage's pinned counter block holds the pass's counters");

void cs_cigar_gpu_release_(cs_cigar_gpu *g) { cs_dev_stage_delete_(g); }
int cs_cigar_gpu_stats_(const cs_cigar_gpu *g, cs_cigar_stats_t *st) { return cs_dev_stage_stats_(g, st); }

int cs_regions_cigar_gpu_(cs_cigar_gpu **gp, int device, const cs_refseq_view &R, const std::vector<uint8_t> &pac, const cs_aln_params_t &o, const cs_aln_result_t *regs,
                          const uint8_t *bases, const uint64_t *read_offsets, uint32_t flags, cs_cigar_result_t *out)
{
	using namespace cscg;
	if (int rc = cs_dev_stage_make_(gp, device, true, [&](cs_cigar_gpu &g) {
		if (int rc = g.pac.ensure(pac.size(), 64)) return rc;
		if (int rc = g.ctg.ensure(R.offset.size(), 8)) return rc;
		HIP_TRY(hipMemcpy(g.pac.p, pac.data(), pac.size(), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(g.ctg.p, R.offset.data(), R.offset.size() * sizeof(int64_t), hipMemcpyHostToDevice));
		return CS_OK;
	})) return rc;
	cs_cigar_gpu &G = **gp;
	HIP_TRY(hipSetDevice(G.device));
	hipStream_t s = G.s;
	const int64_t n = regs->n_reads;
	const uint64_t n_regs = regs->n_regs;
	G.alns.assign((size_t)n_regs, cs_aln_t()); G.cigar.clear(); G.md.assign(1, 0);
	auto deliver = [&]() { out->n_regs = n_regs; out->n_cigar = G.cigar.size(); out->md_bytes = G.md.size(); out->alns = G.alns.data(); out->cigar = G.cigar.data(); out->md = G.md.data(); };
	deliver();
	if (n == 0 || n_regs == 0) return cs_check_no_regions_("cs_regions_cigar", regs, read_offsets);
	const uint64_t n_bases = read_offsets[n];
	const size_t per_reg = (size_t)n_regs + 1, per_read = (size_t)n + 1;
	if (int rc = cs_ensure_each_(per_reg, 0, G.rd, G.cls, G.w2, G.tries, G.score, G.last_sc, G.d_alns, G.flag, G.slot, G.jobs, G.zb, G.d_zoff)) return rc;
	if (int rc = G.ctr.ensure(N_CTRW)) return rc;
	if (int rc = G.up(G.reg_off, regs->reg_off, per_read)) return rc;
	if (int rc = G.up(G.read_off, read_offsets, per_read)) return rc;
	if (int rc = G.up(G.regs, regs->regs, (size_t)n_regs)) return rc;
	if (int rc = G.up(G.bases, bases, (size_t)n_bases)) return rc;
	Args A = {};
	A.D = {G.reg_off.p, G.read_off.p, G.regs.p, G.bases.p, n, n_regs};
	A.R = {R.l_pac, G.pac.p, G.ctg.p, (int)R.offset.size()};
	A.o = o;
	A.S = {G.rd.p, G.cls.p, G.w2.p, G.tries.p, G.score.p, G.last_sc.p};
	A.alns = G.d_alns.p; A.ctr = G.ctr.p;
	A.flag = G.flag.p; A.slot = G.slot.p; A.jobs = G.jobs.p; A.zb = G.zb.p; A.zoff = G.d_zoff.p;
	unsigned long long *h = G.h_ctr.p;
	uint64_t launches = 0;
	HIP_TRY(hipMemsetAsync(A.ctr, 0, N_CTRW * sizeof *A.ctr, s));
	HIP_TRY(hipEventRecord(G.ev[0], s));
	hipLaunchKernelGGL(check_kernel, G.grid(n, 256), dim3(256), 0, s, A); ++launches;
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(h, A.ctr, N_CTRW * sizeof *A.ctr, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));                                  // the verdict, before any kernel follows an offset
	if (h[C_BAD]) return cs_fail_(CS_EINVAL, "cs_regions_cigar: reg_off / read_offsets are not CSR offset arrays from 0, a read with regions has 65,536 bases or more, or a region lies outside its read or the reference");
	const int64_t rows = (int64_t)h[C_LONGEST] + 1;
	const unsigned fill_blocks_max = (unsigned)G.n_cu * 8;             // (blocks of one wave; unmeasured)
	A.rows = rows;
	hipLaunchKernelGGL(classify_kernel, G.grid((int64_t)n_regs + 1, 256), dim3(256), 0, s, A); ++launches;
	HIP_TRY(hipGetLastError());
	const uint64_t budget = (flags & CS_CIGAR_SMALL_SCRATCH) ? SMALL_BUDGET : SCRATCH_BUDGET;
	for (int pass = 0; pass < 3; ++pass) {
		if (int rc = G.scan<uint32_t>(A.flag, A.slot, per_reg, 0u)) return rc;
		HIP_TRY(hipMemcpyAsync(h, A.slot + n_regs, sizeof *A.slot, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		const uint64_t nj = *(const uint32_t *)h;
		if (nj == 0) break;
		hipLaunchKernelGGL(list_kernel, G.grid((int64_t)n_regs, 256), dim3(256), 0, s, A); ++launches;
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemsetAsync(A.zb + nj, 0, sizeof *A.zb, s));
		if (int rc = G.scan<uint64_t>(A.zb, A.zoff, (size_t)nj + 1, 0ull)) return rc;
		G.zoff.resize((size_t)nj + 1);
		HIP_TRY(hipMemcpyAsync(G.zoff.data(), A.zoff, ((size_t)nj + 1) * sizeof *A.zoff, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		const std::vector<uint64_t> &zoff = G.zoff;
		for (uint64_t a = 0; a < nj; ) {                               // chunks under the budget; a job above it has a chunk of its own
			uint64_t b = a + 1;
			while (b < nj && zoff[b + 1] - zoff[a] <= budget) ++b;
			const uint64_t nb = b - a;
			if (int rc = G.z.ensure((size_t)(zoff[b] - zoff[a]), 64)) return rc;
			if (int rc = G.cnt.ensure((size_t)nb)) return rc;
			if (int rc = cs_ensure_each_((size_t)nb + 1, 0, G.nc, G.nmd, G.coff, G.moff)) return rc;
			const unsigned fill_blocks = (unsigned)std::min<uint64_t>(nb, fill_blocks_max);
			// H and E beyond the LDS rows: 2 x (longest read + 1) words for each block of THIS chunk's fill
			if (rows > LDS_ROWS) { if (int rc = G.hbm.ensure((size_t)fill_blocks * 2 * (size_t)rows)) return rc; }
			A.hbm = G.hbm.p;
			A.a = a; A.b = b; A.z = G.z.p; A.cnt = G.cnt.p;
			A.nc = G.nc.p; A.nmd = G.nmd.p; A.coff = G.coff.p; A.moff = G.moff.p;
			HIP_TRY(hipMemsetAsync(A.nc + nb, 0, sizeof *A.nc, s));
			HIP_TRY(hipMemsetAsync(A.nmd + nb, 0, sizeof *A.nmd, s));
			hipLaunchKernelGGL(fill_kernel, dim3(fill_blocks), dim3(64), 0, s, A);
			hipLaunchKernelGGL(count_kernel, G.grid((int64_t)nb, 64), dim3(64), 0, s, A); launches += 2;
			HIP_TRY(hipGetLastError());
			if (int rc = G.scan<uint64_t>(A.nc, A.coff, A.nmd, A.moff, (size_t)nb + 1, 0ull)) return rc;
			HIP_TRY(hipMemcpyAsync(h, A.coff + nb, sizeof *h, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipMemcpyAsync(h + 1, A.moff + nb, sizeof *h, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
			const uint64_t tc = h[0], tm = h[1];
			if (int rc = G.d_cigar.ensure((size_t)tc, 64)) return rc;
			if (int rc = G.d_md.ensure((size_t)tm, 64)) return rc;
			A.cigar = G.d_cigar.p; A.md = G.d_md.p; A.c0 = G.cigar.size(); A.m0 = G.md.size();
			hipLaunchKernelGGL(finish_kernel, G.grid((int64_t)nb, 64), dim3(64), 0, s, A); ++launches;
			HIP_TRY(hipGetLastError());
			G.cigar.resize((size_t)(A.c0 + tc)); G.md.resize((size_t)(A.m0 + tm));
			if (tc) HIP_TRY(hipMemcpyAsync(G.cigar.data() + A.c0, A.cigar, (size_t)tc * sizeof *A.cigar, hipMemcpyDeviceToHost, s));
			if (tm) HIP_TRY(hipMemcpyAsync(G.md.data() + A.m0, A.md, (size_t)tm, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
			a = b;
		}
	}
	HIP_TRY(hipEventRecord(G.ev[1], s));
	HIP_TRY(hipMemcpyAsync(G.alns.data(), A.alns, (size_t)n_regs * sizeof(cs_aln_t), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h, A.ctr, N_CTRW * sizeof *A.ctr, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	deliver();
	float ms = 0.f;
	if (hipEventElapsedTime(&ms, G.ev[0], G.ev[1]) == hipSuccess) G.st.kernel_ms += ms; else (void)hipGetLastError();
	G.st.regions += n_regs; G.st.dp_jobs += h[C_DP]; G.st.nodp_jobs += h[C_NODP]; G.st.retries += h[C_RETRY]; G.st.rejected += h[C_REJECT]; G.st.cells += h[C_CELLS]; G.st.launches += launches;
	if (h[C_BROKEN]) return cs_fail_(CS_EDEVICE, "cs_regions_cigar: a backtrack left its band, or a job was written otherwise than counted");
	if (h[C_REJECT]) return cs_fail_(CS_EINVAL, "cs_regions_cigar: regions that bridge the strands were delivered empty (nm = -1)");
	return CS_OK;
}
