// sam_gpu.hip -- cs_regions_sam: the SAM text of a batch on the GPU (mem_aln2sam, the string part of mem_gen_alt, the unmapped record of
// mem_reg2sam; single-end).  The bodies are sam_scan.hpp's, CPU-tested in this order by tests/cpp/sam_scan_check.cpp; a kernel here is a
// grid-stride or block-stride loop around one of them.  Kernel boundaries give all ordering: no kernel waits for another wave or block,
// and every loop's trip count follows from what the checks accepted.  Per call:
//   check_kernel      a lane per read (check_read) and a lane per cigar_regs entry (check_ent: md_len).  The host waits for the verdict.
//   index_kernel      a lane per read: index_read; the counters of the statistics, summed per lane before they reach the counter words
//   size_kernel       a lane per read: emit_read counting -> nb[r], and where each of the read's lines starts (line_pos)
//   an exclusive scan of nb (text_off); the host reads the total and sizes the text by it
//   write_kernel      one wave per RECORD, block-stride over the n_lines lines and then the reads (a read without lines writes its unmapped
//                     record, any other is passed over): emit_line<64> / emit_unmapped<64> storing into the record's own range
// A writer stores only inside its record's range and counts a disagreement with the size pass in C_BROKEN (CS_EDEVICE).
// One path: the first build also had a lane-per-read writer for reads of one record without lists.  It lost on the MI355X -- byte stores of
// one lane do not coalesce -- by a factor of two on main100 (0.26 against 0.11 ms of kernels) and in tools/align_bench.py's default row
// (195 against 98 ms per million reads), so it is gone; CS_SAM_WAVE_ONLY is accepted and changes nothing.
// A wave per read, its first shape, left a batch of few reads with many lines (-a) to a handful of waves: hence a wave per record.
#include "dev_stage.hpp"
#include "sam_scan.hpp"

namespace cssm {
enum { C_BAD, C_BROKEN, C_UNMAPPED, C_XA, C_SA, C_COUNT };

struct Args {
	In D; Index X; unsigned long long *ctr;
	uint64_t *nb, *text_off; char *text;                              // nb / text_off: n_reads + 1
};

__global__ void check_kernel(Args A)
{
	const uint64_t n = (uint64_t)A.D.n_reads;
	for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n + A.D.n_ents; g += (uint64_t)gridDim.x * blockDim.x)
		if ((g < n ? check_read(A.D, (int64_t)g) : check_ent(A.D, g - n, A.X.md_len)) != V_OK) atomicOr(&A.ctr[C_BAD], 1ull);
}
__global__ void index_kernel(Args A)
{
	unsigned long long unmapped = 0, xa = 0, sa = 0;
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= A.D.n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		if (r == A.D.n_reads) { A.nb[r] = 0; continue; }              // the scan's total
		index_read(A.D, A.X, r);
		const unsigned long long p = A.X.n_pri[r];
		unmapped += A.D.line_off[r + 1] == A.D.line_off[r]; xa += A.X.n_xa[r]; sa += p >= 2 ? p * (p - 1) : 0;
	}
	if (unmapped) atomicAdd(&A.ctr[C_UNMAPPED], unmapped);
	if (xa) atomicAdd(&A.ctr[C_XA], xa);
	if (sa) atomicAdd(&A.ctr[C_SA], sa);
}
__global__ void size_kernel(Args A)
{
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < A.D.n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		Sink<1, false> S = {nullptr, 0, 0, 0, 0, false};
		emit_read<1, false>(A.D, A.X, r, S, A.X.line_pos);
		A.nb[r] = S.pos;
	}
}
__global__ void __launch_bounds__(64) write_kernel(Args A)
{
	const uint64_t n_lines = A.D.n_lines, n_items = n_lines + (uint64_t)A.D.n_reads;
	for (uint64_t t = blockIdx.x; t < n_items; t += gridDim.x) {
		const bool line = t < n_lines;
		const int64_t r = line ? (int64_t)A.X.line_read[t] : (int64_t)(t - n_lines);
		const uint64_t l0 = A.D.line_off[r], l1 = A.D.line_off[r + 1], t0 = A.text_off[r];
		if (!line && l1 != l0) continue;                              // a read with lines: they are items of their own
		const uint64_t lo = line ? t0 + A.X.line_pos[t] : t0, hi = line && t + 1 < l1 ? t0 + A.X.line_pos[t + 1] : A.text_off[r + 1];
		Sink<64, true> S = {A.text, lo, hi, lo, (int)threadIdx.x, false};
		if (line) emit_line<64, true>(A.D, A.X, r, t - l0, S); else emit_unmapped<64, true>(A.D, r, S);
		if (S.bad || S.pos != S.hi) atomicAdd(&A.ctr[C_BROKEN], 1ull);
	}
}
} // namespace cssm

struct cs_sam_gpu : cs_dev_stage {
	cs_sam_stats_t st = {};
	std::vector<uint64_t> text_off; std::vector<char> text;                                   // the result
	DevBuf<char> ctg_names; DevBuf<uint32_t> ctg_name_off; DevBuf<uint8_t> ctg_alt;            // the contig table: once
	DevBuf<uint64_t> mark_off, line_off, ent_off, read_off, name_off, comment_off; DevBuf<cs_mark_t> marks; DevBuf<uint32_t> ent_src; DevBuf<cs_alnreg_t> ent_regs;   // the call's input
	DevBuf<cs_aln_t> alns; DevBuf<uint32_t> cigar; DevBuf<char> md, names, comments, rg; DevBuf<uint8_t> bases, quals;
	DevBuf<unsigned long long> ctr; DevBuf<uint32_t> md_len, line_ent, line_read, n_pri, n_xa; DevBuf<uint64_t> line_pos, nb, d_text_off; DevBuf<char> d_text;
};
static_assert(cssm::C_COUNT < cs_sam_gpu::N_CTR, "the stage's pinned counter block holds the pass's counters and the text's size behind them");

void cs_sam_gpu_release_(cs_sam_gpu *g) { cs_dev_stage_delete_(g); }
int cs_sam_gpu_stats_(const cs_sam_gpu *g, cs_sam_stats_t *st) { return cs_dev_stage_stats_(g, st); }
void cs_sam_gpu_exchange_(cs_sam_gpu *g, std::vector<uint64_t> &text_off, std::vector<char> &text) { if (g) { g->text_off.swap(text_off); g->text.swap(text); } }

int cs_regions_sam_gpu_(cs_sam_gpu **gp, int device, const cs_refseq_view &R, const std::vector<std::string> &ctg, uint32_t flags, const char *rg_id, const cs_mark_result_t *marks,
                        const uint64_t *reg_off, const cs_cigar_result_t *alns, const uint8_t *bases, const uint64_t *read_offsets, const uint8_t *quals, const char *names,
                        const uint64_t *name_off, const char *comments, const uint64_t *comment_off, cs_sam_result_t *out)
{
	using namespace cssm;
	if (int rc = cs_dev_stage_make_(gp, device, true, [&](cs_sam_gpu &g) {
		std::string all; std::vector<uint32_t> off(1, 0);
		for (const std::string &s : ctg) { all += s; off.push_back((uint32_t)all.size()); }
		if (int rc = g.ctg_names.ensure(all.size(), 64)) return rc;
		if (int rc = g.ctg_name_off.ensure(off.size())) return rc;
		if (int rc = g.ctg_alt.ensure(R.is_alt.size(), 64)) return rc;
		if (!all.empty()) HIP_TRY(hipMemcpy(g.ctg_names.p, all.data(), all.size(), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(g.ctg_name_off.p, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(g.ctg_alt.p, R.is_alt.data(), R.is_alt.size(), hipMemcpyHostToDevice));
		return CS_OK;
	})) return rc;
	cs_sam_gpu &G = **gp;
	HIP_TRY(hipSetDevice(G.device));
	hipStream_t s = G.s;
	const int64_t n = marks->n_reads;
	const uint64_t n_marks = marks->n_regs, n_ents = marks->cigar_regs.n_regs, n_lines = marks->n_lines;
	G.text_off.assign((size_t)n + 1, 0); G.text.clear();
	auto deliver = [&]() { out->n_reads = n; out->n_lines = n_lines; out->n_bytes = G.text.size(); out->text_off = G.text_off.data(); out->text = G.text.data(); };
	deliver();
	if (n == 0) {
		if (n_marks || n_ents || n_lines) return cs_fail_(CS_EINVAL, "cs_regions_sam: regions or lines without reads");
		return CS_OK;
	}
	const size_t per_read = (size_t)n + 1, rg_len = rg_id ? strlen(rg_id) : 0;
	if (int rc = G.ctr.ensure(cs_sam_gpu::N_CTR)) return rc;
	if (int rc = cs_ensure_each_(per_read, 0, G.n_pri, G.n_xa, G.nb, G.d_text_off)) return rc;
	if (int rc = G.md_len.ensure((size_t)n_ents + 1)) return rc;
	if (int rc = cs_ensure_each_((size_t)n_lines + 1, 0, G.line_ent, G.line_read, G.line_pos)) return rc;
	if (int rc = G.up(G.mark_off, reg_off, per_read)) return rc;
	if (int rc = G.up(G.line_off, marks->line_off, per_read)) return rc;
	if (int rc = G.up(G.ent_off, marks->cigar_regs.reg_off, per_read)) return rc;
	if (int rc = G.up(G.read_off, read_offsets, per_read)) return rc;
	if (int rc = G.up(G.name_off, name_off, per_read)) return rc;
	if (comment_off) { if (int rc = G.up(G.comment_off, comment_off, per_read)) return rc; }
	if (int rc = G.up(G.marks, marks->marks, (size_t)n_marks)) return rc;
	if (int rc = G.up(G.ent_src, marks->cigar_src, (size_t)n_ents)) return rc;
	if (int rc = G.up(G.ent_regs, marks->cigar_regs.regs, (size_t)n_ents)) return rc;
	if (int rc = G.up(G.alns, alns->alns, (size_t)n_ents)) return rc;
	if (int rc = G.up(G.cigar, alns->cigar, (size_t)alns->n_cigar)) return rc;
	if (int rc = G.up(G.md, alns->md, (size_t)alns->md_bytes)) return rc;
	// the byte arrays are as long as their last offsets say; the checking kernel accepts offsets only if they rise from 0 to there
	if (int rc = G.up(G.bases, bases, (size_t)read_offsets[n])) return rc;
	if (quals) { if (int rc = G.up(G.quals, quals, (size_t)read_offsets[n])) return rc; }
	if (int rc = G.up(G.names, names, (size_t)name_off[n])) return rc;
	if (comment_off) { if (int rc = G.up(G.comments, comments, (size_t)comment_off[n])) return rc; }
	if (int rc = G.up(G.rg, rg_id, rg_len)) return rc;
	Args A = {};
	A.D.n_reads = n; A.D.n_marks = n_marks; A.D.n_lines = n_lines; A.D.n_ents = n_ents; A.D.n_cigar = alns->n_cigar; A.D.md_bytes = alns->md_bytes;
	A.D.mark_off = G.mark_off.p; A.D.line_off = G.line_off.p; A.D.ent_off = G.ent_off.p; A.D.read_off = G.read_off.p; A.D.name_off = G.name_off.p; A.D.comment_off = comment_off ? G.comment_off.p : nullptr;
	A.D.marks = G.marks.p; A.D.ent_src = G.ent_src.p; A.D.ent_regs = G.ent_regs.p; A.D.alns = G.alns.p; A.D.cigar = G.cigar.p; A.D.md = G.md.p;
	A.D.bases = G.bases.p; A.D.quals = quals ? G.quals.p : nullptr; A.D.names = G.names.p; A.D.comments = comment_off ? G.comments.p : nullptr;
	A.D.ctg_names = G.ctg_names.p; A.D.ctg_name_off = G.ctg_name_off.p; A.D.ctg_alt = G.ctg_alt.p; A.D.n_ctg = (int)R.offset.size();
	A.D.rg = G.rg.p; A.D.rg_len = (int)rg_len; A.D.flags = flags;
	A.X = {G.md_len.p, G.line_ent.p, G.line_read.p, G.n_pri.p, G.n_xa.p, G.line_pos.p};
	A.ctr = G.ctr.p; A.nb = G.nb.p; A.text_off = G.d_text_off.p;
	unsigned long long *h = G.h_ctr.p;
	uint64_t launches = 0;
	HIP_TRY(hipMemsetAsync(A.ctr, 0, cs_sam_gpu::N_CTR * sizeof *A.ctr, s));
	HIP_TRY(hipEventRecord(G.ev[0], s));
	hipLaunchKernelGGL(check_kernel, G.grid(n + (int64_t)n_ents, 256), dim3(256), 0, s, A); ++launches;
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(h, A.ctr, cs_sam_gpu::N_CTR * sizeof *A.ctr, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));                                  // the verdict, before any kernel follows an offset
	if (h[C_BAD]) return cs_fail_(CS_EINVAL, "cs_regions_sam: the offsets are not CSR arrays from 0 to their counts, a read has 65,536 bases or more, the marks' lines are not numbered in rank order, "
	                                         "cigar_src does not name exactly the marks with a line or an XA membership, or an alignment lacks a contig, a position or a CIGAR or lies outside the arrays");
	hipLaunchKernelGGL(index_kernel, G.grid(n + 1, 256), dim3(256), 0, s, A);
	hipLaunchKernelGGL(size_kernel, G.grid(n, 64), dim3(64), 0, s, A); launches += 2;
	HIP_TRY(hipGetLastError());
	if (int rc = G.scan<uint64_t>(A.nb, A.text_off, per_read, 0ull)) return rc;
	HIP_TRY(hipMemcpyAsync(h, A.ctr, cs_sam_gpu::N_CTR * sizeof *A.ctr, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h + C_COUNT, A.text_off + n, sizeof *A.text_off, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const uint64_t n_bytes = h[C_COUNT];
	if (int rc = G.d_text.ensure((size_t)n_bytes, 64)) return rc;
	A.text = G.d_text.p;
	hipLaunchKernelGGL(write_kernel, dim3((unsigned)std::min<uint64_t>(n_lines + (uint64_t)n, (uint64_t)G.n_cu * 32)), dim3(64), 0, s, A); ++launches;   // (blocks of one wave; 32 a CU: unmeasured)
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(G.ev[1], s));
	HIP_TRY(hipMemcpyAsync(h, A.ctr, cs_sam_gpu::N_CTR * sizeof *A.ctr, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(G.text_off.data(), A.text_off, per_read * sizeof *A.text_off, hipMemcpyDeviceToHost, s));
	G.text.resize((size_t)n_bytes);
	if (n_bytes) HIP_TRY(hipMemcpyAsync(G.text.data(), A.text, (size_t)n_bytes, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	float ms = 0.f;
	if (hipEventElapsedTime(&ms, G.ev[0], G.ev[1]) == hipSuccess) G.st.kernel_ms += ms; else (void)hipGetLastError();
	G.st.launches += launches;
	if (h[C_BROKEN]) { G.text.clear(); G.text_off.assign((size_t)n + 1, 0); deliver(); return cs_fail_(CS_EDEVICE, "cs_regions_sam: a record was written otherwise than counted"); }
	deliver();
	G.st.reads += (uint64_t)n; G.st.lines += n_lines; G.st.unmapped += h[C_UNMAPPED]; G.st.bytes += n_bytes; G.st.xa_entries += h[C_XA]; G.st.sa_entries += h[C_SA];
	return CS_OK;
}
