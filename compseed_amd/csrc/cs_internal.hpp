// cs_internal.hpp -- declarations shared by the translation units of libcompseed_amd.so (not part of the C ABI)
#pragma once
#include "../../include/compseed_amd.h"
#include <algorithm>
#include <string>
#include <vector>

struct cs_index { // host copy of an index: the arrays behind a cs_index_view_t
	cs_index_view_t v;
	std::vector<uint32_t> bwt;
	std::vector<uint64_t> sa;
};

int cs_fail_(int code, const std::string &msg); // records the calling thread's error message, returns code

// contig table of an index (<prefix>.ann, ALT flags from <prefix>.alt): shared by the chainer and the extension driver
struct cs_refseq_view { int64_t l_pac; std::vector<int64_t> offset; std::vector<int32_t> len; std::vector<uint8_t> is_alt; };
int cs_load_contigs_(const char *prefix, cs_refseq_view &ref);
int cs_load_pac_(const char *prefix, int64_t l_pac, std::vector<uint8_t> &pac); // <prefix>.pac: four bases per byte, first base in the top bits (bntseq.c:236-237)
// The two base decoders exist once, for the host passes and for the kernels of align_gpu.hip and chain_filter_gpu.hip alike (this header is
// also compiled as plain C++, where CS_HD is nothing).  cs_pac_base_ returns int: a narrower return type costs csf::sw_kernel a register.
#ifdef __HIP__
#define CS_HD __host__ __device__
#else
#define CS_HD
#endif
CS_HD inline int cs_pac_base_(const uint8_t *pac, int64_t p) { return (pac[p >> 2] >> ((~p & 3) << 1)) & 3; }
inline uint8_t cs_pac_base_(const std::vector<uint8_t> &pac, int64_t p) { return (uint8_t)cs_pac_base_(pac.data(), p); }
// ASCII -> code as the reference's table does it (nst_nt4_table, bntseq.c:46-63): ACGT in either case 0..3, '-' 5, everything else 4;
// bytes 0..4 are codes already (comp_seed.cpp:2258-2260 converts only bytes above 4)
CS_HD inline uint8_t cs_base_code_(uint8_t c)
{
	if (c <= 4) return c;
	switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; case '-': return 5; default: return 4; }
}

// The device stage states: what they have in common (device, stream, events, pinned counters, rocPRIM's scratch) is cs_dev_stage of
// dev_stage.hpp, whose cs_dev_stage_delete_ is the body of every cs_*_gpu_release_ below.
// the device side of a chainer (chain_gpu.hip: cs_chain_batch_device / cs_chain_batch_gpu)
struct cs_chainer_gpu;
void cs_chainer_gpu_release_(cs_chainer_gpu *g);
int cs_chainer_gpu_device_(const cs_chainer_gpu *g);
// the device side of the chain filters (chain_filter_gpu.hip: cs_chain_filter_device / cs_chain_filter_gpu), made by the first such call
struct cs_chainer_flt_gpu;
void cs_chainer_flt_gpu_release_(cs_chainer_flt_gpu *g);

// the chainer (chain.cpp: cs_chain_batch; chain_filter.cpp: cs_chain_filter)
struct cs_chainer {
	cs_chainer_gpu *gpu = nullptr;                                                                                                       // cs_chainer_create_device only
	cs_chainer_flt_gpu *flt = nullptr;                                                                                                   // ... and after its first device filter call
	cs_refseq_view ref; std::string prefix;
	std::vector<cs_chain_t> chains; std::vector<uint64_t> chain_off, cseed_off; std::vector<cs_seed_t> cseeds;                          // cs_chain_batch's result
	std::vector<uint8_t> pac;                                                                                                            // loaded when cs_chain_filter first needs it
	std::vector<cs_chain_t> f_chains; std::vector<uint64_t> f_chain_off, f_cseed_off; std::vector<cs_seed_t> f_cseeds; std::vector<int32_t> f_score; // cs_chain_filter's
};

// the reads of a part as 16-byte records of 32 bases, made on host threads (host_pack.cpp; bit-identical to pack_reads_kernel's)
void cs_pack_reads_host_(const uint8_t *bases, const uint64_t *offsets, int64_t r0, int64_t n, int64_t lo, int64_t hi, void *rec_out, int threads, int force_scalar);

// the part of an aligner the host-side region passes need (dedup.cpp: mem_sort_dedup_patch)
struct cs_aligner_core { const cs_refseq_view *ref; const std::vector<uint8_t> *pac; const cs_aln_params_t *par; };
int cs_dedup_regions_(const cs_aligner_core &A, const cs_dedup_params_t *par, const cs_aln_result_t *regs, const uint8_t *bases, const uint64_t *read_offsets,
                      std::vector<uint64_t> &out_off, std::vector<cs_alnreg_t> &out_regs, std::vector<int32_t> &out_ncomp);

// the device side of cs_extend_chains (align_gpu.hip): windows, regions, pair lists, result passes and the purge as kernels
struct cs_aligner_gpu;
void cs_aligner_gpu_release_(cs_aligner_gpu *g);
int cs_extend_chains_gpu_(cs_aligner_gpu **gp, int device, cs_extender_t *ext, const cs_refseq_view &R, const std::vector<uint8_t> &pac, const cs_aln_params_t &o,
                          const cs_chain_result_t *chains, const int32_t *cseed_score, const uint8_t *bases, const uint64_t *read_offsets,
                          std::vector<uint64_t> &reg_off, std::vector<cs_alnreg_t> &regs, cs_aln_stats_t &st);
// ... and of cs_extend_chains_device: the same core over the caller's device arrays, behind checking kernels; the result stays on the device
int cs_extend_chains_device_gpu_(cs_aligner_gpu **gp, int device, cs_extender_t *ext, const cs_refseq_view &R, const std::vector<uint8_t> &pac, const cs_aln_params_t &o,
                                 const cs_chain_result_t *d_chains, const int32_t *d_cseed_score, const uint8_t *d_bases, const uint64_t *d_read_offsets, uint32_t flags,
                                 cs_aln_result_t *d_out, cs_aln_stats_t &st);

// the device side of cs_regions_cigar (cigar_gpu.hip): from regions to CIGAR, NM and MD; made by the first call
struct cs_cigar_gpu;
void cs_cigar_gpu_release_(cs_cigar_gpu *g);
int cs_cigar_gpu_stats_(const cs_cigar_gpu *g, cs_cigar_stats_t *st);
int cs_regions_cigar_gpu_(cs_cigar_gpu **gp, int device, const cs_refseq_view &R, const std::vector<uint8_t> &pac, const cs_aln_params_t &o, const cs_aln_result_t *regs,
                          const uint8_t *bases, const uint64_t *read_offsets, uint32_t flags, cs_cigar_result_t *out);
// ... and of cs_regions_mark (mark_gpu.hip): marking, MAPQ, line selection and XA membership, with the state it keeps between calls
struct cs_mark_gpu;
void cs_mark_gpu_release_(cs_mark_gpu *g);
int cs_mark_gpu_stats_(const cs_mark_gpu *g, cs_mark_stats_t *st);
int cs_regions_mark_gpu_(cs_mark_gpu **gp, int device, const cs_refseq_view &R, const cs_aln_params_t &o, const cs_mark_params_t &par, const cs_aln_result_t *regs,
                         const uint64_t *read_offsets, int64_t id_base, uint32_t flags, cs_mark_result_t *out);
// ... and of cs_regions_sam (sam_gpu.hip): the SAM text from marks and alignments; ctg: the contigs' names
struct cs_sam_gpu;
void cs_sam_gpu_release_(cs_sam_gpu *g);
int cs_sam_gpu_stats_(const cs_sam_gpu *g, cs_sam_stats_t *st);
int cs_regions_sam_gpu_(cs_sam_gpu **gp, int device, const cs_refseq_view &R, const std::vector<std::string> &ctg, uint32_t flags, const char *rg_id, const cs_mark_result_t *marks,
                        const uint64_t *reg_off, const cs_cigar_result_t *alns, const uint8_t *bases, const uint64_t *read_offsets, const uint8_t *quals, const char *names,
                        const uint64_t *name_off, const char *comments, const uint64_t *comment_off, cs_sam_result_t *out);
// The stage's host result arrays against the caller's vectors (host only, no copy): what was the stage's result is the caller's from then
// on, and the stage writes its next result into what the caller gave.  A null stage (no call yet) exchanges nothing.
void cs_sam_gpu_exchange_(cs_sam_gpu *g, std::vector<uint64_t> &text_off, std::vector<char> &text);
// The same through an aligner, for the mapper's streamed batches (mapper.hip), and its counterpart for cs_dedup_regions' result: the arrays
// of the last call leave the aligner, so that its next call does not overwrite a result that is still being read.
void cs_aligner_sam_exchange_(cs_aligner_t *a, std::vector<uint64_t> &text_off, std::vector<char> &text);
void cs_aligner_dedup_exchange_(cs_aligner_t *a, std::vector<uint64_t> &reg_off, std::vector<cs_alnreg_t> &regs);

// ---- the host passes' work sharing: fn(k) for k in [0, n_chunks) on T threads, chunks of reads handed out by a counter.  (A read inside a
// repeat costs a hundred times the average in the quadratic passes -- chain filter, dedup --; equal shares left fifteen threads waiting for
// the one that drew them: cs_chain_filter 107 -> 40 ms per million reads on 16 threads.)
#include <atomic>
#include <thread>
template <class F> inline void cs_for_chunks_(int T, int64_t n_chunks, F fn)
{
	if (T <= 1 || n_chunks <= 1) { for (int64_t k = 0; k < n_chunks; ++k) fn(k); return; }
	std::atomic<int64_t> next{0};
	std::vector<std::thread> th;
	const int nt = (int)std::min<int64_t>(T, n_chunks);
	for (int t = 0; t < nt; ++t) th.emplace_back([&]() { for (int64_t k; (k = next.fetch_add(1)) < n_chunks; ) fn(k); });
	for (auto &t : th) t.join();
}
inline int64_t cs_chunk_reads_(int64_t n, int T) { return std::max<int64_t>(256, std::min<int64_t>(2048, n / ((int64_t)T * 8) + 1)); }

