// align.cpp -- the aligner object behind chaining (SURVEY 8f row 4 as a whole): cs_aligner_create / destroy / stats, the argument checks
// of cs_extend_chains and cs_extend_chains_device (whose work -- mem_chain2aln_across_reads_V2, mapping/comp_seed.cpp:1319-2237 -- runs on the GPU: align_gpu.hip around
// extend.hip) and cs_dedup_regions (dedup.cpp).  Sequences are laid out so that NO per-pair copy is made: the query buffer holds every
// read once forward and once reversed, the target buffer every chain's reference window once forward and once reversed, and a pair is
// four numbers.  Results are the reference's regions field by field (tests/golden/aln1, flt1, ddp1; tests/test_gpu_align.py).
#include "cs_internal.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

struct cs_aligner {
	cs_refseq_view ref;
	std::vector<uint8_t> pac;             // forward strand, four bases per byte, first base in the top bits (bntseq.c:236-237)
	cs_aln_params_t par{};
	cs_extender_t *ext = nullptr; int device = -1; cs_aligner_gpu *gpu = nullptr;   // gpu: the device side of cs_extend_chains (align_gpu.hip)
	std::vector<uint64_t> reg_off; std::vector<cs_alnreg_t> regs;
	std::vector<uint64_t> dd_off; std::vector<cs_alnreg_t> dd_regs; std::vector<int32_t> dd_ncomp;   // cs_dedup_regions' result
	cs_aln_stats_t st{};
	cs_cigar_gpu *cig = nullptr;          // the device side of cs_regions_cigar (cigar_gpu.hip), with its result
	cs_mark_gpu *mrk = nullptr;           // the device side of cs_regions_mark (mark_gpu.hip), with its result
	cs_sam_gpu *sam = nullptr;            // the device side of cs_regions_sam (sam_gpu.hip), with its result
	std::vector<std::string> ctg_names;   // the contigs' names from <prefix>.ann: the SAM stage's RNAME and cs_sam_header's SN
};


extern "C" void cs_aln_params_default(cs_aln_params_t *p)
{
	if (!p) return;
	// mem_opt_init (comp_seed.cpp:26-58)
	p->a = 1; p->b = 4; p->o_del = p->o_ins = 6; p->e_del = p->e_ins = 1; p->pen_clip5 = p->pen_clip3 = 5; p->w = 100; p->zdrop = 100;
	p->threads = 16; p->flags = 0;
}

// the names of <prefix>.ann's contigs (cs_load_contigs_ reads the same lines for the offsets: "gi name [comment]", then "offset len n_ambs")
static int cs_load_contig_names_(const char *prefix, size_t n_seqs, std::vector<std::string> &names)
{
	FILE *fp = fopen((std::string(prefix) + ".ann").c_str(), "r");
	if (!fp) return cs_fail_(CS_EIO, std::string("cannot read ") + prefix + ".ann");
	std::vector<char> line(1 << 16), name(8192);
	bool ok = fgets(line.data(), (int)line.size(), fp) != nullptr;
	names.clear();
	for (size_t i = 0; ok && i < n_seqs; ++i) {
		unsigned gi = 0;
		ok = fscanf(fp, "%u%8191s", &gi, name.data()) == 2 && fgets(line.data(), (int)line.size(), fp) != nullptr;   // the comment up to the end of the line
		if (ok) { names.push_back(name.data()); ok = fgets(line.data(), (int)line.size(), fp) != nullptr; }
	}
	fclose(fp);
	return ok ? CS_OK : cs_fail_(CS_EIO, std::string(prefix) + ".ann is malformed");
}

extern "C" int cs_aligner_create(const char *prefix, int device, const cs_aln_params_t *par, cs_aligner_t **out)
{
	if (!prefix || !out) return cs_fail_(CS_EINVAL, "cs_aligner_create: null argument");
	*out = nullptr;
	cs_aligner *A = new cs_aligner();
	if (par) A->par = *par; else cs_aln_params_default(&A->par);
	const cs_aln_params_t &o = A->par;
	if (o.a < 1 || o.b < 0 || o.e_del < 1 || o.e_ins < 1 || o.o_del < 0 || o.o_ins < 0 || o.w < 1 || o.zdrop < 0 || (o.flags & ~(CS_ALN_NO_LIGHT_PATHS | CS_ALN_PURGE_FROM_HBM))) { delete A; return cs_fail_(CS_EINVAL, "cs_aligner_create: bad scoring parameters or unknown flags"); }
	int rc = cs_load_contigs_(prefix, A->ref);
	if (rc != CS_OK) { delete A; return rc; }
	rc = cs_load_pac_(prefix, A->ref.l_pac, A->pac);
	if (rc != CS_OK) { delete A; return rc; }
	rc = cs_load_contig_names_(prefix, A->ref.offset.size(), A->ctg_names);
	if (rc != CS_OK) { delete A; return rc; }
	cs_ext_params_t xp;
	for (int i = 0, k = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) xp.mat[k++] = (int8_t)(i == 4 || j == 4 ? -1 : i == j ? o.a : -o.b); // bwa_fill_scmat (bwalib/bwa.c:17-29)
	xp.o_del = o.o_del; xp.e_del = o.e_del; xp.o_ins = o.o_ins; xp.e_ins = o.e_ins; xp.zdrop = o.zdrop; xp.end_bonus = o.pen_clip5;
	// mem_chain2aln_across_reads_V2 extends through the reference's vectorised code, whose Z-drop test is ksw_extend2's only at unit gap extensions and zdrop > 0
	// (bandedSWA.cpp ZSCORE8 / ZSCORE16: no gap-extension factor, live at zdrop 0): the stage's regions under -E 2 or -d 0 are that test's (tests/golden/aln2)
	xp.flags = CS_EXT_VECTOR_ZDROP;
	// (the end bonus only enters the band limit, ksw.c:402-410; the reference builds one object per side, with pen_clip5 and pen_clip3,
	// comp_seed.cpp:1702-1708: two extenders are kept when the two differ)
	A->device = device;
	if (device >= 0) { // device -1: an aligner for the host-side passes only (cs_dedup_regions); cs_extend_chains then fails with CS_EDEVICE
		rc = cs_extender_create(device, &xp, &A->ext);
		if (rc != CS_OK) { delete A; return rc; }
	}
	*out = A;
	return CS_OK;
}
extern "C" void cs_aligner_destroy(cs_aligner_t *A)
{
	if (!A) return;
	if (A->gpu) cs_aligner_gpu_release_(A->gpu);
	if (A->cig) cs_cigar_gpu_release_(A->cig);
	if (A->mrk) cs_mark_gpu_release_(A->mrk);
	if (A->sam) cs_sam_gpu_release_(A->sam);
	if (A->ext) cs_extender_destroy(A->ext);
	delete A;
}

extern "C" int cs_extend_chains(cs_aligner_t *A, const cs_chain_result_t *chains, const int32_t *cseed_score, const uint8_t *bases,
                                const uint64_t *read_offsets, cs_aln_result_t *out)
{
	if (A && !A->ext) return cs_fail_(CS_EDEVICE, "cs_extend_chains: this aligner was created without a device (device -1): the extension runs on the GPU only");
	if (!A || !chains || !out || (chains->n_reads > 0 && (!read_offsets || !chains->chain_off)) || (chains->n_chains > 0 && (!chains->chains || !chains->cseed_off)) ||
	    (chains->n_seeds > 0 && (!chains->cseeds || !bases)))
		return cs_fail_(CS_EINVAL, "cs_extend_chains: bad argument");
	if (A->par.pen_clip5 != A->par.pen_clip3) return cs_fail_(CS_EINVAL, "cs_extend_chains: pen_clip5 != pen_clip3 is not supported yet (one extender, one end bonus)");
	for (int64_t r = 0; r < chains->n_reads; ++r) if (chains->chain_off[r + 1] < chains->chain_off[r] || chains->chain_off[r + 1] > chains->n_chains) return cs_fail_(CS_EINVAL, "cs_extend_chains: chain_off is not a CSR offset array");
	for (uint64_t c = 0; c < chains->n_chains; ++c) if (chains->cseed_off[c + 1] < chains->cseed_off[c] || chains->cseed_off[c + 1] > chains->n_seeds || (int64_t)(chains->cseed_off[c + 1] - chains->cseed_off[c]) != (int64_t)chains->chains[c].n_seeds)
		return cs_fail_(CS_EINVAL, "cs_extend_chains: cseed_off does not match the chains' seed counts");
	// everything per chain, seed and read runs on the GPU (align_gpu.hip)
	const int rc = cs_extend_chains_gpu_(&A->gpu, A->device, A->ext, A->ref, A->pac, A->par, chains, cseed_score, bases, read_offsets, A->reg_off, A->regs, A->st);
	if (rc != CS_OK) return rc;
	out->n_reads = chains->n_reads; out->n_regs = A->regs.size(); out->reg_off = A->reg_off.data(); out->regs = A->regs.data();
	return CS_OK;
}

// the same stage over device-resident chains: only what the host can know is checked here, the arrays are checked by kernels (align_gpu.hip)
extern "C" int cs_extend_chains_device(cs_aligner_t *A, const cs_chain_result_t *d_chains, const int32_t *d_cseed_score, const uint8_t *d_bases,
                                       const uint64_t *d_read_offsets, uint32_t flags, cs_aln_result_t *d_out)
{
	if (!A || !d_chains || !d_out) return cs_fail_(CS_EINVAL, "cs_extend_chains_device: null argument");
	if (flags & ~CS_ALN_DEV_COMPACT) return cs_fail_(CS_EINVAL, "cs_extend_chains_device: unknown flags");
	if (d_chains->n_reads < 0 || (d_chains->n_reads > 0 && (!d_read_offsets || !d_chains->chain_off)) || (d_chains->n_chains > 0 && (!d_chains->chains || !d_chains->cseed_off)) ||
	    (d_chains->n_seeds > 0 && (!d_chains->cseeds || !d_bases)))
		return cs_fail_(CS_EINVAL, "cs_extend_chains_device: bad argument");
	if (!A->ext) return cs_fail_(CS_EDEVICE, "cs_extend_chains_device: this aligner was created without a device (device -1): the extension runs on the GPU only");
	if (A->par.pen_clip5 != A->par.pen_clip3) return cs_fail_(CS_EINVAL, "cs_extend_chains_device: pen_clip5 != pen_clip3 is not supported yet (one extender, one end bonus)");
	if (d_chains->n_seeds >= 0x7fffffffull || d_chains->n_chains >= 0xffffffffull) return cs_fail_(CS_ERANGE, "cs_extend_chains_device: more than 2^31 regions in one call");
	return cs_extend_chains_device_gpu_(&A->gpu, A->device, A->ext, A->ref, A->pac, A->par, d_chains, d_cseed_score, d_bases, d_read_offsets, flags, d_out, A->st);
}

extern "C" int cs_dedup_regions(cs_aligner_t *A, const cs_dedup_params_t *par, const cs_aln_result_t *regs, const uint8_t *bases, const uint64_t *read_offsets,
                                cs_aln_result_t *out, const int32_t **n_comp)
{
	if (!A || !par || !regs || !out || (regs->n_reads > 0 && (!regs->reg_off || !read_offsets)) || (regs->n_regs > 0 && (!regs->regs || !bases))) return cs_fail_(CS_EINVAL, "cs_dedup_regions: bad argument");
	if (regs->regs == A->dd_regs.data() && regs->n_regs) return cs_fail_(CS_EINVAL, "cs_dedup_regions: the input is this function's own previous output");
	if (par->max_chain_gap < 0 || !(par->mask_level_redun > 0.f)) return cs_fail_(CS_EINVAL, "cs_dedup_regions: bad parameters");
	const cs_aligner_core core = {&A->ref, &A->pac, &A->par};
	const int rc = cs_dedup_regions_(core, par, regs, bases, read_offsets, A->dd_off, A->dd_regs, A->dd_ncomp);
	if (rc != CS_OK) return rc;
	out->n_reads = regs->n_reads; out->n_regs = A->dd_regs.size(); out->reg_off = A->dd_off.data(); out->regs = A->dd_regs.data();
	if (n_comp) *n_comp = A->dd_ncomp.data();
	return CS_OK;
}

// from regions to CIGAR / NM / MD (mem_reg2aln without primary marking, MAPQ and SAM text): only what the host can know is checked here,
// the arrays are checked by a kernel (cigar_gpu.hip)
extern "C" int cs_regions_cigar(cs_aligner_t *A, const cs_aln_result_t *regs, const uint8_t *bases, const uint64_t *read_offsets, uint32_t flags, cs_cigar_result_t *out)
{
	if (!A || !regs || !out) return cs_fail_(CS_EINVAL, "cs_regions_cigar: null argument");
	if (flags & ~CS_CIGAR_SMALL_SCRATCH) return cs_fail_(CS_EINVAL, "cs_regions_cigar: unknown flags");
	if (regs->n_reads < 0 || (regs->n_reads > 0 && (!regs->reg_off || !read_offsets)) || (regs->n_regs > 0 && (!regs->regs || !bases))) return cs_fail_(CS_EINVAL, "cs_regions_cigar: bad argument");
	if (A->device < 0) return cs_fail_(CS_EDEVICE, "cs_regions_cigar: this aligner was created without a device (device -1): the alignments are made on the GPU only");
	if (regs->n_regs >= 0xffffffffull || regs->n_reads >= 0xffffffffll) return cs_fail_(CS_ERANGE, "cs_regions_cigar: 2^32 regions or reads or more in one call");
	return cs_regions_cigar_gpu_(&A->cig, A->device, A->ref, A->pac, A->par, regs, bases, read_offsets, flags, out);
}
extern "C" int cs_cigar_stats(const cs_aligner_t *A, cs_cigar_stats_t *st)
{
	if (!A || !st) return cs_fail_(CS_EINVAL, "null argument");
	return cs_cigar_gpu_stats_(A->cig, st);
}

// marking, MAPQ, line selection and XA membership (mark_gpu.hip): only what the host can know is checked here, the arrays by a kernel
extern "C" void cs_mark_params_default(cs_mark_params_t *p)
{
	if (!p) return;
	// mem_opt_init (comp_seed.cpp:26-58)
	p->T = 30; p->mapq_coef_len = 50; p->max_xa_hits = 5; p->max_xa_hits_alt = 200; p->min_seed_len = 19; p->mask_level = 0.50f; p->drop_ratio = 0.50f; p->xa_drop_ratio = 0.80f;
}
extern "C" int cs_regions_mark(cs_aligner_t *A, const cs_mark_params_t *par, const cs_aln_result_t *regs, const uint64_t *read_offsets, int64_t id_base, uint32_t flags, cs_mark_result_t *out)
{
	if (!A || !par || !regs || !out) return cs_fail_(CS_EINVAL, "cs_regions_mark: null argument");
	if (flags & ~(CS_MARK_ALL | CS_MARK_NO_MULTI | CS_MARK_KEEP_SUPP_MAPQ | CS_MARK_NO_LIGHT_PATH | CS_MARK_FROM_HBM)) return cs_fail_(CS_EINVAL, "cs_regions_mark: unknown flags");
	if (regs->n_reads < 0 || (regs->n_reads > 0 && (!regs->reg_off || !read_offsets)) || (regs->n_regs > 0 && !regs->regs)) return cs_fail_(CS_EINVAL, "cs_regions_mark: bad argument");
	if (par->mapq_coef_len <= 0) return cs_fail_(CS_EINVAL, "cs_regions_mark: mapq_coef_len <= 0 (that MAPQ formula stays the caller's)");
	if (par->min_seed_len < 0 || par->max_xa_hits < 0 || par->max_xa_hits_alt < 0 || id_base < 0) return cs_fail_(CS_EINVAL, "cs_regions_mark: bad parameters");
	if (A->device < 0) return cs_fail_(CS_EDEVICE, "cs_regions_mark: this aligner was created without a device (device -1): the marks are made on the GPU only");
	if (regs->n_regs >= 0xffffffffull || regs->n_reads >= 0xffffffffll) return cs_fail_(CS_ERANGE, "cs_regions_mark: 2^32 regions or reads or more in one call");
	if (par->mapq_coef_len > 131072) return cs_fail_(CS_ERANGE, "cs_regions_mark: mapq_coef_len above 131,072");
	return cs_regions_mark_gpu_(&A->mrk, A->device, A->ref, A->par, *par, regs, read_offsets, id_base, flags, out);
}
extern "C" int cs_mark_stats(const cs_aligner_t *A, cs_mark_stats_t *st)
{
	if (!A || !st) return cs_fail_(CS_EINVAL, "null argument");
	return cs_mark_gpu_stats_(A->mrk, st);
}

// the SAM text (sam_gpu.hip): only what the host can know is checked here, the arrays by a kernel
extern "C" int cs_regions_sam(cs_aligner_t *A, const cs_sam_params_t *par, const cs_mark_result_t *marks, const uint64_t *reg_off, const cs_cigar_result_t *alns,
                              const uint8_t *bases, const uint64_t *read_offsets, const uint8_t *quals, const char *names, const uint64_t *name_off,
                              const char *comments, const uint64_t *comment_off, cs_sam_result_t *out)
{
	if (!A || !par || !marks || !alns || !out) return cs_fail_(CS_EINVAL, "cs_regions_sam: null argument");
	if (par->flags & ~(CS_SAM_SOFTCLIP | CS_SAM_WAVE_ONLY)) return cs_fail_(CS_EINVAL, "cs_regions_sam: unknown flags");
	if (par->rg_id && strlen(par->rg_id) > 255) return cs_fail_(CS_EINVAL, "cs_regions_sam: an RG id of more than 255 characters");
	const int64_t n = marks->n_reads;
	const uint64_t n_ents = marks->cigar_regs.n_regs;
	if (n < 0 || marks->cigar_regs.n_reads != n || (n > 0 && (!reg_off || !marks->line_off || !marks->cigar_regs.reg_off || !read_offsets || !name_off)) || (marks->n_regs > 0 && !marks->marks) ||
	    (n_ents > 0 && (!marks->cigar_src || !marks->cigar_regs.regs)) || (alns->n_regs > 0 && !alns->alns) || (alns->n_cigar > 0 && !alns->cigar) || (alns->md_bytes > 0 && !alns->md) ||
	    (n > 0 && ((read_offsets[n] > 0 && !bases) || (name_off[n] > 0 && !names))))
		return cs_fail_(CS_EINVAL, "cs_regions_sam: bad argument");
	if (alns->n_regs != n_ents) return cs_fail_(CS_EINVAL, "cs_regions_sam: alns is not cs_regions_cigar's result over marks->cigar_regs (one entry per entry)");
	if (!comments != !comment_off) return cs_fail_(CS_EINVAL, "cs_regions_sam: comments and comment_off come together or not at all");
	if (A->device < 0) return cs_fail_(CS_EDEVICE, "cs_regions_sam: this aligner was created without a device (device -1): the text is made on the GPU only");
	if (n >= 0xffffffffll || marks->n_regs >= 0xffffffffull || marks->n_lines >= 0xffffffffull) return cs_fail_(CS_ERANGE, "cs_regions_sam: 2^32 reads, regions or lines or more in one call");
	return cs_regions_sam_gpu_(&A->sam, A->device, A->ref, A->ctg_names, par->flags, par->rg_id, marks, reg_off, alns, bases, read_offsets, quals, names, name_off, comments, comment_off, out);
}
extern "C" int cs_sam_stats(const cs_aligner_t *A, cs_sam_stats_t *st)
{
	if (!A || !st) return cs_fail_(CS_EINVAL, "null argument");
	return cs_sam_gpu_stats_(A->sam, st);
}
// the result arrays of the last cs_regions_sam / cs_dedup_regions against the caller's (cs_internal.hpp): the mapper's streamed batches
void cs_aligner_sam_exchange_(cs_aligner_t *A, std::vector<uint64_t> &text_off, std::vector<char> &text) { cs_sam_gpu_exchange_(A->sam, text_off, text); }
void cs_aligner_dedup_exchange_(cs_aligner_t *A, std::vector<uint64_t> &reg_off, std::vector<cs_alnreg_t> &regs) { A->dd_off.swap(reg_off); A->dd_regs.swap(regs); }
// bwa_print_sam_hdr (bwalib/bwa.c:406-427) for the aligner's contigs, behind it the read-group line unescaped as bwa_set_rg / bwa_escape do (:429-476)
extern "C" int cs_sam_header(const cs_aligner_t *A, const char *rg_line, char *buf, size_t cap, size_t *need)
{
	if (!A || !need || (!buf && cap)) return cs_fail_(CS_EINVAL, "cs_sam_header: null argument");
	std::string h;
	for (size_t i = 0; i < A->ctg_names.size(); ++i) h += "@SQ\tSN:" + A->ctg_names[i] + "\tLN:" + std::to_string(A->ref.len[i]) + (A->ref.is_alt[i] ? "\tAH:*\n" : "\n");
	if (rg_line) {
		if (strncmp(rg_line, "@RG", 3) != 0 || strchr(rg_line, '\t')) return cs_fail_(CS_EINVAL, "cs_sam_header: the read group line starts with @RG and holds no literal tab (write \\t)");
		std::string rg;
		for (const char *p = rg_line; *p; ++p) {
			if (*p != '\\') { rg += *p; continue; }
			++p;
			if (*p == 't') rg += '\t'; else if (*p == 'n') rg += '\n'; else if (*p == 'r') rg += '\r'; else if (*p == '\\') rg += '\\';
			if (!*p) break;
		}
		if (rg.find("\tID:") == std::string::npos) return cs_fail_(CS_EINVAL, "cs_sam_header: no ID in the read group line");
		h += rg + "\n";
	}
	*need = h.size();
	if (h.size() > cap) return cs_fail_(CS_ERANGE, "cs_sam_header: the buffer is too small");
	if (!h.empty()) memcpy(buf, h.data(), h.size());
	return CS_OK;
}

extern "C" int cs_aligner_stats(const cs_aligner_t *A, cs_aln_stats_t *st)
{
	if (!A || !st) return cs_fail_(CS_EINVAL, "null argument");
	*st = A->st;
	if (A->ext) { cs_ext_stats_t x; if (cs_extender_stats(A->ext, &x) == CS_OK) { st->ext_cells = x.cells; st->ext_kernel_ms = x.kernel_ms; } } // (the extender is this aligner's own)
	return CS_OK;
}
