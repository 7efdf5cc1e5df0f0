// mapper.hip -- cs_mapper_t: reads to SAM text in one call (seed_and_extend behind mem_process_seqs, comp_seed.cpp:2239-2420, single-end).
// The unit adds no kernel.  It owns one engine, one device chainer and three aligners on one GPU and the device copy of a batch's reads, and
// it is the one place that knows the order of the stage calls: seeding, chaining, the chain filters and the extension run over the
// device-resident reads and hand device pointers to each other; the live regions come to the host for cs_dedup_regions, and marking, the
// CIGAR stage and the SAM text are the host-array calls of the aligner (each uploads its own copy of the reads: about 450 bytes a read,
// beside a CIGAR stage of 2.9 us a read -- DESIGN.md section 12).  A stage's error is the call's error with the stage's name in front;
// every stage leaves its object usable after an error, so the mapper is too.  Every stage accepts the empty input its predecessor can
// produce (no seeds, no chains, no regions), so no stage is stepped over.
// A batch is three parts -- front (upload .. download), de-duplication, tail (marking, CIGAR, SAM text) -- as three functions.  cs_map_batch
// calls them one after the other; cs_map_submit / cs_map_collect run them on the three worker threads of map_stream.hpp's ring, one per part,
// so that the host's de-duplication of batch n runs beside the device stages of batches n + 1 and n - 1.  Each part
// has objects of its own, an aligner among them, so no stage object is ever under two threads.
#include "dev_stage.hpp"
#include "map_stream.hpp"

#include <chrono>
#include <memory>

namespace {
struct StepClock {   // host wall time of the steps of one batch, added to the mapper's sums when the batch has succeeded
	using clk = std::chrono::steady_clock;
	double ms[CS_MAP_N_STAGES] = {}; clk::time_point t0 = clk::now(), t = t0;   // t0: the call, or the submit
	void start() { t = clk::now(); }                                  // a part begins (in whichever thread runs it)
	void lap(int k) { const clk::time_point n = clk::now(); ms[k] += std::chrono::duration<double, std::milli>(n - t).count(); t = n; }
	void end() { ms[CS_MAP_T_TOTAL] = std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }
};
// A batch on its way: the caller's arrays and the host state the parts hand to each other.  cs_map_batch has one; a streamed batch has its
// slot's (map_stream.hpp), and there the de-duplicated regions are exchanged out of the aligner that made them into dd_off / dd_regs, since
// the de-duplication of the next batch runs beside this batch's tail.
struct MapJob {
	int64_t n = 0, id_base = 0;
	const uint8_t *bases = nullptr; const uint64_t *off = nullptr; const uint8_t *quals = nullptr; const char *names = nullptr; const uint64_t *name_off = nullptr;
	const char *comments = nullptr; const uint64_t *comment_off = nullptr;
	std::vector<uint64_t> reg_off; std::vector<cs_alnreg_t> regs;     // the live regions as the extension left them
	std::vector<uint64_t> dd_off; std::vector<cs_alnreg_t> dd_regs;   // streamed batches only
	cs_aln_result_t live{}, dd{};                                     // front -> de-duplication -> tail
	StepClock T;
};
// what a batch adds to the mapper and, for a streamed batch, its text: the SAM stage's host arrays, exchanged out of the stage
struct MapResult { std::vector<uint64_t> text_off; std::vector<char> text; cs_sam_result_t res{}; cs_map_stats_t add{}; };
using MapRing = map_stream::Ring<MapJob, MapResult>;
} // namespace

struct cs_mapper {
	cs_map_params_t par{}; std::string rg_id;
	cs_params_t seed{}; cs_chain_params_t chain{}; cs_flt_params_t flt{}; cs_aln_params_t aln{}; cs_dedup_params_t dedup{}; cs_mark_params_t mark{};
	uint32_t mark_flags = 0; cs_sam_params_t sam{};
	int device = 0;
	cs_index_t *idx = nullptr; cs_engine_t *eng = nullptr; cs_chainer_t *chn = nullptr;
	// One aligner per part, since an aligner takes one thread at a time: the extension's (front), a host-only one (device -1) for
	// cs_dedup_regions, and the tail's with the marking, CIGAR and SAM stages.  cs_map_batch runs on the same three.
	cs_aligner_t *al = nullptr, *al_dd = nullptr, *al_tail = nullptr;
	HipStream s; DevBuf<uint8_t> d_bases; DevBuf<uint64_t> d_off;     // the batch's reads on the device: uploaded once per batch, the front's alone
	MapJob blk;                                                       // cs_map_batch's batch
	std::vector<uint64_t> no_text_off;                                // text_off of a batch without reads
	cs_map_stats_t st{};
	std::unique_ptr<MapRing> ring;                                    // cs_map_submit / cs_map_collect; owns the three worker threads
};

extern "C" void cs_map_params_default(cs_map_params_t *p)
{
	if (!p) return;
	memset(p, 0, sizeof *p);
	// mem_opt_init (comp_seed.cpp:26-58)
	p->a = 1; p->b = 4; p->o_del = p->o_ins = 6; p->e_del = p->e_ins = 1; p->pen_clip5 = p->pen_clip3 = 5; p->w = 100; p->zdrop = 100;
	p->T = 30;
	p->min_seed_len = 19; p->split_factor = 1.5f; p->split_width = 10; p->max_occ = 500; p->max_mem_intv = 20;
	p->max_chain_gap = 10000; p->max_chain_extend = 1 << 30; p->min_chain_weight = 0;
	p->mask_level = 0.50f; p->drop_ratio = 0.50f; p->xa_drop_ratio = 0.80f; p->mask_level_redun = 0.95f;
	p->mapq_coef_len = 50; p->max_xa_hits = 5; p->max_xa_hits_alt = 200;
	p->flags = 0; p->threads = 16; p->rg_id = nullptr;
}

extern "C" int cs_map_params_split(const cs_map_params_t *p, cs_params_t *seed, cs_chain_params_t *chain, cs_flt_params_t *flt, cs_aln_params_t *aln,
                                   cs_dedup_params_t *dedup, cs_mark_params_t *mark, uint32_t *mark_flags, cs_sam_params_t *sam)
{
	if (!p || !seed || !chain || !flt || !aln || !dedup || !mark || !mark_flags || !sam) return cs_fail_(CS_EINVAL, "cs_map_params_split: null argument");
	cs_params_default(seed);                                          // (want_sal 1 and the engine-side knobs: sst_mode, disable, result_flags)
	seed->min_seed_len = p->min_seed_len; seed->split_factor = p->split_factor; seed->split_width = p->split_width; seed->max_occ = p->max_occ; seed->max_mem_intv = p->max_mem_intv;
	chain->w = p->w; chain->max_chain_gap = p->max_chain_gap; chain->min_seed_len = p->min_seed_len; chain->max_occ = p->max_occ;
	flt->min_chain_weight = p->min_chain_weight; flt->max_chain_extend = p->max_chain_extend; flt->max_chain_gap = p->max_chain_gap; flt->min_seed_len = p->min_seed_len;
	flt->mask_level = p->mask_level; flt->drop_ratio = p->drop_ratio;
	flt->a = p->a; flt->b = p->b; flt->o_del = p->o_del; flt->e_del = p->e_del; flt->o_ins = p->o_ins; flt->e_ins = p->e_ins;
	cs_aln_params_default(aln);                                       // (flags 0)
	aln->a = p->a; aln->b = p->b; aln->o_del = p->o_del; aln->e_del = p->e_del; aln->o_ins = p->o_ins; aln->e_ins = p->e_ins;
	aln->pen_clip5 = p->pen_clip5; aln->pen_clip3 = p->pen_clip3; aln->w = p->w; aln->zdrop = p->zdrop; aln->threads = p->threads;
	dedup->max_chain_gap = p->max_chain_gap; dedup->mask_level_redun = p->mask_level_redun;
	mark->T = p->T; mark->mapq_coef_len = p->mapq_coef_len; mark->max_xa_hits = p->max_xa_hits; mark->max_xa_hits_alt = p->max_xa_hits_alt; mark->min_seed_len = p->min_seed_len;
	mark->mask_level = p->mask_level; mark->drop_ratio = p->drop_ratio; mark->xa_drop_ratio = p->xa_drop_ratio;
	*mark_flags = (p->flags & CS_MAP_ALL ? CS_MARK_ALL : 0u) | (p->flags & CS_MAP_NO_MULTI ? CS_MARK_NO_MULTI : 0u) | (p->flags & CS_MAP_KEEP_SUPP_MAPQ ? CS_MARK_KEEP_SUPP_MAPQ : 0u);
	sam->flags = p->flags & CS_MAP_SOFTCLIP ? CS_SAM_SOFTCLIP : 0u;
	sam->rg_id = p->rg_id;
	return CS_OK;
}

// what the stages' own checks refuse of their parameters (chain_filter_gpu.hip check_call, cs_aligner_create, cs_dedup_regions, cs_regions_mark,
// cs_regions_sam, the seed entry points), asked before anything is loaded; the stages keep their checks
static int check_params(const cs_mapper &m)
{
	const cs_map_params_t &p = m.par;
	for (uint32_t r : p.reserved) if (r) return cs_fail_(CS_EINVAL, "cs_mapper_create: reserved must be 0");
	if (p.flags & ~(CS_MAP_ALL | CS_MAP_NO_MULTI | CS_MAP_KEEP_SUPP_MAPQ | CS_MAP_SOFTCLIP)) return cs_fail_(CS_EINVAL, "cs_mapper_create: unknown flags");
	if (p.pen_clip5 != p.pen_clip3) return cs_fail_(CS_EINVAL, "cs_mapper_create: pen_clip5 != pen_clip3 is not supported (the extension stage's limit: one extender, one end bonus)");
	if (p.mapq_coef_len <= 0) return cs_fail_(CS_EINVAL, "cs_mapper_create: mapq_coef_len <= 0 (that MAPQ formula is not in cs_regions_mark)");
	if (p.mapq_coef_len > 131072) return cs_fail_(CS_EINVAL, "cs_mapper_create: mapq_coef_len above 131,072");
	if (p.a < 1 || p.b < 0 || p.e_del < 1 || p.e_ins < 1 || p.o_del < 0 || p.o_ins < 0 || p.w < 1 || p.zdrop < 0) return cs_fail_(CS_EINVAL, "cs_mapper_create: bad scoring parameters");
	if (p.min_seed_len < 1 || p.max_occ < 1 || p.max_chain_extend < 1 || p.max_chain_gap < 0 || !(p.mask_level_redun > 0.f) || p.max_xa_hits < 0 || p.max_xa_hits_alt < 0 || p.threads < 1)
		return cs_fail_(CS_EINVAL, "cs_mapper_create: bad parameters");
	if (m.rg_id.size() > 255) return cs_fail_(CS_EINVAL, "cs_mapper_create: an RG id of more than 255 characters");
	return CS_OK;
}

static MapRing *make_ring(cs_mapper *m);

extern "C" void cs_mapper_destroy(cs_mapper_t *m)
{
	if (!m) return;
	m->ring.reset();                                                  // waits for the batches in flight, then ends the workers
	if (m->al_tail) cs_aligner_destroy(m->al_tail);
	if (m->al_dd) cs_aligner_destroy(m->al_dd);
	if (m->al) cs_aligner_destroy(m->al);
	if (m->chn) cs_chainer_destroy(m->chn);
	if (m->eng) cs_engine_destroy(m->eng);
	if (m->idx) cs_index_free(m->idx);
	if (m->s) { (void)hipSetDevice(m->device); (void)hipStreamSynchronize(m->s); }
	delete m;                                                         // (the buffers, then the stream)
}

extern "C" int cs_mapper_create(const char *prefix, int device, const cs_engine_options_t *eopt, const cs_map_params_t *par, cs_mapper_t **out)
{
	if (out) *out = nullptr;
	if (!prefix || !out || device < 0) return cs_fail_(CS_EINVAL, "cs_mapper_create: bad argument");
	cs_mapper *m = new cs_mapper();
	auto fail = [&](int rc) { cs_mapper_destroy(m); return rc; };
	if (par) m->par = *par; else cs_map_params_default(&m->par);
	if (m->par.rg_id) m->rg_id = m->par.rg_id;
	m->par.rg_id = m->rg_id.empty() ? nullptr : m->rg_id.c_str();    // the mapper's own copy
	m->device = device;
	if (int rc = check_params(*m)) return fail(rc);
	if (int rc = cs_map_params_split(&m->par, &m->seed, &m->chain, &m->flt, &m->aln, &m->dedup, &m->mark, &m->mark_flags, &m->sam)) return fail(rc);
	if (int rc = cs_index_load(prefix, &m->idx)) return fail(rc);
	// the other index files, before the device is asked for: a missing file is CS_EIO with or without a GPU
	if (int rc = cs_aligner_create(prefix, -1, &m->aln, &m->al_dd)) return fail(rc);
	int ndev = 0;
	const int drc = cs_device_count(&ndev);
	if (drc || ndev < 1) { const std::string why = drc ? std::string(": ") + cs_last_error() : std::string(); return fail(cs_fail_(CS_EDEVICE, "cs_mapper_create: no GPU" + why)); }
	if (device >= ndev) return fail(cs_fail_(CS_EINVAL, "cs_mapper_create: no such device"));
	cs_index_view_t view;
	if (int rc = cs_index_view(m->idx, &view)) return fail(rc);
	if (int rc = eopt ? cs_engine_create_opts(&view, device, eopt, &m->eng) : cs_engine_create(&view, device, &m->eng)) return fail(rc);
	if (int rc = cs_chainer_create_device(prefix, device, &m->chn)) return fail(rc);
	if (int rc = cs_aligner_create(prefix, device, &m->aln, &m->al)) return fail(rc);
	if (int rc = cs_aligner_create(prefix, device, &m->aln, &m->al_tail)) return fail(rc);
	if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&m->s.h, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return fail(cs_fail_(CS_EDEVICE, "cs_mapper_create: no stream")); }
	m->ring.reset(make_ring(m));                                      // (no thread before the first cs_map_submit)
	*out = m;
	return CS_OK;
}

namespace {
// a stage's error as a part hands it on: "<stage>: <the stage's message>", read in the thread that ran the stage; the entry point that
// reports it (cs_map_batch, cs_map_collect) puts its own name in front
int stage_fail(std::string &err, const char *stage, int rc) { err = std::string(stage) + ": " + cs_last_error(); return rc; }

// the reads into the mapper's device buffers, complete when this returns (the stages work on streams of their own)
int upload_reads(cs_mapper &m, int64_t n, const uint8_t *bases, const uint64_t *off)
{
	HIP_TRY(hipSetDevice(m.device));
	const size_t nb = (size_t)off[n];
	if (int rc = m.d_bases.ensure(nb, 64)) return rc;
	if (int rc = m.d_off.ensure((size_t)n + 1)) return rc;
	if (nb) HIP_TRY(hipMemcpyAsync(m.d_bases.p, bases, nb, hipMemcpyHostToDevice, m.s));
	HIP_TRY(hipMemcpyAsync(m.d_off.p, off, ((size_t)n + 1) * sizeof *off, hipMemcpyHostToDevice, m.s));
	HIP_TRY(hipStreamSynchronize(m.s));
	return CS_OK;
}
// reg_off and the live regions of the extension's device result into the batch's host vectors
int download_regions(cs_mapper &m, MapJob &b, const cs_aln_result_t &d)
{
	HIP_TRY(hipSetDevice(m.device));
	b.reg_off.resize((size_t)d.n_reads + 1); b.regs.resize((size_t)d.n_regs);
	HIP_TRY(hipMemcpyAsync(b.reg_off.data(), d.reg_off, ((size_t)d.n_reads + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, m.s));
	if (d.n_regs) HIP_TRY(hipMemcpyAsync(b.regs.data(), d.regs, (size_t)d.n_regs * sizeof(cs_alnreg_t), hipMemcpyDeviceToHost, m.s));
	HIP_TRY(hipStreamSynchronize(m.s));
	if (b.reg_off[0] != 0 || b.reg_off[(size_t)d.n_reads] != d.n_regs) return cs_fail_(CS_EDEVICE, "the extension's reg_off does not end at its region count");
	b.live.n_reads = d.n_reads; b.live.n_regs = d.n_regs; b.live.reg_off = b.reg_off.data(); b.live.regs = b.regs.data();
	return CS_OK;
}

// ---- the three parts of a batch of n > 0 reads, in the order cs_map_batch runs them.  A streamed batch runs each on the worker of that
// part (map_stream.hpp); every step adds its wall time to the batch's clock in the thread that runs it.
// front: the engine, the chainer, the extension's aligner, the mapper's stream and its device copy of the reads -> b.live
int part_front(cs_mapper &m, MapJob &b, std::string &err)
{
	StepClock &T = b.T;
	T.start();
	if (int rc = upload_reads(m, b.n, b.bases, b.off)) return stage_fail(err, "upload", rc);
	T.lap(CS_MAP_T_UPLOAD);
	cs_result_t seeds;
	if (int rc = cs_engine_seed_batch_device(m.eng, &m.seed, b.n, m.d_bases.p, m.d_off.p, b.off[b.n], &seeds)) return stage_fail(err, "seeding", rc);
	T.lap(CS_MAP_T_SEED);
	cs_chain_result_t chains, kept; const int32_t *d_score = nullptr;
	if (int rc = cs_chain_batch_device(m.chn, &m.chain, &seeds, m.d_off.p, 0, &chains)) return stage_fail(err, "chaining", rc);
	T.lap(CS_MAP_T_CHAIN);
	if (int rc = cs_chain_filter_device(m.chn, &m.flt, &chains, m.d_bases.p, m.d_off.p, 0, &kept, &d_score)) return stage_fail(err, "chain filter", rc);
	T.lap(CS_MAP_T_FILTER);
	cs_aln_result_t d_regs;
	if (int rc = cs_extend_chains_device(m.al, &kept, d_score, m.d_bases.p, m.d_off.p, CS_ALN_DEV_COMPACT, &d_regs)) return stage_fail(err, "extension", rc);
	T.lap(CS_MAP_T_EXTEND);
	if (int rc = download_regions(m, b, d_regs)) return stage_fail(err, "download", rc);
	T.lap(CS_MAP_T_DOWNLOAD);
	return CS_OK;
}
// de-duplication: the host-only aligner; b.live -> b.dd, in that aligner's arrays
int part_dedup(cs_mapper &m, MapJob &b, std::string &err)
{
	b.T.start();
	if (int rc = cs_dedup_regions(m.al_dd, &m.dedup, &b.live, b.bases, b.off, &b.dd, nullptr)) return stage_fail(err, "de-duplication", rc);
	b.T.lap(CS_MAP_T_DEDUP);
	return CS_OK;
}
// tail: the tail's aligner; b.dd -> the text in the SAM stage's arrays (*out) and what the batch adds to the counters
int part_tail(cs_mapper &m, MapJob &b, std::string &err, cs_sam_result_t *out, cs_map_stats_t &add)
{
	StepClock &T = b.T;
	T.start();
	cs_mark_result_t marks;
	if (int rc = cs_regions_mark(m.al_tail, &m.mark, &b.dd, b.off, b.id_base, m.mark_flags, &marks)) return stage_fail(err, "marking", rc);
	T.lap(CS_MAP_T_MARK);
	cs_cigar_result_t alns;
	if (int rc = cs_regions_cigar(m.al_tail, &marks.cigar_regs, b.bases, b.off, 0, &alns)) return stage_fail(err, "CIGAR", rc);
	T.lap(CS_MAP_T_CIGAR);
	cs_sam_stats_t s0, s1;
	(void)cs_sam_stats(m.al_tail, &s0);
	if (int rc = cs_regions_sam(m.al_tail, &m.sam, &marks, b.dd.reg_off, &alns, b.bases, b.off, b.quals, b.names, b.name_off, b.comments, b.comment_off, out)) return stage_fail(err, "SAM text", rc);
	(void)cs_sam_stats(m.al_tail, &s1);
	T.lap(CS_MAP_T_SAM);
	T.end();
	add = cs_map_stats_t{};
	add.reads = (uint64_t)b.n; add.bases = b.off[b.n]; add.regions = b.dd.n_regs; add.lines = s1.lines - s0.lines; add.unmapped = s1.unmapped - s0.unmapped;
	add.bytes = s1.bytes - s0.bytes; add.batches = 1;
	for (int k = 0; k < CS_MAP_N_STAGES; ++k) add.stage_ms[k] = T.ms[k];
	return CS_OK;
}
void add_stats(cs_map_stats_t &st, const cs_map_stats_t &add)
{
	st.reads += add.reads; st.bases += add.bases; st.regions += add.regions; st.lines += add.lines; st.unmapped += add.unmapped; st.bytes += add.bytes; st.batches += add.batches;
	for (int k = 0; k < CS_MAP_N_STAGES; ++k) st.stage_ms[k] += add.stage_ms[k];
}

// what cs_map_batch and cs_map_submit refuse of a batch before anything runs
int check_batch(const char *who, const cs_mapper_t *m, int64_t n, const uint8_t *bases, const uint64_t *read_offsets, const char *names, const uint64_t *name_off, const char *comments,
                const uint64_t *comment_off, int64_t id_base)
{
	const std::string w(who);
	if (!m || n < 0 || id_base < 0) return cs_fail_(CS_EINVAL, w + ": bad argument");
	if (n == 0) return CS_OK;
	if (!read_offsets || !name_off || !comments != !comment_off) return cs_fail_(CS_EINVAL, w + ": null argument, or one of comments / comment_off without the other");
	if (read_offsets[0] != 0) return cs_fail_(CS_EINVAL, w + ": read_offsets does not start at 0");
	for (int64_t r = 0; r < n; ++r) if (read_offsets[r + 1] < read_offsets[r]) return cs_fail_(CS_EINVAL, w + ": read_offsets decreases");
	if ((read_offsets[n] && !bases) || (name_off[n] && !names)) return cs_fail_(CS_EINVAL, w + ": null argument");
	return CS_OK;
}
void fill_job(MapJob &b, int64_t n, const uint8_t *bases, const uint64_t *read_offsets, const uint8_t *quals, const char *names, const uint64_t *name_off, const char *comments,
              const uint64_t *comment_off, int64_t id_base)
{
	b.n = n; b.id_base = id_base; b.bases = bases; b.off = read_offsets; b.quals = quals; b.names = names; b.name_off = name_off; b.comments = comments; b.comment_off = comment_off;
	b.live = cs_aln_result_t{}; b.dd = cs_aln_result_t{};
	b.T = StepClock();
}
} // namespace

// The workers' parts.  A batch without reads passes through untouched and its tail leaves the empty result.  Behind de-duplication the
// regions are exchanged out of the host-only aligner into the slot, and behind the SAM stage the text out of the stage into the slot's
// result (host pointers change hands, nothing is copied): the next batch's de-duplication and tail overwrite the aligners' arrays while
// this batch's tail reads the regions and while its text waits for cs_map_collect.
static MapRing *make_ring(cs_mapper *m)
{
	return new MapRing(
		[m](MapJob &b, MapResult &, std::string &err) { return b.n ? part_front(*m, b, err) : CS_OK; },
		[m](MapJob &b, MapResult &, std::string &err) {
			if (!b.n) return (int)CS_OK;
			if (int rc = part_dedup(*m, b, err)) return rc;
			cs_aligner_dedup_exchange_(m->al_dd, b.dd_off, b.dd_regs);
			b.dd.reg_off = b.dd_off.data(); b.dd.regs = b.dd_regs.data();
			return (int)CS_OK;
		},
		[m](MapJob &b, MapResult &r, std::string &err) {
			if (!b.n) {
				r.text_off.assign(1, 0); r.text.clear(); r.add = cs_map_stats_t{};
				r.res.n_reads = 0; r.res.n_lines = 0; r.res.n_bytes = 0; r.res.text_off = r.text_off.data(); r.res.text = nullptr;
				return (int)CS_OK;
			}
			if (int rc = part_tail(*m, b, err, &r.res, r.add)) return rc;
			cs_aligner_sam_exchange_(m->al_tail, r.text_off, r.text);
			r.res.text_off = r.text_off.data(); r.res.text = r.text.data();
			return (int)CS_OK;
		},
		[m]() { (void)hipSetDevice(m->device); });
}

extern "C" int cs_map_batch(cs_mapper_t *m, int64_t n_reads, const uint8_t *bases, const uint64_t *read_offsets, const uint8_t *quals, const char *names,
                            const uint64_t *name_off, const char *comments, const uint64_t *comment_off, int64_t id_base, cs_sam_result_t *out)
{
	if (!m || !out) return cs_fail_(CS_EINVAL, "cs_map_batch: bad argument");
	if (int rc = check_batch("cs_map_batch", m, n_reads, bases, read_offsets, names, name_off, comments, comment_off, id_base)) return rc;
	if (!m->ring->idle()) return cs_fail_(CS_EINVAL, "cs_map_batch: batches are in flight (cs_map_submit): collect them first");
	if (n_reads == 0) {
		m->no_text_off.assign(1, 0);
		out->n_reads = 0; out->n_lines = 0; out->n_bytes = 0; out->text_off = m->no_text_off.data(); out->text = nullptr;
		return CS_OK;
	}
	MapJob &b = m->blk;
	fill_job(b, n_reads, bases, read_offsets, quals, names, name_off, comments, comment_off, id_base);
	std::string err; cs_map_stats_t add;
	int rc = part_front(*m, b, err);
	if (rc == CS_OK) rc = part_dedup(*m, b, err);
	if (rc == CS_OK) rc = part_tail(*m, b, err, out, add);
	if (rc != CS_OK) return cs_fail_(rc, "cs_map_batch: " + err);
	add_stats(m->st, add);
	return CS_OK;
}

extern "C" int cs_map_submit(cs_mapper_t *m, int64_t n_reads, const uint8_t *bases, const uint64_t *read_offsets, const uint8_t *quals, const char *names,
                             const uint64_t *name_off, const char *comments, const uint64_t *comment_off, int64_t id_base)
{
	if (int rc = check_batch("cs_map_submit", m, n_reads, bases, read_offsets, names, name_off, comments, comment_off, id_base)) return rc;
	if (!m->ring->submit([&](MapJob &b) { fill_job(b, n_reads, bases, read_offsets, quals, names, name_off, comments, comment_off, id_base); }))
		return cs_fail_(CS_EINVAL, "cs_map_submit: CS_MAP_MAX_IN_FLIGHT batches are in flight already: collect one first");
	return CS_OK;
}

extern "C" int cs_map_collect(cs_mapper_t *m, cs_sam_result_t *out)
{
	if (!m || !out) return cs_fail_(CS_EINVAL, "cs_map_collect: null argument");
	MapResult *r = nullptr; std::string err;
	const int rc = m->ring->collect(&r, err);
	if (rc == map_stream::NOTHING_IN_FLIGHT) return cs_fail_(CS_EINVAL, "cs_map_collect: nothing in flight");
	if (rc != CS_OK) return cs_fail_(rc, "cs_map_collect: " + err);
	add_stats(m->st, r->add);
	*out = r->res;
	return CS_OK;
}

extern "C" int cs_mapper_in_flight(const cs_mapper_t *m, int *submitted, int *finished)
{
	if (!m || !submitted || !finished) return cs_fail_(CS_EINVAL, "cs_mapper_in_flight: null argument");
	m->ring->in_flight(submitted, finished);
	return CS_OK;
}

extern "C" int cs_mapper_header(const cs_mapper_t *m, const char *rg_line, char *buf, size_t cap, size_t *need)
{
	if (!m) return cs_fail_(CS_EINVAL, "cs_mapper_header: null argument");
	return cs_sam_header(m->al, rg_line, buf, cap, need);
}
extern "C" int cs_mapper_stats(const cs_mapper_t *m, cs_map_stats_t *st)
{
	if (!m || !st) return cs_fail_(CS_EINVAL, "cs_mapper_stats: null argument");
	*st = m->st;
	return CS_OK;
}
extern "C" int cs_mapper_engine_stats(const cs_mapper_t *m, cs_stats_t *st)
{
	if (!m || !st) return cs_fail_(CS_EINVAL, "cs_mapper_engine_stats: null argument");
	return cs_engine_stats(m->eng, st);
}
