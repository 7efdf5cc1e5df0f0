// engine.hip -- C-ABI implementation (include/compseed_amd.h): the engine's lifecycle and the device residency of the index.
//
// Host-side counterpart of mem_process_seqs -> seed_and_extend (mapping/comp_seed.cpp:2527, 2242) for the seeding
// and SAL blocks only.  No CPU fallback exists: without a HIP device every entry point fails with CS_EDEVICE.
#include "engine.hpp"

#include <cstdio>
#include <string>
#include <vector>

thread_local std::string g_err;
int cs_fail_(int code, const std::string &msg) { return fail(code, msg); }

extern "C" const char *cs_last_error(void) { return g_err.c_str(); }
extern "C" const char *cs_version(void) { return "compseed_amd 0.1 (gfx950)"; }

extern "C" void cs_params_default(cs_params_t *p)
{
	if (!p) return;
	p->min_seed_len = 19; p->split_factor = 1.5f; p->split_width = 10; p->max_occ = 500; p->max_mem_intv = 20;
	p->want_sal = 1; p->sst_mode = 1; p->disable = 0; p->count_traffic = 0;
	p->result_flags = 0; p->reserved = 0;
}
extern "C" void cs_engine_options_default(cs_engine_options_t *o)
{
	if (!o) return;
	memset(o, 0, sizeof *o);
	o->full_sa = 1; o->sa64 = 0; o->sa40 = 0; o->text_mode = 1; o->text_arrays = 1; o->jump_k = 15; o->kmer_filter = 1; o->fused = 0;
	o->mem_cap = 64; o->lep_arena_mb = 16384; o->max_raw_mb = 24576; o->r3_text_iter = 5; o->count_sal_merged = 0; o->verbose = 0;
	o->pipeline_reads = 5000000; o->expand_threads = 16; o->host_pack_threads = 8; o->passes_in_flight = 2;
}

// ------------------------------------------------------------------------------------------------ index files
static bool read_file(const std::string &fn, std::vector<uint8_t> &buf)
{
	FILE *fp = fopen(fn.c_str(), "rb");
	if (!fp) return false;
	fseek(fp, 0, SEEK_END);
	long sz = ftell(fp);
	fseek(fp, 0, SEEK_SET);
	buf.resize((size_t)sz);
	size_t got = sz ? fread(buf.data(), 1, (size_t)sz, fp) : 0;
	fclose(fp);
	return got == (size_t)sz;
}

extern "C" int cs_index_load(const char *prefix, cs_index_t **out)
{
	if (!prefix || !out) return fail(CS_EINVAL, "cs_index_load: null argument");
	*out = nullptr;
	std::string pre(prefix);
	{ // bwa_idx_infer_prefix (bwalib/bwa.c:244-268): accept "<hint>.64" if it exists
		FILE *fp = fopen((pre + ".64.bwt").c_str(), "rb");
		if (fp) { fclose(fp); pre += ".64"; }
	}
	std::vector<uint8_t> raw;
	if (!read_file(pre + ".bwt", raw) || raw.size() < 40 + 64) return fail(CS_EIO, "cannot read " + pre + ".bwt");
	cs_index *ix = new cs_index();
	cs_index_view_t &v = ix->v;
	memset(&v, 0, sizeof v);
	memcpy(&v.primary, raw.data(), 8);           // bwt_restore_bwt, bwt.c:443-462
	memcpy(&v.L2[1], raw.data() + 8, 32);
	v.L2[0] = 0; v.seq_len = v.L2[4];
	v.bwt_size = (raw.size() - 40) >> 2;
	ix->bwt.resize(v.bwt_size);
	memcpy(ix->bwt.data(), raw.data() + 40, v.bwt_size * 4);
	if (!read_file(pre + ".sa", raw) || raw.size() < 56) { delete ix; return fail(CS_EIO, "cannot read " + pre + ".sa"); }
	uint64_t h[7];
	memcpy(h, raw.data(), 56);                   // bwt_restore_sa, bwt.c:421-441
	if (h[0] != v.primary) { delete ix; return fail(CS_EIO, "SA-BWT inconsistency: primary is not the same"); }
	if (h[6] != v.seq_len) { delete ix; return fail(CS_EIO, "SA-BWT inconsistency: seq_len is not the same"); }
	v.sa_intv = h[5];
	if (v.sa_intv == 0 || (v.sa_intv & (v.sa_intv - 1))) { delete ix; return fail(CS_EIO, "SA sample interval is not a power of 2"); }
	v.n_sa = (v.seq_len + v.sa_intv) / v.sa_intv;
	if ((raw.size() - 56) / 8 < v.n_sa - 1) { delete ix; return fail(CS_EIO, pre + ".sa is truncated"); }
	ix->sa.resize(v.n_sa);
	ix->sa[0] = ~0ull;
	memcpy(ix->sa.data() + 1, raw.data() + 56, (v.n_sa - 1) * 8);
	v.bwt = ix->bwt.data(); v.sa = ix->sa.data();
	*out = ix;
	return CS_OK;
}
extern "C" int cs_index_view(const cs_index_t *idx, cs_index_view_t *view)
{
	if (!idx || !view) return fail(CS_EINVAL, "cs_index_view: null argument");
	*view = idx->v;
	return CS_OK;
}
extern "C" void cs_index_free(cs_index_t *idx) { delete idx; }

// ------------------------------------------------------------------------------------------------ engine
extern "C" int cs_device_count(int *n)
{
	if (!n) return fail(CS_EINVAL, "null argument");
	*n = 0;
	HIP_TRY(hipGetDeviceCount(n));
	return CS_OK;
}

// ------------------------------------------------------------------------------------------------ index residency (engine_init)
namespace csd {

// file layout -> device layout, in place, one thread per 128-row block of the file (run once per engine)
__global__ void relayout_kernel(uint4 *bwt, uint64_t n_blocks, unsigned long long *overflow)
{
	uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= n_blocks) return;
	uint4 q0 = bwt[b * 4], q1 = bwt[b * 4 + 1], q2 = bwt[b * 4 + 2], q3 = bwt[b * 4 + 3];
	const uint32_t w[8] = {q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
	uint64_t h[4] = {u64_of(q0.x, q0.y), u64_of(q0.z, q0.w), u64_of(q1.x, q1.y), u64_of(q1.z, q1.w)};
	uint32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0}, first64[4] = {0, 0, 0, 0};
	for (int i = 0; i < 128; ++i) {
		uint32_t code = (w[i >> 4] >> ((15 - (i & 15)) << 1)) & 3u; // bwt_B0, bwt.h:80
		lo[i >> 5] |= (code & 1u) << (i & 31);
		hi[i >> 5] |= (code >> 1) << (i & 31);
		if (i < 64) ++first64[code];
	}
	for (int c = 0; c < 4; ++c) if ((h[c] + first64[c]) >> 32) atomicAdd(overflow, 1ull);
	bwt[b * 4]     = make_uint4((uint32_t)h[0], (uint32_t)h[1], (uint32_t)h[2], (uint32_t)h[3]);
	bwt[b * 4 + 1] = make_uint4(lo[0], lo[1], hi[0], hi[1]);
	bwt[b * 4 + 2] = make_uint4((uint32_t)(h[0] + first64[0]), (uint32_t)(h[1] + first64[1]), (uint32_t)(h[2] + first64[2]), (uint32_t)(h[3] + first64[3]));
	bwt[b * 4 + 3] = make_uint4(lo[2], lo[3], hi[2], hi[3]);
}

// one-time preparation of the text-mode arrays from the full suffix array: T[SA[r] - 1] is the BWT character of row r
// (the suffix array and its inverse come as Plain<u32>, Plain<u64> or Pack40, fm_device.hpp: get / put by entry)
template <typename A>
__global__ void text_isa_fill_kernel(const DevIndex ix, const A fsa, uint8_t *tbytes, const A isa)
{
	for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= ix.seq_len; r += (uint64_t)gridDim.x * blockDim.x) {
		uint64_t s = fsa.get(r);
		isa.put(s, r);
		if (r == ix.primary) continue; // the row of the whole text: its BWT character is the sentinel
		uint64_t row = r - (r > ix.primary);
		Block b = load_block(ix, row >> OCC_SHIFT);
		uint32_t p = (uint32_t)row & OCC_MASK, w = p >> 5, bit = p & 31;
		uint32_t lo = w == 0 ? b.pl.x : b.pl.y, hi = w == 0 ? b.pl.z : b.pl.w;
		tbytes[s - 1] = (uint8_t)(((lo >> bit) & 1u) | (((hi >> bit) & 1u) << 1));
	}
}
__global__ void text_pack_kernel(const uint8_t *tbytes, uint64_t n, uint32_t *text2)
{
	uint64_t nw = (n + 15) >> 4;
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += (uint64_t)gridDim.x * blockDim.x) {
		uint32_t v = 0;
		for (int j = 0; j < 16; ++j) { uint64_t p = w * 16 + j; if (p < n) v |= (uint32_t)(tbytes[p] & 3) << (2 * j); }
		text2[w] = v;
	}
}

template <typename A>
__global__ void lcp_fill_kernel(const DevIndex ix, const A fsa, uint8_t *lcp)
{
	for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= ix.seq_len + 1; r += (uint64_t)gridDim.x * blockDim.x)
		lcp[r] = (r == 0 || r > ix.seq_len) ? 0 : (uint8_t)text_lcp(ix, fsa.get(r - 1), fsa.get(r), 255u);
}
template <typename A>
__global__ void rep_fill_kernel(const DevIndex ix, const A fsa, const uint8_t *lcp, uint8_t *rep, uint64_t *isa_fuse)
{
	for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= ix.seq_len; r += (uint64_t)gridDim.x * blockDim.x) {
		const uint8_t a = lcp[r], b = lcp[r + 1], v = a > b ? a : b;
		const uint64_t p = fsa.get(r);
		rep[p] = v; // row 0 (the empty suffix) writes rep[seq_len] = 0
		// 8-byte inverse-SA entries carry the same byte above the rank (DevIndex::isa_fused): the top byte of entry p, which this thread
		// alone writes and nothing reads here
		if (isa_fuse) reinterpret_cast<uint8_t *>(isa_fuse + p)[7] = v;
	}
}

// Materialise SA[row] for every row from the 1-in-sa_intv samples: lane t starts at sampled row t*sa_intv, whose value is
// known, and follows bwt_invPsi (one text position back per step, bwt.c:53-59) writing SA = value - steps until it
// reaches the next sampled row.  Every row lies on exactly one such chain, so all seq_len+1 rows get written once.
template <typename A>
__global__ void sa_fill_kernel(const DevIndex ix, const A full)
{
	uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= ix.n_sa) return;
	uint64_t k = t << ix.sa_shift;
	uint64_t s = (t == 0) ? ix.seq_len : ix.sa[t]; // row 0 is the "$" suffix at text position seq_len
	full.put(k, s);
	for (;;) {
		k = inv_psi(ix, k);
		if ((k & ix.sa_mask) == 0) break;
		--s;
		full.put(k, s);
	}
}

// Round-3 jump table.  bwt_seed_strategy1 (bwt.c:358-379) extends forward from a start x and looks at the interval only
// once i - x >= min_seed_len, so the first min_seed_len bases of every segment are pure pointer chasing whose
// intermediate intervals nobody reads -- and at those depths the interval is still wide, so every step costs TWO random
// records.  The bi-interval of every k-mer (k = jump_k <= min_seed_len) is therefore precomputed once per engine into a
// table in HBM (4^15 x 16 B = 17 GB by default: this is what 288 GB are for) and a segment starts with ONE lookup instead of k - 1
// extensions.  A k-mer that does not occur has size 0 and every later extension keeps it at 0, exactly as in the
// reference, so the emitted seeds are unchanged; the skipped steps are counted as queries answered by the cache.
__global__ void jump_fill_kernel(const DevIndex ix, int k, uint4 *table)
{
	uint64_t n = 1ull << (2 * k);
	for (uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; m < n; m += (uint64_t)gridDim.x * blockDim.x) {
		Intv v = set_intv(ix, (int)((m >> (2 * (k - 1))) & 3));
		NoCtr W;
		for (int j = k - 2; j >= 0; --j) v = extend1<false>(ix, v, 3 - (int)((m >> (2 * j)) & 3), W);
		table[m] = pack_lep(v, 0);
	}
}

} // namespace csd

static int engine_init(cs_engine *e, const cs_index_view_t *v)
{
	int ndev = 0;
	HIP_TRY(hipGetDeviceCount(&ndev));
	if (ndev <= 0) return fail(CS_EDEVICE, "no HIP device: the seeding engine has no CPU path");
	if (e->device < 0 || e->device >= ndev) return fail(CS_EINVAL, "device ordinal out of range");
	HIP_TRY(hipSetDevice(e->device));
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, e->device));
	e->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	const cs_engine_options_t &opt = e->opt;
	const bool verbose = opt.verbose != 0;
	if (opt.mem_cap < 1 || opt.mem_cap > 4096 || opt.lep_arena_mb < 1 || opt.max_raw_mb < 1 || (opt.jump_k != 0 && (opt.jump_k < 6 || opt.jump_k > 15)))
		return fail(CS_EINVAL, "cs_engine_options_t: mem_cap 1..4096, lep_arena_mb >= 1, max_raw_mb >= 1, jump_k 0 or 6..15");
	for (int r : opt.reserved) if (r) return fail(CS_EINVAL, "cs_engine_options_t.reserved must be 0");
	if (opt.passes_in_flight < 1 || opt.passes_in_flight > 2 || opt.host_pack_threads < 0) return fail(CS_EINVAL, "cs_engine_options_t: passes_in_flight 1 or 2, host_pack_threads >= 0");
	if (verbose) { fprintf(stderr, "[cs_engine] creating engine on device %d, seq_len %llu\n", e->device, (unsigned long long)v->seq_len); fflush(stderr); }
	CS_TRY(add_pass_ctx(e));
	PassCtx &c = *e->ctx[0];
	CS_TRY(host_pipe_create(e)); // here, before the index upload: its copy streams are the next streams made after the context's

	if (v->seq_len == 0 || v->seq_len != v->L2[4] || v->L2[0] != 0) return fail(CS_EINVAL, "index view: L2 / seq_len inconsistent");
	if (v->seq_len >> 37) return fail(CS_ERANGE, "index longer than 2^37 symbols does not fit the packed LEP entries");
	if (opt.sa40 && (v->seq_len + 1) >> 40) return fail(CS_ERANGE, "sa40: 2^40 rows or more do not fit 40-bit suffix-array entries");
	if (v->primary > v->seq_len) return fail(CS_EINVAL, "index view: primary out of range");
	uint64_t n_blocks = (v->seq_len + 127) >> 7;
	// the file holds one extra count record after the last block (bwt_bwtupdate_core, index_main.c:152-174)
	if (v->bwt_size < n_blocks * 16) return fail(CS_EINVAL, "index view: bwt array shorter than seq_len requires");
	if (v->sa_intv == 0 || (v->sa_intv & (v->sa_intv - 1))) return fail(CS_EINVAL, "index view: sa_intv is not a power of two");
	if (v->n_sa != (v->seq_len + v->sa_intv) / v->sa_intv) return fail(CS_EINVAL, "index view: n_sa inconsistent");

	size_t quads = (size_t)((v->bwt_size + 3) >> 2) + 8; // pad: a block load never leaves the allocation
	CS_TRY(e->d_bwt.reserve(quads));
	HIP_TRY(hipMemsetAsync(e->d_bwt.p, 0, quads * sizeof(uint4), c.stream));
	HIP_TRY(hipMemcpyAsync(e->d_bwt.p, v->bwt, (size_t)v->bwt_size * 4, hipMemcpyHostToDevice, c.stream));
	CS_TRY(e->d_sa.reserve((size_t)v->n_sa));
	HIP_TRY(hipMemcpyAsync(e->d_sa.p, v->sa, (size_t)v->n_sa * 8, hipMemcpyHostToDevice, c.stream));
	// one-time conversion of the 2-bit packed bases of every block into bit planes (fm_device.hpp)
	// (the context's counter words are zero)
	hipLaunchKernelGGL(relayout_kernel, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, c.stream, e->d_bwt.p, n_blocks, c.d_sctr.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(c.h_sctr.p, c.d_sctr.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	if (c.h_sctr.p[0]) return fail(CS_ERANGE, "a single base occurs 2^32 times or more: 32-bit Occ counts of the device layout overflow");
	e->smem_mode = opt.fused ? 0 : 1;
	e->lep_arena_bytes = (size_t)opt.lep_arena_mb << 20;
	e->cap = (uint32_t)opt.mem_cap;
	e->max_raw_bytes = (size_t)opt.max_raw_mb << 20;

	DevIndex &ix = e->ix;
	ix.bwt = e->d_bwt.p; ix.sa = e->d_sa.p;
	ix.primary = v->primary; ix.seq_len = v->seq_len; ix.n_sa = v->n_sa; ix.n_blocks = n_blocks;
	for (int i = 0; i < 5; ++i) ix.L2[i] = v->L2[i];
	ix.sa_mask = (uint32_t)(v->sa_intv - 1);
	ix.sa_shift = (uint32_t)__builtin_ctzll(v->sa_intv);

	if (verbose) { fprintf(stderr, "[cs_engine] index uploaded and re-laid out\n"); fflush(stderr); }
	// full suffix array in HBM (4 B/row below 2^32 rows, else 8 B/row: 50 GB for hg19 of the 288 GB on board; 40-bit entries, 5.33 B/row,
	// with engine option sa40: 33 GB)
	ix.fsa32 = nullptr; ix.fsa64 = nullptr; ix.fsa40 = nullptr;
	const uint64_t rows = v->seq_len + 1;
	const bool pack40 = opt.sa40 != 0;
	const bool small = !pack40 && rows < 0xffffffffull && !opt.sa64; // sa64: 8-byte entries on a small index (tests of the hg19-scale instantiation)
	const size_t sa_bytes = pack40 ? pack40_groups(rows) * sizeof(uint4) : (size_t)rows * (small ? 4 : 8); // of the full SA, and of its inverse
	if (opt.full_sa) {
		size_t free_b = 0, total_b = 0;
		HIP_TRY(hipMemGetInfo(&free_b, &total_b));
		if (sa_bytes + ((size_t)8 << 30) < free_b) {
			unsigned grid = (unsigned)((v->n_sa + 255) / 256);
			if (pack40) {
				CS_TRY(e->d_fsa40.reserve(pack40_groups(rows) + 4));
				hipLaunchKernelGGL(sa_fill_kernel<Pack40>, dim3(grid), dim3(256), 0, c.stream, ix, Pack40{e->d_fsa40.p});
				HIP_TRY(hipGetLastError()); HIP_TRY(hipStreamSynchronize(c.stream));
				ix.fsa40 = e->d_fsa40.p;
			} else if (small) {
				CS_TRY(e->d_fsa32.reserve((size_t)rows + 16));
				hipLaunchKernelGGL(sa_fill_kernel<Plain<uint32_t>>, dim3(grid), dim3(256), 0, c.stream, ix, Plain<uint32_t>{e->d_fsa32.p});
				HIP_TRY(hipGetLastError()); HIP_TRY(hipStreamSynchronize(c.stream));
				ix.fsa32 = e->d_fsa32.p;
			} else {
				CS_TRY(e->d_fsa64.reserve((size_t)rows + 16));
				hipLaunchKernelGGL(sa_fill_kernel<Plain<uint64_t>>, dim3(grid), dim3(256), 0, c.stream, ix, Plain<uint64_t>{e->d_fsa64.p});
				HIP_TRY(hipGetLastError()); HIP_TRY(hipStreamSynchronize(c.stream));
				ix.fsa64 = e->d_fsa64.p;
			}
		}
	}

	// text mode (smem_common.hpp, text_step): the 2-bit text and the inverse suffix array, derived from the full suffix array
	ix.text2 = nullptr; ix.isa32 = nullptr; ix.isa64 = nullptr; ix.isa40 = nullptr;
	{
		size_t free_b = 0, total_b = 0;
		HIP_TRY(hipMemGetInfo(&free_b, &total_b));
		size_t need = sa_bytes + (size_t)v->seq_len + (size_t)v->seq_len / 4 + ((size_t)24 << 30);
		if (opt.text_mode && has_full_sa(ix) && need < free_b) {
			DevBuf<uint8_t> tbytes;
			CS_TRY(tbytes.reserve((size_t)v->seq_len + 64));
			CS_TRY(e->d_text2.reserve((size_t)((v->seq_len + 15) >> 4) + 16));
			unsigned grid = (unsigned)std::min<uint64_t>((rows + 255) / 256, 1u << 22);
			if (ix.fsa40) {
				CS_TRY(e->d_isa40.reserve(pack40_groups(rows) + 4));
				hipLaunchKernelGGL(text_isa_fill_kernel<Pack40>, dim3(grid), dim3(256), 0, c.stream, ix, Pack40{e->d_fsa40.p}, tbytes.p, Pack40{e->d_isa40.p});
			} else if (ix.fsa32) {
				CS_TRY(e->d_isa32.reserve((size_t)rows + 16));
				hipLaunchKernelGGL(text_isa_fill_kernel<Plain<uint32_t>>, dim3(grid), dim3(256), 0, c.stream, ix, Plain<uint32_t>{e->d_fsa32.p}, tbytes.p, Plain<uint32_t>{e->d_isa32.p});
			} else {
				CS_TRY(e->d_isa64.reserve((size_t)rows + 16));
				hipLaunchKernelGGL(text_isa_fill_kernel<Plain<uint64_t>>, dim3(grid), dim3(256), 0, c.stream, ix, Plain<uint64_t>{e->d_fsa64.p}, tbytes.p, Plain<uint64_t>{e->d_isa64.p});
			}
			hipLaunchKernelGGL(text_pack_kernel, dim3(grid), dim3(256), 0, c.stream, tbytes.p, v->seq_len, e->d_text2.p);
			HIP_TRY(hipGetLastError()); HIP_TRY(hipStreamSynchronize(c.stream));
			ix.text2 = e->d_text2.p; ix.isa32 = e->d_isa32.p; ix.isa64 = e->d_isa64.p; ix.isa40 = e->d_isa40.p;
		}
		if (verbose) { fprintf(stderr, "[cs_engine] text mode: %s\n", ix.text2 ? "on" : "off"); fflush(stderr); }
	}
	// re-seeding from the text (smem_text.hpp, r2text_kernel): capped LCP array and repeat-length array, 1 byte per row each
	ix.lcp = nullptr; ix.rep = nullptr; ix.isa_fused = 0;
	{
		size_t free_b = 0, total_b = 0;
		HIP_TRY(hipMemGetInfo(&free_b, &total_b));
		size_t need = (size_t)v->seq_len * 2 + ((size_t)24 << 30);
		if (opt.text_arrays && ix.text2 && need < free_b) {
			CS_TRY(e->d_lcp.reserve((size_t)rows + 64)); CS_TRY(e->d_rep.reserve((size_t)rows + 64));
			unsigned grid = (unsigned)std::min<uint64_t>((rows + 256) / 256, 1u << 22);
			if (ix.fsa40) {
				hipLaunchKernelGGL(lcp_fill_kernel<Pack40>, dim3(grid), dim3(256), 0, c.stream, ix, Pack40{e->d_fsa40.p}, e->d_lcp.p);
				hipLaunchKernelGGL(rep_fill_kernel<Pack40>, dim3(grid), dim3(256), 0, c.stream, ix, Pack40{e->d_fsa40.p}, (const uint8_t *)e->d_lcp.p, e->d_rep.p, (uint64_t *)nullptr);
			} else if (ix.fsa32) {
				hipLaunchKernelGGL(lcp_fill_kernel<Plain<uint32_t>>, dim3(grid), dim3(256), 0, c.stream, ix, Plain<uint32_t>{e->d_fsa32.p}, e->d_lcp.p);
				hipLaunchKernelGGL(rep_fill_kernel<Plain<uint32_t>>, dim3(grid), dim3(256), 0, c.stream, ix, Plain<uint32_t>{e->d_fsa32.p}, (const uint8_t *)e->d_lcp.p, e->d_rep.p, (uint64_t *)nullptr);
			} else {
				hipLaunchKernelGGL(lcp_fill_kernel<Plain<uint64_t>>, dim3(grid), dim3(256), 0, c.stream, ix, Plain<uint64_t>{e->d_fsa64.p}, e->d_lcp.p);
				hipLaunchKernelGGL(rep_fill_kernel<Plain<uint64_t>>, dim3(grid), dim3(256), 0, c.stream, ix, Plain<uint64_t>{e->d_fsa64.p}, (const uint8_t *)e->d_lcp.p, e->d_rep.p, e->d_isa64.p);
			}
			HIP_TRY(hipGetLastError()); HIP_TRY(hipStreamSynchronize(c.stream));
			ix.lcp = e->d_lcp.p; ix.rep = e->d_rep.p; ix.isa_fused = ix.isa64 ? 1u : 0u;
		}
		if (verbose) {
			HIP_TRY(hipMemGetInfo(&free_b, &total_b));
			fprintf(stderr, "[cs_engine] re-seeding from the text: %s; device memory free %.1f of %.1f GB\n", ix.rep ? "on" : "off", free_b / 1e9, total_b / 1e9); fflush(stderr);
		}
	}
	// round-3 jump table (smem_fwd.hpp): every 15-mer, 17 GB (13: 1 GB, measured 2 % slower); CS_JUMP_K = 0 disables
	{
		const int jk = opt.jump_k;
		size_t free_b = 0, total_b = 0;
		HIP_TRY(hipMemGetInfo(&free_b, &total_b));
		if (jk >= 6 && jk <= 15 && ((size_t)16 << (2 * jk)) + ((size_t)8 << 30) < free_b) {
			CS_TRY(e->d_jump.reserve((size_t)1 << (2 * jk)));
			hipLaunchKernelGGL(jump_fill_kernel, dim3((unsigned)(e->n_cu * 32)), dim3(256), 0, c.stream, ix, jk, e->d_jump.p);
			HIP_TRY(hipGetLastError()); HIP_TRY(hipStreamSynchronize(c.stream));
			e->jump_k = jk;
		}
	}
	CS_TRY(seed_pass_init(e));
	if (verbose) { fprintf(stderr, "[cs_engine] full suffix array: %s\n", ix.fsa32 ? "4-byte" : ix.fsa64 ? "8-byte" : ix.fsa40 ? "5-byte" : "off"); fflush(stderr); }
	return CS_OK;
}

extern "C" int cs_engine_create(const cs_index_view_t *index, int device, cs_engine_t **out)
{
	return cs_engine_create_opts(index, device, nullptr, out);
}
extern "C" int cs_engine_create_opts(const cs_index_view_t *index, int device, const cs_engine_options_t *opts, cs_engine_t **out)
{
	if (!index || !out || !index->bwt || !index->sa) return fail(CS_EINVAL, "cs_engine_create: null argument");
	*out = nullptr;
	cs_engine *e = new cs_engine();
	e->device = device;
	if (opts) e->opt = *opts; else cs_engine_options_default(&e->opt);
	int rc = engine_init(e, index);
	if (rc != CS_OK) { std::string keep = g_err; cs_engine_destroy(e); g_err = keep; return rc; }
	*out = e;
	return CS_OK;
}

extern "C" void cs_engine_destroy(cs_engine_t *e)
{
	if (!e) return;
	(void)hipSetDevice(e->device);
	// The teardown order, also for an engine whose creation failed half-way (any of these may not exist yet):
	//   1. both pipes' threads are stopped and joined: nothing queues work any more;
	//   2. every pass context's four streams are drained: the seeding thread queued pack kernels on the context's stream, and those
	//      write the host pipeline's pack slots;
	//   3. the copy streams are drained: the downloads read the pack slots and write the pinned result slots;
	//   4. only then is any pipeline buffer freed (the members' destructors, whoever owns them).
	pipes_stop(e);
	for (auto &c : e->ctx)
		if (c) for (hipStream_t s : {c->stream.h, c->stream2.h, c->stream3.h, c->stream4.h}) if (s) (void)hipStreamSynchronize(s);
	host_pipe_drain(e);
	delete e;
}

extern "C" int cs_engine_stats(const cs_engine_t *e, cs_stats_t *st)
{
	if (!e || !st) return fail(CS_EINVAL, "null argument");
	memset(st, 0, sizeof *st);
	for (auto &c : e->ctx) { // every pass context counts
		if (!c) continue;
		const cs_stats_t &t = c->st;
		st->reads += t.reads; st->bases += t.bases; st->mems += t.mems; st->seeds += t.seeds; st->bwt_queries += t.bwt_queries; st->bwt_calls += t.bwt_calls;
		st->sal_queries += t.sal_queries; st->sal_calls += t.sal_calls; st->overflow_mems += t.overflow_mems; st->seed_kernel_ms += t.seed_kernel_ms;
		st->sal_kernel_ms += t.sal_kernel_ms; st->total_ms += t.total_ms; st->seed_kernel_launches += t.seed_kernel_launches; st->overflow_kernel_ms += t.overflow_kernel_ms;
		st->overflow_kernel_launches += t.overflow_kernel_launches; st->reseed_text_calls += t.reseed_text_calls; st->reseed_index_calls += t.reseed_index_calls;
		st->sweep_text_calls += t.sweep_text_calls; st->r3_text_seeds += t.r3_text_seeds;
	}
	return CS_OK;
}
extern "C" int cs_engine_memory(const cs_engine_t *e, cs_memory_t *out)
{
	if (!e || !out) return fail(CS_EINVAL, "null argument");
	memset(out, 0, sizeof *out);
	auto bytes = [](const auto &b) { return (uint64_t)b.cap * sizeof(*b.p); };
	// the index-side buffers do not change once the engine exists; the rest comes from counters the passes publish
	out->occ_bwt = bytes(e->d_bwt); out->sampled_sa = bytes(e->d_sa);
	out->full_sa = bytes(e->d_fsa32) + bytes(e->d_fsa64) + bytes(e->d_fsa40);
	out->isa = bytes(e->d_isa32) + bytes(e->d_isa64) + bytes(e->d_isa40);
	out->text = bytes(e->d_text2); out->lcp_rep = bytes(e->d_lcp) + bytes(e->d_rep); out->jump_table = bytes(e->d_jump);
	out->kmer_filter = e->bloom_bytes.load(std::memory_order_relaxed);
	out->total = out->occ_bwt + out->sampled_sa + out->full_sa + out->isa + out->text + out->lcp_rep + out->jump_table + out->kmer_filter;
	for (int i = 0; i < 2; ++i) {
		out->pass_ctx[i] = e->ctx_bytes[i].load(std::memory_order_relaxed);
		if (i == 0) out->pass_ctx[0] += e->held_bytes.load(std::memory_order_relaxed); // the result set of cs_engine_collect_device belongs to no context
		out->total += out->pass_ctx[i];
		if (out->pass_ctx[i]) out->n_pass_ctx = i + 1;
	}
	out->sa_entry_bits = e->ix.fsa32 ? 32 : e->ix.fsa64 ? 64 : e->ix.fsa40 ? 40 : 0;
	return CS_OK;
}
extern "C" void cs_engine_reset_stats(cs_engine_t *e)
{
	if (!e || pipe_busy(e)) return; // (the seeding thread owns the counters while batches are in flight)
	(void)hipSetDevice(e->device);
	for (auto &c : e->ctx) {
		if (!c) continue;
		memset(&c->st, 0, sizeof c->st);
		c->stream_bytes = 0;
		(void)hipMemsetAsync(c->d_evc.p, 0, (size_t)N_KID * N_EV * sizeof(unsigned long long), c->stream);
		(void)hipStreamSynchronize(c->stream);
	}
}
extern "C" int cs_engine_traffic_model(cs_engine_t *e, cs_traffic_t *out)
{
	if (!e || !out) return fail(CS_EINVAL, "null argument");
	if (pipe_busy(e)) return fail(CS_EINVAL, "cs_engine_traffic_model: submitted batches are in flight, collect them first");
	HIP_TRY(hipSetDevice(e->device));
	memset(out->events, 0, sizeof out->events);
	uint64_t stream_bytes = 0;
	std::vector<unsigned long long> ev((size_t)N_KID * N_EV);
	for (auto &c : e->ctx) { // every pass context counts
		if (!c) continue;
		HIP_TRY(hipMemcpyAsync(ev.data(), c->d_evc.p, ev.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
		for (int a = 0; a < N_KID; ++a) for (int b = 0; b < N_EV; ++b) out->events[a][b] += ev[(size_t)a * N_EV + b];
		stream_bytes += c->stream_bytes;
	}
	const uint64_t sa_b = e->ix.fsa64 ? 8 : e->ix.fsa40 ? 5 : 4;
	const uint64_t eb[N_EV] = {32, 16, 8, sa_b, sa_b, 4, 8, 1, 16, 32};
	for (int i = 0; i < N_EV; ++i) out->event_bytes[i] = eb[i];
	out->stream_bytes = stream_bytes;
	return CS_OK;
}

// ------------------------------------------------------------------------------------------------ device memory helpers
extern "C" int cs_device_alloc(cs_engine_t *e, size_t bytes, void **dptr)
{
	if (!e || !dptr) return fail(CS_EINVAL, "null argument");
	HIP_TRY(hipSetDevice(e->device));
	HIP_TRY(hipMalloc(dptr, bytes ? bytes : 1));
	return CS_OK;
}
extern "C" int cs_device_free(cs_engine_t *e, void *dptr)
{
	if (!e) return fail(CS_EINVAL, "null argument");
	HIP_TRY(hipSetDevice(e->device));
	HIP_TRY(hipFree(dptr));
	return CS_OK;
}
extern "C" int cs_device_upload(cs_engine_t *e, void *dst, const void *src, size_t bytes)
{
	if (!e || (bytes && (!dst || !src))) return fail(CS_EINVAL, "null argument");
	HIP_TRY(hipSetDevice(e->device));
	HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->ctx[0]->stream));
	HIP_TRY(hipStreamSynchronize(e->ctx[0]->stream));
	return CS_OK;
}
extern "C" int cs_device_download(cs_engine_t *e, void *dst, const void *src, size_t bytes)
{
	if (!e || (bytes && (!dst || !src))) return fail(CS_EINVAL, "null argument");
	HIP_TRY(hipSetDevice(e->device));
	HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->ctx[0]->stream));
	HIP_TRY(hipStreamSynchronize(e->ctx[0]->stream));
	return CS_OK;
}
extern "C" int cs_device_sync(cs_engine_t *e)
{
	if (!e) return fail(CS_EINVAL, "null argument");
	HIP_TRY(hipSetDevice(e->device));
	HIP_TRY(hipStreamSynchronize(e->ctx[0]->stream));
	return CS_OK;
}
