// inspect.hip -- looking at what the engine holds: digest and gather of the last result, validation of the resident index, the FM-index
// primitives (tests) and the random-line probe.
#include "engine.hpp"

#include <string>

#include <rocprim/device/device_scan.hpp>

// ------------------------------------------------------------------------------------------------ digest / gather of the last result
__device__ __forceinline__ uint64_t splitmix64(uint64_t z)
{
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}
__global__ void digest_kernel(const uint64_t *w, uint64_t n, unsigned long long *out)
{
	unsigned long long acc = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
		acc += splitmix64(w[i] + i * 0x9E3779B97F4A7C15ull);
	for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
	if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}
extern "C" int cs_engine_result_digest(cs_engine_t *e, cs_digest_t *out)
{
	if (!e || !out) return fail(CS_EINVAL, "null argument");
	PassCtx *c = e->last_ctx ? e->last_ctx : e->ctx[0].get(); // the pass context that holds the result; everything below runs on it
	if (!c->last.valid || pipe_busy(e)) return fail(CS_EINVAL, "cs_engine_result_digest: no whole-batch result is held on the device (call a seed function first)");
	HIP_TRY(hipSetDevice(e->device));
	hipStream_t s = c->stream;
	HIP_TRY(hipMemsetAsync(c->d_ctr.p, 0, 4 * sizeof(unsigned long long), s));
	const uint64_t n = (uint64_t)c->last.n_reads;
	const unsigned g = (unsigned)e->n_cu * 8;
	const LastArrays r = last_arrays(e, c);
	hipLaunchKernelGGL(digest_kernel, dim3(g), dim3(256), 0, s, r.mem_off, n + 1, c->d_ctr.p + 0);
	if (c->last.n_mems) hipLaunchKernelGGL(digest_kernel, dim3(g), dim3(256), 0, s, (const uint64_t *)r.mems, c->last.n_mems * 4, c->d_ctr.p + 1);
	if (c->last.want_sal) {
		hipLaunchKernelGGL(digest_kernel, dim3(g), dim3(256), 0, s, r.seed_off, n + 1, c->d_ctr.p + 2);
		if (c->last.n_seeds) hipLaunchKernelGGL(digest_kernel, dim3(g), dim3(256), 0, s, (const uint64_t *)r.seeds, c->last.n_seeds * 2, c->d_ctr.p + 3);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(c->h_ctr.p, c->d_ctr.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	out->mem_off = c->h_ctr.p[0]; out->mems = c->h_ctr.p[1]; out->seed_off = c->h_ctr.p[2]; out->seeds = c->h_ctr.p[3];
	return CS_OK;
}

__global__ void sel_counts_kernel(const uint64_t *ids, int64_t n_sel, uint64_t n_reads, const uint64_t *mem_off, const uint64_t *seed_off,
                                  uint64_t *cm, uint64_t *cs, unsigned long long *bad)
{
	int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t > n_sel) return;
	if (t == n_sel) { cm[t] = 0; if (cs) cs[t] = 0; return; }
	const uint64_t r = ids[t];
	if (r >= n_reads) { atomicAdd(bad, 1ull); cm[t] = 0; if (cs) cs[t] = 0; return; }
	cm[t] = mem_off[r + 1] - mem_off[r];
	if (cs) cs[t] = seed_off[r + 1] - seed_off[r];
}
// 16 lanes per selected read copy its mems and seeds
__global__ void sel_copy_kernel(const uint64_t *ids, int64_t n_sel, const uint64_t *mem_off, const uint64_t *seed_off, const OutMem *mems, const OutSeed *seeds,
                                const uint64_t *om, const uint64_t *os, OutMem *out_m, OutSeed *out_s)
{
	const int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
	const uint32_t a = threadIdx.x & 15u;
	if (t >= n_sel) return;
	const uint64_t r = ids[t];
	for (uint64_t j = a, n = om[t + 1] - om[t]; j < n; j += 16) out_m[om[t] + j] = mems[mem_off[r] + j];
	if (seeds) for (uint64_t j = a, n = os[t + 1] - os[t]; j < n; j += 16) out_s[os[t] + j] = seeds[seed_off[r] + j];
}
extern "C" int cs_engine_gather_reads(cs_engine_t *e, int64_t n_sel, const uint64_t *read_ids, cs_result_t *out)
{
	if (!e || !out || n_sel < 0 || (n_sel > 0 && !read_ids)) return fail(CS_EINVAL, "cs_engine_gather_reads: bad argument");
	PassCtx *c = e->last_ctx ? e->last_ctx : e->ctx[0].get(); // the pass context that holds the result; everything below runs on it
	if (!c->last.valid || pipe_busy(e)) return fail(CS_EINVAL, "cs_engine_gather_reads: no whole-batch result is held on the device (call a seed function first)");
	HIP_TRY(hipSetDevice(e->device));
	hipStream_t s = c->stream;
	const bool sal = c->last.want_sal != 0;
	const LastArrays r = last_arrays(e, c);
	CS_TRY(e->d_sel.reserve((size_t)n_sel + 1)); CS_TRY(e->d_sel_moff.reserve((size_t)n_sel + 2)); CS_TRY(e->d_sel_soff.reserve((size_t)n_sel + 2));
	CS_TRY(c->d_tmp.reserve(((size_t)n_sel + 2) * 16 + 1024));
	uint64_t *cm = (uint64_t *)c->d_tmp.p, *cs = cm + n_sel + 1;
	if (n_sel) HIP_TRY(hipMemcpyAsync(e->d_sel.p, read_ids, (size_t)n_sel * 8, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemsetAsync(c->d_ctr.p + 4, 0, sizeof(unsigned long long), s));
	hipLaunchKernelGGL(sel_counts_kernel, dim3(grid_for(n_sel + 1, 256)), dim3(256), 0, s, (const uint64_t *)e->d_sel.p, n_sel, (uint64_t)c->last.n_reads,
	                   r.mem_off, sal ? r.seed_off : nullptr, cm, sal ? cs : nullptr, c->d_ctr.p + 4);
	{
		size_t tb = 0;
		HIP_TRY(rocprim::exclusive_scan(nullptr, tb, cm, e->d_sel_moff.p, (uint64_t)0, (size_t)n_sel + 1, rocprim::plus<uint64_t>(), s));
		CS_TRY(c->d_tmp2.reserve(tb + 16));
		HIP_TRY(rocprim::exclusive_scan((void *)c->d_tmp2.p, tb, cm, e->d_sel_moff.p, (uint64_t)0, (size_t)n_sel + 1, rocprim::plus<uint64_t>(), s));
		if (sal) HIP_TRY(rocprim::exclusive_scan((void *)c->d_tmp2.p, tb, cs, e->d_sel_soff.p, (uint64_t)0, (size_t)n_sel + 1, rocprim::plus<uint64_t>(), s));
	}
	CS_TRY(e->h_mem_off.reserve((size_t)n_sel + 1));
	HIP_TRY(hipMemcpyAsync(e->h_mem_off.p, e->d_sel_moff.p, ((size_t)n_sel + 1) * 8, hipMemcpyDeviceToHost, s));
	if (sal) { CS_TRY(e->h_seed_off.reserve((size_t)n_sel + 1)); HIP_TRY(hipMemcpyAsync(e->h_seed_off.p, e->d_sel_soff.p, ((size_t)n_sel + 1) * 8, hipMemcpyDeviceToHost, s)); }
	HIP_TRY(hipMemcpyAsync(c->h_ctr.p + 4, c->d_ctr.p + 4, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if (c->h_ctr.p[4]) return fail(CS_EINVAL, "cs_engine_gather_reads: read id out of range");
	const uint64_t nm = e->h_mem_off.p[n_sel], ns = sal ? e->h_seed_off.p[n_sel] : 0;
	CS_TRY(e->d_sel_mems.reserve((size_t)nm + 1)); CS_TRY(e->h_mems.reserve((size_t)nm + 1));
	if (sal) { CS_TRY(e->d_sel_seeds.reserve((size_t)ns + 1)); CS_TRY(e->h_seeds.reserve((size_t)ns + 1)); }
	if (n_sel) hipLaunchKernelGGL(sel_copy_kernel, dim3(grid_for(n_sel * 16, 256)), dim3(256), 0, s, (const uint64_t *)e->d_sel.p, n_sel, r.mem_off,
	                              r.seed_off, r.mems, sal ? r.seeds : nullptr,
	                              (const uint64_t *)e->d_sel_moff.p, (const uint64_t *)e->d_sel_soff.p, e->d_sel_mems.p, e->d_sel_seeds.p);
	HIP_TRY(hipGetLastError());
	if (nm) HIP_TRY(hipMemcpyAsync(e->h_mems.p, e->d_sel_mems.p, (size_t)nm * sizeof(OutMem), hipMemcpyDeviceToHost, s));
	if (ns) HIP_TRY(hipMemcpyAsync(e->h_seeds.p, e->d_sel_seeds.p, (size_t)ns * sizeof(OutSeed), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	out->n_reads = n_sel; out->n_mems = nm; out->n_seeds = ns;
	out->mem_off = e->h_mem_off.p; out->mems = (const cs_intv_t *)e->h_mems.p;
	out->seed_off = sal ? e->h_seed_off.p : nullptr; out->seeds = sal ? (const cs_seed_t *)e->h_seeds.p : nullptr;
	return CS_OK;
}

// ------------------------------------------------------------------------------------------------ index validation at the size it is used
// The index a 3.1 Gbp engine runs on is built on the GPU in the same process (index_build.hip), and the arrays the shortcuts read are derived
// from it at engine creation; the byte-for-byte comparisons with bwaidx stop at 64 Mbp.  This check is independent of how any of it was
// made: (1) the recovered 2-bit text equals the caller's genome and its reverse complement; (2) every pair of neighbouring rows of the
// full suffix array is in suffix order, decided by comparing the TEXT (end of text smallest, as the sentinel); (3) ISA[SA[r]] = r, so
// SA is a permutation; (4) the BWT character of row r is T[SA[r] - 1] and the row of suffix 0 is `primary`; (5) the sampled suffix
// array of the file equals the full one at the sampled rows.  (1)-(3) make SA THE suffix array of the given text, (4)-(5) tie the
// reference's two files to it (FM_index/bwt.c:62-96, index_main.c:152-174).
__global__ void check_text_kernel(const DevIndex ix, const uint8_t *fwd, uint64_t l_pac, unsigned long long *bad)
{
	unsigned long long c = 0;
	for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < l_pac; p += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t q = 2 * l_pac - 1 - p;                       // the position of base p on the reverse-complement strand
		const uint32_t f = fwd[p] & 3u;
		const uint32_t a = (ix.text2[p >> 4] >> ((p & 15) << 1)) & 3u, b = (ix.text2[q >> 4] >> ((q & 15) << 1)) & 3u;
		c += (a != f) + (b != 3u - f);
	}
	for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
	if ((threadIdx.x & 63) == 0 && c) atomicAdd(bad, c);
}
__global__ void check_rows_kernel(const DevIndex ix, uint32_t cap, unsigned long long *out /* [0] order [1] isa [2] bwt [3] sampled SA [4] undecided (LCP beyond cap) */)
{
	unsigned long long v[5] = {0, 0, 0, 0, 0};
	const uint32_t *t2 = ix.text2;
	auto base = [&](uint64_t p) { return (t2[p >> 4] >> ((p & 15) << 1)) & 3u; };
	for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; r <= ix.seq_len; r += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t a = r == 1 ? ix.seq_len : sa_direct(ix, r - 1), b = sa_direct(ix, r);
		if (b >= ix.seq_len || a > ix.seq_len) { ++v[0]; continue; }
		const uint32_t l = text_lcp(ix, a, b, cap);
		if (l >= cap) ++v[4];
		else if (!(a + l == ix.seq_len || (b + l < ix.seq_len && base(a + l) < base(b + l)))) ++v[0];
		if (isa_direct(ix, b) != r) ++v[1];
		else if (ix.isa_fused && (uint32_t)(ix.isa64[b] >> 56) != (uint32_t)ix.rep[b]) ++v[1]; // the rep byte that rides in the entry
		if (b == 0) { if (r != ix.primary) ++v[2]; }
		else {
			if (r == ix.primary) ++v[2];
			else {
				const uint64_t row = r - (r > ix.primary);
				const Block k = load_block(ix, row >> OCC_SHIFT);
				const uint32_t p = (uint32_t)row & OCC_MASK, w = p >> 5, bit = p & 31;
				const uint32_t lo = w == 0 ? k.pl.x : k.pl.y, hi = w == 0 ? k.pl.z : k.pl.w;
				if ((((lo >> bit) & 1u) | (((hi >> bit) & 1u) << 1)) != base(b - 1)) ++v[2];
			}
		}
		if ((r & ix.sa_mask) == 0 && ix.sa[r >> ix.sa_shift] != b) ++v[3];
	}
	for (int i = 0; i < 5; ++i) {
		unsigned long long c = v[i];
		for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
		if ((threadIdx.x & 63) == 0 && c) atomicAdd(out + i, c);
	}
}
extern "C" int cs_engine_check_index(cs_engine_t *e, const uint8_t *d_fwd_nt4, uint64_t l_pac, cs_index_check_t *out)
{
	if (!e || !out) return fail(CS_EINVAL, "cs_engine_check_index: null argument");
	if (pipe_busy(e)) return fail(CS_EINVAL, "cs_engine_check_index: submitted batches are in flight, collect them first");
	if (!e->ix.text2 || !has_full_sa(e->ix)) return fail(CS_EINVAL, "cs_engine_check_index: needs the full suffix array and the text arrays (engine options full_sa, text_mode)");
	if (d_fwd_nt4 && 2 * l_pac != e->ix.seq_len) return fail(CS_EINVAL, "cs_engine_check_index: l_pac is not half of the index length");
	HIP_TRY(hipSetDevice(e->device));
	PassCtx *c = e->ctx[0].get();
	hipStream_t s = c->stream;
	HIP_TRY(hipMemsetAsync(c->d_ctr.p, 0, 8 * sizeof(unsigned long long), s));
	const unsigned grid = (unsigned)e->n_cu * 16;
	if (d_fwd_nt4) hipLaunchKernelGGL(check_text_kernel, dim3(grid), dim3(256), 0, s, e->ix, d_fwd_nt4, l_pac, c->d_ctr.p + 5);
	hipLaunchKernelGGL(check_rows_kernel, dim3(grid), dim3(256), 0, s, e->ix, 1u << 20, c->d_ctr.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(c->h_ctr.p, c->d_ctr.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	out->rows_checked = e->ix.seq_len; out->order_violations = c->h_ctr.p[0]; out->isa_violations = c->h_ctr.p[1]; out->bwt_violations = c->h_ctr.p[2];
	out->sampled_sa_violations = c->h_ctr.p[3]; out->undecided_rows = c->h_ctr.p[4]; out->text_violations = c->h_ctr.p[5]; out->text_checked = d_fwd_nt4 ? 1 : 0;
	return CS_OK;
}

// ------------------------------------------------------------------------------------------------ primitives (tests)
namespace csd {

__global__ void occ4_kernel(const DevIndex ix, const uint64_t *k, uint64_t *cnt, int64_t n)
{
	int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) return;
	uint64_t c[4]; occ4(ix, k[t], c);
	cnt[4 * t] = c[0]; cnt[4 * t + 1] = c[1]; cnt[4 * t + 2] = c[2]; cnt[4 * t + 3] = c[3];
}
__global__ void extend_kernel(const DevIndex ix, const OutMem *ik, const uint8_t *is_back, OutMem *ok, int64_t n)
{
	int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) return;
	Intv64 v64 = {ik[t].x0, ik[t].x1, ik[t].x2}, o[4];
	extend4(ix, v64, is_back[t] != 0, o);
	const bool small = ik[t].x2 < (1ull << 32);            // the single-child forms serve the search: sizes below 2^32
	Intv v = {ik[t].x0, ik[t].x1, (uint32_t)ik[t].x2};
	for (int c = 0; c < 4; ++c) {
		OutMem m = {o[c].x0, o[c].x1, o[c].x2, 0};
		ok[4 * t + c] = m;
		// the single-child paths used by the search must agree with the four-child one
		NoCtr W;
		Intv o1 = extend1_rt(ix, v, is_back[t] != 0, c, W);
		Intv o2 = is_back[t] ? extend1<true>(ix, v, c, W) : extend1<false>(ix, v, c, W);
		if (small && v.x0 != 0 && v.x1 != 0 && (o2.x0 != o[c].x0 || o2.x1 != o[c].x1 || o2.x2 != o[c].x2)) ok[4 * t + c].info = 2;
		if (small && (o1.x0 != o[c].x0 || o1.x1 != o[c].x1 || o1.x2 != o[c].x2)) ok[4 * t + c].info = 1;
	}
}
__global__ void sa_kernel(const DevIndex ix, const uint64_t *k, uint64_t *sa, int64_t n)
{
	int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) return;
	uint64_t walked = sa_lookup(ix, k[t]);
	// when the full suffix array is resident it must agree with the walk on every row (mismatch => poison the answer)
	if (has_full_sa(ix) && sa_direct(ix, k[t]) != walked) walked = 0xdeadbeefdeadbeefull;
	sa[t] = walked;
}

} // namespace csd

template <typename In, typename Out, typename Launch>
static int run_prim(cs_engine *e, int64_t n, const In *h_in, size_t in_per, Out *h_out, size_t out_per, const uint8_t *h_flag, Launch launch)
{
	if (!e || n < 0 || (n > 0 && (!h_in || !h_out))) return fail(CS_EINVAL, "bad argument");
	if (n == 0) return CS_OK;
	HIP_TRY(hipSetDevice(e->device));
	DevBuf<In> d_in; DevBuf<Out> d_out; DevBuf<uint8_t> d_flag;
	CS_TRY(d_in.reserve((size_t)n * in_per));
	CS_TRY(d_out.reserve((size_t)n * out_per));
	if (h_flag) { CS_TRY(d_flag.reserve((size_t)n)); HIP_TRY(hipMemcpy(d_flag.p, h_flag, (size_t)n, hipMemcpyHostToDevice)); }
	HIP_TRY(hipMemcpy(d_in.p, h_in, (size_t)n * in_per * sizeof(In), hipMemcpyHostToDevice));
	launch(d_in.p, d_flag.p, d_out.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(e->ctx[0]->stream));
	HIP_TRY(hipMemcpy(h_out, d_out.p, (size_t)n * out_per * sizeof(Out), hipMemcpyDeviceToHost));
	return CS_OK;
}

extern "C" int cs_engine_occ4(cs_engine_t *e, int64_t n, const uint64_t *k, uint64_t *cnt4)
{
	return run_prim<uint64_t, uint64_t>(e, n, k, 1, cnt4, 4, nullptr, [&](const uint64_t *di, const uint8_t *, uint64_t *dout) {
		hipLaunchKernelGGL(occ4_kernel, dim3(grid_for(n, 256)), dim3(256), 0, e->ctx[0]->stream, e->ix, di, dout, n);
	});
}
extern "C" int cs_engine_extend(cs_engine_t *e, int64_t n, const cs_intv_t *ik, const uint8_t *is_back, cs_intv_t *ok4)
{
	if (n > 0 && !is_back) return fail(CS_EINVAL, "is_back is null");
	return run_prim<OutMem, OutMem>(e, n, (const OutMem *)ik, 1, (OutMem *)ok4, 4, is_back, [&](const OutMem *di, const uint8_t *df, OutMem *dout) {
		hipLaunchKernelGGL(extend_kernel, dim3(grid_for(n, 256)), dim3(256), 0, e->ctx[0]->stream, e->ix, di, df, dout, n);
	});
}
extern "C" int cs_engine_sa(cs_engine_t *e, int64_t n, const uint64_t *k, uint64_t *sa)
{
	if (e) for (int64_t i = 0; i < n; ++i) if (k && k[i] > e->ix.seq_len) return fail(CS_EINVAL, "SA row out of range");
	return run_prim<uint64_t, uint64_t>(e, n, k, 1, sa, 1, nullptr, [&](const uint64_t *di, const uint8_t *, uint64_t *dout) {
		hipLaunchKernelGGL(sa_kernel, dim3(grid_for(n, 256)), dim3(256), 0, e->ctx[0]->stream, e->ix, di, dout, n);
	});
}

// ------------------------------------------------------------------------------------------------ access-shape micro-benchmark
// Dependent chains of random 64-byte Occ-block reads, one chain per lane, nothing else: the ceiling of this access shape on
// the resident index (SURVEY 8d asks for it next to the roofline).  Returns lines per second.
__global__ void random_block_chain_kernel(const DevIndex ix, uint32_t steps, uint64_t *sink)
{
	uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 0x9E3779B97F4A7C15ull + 12345;
	for (uint32_t i = 0; i < steps; ++i) {
		uint64_t b = (k >> 11) % (2 * ix.n_blocks); // 32-byte records
		Block blk = load_block(ix, b);
		k = k * 6364136223846793005ull + (blk.cnt.x ^ blk.cnt.w ^ blk.pl.y ^ blk.pl.z) + 1442695040888963407ull;
	}
	if (k == 42) *sink = k;
}
extern "C" int cs_engine_probe_random_lines(cs_engine_t *e, int waves_per_simd, int steps, double *lines_per_sec)
{
	if (!e || !lines_per_sec || waves_per_simd < 1 || waves_per_simd > 8 || steps < 1) return fail(CS_EINVAL, "bad argument");
	HIP_TRY(hipSetDevice(e->device));
	unsigned blocks = (unsigned)(e->n_cu * waves_per_simd); // 256-thread blocks: 4 waves each => waves_per_simd blocks per CU
	PassCtx *c = e->ctx[0].get();
	HIP_TRY(hipEventRecord(c->ev[0], c->stream));
	hipLaunchKernelGGL(random_block_chain_kernel, dim3(blocks), dim3(256), 0, c->stream, e->ix, (uint32_t)steps, (uint64_t *)c->d_ctr.p + 7);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c->ev[1], c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
	*lines_per_sec = (double)blocks * 256.0 * steps / (ms * 1e-3);
	return CS_OK;
}
