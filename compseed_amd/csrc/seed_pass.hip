// seed_pass.hip -- one seeding pass on a pass context: the SMEM stage (split kernels, fused fallback), compaction and SAL, the k-mer
// filter of the window lanes, and the pass entry every caller goes through (run_pass).
//
// Host-side counterpart of mem_process_seqs -> seed_and_extend (mapping/comp_seed.cpp:2527, 2242) for the seeding
// and SAL blocks only.
#include "engine.hpp"
#include "seed_kernels.hpp"
#include "smem_common.hpp"
#include "smem_reads.hpp"
#include "smem_fwd.hpp"
#include "smem_bwd.hpp"
#include "smem_text.hpp"
#include "smem_sort.hpp"

#include <cstdio>
#include <mutex>
#include <shared_mutex>
#include <string>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

// A pass context with its streams and events, and the counters and tables its passes start from.  Context 0 is made at engine
// creation, context 1 on the first call that can use two passes at a time.
int add_pass_ctx(cs_engine *e)
{
	const int ci = e->ctx[0] ? 1 : 0;
	std::unique_ptr<PassCtx> c(new PassCtx());
	int lo = 0, hi = 0;
	(void)hipDeviceGetStreamPriorityRange(&lo, &hi); // lo = least urgent
	for (HipStream *st : {&c->stream, &c->stream2, &c->stream3, &c->stream4}) {
		if (st == &c->stream2) HIP_TRY(hipStreamCreateWithPriority(&st->h, hipStreamNonBlocking, lo));
		else HIP_TRY(hipStreamCreateWithFlags(&st->h, hipStreamNonBlocking));
	}
	for (auto &ev : c->ev) HIP_TRY(hipEventCreate(&ev.h)); // these are timed
	for (HipEvent *ev : {&c->ev_r3a, &c->ev_r3b, &c->ev_wa, &c->ev_wb, &c->ev_wc}) HIP_TRY(hipEventCreateWithFlags(&ev->h, hipEventDisableTiming));
	CS_TRY(c->d_sctr.reserve(SC_WORDS)); CS_TRY(c->h_sctr.reserve(SC_WORDS));
	CS_TRY(c->d_sst2.reserve(SST2_ENTRIES));
	HIP_TRY(hipMemsetAsync(c->d_sst2.p, 0xff, SST2_ENTRIES * sizeof(uint4), c->stream)); // empty second-level SST
	HIP_TRY(hipMemsetAsync(c->d_sctr.p, 0, SC_WORDS * sizeof(unsigned long long), c->stream));
	CS_TRY(c->d_ctr.reserve(CTR_WORDS)); CS_TRY(c->h_ctr.reserve(CTR_WORDS));
	HIP_TRY(hipMemsetAsync(c->d_ctr.p, 0, CTR_WORDS * sizeof(unsigned long long), c->stream));
	static_assert(N_KID == CS_N_KERNELS && N_EV == CS_N_EVENTS, "cs_traffic_t mirrors the device-side event table");
	CS_TRY(c->d_evc.reserve((size_t)N_KID * N_EV));
	HIP_TRY(hipMemsetAsync(c->d_evc.p, 0, (size_t)N_KID * N_EV * sizeof(unsigned long long), c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	c->id = ci;
	note_ctx_bytes(e, c.get());
	e->ctx[ci] = std::move(c);
	if (ci && e->opt.verbose) { fprintf(stderr, "[cs_engine] second pass context created\n"); fflush(stderr); }
	return CS_OK;
}

// ------------------------------------------------------------------------------------------------ helpers
// launch the counting instantiation of a kernel (cs_params_t.count_traffic) or the plain one; in general, one of two instantiations
#define LAUNCH_EITHER(first, K_FIRST, K_OTHER, grid, block, stream, ...)                                       \
	do {                                                                                                       \
		if (first) hipLaunchKernelGGL(K_FIRST, grid, block, 0, stream, __VA_ARGS__);                           \
		else hipLaunchKernelGGL(K_OTHER, grid, block, 0, stream, __VA_ARGS__);                                 \
	} while (0)
#define LAUNCH_CT(count, KERN, grid, stream, ...) LAUNCH_EITHER(count, (KERN<256, true>), (KERN<256, false>), grid, dim3(256), stream, __VA_ARGS__)

// rocPRIM's two-call idiom: call(nullptr, bytes) asks for the size of the temporary storage, `tmp` grows to it, the second call runs
template <typename Call>
static int with_rocprim_tmp(DevBuf<uint8_t> &tmp, Call rocprim_call)
{
	size_t bytes = 0;
	HIP_TRY(rocprim_call(nullptr, bytes));
	CS_TRY(tmp.reserve(bytes + 16));
	HIP_TRY(rocprim_call((void *)tmp.p, bytes));
	return CS_OK;
}

struct U32ToU64 { __device__ uint64_t operator()(uint32_t v) const { return (uint64_t)v; } };

// exclusive prefix sum of n u32 counts into n+1 u64 offsets starting at `init`
static int scan_counts(PassCtx *c, const uint32_t *cnt, uint64_t *off, size_t n, uint64_t init)
{
	auto in = rocprim::make_transform_iterator(cnt, U32ToU64());
	// n+1 outputs: the input iterator is read one past the end, so cnt has a zeroed tail slot
	return with_rocprim_tmp(c->d_tmp, [&](void *tmp, size_t &bytes) {
		return rocprim::exclusive_scan(tmp, bytes, in, off, init, n + 1, rocprim::plus<uint64_t>(), c->stream);
	});
}

__global__ void max_len_kernel(const uint64_t *off, int64_t n, uint64_t n_bases, unsigned long long *out_max, unsigned long long *bad)
{
	unsigned long long len = 0;
	if (blockIdx.x == 0 && threadIdx.x == 0 && (off[0] != 0 || off[n] != n_bases)) atomicAdd(bad, 1ull); // the reads must tile [0, n_bases)
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) { // few waves: few atomics
		uint64_t a = off[r], b = off[r + 1];
		if (b < a || b > n_bases) atomicAdd(bad, 1ull); else if (b - a > len) len = b - a;
	}
	for (int o = 32; o > 0; o >>= 1) { unsigned long long other = __shfl_xor(len, o); len = other > len ? other : len; } // one atomic per wave
	if ((threadIdx.x & 63) == 0) atomicMax(out_max, len);
}
__global__ void collect_overflow_kernel(const uint32_t *cnt, int64_t n, uint32_t cap, uint32_t first_read, uint32_t *list, unsigned long long *n_ovf)
{
	int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n || cnt[r] <= cap) return;
	unsigned long long slot = atomicAdd(n_ovf, 1ull);
	list[slot] = first_read + (uint32_t)r;
}
__global__ void patch_counts_kernel(const uint32_t *cnt2, const uint32_t *list, int64_t n_ovf, uint32_t first_read, uint32_t *cnt)
{
	int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n_ovf) return;
	cnt[list[t] - first_read] = cnt2[t];
}
// second-pass variant of sort_compact_kernel: task t holds read list[t]
template <bool LEAN>
__global__ void sort_compact_list_kernel(const OutMem *raw, const uint32_t *cnt2, uint32_t cap2, const uint32_t *list, int64_t n_tasks,
                                         const uint64_t *mem_off, OutMem *mems)
{
	int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n_tasks) return;
	uint32_t n = cnt2[t];
	const OutMem *src = raw + (size_t)t * cap2;
	OutMem *dst = mems + mem_off[list[t]];
	for (uint32_t a = 0; a < n; ++a) {
		uint64_t ka = src[a].info; uint32_t rank = 0;
		for (uint32_t b = 0; b < n; ++b) { uint64_t kb = src[b].info; rank += (kb < ka) || (kb == ka && b < a); }
		if (LEAN) { OutMem m = src[a]; m.x1 = 0; dst[rank] = m; }
		else dst[rank] = src[a];
	}
}

// SA slots as CompSeed merges them (comp_seed.cpp:2327-2334): identical slots inside one 512-read batch are looked up once.
// key = batch << 37 | slot (slots < 2^37: checked at engine creation); sorted, then the distinct keys are counted.
__global__ void sal_keys_kernel(const OutSeed *seeds, const uint64_t *seed_off, int64_t n_reads, uint64_t *keys)
{
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		const uint64_t hi = (uint64_t)(r >> 9) << 37; // BATCH_SIZE 512, comp_seed.h:36
		for (uint64_t j = seed_off[r]; j < seed_off[r + 1]; ++j) keys[j] = hi | (uint64_t)seeds[j].rbeg;
	}
}
__global__ void count_distinct_kernel(const uint64_t *keys, uint64_t n, unsigned long long *out)
{
	unsigned long long c = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
		c += (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
	for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
	if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

// A few counter words from the device to the host.  Not a hipMemcpyAsync: that would queue behind whatever large transfer the
// copy engine is busy with (the results of the previous sub-batch on their way to the host, cs_engine_seed_batch), and the
// SMEM stage reads its counters back ten times per pass.  A one-wave kernel stores the words straight into pinned host memory.
__global__ void fetch_words_kernel(unsigned long long *dst_host, const unsigned long long *src, int n)
{
	if ((int)threadIdx.x < n) dst_host[threadIdx.x] = src[threadIdx.x];
	__threadfence_system();
}
template <typename T>
static int fetch_words(PinBuf<unsigned long long> &h, size_t at, const T *d_src, int n, hipStream_t s)
{
	static_assert(sizeof(T) == 8, "64-bit words");
	if (h.dp && n <= 64) {
		hipLaunchKernelGGL(fetch_words_kernel, dim3(1), dim3(64), 0, s, h.dp + at, (const unsigned long long *)d_src, n);
		HIP_TRY(hipGetLastError());
	} else HIP_TRY(hipMemcpyAsync(h.p + at, d_src, (size_t)n * 8, hipMemcpyDeviceToHost, s));
	return CS_OK;
}

// two words that do not lie side by side (the running totals of mems and seeds), the same way
__global__ void fetch_pair_kernel(unsigned long long *dst_host, const unsigned long long *a, const unsigned long long *b)
{
	if (threadIdx.x == 0) dst_host[0] = *a;
	if (threadIdx.x == 1) dst_host[1] = *b;
	__threadfence_system();
}
static int fetch_pair(PinBuf<unsigned long long> &h, size_t at, const uint64_t *d_a, const uint64_t *d_b, hipStream_t s)
{
	if (h.dp) {
		hipLaunchKernelGGL(fetch_pair_kernel, dim3(1), dim3(64), 0, s, h.dp + at, (const unsigned long long *)d_a, (const unsigned long long *)d_b);
		HIP_TRY(hipGetLastError());
	} else {
		HIP_TRY(hipMemcpyAsync(h.p + at, d_a, 8, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemcpyAsync(h.p + at + 1, d_b, 8, hipMemcpyDeviceToHost, s));
	}
	return CS_OK;
}

constexpr int SMEM_BLOCK = 256;
// LEP entries kept in LDS per lane by the fused kernel: 20 x 16 B x 256 lanes = 80 KiB per workgroup => two workgroups (8 waves) per
// CU; 10 => 40 KiB => four workgroups (16 waves) per CU, more of the list spilling to global memory (13 and 10 were measured: slower)
constexpr int SMEM_LEP_LDS = 20;

static int launch_smem(const cs_engine *e, PassCtx *c, const cs_params_t *par, const uint64_t *d_off, const uint32_t *d_ids, int64_t n_tasks,
                       OutMem *out, uint32_t *cnt, uint32_t cap, uint32_t max_len)
{
	unsigned blocks = (unsigned)std::min<int64_t>((int64_t)e->n_cu * 2, (n_tasks + SMEM_BLOCK - 1) / SMEM_BLOCK);
	if (blocks == 0) return CS_OK;
	uint32_t spill_cap = max_len + 1 > (uint32_t)SMEM_LEP_LDS ? max_len + 1 - SMEM_LEP_LDS : 1;
	// long reads: fewer resident workgroups rather than an unbounded spill area (one LEP list per lane, worst case = read length)
	size_t per_block = (size_t)SMEM_BLOCK * spill_cap * sizeof(uint4);
	blocks = (unsigned)std::max<size_t>(1, std::min<size_t>(blocks, ((size_t)8 << 30) / per_block));
	CS_TRY(c->d_spill.reserve((size_t)blocks * SMEM_BLOCK * spill_cap));
	SeedArgs A;
	A.ix = e->ix; A.seq = c->d_seq.p; A.off = d_off; A.read_ids = d_ids; A.n_tasks = n_tasks;
	A.out = out; A.out_cnt = cnt; A.cap = cap;
	A.min_seed_len = par->min_seed_len;
	A.split_len = (int)(1.0 * par->min_seed_len * par->split_factor + .499); // comp_seed.cpp:2279 (double arithmetic)
	A.split_width = (uint32_t)par->split_width;
	A.max_mem_intv = par->max_mem_intv;
	A.task_counter = c->d_ctr.p + CTR_TASK; A.spill = c->d_spill.p; A.spill_cap = spill_cap; A.n_queries = c->d_ctr.p + CTR_QUERIES; A.evc = c->d_evc.p;
	HIP_TRY(hipMemsetAsync(c->d_ctr.p + CTR_TASK, 0, sizeof(unsigned long long), c->stream));
	HIP_TRY(hipEventRecord(c->ev[0], c->stream));
	LAUNCH_EITHER(par->count_traffic, (smem_kernel<SMEM_BLOCK, SMEM_LEP_LDS, true>), (smem_kernel<SMEM_BLOCK, SMEM_LEP_LDS, false>), dim3(blocks), dim3(SMEM_BLOCK), c->stream, A);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c->ev[1], c->stream));
	if (d_ids) c->st.overflow_kernel_launches++; else c->st.seed_kernel_launches++;
	return CS_OK;
}

static int add_event_ms(hipEvent_t a, hipEvent_t b, double *acc)
{
	float ms = 0.f;
	HIP_TRY(hipEventElapsedTime(&ms, a, b));
	*acc += ms;
	return CS_OK;
}

// k-mer filter of the text for the window lanes (smem_common.hpp, kmer_filter_*): ~22 bits per text position, one per engine,
// rebuilt when a call uses another min_seed_len (0.3 s at hg19 scale; run_pass, with no pass running)
static int build_kmer_filter(cs_engine *e, int k, hipStream_t s)
{
	if (!e->ix.text2 || k < 8 || k > 24 || !e->opt.kmer_filter) return CS_OK;
	if (e->bloom_k == k) return CS_OK;
	uint32_t bits = 10; // 2^bits words: at least seq_len / 3 of them
	while (bits < 34 && ((uint64_t)1 << bits) * 3 < e->ix.seq_len) ++bits;
	size_t free_b = 0, total_b = 0;
	HIP_TRY(hipMemGetInfo(&free_b, &total_b));
	e->bloom_k = 0;
	if ((((size_t)8) << bits) + ((size_t)24 << 30) >= free_b + e->d_bloom.cap * 8) return CS_OK; // no room: the window lanes do without
	CS_TRY(e->d_bloom.reserve((size_t)1 << bits));
	HIP_TRY(hipMemsetAsync(e->d_bloom.p, 0, ((size_t)8) << bits, s));
	hipLaunchKernelGGL(kmer_filter_fill_kernel, dim3((unsigned)(e->n_cu * 32)), dim3(256), 0, s, e->ix, k, e->d_bloom.p, bits);
	HIP_TRY(hipGetLastError()); HIP_TRY(hipStreamSynchronize(s));
	e->bloom_k = k; e->bloom_bits = bits; e->bloom_tried_k = k;
	e->bloom_bytes.store((uint64_t)e->d_bloom.cap * sizeof(uint64_t), std::memory_order_relaxed);
	return CS_OK;
}

// ------------------------------------------------------------------------------------------------ split SMEM path
// What one run of the split path has settled before its first launch.  count: the counting instantiations (cs_params_t.count_traffic);
// r2text: r2text_kernel answers re-seeding calls; r3_text / r3_async: round 3 after rounds 1/2 from the text, or on the index beside the
// first forward launch; fwd0_on: the first launch of a batch goes through fwd0_kernel
struct SplitRun {
	SplitArgs A;
	int64_t nb;
	uint64_t fq_cap, ovf_cap, chunk;
	bool count, r2text, r3_text, r3_async, fwd0_on;
	bool lean; // CS_RESULT_LEAN: r3text_kernel leaves x1 alone (the sort stores 0 there)
};

// The kernels' arguments for reads [0, nb) of d_off; the iterations set the queue fields (fq, n_f, fq_next, aux_next) per launch.
static SplitArgs split_args(const cs_engine *e, PassCtx *c, const cs_params_t *par, const uint64_t *d_off, int64_t nb, uint32_t max_len, uint32_t dis,
                            uint64_t fq_cap, uint64_t ovf_cap, bool r2text, bool count_slots)
{
	unsigned long long *C = c->d_sctr.p;
	SplitArgs A;
	A.ix = e->ix; A.off = d_off; A.n_reads = nb;
	A.seqp = c->seqp_cur + (d_off - c->off_base); // record index = (off[r] >> 5) + r with r counted from the batch's first read
	if (dis & CS_DISABLE_TEXT_MODE) A.ix.text2 = nullptr;
	A.out = c->d_out.p; A.out_cnt = c->d_cnt.p; A.cap = e->cap;
	A.out_scnt = count_slots ? c->d_scnt.p : nullptr; A.max_occ = (uint32_t)par->max_occ;
	A.ovf = c->d_ovfrec.p; A.ovf_cnt = C + SC_OVF_MEMS; A.ovf_cap = ovf_cap;
	A.min_seed_len = par->min_seed_len;
	A.split_len = (int)(1.0 * par->min_seed_len * par->split_factor + .499); // comp_seed.cpp:2279 (double arithmetic)
	A.split_width = (uint32_t)par->split_width; A.max_mem_intv = par->max_mem_intv;
	A.bq = c->d_bq.p;
	A.lep = c->d_lep.p; A.lep_stride = max_len + 1;
	A.task_ctr = C + SC_TASK; A.n_queries = C + SC_QUERIES; A.err = C + SC_ERR; A.n_sst_hits = C + SC_SST_HITS; A.sst = par->sst_mode;
	A.jump = e->jump_k ? e->d_jump.p : nullptr; A.jump_k = e->jump_k;
	A.evc = c->d_evc.p; A.seq = c->d_seq.p; A.sst2 = c->d_sst2.p;
	A.fq_cap = fq_cap; A.n_f_next = C + SC_NEXT_N; A.n_btasks = C + SC_BTASKS; A.n_text_sweeps = C + SC_TEXT_SWEEPS; A.n_r2_quick = C + SC_R2_TEXT;
	A.text_sweep = ((dis & CS_DISABLE_TEXT_SWEEP) ? 0 : TS_SWEEP) | ((dis & CS_DISABLE_MEM_POS) ? 0 : TS_MEM_POS); // (sst_mode 0: dis = ~0, both off)
	// window scheme for the backward sweeps (smem_bwd.hpp, bwd_win_run): needs the jump table and jump_k <= min_seed_len <= jump_k + 4
	A.win = !(dis & CS_DISABLE_WINDOW) && par->sst_mode != 0 && A.jump && A.jump_k <= A.min_seed_len && A.min_seed_len - 1 <= WIN_LANES ? 1 : 0;
	A.bloom = nullptr; A.bloom_bits = 0;
	if (A.win && !(dis & CS_DISABLE_KMER_FILTER) && e->bloom_k == A.min_seed_len) { A.bloom = e->d_bloom.p; A.bloom_bits = e->bloom_bits; } // k-mer filter for the window lanes (run_pass)
	A.fq = c->d_fqA.p; A.n_f = 0; A.fq_next = c->d_fqB.p; A.aux_next = r2text ? c->d_aux.p : nullptr;
	return A;
}

// Round 3 on the index alone: it depends on nothing, runs on the low-priority second stream and fills the tails of the launches
// of rounds 1 and 2.  At once, beside the first forward launch (measured: best).
static int launch_r3_index(const cs_engine *e, PassCtx *c, const SplitRun &R)
{
	SplitArgs A3 = R.A;
	A3.fq = c->d_fqR.p; A3.n_f = (uint64_t)R.nb; A3.task_ctr = c->d_sctr.p + SC_R3_TASK;
	HIP_TRY(hipEventRecord(c->ev_r3a, c->stream));
	HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_r3a, 0));
	unsigned gr = (unsigned)std::min<uint64_t>((uint64_t)e->n_cu * e->occ_fwd, ((uint64_t)R.nb + 255) / 256);
	LAUNCH_CT(R.count, fwd_kernel, dim3(gr), c->stream2, A3);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c->ev_r3b, c->stream2));
	return CS_OK;
}

// r3text_kernel runs on the second stream beside the late iterations (from the 5th on they carry < 2 % of the tasks but
// still cost a launch chain and a host round trip each); it works from a snapshot of the mem counts.  queue / queue_n: the
// forward queue of the next iteration and its length, or null when nothing is left.
static int launch_r3text(const cs_engine *e, PassCtx *c, const SplitRun &R, const uint64_t *queue, const unsigned long long *queue_n)
{
	hipStream_t s = c->stream;
	const int64_t nb = R.nb;
	// which reads still have calls in the queue (their mem lists are not final; for all others the text answers everything)
	HIP_TRY(hipMemsetAsync(c->d_pending.p, 0, (size_t)nb, s));
	if (queue) hipLaunchKernelGGL(mark_pending_kernel, dim3((unsigned)e->n_cu * 4), dim3(256), 0, s, queue, queue_n, R.fq_cap, nb, c->d_pending.p);
	// the snapshot of the mem counts is taken on the main stream, between two iterations: every entry below a count is complete
	// (on the side stream it could run beside the next iteration's kernels, which bump a count before they store the mem)
	HIP_TRY(hipMemcpyAsync(c->d_cnt_snap.p, c->d_cnt.p, (size_t)nb * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
	HIP_TRY(hipEventRecord(c->ev_r3a, s));
	HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_r3a, 0));
	const dim3 grid((unsigned)std::min<uint64_t>((uint64_t)e->n_cu * 16, ((uint64_t)nb + 255) / 256));
	// (the instantiation follows the index: 8-byte inverse-SA entries that carry rep[] answer "unique? its rank" with one load; and the
	// call: a lean result does not ask for the reverse-strand ranks, which only make x1)
#define LAUNCH_R3TEXT(FUSED, LEAN) hipLaunchKernelGGL((r3text_kernel<FUSED, LEAN>), grid, dim3(256), 0, c->stream2, R.A, (const uint32_t *)c->d_cnt_snap.p, c->d_sctr.p + SC_R3_TEXT_SEEDS, (const uint8_t *)c->d_pending.p)
	if (e->ix.isa_fused) { if (R.lean) LAUNCH_R3TEXT(true, true); else LAUNCH_R3TEXT(true, false); }
	else { if (R.lean) LAUNCH_R3TEXT(false, true); else LAUNCH_R3TEXT(false, false); }
#undef LAUNCH_R3TEXT
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c->ev_r3b, c->stream2));
	return CS_OK;
}

// One chunk of an iteration: the forward passes of the cn calls A.fq[0 .. cn), then their backward sweeps.  first: the batch's
// first iteration.
static int launch_chunk(const cs_engine *e, PassCtx *c, const SplitRun &R, const SplitArgs &A, uint64_t *fq, uint64_t cn, bool first)
{
	hipStream_t s = c->stream;
	unsigned long long *C = c->d_sctr.p;
	const bool count = R.count;
	HIP_TRY(hipMemsetAsync(C + SC_TASK, 0, sizeof(unsigned long long), s));
	HIP_TRY(hipMemsetAsync(C + SC_BTASKS, 0, sizeof(unsigned long long), s));
	HIP_TRY(hipMemsetAsync(c->d_bq.p, 0xff, cn * sizeof(BTask), s)); // slots without a call stay "no class"
	unsigned gf = (unsigned)std::min<uint64_t>((uint64_t)e->n_cu * e->occ_fwd, (cn + 255) / 256);
	if (first && R.fwd0_on) { // the calls at the first base of each read: a kernel without LEPs, backward tasks, SST (smem_fwd.hpp)
		unsigned g0 = (unsigned)std::min<uint64_t>((uint64_t)e->n_cu * 8, (cn + 255) / 256);
		LAUNCH_CT(count, fwd0_kernel, dim3(g0), s, A, fq);
		HIP_TRY(hipMemsetAsync(C + SC_TASK, 0, sizeof(unsigned long long), s));
	}
	LAUNCH_CT(count, fwd_kernel, dim3(gf), s, A);
	HIP_TRY(hipGetLastError());
	// one launch works through all four size classes of the chunk's backward sweeps
	unsigned cap_blocks = (unsigned)(e->n_cu * (A.win ? e->occ_win : e->occ_bwd));
	HIP_TRY(hipMemsetAsync(C + SC_BWD_CLS, 0, 4 * sizeof(unsigned long long), s));
	HIP_TRY(hipEventRecord(c->ev_wa, s)); // forward launch done, counters zeroed
	HIP_TRY(hipStreamWaitEvent(c->stream3, c->ev_wa, 0));
	// side streams: the calls with more than 46 / 64 LEPs, one wave each (few on a mostly unique genome, many on a repeat-rich one;
	// chains of dependent reads, so what counts is waves in flight: six blocks per CU, registers spilled and all, run a
	// repeat-rich genome 6 % faster than four), and the calls without stored LEPs (the bulk of the calls)
	HIP_TRY(hipStreamWaitEvent(c->stream4, c->ev_wa, 0));
	LAUNCH_EITHER(count, bwd_wide_kernel<true>, bwd_wide_kernel<false>, dim3((unsigned)std::min<uint64_t>((uint64_t)e->n_cu * CS_WIDE_BLOCKS, (cn + 255) / 256)), dim3(256), c->stream4, A,
	              (const BTask *)c->d_bq.p, cn, C + SC_BWD_WIDE);
	HIP_TRY(hipEventRecord(c->ev_wc, c->stream4));
	if (A.win)
		LAUNCH_CT(count, bwd_win0_kernel, dim3((unsigned)std::min<uint64_t>((uint64_t)e->n_cu * 8, (cn + 255) / 256)), c->stream3, A, // (sharing the CUs between the two window kernels by grid size was measured: slower in every split)
		          (const BTask *)c->d_bq.p, cn);
	HIP_TRY(hipEventRecord(c->ev_wb, c->stream3));
	if (A.win) LAUNCH_CT(count, bwd_win_kernel, dim3((unsigned)std::min<uint64_t>(cap_blocks, (cn + 7) / 8)), s, A, (const BTask *)c->d_bq.p, cn, C + SC_BWD_CLS);
	else LAUNCH_CT(count, bwd_all_kernel, dim3((unsigned)std::min<uint64_t>(cap_blocks, (cn + 15) / 16)), s, A, (const BTask *)c->d_bq.p, cn, C + SC_BWD_CLS);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamWaitEvent(s, c->ev_wb, 0)); // all must be done before the slots and the LEP arena are reused
	HIP_TRY(hipStreamWaitEvent(s, c->ev_wc, 0));
	return CS_OK;
}

// The iterations: each consumes the forward queue `cur` in chunks and fills the next one, until no call is left.
static int run_split_iterations(const cs_engine *e, PassCtx *c, SplitRun &R, uint32_t max_len)
{
	hipStream_t s = c->stream;
	unsigned long long *C = c->d_sctr.p, *H = c->h_sctr.p;
	SplitArgs &A = R.A;
	const bool r2text = R.r2text, r3_text = R.r3_text;
	uint64_t *cur = c->d_fqA.p, *nxt = c->d_fqB.p;
	uint64_t *const aux_nxt = r2text ? c->d_aux.p : nullptr; // (one side array is enough: with r2text_kernel the next queue is always d_fqB)
	const int r3t_iter = e->opt.r3_text_iter; // measured in round 2, one pass at a time: 2: 67.8, 3: 66.9, 4: 66.0, 5: 66.8, 6: 68.0 ms; with two passes in flight (round 3): 4: 47.6, 5: 47.0, 6: 47.0 ms per step, one at a time 54.6 / 54.6 / 55.7; repeat50: 4 and 5 the same (110.8 / 111.1 ms per step)
	bool r3t_launched = false;
	uint64_t n_f = (uint64_t)R.nb;
	for (int iter = 0; n_f > 0; ++iter) {
		A.fq_next = nxt; A.aux_next = aux_nxt;
		for (uint64_t c0 = 0; c0 < n_f; ) {
			uint64_t cn = std::min<uint64_t>(R.chunk, n_f - c0);
			A.fq = cur + c0; A.n_f = cn;
			CS_TRY(launch_chunk(e, c, R, A, cur + c0, cn, iter == 0));
			c0 += cn;
		}
		if (r2text) { // re-seeding calls of unique SMEMs pushed by this iteration: answer from the text what the text can answer
			// ... and copy what is left, without the no-op slots, into the queue this iteration has just consumed
			HIP_TRY(hipMemsetAsync(C + SC_DENSE_N, 0, sizeof(unsigned long long), s));
			hipLaunchKernelGGL(r2text_kernel, dim3((unsigned)e->n_cu * 8), dim3(256), 0, s, A, (const uint64_t *)nxt, (const uint64_t *)aux_nxt,
			                   (const unsigned long long *)(C + SC_NEXT_N), C + SC_R2_TEXT, C + SC_R2_INDEX, cur, C + SC_DENSE_N);
			HIP_TRY(hipGetLastError());
		}
		if (r3_text && !r3t_launched && iter + 1 >= r3t_iter) { // (the queue of the next iteration: what r2text_kernel has left, or what was pushed)
			CS_TRY(launch_r3text(e, c, R, r2text ? cur : nxt, r2text ? C + SC_DENSE_N : C + SC_NEXT_N)); r3t_launched = true;
		}
		CS_TRY(fetch_words(c->h_sctr, 0, C, SC_WORDS, s));
		HIP_TRY(hipStreamSynchronize(s));
		if (H[SC_ERR]) return 1; // a queue or the overflow records ran full: the caller redoes the sub-batch with the fused kernel
		// byte model, stream part: this iteration's queue words read (8 B), words pushed (8 B + 8 B side word), and per slot a
		// backward task record cleared, written and scanned by three kernels (16 B each)
		c->stream_bytes += n_f * (8 + 16 * 5) + H[SC_NEXT_N] * (r2text ? 16 + 16 + 8 : 16);
		n_f = r2text ? H[SC_DENSE_N] : H[SC_NEXT_N];
		if (e->opt.verbose > 1) fprintf(stderr, "[cs_engine] iter %d: next queue %llu, sweeps created (last chunk) %llu, text sweeps so far %llu, reseed text %llu / index %llu\n", iter, H[SC_NEXT_N], H[SC_BTASKS], H[SC_TEXT_SWEEPS], H[SC_R2_TEXT], H[SC_R2_INDEX]);
		HIP_TRY(hipMemsetAsync(C + SC_NEXT_N, 0, sizeof(unsigned long long), s));
		if (!r2text) std::swap(cur, nxt); // (r2text_kernel has compacted the next queue into `cur`)
		if (iter > (int)max_len + 8) return fail(CS_EDEVICE, "SMEM task chain did not terminate"); // a read has at most len pivots
	}
	if (r3_text && !r3t_launched) { CS_TRY(launch_r3text(e, c, R, nullptr, nullptr)); r3t_launched = true; }
	return CS_OK;
}

static int run_smem_split_body(const cs_engine *e, PassCtx *c, const cs_params_t *par, const uint64_t *d_off, int64_t nb, uint32_t max_len, bool count_slots, uint64_t *n_ovf_out)
{
	hipStream_t s = c->stream;
	const uint32_t dis = par->sst_mode != 0 ? par->disable : ~0u; // sst_mode 0: the literal algorithm, every shortcut off
	*n_ovf_out = 0;
	if (par->split_width > 16382) return 1; // min_intv does not fit the 14-bit task field: use the fused kernel
	const uint32_t stride = max_len + 1;
	SplitRun R;
	R.nb = nb; R.count = par->count_traffic != 0; R.lean = lean_results(par);
	R.fq_cap = (uint64_t)nb * 8 + 4096; R.ovf_cap = (uint64_t)nb * 4 + 65536;
	R.chunk = std::max<uint64_t>(4096, e->lep_arena_bytes / ((size_t)stride * sizeof(uint4)));
	R.chunk = std::min<uint64_t>(R.chunk, R.fq_cap);
	CS_TRY(c->d_fqA.reserve(R.fq_cap)); CS_TRY(c->d_fqB.reserve(R.fq_cap)); CS_TRY(c->d_fqR.reserve((size_t)nb + 1));
	const bool have_arrays = e->ix.rep != nullptr && par->sst_mode != 0;
	R.r2text = have_arrays && !(dis & CS_DISABLE_R2_TEXT);
	if (R.r2text) CS_TRY(c->d_aux.reserve(R.fq_cap));
	CS_TRY(c->d_bq.reserve(R.chunk)); CS_TRY(c->d_lep.reserve(R.chunk * stride));
	CS_TRY(c->d_ovfrec.reserve(R.ovf_cap));
	unsigned long long *C = c->d_sctr.p, *H = c->h_sctr.p;
	HIP_TRY(hipMemsetAsync(C, 0, SC_WORDS * sizeof(unsigned long long), s));
	HIP_TRY(hipMemsetAsync(c->d_cnt.p, 0, ((size_t)nb + 1) * sizeof(uint32_t), s));
	if (count_slots) HIP_TRY(hipMemsetAsync(c->d_scnt.p, 0, ((size_t)nb + 1) * sizeof(uint32_t), s));

	R.A = split_args(e, c, par, d_off, nb, max_len, dis, R.fq_cap, R.ovf_cap, R.r2text, count_slots);
	const SplitArgs &A = R.A;
	HIP_TRY(hipEventRecord(c->ev[0], s));
	hipLaunchKernelGGL(init_tasks_kernel, dim3(grid_for(nb, 256)), dim3(256), 0, s, A, c->d_fqA.p, c->d_fqR.p);
	// round 3 after rounds 1/2, mostly from the text (r3text_kernel).  Its text paths take "fewer than max_mem_intv occurrences" as
	// "unique" and compare the 255-capped rep[] bytes with min_seed_len + 1, so -y 1 and -k >= 254 stay on the index (fwd_kernel).
	// They also take every mem of rounds 1/2 for an occurrence of the read in the text, and a read none of whose mems covers a k-mer for
	// one that does not hold it.  A call whose pivot is a base the text does not contain starts from an EMPTY interval (bwt_set_intv) and
	// reports it as a mem of size 0 that runs to the read's end (bwt.c:303-320) -- no occurrence, and it hides the matches behind the
	// pivot.  Only an index that lacks one of the four bases has such mems; its round 3 stays on the index.
	bool every_base = true;
	for (int b = 0; b < 4; ++b) every_base = every_base && A.ix.L2[b + 1] > A.ix.L2[b];
	R.r3_text = have_arrays && !(dis & CS_DISABLE_R3_TEXT) && A.max_mem_intv >= 2 && A.min_seed_len + 1 <= 254 && every_base;
	R.r3_async = A.max_mem_intv > 0 && !R.r3_text;
	if (R.r3_async) CS_TRY(launch_r3_index(e, c, R));
	if (R.r3_text) { CS_TRY(c->d_cnt_snap.reserve((size_t)nb + 1)); CS_TRY(c->d_pending.reserve((size_t)nb + 1)); }
	R.fwd0_on = par->sst_mode != 0 && A.ix.text2 && A.jump && A.jump_k >= 8 && !(dis & CS_DISABLE_FWD0);
	{ const int rc = run_split_iterations(e, c, R, max_len); if (rc != CS_OK) return rc; }
	if (R.r3_async || R.r3_text) HIP_TRY(hipStreamWaitEvent(s, c->ev_r3b, 0)); // join the round-3 stream
	HIP_TRY(hipEventRecord(c->ev[1], s));
	CS_TRY(fetch_words(c->h_sctr, 0, C, SC_WORDS, s));
	HIP_TRY(hipStreamSynchronize(s));
	if (H[SC_ERR]) return 1; // round 3 is joined only here: it may have run the overflow records full after the last check in the loop
	CS_TRY(add_event_ms(c->ev[0], c->ev[1], &c->st.seed_kernel_ms));
	c->st.seed_kernel_launches++;
	c->st.bwt_queries += H[SC_QUERIES]; c->st.bwt_calls += H[SC_QUERIES] - H[SC_SST_HITS]; // calls = queries not answered by the on-device SST
	c->st.reseed_text_calls += H[SC_R2_TEXT]; c->st.reseed_index_calls += H[SC_R2_INDEX]; c->st.sweep_text_calls += H[SC_TEXT_SWEEPS]; c->st.r3_text_seeds += H[SC_R3_TEXT_SEEDS];
	*n_ovf_out = H[SC_OVF_MEMS]; // (<= ovf_cap: a record beyond it sets the error flag)
	return CS_OK;
}
// Runs the three rounds for reads [0, nb) of d_off with the split kernels (smem_*.hpp).  On return d_cnt holds the number of
// mems per read, d_out the first `cap` of each, d_ovfrec/*n_ovf the rest; with count_slots, d_scnt the SA slots per read.  Returns 1 when
// a task queue overflowed (the caller then falls back to the fused kernel for this sub-batch).
static int run_smem_split(const cs_engine *e, PassCtx *c, const cs_params_t *par, const uint64_t *d_off, int64_t nb, uint32_t max_len, bool count_slots, uint64_t *n_ovf_out)
{
	const int rc = run_smem_split_body(e, c, par, d_off, nb, max_len, count_slots, n_ovf_out);
	if (rc != CS_OK) { // every early exit: kernels on the side streams may still be appending to buffers the next call reuses
		const std::string keep = g_err;
		(void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->stream2); (void)hipStreamSynchronize(c->stream3); (void)hipStreamSynchronize(c->stream4);
		(void)hipGetLastError();
		g_err = keep;
	}
	return rc;
}

// ------------------------------------------------------------------------------------------------ the hot path
// The reads of one pass.  d_recs: the reads as pack_reads_kernel's records when the host made them (d_bases is then null), else null
struct PassReads {
	int64_t n_reads; const uint8_t *d_bases; const uint64_t *d_off; uint64_t n_bases; const uint4 *d_recs;
	uint32_t max_len;
	bool have_nt4; // the byte-per-base copy in d_seq has been made
};

// checks the offsets and measures the longest read.  MAX_READ_LEN 65535 (comp_seed.h:39; the reference aborts at main.cpp:83-86)
static int measure_reads(const cs_engine *e, PassCtx *c, PassReads &in)
{
	hipStream_t s = c->stream;
	HIP_TRY(hipMemsetAsync(c->d_ctr.p + CTR_OVERFLOW, 0, 3 * sizeof(unsigned long long), s)); // ... CTR_MAX_LEN, CTR_BAD_OFFSETS
	hipLaunchKernelGGL(max_len_kernel, dim3((unsigned)std::min<int64_t>(grid_for(in.n_reads, 256), (int64_t)e->n_cu * 8)), dim3(256), 0, s, in.d_off, in.n_reads, in.n_bases, c->d_ctr.p + CTR_MAX_LEN, c->d_ctr.p + CTR_BAD_OFFSETS);
	CS_TRY(fetch_words(c->h_ctr, 0, c->d_ctr.p, CTR_WORDS, s));
	HIP_TRY(hipStreamSynchronize(s));
	if (c->h_ctr.p[CTR_BAD_OFFSETS]) return fail(CS_EINVAL, "offsets must start at 0, be non-decreasing and end at n_bases");
	in.max_len = (uint32_t)c->h_ctr.p[CTR_MAX_LEN];
	if (c->h_ctr.p[CTR_MAX_LEN] >= 65535) return fail(CS_ERANGE, "read length exceeds the limit 65535 (MAX_READ_LEN)");
	return CS_OK;
}

// the byte-per-base nt4 copy of the reads, made once per pass and only when something reads it
static int make_nt4(const cs_engine *e, PassCtx *c, PassReads &in)
{
	hipStream_t s = c->stream;
	if (in.have_nt4) return CS_OK;
	CS_TRY(c->d_seq.reserve((size_t)in.n_bases + 64));
	if (in.n_bases && in.d_recs) hipLaunchKernelGGL(unpack_reads_kernel, dim3((unsigned)std::min<int64_t>(grid_for(in.n_reads * 8, 256), (int64_t)e->n_cu * 16)), dim3(256), 0, s, in.d_recs, in.d_off, in.n_reads, c->d_seq.p);
	else if (in.n_bases) {
		unsigned g = (unsigned)std::min<uint64_t>((in.n_bases + 255) / 256, (uint64_t)e->n_cu * 16);
		hipLaunchKernelGGL(nt4_kernel, dim3(g), dim3(256), 0, s, in.d_bases, c->d_seq.p, in.n_bases);
	}
	HIP_TRY(hipMemsetAsync(c->d_seq.p + in.n_bases, 4, 64, s));
	in.have_nt4 = true;
	return CS_OK;
}

// The split kernels read the reads as 16-byte records of 32 bases (pack_reads_kernel), made straight from the caller's bytes
// (which stay untouched).  The byte-per-base nt4 copy is what the fused kernel reads: made only when that one runs.
static int prepare_reads(const cs_engine *e, PassCtx *c, PassReads &in)
{
	hipStream_t s = c->stream;
	const int64_t n_reads = in.n_reads; const uint64_t n_bases = in.n_bases; const uint4 *d_recs = in.d_recs;
	if (d_recs && e->smem_mode != 1) return fail(CS_EINVAL, "host-made records need the split kernels");
	const bool raw_ok = e->smem_mode == 1 && (d_recs || ((uintptr_t)in.d_bases & 7u) == 0);
	if (!raw_ok) CS_TRY(make_nt4(e, c, in));
	const uint64_t n_rec = (n_bases >> 5) + (uint64_t)n_reads;
	if (d_recs) { c->seqp_cur = d_recs; c->off_base = in.d_off; }
	else if (e->smem_mode == 1) {
		CS_TRY(c->d_seqp.reserve((size_t)n_rec + 4));
		c->seqp_cur = c->d_seqp.p;
		const dim3 gp((unsigned)std::min<int64_t>(grid_for(n_reads * 8, 256), (int64_t)e->n_cu * 16));
		LAUNCH_EITHER(raw_ok, pack_reads_kernel<true>, pack_reads_kernel<false>, gp, dim3(256), s, raw_ok ? in.d_bases : (const uint8_t *)c->d_seq.p, in.d_off, n_reads, n_bases, c->d_seqp.p);
		c->off_base = in.d_off;
	}
	// byte model, stream part: the bases are read once (twice and written once where the nt4 copy is made), the records written, and
	// read by the forward, backward and round-3 kernels
	c->stream_bytes += (d_recs ? 0 : n_bases * (raw_ok ? 1 : 3)) + (e->smem_mode == 1 ? 16 * n_rec * (d_recs ? 3 : 4) : n_bases * 3);
	return CS_OK;
}

// Offsets of the mems of reads [b0, b0 + nb), continuing the running total: scans d_cnt, fetches the new total and grows d_mems (and
// d_salcnt, where the sort fills it) to it.  total_seeds (the fused sort + SAL path): the same for the seeds in the same round trip --
// d_scnt scanned into d_seed_off, the running seed total continued, d_seeds grown to it.  keep_salcnt false: d_salcnt only has to be large
// enough for the sort to write into (after a sub-batch that did not fill it nothing reads it, and it may be shorter than total_mems).
static int place_mems(PassCtx *c, int64_t b0, int64_t nb, uint64_t total_mems, bool with_salcnt, uint64_t *new_total, uint64_t *total_seeds = nullptr, bool keep_salcnt = true)
{
	hipStream_t s = c->stream;
	CS_TRY(scan_counts(c, c->d_cnt.p, c->d_mem_off.p + b0, (size_t)nb, total_mems));
	if (total_seeds) {
		CS_TRY(scan_counts(c, c->d_scnt.p, c->d_seed_off.p + b0, (size_t)nb, *total_seeds));
		CS_TRY(fetch_pair(c->h_ctr, CTR_FETCHED, c->d_mem_off.p + b0 + nb, c->d_seed_off.p + b0 + nb, s));
	} else CS_TRY(fetch_words(c->h_ctr, CTR_FETCHED, c->d_mem_off.p + b0 + nb, 1, s));
	HIP_TRY(hipStreamSynchronize(s));
	*new_total = c->h_ctr.p[CTR_FETCHED];
	CS_TRY(c->d_mems.reserve((size_t)*new_total + 16, true, s, (size_t)total_mems));
	if (with_salcnt) CS_TRY(c->d_salcnt.reserve((size_t)*new_total + 16, keep_salcnt, s, keep_salcnt ? (size_t)total_mems : 0));
	if (total_seeds) {
		const uint64_t new_seeds = c->h_ctr.p[CTR_FETCHED2];
		CS_TRY(c->d_seeds.reserve((size_t)new_seeds + 16, true, s, (size_t)*total_seeds));
		*total_seeds = new_seeds;
	}
	return CS_OK;
}

// What follows run_smem_split for reads [b0, b0 + nb): the overflow records sorted by read, the offsets, the two sort kernels.
// total_seeds (the fused sort + SAL path, the stage has counted d_scnt): the seeds are written here as well -- sort_expand16_kernel for
// the bulk, sal_expand_heavy_kernel behind sort_compact_wave_kernel for the rest (smem_sort.hpp) -- and run_sal does not run.
static int finish_split_batch(const cs_engine *e, PassCtx *c, const cs_params_t *par, int64_t b0, int64_t nb, uint64_t n_ovf, uint64_t *total_mems, uint64_t *total_seeds, bool salcnt_ok)
{
	hipStream_t s = c->stream;
	const uint32_t cap = e->cap;
	if (n_ovf) { // the few mems beyond a read's first `cap`: sort their records by read id
		c->st.overflow_mems += n_ovf;
		CS_TRY(c->d_okey.reserve(n_ovf)); CS_TRY(c->d_oidx.reserve(n_ovf)); CS_TRY(c->d_okey2.reserve(n_ovf)); CS_TRY(c->d_oidx2.reserve(n_ovf));
		hipLaunchKernelGGL(ovf_keys_kernel, dim3(grid_for((int64_t)n_ovf, 256)), dim3(256), 0, s, c->d_ovfrec.p, n_ovf, c->d_okey.p, c->d_oidx.p);
		CS_TRY(with_rocprim_tmp(c->d_tmp2, [&](void *tmp, size_t &bytes) {
			return rocprim::radix_sort_pairs(tmp, bytes, c->d_okey.p, c->d_okey2.p, c->d_oidx.p, c->d_oidx2.p, (size_t)n_ovf, 0u, 32u, s);
		}));
	}
	uint64_t new_total = 0;
	const uint32_t mo = (uint32_t)par->max_occ;
	const bool lean = lean_results(par); // the kernels below write the final mems[]: their <true> instantiations store x1 = 0
	if (total_seeds) {
		CS_TRY(place_mems(c, b0, nb, *total_mems, false, &new_total, total_seeds));
		unsigned long long *bad = c->d_ctr.p + CTR_SEED_RANGE;
		HIP_TRY(hipMemsetAsync(bad, 0, sizeof(unsigned long long), s));
		HIP_TRY(hipEventRecord(c->ev[0], s));
		LAUNCH_EITHER(lean, sort_expand16_kernel<true>, sort_expand16_kernel<false>, dim3(grid_for(nb * 16, 256)), dim3(256), s, e->ix, c->d_out.p, c->d_cnt.p, cap, c->d_mem_off.p + b0,
		              c->d_seed_off.p + b0, nb, c->d_mems.p, c->d_seeds.p, mo, bad);
		LAUNCH_EITHER(lean, sort_compact_wave_kernel<true>, sort_compact_wave_kernel<false>, dim3(grid_for(nb, 256)), dim3(256), s, c->d_out.p, c->d_cnt.p, cap, c->d_ovfrec.p,
		              c->d_okey2.p, c->d_oidx2.p, n_ovf, c->d_mem_off.p + b0, nb, c->d_mems.p, (uint64_t *)nullptr, mo);
		hipLaunchKernelGGL(sal_expand_heavy_kernel, dim3(grid_for(nb, 256)), dim3(256), 0, s, e->ix, c->d_cnt.p, cap, c->d_mem_off.p + b0, c->d_seed_off.p + b0,
		                   nb, (const OutMem *)c->d_mems.p, c->d_seeds.p, mo, bad);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipEventRecord(c->ev[1], s));
		CS_TRY(fetch_words(c->h_ctr, CTR_SEED_RANGE, bad, 1, s));
		HIP_TRY(hipStreamSynchronize(s));
		if (c->h_ctr.p[CTR_SEED_RANGE]) return fail(CS_EDEVICE, "the SA slots counted while the mems were emitted do not match the sorted mems");
		CS_TRY(add_event_ms(c->ev[0], c->ev[1], &c->st.sal_kernel_ms)); // (here: the sort and the expansion together)
		*total_mems = new_total;
		return CS_OK;
	}
	CS_TRY(place_mems(c, b0, nb, *total_mems, true, &new_total, nullptr, salcnt_ok));
	// (up to 64 mems and none beyond `cap`: 16 lanes per read; all other reads: a wave each)
	LAUNCH_EITHER(lean, sort_compact16_kernel<true>, sort_compact16_kernel<false>, dim3(grid_for(nb * 16, 256)), dim3(256), s, c->d_out.p, c->d_cnt.p, cap,
	              c->d_mem_off.p + b0, nb, c->d_mems.p, c->d_salcnt.p, mo);
	LAUNCH_EITHER(lean, sort_compact_wave_kernel<true>, sort_compact_wave_kernel<false>, dim3(grid_for(nb, 256)), dim3(256), s, c->d_out.p, c->d_cnt.p, cap, c->d_ovfrec.p,
	              c->d_okey2.p, c->d_oidx2.p, n_ovf, c->d_mem_off.p + b0, nb, c->d_mems.p, c->d_salcnt.p, mo);
	HIP_TRY(hipGetLastError());
	*total_mems = new_total;
	return CS_OK;
}

// one launch of the fused kernel and the reads whose mems did not fit `cap`: listed in `list`, counted in h_ctr[CTR_OVERFLOW]
static int fused_launch_and_collect(const cs_engine *e, PassCtx *c, const cs_params_t *par, const uint64_t *d_off, const uint32_t *d_ids, int64_t n_tasks,
                                    OutMem *out, uint32_t *cnt, uint32_t cap, uint32_t max_len, uint32_t *list, double *ms_acc)
{
	hipStream_t s = c->stream;
	CS_TRY(launch_smem(e, c, par, d_off, d_ids, n_tasks, out, cnt, cap, max_len));
	HIP_TRY(hipMemsetAsync(c->d_ctr.p + CTR_OVERFLOW, 0, sizeof(unsigned long long), s));
	hipLaunchKernelGGL(collect_overflow_kernel, dim3(grid_for(n_tasks, 256)), dim3(256), 0, s, cnt, n_tasks, cap, 0u, list, c->d_ctr.p + CTR_OVERFLOW);
	CS_TRY(fetch_words(c->h_ctr, 0, c->d_ctr.p, CTR_WORDS, s));
	HIP_TRY(hipStreamSynchronize(s));
	CS_TRY(add_event_ms(c->ev[0], c->ev[1], ms_acc));
	c->st.bwt_queries += c->h_ctr.p[CTR_QUERIES]; c->st.bwt_calls += c->h_ctr.p[CTR_QUERIES];
	HIP_TRY(hipMemsetAsync(c->d_ctr.p + CTR_QUERIES, 0, sizeof(unsigned long long), s));
	return CS_OK;
}

// Reads [b0, b0 + nb) through the fused kernel (engine option `fused`, or a sub-batch whose task queues overflowed).
static int run_fused_batch(const cs_engine *e, PassCtx *c, const cs_params_t *par, PassReads &in, int64_t b0, int64_t nb, uint64_t *total_mems)
{
	hipStream_t s = c->stream;
	const uint32_t cap = e->cap, max_len = in.max_len;
	const uint64_t *d_off = in.d_off;
	CS_TRY(make_nt4(e, c, in)); // (the fused kernel reads a byte per base)
	HIP_TRY(hipMemsetAsync(c->d_cnt.p + nb, 0, sizeof(uint32_t), s));
	CS_TRY(fused_launch_and_collect(e, c, par, d_off + b0, nullptr, nb, c->d_out.p, c->d_cnt.p, cap, max_len, c->d_ovf.p, &c->st.seed_kernel_ms));
	int64_t n_ovf = (int64_t)c->h_ctr.p[CTR_OVERFLOW];
	uint32_t cap2 = 0;
	if (n_ovf > 0) { // second pass over the few reads with more than `cap` mems, capacity grown until everything fits
		c->st.overflow_mems += (uint64_t)n_ovf;
		cap2 = std::max<uint32_t>(256, cap * 8);
		for (;;) {
			CS_TRY(c->d_out2.reserve((size_t)n_ovf * cap2));
			CS_TRY(c->d_cnt2.reserve((size_t)n_ovf));
			CS_TRY(c->d_tmp2.reserve((size_t)n_ovf * 4 + 16));
			// reuse the overflow counter to see whether any task still does not fit
			CS_TRY(fused_launch_and_collect(e, c, par, d_off + b0, c->d_ovf.p, n_ovf, c->d_out2.p, c->d_cnt2.p, cap2, max_len, (uint32_t *)c->d_tmp2.p, &c->st.overflow_kernel_ms));
			if (c->h_ctr.p[CTR_OVERFLOW] == 0) break;
			if (cap2 >= (1u << 22)) return fail(CS_ERANGE, "a read produced more than 4M mems");
			cap2 *= 8;
		}
		hipLaunchKernelGGL(patch_counts_kernel, dim3(grid_for(n_ovf, 256)), dim3(256), 0, s, c->d_cnt2.p, c->d_ovf.p, n_ovf, 0u, c->d_cnt.p);
	}
	// offsets of this sub-batch, continuing the running total
	uint64_t new_total = 0;
	CS_TRY(place_mems(c, b0, nb, *total_mems, false, &new_total));
	// mem_off already holds absolute offsets, so base_off = 0 and the per-read offset array is shifted by b0
	const bool lean = lean_results(par); // the two kernels that write this path's final mems[]
	LAUNCH_EITHER(lean, sort_compact_kernel<true>, sort_compact_kernel<false>, dim3(grid_for(nb, 128)), dim3(128), s, c->d_out.p, c->d_cnt.p, cap, c->d_mem_off.p + b0,
	              (uint64_t)0, nb, (const uint32_t *)nullptr, c->d_mems.p);
	if (n_ovf > 0)
		LAUNCH_EITHER(lean, sort_compact_list_kernel<true>, sort_compact_list_kernel<false>, dim3(grid_for(n_ovf, 64)), dim3(64), s, c->d_out2.p, c->d_cnt2.p, cap2, c->d_ovf.p,
		              n_ovf, c->d_mem_off.p + b0, c->d_mems.p);
	HIP_TRY(hipGetLastError());
	*total_mems = new_total;
	return CS_OK;
}

// The "distinct SA slots per 512-read batch" statistic (engine option count_sal_merged); the slots are still in rbeg here
static int count_merged_sal(const cs_engine *e, PassCtx *c, int64_t n_reads, uint64_t total_seeds, uint64_t *sal_calls)
{
	hipStream_t s = c->stream;
	unsigned bits = 38;
	while (bits < 64 && ((uint64_t)(n_reads >> 9) >> (bits - 37))) ++bits;
	CS_TRY(c->d_okey64.reserve((size_t)total_seeds)); CS_TRY(c->d_okey64b.reserve((size_t)total_seeds));
	hipLaunchKernelGGL(sal_keys_kernel, dim3((unsigned)std::min<int64_t>(grid_for(n_reads, 256), (int64_t)e->n_cu * 16)), dim3(256), 0, s,
	                   (const OutSeed *)c->d_seeds.p, (const uint64_t *)c->d_seed_off.p, n_reads, c->d_okey64.p);
	rocprim::double_buffer<uint64_t> kb(c->d_okey64.p, c->d_okey64b.p);
	CS_TRY(with_rocprim_tmp(c->d_tmp2, [&](void *tmp, size_t &bytes) { return rocprim::radix_sort_keys(tmp, bytes, kb, (size_t)total_seeds, 0u, bits, s); }));
	HIP_TRY(hipMemsetAsync(c->d_ctr.p + CTR_SAL_DISTINCT, 0, sizeof(unsigned long long), s));
	hipLaunchKernelGGL(count_distinct_kernel, dim3((unsigned)e->n_cu * 8), dim3(256), 0, s, (const uint64_t *)kb.current(), total_seeds, c->d_ctr.p + CTR_SAL_DISTINCT);
	CS_TRY(fetch_words(c->h_ctr, CTR_SAL_DISTINCT, c->d_ctr.p + CTR_SAL_DISTINCT, 1, s));
	HIP_TRY(hipStreamSynchronize(s));
	*sal_calls = c->h_ctr.p[CTR_SAL_DISTINCT];
	return CS_OK;
}

// The SAL stage (comp_seed.cpp:2306-2347): the mems' suffix-array slots expanded into seeds.  salcnt_ok: every mem's slot count
// was written by a sort_compact*_kernel of the split path.
static int run_sal(const cs_engine *e, PassCtx *c, const cs_params_t *par, int64_t n_reads, uint64_t total_mems, bool salcnt_ok, uint64_t *n_seeds_out)
{
	hipStream_t s = c->stream;
	CS_TRY(c->d_seed_off.reserve((size_t)n_reads + 2));
	CS_TRY(c->d_seed_of_mem.reserve((size_t)total_mems + 2));
	// per-mem slot counts are written into the tail of d_seed_of_mem's own storage via a temp
	DevBuf<uint64_t> &som = c->d_seed_of_mem;
	CS_TRY(c->d_tmp.reserve(((size_t)total_mems + 2) * 8 + 1024));
	uint64_t *cnt64 = (uint64_t *)c->d_tmp.p;
	if (salcnt_ok && e->smem_mode == 1) { CS_TRY(c->d_salcnt.reserve((size_t)total_mems + 16, true, s, (size_t)total_mems)); cnt64 = c->d_salcnt.p; } // (counted while sorting)
	HIP_TRY(hipEventRecord(c->ev[0], s));
	HIP_TRY(hipMemsetAsync(cnt64 + total_mems, 0, 8, s));
	if (total_mems && cnt64 != c->d_salcnt.p)
		hipLaunchKernelGGL(sal_count_kernel, dim3(grid_for((int64_t)total_mems, 256)), dim3(256), 0, s, c->d_mems.p, total_mems,
		                   (uint32_t)par->max_occ, cnt64);
	// scan needs its own temp storage: keep the counts where they are and scan with a second buffer
	CS_TRY(with_rocprim_tmp(c->d_tmp2, [&](void *tmp, size_t &bytes) {
		return rocprim::exclusive_scan(tmp, bytes, cnt64, som.p, (uint64_t)0, (size_t)total_mems + 1, rocprim::plus<uint64_t>(), s);
	}));
	CS_TRY(fetch_words(c->h_ctr, CTR_FETCHED, som.p + total_mems, 1, s));
	HIP_TRY(hipStreamSynchronize(s));
	uint64_t total_seeds = c->h_ctr.p[CTR_FETCHED];
	CS_TRY(c->d_seeds.reserve((size_t)total_seeds + 16));
	const bool fused_gather = !e->opt.count_sal_merged && has_full_sa(e->ix); // (the merged-call statistic needs the slots)
	if (total_mems)
		LAUNCH_EITHER(fused_gather, sal_expand_kernel<true>, sal_expand_kernel<false>, dim3(grid_for((int64_t)total_mems, 256)), dim3(256), s, e->ix, c->d_mems.p, total_mems,
		              (uint32_t)par->max_occ, som.p, c->d_seeds.p);
	hipLaunchKernelGGL(seed_off_kernel, dim3(grid_for(n_reads + 1, 256)), dim3(256), 0, s, c->d_mem_off.p, som.p, n_reads, c->d_seed_off.p);
	uint64_t sal_calls = total_seeds;
	if (e->opt.count_sal_merged && total_seeds) CS_TRY(count_merged_sal(e, c, n_reads, total_seeds, &sal_calls)); // (the gather below overwrites the slots)
	if (total_seeds && !fused_gather) {
		if (has_full_sa(e->ix))
			hipLaunchKernelGGL(sal_gather_kernel, dim3(grid_for((int64_t)total_seeds, 256)), dim3(256), 0, s, e->ix, c->d_seeds.p, total_seeds);
		else
			hipLaunchKernelGGL(sal_walk_kernel, dim3(grid_for((int64_t)total_seeds, 256)), dim3(256), 0, s, e->ix, c->d_seeds.p, total_seeds);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c->ev[1], s));
	HIP_TRY(hipStreamSynchronize(s));
	CS_TRY(add_event_ms(c->ev[0], c->ev[1], &c->st.sal_kernel_ms));
	*n_seeds_out = total_seeds;
	c->st.sal_queries += total_seeds; c->st.sal_calls += sal_calls;
	return CS_OK;
}

// d_recs: the reads as pack_reads_kernel's records when the host made them (d_bases is then null), else null
static int seed_device_impl(const cs_engine *e, PassCtx *c, const cs_params_t *par, int64_t n_reads, const uint8_t *d_bases, const uint64_t *d_off,
                            uint64_t n_bases, uint64_t *n_mems_out, uint64_t *n_seeds_out, const uint4 *d_recs)
{
	hipStream_t s = c->stream;
	*n_mems_out = *n_seeds_out = 0;
	if (par->min_seed_len < 1 || par->max_occ < 1 || par->split_width < 0) return fail(CS_EINVAL, "bad seeding parameters");
	CS_TRY(c->d_mem_off.reserve((size_t)n_reads + 2));
	if (n_reads == 0) {
		HIP_TRY(hipMemsetAsync(c->d_mem_off.p, 0, 8, s));
		if (par->want_sal) { CS_TRY(c->d_seed_off.reserve(2)); HIP_TRY(hipMemsetAsync(c->d_seed_off.p, 0, 8, s)); }
		HIP_TRY(hipStreamSynchronize(s));
		return CS_OK;
	}
	HIP_TRY(hipEventRecord(c->ev[2], s));
	PassReads in = {n_reads, d_bases, d_off, n_bases, d_recs, 0, false};
	CS_TRY(measure_reads(e, c, in));
	CS_TRY(prepare_reads(e, c, in));

	const uint32_t cap = e->cap;
	int64_t per_launch = (int64_t)std::max<size_t>(1024, e->max_raw_bytes / ((size_t)cap * sizeof(OutMem)));
	per_launch = std::min<int64_t>(per_launch, n_reads);
	CS_TRY(c->d_out.reserve((size_t)per_launch * cap));
	CS_TRY(c->d_cnt.reserve((size_t)per_launch + 1));
	CS_TRY(c->d_ovf.reserve((size_t)per_launch));
	// Sort and SAL in one pass over the mems (smem_sort.hpp) where the seeds are wanted as the gather from the full suffix array makes
	// them; everything else takes the sort and then run_sal.  (sst_mode 0, the literal algorithm, switches every shortcut off.)
	const uint32_t dis = par->sst_mode != 0 ? par->disable : ~0u;
	bool fused_sal = e->smem_mode == 1 && par->want_sal && !e->opt.count_sal_merged && has_full_sa(e->ix) && !(dis & CS_DISABLE_FUSED_SAL);
	// a read's slots are counted in 32 bits: fewer than 2^22 mems per read, max_occ slots each
	if (fused_sal && (uint64_t)par->max_occ << 22 > (uint64_t)1 << 32) return fail(CS_ERANGE, "max_occ above 1024: a read's seed count may not fit 32 bits (CS_DISABLE_FUSED_SAL lifts the limit)");
	CS_TRY(c->d_mems.reserve((size_t)n_reads * 10 + 1024));
	if (fused_sal) { CS_TRY(c->d_scnt.reserve((size_t)per_launch + 1)); CS_TRY(c->d_seed_off.reserve((size_t)n_reads + 2)); }
	else CS_TRY(c->d_salcnt.reserve((size_t)n_reads * 10 + 1024));
	bool salcnt_ok = true; // every mem's slot count was written by a sort_compact*_kernel of the split path

	uint64_t total_mems = 0, total_seeds = 0;
	for (int64_t b0 = 0; b0 < n_reads; b0 += per_launch) {
		int64_t nb = std::min<int64_t>(per_launch, n_reads - b0);
		if (e->smem_mode == 1) {
			uint64_t n_ovf2 = 0;
			int rc = run_smem_split(e, c, par, d_off + b0, nb, in.max_len, fused_sal, &n_ovf2);
			if (rc < 0) return rc;
			if (rc == 0) { CS_TRY(finish_split_batch(e, c, par, b0, nb, n_ovf2, &total_mems, fused_sal ? &total_seeds : nullptr, salcnt_ok)); continue; }
			// rc == 1: a task queue overflowed -- redo this sub-batch with the fused kernel
		}
		// run_sal then makes all seeds from the sorted mems: those of earlier sub-batches a second time, and sal_kernel_ms holds their
		// sort-and-expand passes as well as run_sal's time (a queue overflow is rare: DESIGN 4.3)
		salcnt_ok = false; fused_sal = false;
		CS_TRY(run_fused_batch(e, c, par, in, b0, nb, &total_mems));
	}
	*n_mems_out = total_mems;

	if (fused_sal) { *n_seeds_out = total_seeds; c->st.sal_queries += total_seeds; c->st.sal_calls += total_seeds; }
	else if (par->want_sal) CS_TRY(run_sal(e, c, par, n_reads, total_mems, salcnt_ok, n_seeds_out));
	HIP_TRY(hipEventRecord(c->ev[3], s));
	HIP_TRY(hipStreamSynchronize(s));
	CS_TRY(add_event_ms(c->ev[2], c->ev[3], &c->st.total_ms));
	c->st.reads += (uint64_t)n_reads; c->st.bases += n_bases; c->st.mems += total_mems; c->st.seeds += *n_seeds_out;
	// byte model, stream part: a mem is written raw, read by the sort and written again (32 B each)
	c->stream_bytes += total_mems * 96;
	return CS_OK;
}

// ------------------------------------------------------------------------------------------------ the pass entry
// One seeding pass on context c of engine e.  The k-mer filter of the window lanes belongs to the engine and is built for one
// min_seed_len at a time: a pass holds filter_rw shared; a pass that wants the filter for another value waits for the others to
// end, rebuilds it alone (once per value) and starts over.  (If it does not fit, the window lanes do without: results never depend
// on it.)
int run_pass(cs_engine *e, PassCtx *c, const cs_params_t *par, int64_t n_reads, const uint8_t *d_bases, const uint64_t *d_off,
             uint64_t n_bases, uint64_t *nm, uint64_t *ns, const uint4 *d_recs)
{
	const int k = par->min_seed_len;
	auto wants_build = [&]() { return e->jump_k && e->ix.text2 && e->opt.kmer_filter && e->smem_mode == 1 && par->sst_mode != 0 && k >= 8 && k <= 24 && e->bloom_k != k && e->bloom_tried_k != k; };
	for (;;) {
		{
			std::shared_lock<std::shared_mutex> sl(e->filter_rw);
			if (!wants_build()) {
				const int rc = seed_device_impl(e, c, par, n_reads, d_bases, d_off, n_bases, nm, ns, d_recs);
				note_ctx_bytes(e, c); // what the pass made its buffers grow to
				return rc;
			}
		}
		std::unique_lock<std::shared_mutex> ul(e->filter_rw);
		if (wants_build()) { e->bloom_tried_k = k; CS_TRY(build_kmer_filter(e, k, c->stream)); }
	}
}

int seed_pass_init(cs_engine *e)
{
	int nb = 0;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fwd_kernel<256, false>, 256, 0) == hipSuccess && nb > 0) e->occ_fwd = std::min(nb, 8);
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, bwd_all_kernel<256, false>, 256, 0) == hipSuccess && nb > 0) e->occ_bwd = std::min(nb, 8);
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, bwd_win_kernel<256, false>, 256, 0) == hipSuccess && nb > 0) e->occ_win = std::min(nb, 8);
	(void)hipGetLastError();
	if (e->jump_k) { // the k-mer filter of the window lanes for the default min_seed_len (mem_opt_init: 19); other values on first use
		cs_params_t dp; cs_params_default(&dp);
		CS_TRY(build_kmer_filter(e, dp.min_seed_len, e->ctx[0]->stream));
		if (e->opt.verbose) { fprintf(stderr, "[cs_engine] k-mer filter: %s\n", e->bloom_k ? "on" : "off"); fflush(stderr); }
	}
	return CS_OK;
}

extern "C" int cs_engine_seed_batch_device(cs_engine_t *e, const cs_params_t *par, int64_t n_reads, const uint8_t *d_bases,
                                           const uint64_t *d_offsets, uint64_t n_bases, cs_result_t *out)
{
	if (!e || !par || !out || n_reads < 0 || (n_reads > 0 && !d_offsets) || (n_bases > 0 && !d_bases))
		return fail(CS_EINVAL, "cs_engine_seed_batch_device: bad argument");
	if (!result_flags_ok(par)) return fail(CS_EINVAL, "unknown bits in result_flags, or reserved is not 0");
	if (n_reads >=(int64_t)0xffffffffll) return fail(CS_ERANGE, "more than 2^32-1 reads in one call");
	if (pipe_busy(e)) return fail(CS_EINVAL, "cs_engine_seed_batch_device: submitted batches are in flight, collect them first");
	HIP_TRY(hipSetDevice(e->device));
	uint64_t nm = 0, ns = 0;
	invalidate_last(e);
	drop_held(e);
	PassCtx *c = e->ctx[0].get();
	CS_TRY(run_pass(e, c, par, n_reads, d_bases, d_offsets, n_bases, &nm, &ns, nullptr));
	c->last.valid = true; c->last.n_reads = n_reads; c->last.n_mems = nm; c->last.n_seeds = ns; c->last.want_sal = par->want_sal; e->last_ctx = c;
	out->n_reads = n_reads; out->n_mems = nm; out->n_seeds = ns;
	out->mem_off = c->d_mem_off.p; out->mems = (const cs_intv_t *)c->d_mems.p;
	out->seed_off = par->want_sal ? c->d_seed_off.p : nullptr;
	out->seeds = par->want_sal ? (const cs_seed_t *)c->d_seeds.p : nullptr;
	return CS_OK;
}
