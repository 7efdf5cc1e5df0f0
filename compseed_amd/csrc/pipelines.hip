// pipelines.hip -- the engine's two pipelines: the host pipeline behind cs_engine_submit / cs_engine_collect_packed and the blocking
// host variants, and the device pipeline behind cs_engine_submit_device / cs_engine_collect_device.
#include "engine.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// ------------------------------------------------------------------------------------------------ the host variants
// cs_engine_seed_batch_packed / cs_engine_seed_batch: the boundary the reference-side patch calls, i.e. the part
// of the path the reference overlaps with kt_pipeline (main.cpp:438, cstl/kthread.c:121: read the next chunk / process / write).
// The batch is cut into sub-batches; an upload thread stages sub-batch i+1 while the calling thread seeds sub-batch i, whose
// results are packed on the device (16-byte mems, 8-byte seeds: include/compseed_amd.h) into one of two buffers and go to pinned
// host memory on a copy stream of their own while sub-batch i+1 is seeded; cs_engine_seed_batch additionally expands finished
// sub-batches to cs_intv_t / cs_seed_t on an expander thread (itself multi-threaded) beside all that.
__global__ void pack_mems16_kernel(const OutMem *m, uint64_t n, uint4 *out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const OutMem v = m[i];
		const uint64_t beg = v.info >> 32, end = v.info & 0xffffffffull;
		const uint64_t w0 = v.x0 | (v.x2 & 0x7fffffffull) << 33, w1 = v.x1 | beg << 33 | end << 48 | (v.x2 >> 31) << 63;
		out[i] = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
	}
}
// a seed travels as its rbeg only, in 40 bits: positions are below 2^37 (checked at engine creation), so the low word and the fifth byte go
// into two planes (coalesced stores, aligned loads for the consumer: cs_packed_seed_rbeg) -- 5 instead of 8 bytes of PCIe traffic per seed
__global__ void pack_rbeg_kernel(const OutSeed *sd, uint64_t n, uint32_t *lo, uint8_t *hi)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) { const uint64_t v = (uint64_t)sd[i].rbeg; lo[i] = (uint32_t)v; hi[i] = (uint8_t)(v >> 32); }
}
__global__ void shift_words_kernel(const uint64_t *in, uint64_t n, uint64_t add, uint64_t *out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = in[i] + add;
}
__global__ void rebase_words_kernel(uint64_t *io, uint64_t n)
{
	const uint64_t base = io[0]; // read by every thread before the grid-wide... single block: see launch
	__syncthreads();
	for (uint64_t i = threadIdx.x; i < n; i += blockDim.x) io[i] -= base;
}

extern "C" int cs_host_alloc(size_t bytes, void **ptr)
{
	if (!ptr) return fail(CS_EINVAL, "null argument");
	*ptr = nullptr;
	HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault));
	return CS_OK;
}
extern "C" int cs_host_free(void *ptr)
{
	if (ptr) HIP_TRY(hipHostFree(ptr));
	return CS_OK;
}

namespace {
struct SubBatch { int64_t r0 = 0, n = 0; uint64_t b0 = 0, nb = 0, mem_base = 0, nm = 0, seed_base = 0, ns = 0; int slot = 0; };

// expand packed sub-batch results into cs_intv_t / cs_seed_t arrays, `threads` workers over contiguous read ranges
void expand_range(const cs_packed_result_t &P, cs_intv_t *mems, cs_seed_t *seeds, int64_t r0, int64_t r1)
{
	for (int64_t r = r0; r < r1; ++r) {
		uint64_t sd = P.seed_off ? P.seed_off[r] : 0;
		for (uint64_t m = P.mem_off[r]; m < P.mem_off[r + 1]; ++m) {
			cs_intv_t v; cs_unpack_mem(&P, m, &v);
			mems[m] = v;
			if (P.seed_off) {
				const int32_t qb = (int32_t)(v.info >> 32), ln = (int32_t)(uint32_t)v.info - qb;
				const uint32_t c = cs_mem_seed_count(&v, P.max_occ);
				for (uint32_t j = 0; j < c; ++j) { cs_seed_t x = {cs_packed_seed_rbeg(&P, sd + j), qb, ln}; seeds[sd + j] = x; }
				sd += c;
			}
		}
	}
}
void expand_parallel(const cs_packed_result_t &P, cs_intv_t *mems, cs_seed_t *seeds, int64_t r0, int64_t r1, int threads)
{
	if (threads < 1) threads = 1;
	if (r1 - r0 < 4096 || threads == 1) { expand_range(P, mems, seeds, r0, r1); return; }
	std::vector<std::thread> th;
	// equal shares of the MEMS, not of the reads: find read boundaries by bisection on mem_off
	const uint64_t m0 = P.mem_off[r0], m1 = P.mem_off[r1];
	int64_t prev = r0;
	for (int t = 1; t <= threads; ++t) {
		int64_t cut = r1;
		if (t < threads) {
			const uint64_t want = m0 + (m1 - m0) * (uint64_t)t / (uint64_t)threads;
			cut = std::lower_bound(P.mem_off + r0, P.mem_off + r1, want) - P.mem_off;
			if (cut < prev) cut = prev;
		}
		if (cut > prev) th.emplace_back(expand_range, std::cref(P), mems, seeds, prev, cut);
		prev = cut;
	}
	for (auto &t : th) t.join();
}
} // namespace

// ---- the engine's host pipeline: three threads behind cs_engine_submit / cs_engine_collect_packed
//   upload thread   stages the parts (sub-batches) of submitted batches, in order, into one of two device input slots
//   seeding thread  seeds a staged part (run_pass), packs its results into one of two device pack slots and queues their
//                   download into the batch's pinned result slot (one of two) on the copy stream
//   expander thread (cs_engine_seed_batch only) expands downloaded parts into cs_intv_t / cs_seed_t arrays
// so that, for a caller that keeps two batches submitted, the upload of batch n+1, the seeding of batch n and the download of
// batch n-1 run at the same time -- what kt_pipeline (main.cpp:438) does for the reference's read / process / write steps.
// All engine state touched by a pass belongs to the seeding thread while a batch is in flight: the blocking entry
// points (device variant, digest, gather, primitives) refuse to run then.
static double pipe_ms() // wall clock of the verbose log lines, from the first one
{
	static const auto t_epoch = std::chrono::steady_clock::now();
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_epoch).count();
}
struct HostJob {
	uint64_t batch = 0; int part = 0, n_parts = 0;
	const uint8_t *bases = nullptr; const uint64_t *offsets = nullptr;
	int64_t r0 = 0, n = 0, n_reads = 0; uint64_t b0 = 0, nb = 0;
	cs_params_t par{}; bool pk16 = false, expand = false, packed = false; // packed: the host makes the records (host_pack.cpp)
	int in_slot = 0;
};
struct XJob { uint64_t batch; int64_t r0, n; uint64_t mem_base, nm, seed_base, ns; hipEvent_t ev; bool last; };
struct BatchState {
	uint64_t id = ~0ull; int64_t n_reads = 0; int parts_total = 0, parts_queued = 0; uint64_t mem_base = 0, seed_base = 0;
	int rc = CS_OK; std::string err; bool pk16 = false, sal = false, expand = false, expanded = false; int max_occ = 0;
	int ctx = 0;                         // pass context that seeded its last part (the whole batch, if it was not cut)
};
struct HostPipe {
	std::thread th_up, th_seed[2], th_x;
	std::mutex mu; std::condition_variable cv;
	bool started = false, quit = false;
	std::deque<HostJob> q_up, q_seed; std::deque<XJob> q_x; bool x_busy = false;
	int in_free[3] = {1, 1, 1};
	uint64_t pack_turn = 0;              // running number of the part whose results are packed and sent home next: parts are seeded by two threads, packed in order
	std::atomic<uint64_t> n_submitted{0}, n_collected{0}; uint64_t parts_seen = 0; // (one submitting and one collecting thread may run at the same time)
	long long handed = -1;               // batch whose pinned result slot the caller currently holds (until its next collect)
	BatchState bs[PIPE_DEPTH];           // batch id % PIPE_DEPTH
};

static void pipe_upload_thread(cs_engine *e)
{
	HostPipe &hp = *e->hp;
	(void)hipSetDevice(e->device);
	for (;;) {
		HostJob j;
		{
			std::unique_lock<std::mutex> lk(hp.mu);
			hp.cv.wait(lk, [&] { return hp.quit || (!hp.q_up.empty() && (hp.in_free[0] || hp.in_free[1] || hp.in_free[2])); });
			if (hp.quit) return;
			j = hp.q_up.front(); hp.q_up.pop_front();
			j.in_slot = hp.in_free[0] ? 0 : hp.in_free[1] ? 1 : 2; hp.in_free[j.in_slot] = 0;
		}
		hipError_t he = hipSuccess;
		const double tu0 = e->opt.verbose > 1 ? pipe_ms() : 0.0;
		if (j.packed) {
			// the reads as records, made here chunk by chunk: the copy of chunk i runs beside the packing of chunk i + 1
			uint4 *st = e->hp_stage[j.in_slot].p;
			const int64_t csz = std::max<int64_t>(262144, (j.n + 7) / 8);
			for (int64_t c0 = 0; c0 < j.n && he == hipSuccess; c0 += csz) {
				const int64_t c1 = std::min<int64_t>(j.n, c0 + csz);
				cs_pack_reads_host_(j.bases, j.offsets, j.r0, j.n, c0, c1, st, e->opt.host_pack_threads, 0);
				const uint64_t f = ((j.offsets[j.r0 + c0] - j.b0) >> 5) + (uint64_t)c0, l = ((j.offsets[j.r0 + c1] - j.b0) >> 5) + (uint64_t)c1;
				he = hipMemcpyAsync(e->hp_in[j.in_slot].p + f * 16, st + f, (size_t)(l - f) * 16, hipMemcpyHostToDevice, e->s_up);
			}
		} else if (j.nb) he = hipMemcpyAsync(e->hp_in[j.in_slot].p, j.bases + j.b0, (size_t)j.nb, hipMemcpyHostToDevice, e->s_up);
		if (he == hipSuccess && j.offsets) he = hipMemcpyAsync(e->hp_inoff[j.in_slot].p, j.offsets + j.r0, ((size_t)j.n + 1) * 8, hipMemcpyHostToDevice, e->s_up);
		if (he == hipSuccess && j.offsets) { hipLaunchKernelGGL(rebase_words_kernel, dim3(1), dim3(1024), 0, e->s_up, e->hp_inoff[j.in_slot].p, (uint64_t)j.n + 1); he = hipGetLastError(); }
		if (he == hipSuccess) he = hipStreamSynchronize(e->s_up);
		if (e->opt.verbose > 1) fprintf(stderr, "[cs_engine] batch %llu part %d/%d: %.1f MB %s in %.1f ms (from %.1f to %.1f ms)\n", (unsigned long long)j.batch, j.part + 1, j.n_parts, (double)(j.packed ? ((j.nb >> 5) + (uint64_t)j.n) * 16 : j.nb) / 1e6, j.packed ? "packed on the host and uploaded" : "uploaded", pipe_ms() - tu0, tu0, pipe_ms());
		std::lock_guard<std::mutex> lk(hp.mu);
		if (he != hipSuccess) { (void)hipGetLastError(); BatchState &b = hp.bs[j.batch % PIPE_DEPTH]; if (b.rc == CS_OK) { b.rc = CS_EDEVICE; b.err = std::string("upload: ") + hipGetErrorString(he); } }
		hp.q_seed.push_back(j);
		hp.cv.notify_all();
	}
}

static void pipe_expand_thread(cs_engine *e)
{
	HostPipe &hp = *e->hp;
	(void)hipSetDevice(e->device);
	for (;;) {
		XJob x;
		{
			std::unique_lock<std::mutex> lk(hp.mu);
			hp.cv.wait(lk, [&] { return hp.quit || !hp.q_x.empty(); });
			if (hp.quit) return;
			x = hp.q_x.front(); hp.q_x.pop_front(); hp.x_busy = true;
		}
		BatchState &b = hp.bs[x.batch % PIPE_DEPTH];
		const int rs = (int)(x.batch % PIPE_DEPTH);
		bool ok = hipEventSynchronize(x.ev) == hipSuccess;
		if (ok) {
			const double scale = x.last ? 1.0 : (double)b.n_reads / (double)(x.r0 + x.n) * ((x.r0 + x.n) * 4 < b.n_reads ? 1.2 : 1.08); // room for the whole batch at the first growth
			ok = !e->x_mems.reserve((size_t)((double)(x.mem_base + x.nm) * scale) + 1, (size_t)x.mem_base) &&
			     (!b.sal || !e->x_seeds.reserve((size_t)((double)(x.seed_base + x.ns) * scale) + 1, (size_t)x.seed_base));
		}
		if (ok) {
			cs_packed_result_t Q; memset(&Q, 0, sizeof Q);
			Q.n_reads = b.n_reads; Q.mem_format = b.pk16 ? CS_MEM_PACKED16 : CS_MEM_FULL32; Q.max_occ = b.max_occ;
			Q.mem_off = e->hp_moff[rs].p; Q.mems = e->hp_mems[rs].p; Q.seed_off = b.sal ? e->hp_soff[rs].p : nullptr; Q.seed_format = CS_SEED_RBEG40; Q.seed_rbeg_lo = b.sal ? e->hp_rlo[rs].p : nullptr; Q.seed_rbeg_hi = b.sal ? e->hp_rhi[rs].p : nullptr;
			expand_parallel(Q, e->x_mems.p, e->x_seeds.p, x.r0, x.r0 + x.n, e->opt.expand_threads);
		}
		std::lock_guard<std::mutex> lk(hp.mu);
		if (!ok && b.rc == CS_OK) { b.rc = CS_ENOMEM; b.err = "expanding the packed results failed"; }
		if (x.last) b.expanded = true;
		hp.x_busy = false;
		hp.cv.notify_all();
	}
}

// One of the (up to) two seeding threads: thread ci runs its passes on pass context ci.  Parts are taken in order; the running number a
// part gets when it is taken (k) fixes the order of the second stage -- packing the results and queueing their download, which needs
// the mem / seed totals of all earlier parts of the batch -- so a part that was seeded faster than its predecessor waits for it there.
static void pipe_seed_thread(cs_engine *e, int ci)
{
	HostPipe &hp = *e->hp;
	(void)hipSetDevice(e->device);
	PassCtx *c = e->ctx[ci].get();
	for (;;) {
		HostJob j;
		uint64_t k;
		{
			std::unique_lock<std::mutex> lk(hp.mu);
			hp.cv.wait(lk, [&] { return hp.quit || !hp.q_seed.empty(); });
			if (hp.quit) return;
			j = hp.q_seed.front(); hp.q_seed.pop_front();
			k = hp.parts_seen++;                       // running part number: pack slot k & 1, part events k % 4
		}
		const int rs = (int)(j.batch % PIPE_DEPTH);
		BatchState &b = hp.bs[rs];
		int rc; { std::lock_guard<std::mutex> lk(hp.mu); rc = b.rc; }
		std::string err;
		auto hipf = [&](hipError_t he, const char *what) { if (he != hipSuccess && rc == CS_OK) { (void)hipGetLastError(); rc = he == hipErrorOutOfMemory ? CS_ENOMEM : CS_EDEVICE; err = std::string(what) + ": " + hipGetErrorString(he); } };
		uint64_t nm = 0, ns = 0;
		const bool sal = j.par.want_sal != 0;
		const size_t msz = j.pk16 ? 16 : 32;
		const double t0 = e->opt.verbose ? pipe_ms() : 0.0;
		if (rc == CS_OK) {
			rc = run_pass(e, c, &j.par, j.n, j.packed ? nullptr : e->hp_in[j.in_slot].p, e->hp_inoff[j.in_slot].p, j.nb, &nm, &ns, j.packed ? reinterpret_cast<const uint4 *>(e->hp_in[j.in_slot].p) : nullptr);
			if (rc != CS_OK) err = g_err;
		}
		if (e->opt.verbose) { // (with the wall clock of the seeding thread: idle gaps between parts show which neighbour it waited for)
			const double t1 = pipe_ms();
			fprintf(stderr, "[cs_engine] batch %llu part %d/%d: %lld reads seeded on context %d in %.1f ms (from %.1f to %.1f ms)\n", (unsigned long long)j.batch, j.part + 1, j.n_parts, (long long)j.n, ci, t1 - t0, t0, t1);
		}
		{ // the input slot is free again (the reads were converted into the context's own buffers); then wait for this part's turn in the second stage
			std::unique_lock<std::mutex> lk(hp.mu);
			hp.in_free[j.in_slot] = 1; hp.cv.notify_all();
			hp.cv.wait(lk, [&] { return hp.quit || hp.pack_turn == k; });
			if (hp.quit) return;
			if (rc == CS_OK) rc = b.rc;               // (an earlier part of the batch failed meanwhile)
		}
		const int ps = (int)(k & 1);
		const uint64_t mem_base = b.mem_base, seed_base = b.seed_base;
		if (rc == CS_OK) {
			// the pack buffers of this slot were last used by the part before the previous one: its download must be over
			if (k >= 2) hipf(hipEventSynchronize(e->hp_ev_dn[(k - 2) % 4]), "waiting for a download");
			// the batch that used this pinned result slot before may still be in the caller's hands: wait until it is given back
			{ std::unique_lock<std::mutex> lk(hp.mu); hp.cv.wait(lk, [&] { return hp.quit || hp.handed < 0 || (uint64_t)hp.handed == j.batch || (uint64_t)hp.handed % PIPE_DEPTH != j.batch % PIPE_DEPTH; }); if (hp.quit) return; }
			// (from here on the result slot is this batch's) offsets: one entry per read + 1
			if (j.part == 0 && (e->hp_moff[rs].reserve((size_t)j.n_reads + 1) != CS_OK || (sal && e->hp_soff[rs].reserve((size_t)j.n_reads + 1) != CS_OK))) { rc = CS_ENOMEM; err = g_err; }
			// pinned room for the whole batch: estimated from its first part, grown (keeping what has arrived) if that was too little
			const size_t need_m = (size_t)(mem_base + nm), need_s = (size_t)(seed_base + ns);
			if (need_m * msz > e->hp_mems[rs].cap || (sal && need_s > e->hp_rlo[rs].cap)) {
				hipf(hipStreamSynchronize(e->s_down), "draining downloads before growing the result buffers");
				{ std::unique_lock<std::mutex> lk(hp.mu); hp.cv.wait(lk, [&] { return hp.quit || (hp.q_x.empty() && !hp.x_busy); }); if (hp.quit) return; } // the expander reads these buffers
				const double scale = (double)j.n_reads / (double)(j.r0 + j.n) * ((j.r0 + j.n) * 4 < j.n_reads ? 1.2 : 1.08); // (a small first part predicts the batch less well)
				if (rc == CS_OK && e->hp_mems[rs].reserve((size_t)((double)need_m * scale) * msz + 4096, true, (size_t)mem_base * msz) != CS_OK) { rc = CS_ENOMEM; err = g_err; }
				if (rc == CS_OK && sal && (e->hp_rlo[rs].reserve((size_t)((double)need_s * scale) + 512, true, (size_t)seed_base) != CS_OK ||
				                            e->hp_rhi[rs].reserve((size_t)((double)need_s * scale) + 512, true, (size_t)seed_base) != CS_OK)) { rc = CS_ENOMEM; err = g_err; }
			}
		}
		if (rc == CS_OK && (e->hp_pk_mems[ps].reserve((size_t)nm * msz + 64) != CS_OK || (sal && (e->hp_pk_rlo[ps].reserve((size_t)ns + 8) != CS_OK || e->hp_pk_rhi[ps].reserve((size_t)ns + 8) != CS_OK)))) { rc = CS_ENOMEM; err = g_err; }
		if (rc == CS_OK) {
			hipStream_t s = c->stream;                 // (the context's own stream: its next pass starts behind these kernels)
			const unsigned g = (unsigned)e->n_cu * 8;
			hipLaunchKernelGGL(shift_words_kernel, dim3(g), dim3(256), 0, s, (const uint64_t *)c->d_mem_off.p, (uint64_t)j.n + 1, mem_base, e->hp_pk_moff[ps].p);
			if (nm) {
				if (j.pk16) hipLaunchKernelGGL(pack_mems16_kernel, dim3(g), dim3(256), 0, s, (const OutMem *)c->d_mems.p, nm, (uint4 *)e->hp_pk_mems[ps].p);
				else hipf(hipMemcpyAsync(e->hp_pk_mems[ps].p, c->d_mems.p, (size_t)nm * 32, hipMemcpyDeviceToDevice, s), "copying mems");
			}
			if (sal) {
				hipLaunchKernelGGL(shift_words_kernel, dim3(g), dim3(256), 0, s, (const uint64_t *)c->d_seed_off.p, (uint64_t)j.n + 1, seed_base, e->hp_pk_soff[ps].p);
				if (ns) hipLaunchKernelGGL(pack_rbeg_kernel, dim3(g), dim3(256), 0, s, (const OutSeed *)c->d_seeds.p, ns, e->hp_pk_rlo[ps].p, e->hp_pk_rhi[ps].p);
			}
			hipf(hipGetLastError(), "pack kernels");
			hipf(hipEventRecord(e->hp_ev_pk[ps], s), "event");
			hipf(hipStreamWaitEvent(e->s_down, e->hp_ev_pk[ps], 0), "event");
			hipf(hipMemcpyAsync(e->hp_moff[rs].p + j.r0, e->hp_pk_moff[ps].p, ((size_t)j.n + 1) * 8, hipMemcpyDeviceToHost, e->s_down), "download");
			if (nm) hipf(hipMemcpyAsync(e->hp_mems[rs].p + (size_t)mem_base * msz, e->hp_pk_mems[ps].p, (size_t)nm * msz, hipMemcpyDeviceToHost, e->s_down), "download");
			if (sal) {
				hipf(hipMemcpyAsync(e->hp_soff[rs].p + j.r0, e->hp_pk_soff[ps].p, ((size_t)j.n + 1) * 8, hipMemcpyDeviceToHost, e->s_down), "download");
				if (ns) hipf(hipMemcpyAsync(e->hp_rlo[rs].p + seed_base, e->hp_pk_rlo[ps].p, (size_t)ns * 4, hipMemcpyDeviceToHost, e->s_down), "download");
				if (ns) hipf(hipMemcpyAsync(e->hp_rhi[rs].p + seed_base, e->hp_pk_rhi[ps].p, (size_t)ns, hipMemcpyDeviceToHost, e->s_down), "download");
			}
			hipf(hipEventRecord(e->hp_ev_dn[k % 4], e->s_down), "event");
			if (j.part + 1 == j.n_parts) hipf(hipEventRecord(e->hp_ev_done[rs], e->s_down), "event");
		} else {
			// a failed part still owns hp_ev_dn[k % 4] in the eyes of part k + 2: leave a recorded event behind
			(void)hipEventRecord(e->hp_ev_dn[k % 4], e->s_down);
		}
		std::lock_guard<std::mutex> lk(hp.mu);
		if (rc != CS_OK && b.rc == CS_OK) { b.rc = rc; b.err = err; }
		if (rc == CS_OK) {
			b.mem_base += nm; b.seed_base += ns; b.ctx = ci;
			if (j.expand) { XJob x = {j.batch, j.r0, j.n, mem_base, nm, seed_base, ns, e->hp_ev_dn[k % 4], j.part + 1 == j.n_parts}; hp.q_x.push_back(x); }
		}
		b.parts_queued++;
		hp.pack_turn = k + 1;
		hp.cv.notify_all();
	}
}

void pipe_stop(cs_engine *e)
{
	if (!e->hp) return;
	HostPipe &hp = *e->hp;
	{ std::lock_guard<std::mutex> lk(hp.mu); hp.quit = true; hp.cv.notify_all(); }
	if (hp.th_up.joinable()) hp.th_up.join();
	for (auto &t : hp.th_seed) if (t.joinable()) t.join();
	if (hp.th_x.joinable()) hp.th_x.join();
	delete e->hp; e->hp = nullptr;
}
static bool host_pipe_busy(const cs_engine *e) { return e->hp && e->hp->n_submitted.load() != e->hp->n_collected.load(); }
static bool dev_pipe_busy(const cs_engine *e);
bool pipe_busy(const cs_engine *e) { return host_pipe_busy(e) || dev_pipe_busy(e); }


static int pipe_submit(cs_engine *e, const cs_params_t *par, int64_t n_reads, const uint8_t *bases, const uint64_t *offsets, bool expand)
{
	if (!e || !par || n_reads < 0 || (n_reads > 0 && !offsets)) return fail(CS_EINVAL, "cs_engine_submit: bad argument");
	if (n_reads >= (int64_t)0xffffffffll) return fail(CS_ERANGE, "more than 2^32-1 reads in one call");
	if (par->min_seed_len < 1 || par->max_occ < 1 || par->split_width < 0) return fail(CS_EINVAL, "bad seeding parameters");
	HIP_TRY(hipSetDevice(e->device));
	if (dev_pipe_busy(e)) return fail(CS_EINVAL, "cs_engine_submit: device batches are in flight (cs_engine_submit_device), collect them first");
	drop_held(e);
	if (!e->hp) e->hp = new HostPipe();
	HostPipe &hp = *e->hp;
	if (hp.n_submitted.load() - hp.n_collected.load() >= (uint64_t)PIPE_DEPTH) return fail(CS_EINVAL, "cs_engine_submit: four batches are in flight already, collect one first");
	uint64_t n_bases = 0, max_len = 0;
	if (n_reads > 0) {
		if (offsets[0] != 0) return fail(CS_EINVAL, "offsets[0] must be 0");
		n_bases = offsets[n_reads];
		if (n_bases > 0 && !bases) return fail(CS_EINVAL, "bases is null");
		// (10 M offsets are 6 ms on one thread, in front of everything else a blocking call does: four threads)
		const int vt = n_reads >= (1 << 20) ? 4 : 1;
		uint64_t vmax[4] = {0, 0, 0, 0}; bool vbad[4] = {false, false, false, false};
		auto vrange = [&](int t) {
			uint64_t m = 0; bool bad = false;
			for (int64_t r = n_reads * t / vt, r1 = n_reads * (t + 1) / vt; r < r1; ++r) { bad |= offsets[r + 1] < offsets[r]; m = std::max(m, offsets[r + 1] - offsets[r]); }
			vmax[t] = m; vbad[t] = bad;
		};
		if (vt == 1) vrange(0);
		else { std::thread th[3]; for (int t = 1; t < vt; ++t) th[t - 1] = std::thread(vrange, t); vrange(0); for (auto &t : th) t.join(); }
		for (int t = 0; t < vt; ++t) { if (vbad[t]) return fail(CS_EINVAL, "offsets must start at 0, be non-decreasing and end at n_bases"); max_len = std::max(max_len, vmax[t]); }
		if (max_len >= 65535) return fail(CS_ERANGE, "read length exceeds the limit 65535 (MAX_READ_LEN)");
	}
	const uint64_t id = hp.n_submitted.load();
	const int rs = (int)(id % PIPE_DEPTH);
	// parts: contiguous read ranges of about pipeline_reads reads (one, if the batch is not much larger than that)
	std::vector<HostJob> parts;
	const int64_t per = e->opt.pipeline_reads > 0 ? e->opt.pipeline_reads : std::max<int64_t>(n_reads, 1);
	// Parts exist to overlap upload, seeding and download INSIDE one batch, and each part pays the fixed cost of a pass (two passes over
	// 5 M reads take ~8 ms longer than one over 10 M).  When other batches are in flight the overlap comes from them -- upload of n+1 and
	// download of n-1 beside the seeding of n -- so a batch submitted behind another one is seeded whole.  This needs THREE batches in
	// flight to pay: with two, collect(n) returns when download(n) ends, only then can batch n+2 be submitted and uploaded, and download +
	// upload (79 ms) is longer than the seeding of batch n+1 (55 ms): measured 92 ms per batch whole against 65 ms in parts.
	const bool streaming = hp.n_submitted.load() - hp.n_collected.load() >= 2 && !expand;
	// part boundaries.  A batch that has the engine to itself (a blocking call, the first batch of a stream) cannot hide the upload of its
	// first part or the download of its last one behind anything, so those two are made small (0.2 of the nominal part) and the rest is
	// cut into parts of about 0.8: 10 M reads at 5 M nominal = 1 / 4 / 4 / 1 M (measured against 1.5 / 3.5 / 3.5 / 1.5: section 8 of DESIGN.md).
	std::vector<int64_t> cut(1, 0);
	const int64_t even = std::max<int64_t>(1, (n_reads + per / 2) / per);
	if (streaming || even < 2) cut.push_back(n_reads);
	else {
		const int64_t h = std::max<int64_t>(1, std::min<int64_t>(n_reads / 4, per * 2 / 10)), rest = n_reads - 2 * h;
		const int64_t km = std::max<int64_t>(1, (rest + per * 8 / 20) / std::max<int64_t>(1, per * 8 / 10));
		cut.push_back(h);
		for (int64_t i = 1; i <= km; ++i) cut.push_back(h + rest * i / km);
		cut.push_back(n_reads);
	}
	const int64_t kparts = (int64_t)cut.size() - 1;
	size_t in_cap = 0, off_cap = 0, stage_cap = 0;
	const bool host_pack = e->opt.host_pack_threads > 0 && e->smem_mode == 1;
	for (int64_t i = 0; i < kparts; ++i) {
		HostJob j; j.batch = id; j.part = (int)i; j.n_parts = (int)kparts; j.bases = bases; j.offsets = offsets; j.n_reads = n_reads;
		j.r0 = cut[(size_t)i]; j.n = cut[(size_t)i + 1] - j.r0;
		j.b0 = n_reads ? offsets[j.r0] : 0; j.nb = n_reads ? offsets[j.r0 + j.n] - j.b0 : 0;
		j.par = *par; j.pk16 = (e->ix.seq_len >> 33) == 0 && max_len < (1u << 15); j.expand = expand;
		j.packed = host_pack;
		const size_t n_rec = (size_t)(j.nb >> 5) + (size_t)j.n;
		in_cap = std::max<size_t>(in_cap, host_pack ? (n_rec + 4) * 16 : j.nb); off_cap = std::max<size_t>(off_cap, (size_t)j.n + 1);
		if (host_pack) stage_cap = std::max<size_t>(stage_cap, n_rec + 4);
		parts.push_back(j);
	}
	{ // buffers the threads will use: sized here, while no part of this batch is in flight (earlier batches never need more than they have)
		std::unique_lock<std::mutex> lk(hp.mu);
		if (in_cap + 64 > e->hp_in[0].cap || stage_cap > e->hp_stage[0].cap || off_cap > e->hp_inoff[0].cap || off_cap > e->hp_pk_moff[0].cap || (par->want_sal && off_cap > e->hp_pk_soff[0].cap)) {
			// a reallocation frees buffers the other batch may still be using: not only while its parts are queued or being seeded
			// (the input slots are given back right after run_pass), but until the seeding thread has queued the pack kernels
			// and downloads of its LAST part (parts_queued == parts_total) and those have drained (s_down below)
			auto others_queued = [&] { for (int o = 1; o < PIPE_DEPTH; ++o) { const BatchState &ob = hp.bs[(rs + o) % PIPE_DEPTH]; if (ob.parts_queued != ob.parts_total) return false; } return true; };
			hp.cv.wait(lk, [&] { return hp.quit || (hp.q_up.empty() && hp.q_seed.empty() && hp.in_free[0] && hp.in_free[1] && hp.in_free[2] && others_queued()); });
			lk.unlock();
			for (auto &c : e->ctx) if (c) HIP_TRY(hipStreamSynchronize(c->stream));
			HIP_TRY(hipStreamSynchronize(e->s_down));
			for (int k = 0; k < 3; ++k) { CS_TRY(e->hp_in[k].reserve(in_cap + 64)); CS_TRY(e->hp_stage[k].reserve(stage_cap)); CS_TRY(e->hp_inoff[k].reserve(off_cap)); }
			for (int k = 0; k < 2; ++k) {
				CS_TRY(e->hp_pk_moff[k].reserve(off_cap));
				if (par->want_sal) CS_TRY(e->hp_pk_soff[k].reserve(off_cap));
			}
			lk.lock();
		}
		BatchState &b = hp.bs[rs];
		b = BatchState();
		b.id = id; b.n_reads = n_reads; b.parts_total = (int)kparts; b.pk16 = parts[0].pk16; b.sal = par->want_sal != 0; b.expand = expand; b.max_occ = par->max_occ;
		for (auto &j : parts) hp.q_up.push_back(j);
		if (e->opt.verbose > 1) fprintf(stderr, "[cs_engine] batch %llu submitted at %.1f ms in %d part(s)\n", (unsigned long long)id, pipe_ms(), (int)kparts);
		hp.n_submitted++;
		invalidate_last(e);
		if (!hp.started) {
			hp.started = true;
			hp.th_up = std::thread(pipe_upload_thread, e); hp.th_x = std::thread(pipe_expand_thread, e);
			// One seeding thread / pass context here.  The code takes two (parts are seeded by whichever thread is free and packed in order), and
			// that was measured at hg19 scale: a stream of batches 59-65 instead of 57 ms per batch, a blocking call 107 instead of 105 ms --
			// two passes that run side by side end together, their downloads queue up behind each other (the stream is within 20 % of what the
			// 246 bytes per read of results allow over PCIe), and the next uploads wait for a free slot.  The device-resident form
			// (cs_engine_submit_device) is where the second context pays: 48 instead of 55 ms per 10 M reads.
			const int n_host_ctx = 1;
			for (int ci = 0; ci < n_host_ctx && ci < n_pass_ctx(e); ++ci) hp.th_seed[ci] = std::thread(pipe_seed_thread, e, ci);
		}
		hp.cv.notify_all();
	}
	return CS_OK;
}

static int pipe_collect(cs_engine *e, cs_packed_result_t *out)
{
	if (!e || !out) return fail(CS_EINVAL, "cs_engine_collect: null argument");
	if (!e->hp || e->hp->n_submitted.load() == e->hp->n_collected.load()) return fail(CS_EINVAL, "cs_engine_collect: nothing has been submitted");
	HIP_TRY(hipSetDevice(e->device));
	HostPipe &hp = *e->hp;
	const uint64_t id = hp.n_collected.load();
	const int rs = (int)(id % PIPE_DEPTH);
	BatchState &b = hp.bs[rs];
	{
		std::unique_lock<std::mutex> lk(hp.mu);
		hp.handed = -1;                      // the result handed out by the previous collect is given back: its slot may be overwritten
		hp.cv.notify_all();
		hp.cv.wait(lk, [&] { return b.parts_queued == b.parts_total; });
	}
	int rc = b.rc; std::string err = b.err;
	const double tc0 = e->opt.verbose > 1 ? pipe_ms() : 0.0;
	if (rc == CS_OK && hipEventSynchronize(e->hp_ev_done[rs]) != hipSuccess) { rc = CS_EDEVICE; err = "waiting for the download"; (void)hipGetLastError(); }
	if (e->opt.verbose > 1) fprintf(stderr, "[cs_engine] batch %llu collected at %.1f ms: waited %.1f ms for its download after its last part was queued\n", (unsigned long long)id, pipe_ms(), pipe_ms() - tc0);
	if (rc == CS_OK && b.expand) {
		std::unique_lock<std::mutex> lk(hp.mu);
		hp.cv.wait(lk, [&] { return b.expanded || b.rc != CS_OK; });
		rc = b.rc; err = b.err;
	}
	memset(out, 0, sizeof *out);
	{
		std::lock_guard<std::mutex> lk(hp.mu);
		hp.n_collected++;
		if (rc == CS_OK) hp.handed = (long long)id;
	}
	if (rc != CS_OK) return fail(rc, err);
	out->n_reads = b.n_reads; out->n_mems = b.mem_base; out->n_seeds = b.seed_base; out->max_occ = b.max_occ;
	out->mem_format = b.pk16 ? CS_MEM_PACKED16 : CS_MEM_FULL32;
	out->mem_off = e->hp_moff[rs].p; out->mems = e->hp_mems[rs].p;
	out->seed_off = b.sal ? e->hp_soff[rs].p : nullptr; out->seed_format = CS_SEED_RBEG40;
	out->seed_rbeg_lo = b.sal ? e->hp_rlo[rs].p : nullptr; out->seed_rbeg_hi = b.sal ? e->hp_rhi[rs].p : nullptr;
	{ // cs_engine_result_digest / gather_reads work on the device-side result, which is the whole batch only if it was not cut
		std::lock_guard<std::mutex> lk(hp.mu); // (a submit on another thread invalidates it under the same lock)
		PassCtx *c = e->ctx[b.ctx].get();
		invalidate_last(e);
		c->last.valid = b.parts_total == 1 && !pipe_busy(e); c->last.n_reads = b.n_reads; c->last.n_mems = b.mem_base; c->last.n_seeds = b.seed_base; c->last.want_sal = b.sal;
		e->last_ctx = c;
	}
	return CS_OK;
}

// ---- device batches, two in flight: cs_engine_submit_device / cs_engine_collect_device.  Batch n runs on pass context n & 1, on a thread
// of its own, so the thin tail of one pass overlaps the dense start of the next; results come back in submission order as device
// pointers into the engine's spare result set (cs_engine::held), which a collect exchanges with its context's result buffers.
struct DevPipe {
	std::thread th[2]; std::mutex mu; std::condition_variable cv; bool quit = false;
	int n_ctx = 1;
	int state[2] = {0, 0};                // 0 idle, 1 queued, 2 running, 3 done
	struct Job { cs_params_t par; int64_t n; const uint8_t *bases; const uint64_t *off; uint64_t nb; } job[2];
	int rc[2] = {0, 0}; std::string err[2]; uint64_t nm[2] = {0, 0}, ns[2] = {0, 0};
	std::atomic<uint64_t> n_sub{0}, n_col{0};
};
static bool dev_pipe_busy(const cs_engine *e) { return e->dp && e->dp->n_sub.load() != e->dp->n_col.load(); }
static void dev_pipe_thread(cs_engine *e, int ci)
{
	DevPipe &dp = *e->dp;
	(void)hipSetDevice(e->device);
	PassCtx *c = e->ctx[ci].get();
	for (;;) {
		DevPipe::Job j;
		{
			std::unique_lock<std::mutex> lk(dp.mu);
			dp.cv.wait(lk, [&] { return dp.quit || dp.state[ci] == 1; });
			if (dp.quit) return;
			dp.state[ci] = 2; j = dp.job[ci];
		}
		uint64_t nm = 0, ns = 0;
		const int rc = run_pass(e, c, &j.par, j.n, j.bases, j.off, j.nb, &nm, &ns, nullptr);
		std::lock_guard<std::mutex> lk(dp.mu);
		dp.rc[ci] = rc; dp.err[ci] = rc != CS_OK ? g_err : std::string(); dp.nm[ci] = nm; dp.ns[ci] = ns;
		dp.state[ci] = 3;
		dp.cv.notify_all();
	}
}
void dev_pipe_stop(cs_engine *e)
{
	if (!e->dp) return;
	DevPipe &dp = *e->dp;
	{ std::lock_guard<std::mutex> lk(dp.mu); dp.quit = true; dp.cv.notify_all(); }
	for (auto &t : dp.th) if (t.joinable()) t.join();
	delete e->dp; e->dp = nullptr;
}
extern "C" int cs_engine_submit_device(cs_engine_t *e, const cs_params_t *par, int64_t n_reads, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_bases)
{
	if (!e || !par || n_reads < 0 || (n_reads > 0 && !d_offsets) || (n_bases > 0 && !d_bases)) return fail(CS_EINVAL, "cs_engine_submit_device: bad argument");
	if (n_reads >= (int64_t)0xffffffffll) return fail(CS_ERANGE, "more than 2^32-1 reads in one call");
	if (host_pipe_busy(e)) return fail(CS_EINVAL, "cs_engine_submit_device: host batches are in flight (cs_engine_submit), collect them first");
	HIP_TRY(hipSetDevice(e->device));
	if (!e->dp) {
		if (e->opt.passes_in_flight >= 2 && !e->ctx[1]) CS_TRY(add_pass_ctx(e));
		e->dp = new DevPipe();
		e->dp->n_ctx = n_pass_ctx(e);
		for (int ci = 0; ci < e->dp->n_ctx; ++ci) e->dp->th[ci] = std::thread(dev_pipe_thread, e, ci);
	}
	DevPipe &dp = *e->dp;
	if (dp.n_sub.load() - dp.n_col.load() >= (uint64_t)dp.n_ctx) return fail(CS_EINVAL, dp.n_ctx == 2 ? "cs_engine_submit_device: two batches are in flight already, collect one first" : "cs_engine_submit_device: a batch is in flight already (passes_in_flight = 1), collect it first");
	const int ci = (int)(dp.n_sub.load() % (uint64_t)dp.n_ctx);
	std::lock_guard<std::mutex> lk(dp.mu);
	invalidate_last(e);
	dp.job[ci] = {*par, n_reads, d_bases, d_offsets, n_bases};
	dp.state[ci] = 1;
	dp.n_sub++;
	dp.cv.notify_all();
	return CS_OK;
}
extern "C" int cs_engine_collect_device(cs_engine_t *e, cs_result_t *out)
{
	if (!e || !out) return fail(CS_EINVAL, "cs_engine_collect_device: null argument");
	if (!e->dp || e->dp->n_sub.load() == e->dp->n_col.load()) return fail(CS_EINVAL, "cs_engine_collect_device: nothing has been submitted");
	DevPipe &dp = *e->dp;
	const int ci = (int)(dp.n_col.load() % (uint64_t)dp.n_ctx);
	PassCtx *c = e->ctx[ci].get();
	int rc; std::string err; uint64_t nm, ns; bool sal; int64_t n;
	{
		std::unique_lock<std::mutex> lk(dp.mu);
		dp.cv.wait(lk, [&] { return dp.state[ci] == 3; });
		rc = dp.rc[ci]; err = dp.err[ci]; nm = dp.nm[ci]; ns = dp.ns[ci]; sal = dp.job[ci].par.want_sal != 0; n = dp.job[ci].n;
		if (rc == CS_OK) {
			// The result leaves its context: the context's four result buffers are exchanged with the engine's one spare set (e->held), and
			// the caller gets the spare set's pointers.  No pass runs on this context (its state is 3, the submit that could start one
			// waits for n_col below, under this lock), so nothing reads or writes either set meanwhile.  One spare set is enough for "valid
			// until the SECOND submit after its collect": r_n stays in `held` until collect(n+1) -- a failed batch hands nothing out and
			// swaps nothing, so then until the next collect that succeeds -- which moves r_n's buffers into context (n+1) % n_ctx.
			// That context has just been collected, so the next pass on it is batch n+1+n_ctx.  With two contexts at most n+1 had been
			// submitted when n was collected (two in flight), so n+3 is at the earliest the second submit after collect(n); with one
			// context, submit(n+1) came after collect(n) and n+2 is the second.  Drained orders (col n, col n+1, sub, sub) are the same
			// count: the first of the two submits runs on the other context, or (one context) precedes collect(n+1).  A batch of
			// want_sal = 0 leaves the seed buffers as it found them; they travel with the set all the same, only their capacity matters.
			invalidate_last(e);
			std::swap(c->d_mem_off, e->held.mem_off); std::swap(c->d_mems, e->held.mems);
			std::swap(c->d_seed_off, e->held.seed_off); std::swap(c->d_seeds, e->held.seeds);
			note_ctx_bytes(e, c);
			e->held_bytes.store(e->held.device_bytes(), std::memory_order_relaxed);
			// cs_engine_result_digest / cs_engine_gather_reads follow the arrays (a submit on another thread invalidates under the same lock)
			c->last.n_reads = n; c->last.n_mems = nm; c->last.n_seeds = ns; c->last.want_sal = sal;
			c->last.valid = dp.n_sub.load() == dp.n_col.load() + 1; // drained by this collect
			e->last_ctx = c; e->last_in_held = true;
		}
		dp.state[ci] = 0;
		dp.n_col++;
	}
	memset(out, 0, sizeof *out);
	if (rc != CS_OK) return fail(rc, err);
	out->n_reads = n; out->n_mems = nm; out->n_seeds = ns;
	out->mem_off = e->held.mem_off.p; out->mems = (const cs_intv_t *)e->held.mems.p;
	out->seed_off = sal ? e->held.seed_off.p : nullptr; out->seeds = sal ? (const cs_seed_t *)e->held.seeds.p : nullptr;
	return CS_OK;
}

extern "C" int cs_engine_submit(cs_engine_t *e, const cs_params_t *par, int64_t n_reads, const uint8_t *bases, const uint64_t *offsets)
{
	return pipe_submit(e, par, n_reads, bases, offsets, false);
}
extern "C" int cs_engine_collect_packed(cs_engine_t *e, cs_packed_result_t *out) { return pipe_collect(e, out); }

extern "C" int cs_engine_seed_batch_packed(cs_engine_t *e, const cs_params_t *par, int64_t n_reads, const uint8_t *bases,
                                           const uint64_t *offsets, cs_packed_result_t *out)
{
	if (!e || !par || !out) return fail(CS_EINVAL, "cs_engine_seed_batch_packed: bad argument");
	if (pipe_busy(e)) return fail(CS_EINVAL, "cs_engine_seed_batch_packed: submitted batches are in flight, collect them first");
	CS_TRY(pipe_submit(e, par, n_reads, bases, offsets, false));
	return pipe_collect(e, out);
}

extern "C" int cs_engine_seed_batch(cs_engine_t *e, const cs_params_t *par, int64_t n_reads, const uint8_t *bases,
                                    const uint64_t *offsets, cs_result_t *out)
{
	if (!e || !par || !out) return fail(CS_EINVAL, "cs_engine_seed_batch: bad argument");
	if (pipe_busy(e)) return fail(CS_EINVAL, "cs_engine_seed_batch: submitted batches are in flight, collect them first");
	CS_TRY(pipe_submit(e, par, n_reads, bases, offsets, true));
	cs_packed_result_t P;
	CS_TRY(pipe_collect(e, &P));
	out->n_reads = n_reads; out->n_mems = P.n_mems; out->n_seeds = P.n_seeds;
	out->mem_off = P.mem_off; out->mems = e->x_mems.p;
	out->seed_off = P.seed_off; out->seeds = par->want_sal ? e->x_seeds.p : nullptr;
	return CS_OK;
}
