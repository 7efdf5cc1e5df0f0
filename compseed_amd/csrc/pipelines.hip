// pipelines.hip -- the engine's two pipelines: the host pipeline behind cs_engine_submit / cs_engine_collect_packed and the blocking
// host variants, and the device pipeline behind cs_engine_submit_device / cs_engine_collect_device.
#include "engine.hpp"
#include "host_parts.hpp"

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
// results are packed on the device (16-byte mems, 8-byte under CS_RESULT_LEAN, 5-byte seeds: include/compseed_amd.h) into one of two buffers and go to pinned
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
// CS_RESULT_LEAN: x2 and the two query positions in one word (cs_mem8_t); 32 bytes read, 8 written per lane, both coalesced
__global__ void pack_mems8_kernel(const OutMem *m, uint64_t n, uint64_t *out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const OutMem v = m[i];
		const uint64_t beg = v.info >> 32, end = v.info & 0xffffffffull;
		out[i] = v.x2 | beg << 34 | end << 49;
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
//   upload thread   stages the parts (sub-batches) of submitted batches, in order, into one of three device input slots
//   seeding thread  seeds a staged part (run_pass), packs its results into one of two device pack slots and queues their
//                   download into the batch's pinned result slot (one of PIPE_DEPTH) on the copy stream
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
// grow-only plain host memory (the expanded results of cs_engine_seed_batch; `keep_n` elements survive a reallocation)
template <typename T> struct HostBuf {
	T *p = nullptr; size_t cap = 0;
	HostBuf() = default;
	HostBuf(const HostBuf &) = delete;
	HostBuf &operator=(const HostBuf &) = delete;
	HostBuf(HostBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
	HostBuf &operator=(HostBuf &&o) noexcept { if (this != &o) { release(); std::swap(p, o.p); std::swap(cap, o.cap); } return *this; }
	~HostBuf() { release(); }
	int reserve(size_t n, size_t keep_n = 0)
	{
		if (n <= cap) return 0;
		size_t want = std::max(n, cap + cap / 4);
		T *q = (T *)malloc(want * sizeof(T));
		if (!q) return 1;
		if (p && keep_n) memcpy(q, p, keep_n * sizeof(T));
		free(p);
		p = q; cap = want;
		return 0;
	}
	void release() { free(p); p = nullptr; cap = 0; }
};
// The slots, by what one is.  Which slot a part uses is decided in one place each (the upload thread takes a free input slot; the seeding
// thread's running part number k gives the pack slot k & 1 and the download event k % 4; the batch number gives the result slot); from
// there on the slot travels as a reference.
struct InSlot {                          // a staged part: taken by the upload thread, given back by the seeding thread after run_pass
	PinBuf<uint4> stage;                 // records made by the host (host_pack.cpp), staged for the upload into `in`
	DevBuf<uint8_t> in; DevBuf<uint64_t> inoff;
	bool is_free = true;
};
struct PackSlot {                        // a part's results as they travel, packed on the device by part k for k & 1 == the slot
	DevBuf<uint8_t> mems; DevBuf<uint64_t> moff, soff; DevBuf<uint32_t> rlo; DevBuf<uint8_t> rhi; // seeds: low words and fifth bytes of rbeg
	HipEvent packed;
};
struct BatchState {
	uint64_t id = ~0ull; int64_t n_reads = 0; int parts_total = 0, parts_queued = 0; uint64_t mem_base = 0, seed_base = 0;
	int rc = CS_OK; std::string err; bool sal = false, expand = false, expanded = false; int mem_format = CS_MEM_FULL32, max_occ = 0;
};
struct ResultSlot {                      // a batch's packed results in pinned memory, and the batch they belong to: batch id % PIPE_DEPTH
	PinBuf<uint64_t> moff, soff; PinBuf<uint8_t> mems; PinBuf<uint32_t> rlo; PinBuf<uint8_t> rhi;
	HipEvent done;                       // the download of the batch's last part
	BatchState b;
};
struct HostJob {
	uint64_t batch = 0; int part = 0, n_parts = 0;
	const uint8_t *bases = nullptr; const uint64_t *offsets = nullptr;
	int64_t r0 = 0, n = 0, n_reads = 0; uint64_t b0 = 0, nb = 0;
	cs_params_t par{}; int mem_format = CS_MEM_FULL32; bool expand = false, packed = false; // packed: the host makes the records (host_pack.cpp)
	InSlot *in = nullptr;                // from the upload thread on
};
struct XJob { uint64_t batch; int64_t r0, n; uint64_t mem_base, nm, seed_base, ns; hipEvent_t ev; bool last; };
struct HostPipe {
	HipStream s_up, s_down;              // the two copy streams (high priority: host_pipe_create)
	InSlot in[3]; PackSlot pack[2]; ResultSlot res[PIPE_DEPTH];
	HipEvent ev_dn[4];                   // the downloads of the last four parts: part k records ev_dn[k % 4]
	HostBuf<cs_intv_t> x_mems; HostBuf<cs_seed_t> x_seeds; // the expanded results of cs_engine_seed_batch
	std::thread th_up, th_seed, th_x;
	std::mutex mu; std::condition_variable cv;
	bool started = false, quit = false;
	std::deque<HostJob> q_up, q_seed; std::deque<XJob> q_x; bool x_busy = false;
	std::atomic<uint64_t> n_submitted{0}, n_collected{0}; // (one submitting and one collecting thread may run at the same time)
	long long handed = -1;               // batch whose pinned result slot the caller currently holds (until its next collect)

	ResultSlot &slot_of(uint64_t batch) { return res[batch % PIPE_DEPTH]; }
	InSlot *free_input() { for (InSlot &s : in) if (s.is_free) return &s; return nullptr; }
	void stop()                          // ends and joins the threads; what they queued on the streams is the caller's to drain
	{
		{ std::lock_guard<std::mutex> lk(mu); quit = true; cv.notify_all(); }
		for (std::thread *t : {&th_up, &th_seed, &th_x}) if (t->joinable()) t->join();
	}
	void drain() { for (hipStream_t s : {s_up.h, s_down.h}) if (s) (void)hipStreamSynchronize(s); }
	~HostPipe() { stop(); drain(); }     // (cs_engine_destroy has done both, in the order it states; the members then free their memory)
};

int host_pipe_create(cs_engine *e)
{
	e->hp.reset(new HostPipe());
	HostPipe &hp = *e->hp;
	int lo = 0, hi = 0;
	(void)hipDeviceGetStreamPriorityRange(&lo, &hi); // lo = least urgent
	// The runtime multiplexes the normal-priority streams of a process onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by
	// default), and a stream that shares its queue with a 30-ms download stands still for 30 ms -- measured: the seeding kernels
	// of a sub-batch took 65 instead of 45 ms beside the download of the previous one.  So the engine keeps to three normal
	// streams (main and two side streams; with the process's default stream that makes four); round 3 runs at low priority and
	// the two copy streams at high priority, which have queues of their own.  (The runtime maps streams to queues in creation
	// order: engine_init makes the pipe right after pass context 0.)
	HIP_TRY(hipStreamCreateWithPriority(&hp.s_up.h, hipStreamNonBlocking, hi));
	HIP_TRY(hipStreamCreateWithPriority(&hp.s_down.h, hipStreamNonBlocking, hi));
	for (PackSlot &s : hp.pack) HIP_TRY(hipEventCreateWithFlags(&s.packed.h, hipEventDisableTiming));
	for (HipEvent &ev : hp.ev_dn) HIP_TRY(hipEventCreateWithFlags(&ev.h, hipEventDisableTiming));
	for (ResultSlot &s : hp.res) HIP_TRY(hipEventCreateWithFlags(&s.done.h, hipEventDisableTiming));
	return CS_OK;
}
void PipeDelete::operator()(HostPipe *p) const { delete p; }

static void pipe_upload_thread(cs_engine *e)
{
	HostPipe &hp = *e->hp;
	(void)hipSetDevice(e->device);
	for (;;) {
		HostJob j;
		{
			std::unique_lock<std::mutex> lk(hp.mu);
			hp.cv.wait(lk, [&] { return hp.quit || (!hp.q_up.empty() && hp.free_input()); });
			if (hp.quit) return;
			j = hp.q_up.front(); hp.q_up.pop_front();
			j.in = hp.free_input(); j.in->is_free = false;
		}
		InSlot &in = *j.in;
		hipError_t he = hipSuccess;
		const double tu0 = e->opt.verbose > 1 ? pipe_ms() : 0.0;
		if (j.packed) {
			// the reads as records, made here chunk by chunk: the copy of chunk i runs beside the packing of chunk i + 1
			uint4 *st = in.stage.p;
			const int64_t csz = std::max<int64_t>(262144, (j.n + 7) / 8);
			for (int64_t c0 = 0; c0 < j.n && he == hipSuccess; c0 += csz) {
				const int64_t c1 = std::min<int64_t>(j.n, c0 + csz);
				cs_pack_reads_host_(j.bases, j.offsets, j.r0, j.n, c0, c1, st, e->opt.host_pack_threads, 0);
				const uint64_t f = ((j.offsets[j.r0 + c0] - j.b0) >> 5) + (uint64_t)c0, l = ((j.offsets[j.r0 + c1] - j.b0) >> 5) + (uint64_t)c1;
				he = hipMemcpyAsync(in.in.p + f * 16, st + f, (size_t)(l - f) * 16, hipMemcpyHostToDevice, hp.s_up);
			}
		} else if (j.nb) he = hipMemcpyAsync(in.in.p, j.bases + j.b0, (size_t)j.nb, hipMemcpyHostToDevice, hp.s_up);
		if (he == hipSuccess && j.offsets) he = hipMemcpyAsync(in.inoff.p, j.offsets + j.r0, ((size_t)j.n + 1) * 8, hipMemcpyHostToDevice, hp.s_up);
		if (he == hipSuccess && j.offsets) { hipLaunchKernelGGL(rebase_words_kernel, dim3(1), dim3(1024), 0, hp.s_up, in.inoff.p, (uint64_t)j.n + 1); he = hipGetLastError(); }
		if (he == hipSuccess) he = hipStreamSynchronize(hp.s_up);
		if (e->opt.verbose > 1) fprintf(stderr, "[cs_engine] batch %llu part %d/%d: %.1f MB %s in %.1f ms (from %.1f to %.1f ms)\n", (unsigned long long)j.batch, j.part + 1, j.n_parts, (double)(j.packed ? ((j.nb >> 5) + (uint64_t)j.n) * 16 : j.nb) / 1e6, j.packed ? "packed on the host and uploaded" : "uploaded", pipe_ms() - tu0, tu0, pipe_ms());
		std::lock_guard<std::mutex> lk(hp.mu);
		if (he != hipSuccess) { (void)hipGetLastError(); BatchState &b = hp.slot_of(j.batch).b; if (b.rc == CS_OK) { b.rc = CS_EDEVICE; b.err = std::string("upload: ") + hipGetErrorString(he); } }
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
		ResultSlot &rs = hp.slot_of(x.batch);
		BatchState &b = rs.b;
		bool ok = hipEventSynchronize(x.ev) == hipSuccess;
		if (ok) {
			const double scale = x.last ? 1.0 : (double)b.n_reads / (double)(x.r0 + x.n) * ((x.r0 + x.n) * 4 < b.n_reads ? 1.2 : 1.08); // room for the whole batch at the first growth
			ok = !hp.x_mems.reserve((size_t)((double)(x.mem_base + x.nm) * scale) + 1, (size_t)x.mem_base) &&
			     (!b.sal || !hp.x_seeds.reserve((size_t)((double)(x.seed_base + x.ns) * scale) + 1, (size_t)x.seed_base));
		}
		if (ok) {
			cs_packed_result_t Q; memset(&Q, 0, sizeof Q);
			Q.n_reads = b.n_reads; Q.mem_format = b.mem_format; Q.max_occ = b.max_occ;
			Q.mem_off = rs.moff.p; Q.mems = rs.mems.p; Q.seed_off = b.sal ? rs.soff.p : nullptr; Q.seed_format = CS_SEED_RBEG40; Q.seed_rbeg_lo = b.sal ? rs.rlo.p : nullptr; Q.seed_rbeg_hi = b.sal ? rs.rhi.p : nullptr;
			expand_parallel(Q, hp.x_mems.p, hp.x_seeds.p, x.r0, x.r0 + x.n, e->opt.expand_threads);
		}
		std::lock_guard<std::mutex> lk(hp.mu);
		if (!ok && b.rc == CS_OK) { b.rc = CS_ENOMEM; b.err = "expanding the packed results failed"; }
		if (x.last) b.expanded = true;
		hp.x_busy = false;
		hp.cv.notify_all();
	}
}

// What went wrong with a part, if anything: the code and the message its batch's collect returns.  The first error wins.
struct PartStatus {
	int rc = CS_OK; std::string err;
	bool ok() const { return rc == CS_OK; }
	void hip(hipError_t he, const char *what) { if (he != hipSuccess && rc == CS_OK) { (void)hipGetLastError(); rc = he == hipErrorOutOfMemory ? CS_ENOMEM : CS_EDEVICE; err = std::string(what) + ": " + hipGetErrorString(he); } }
	void cs(int r) { if (r != CS_OK && rc == CS_OK) { rc = r; err = g_err; } } // a CS_* return on this thread, with the message it left
	void grow(int r) { cs(r == CS_OK ? CS_OK : CS_ENOMEM); }                   // a buffer's reserve(): CS_ENOMEM whatever kept it from growing
};
// The part the seeding thread works on and the slots it uses.  k, the running number of the part, chose the pack slot and the download event.
struct Part {
	HostJob j; uint64_t k;
	ResultSlot &rs; PackSlot &ps; hipEvent_t dn; // dn: recorded behind this part's downloads
	uint64_t mem_base, seed_base;        // mems / seeds of the earlier parts of the batch
	PartStatus st; uint64_t nm = 0, ns = 0;
	bool sal() const { return j.par.want_sal != 0; }
	size_t msz() const { return j.mem_format == CS_MEM_LEAN8 ? sizeof(cs_mem8_t) : j.mem_format == CS_MEM_PACKED16 ? sizeof(cs_mem16_t) : sizeof(cs_intv_t); } // an element of the batch's own format
};

// The steps of the seeding thread, in the order it takes them.  Those that wait return false when the pipe is being stopped.
static bool take_part(HostPipe &hp, HostJob &j, PartStatus &st) // the next staged part, and how its batch has fared so far
{
	std::unique_lock<std::mutex> lk(hp.mu);
	hp.cv.wait(lk, [&] { return hp.quit || !hp.q_seed.empty(); });
	if (hp.quit) return false;
	j = hp.q_seed.front(); hp.q_seed.pop_front();
	st.rc = hp.slot_of(j.batch).b.rc;
	return true;
}
static void seed_part(cs_engine *e, PassCtx *c, Part &p)
{
	const HostJob &j = p.j;
	const double t0 = e->opt.verbose ? pipe_ms() : 0.0;
	if (p.st.ok()) p.st.cs(run_pass(e, c, &j.par, j.n, j.packed ? nullptr : j.in->in.p, j.in->inoff.p, j.nb, &p.nm, &p.ns, j.packed ? reinterpret_cast<const uint4 *>(j.in->in.p) : nullptr));
	if (e->opt.verbose) { // (with the wall clock of the seeding thread: idle gaps between parts show which neighbour it waited for)
		const double t1 = pipe_ms();
		fprintf(stderr, "[cs_engine] batch %llu part %d/%d: %lld reads seeded on context %d in %.1f ms (from %.1f to %.1f ms)\n", (unsigned long long)j.batch, j.part + 1, j.n_parts, (long long)j.n, c->id, t1 - t0, t0, t1);
	}
}
static void release_input(HostPipe &hp, Part &p) // the input slot is free again: the reads were converted into the context's own buffers
{
	std::lock_guard<std::mutex> lk(hp.mu);
	p.j.in->is_free = true; hp.cv.notify_all();
	if (p.st.ok()) p.st.rc = p.rs.b.rc;          // (the upload of a later part of the batch failed meanwhile)
}
static bool claim_result_slot(HostPipe &hp, Part &p)
{
	if (!p.st.ok()) return true;
	const HostJob &j = p.j; ResultSlot &rs = p.rs; const bool sal = p.sal(); const size_t msz = p.msz();
	// the batch that used this pinned result slot before may still be in the caller's hands: wait until it is given back
	{ std::unique_lock<std::mutex> lk(hp.mu); hp.cv.wait(lk, [&] { return hp.quit || hp.handed < 0 || (uint64_t)hp.handed == j.batch || &hp.slot_of((uint64_t)hp.handed) != &rs; }); if (hp.quit) return false; }
	// (from here on the result slot is this batch's) offsets: one entry per read + 1
	if (j.part == 0) { p.st.grow(rs.moff.reserve((size_t)j.n_reads + 1)); if (sal && p.st.ok()) p.st.grow(rs.soff.reserve((size_t)j.n_reads + 1)); }
	// pinned room for the whole batch: estimated from its first part, grown (keeping what has arrived) if that was too little
	const size_t need_m = (size_t)(p.mem_base + p.nm), need_s = (size_t)(p.seed_base + p.ns);
	if (need_m * msz > rs.mems.cap || (sal && need_s > rs.rlo.cap)) {
		p.st.hip(hipStreamSynchronize(hp.s_down), "draining downloads before growing the result buffers");
		{ std::unique_lock<std::mutex> lk(hp.mu); hp.cv.wait(lk, [&] { return hp.quit || (hp.q_x.empty() && !hp.x_busy); }); if (hp.quit) return false; } // the expander reads these buffers
		const double scale = (double)j.n_reads / (double)(j.r0 + j.n) * ((j.r0 + j.n) * 4 < j.n_reads ? 1.2 : 1.08); // (a small first part predicts the batch less well)
		if (p.st.ok()) p.st.grow(rs.mems.reserve((size_t)((double)need_m * scale) * msz + 4096, true, (size_t)p.mem_base * msz));
		if (p.st.ok() && sal) p.st.grow(rs.rlo.reserve((size_t)((double)need_s * scale) + 512, true, (size_t)p.seed_base));
		if (p.st.ok() && sal) p.st.grow(rs.rhi.reserve((size_t)((double)need_s * scale) + 512, true, (size_t)p.seed_base));
	}
	return true;
}
static void size_pack_slot(Part &p)
{
	if (p.st.ok()) p.st.grow(p.ps.mems.reserve((size_t)p.nm * p.msz() + 64));
	if (p.st.ok() && p.sal()) p.st.grow(p.ps.rlo.reserve((size_t)p.ns + 8));
	if (p.st.ok() && p.sal()) p.st.grow(p.ps.rhi.reserve((size_t)p.ns + 8));
}
static void pack_and_download(cs_engine *e, HostPipe &hp, PassCtx *c, Part &p)
{
	if (!p.st.ok()) {
		// a failed part still owns hp.ev_dn[k % 4] in the eyes of part k + 2: leave a recorded event behind
		(void)hipEventRecord(p.dn, hp.s_down);
		return;
	}
	const HostJob &j = p.j; ResultSlot &rs = p.rs; PackSlot &ps = p.ps; PartStatus &st = p.st;
	const uint64_t nm = p.nm, ns = p.ns; const size_t msz = p.msz();
	hipStream_t s = c->stream;                 // (the context's own stream: its next pass starts behind these kernels)
	const unsigned g = (unsigned)e->n_cu * 8;
	hipLaunchKernelGGL(shift_words_kernel, dim3(g), dim3(256), 0, s, (const uint64_t *)c->d_mem_off.p, (uint64_t)j.n + 1, p.mem_base, ps.moff.p);
	if (nm) {
		if (j.mem_format == CS_MEM_LEAN8) hipLaunchKernelGGL(pack_mems8_kernel, dim3(g), dim3(256), 0, s, (const OutMem *)c->d_mems.p, nm, (uint64_t *)ps.mems.p);
		else if (j.mem_format == CS_MEM_PACKED16) hipLaunchKernelGGL(pack_mems16_kernel, dim3(g), dim3(256), 0, s, (const OutMem *)c->d_mems.p, nm, (uint4 *)ps.mems.p);
		else st.hip(hipMemcpyAsync(ps.mems.p, c->d_mems.p, (size_t)nm * 32, hipMemcpyDeviceToDevice, s), "copying mems");
	}
	if (p.sal()) {
		hipLaunchKernelGGL(shift_words_kernel, dim3(g), dim3(256), 0, s, (const uint64_t *)c->d_seed_off.p, (uint64_t)j.n + 1, p.seed_base, ps.soff.p);
		if (ns) hipLaunchKernelGGL(pack_rbeg_kernel, dim3(g), dim3(256), 0, s, (const OutSeed *)c->d_seeds.p, ns, ps.rlo.p, ps.rhi.p);
	}
	st.hip(hipGetLastError(), "pack kernels");
	st.hip(hipEventRecord(ps.packed, s), "event");
	st.hip(hipStreamWaitEvent(hp.s_down, ps.packed, 0), "event");
	st.hip(hipMemcpyAsync(rs.moff.p + j.r0, ps.moff.p, ((size_t)j.n + 1) * 8, hipMemcpyDeviceToHost, hp.s_down), "download");
	if (nm) st.hip(hipMemcpyAsync(rs.mems.p + (size_t)p.mem_base * msz, ps.mems.p, (size_t)nm * msz, hipMemcpyDeviceToHost, hp.s_down), "download");
	if (p.sal()) {
		st.hip(hipMemcpyAsync(rs.soff.p + j.r0, ps.soff.p, ((size_t)j.n + 1) * 8, hipMemcpyDeviceToHost, hp.s_down), "download");
		if (ns) st.hip(hipMemcpyAsync(rs.rlo.p + p.seed_base, ps.rlo.p, (size_t)ns * 4, hipMemcpyDeviceToHost, hp.s_down), "download");
		if (ns) st.hip(hipMemcpyAsync(rs.rhi.p + p.seed_base, ps.rhi.p, (size_t)ns, hipMemcpyDeviceToHost, hp.s_down), "download");
	}
	st.hip(hipEventRecord(p.dn, hp.s_down), "event");
	if (j.part + 1 == j.n_parts) st.hip(hipEventRecord(rs.done, hp.s_down), "event");
}
static void publish(HostPipe &hp, Part &p) // the part counts as queued, failed or not
{
	const HostJob &j = p.j; BatchState &b = p.rs.b;
	std::lock_guard<std::mutex> lk(hp.mu);
	if (!p.st.ok() && b.rc == CS_OK) { b.rc = p.st.rc; b.err = p.st.err; }
	if (p.st.ok()) {
		b.mem_base += p.nm; b.seed_base += p.ns;
		if (j.expand) { XJob x = {j.batch, j.r0, j.n, p.mem_base, p.nm, p.seed_base, p.ns, p.dn, j.part + 1 == j.n_parts}; hp.q_x.push_back(x); }
	}
	b.parts_queued++;
	hp.cv.notify_all();
}

// The seeding thread: parts are taken in order and seeded on pass context 0, one at a time.
static void pipe_seed_thread(cs_engine *e)
{
	HostPipe &hp = *e->hp;
	(void)hipSetDevice(e->device);
	PassCtx *c = e->ctx[0].get();
	for (uint64_t k = 0;; ++k) {                   // running part number: pack slot k & 1, download event k % 4
		HostJob j; PartStatus st;
		if (!take_part(hp, j, st)) return;
		ResultSlot &rs = hp.slot_of(j.batch);
		Part p{j, k, rs, hp.pack[k & 1], hp.ev_dn[k % 4], rs.b.mem_base, rs.b.seed_base, st};
		seed_part(e, c, p);
		release_input(hp, p);
		// the pack buffers of this slot were last used by the part before the previous one: its download must be over
		if (p.st.ok() && k >= 2) p.st.hip(hipEventSynchronize(hp.ev_dn[(k - 2) % 4]), "waiting for a download");
		if (!claim_result_slot(hp, p)) return;
		size_pack_slot(p);
		pack_and_download(e, hp, c, p);
		publish(hp, p);
	}
}

static bool host_pipe_busy(const cs_engine *e) { return e->hp->n_submitted.load() != e->hp->n_collected.load(); }
static bool dev_pipe_busy(const cs_engine *e);
bool pipe_busy(const cs_engine *e) { return host_pipe_busy(e) || dev_pipe_busy(e); }


// The parts of batch `id` as jobs, and the capacities they need of the buffers all batches share (input slots, the pack slots' offsets)
struct SharedCaps { size_t in = 0, off = 0, stage = 0; };
static std::vector<HostJob> make_parts(const cs_engine *e, uint64_t id, const std::vector<int64_t> &cut, const cs_params_t *par, int64_t n_reads, const uint8_t *bases,
                                       const uint64_t *offsets, uint64_t max_len, bool expand, SharedCaps &cap)
{
	std::vector<HostJob> parts;
	const int64_t kparts = (int64_t)cut.size() - 1;
	const bool host_pack = e->opt.host_pack_threads > 0 && e->smem_mode == 1;
	for (int64_t i = 0; i < kparts; ++i) {
		HostJob j; j.batch = id; j.part = (int)i; j.n_parts = (int)kparts; j.bases = bases; j.offsets = offsets; j.n_reads = n_reads;
		j.r0 = cut[(size_t)i]; j.n = cut[(size_t)i + 1] - j.r0;
		j.b0 = n_reads ? offsets[j.r0] : 0; j.nb = n_reads ? offsets[j.r0 + j.n] - j.b0 : 0;
		j.par = *par; j.expand = expand;
		// the packed forms need an index shorter than 2^33 symbols and reads shorter than 2^15 bases; a lean batch takes the 8-byte one
		j.mem_format = (e->ix.seq_len >> 33) == 0 && max_len < (1u << 15) ? (lean_results(par) ? CS_MEM_LEAN8 : CS_MEM_PACKED16) : CS_MEM_FULL32;
		j.packed = host_pack;
		const size_t n_rec = (size_t)(j.nb >> 5) + (size_t)j.n;
		cap.in = std::max<size_t>(cap.in, host_pack ? (n_rec + 4) * 16 : j.nb); cap.off = std::max<size_t>(cap.off, (size_t)j.n + 1);
		if (host_pack) cap.stage = std::max<size_t>(cap.stage, n_rec + 4);
		parts.push_back(j);
	}
	return parts;
}
// The shared buffers, sized while no part of the new batch (result slot `mine`) is in flight: earlier batches never need more than they
// have.  Called with hp.mu held through lk; returns with it held unless it fails.
static int grow_shared(cs_engine *e, HostPipe &hp, std::unique_lock<std::mutex> &lk, const ResultSlot &mine, const SharedCaps &cap, bool sal)
{
	if (!(cap.in + 64 > hp.in[0].in.cap || cap.stage > hp.in[0].stage.cap || cap.off > hp.in[0].inoff.cap || cap.off > hp.pack[0].moff.cap || (sal && cap.off > hp.pack[0].soff.cap))) return CS_OK;
	// a reallocation frees buffers the other batch may still be using: not only while its parts are queued or being seeded
	// (the input slots are given back right after run_pass), but until the seeding thread has queued the pack kernels
	// and downloads of its LAST part (parts_queued == parts_total) and those have drained (s_down below)
	auto others_queued = [&] { for (const ResultSlot &o : hp.res) if (&o != &mine && o.b.parts_queued != o.b.parts_total) return false; return true; };
	hp.cv.wait(lk, [&] { return hp.quit || (hp.q_up.empty() && hp.q_seed.empty() && hp.in[0].is_free && hp.in[1].is_free && hp.in[2].is_free && others_queued()); });
	lk.unlock();
	for (auto &c : e->ctx) if (c) HIP_TRY(hipStreamSynchronize(c->stream));
	HIP_TRY(hipStreamSynchronize(hp.s_down));
	for (InSlot &s : hp.in) { CS_TRY(s.in.reserve(cap.in + 64)); CS_TRY(s.stage.reserve(cap.stage)); CS_TRY(s.inoff.reserve(cap.off)); }
	for (PackSlot &s : hp.pack) {
		CS_TRY(s.moff.reserve(cap.off));
		if (sal) CS_TRY(s.soff.reserve(cap.off));
	}
	lk.lock();
	return CS_OK;
}

static int pipe_submit(cs_engine *e, const cs_params_t *par, int64_t n_reads, const uint8_t *bases, const uint64_t *offsets, bool expand)
{
	if (!e || !par || n_reads < 0 || (n_reads > 0 && !offsets)) return fail(CS_EINVAL, "cs_engine_submit: bad argument");
	if (!result_flags_ok(par)) return fail(CS_EINVAL, "unknown bits in result_flags, or reserved is not 0");
	if (n_reads >= (int64_t)0xffffffffll) return fail(CS_ERANGE, "more than 2^32-1 reads in one call");
	if (par->min_seed_len < 1 || par->max_occ < 1 || par->split_width < 0) return fail(CS_EINVAL, "bad seeding parameters");
	HIP_TRY(hipSetDevice(e->device));
	if (dev_pipe_busy(e)) return fail(CS_EINVAL, "cs_engine_submit: device batches are in flight (cs_engine_submit_device), collect them first");
	drop_held(e);
	HostPipe &hp = *e->hp;
	if (hp.n_submitted.load() - hp.n_collected.load() >= (uint64_t)PIPE_DEPTH) return fail(CS_EINVAL, "cs_engine_submit: four batches are in flight already, collect one first");
	uint64_t max_len = 0;
	if (n_reads > 0) {
		if (offsets[0] == 0 && offsets[n_reads] > 0 && !bases) return fail(CS_EINVAL, "bases is null"); // (reported after offsets[0] != 0, before the rest)
		const host_parts::OffsetCheck v = host_parts::check_offsets(offsets, n_reads);
		if (v.rc != CS_OK) return fail(v.rc, v.msg);
		max_len = v.max_len;
	}
	const uint64_t id = hp.n_submitted.load();
	ResultSlot &rs = hp.slot_of(id);
	const bool streaming = hp.n_submitted.load() - hp.n_collected.load() >= 2 && !expand;
	const std::vector<int64_t> cut = host_parts::cut_parts(n_reads, e->opt.pipeline_reads, streaming);
	SharedCaps cap;
	const std::vector<HostJob> parts = make_parts(e, id, cut, par, n_reads, bases, offsets, max_len, expand, cap);
	std::unique_lock<std::mutex> lk(hp.mu);
	CS_TRY(grow_shared(e, hp, lk, rs, cap, par->want_sal != 0));
	BatchState &b = rs.b;
	b = BatchState();
	b.id = id; b.n_reads = n_reads; b.parts_total = (int)parts.size(); b.mem_format = parts[0].mem_format; b.sal = par->want_sal != 0; b.expand = expand; b.max_occ = par->max_occ;
	for (auto &j : parts) hp.q_up.push_back(j);
	if (e->opt.verbose > 1) fprintf(stderr, "[cs_engine] batch %llu submitted at %.1f ms in %d part(s)\n", (unsigned long long)id, pipe_ms(), (int)parts.size());
	hp.n_submitted++;
	invalidate_last(e);
	if (!hp.started) { // (on the first submit: an engine that never uses the host pipeline has no idle threads)
		hp.started = true;
		hp.th_up = std::thread(pipe_upload_thread, e); hp.th_x = std::thread(pipe_expand_thread, e); hp.th_seed = std::thread(pipe_seed_thread, e);
	}
	hp.cv.notify_all();
	return CS_OK;
}

static int pipe_collect(cs_engine *e, cs_packed_result_t *out)
{
	if (!e || !out) return fail(CS_EINVAL, "cs_engine_collect: null argument");
	if (!host_pipe_busy(e)) return fail(CS_EINVAL, "cs_engine_collect: nothing has been submitted");
	HIP_TRY(hipSetDevice(e->device));
	HostPipe &hp = *e->hp;
	const uint64_t id = hp.n_collected.load();
	ResultSlot &rs = hp.slot_of(id);
	BatchState &b = rs.b;
	int rc; std::string err;
	{
		std::unique_lock<std::mutex> lk(hp.mu);
		hp.handed = -1;                      // the result handed out by the previous collect is given back: its slot may be overwritten
		hp.cv.notify_all();
		hp.cv.wait(lk, [&] { return b.parts_queued == b.parts_total; });
		rc = b.rc; err = b.err;              // (under the lock: the expander may still be writing them)
	}
	const double tc0 = e->opt.verbose > 1 ? pipe_ms() : 0.0;
	if (rc == CS_OK && hipEventSynchronize(rs.done) != hipSuccess) { rc = CS_EDEVICE; err = "waiting for the download"; (void)hipGetLastError(); }
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
	out->mem_format = b.mem_format;
	out->mem_off = rs.moff.p; out->mems = rs.mems.p;
	out->seed_off = b.sal ? rs.soff.p : nullptr; out->seed_format = CS_SEED_RBEG40;
	out->seed_rbeg_lo = b.sal ? rs.rlo.p : nullptr; out->seed_rbeg_hi = b.sal ? rs.rhi.p : nullptr;
	{ // cs_engine_result_digest / gather_reads work on the device-side result, which is the whole batch only if it was not cut
		std::lock_guard<std::mutex> lk(hp.mu); // (a submit on another thread invalidates it under the same lock)
		PassCtx *c = e->ctx[0].get();        // the seeding thread's context
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
	void stop() { { std::lock_guard<std::mutex> lk(mu); quit = true; cv.notify_all(); } for (auto &t : th) if (t.joinable()) t.join(); }
	~DevPipe() { stop(); }
};
void PipeDelete::operator()(DevPipe *p) const { delete p; }
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
// cs_engine_destroy's first and third step (the order is written down there); an engine whose creation failed early has no pipe yet
void pipes_stop(cs_engine *e)
{
	if (e->hp) e->hp->stop();
	if (e->dp) e->dp->stop();
}
void host_pipe_drain(cs_engine *e) { if (e->hp) e->hp->drain(); }
extern "C" int cs_engine_submit_device(cs_engine_t *e, const cs_params_t *par, int64_t n_reads, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_bases)
{
	if (!e || !par || n_reads < 0 || (n_reads > 0 && !d_offsets) || (n_bases > 0 && !d_bases)) return fail(CS_EINVAL, "cs_engine_submit_device: bad argument");
	if (!result_flags_ok(par)) return fail(CS_EINVAL, "unknown bits in result_flags, or reserved is not 0");
	if (n_reads >= (int64_t)0xffffffffll) return fail(CS_ERANGE, "more than 2^32-1 reads in one call");
	if (host_pipe_busy(e)) return fail(CS_EINVAL, "cs_engine_submit_device: host batches are in flight (cs_engine_submit), collect them first");
	HIP_TRY(hipSetDevice(e->device));
	if (!e->dp) {
		if (e->opt.passes_in_flight >= 2 && !e->ctx[1]) CS_TRY(add_pass_ctx(e));
		e->dp.reset(new DevPipe());
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
	out->mem_off = P.mem_off; out->mems = e->hp->x_mems.p;
	out->seed_off = P.seed_off; out->seeds = par->want_sal ? e->hp->x_seeds.p : nullptr;
	return CS_OK;
}
