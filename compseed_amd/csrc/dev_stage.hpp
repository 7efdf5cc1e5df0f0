// dev_stage.hpp -- the host half that the device units share: the HIP error macro; the owning types (DevBuf, PinBuf, HipStream, HipEvent)
// that every unit keeps device memory, pinned memory, streams and events in; and the stage layer of the units outside the engine
// (chain_gpu.hip, chain_filter_gpu.hip, align_gpu.hip, extend.hip, cigar_gpu.hip, mark_gpu.hip): cs_dev_stage, the state every stage keeps
// (device, stream, timing events, pinned counter words, rocPRIM's scratch) with the launch / upload / scan helpers, the creation of a stage
// on first use, its deletion and its statistics, the host's check of a batch without regions, and the download of a chain result.
// Header-only.  A stage derives its state from cs_dev_stage and declares its device buffers as DevBuf<T> members of the type its kernels
// read; it grows them with DevBuf::ensure, which frees before it allocates.  This is the HOST half only: what the kernels of
// chain_filter_gpu.hip, align_gpu.hip, cigar_gpu.hip and mark_gpu.hip loop over are the bodies of chain_filter_scan.hpp, align_scan.hpp,
// cigar_scan.hpp and mark_scan.hpp, on the lanes of wave_lanes.hpp and the alignment of band_align.hpp, which plain C++ programs run on the CPU (tests/cpp/).
#pragma once
#include "cs_internal.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#define HIP_TRY(expr)                                                                               \
	do {                                                                                            \
		hipError_t e__ = (expr);                                                                    \
		if (e__ != hipSuccess) {                                                                    \
			(void)hipGetLastError();                                                                \
			return cs_fail_(e__ == hipErrorOutOfMemory ? CS_ENOMEM : CS_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e__)); \
		}                                                                                           \
	} while (0)

// ---- owning buffers and handles: what the engine's units, the extender and the index builder keep their device state in
// Grow-only buffers that free their memory when destroyed; move-only.
template <typename T> struct DevBuf {
	T *p = nullptr; size_t cap = 0;
	DevBuf() = default;
	DevBuf(const DevBuf &) = delete;
	DevBuf &operator=(const DevBuf &) = delete;
	DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
	DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); std::swap(p, o.p); std::swap(cap, o.cap); } return *this; }
	~DevBuf() { release(); }
	int reserve(size_t n, bool keep = false, hipStream_t s = nullptr, size_t keep_n = 0)
	{
		if (n <= cap) return CS_OK;
		size_t want = std::max(n, cap + cap / 2);
		T *q = nullptr;
		HIP_TRY(hipMalloc((void **)&q, want * sizeof(T)));
		if (keep && p && keep_n) {
			hipError_t e = hipMemcpyAsync(q, p, keep_n * sizeof(T), hipMemcpyDeviceToDevice, s);
			if (e == hipSuccess) e = hipStreamSynchronize(s);
			if (e != hipSuccess) { (void)hipFree(q); return cs_fail_(CS_EDEVICE, hipGetErrorString(e)); }
		}
		if (p) (void)hipFree(p);
		p = q; cap = want;
		return CS_OK;
	}
	// the stages' way to grow: room for n elements and `pad` more bytes (what a kernel's wide loads may read behind the last element).
	// The contents are not kept and the old memory is freed BEFORE the new is allocated (a stage's peak at hg19 size depends on it); a
	// failed growth leaves the buffer empty (p == nullptr, cap == 0), never dangling.  cap counts the whole elements of what was allocated.
	int ensure(size_t n, size_t pad = 0)
	{
		const size_t bytes = n * sizeof(T) + pad;
		if (bytes <= cap * sizeof(T)) return CS_OK;
		release();
		const size_t want = bytes + bytes / 8 + 256;
		HIP_TRY(hipMalloc((void **)&p, want));
		cap = want / sizeof(T);
		return CS_OK;
	}
	void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
// DevBuf::ensure(n, pad) on each of the buffers, up to the first that fails
template <class... B> int cs_ensure_each_(size_t n, size_t pad, B &...b)
{
	int rc = CS_OK;
	(void)(((rc = b.ensure(n, pad)) == CS_OK) && ...);
	return rc;
}
template <typename T> struct PinBuf {
	T *p = nullptr, *dp = nullptr; size_t cap = 0; // dp: the same memory as the device addresses it (kernels may store into it)
	PinBuf() = default;
	PinBuf(const PinBuf &) = delete;
	PinBuf &operator=(const PinBuf &) = delete;
	PinBuf(PinBuf &&o) noexcept : p(o.p), dp(o.dp), cap(o.cap) { o.p = o.dp = nullptr; o.cap = 0; }
	PinBuf &operator=(PinBuf &&o) noexcept { if (this != &o) { release(); std::swap(p, o.p); std::swap(dp, o.dp); std::swap(cap, o.cap); } return *this; }
	~PinBuf() { release(); }
	int reserve(size_t n, bool keep = false, size_t keep_n = 0)
	{
		if (n <= cap) return CS_OK;
		size_t want = std::max(n, cap + cap / 2);
		T *q = nullptr;
		HIP_TRY(hipHostMalloc((void **)&q, want * sizeof(T), hipHostMallocDefault));
		if (keep && p && keep_n) memcpy(q, p, keep_n * sizeof(T));
		if (p) (void)hipHostFree(p);
		p = q; cap = want; dp = nullptr;
		void *d = nullptr;
		if (hipHostGetDevicePointer(&d, p, 0) == hipSuccess) dp = (T *)d; else (void)hipGetLastError();
		return CS_OK;
	}
	void release() { if (p) (void)hipHostFree(p); p = nullptr; dp = nullptr; cap = 0; }
};
// a stream or an event, destroyed with its holder; converts to the raw handle, so it is passed to the HIP calls as it is
template <typename H, hipError_t (*Destroy)(H)> struct HipHandle {
	H h = nullptr;
	HipHandle() = default;
	HipHandle(const HipHandle &) = delete;
	HipHandle &operator=(const HipHandle &) = delete;
	HipHandle(HipHandle &&o) noexcept : h(o.h) { o.h = nullptr; }
	HipHandle &operator=(HipHandle &&o) noexcept { std::swap(h, o.h); return *this; }
	~HipHandle() { if (h) (void)Destroy(h); }
	operator H() const { return h; }
};
using HipStream = HipHandle<hipStream_t, hipStreamDestroy>;
using HipEvent = HipHandle<hipEvent_t, hipEventDestroy>;

// ---- the stage layer
struct cs_dev_stage {
	static constexpr int N_CTR = 8;                                   // pinned counter words, and the size of a stage's device counter block
	int device = 0, n_cu = 256;
	// Members are destroyed in the reverse of their declaration and a derived stage's before these: its buffers (and the extender's side
	// streams) go first, then rocPRIM's scratch, the pinned words and the events, and the stream they were used on is destroyed last.
	HipStream s; HipEvent ev[4];                                      // ev: two pairs around a call's kernels (init's `timing`)
	PinBuf<unsigned long long> h_ctr; DevBuf<uint8_t> scratch;        // scratch: rocPRIM's, for scan() and the extender's sort

	int init(int device, bool timing)
	{
		HIP_TRY(hipSetDevice(device));
		this->device = device;
		hipDeviceProp_t prop;
		if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) n_cu = prop.multiProcessorCount;
		HIP_TRY(hipStreamCreateWithFlags(&s.h, hipStreamNonBlocking));
		if (timing) for (HipEvent &e : ev) HIP_TRY(hipEventCreate(&e.h));
		return h_ctr.reserve(N_CTR);
	}
	void drain() const { if (s) (void)hipStreamSynchronize(s); }       // what cs_dev_stage_delete_ waits for

	dim3 grid(int64_t items, int per_block = 256) const { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, (int64_t)n_cu * 16))); }
	template <class T> int up(DevBuf<T> &b, const T *src, size_t n)   // host -> b on the stream; the caller keeps src alive until it has waited
	{
		if (int rc = b.ensure(n, 64)) return rc;
		if (n) HIP_TRY(hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
		return CS_OK;
	}
	// exclusive sums on the stream, rocprim's scratch in `scratch`; the two-array form: one scratch buffer of the larger size, two scans
	template <class T> int scan(T *in, T *out, size_t n, T init)   // (`in` is not const: the kernels rocprim instantiates carry the iterator types)
	{
		size_t tb = 0;
		HIP_TRY(rocprim::exclusive_scan(nullptr, tb, in, out, init, n, rocprim::plus<T>(), s));
		if (int rc = scratch.ensure(tb, 16)) return rc;
		HIP_TRY(rocprim::exclusive_scan(scratch.p, tb, in, out, init, n, rocprim::plus<T>(), s));
		return CS_OK;
	}
	template <class T> int scan(T *in, T *out, T *in2, T *out2, size_t n, T init)
	{
		size_t tb = 0, tb2 = 0;
		HIP_TRY(rocprim::exclusive_scan(nullptr, tb, in, out, init, n, rocprim::plus<T>(), s));
		HIP_TRY(rocprim::exclusive_scan(nullptr, tb2, in2, out2, init, n, rocprim::plus<T>(), s));
		tb = std::max(tb, tb2);
		if (int rc = scratch.ensure(tb, 16)) return rc;
		HIP_TRY(rocprim::exclusive_scan(scratch.p, tb, in, out, init, n, rocprim::plus<T>(), s));
		HIP_TRY(rocprim::exclusive_scan(scratch.p, tb, in2, out2, init, n, rocprim::plus<T>(), s));
		return CS_OK;
	}
	int empty_csr(uint64_t *chain_off, uint64_t *cseed_off)   // the result of a call without reads: both offset arrays are {0}
	{
		HIP_TRY(hipMemsetAsync(chain_off, 0, sizeof *chain_off, s));
		HIP_TRY(hipMemsetAsync(cseed_off, 0, sizeof *cseed_off, s));
		HIP_TRY(hipStreamSynchronize(s));
		return CS_OK;
	}
	void add_kernel_ms(double &kernel_ms) const   // ev[0]..ev[1] and ev[2]..ev[3], after the stream has been waited for
	{
		float ms0 = 0.f, ms1 = 0.f;
		if (hipEventElapsedTime(&ms0, ev[0], ev[1]) == hipSuccess && hipEventElapsedTime(&ms1, ev[2], ev[3]) == hipSuccess) kernel_ms += (double)ms0 + ms1;
	}
};

// the end of a stage (null-safe): its device current, its streams waited for, then the members in the order cs_dev_stage declares
template <class Stage> void cs_dev_stage_delete_(Stage *g)
{
	if (!g) return;
	(void)hipSetDevice(g->device);
	g->drain();
	delete g;
}
// A stage on first use: init and the unit's one-time uploads (setup(stage): reference, contig table, ...).  The owner sees the state only
// when all of that has succeeded; otherwise it is destroyed, the error returned, and the next call starts over.
template <class Stage, class Setup> int cs_dev_stage_make_(Stage **owner, int device, bool timing, Setup setup)
{
	if (*owner) return CS_OK;
	Stage *g = new Stage();
	int rc = g->init(device, timing);
	if (rc == CS_OK) rc = setup(*g);
	if (rc != CS_OK) { cs_dev_stage_delete_(g); return rc; }
	*owner = g;
	return CS_OK;
}
template <class Stage, class Stats> int cs_dev_stage_stats_(const Stage *g, Stats *st)   // a stage's `st`, zeroes before its first call
{
	if (g) *st = g->st; else memset(st, 0, sizeof *st);
	return CS_OK;
}

// a batch without reads or without regions has nothing for the device: what the host can refuse of it (`what`: the call's name)
inline int cs_check_no_regions_(const char *what, const cs_aln_result_t *regs, const uint64_t *read_offsets)
{
	const int64_t n = regs->n_reads;
	if (n == 0 && regs->n_regs) return cs_fail_(CS_EINVAL, std::string(what) + ": regions without reads");
	if (n && (regs->reg_off[0] != 0 || read_offsets[0] != 0)) return cs_fail_(CS_EINVAL, std::string(what) + ": the offsets do not start at 0");
	for (int64_t r = 0; r < n; ++r) if (regs->reg_off[r + 1] != 0 || read_offsets[r + 1] < read_offsets[r]) return cs_fail_(CS_EINVAL, std::string(what) + ": reg_off / read_offsets are not CSR offset arrays");
	return CS_OK;
}

// a chain result in device memory into host vectors (d_score / score: the filter's seed scores, or null), and `out` onto the vectors
inline int cs_download_chains_(hipStream_t s, const cs_chain_result_t &d, const int32_t *d_score, std::vector<uint64_t> &chain_off, std::vector<cs_chain_t> &chains,
                               std::vector<uint64_t> &cseed_off, std::vector<cs_seed_t> &cseeds, std::vector<int32_t> *score, cs_chain_result_t *out)
{
	const size_t n = (size_t)d.n_reads;
	chain_off.resize(n + 1); chains.resize(d.n_chains); cseed_off.resize(d.n_chains + 1); cseeds.resize(d.n_seeds);
	if (score) score->resize(d.n_seeds);
	HIP_TRY(hipMemcpyAsync(chain_off.data(), d.chain_off, (n + 1) * sizeof *d.chain_off, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(cseed_off.data(), d.cseed_off, ((size_t)d.n_chains + 1) * sizeof *d.cseed_off, hipMemcpyDeviceToHost, s));
	if (d.n_chains) HIP_TRY(hipMemcpyAsync(chains.data(), d.chains, (size_t)d.n_chains * sizeof(cs_chain_t), hipMemcpyDeviceToHost, s));
	if (d.n_seeds) {
		HIP_TRY(hipMemcpyAsync(cseeds.data(), d.cseeds, (size_t)d.n_seeds * sizeof(cs_seed_t), hipMemcpyDeviceToHost, s));
		if (score) HIP_TRY(hipMemcpyAsync(score->data(), d_score, (size_t)d.n_seeds * sizeof *d_score, hipMemcpyDeviceToHost, s));
	}
	HIP_TRY(hipStreamSynchronize(s));
	out->n_reads = d.n_reads; out->n_chains = d.n_chains; out->n_seeds = d.n_seeds;
	out->chain_off = chain_off.data(); out->chains = chains.data(); out->cseed_off = cseed_off.data(); out->cseeds = cseeds.data();
	return CS_OK;
}
