// engine.hpp -- what the translation units of the seeding engine share (not part of the C ABI):
//   engine.hip     ABI lifecycle, options, index load / residency, statistics, device memory helpers
//   seed_pass.hip  one seeding pass on a pass context: SMEM stage, sort, SAL; the k-mer filter.  The only unit that includes the
//                  kernels of the default SMEM path, smem_common.hpp and smem_{reads,fwd,bwd,text,sort}.hpp
//   pipelines.hip  the host pipeline (cs_engine_submit / collect, blocking host variants) and the device pipeline, each with all the state
//                  only it uses (HostPipe, DevPipe: the engine holds an owning pointer to either); host_parts.hpp: the offset check and the
//                  cut into parts of a host submit, plain C++
//   inspect.hip    digest and gather of the last result, index validation, primitives, the random-line probe
//   dev_stage.hpp  HIP_TRY, the owning types the members below are made of (DevBuf, PinBuf, HipStream, HipEvent), and the stage layer of the
//                  units outside the engine (chain_gpu.hip, chain_filter_gpu.hip, align_gpu.hip, extend.hip)
// Kernels are defined in the unit that launches them; the headers included by more than one unit hold types and __device__ functions.
#pragma once
#include "cs_internal.hpp"
#include "dev_stage.hpp"
#include "fm_device.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <shared_mutex>
#include <string>

#include <hip/hip_runtime.h>

using namespace csd;

extern thread_local std::string g_err;
inline int fail(int code, const std::string &msg) { g_err = msg; return code; }

#define CS_TRY(expr) do { int rc__ = (expr); if (rc__ != CS_OK) return rc__; } while (0)

inline unsigned grid_for(int64_t n, int block) { return (unsigned)std::max<int64_t>(1, (n + block - 1) / block); }

// ------------------------------------------------------------------------------------------------ engine
// The words of PassCtx::d_sctr / h_sctr, the counters of the split SMEM stage.  seed_pass.hip hands the kernels pointers to them
// (SplitArgs and kernel arguments) and reads the whole block back after every iteration.
enum : int {
	SC_TASK = 0,           // task dispenser of the forward kernels
	SC_NEXT_N = 1,         // length of the next forward queue, no-op slots included
	SC_BWD_CLS = 2,        // 2..5: slot counters of the backward kernels' size classes
	SC_BWD_WIDE = 5,       // ... the last of them: calls with more than 64 LEPs (bwd_wide_kernel)
	SC_OVF_MEMS = 6,       // mems beyond a read's first `cap` (overflow records)
	SC_ERR = 7,            // sticky: a queue or the overflow records ran full
	SC_QUERIES = 8,        // bwt_extend queries
	SC_SST_HITS = 9,       // ... of which the on-device SST answered
	SC_R3_TASK = 10,       // task dispenser of round 3 on the index (its own stream)
	SC_R2_TEXT = 11,       // re-seeding calls answered from the text (r2text_kernel, fwd0_kernel's quick test)
	SC_R2_INDEX = 12,      // re-seeding calls left to the index
	SC_BTASKS = 13,        // backward calls created by the last forward launch
	SC_TEXT_SWEEPS = 14,   // backward sweeps answered from the text
	SC_R3_TEXT_SEEDS = 15, // round-3 seeds made by r3text_kernel
	SC_DENSE_N = 16,       // length of the next forward queue as r2text_kernel has compacted it
	SC_WORDS = 32
};
// The words of PassCtx::d_ctr / h_ctr as seed_pass.hip uses them (inspect.hip takes d_ctr as scratch of its own)
enum : int {
	CTR_TASK = 0,          // task dispenser of the fused kernel
	CTR_FETCHED = 0,       // h_ctr only: where a single fetched word (a running total) lands
	CTR_FETCHED2 = 1,      // h_ctr only: ... and the second of a pair (place_mems: the seed total beside the mem total)
	CTR_QUERIES = 1,       // bwt_extend queries of the fused kernel
	CTR_OVERFLOW = 2,      // reads with more than `cap` mems (fused path)
	CTR_MAX_LEN = 3,       // longest read of the batch
	CTR_BAD_OFFSETS = 4,   // offsets that do not tile [0, n_bases)
	CTR_SAL_DISTINCT = 5,  // distinct SA slots per 512-read batch (engine option count_sal_merged)
	CTR_SEED_RANGE = 6,    // raised by sort_expand16_kernel / sal_expand_heavy_kernel: a read's seeds did not fill its range of seed_off[] exactly
	CTR_WORDS = 8
};
// What one seeding pass owns.  An engine has one or two of them: the tail of a pass (late iterations with a few thousand calls each,
// the sort, SAL, ten host round trips) leaves most of the GPU idle, and a small part of a batch is nearly all tail; a second pass,
// on a context of its own, fills it.
struct PassCtx {
	HipStream stream, stream2, stream3, stream4; // stream2: round 3 (low priority); stream3: calls without LEPs; stream4: wide sweeps
	HipEvent ev_r3a, ev_r3b, ev_wa, ev_wb, ev_wc;
	HipEvent ev[4];
	DevBuf<uint8_t> d_pending; // r3text_kernel: reads with calls of rounds 1/2 still queued when it starts
	DevBuf<uint32_t> d_cnt_snap; DevBuf<uint64_t> d_aux; // re-seeding from the text: r3text_kernel's snapshot of the mem counts; side words of d_fqB's re-seeding calls
	// inputs
	DevBuf<uint8_t> d_seq; DevBuf<uint4> d_seqp; const uint4 *seqp_cur = nullptr; const uint64_t *off_base = nullptr; // d_seqp: pack_reads_kernel's records for the batch whose offsets start at off_base
	// SMEM stage
	DevBuf<OutMem> d_out, d_out2; DevBuf<uint32_t> d_cnt, d_cnt2, d_ovf; DevBuf<uint4> d_spill;
	DevBuf<uint32_t> d_scnt; // SA slots per read, counted beside d_cnt while the split kernels emit the mems (SplitArgs::out_scnt)
	DevBuf<unsigned long long> d_ctr; // CTR_WORDS words: the CTR_* enum above for seed_pass.hip, anonymous scratch for inspect.hip
	DevBuf<uint8_t> d_tmp, d_tmp2;
	PinBuf<unsigned long long> h_ctr;
	// results (device)
	DevBuf<uint64_t> d_mem_off, d_seed_off, d_seed_of_mem; DevBuf<OutMem> d_mems; DevBuf<uint64_t> d_salcnt; DevBuf<OutSeed> d_seeds; // d_salcnt: SA slots per mem, written by the sort that makes d_mems; with d_seed_of_mem only where run_sal runs (seed_pass.hip)
	// split (forward / cooperative backward) SMEM path
	DevBuf<uint64_t> d_fqA, d_fqB, d_fqR; DevBuf<uint4> d_sst2; DevBuf<BTask> d_bq; DevBuf<uint4> d_lep; DevBuf<OvfRec> d_ovfrec;
	DevBuf<uint32_t> d_okey, d_oidx, d_okey2, d_oidx2; DevBuf<uint64_t> d_okey64, d_okey64b; DevBuf<unsigned long long> d_sctr; PinBuf<unsigned long long> h_sctr;
	cs_stats_t st{};
	DevBuf<unsigned long long> d_evc; uint64_t stream_bytes = 0; // byte model: event counters [N_KID][N_EV] on the device, stream part on the host
	struct { bool valid = false; int64_t n_reads = 0; uint64_t n_mems = 0, n_seeds = 0; int want_sal = 0; } last; // the result held in d_mems / d_seeds
	int id = 0; // index in cs_engine::ctx
	// device bytes of every buffer above, as reserved (cs_engine_memory)
	uint64_t device_bytes() const
	{
		uint64_t b = 0;
		auto add = [&b](const auto &...buf) { ((b += (uint64_t)buf.cap * sizeof(*buf.p)), ...); };
		add(d_pending, d_cnt_snap, d_aux, d_seq, d_seqp, d_out, d_out2, d_cnt, d_cnt2, d_scnt, d_ovf, d_spill, d_ctr, d_tmp, d_tmp2);
		add(d_mem_off, d_seed_off, d_seed_of_mem, d_mems, d_salcnt, d_seeds, d_fqA, d_fqB, d_fqR, d_sst2, d_bq, d_lep, d_ovfrec);
		add(d_okey, d_oidx, d_okey2, d_oidx2, d_okey64, d_okey64b, d_sctr, d_evc);
		return b;
	}
};

// One result of a pass outside the pass contexts: the batch cs_engine_collect_device handed out last lives here (pipelines.hip).
struct ResultSet {
	DevBuf<uint64_t> mem_off, seed_off; DevBuf<OutMem> mems; DevBuf<OutSeed> seeds;
	uint64_t device_bytes() const { return (uint64_t)mem_off.cap * 8 + (uint64_t)seed_off.cap * 8 + (uint64_t)mems.cap * sizeof(OutMem) + (uint64_t)seeds.cap * sizeof(OutSeed); }
	bool empty() const { return !mem_off.p && !seed_off.p && !mems.p && !seeds.p; }
	void release() { mem_off.release(); seed_off.release(); mems.release(); seeds.release(); }
};

constexpr int PIPE_DEPTH = 4; // batches in flight in the host pipeline (cs_engine_submit): one pinned result slot each
// the two pipelines and everything only they use are private to pipelines.hip
struct HostPipe; struct DevPipe;
struct PipeDelete { void operator()(HostPipe *) const; void operator()(DevPipe *) const; };
struct cs_engine {
	int device = 0;
	int n_cu = 256;
	cs_engine_options_t opt{};
	int smem_mode = 1;          // 1 = split kernels (default), 0 = fused one-lane-per-read kernel (engine option `fused`)
	int occ_win = 5; // ... of bwd_win_kernel
	int occ_fwd = 4, occ_bwd = 4; // resident 256-thread blocks per CU of fwd_kernel / bwd_kernel
	size_t lep_arena_bytes = (size_t)32 << 30;
	uint32_t cap = 64;          // mems per read kept by the first pass
	size_t max_raw_bytes = (size_t)24 << 30;
	DevIndex ix{};
	DevBuf<uint4> d_bwt; DevBuf<uint64_t> d_sa;
	DevBuf<uint32_t> d_fsa32; DevBuf<uint64_t> d_fsa64; DevBuf<uint4> d_fsa40; // full suffix array (one of the three; d_fsa40: engine option sa40, fm_device.hpp Pack40)
	DevBuf<uint32_t> d_text2, d_isa32; DevBuf<uint64_t> d_isa64; DevBuf<uint4> d_isa40; // text mode: 2-bit text + inverse suffix array
	DevBuf<uint8_t> d_lcp, d_rep; // re-seeding from the text: capped LCP by row, repeat length by position
	DevBuf<uint4> d_jump; int jump_k = 0; // round-3 jump table
	// k-mer filter of the text for the min_seed_len in use: passes hold filter_rw shared; rebuilding it for another min_seed_len
	// (run_pass) takes it exclusively
	DevBuf<uint64_t> d_bloom; int bloom_k = 0; uint32_t bloom_bits = 0;
	std::shared_mutex filter_rw;
	int bloom_tried_k = 0;                         // last min_seed_len the filter was (re)built or found not to fit for
	std::unique_ptr<PassCtx> ctx[2];               // the second one is made on the first call that can use two passes at a time
	PassCtx *last_ctx = nullptr;                   // which context holds the last whole-batch result (`last` lives in that one)
	ResultSet held;                                // the device batch collected last (cs_engine_collect_device swaps it out of its context)
	bool last_in_held = false;                     // the last result's arrays are `held`'s, not last_ctx's (its counts and streams still are)
	// cs_engine_memory reads these and nothing a running pass writes: bytes of each pass context as of the end of its last pass (0: no
	// such context), of `held` as of the last cs_engine_collect_device (reported within pass_ctx[0]), and of the k-mer filter
	std::atomic<uint64_t> ctx_bytes[2] = {{0}, {0}}, held_bytes{0}, bloom_bytes{0};
	std::unique_ptr<HostPipe, PipeDelete> hp;      // host variants: copy streams, slots, threads, expanded results (made by engine_init)
	std::unique_ptr<DevPipe, PipeDelete> dp;       // cs_engine_submit_device / cs_engine_collect_device (made by the first submit)
	// cs_engine_gather_reads
	DevBuf<uint64_t> d_sel, d_sel_moff, d_sel_soff; DevBuf<OutMem> d_sel_mems; DevBuf<OutSeed> d_sel_seeds;
	PinBuf<uint64_t> h_mem_off, h_seed_off; PinBuf<OutMem> h_mems; PinBuf<OutSeed> h_seeds;
};

// cs_params_t.result_flags / reserved, checked by every seed entry point before it touches the device
inline bool result_flags_ok(const cs_params_t *par) { return (par->result_flags & ~CS_RESULT_LEAN) == 0 && par->reserved == 0; }
inline bool lean_results(const cs_params_t *par) { return (par->result_flags & CS_RESULT_LEAN) != 0; }
inline int n_pass_ctx(const cs_engine *e) { return e->ctx[1] ? 2 : 1; }
inline void note_ctx_bytes(cs_engine *e, const PassCtx *c) { e->ctx_bytes[c->id].store(c->device_bytes(), std::memory_order_relaxed); }
inline void invalidate_last(cs_engine *e) { for (auto &c : e->ctx) if (c) c->last.valid = false; e->last_ctx = nullptr; e->last_in_held = false; }
// the arrays of the last whole-batch result, whose counts are c->last (c = e->last_ctx): c's own, or the set a device collect handed out
struct LastArrays { const uint64_t *mem_off, *seed_off; const OutMem *mems; const OutSeed *seeds; };
inline LastArrays last_arrays(const cs_engine *e, const PassCtx *c)
{
	if (e->last_in_held) return {e->held.mem_off.p, e->held.seed_off.p, e->held.mems.p, e->held.seeds.p};
	return {c->d_mem_off.p, c->d_seed_off.p, c->d_mems.p, c->d_seeds.p};
}
// A blocking seed call or a host batch, which need the device stream drained, end the validity of every collected device result: the
// spare set's memory goes back (an engine that streams device batches gets it again at its next collect, by the swap).  Only a device
// collect fills `held`, so a non-empty set means no host batch has been submitted since, and no other thread is in the engine.
inline void drop_held(cs_engine *e)
{
	if (e->held.empty()) return;
	if (e->last_in_held) invalidate_last(e);
	e->held.release();
	e->held_bytes.store(0, std::memory_order_relaxed);
}

// seed_pass.hip
int add_pass_ctx(cs_engine *e);   // makes the engine's next pass context (the first at engine creation)
int seed_pass_init(cs_engine *e); // occupancy of the split kernels, the k-mer filter for the default min_seed_len
// One seeding pass on context c; every caller runs its passes through here.  d_recs: the reads as pack_reads_kernel's records when
// the host made them (d_bases is then null), else null.
int run_pass(cs_engine *e, PassCtx *c, const cs_params_t *par, int64_t n_reads, const uint8_t *d_bases, const uint64_t *d_off,
             uint64_t n_bases, uint64_t *nm, uint64_t *ns, const uint4 *d_recs);
// pipelines.hip
int host_pipe_create(cs_engine *e);   // the copy streams and events of the host pipeline; its buffers grow on first use, its threads start on the first submit
void pipes_stop(cs_engine *e);        // stops and joins the threads of both pipelines
void host_pipe_drain(cs_engine *e);   // waits for the two copy streams
bool pipe_busy(const cs_engine *e);
