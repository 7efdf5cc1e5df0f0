// smem_common.hpp -- the SMEM collection as a forward kernel and wavefront-cooperative backward kernels (gfx950).
//
// Same result as smem_kernel (seed_kernels.hpp) and as the reference's three rounds (mapping/bwamem.c:218-272 ==
// mapping/comp_seed.cpp:2262-2301), organised around what the hardware is good at.  Measured on MI355X the fused
// one-lane-per-read state machine is bound by instruction issue and by the one-chain-per-lane latency, not by HBM
// (a bare dependent chain of random 64-byte reads runs at 57 G lines/s, 3.6 TB/s; the fused kernel reached 35 % of
// that), and 54 % of all bwt_extend calls belong to backward sweeps that extend ~9 independent intervals per step.
//
//   fwd_kernel   one LANE per task: the forward pass of one SMEM call (bwt.c:300-320), or the whole round-3 chain of a
//                read when round 3 runs on the index only.  Starts from the k-mer jump table, leaves the index for the
//                2-bit text once the match is unique, finishes calls whose sweep is trivial or can be read off the text.
//   bwd_win0_kernel / bwd_win_kernel / bwd_wide_kernel   the backward sweeps under the window scheme (default): short match
//                ends are settled through the jump table, stored LEPs walk on one clock per call; in bwd_win_kernel a call takes the
//                18 + n lanes it needs, any free ones of its wave (lane_sets.hpp).
//   bwd_all_kernel   the literal sweep (bwt.c:325-345), a GROUP of G lanes (16/32/64) per call; lane g holds LEP n-1-g in
//                registers; every step extends ALL live intervals at once and the reference's sequential keep/emit rules
//                are evaluated with a ballot and one shuffle: occurrence counts are monotone along the list (a longer
//                match cannot occur more often), so the intervals that stop form a prefix, only the first of them can be
//                a new SMEM, and "differs from the last kept size" is a comparison with the previous surviving lane.
//   r2text_kernel / r3text_kernel   re-seeding calls and round-3 seeds answered from the text-side arrays.
//   (DESIGN.md section 4.2 states each shortcut and why it is exact.)
//
// Calls are chained through task queues in HBM: a finished backward sweep of round 1 enqueues the forward pass at the
// next pivot (bwamem.c:226-236), and every emitted round-1 SMEM that is long and rare enough enqueues its re-seeding
// call (bwamem.c:241-249) -- those depend only on that one SMEM, so all of them run in parallel.  The host alternates
// fwd / bwd launches until the queues are empty.  Mems of a read are appended with one atomic per mem and sorted
// afterwards (comp_seed.cpp:2301), so the order in which tasks finish is irrelevant to the output.
//
// The kernels by family, all compiled into seed_pass.hip: smem_reads.hpp (the reads as 32-base records), smem_fwd.hpp (forward
// passes), smem_bwd.hpp (backward sweeps), smem_text.hpp (re-seeding and round 3 from the text, the k-mer filter's fill) and
// smem_sort.hpp (per-read sort and compaction).  This header holds what they share: tasks, SplitArgs, the emit functions, the LDS
// SST, the reader over the packed reads, the wave dispensers and the k-mer filter's lookup.
#pragma once
#include "fm_device.hpp"

namespace csd {

enum : uint32_t { TK_ROUND1 = 0, TK_ROUND2 = 1, TK_ROUND3 = 2, TK_NOP = 3, TK_TEXT = 4 /* fwd_kernel-internal: a round-1 call in text mode */ };

// window scheme (bwd_win_run): ranks 0..WIN_LANES-1 of a call's lane set hold the short matches, the rest hold LEPs; the size classes
// 4 (up to WIN_G32_LEPS stored LEPs) and 5 (up to WIN_G64_LEPS: 64 lanes) are both bwd_win_kernel's
constexpr int WIN_LANES = 18, WIN_G32_LEPS = 32 - WIN_LANES, WIN_G64_LEPS = 64 - WIN_LANES;

// forward task, 8 bytes: read | pivot | min_intv | kind
__device__ __host__ __forceinline__ uint64_t ftask_pack(uint32_t r, uint32_t x, uint32_t min_intv, uint32_t kind)
{
	return (uint64_t)r | (uint64_t)x << 32 | (uint64_t)min_intv << 48 | (uint64_t)kind << 62;
}

struct SplitArgs {
	DevIndex ix;
	const uint8_t  *seq;                              // (no reader in these kernels; kept with sst2: DESIGN.md section 4.3)
	const uint4    *seqp;                             // the reads as 16-byte records of 32 bases (pack_reads_kernel), already offset to this launch's first read
	const uint64_t *off;
	int64_t   n_reads;
	OutMem   *out; uint32_t *out_cnt; uint32_t cap;
	uint32_t *out_scnt; uint32_t max_occ;             // SA slots per read, sum of min(x2, max_occ) over its mems, counted as they are emitted (null: not wanted)
	OvfRec   *ovf; unsigned long long *ovf_cnt; uint64_t ovf_cap;
	int32_t   min_seed_len, split_len;
	uint32_t  split_width;
	uint64_t  max_mem_intv;
	const uint64_t *fq; uint64_t n_f;                 // forward tasks of this launch
	uint64_t *fq_next; unsigned long long *n_f_next; uint64_t fq_cap;
	unsigned long long *n_text_sweeps;                // backward sweeps answered from the text (fwd_kernel)
	unsigned long long *n_r2_quick;                   // re-seeding calls settled by fwd0_kernel itself (counted with r2text_kernel's)
	const uint64_t *bloom; uint32_t bloom_bits;       // k-mer filter of the text for k = min_seed_len (kmer_filter_*), or null
	int32_t   win;                                    // window scheme for the backward sweeps (bwd_win_run) is on
	int32_t   text_sweep;                             // bit 0 (TS_SWEEP): that shortcut is enabled (CS_DISABLE_TEXT_SWEEP off); bit 1 (TS_MEM_POS): unique mems
	                                                  // and re-seeding side words carry the text position (CS_DISABLE_MEM_POS off).  One field: DESIGN.md 4.3
	unsigned long long *n_btasks;                     // backward calls created by this forward launch (0: the backward kernels return at once)
	uint64_t *aux_next;                               // side word of fq_next[slot] for re-seeding calls (r2text_kernel), or null
	BTask    *bq;                                     // backward task of forward task t: bq[t] (no atomics: 1:1)
	uint4    *lep; uint32_t lep_stride;               // LEP list of forward task t: lep + t*lep_stride
	unsigned long long *task_ctr;
	unsigned long long *n_queries;
	unsigned long long *err;                          // sticky: a queue overflowed
	unsigned long long *n_sst_hits;                   // bwt_extend queries answered by the on-device SST
	int32_t   sst;                                    // cs_params_t.sst_mode
	uint4    *sst2;                                   // second SST level (global, SST2_ENTRIES)
	const uint4 *jump; int32_t jump_k;                // round-3 jump table: bi-interval of every jump_k-mer (or null)
	unsigned long long *evc;                          // byte-model event counters [N_KID][N_EV] (fm_device.hpp), or null
};

constexpr int32_t TS_SWEEP = 1, TS_MEM_POS = 2; // SplitArgs::text_sweep
constexpr uint64_t FTASK_NONE = ~0ull; // kind bits = TK_NOP
constexpr uint64_t AUX_NONE = ~0ull, POS_NONE = ~0ull;
// side word of a re-seeding call (emit_smem): bit 54 set = bits 0..36 hold the SMEM's text position, not its x0
constexpr uint64_t AUX_POS = 1ull << 54, AUX_LOW = (1ull << 37) - 1ull;
// Appends a mem to read r's raw list.  pos: the text position of the mem's first base where the caller holds it (it must be SA[v.x0]
// exactly), else POS_NONE.  A unique mem with a position is stored tagged (fm_device.hpp, MEM_POS_TAG): the sort and r3text_kernel then take
// P from the record instead of reading the suffix array again.  The slot count is that of x2 = 1 either way.
__device__ __forceinline__ void emit_mem(const SplitArgs &A, uint32_t r, const Intv &v, uint32_t beg, uint32_t end, uint64_t pos = POS_NONE)
{
	OutMem m = {v.x0, v.x1, v.x2, (uint64_t)beg << 32 | end};
	if (v.x2 == 1 && pos != POS_NONE && (A.text_sweep & TS_MEM_POS)) m.x2 = MEM_POS_TAG | pos;
	uint32_t k = atomicAdd(&A.out_cnt[r], 1u);
	if (A.out_scnt) atomicAdd(&A.out_scnt[r], sal_slots(v.x2, A.max_occ)); // (nothing waits for it: no return value)
	if (k < A.cap) A.out[(size_t)r * A.cap + k] = m;
	else {
		unsigned long long s = atomicAdd(A.ovf_cnt, 1ull);
		if (s < A.ovf_cap) { OvfRec o = {m, r, 0}; A.ovf[s] = o; } else atomicMax(A.err, 1ull);
	}
}
__device__ __forceinline__ void push_ftask(const SplitArgs &A, uint64_t t, uint64_t aux = ~0ull) // one atomic per task: rare paths only
{
	unsigned long long s = atomicAdd(A.n_f_next, 1ull);
	if (s < A.fq_cap) { A.fq_next[s] = t; if (aux != ~0ull) A.aux_next[s] = aux; } else atomicMax(A.err, 2ull);
}
// an SMEM of a round-1/2 call: length filter (bwamem.c:232,246); returns the re-seeding call a round-1 SMEM triggers
// (bwamem.c:241-249) or FTASK_NONE.  aux: for the re-seeding call of a UNIQUE SMEM (min_intv 2), what r2text_kernel needs
// to find the SMEM in the text: x0 | beg << 37 | parity(beg + end) << 53 -- or, where the caller holds the SMEM's text position
// (pos, as for emit_mem), that position in the place of x0 and AUX_POS set: r2text_kernel then starts without its suffix-array read.
// (Bits 55..63 stay clear, so no side word equals AUX_NONE.)
__device__ __forceinline__ uint64_t emit_smem(const SplitArgs &A, uint32_t r, uint32_t kind, const Intv &v, int beg, uint32_t end, uint64_t &aux, uint64_t pos = POS_NONE)
{
	int len = (int)end - beg;
	aux = AUX_NONE;
	if (len < A.min_seed_len) return FTASK_NONE;
	emit_mem(A, r, v, (uint32_t)beg, end, pos);
	if (kind == TK_ROUND1 && len >= A.split_len && v.x2 <= A.split_width) {
		if (v.x2 == 1 && A.aux_next) {
			const bool have = pos != POS_NONE && (A.text_sweep & TS_MEM_POS);
			aux = (have ? pos | AUX_POS : v.x0) | (uint64_t)beg << 37 | (uint64_t)(((uint32_t)beg + end) & 1u) << 53;
		}
		return ftask_pack(r, (uint32_t)(beg + (int)end) >> 1, (uint32_t)v.x2 + 1, TK_ROUND2);
	}
	return FTASK_NONE;
}

// ------------------------------------------------------------------------------------------------------------------
// On-device SST (mapping/SST.h on the CPU): a transparent memo of bwt_extend, resident in LDS.
//
// The CPU SST is two tries (forward / backward) of bi-intervals keyed by the path of bases, reset every 512 reads.  A
// bi-interval is a function of the STRING alone, whichever direction it was reached from, so on the device one table
// keyed by the string serves both directions: entry (len, code) holds the interval of the string whose 2-bit packed
// bases are `code`.  It covers every string of up to SST_K bases (sum 4^d = 1364 entries x 16 B = 21.8 KB per
// workgroup, so occupancy is untouched), starts empty in every workgroup and is filled lazily: a miss costs exactly the
// bwt_extend it would have cost anyway and publishes the child; a hit answers from LDS with no HBM/L2 round trip.  Racing
// writers store identical values (the memoised function is pure), entries are single 16-byte LDS accesses.  Deeper
// strings are not cached: beyond ~12 bases every extension is a distinct random line whether a trie node or an Occ
// block answers it, so only an LDS-resident level set saves anything.
constexpr int SST_K = 5;
constexpr int SST_ENTRIES = 4 + 16 + 64 + 256 + 1024;
// Optional second level: strings of SST_K+1 .. SST2_K bases in a table in global memory (L2-resident, persistent across
// launches).  MEASURED AND SWITCHED OFF (SST2_K == SST_K): with SST2_K = 8 (1.4 MB) the hit rate rose from 8.8 % to
// 18.8 % on the bench workload but the SMEM stage got 10 % SLOWER (224 vs 204 ms per 10 M reads) -- the Occ records of
// such short strings are L2 hits already, so a hit only trades two record reads for one table read plus divergence.
// Only a level that answers without leaving the CU (LDS) pays.  The code path is kept for the record.
#ifndef CS_SST2_K
#define CS_SST2_K 5
#endif
constexpr int SST2_K = CS_SST2_K;
constexpr int SST2_ENTRIES = SST2_K > SST_K ? ((1 << (2 * (SST2_K + 1))) - 4096) / 3 : 16;
__device__ __forceinline__ int sst2_index(int len, uint32_t code) { return ((1 << (2 * len)) - 4096) / 3 + (int)code; } // len in 6..8
__device__ __forceinline__ int sst_index(int len, uint32_t code) // len in 1..SST_K
{
	return ((1 << (2 * len)) - 4) / 3 + (int)code; // 4 + 16 + ... + 4^(len-1) entries precede length `len`
}
__device__ __forceinline__ void sst_clear(uint4 *sst)
{
	for (int t = threadIdx.x; t < SST_ENTRIES; t += blockDim.x) sst[t] = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
	__syncthreads();
}
__device__ __forceinline__ bool sst_get(const uint4 *sst, uint4 *sst2, int len, uint32_t code, Intv &v)
{
	uint4 e = len <= SST_K ? sst[sst_index(len, code)] : sst2[sst2_index(len, code)];
	if (e.w == 0xffffffffu) return false; // empty: a stored entry keeps its top 16 bits (the unused query end) zero
	uint32_t end; unpack_lep(e, v, end);
	return true;
}
__device__ __forceinline__ void sst_put(uint4 *sst, uint4 *sst2, int len, uint32_t code, const Intv &v)
{
	if (len <= SST_K) sst[sst_index(len, code)] = pack_lep(v, 0); else sst2[sst2_index(len, code)] = pack_lep(v, 0);
}


// The reads as pack_reads_kernel's records (smem_reads.hpp): one 16-byte record per 32 bases, record k of read r at rec[(off[r] >> 5) + r + k].
// Reader over those records: any position of the read, one load per record entered
struct PackedReader {
	const uint4 *rec; uint64_t bases; uint32_t bad; int wk;
	__device__ __forceinline__ void load() { const uint4 v = rec[wk]; bases = (uint64_t)v.x | (uint64_t)v.y << 32; bad = v.z; }
	__device__ __forceinline__ void start(const uint4 *recs, uint64_t rb, uint32_t r, int pos)
	{
		rec = recs + (rb >> 5) + r; wk = (pos < 0 ? 0 : pos) >> 5; load();
	}
	__device__ __forceinline__ void seek(int pos) { if ((pos >> 5) != wk) { wk = pos >> 5; load(); } }
	__device__ __forceinline__ uint32_t at(int pos) // 0..3, or 4: ambiguous base / behind the end (pos <= len)
	{
		seek(pos);
		const uint32_t j = (uint32_t)pos & 31u;
		return (bad >> j) & 1u ? 4u : (uint32_t)(bases >> (j << 1)) & 3u;
	}
	// the 32 bases from pos on (2 bits each, the first least significant) and their ambiguity bits; the nb (<= 32) first of them must
	// lie inside the read.  The reader stays on the record of pos.
	__device__ __forceinline__ uint64_t window(int pos, int nb, uint32_t &badw)
	{
		seek(pos);
		const uint32_t j = (uint32_t)pos & 31u;
		uint64_t w = bases >> (j << 1); badw = bad >> j;
		if (j + (uint32_t)nb > 32u) { const uint4 v = rec[wk + 1]; w |= ((uint64_t)v.x | (uint64_t)v.y << 32) << ((32u - j) << 1); badw |= v.z << (32u - j); }
		return w;
	}
	// the jk (<= 16) bases from pos on as a jump-table code (first base most significant); pos + jk <= len
	__device__ __forceinline__ uint32_t kmer(int pos, int jk, uint32_t &badk)
	{
		seek(pos);
		const uint32_t j = (uint32_t)pos & 31u;
		uint64_t w = bases >> (j << 1); uint32_t bd = bad >> j;
		if (j + (uint32_t)jk > 32u) { // j >= 17: the code runs into the next record (left loaded: the caller goes on from there)
			++wk; load();
			w |= bases << ((32u - j) << 1); bd |= bad << (32u - j);
		}
		badk = (bd & ((1u << jk) - 1u)) ? 4u : 0u;
		uint32_t rv = __brev((uint32_t)w);                           // group q at 2(15-q), its two bits swapped
		rv = ((rv & 0xAAAAAAAAu) >> 1) | ((rv & 0x55555555u) << 1);
		return rv >> (32 - 2 * jk);
	}
};
// text mode: up to 32 read bases from i against the text from tpos (<= seq_len); true when the match ends here.  Counts what the
// reference would have performed: one bwt_extend per base that is compared (the last one, at a mismatch or the text's end, returns
// size 0); none at an ambiguous base or the read's end (bwt.c:309-316).
template <class WC>
__device__ __forceinline__ bool text_step(const DevIndex &ix, PackedReader &rd, int &i, uint64_t &tpos, uint32_t &my_q, uint32_t &my_hits, WC &W)
{
	rd.seek(i);
	const uint32_t j = (uint32_t)i & 31u, avail = 32u - j;
	const uint64_t x = (rd.bases >> (j << 1)) ^ text_win(ix, tpos); wc_add(W, EV_TEXT, 4u);
	const uint64_t d = (x | x >> 1) & 0x5555555555555555ull;
	uint32_t m = d ? (uint32_t)(__ffsll((long long)d) - 1) >> 1 : 32u;   // first base that differs
	const uint64_t room = ix.seq_len - tpos;
	if (room < m) m = (uint32_t)room;                                    // ... or has no text base to agree with
	const uint32_t bb = rd.bad >> j, m_bad = bb ? (uint32_t)__ffs((int)bb) - 1u : 32u;
	uint32_t n = m < m_bad ? m : m_bad;
	if (n > avail) n = avail;
	i += (int)n; tpos += n; my_q += n; my_hits += n;
	if (n == avail) return false;                                        // the record is used up: on with the next one
	if (n != m_bad) { ++my_q; ++my_hits; }
	return true;
}

// Task dispenser.  One returning atomic on a single word costs ~11 ns and the word saturates near 88 M dequeues/s
// (MI355X_MICROARCH.md "dequeue"), far below the millions of short tasks per launch here, so a wave draws REFILL task
// ids at a time with ONE atomic and hands them to its lanes with a ballot + popcount.  All state is wave-uniform.
struct WavePool { uint64_t cur, end; bool exhausted; };

template <int REFILL>
__device__ __forceinline__ bool pool_take(WavePool &P, bool want, unsigned long long *ctr, uint64_t n_tasks, uint64_t &task)
{
	const uint32_t lane = threadIdx.x & 63u;
	uint64_t m = __ballot(want);
	if (m == 0) return false;
	if (P.cur == P.end && !P.exhausted) {
		int src = __ffsll((long long)m) - 1;
		unsigned long long base = 0;
		if ((int)lane == src) base = atomicAdd(ctr, (unsigned long long)REFILL);
		base = __shfl(base, src);
		if (base >= n_tasks) P.exhausted = true;
		else { P.cur = base; P.end = base + REFILL < n_tasks ? base + REFILL : n_tasks; }
	}
	uint64_t avail = P.end - P.cur, cnt = (uint64_t)__popcll(m);
	uint64_t rank = (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
	task = P.cur + rank;
	P.cur += cnt < avail ? cnt : avail;
	return want && rank < avail;
}

// The reverse direction: a wave reserves RES slots of the next forward queue with one atomic and its lanes fill them
// (ballot + popcount); slots left over when the wave moves on are filled with no-op tasks.
struct WaveOut { uint64_t cur, end; };
template <int RES>
__device__ __forceinline__ void wave_push(WaveOut &O, bool want, uint64_t task, const SplitArgs &A, uint64_t aux = AUX_NONE)
{
	const uint32_t lane = threadIdx.x & 63u;
	uint64_t m = __ballot(want);
	if (m == 0) return;
	uint64_t cnt = (uint64_t)__popcll(m);
	if (O.end - O.cur < cnt) {
		uint64_t rem = O.end - O.cur;
		if (lane < rem) A.fq_next[O.cur + lane] = FTASK_NONE;
		int src = __ffsll((long long)m) - 1;
		unsigned long long base = 0;
		if ((int)lane == src) base = atomicAdd(A.n_f_next, (unsigned long long)RES);
		base = __shfl(base, src);
		if (base + RES > A.fq_cap) { if ((int)lane == src) atomicMax(A.err, 2ull); O.cur = O.end = 0; return; }
		O.cur = base; O.end = base + RES;
	}
	uint64_t rank = (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
	if (want) { A.fq_next[O.cur + rank] = task; if (aux != AUX_NONE) A.aux_next[O.cur + rank] = aux; }
	O.cur += cnt;
}
__device__ __forceinline__ void wave_push_finish(WaveOut &O, const SplitArgs &A)
{
	const uint32_t lane = threadIdx.x & 63u;
	uint64_t rem = O.end - O.cur;
	if (lane < rem) A.fq_next[O.cur + lane] = FTASK_NONE;
	O.cur = O.end;
}

// ------------------------------------------------------------------------------------------------------------------
// A filter over ALL min_seed_len-mers of the text (both strands: the text holds both): 2^bloom_bits 64-bit words, two bits
// per k-mer inside one word chosen by a hash.  "Both bits set" has ~1 % false positives, "not both" is exact: that k-mer
// does not occur.  The window lanes of the backward kernels ask it before anything else -- a chance window exists with
// probability 2 %, so 97 % of them end after one 8-byte read instead of a jump-table read and two to four extensions.
// Codes are 2 bits per base, first base least significant (the order of the 2-bit text), k <= 32.
__device__ __forceinline__ uint64_t kmer_hash(uint64_t code) { uint64_t h = code * 0x9E3779B97F4A7C15ull; return h ^ (h >> 29); }
__device__ __forceinline__ bool kmer_filter_has(const uint64_t *bloom, uint32_t bits, uint64_t code)
{
	const uint64_t h = kmer_hash(code);
	const uint64_t w = bloom[h >> (64u - bits)];
	return ((w >> (h & 63u)) & (w >> ((h >> 6) & 63u)) & 1ull) != 0;
}
// The re-seeding call of a unique SMEM, the part most calls come to: in sequence that is not repeated, rep[] stays
// below min_seed_len around the pivot.  If it does at all the min_seed_len offsets up to the pivot (and is never 0), the sweep of
// r2_by_text ends within them (o + rep[o] <= pivot at the latest at o = pivot - min_seed_len + 1), touches neither end of the SMEM and
// reports nothing: the call is answered by three or four words of rep[].  0: answered; 1: needs the sweep.  P: text position of the
// SMEM's first base, len its length, po the pivot's offset in it; nw: words read.
__device__ __forceinline__ int r2_quick_rep(const DevIndex &ix, uint64_t P, int len, int po, int k, uint32_t &nw)
{
	nw = 0;
	if (po < k || po + k > len || k > 32) return 1;
	const uint64_t lo = P + (uint64_t)(po - k + 1), hi = P + (uint64_t)po;   // the bytes rep[lo .. hi]
	const uint64_t *wp = reinterpret_cast<const uint64_t *>(ix.rep) + (lo >> 3);
	nw = (uint32_t)((hi >> 3) - (lo >> 3)) + 1u;                               // 3..5 aligned words for k <= 32
	uint64_t wd[5];
#pragma unroll
	for (int q = 0; q < 5; ++q) wd[q] = (uint32_t)q < nw ? wp[q] : 0x0101010101010101ull;
	const uint64_t ones = 0x0101010101010101ull, top = 0x8080808080808080ull;
	const uint64_t fl = ((lo & 7) ? ~0ull << ((lo & 7) << 3) : ~0ull), fh = ~0ull >> ((7 - (hi & 7)) << 3); // bytes of the first / last word that count
	uint64_t bad = 0;
#pragma unroll
	for (int q = 0; q < 5; ++q) {
		const uint64_t w = wd[q];
		uint64_t f = ((((w & ~top) + (uint64_t)(0x80 - k) * ones) | w) & top)    // a byte >= k
		           | ((w - ones) & ~w & top);                                    // a byte == 0
		if (q == 0) f &= fl;
		if ((uint32_t)q + 1u == nw) f &= fh;
		if ((uint32_t)q < nw) bad |= f;
	}
	return bad ? 1 : 0;
}
// the call that follows a finished round-1 call at pivot x_cur: next pivot = end of the longest forward match, ambiguous
// bases skipped.  A round-1 task carries, in the field that holds min_intv for round 2 (round 1 always uses 1), the
// distance to the previous pivot + 1 when the forward pass ended ON the new pivot (no ambiguous base in between): no
// match that starts at or before the previous pivot reaches beyond the new one, which bounds the new call's sweep.
__device__ __forceinline__ uint64_t chain_round1(PackedReader &rd, uint32_t r, int len, int ret, int x_cur)
{
	int x = ret;
	while (x < len && rd.at(x) > 3) ++x;
	uint32_t d = (x == ret && ret - x_cur < 16382) ? (uint32_t)(ret - x_cur) : 0u;
	return x < len ? ftask_pack(r, (uint32_t)x, 1u + d, TK_ROUND1) : FTASK_NONE;
}

} // namespace csd
