// smem_sort.hpp -- what follows the SMEM stage of the split path: the per-read sort by info and the compaction into the CSR result,
// and the kernels that expand the mems into seeds in the same pass (sort_expand16_kernel, sal_expand_heavy_kernel).
#pragma once
#include "fm_device.hpp"
#include "seed_kernels.hpp" // SAL_LIGHT

namespace csd {

// per-read sort by info (comp_seed.cpp:2301) + CSR compaction; a read's mems beyond `cap` come from the overflow
// records, which have been sorted by read id
__device__ __forceinline__ const OutMem &mem_at(const OutMem *src, uint32_t cap, const OvfRec *ovf, const uint32_t *ovf_idx, uint64_t olo, uint32_t a)
{
	return a < cap ? src[a] : ovf[ovf_idx[olo + (a - cap)]].m;
}
// The reads sort_compact16_kernel leaves out (more than 64 mems, or mems beyond `cap`: tandem arrays, repeats): one WAVE per
// read.  A wave owns 64 consecutive reads, finds the heavy ones by ballot and rank-sorts each with all 64 lanes: lane j
// owns mems j, j+64, ...; the keys of 64 mems at a time sit in registers and travel by shuffle.  (One lane per read made
// this kernel as slow as its slowest read: 5 ms for a handful of reads with hundreds of mems.)
// LEAN (here and in the two kernels below; CS_RESULT_LEAN): the sorted mems are stored with x1 = 0.  A template parameter, not an
// argument: the <false> instantiations are the kernels as they were.
template <bool LEAN>
__global__ __launch_bounds__(256) void sort_compact_wave_kernel(const OutMem *raw, const uint32_t *cnt, uint32_t cap, const OvfRec *ovf, const uint32_t *ovf_key,
                                                                const uint32_t *ovf_idx, uint64_t n_ovf, const uint64_t *mem_off, int64_t n_reads, OutMem *mems,
                                                                uint64_t *salcnt, uint32_t max_occ)
{
	const uint32_t lane = threadIdx.x & 63u;
	const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const int64_t r0 = w * 64 + lane;
	const uint32_t n_mine = r0 < n_reads ? cnt[r0] : 0;
	uint64_t heavy = __ballot(n_mine > 64 || n_mine > cap);
	while (heavy) {
		const int hs = __ffsll((long long)heavy) - 1; heavy &= heavy - 1;
		const int64_t r = w * 64 + hs; const uint32_t n = __shfl(n_mine, hs);
		const OutMem *src = raw + (size_t)r * cap;
		OutMem *dst = mems + mem_off[r];
		uint64_t olo = 0;
		if (n > cap) { // lower bound of r among the sorted overflow keys
			uint64_t lo = 0, hi = n_ovf;
			while (lo < hi) { uint64_t mid = (lo + hi) >> 1; if (ovf_key[mid] < (uint32_t)r) lo = mid + 1; else hi = mid; }
			olo = lo;
		}
		for (uint32_t a0 = 0; a0 < n; a0 += 64) {
			const uint32_t a = a0 + lane;
			OutMem ma = {0, 0, 0, ~0ull};
			if (a < n) { ma = mem_at(src, cap, ovf, ovf_idx, olo, a); ma.x2 = mem_x2(ma.x2); } // (a raw record may be tagged: fm_device.hpp)
			uint32_t rank = 0;
			for (uint32_t b0 = 0; b0 < n; b0 += 64) {
				const uint32_t b = b0 + lane;
				const uint64_t kb = b < n ? mem_at(src, cap, ovf, ovf_idx, olo, b).info : ~0ull; // padding keys are never smaller
				for (int j = 0; j < 64; ++j) {
					const uint64_t kj = __shfl(kb, j);
					rank += (kj < ma.info) || (kj == ma.info && b0 + (uint32_t)j < a);
				}
			}
			if (LEAN) ma.x1 = 0;
			if (a < n) { dst[rank] = ma; if (salcnt) salcnt[mem_off[r] + rank] = ma.x2 < max_occ ? ma.x2 : max_occ; } // (null: sal_expand_heavy_kernel follows)
		}
	}
}

// Fast form of the same for the bulk: 16 lanes per read (4 reads per wave).  Up to 16 mems: lane a owns mem a; 17..64 mems
// (repeat-rich reads): lane a owns mems a, a+16, a+32, a+48.  Each mem is read once (coalesced: 16 lanes x 32 B contiguous),
// keys travel by shuffle, and every lane writes its mems at their ranks.  Reads with more than 64 mems, or whose mems
// spilled beyond `cap`, are left to sort_compact_wave_kernel.
template <bool LEAN>
__global__ __launch_bounds__(256) void sort_compact16_kernel(const OutMem *raw, const uint32_t *cnt, uint32_t cap, const uint64_t *mem_off,
                                                             int64_t n_reads, OutMem *mems, uint64_t *salcnt, uint32_t max_occ)
{
	const uint32_t lane = threadIdx.x & 63u, a = lane & 15u, gbase = lane & ~15u;
	int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
	uint32_t n = r < n_reads ? cnt[r] : 0;
	if (n > 64 || n > cap) n = 0; // not ours
	const OutMem *src = raw + (size_t)(r < n_reads ? r : 0) * cap;
	OutMem m[4]; uint64_t key[4]; uint32_t rank[4] = {0, 0, 0, 0};
#pragma unroll
	for (int s = 0; s < 4; ++s) {
		uint32_t e = a + 16u * s;
		key[s] = ~0ull;
		if (e < n) { m[s] = src[e]; m[s].x2 = mem_x2(m[s].x2); key[s] = m[s].info; } // (a raw record may be tagged: fm_device.hpp)
	}
	const int rounds = n > 48 ? 4 : n > 32 ? 3 : n > 16 ? 2 : 1; // group-uniform
	for (int sb = 0; sb < rounds; ++sb) {
#pragma unroll
		for (int b = 0; b < 16; ++b) {
			uint64_t kb = __shfl(sb == 0 ? key[0] : sb == 1 ? key[1] : sb == 2 ? key[2] : key[3], (int)(gbase + b));
			uint32_t eb = (uint32_t)b + 16u * sb; // index of the mem whose key this is
#pragma unroll
			for (int s = 0; s < 4; ++s) rank[s] += (kb < key[s]) || (kb == key[s] && eb < a + 16u * s);
		}
	}
	if (n) {
		OutMem *dst = mems + mem_off[r]; uint64_t *dsc = salcnt + mem_off[r];
#pragma unroll
		for (int s = 0; s < 4; ++s) if (a + 16u * s < n) { if (LEAN) m[s].x1 = 0; dst[rank[s]] = m[s]; dsc[rank[s]] = m[s].x2 < max_occ ? m[s].x2 : max_occ; }
	}
}

// ------------------------------------------------------------------------------------------------------------------
// Sort and SAL in one pass over the mems.  The SMEM stage has counted every read's SA slots while it emitted the mems
// (SplitArgs::out_scnt), so seed_off[] comes from a scan over the reads, like mem_off[], before any mem is sorted: a mem's seeds can be
// written while the sort still has the mem in registers.  No per-mem slot counts or seed offsets in memory, no scan over the
// mems, no second read of the sorted mems.
//
// One SA slot of a mem into its seed, as sal_expand_kernel<true> writes it.  `end`: where the read's seeds end (seed_off[r + 1]) --
// a read's seeds stay inside its range of the CSR whatever the stage has counted.  (That is memory safety only: the kernels compare the
// slots of a read's sorted mems with the length of its range and raise `bad` when they differ, too few or too many; the host then fails
// the call.)
__device__ __forceinline__ void put_seed(const DevIndex &ix, OutSeed *seeds, uint64_t at, uint64_t end, uint64_t slot, int32_t qb, int32_t ln)
{
	if (at >= end) return;
	OutSeed s = {(int64_t)sa_direct(ix, slot), qb, ln};
	seeds[at] = s;
}
// The seed of a unique mem whose raw record carried its text position (fm_device.hpp, MEM_POS_TAG): the emitting kernel held P = SA[x0], so
// the seed's rbeg is written from the record and the random 8-byte gather above -- what this kernel's time is made of -- does not happen.
__device__ __forceinline__ void put_seed_pos(OutSeed *seeds, uint64_t at, uint64_t end, uint64_t pos, int32_t qb, int32_t ln)
{
	if (at >= end) return;
	OutSeed s = {(int64_t)pos, qb, ln};
	seeds[at] = s;
}

// x / d for x < 2^48 and d <= 2^16, by long division in 16-bit limbs: three 32-bit divisions where the 64-bit one costs the kernels
// below twenty registers.  (An occurrence count is below 2^37: engine creation refuses a longer index; max_occ <= 1024 on this path.)
__device__ __forceinline__ uint64_t div48_16(uint64_t x, uint32_t d)
{
	const uint32_t l2 = (uint32_t)(x >> 32), l1 = (uint32_t)(x >> 16) & 0xffffu, l0 = (uint32_t)x & 0xffffu;
	const uint32_t q2 = l2 / d, t1 = (l2 - q2 * d) << 16 | l1; // (remainder < d <= 2^16: t1 and t0 fit 32 bits, q1 and q0 fit 16)
	const uint32_t q1 = t1 / d, t0 = (t1 - q1 * d) << 16 | l0;
	return (uint64_t)q2 << 32 | (uint64_t)q1 << 16 | (uint64_t)(t0 / d);
}

// sort_compact16_kernel's load and rank phases, then: the mems to their ranks; their slot counts (sal_slots: sal_expand_kernel's `cnt`,
// which is min(x2, max_occ) for either value of `step`) to their ranks in a 64-entry LDS strip per 16-lane group, where lane a sums entries
// 4a .. 4a+3 and a 16-lane shuffle scan makes the exclusive prefix in rank order; every mem expanded at seed_off[r] + prefix with
// sal_expand_kernel's arithmetic.  Up to SAL_LIGHT slots: by the lane that holds the mem; more: by the 16 lanes of the group, 16 slots per step.
// m[s].x2 stays the RAW word from the load to the expansion (fm_device.hpp, MEM_POS_TAG): everything that wants x2 (sal_slots, step, the
// `bad` check through the slot counts, mems[]) sees mem_x2() of it, and a tagged mem's one seed is put_seed_pos, not put_seed.
template <bool LEAN>
__global__ __launch_bounds__(256, 8) void sort_expand16_kernel(const DevIndex ix, const OutMem *raw, const uint32_t *cnt, uint32_t cap, const uint64_t *mem_off,
                                                            const uint64_t *seed_off, int64_t n_reads, OutMem *mems, OutSeed *seeds, uint32_t max_occ, unsigned long long *bad)
{
	__shared__ uint4 strip[16][16]; // [group][lane]: 64 u32 per group
	const uint32_t lane = threadIdx.x & 63u, a = lane & 15u, gbase = lane & ~15u;
	int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
	uint32_t n = r < n_reads ? cnt[r] : 0;
	if (n > 64 || n > cap) n = 0; // not ours
	const OutMem *src = raw + (size_t)(r < n_reads ? r : 0) * cap;
	OutMem m[4]; uint32_t rank[4] = {0, 0, 0, 0}; // (m[s].info is the key: ~0 where the lane has no mem, never smaller than a mem's)
#pragma unroll
	for (int s = 0; s < 4; ++s) {
		uint32_t e = a + 16u * s;
		m[s] = OutMem{0, 0, 0, ~0ull};
		if (e < n) m[s] = src[e];
	}
	const int rounds = n > 48 ? 4 : n > 32 ? 3 : n > 16 ? 2 : 1; // group-uniform
	for (int sb = 0; sb < rounds; ++sb) {
		const uint64_t ksb = sb == 0 ? m[0].info : sb == 1 ? m[1].info : sb == 2 ? m[2].info : m[3].info;
#pragma unroll 4
		for (int b = 0; b < 16; ++b) {
			uint64_t kb = __shfl(ksb, (int)(gbase + b));
			uint32_t eb = (uint32_t)b + 16u * sb; // index of the mem whose key this is
#pragma unroll
			for (int s = 0; s < 4; ++s) rank[s] += (kb < m[s].info) || (kb == m[s].info && eb < a + 16u * s);
		}
	}
	uint32_t *my = reinterpret_cast<uint32_t *>(strip[threadIdx.x >> 4]);
#pragma unroll
	for (int s = 0; s < 4; ++s) if (a + 16u * s < n) my[rank[s]] = sal_slots(mem_x2(m[s].x2), max_occ); // (a read's ranks are a permutation of 0 .. n-1)
	if (n) {
		OutMem *dst = mems + mem_off[r];
#pragma unroll
		for (int s = 0; s < 4; ++s) if (a + 16u * s < n) { OutMem o = m[s]; o.x2 = mem_x2(o.x2); if (LEAN) o.x1 = 0; dst[rank[s]] = o; } // (no tag leaves the sort)
	}
	__syncthreads(); // (every thread of the block gets here: nothing above returns)
	uint32_t total;
	{
		uint4 c4 = strip[threadIdx.x >> 4][a]; // entries at n and beyond hold leftovers: not counted
		if (4u * a + 0u >= n) c4.x = 0;
		if (4u * a + 1u >= n) c4.y = 0;
		if (4u * a + 2u >= n) c4.z = 0;
		if (4u * a + 3u >= n) c4.w = 0;
		const uint32_t sum = c4.x + c4.y + c4.z + c4.w;
		uint32_t inc = sum;
#pragma unroll
		for (int o = 1; o < 16; o <<= 1) { const uint32_t t = __shfl_up(inc, o, 16); if (a >= (uint32_t)o) inc += t; }
		const uint32_t ex = inc - sum; total = inc;
		strip[threadIdx.x >> 4][a] = make_uint4(ex, ex + c4.x, ex + c4.x + c4.y, ex + c4.x + c4.y + c4.z); // (the lane's own four entries)
	}
	__syncthreads();
	const uint64_t sbase = n ? seed_off[r] : 0, send = n ? seed_off[r + 1] : 0;
	if (a == 15u && n && sbase + total != send) atomicMax(bad, 1ull); // (lane 15 holds the sum over the read's mems)
	// One body for the lane's up to four mems, the mem in turn in m[0] (the others move up after each turn): unrolled four times, the
	// expansion of all four would hold its addresses and slots in registers at once.
#pragma unroll 1
	for (int s = 0; s < rounds; ++s) { // group-uniform
		const bool have = a + 16u * s < n;
		const uint64_t x2w = m[0].x2, x2 = mem_x2(x2w); // (m[].x2 holds the raw word through the sort: no register beside it)
		const uint32_t cv = have ? sal_slots(x2, max_occ) : 0;
		const uint64_t step = x2 > max_occ ? div48_16(x2, max_occ) : 1; // comp_seed.cpp:2313-2325: slots x0 + k * step
		const uint64_t first = sbase + (have ? my[rank[0]] : 0u);
		const int32_t qb = (int32_t)(m[0].info >> 32), ln = (int32_t)(uint32_t)m[0].info - qb;
		if (x2w & MEM_POS_TAG) { if (cv) put_seed_pos(seeds, first, send, mem_pos(x2w), qb, ln); } // its one seed, without the gather
		else if (cv <= SAL_LIGHT)
			for (uint32_t c = 0; c < cv; ++c) put_seed(ix, seeds, first + c, send, m[0].x0 + (uint64_t)c * step, qb, ln);
		uint32_t heavy = (uint32_t)(__ballot(cv > SAL_LIGHT) >> gbase) & 0xffffu; // this group's lanes
		while (heavy) { // group-uniform; the shuffles stay inside the group
			const int j = (int)gbase + __builtin_ctz(heavy); heavy &= heavy - 1;
			const uint64_t x0 = __shfl(m[0].x0, j), st = __shfl(step, j), fj = __shfl(first, j);
			const uint32_t cj = __shfl(cv, j);
			const int32_t qbj = __shfl(qb, j), lnj = __shfl(ln, j);
			for (uint32_t c = a; c < cj; c += 16) put_seed(ix, seeds, fj + c, send, x0 + (uint64_t)c * st, qbj, lnj);
		}
#pragma unroll
		for (int t = 0; t < 3; ++t) { m[t].x0 = m[t + 1].x0; m[t].x2 = m[t + 1].x2; m[t].info = m[t + 1].info; rank[t] = rank[t + 1]; }
	}
}

// The seeds of the reads sort_compact_wave_kernel has sorted (found by the same ballot): one wave per read walks the read's sorted mems
// 64 at a time with a running offset that starts at seed_off[r]; inside a chunk a wave scan of the slot counts places every mem, then
// sal_expand_kernel's two cases: up to SAL_LIGHT slots by the mem's lane, more by the whole wave, 64 slots per step.
__global__ __launch_bounds__(256) void sal_expand_heavy_kernel(const DevIndex ix, const uint32_t *cnt, uint32_t cap, const uint64_t *mem_off, const uint64_t *seed_off,
                                                               int64_t n_reads, const OutMem *mems, OutSeed *seeds, uint32_t max_occ, unsigned long long *bad)
{
	const uint32_t lane = threadIdx.x & 63u;
	const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const int64_t r0 = w * 64 + lane;
	const uint32_t n_mine = r0 < n_reads ? cnt[r0] : 0;
	uint64_t todo = __ballot(n_mine > 64 || n_mine > cap);
	while (todo) { // wave-uniform
		const int hs = __ffsll((long long)todo) - 1; todo &= todo - 1;
		const int64_t r = w * 64 + hs; const uint32_t n = __shfl(n_mine, hs);
		const OutMem *src = mems + mem_off[r];
		uint64_t run = seed_off[r]; const uint64_t send = seed_off[r + 1];
		for (uint32_t a0 = 0; a0 < n; a0 += 64) {
			const bool valid = a0 + lane < n;
			const OutMem v = valid ? src[a0 + lane] : OutMem{0, 0, 0, 0};
			const uint32_t cv = valid ? sal_slots(v.x2, max_occ) : 0;
			uint32_t inc = cv; // (64 mems x max_occ <= 1024 slots: far below 2^32)
#pragma unroll
			for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += t; }
			const uint64_t first = run + (inc - cv);
			run += __shfl(inc, 63);
			const uint64_t step = v.x2 > max_occ ? div48_16(v.x2, max_occ) : 1;
			const int32_t qb = (int32_t)(v.info >> 32), ln = (int32_t)(uint32_t)v.info - qb;
			if (cv <= SAL_LIGHT)
				for (uint32_t c = 0; c < cv; ++c) put_seed(ix, seeds, first + c, send, v.x0 + (uint64_t)c * step, qb, ln);
			unsigned long long heavy = __ballot(cv > SAL_LIGHT);
			while (heavy) { // wave-uniform
				const int j = __builtin_ctzll(heavy); heavy &= heavy - 1;
				const uint64_t x0 = __shfl(v.x0, j), st = __shfl(step, j), fj = __shfl(first, j);
				const uint32_t cj = __shfl(cv, j);
				const int32_t qbj = __shfl(qb, j), lnj = __shfl(ln, j);
				for (uint32_t c = lane; c < cj; c += 64) put_seed(ix, seeds, fj + c, send, x0 + (uint64_t)c * st, qbj, lnj);
			}
		}
		if (lane == 0 && run != send) atomicMax(bad, 1ull);
	}
}

__global__ void ovf_keys_kernel(const OvfRec *ovf, uint64_t n, uint32_t *key, uint32_t *idx)
{
	uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) return;
	key[t] = ovf[t].r; idx[t] = (uint32_t)t;
}

} // namespace csd
