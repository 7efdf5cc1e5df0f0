// smem_sort.hpp -- what follows the SMEM stage of the split path: the per-read sort by info and the compaction into the CSR result.
#pragma once
#include "fm_device.hpp"

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
			if (a < n) ma = mem_at(src, cap, ovf, ovf_idx, olo, a);
			uint32_t rank = 0;
			for (uint32_t b0 = 0; b0 < n; b0 += 64) {
				const uint32_t b = b0 + lane;
				const uint64_t kb = b < n ? mem_at(src, cap, ovf, ovf_idx, olo, b).info : ~0ull; // padding keys are never smaller
				for (int j = 0; j < 64; ++j) {
					const uint64_t kj = __shfl(kb, j);
					rank += (kj < ma.info) || (kj == ma.info && b0 + (uint32_t)j < a);
				}
			}
			if (a < n) { dst[rank] = ma; salcnt[mem_off[r] + rank] = ma.x2 < max_occ ? ma.x2 : max_occ; }
		}
	}
}

// Fast form of the same for the bulk: 16 lanes per read (4 reads per wave).  Up to 16 mems: lane a owns mem a; 17..64 mems
// (repeat-rich reads): lane a owns mems a, a+16, a+32, a+48.  Each mem is read once (coalesced: 16 lanes x 32 B contiguous),
// keys travel by shuffle, and every lane writes its mems at their ranks.  Reads with more than 64 mems, or whose mems
// spilled beyond `cap`, are left to sort_compact_wave_kernel.
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
		if (e < n) { m[s] = src[e]; key[s] = m[s].info; }
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
		for (int s = 0; s < 4; ++s) if (a + 16u * s < n) { dst[rank[s]] = m[s]; dsc[rank[s]] = m[s].x2 < max_occ ? m[s].x2 : max_occ; }
	}
}

__global__ void ovf_keys_kernel(const OvfRec *ovf, uint64_t n, uint32_t *key, uint32_t *idx)
{
	uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) return;
	key[t] = ovf[t].r; idx[t] = (uint32_t)t;
}

} // namespace csd
