// wave_lanes.hpp -- the W lanes (1 or 64) that the per-read and per-job bodies of chain_filter_scan.hpp, dedup_scan.hpp, cigar_scan.hpp,
// mark_scan.hpp and align_scan.hpp are written for: shuffles and ballots of a wave, or nothing at all.  A plain C++ program may define the CSD_ macros before it includes
// this header and run the W > 1 instantiations on lanes of its own (tests/cpp/lockstep.hpp: threads in lockstep); in device code they are
// the wave's own, for a block of one wave.  With W = 1 every primitive is the identity, so a body written once for W lanes is the
// sequential routine when one lane runs it.  The namespace stays csdd, where these primitives began (dedup_scan.hpp), so that no caller
// had to be renamed.
#pragma once
#include "cs_internal.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#define CSD_SYNC() __syncthreads()
#define CSD_BALLOT(b) __ballot(b)
#define CSD_SHFL(v, src, W) __shfl(v, src)
#define CSD_SHFL_UP(v, d, W) __shfl_up(v, d)
#define CSD_SHFL_XOR(v, d, W) __shfl_xor(v, d)
#endif

namespace csdd {
constexpr int64_t NO_G = INT64_MIN / 2;       // "no lane below this one" in the prefix maximum (band_align.hpp: no column before this one)

template <int W> CS_HD inline void wsync()
{
#ifdef CSD_SYNC
	if constexpr (W > 1) CSD_SYNC();
#endif
}
template <int W> CS_HD inline uint64_t wballot(bool b)
{
#ifdef CSD_SYNC
	if constexpr (W > 1) return CSD_BALLOT(b);
#endif
	return b ? 1ull : 0ull;
}
template <int W> CS_HD inline int wbcast(int v, int src)
{
#ifdef CSD_SYNC
	if constexpr (W > 1) return CSD_SHFL(v, src, W);
#endif
	(void)src;
	return v;
}
template <int W> CS_HD inline unsigned long long wbcast64(unsigned long long v, int src)
{
#ifdef CSD_SYNC
	if constexpr (W > 1) return CSD_SHFL(v, src, W);
#endif
	(void)src;
	return v;
}
// what lane 0 wrote to memory before it is what the other lanes read after it: a fence on the device, where the wave runs on by itself;
// the emulation's lanes meet at CSD_SYNC's barrier (no macro of its own: a program's lane macros stay the five above)
template <int W> CS_HD inline void wfence()
{
#if defined(__HIP_DEVICE_COMPILE__)
	if constexpr (W > 1) __threadfence();
#elif defined(CSD_SYNC)
	if constexpr (W > 1) CSD_SYNC();
#endif
}
template <int W, class T> CS_HD inline T wsum(T v)
{
#ifdef CSD_SYNC
	if constexpr (W > 1) for (int d = W >> 1; d > 0; d >>= 1) v += CSD_SHFL_XOR(v, d, W);
#endif
	return v;
}
// the sum of v over the lanes below this one; total: over all W
template <int W> CS_HD inline uint32_t wexcl_sum(uint32_t v, int lane, uint32_t &total)
{
	uint32_t x = v;
#ifdef CSD_SYNC
	if constexpr (W > 1) {
		for (int d = 1; d < W; d <<= 1) { const uint32_t y = CSD_SHFL_UP(x, d, W); if (lane >= d) x += y; }
		total = CSD_SHFL(x, W - 1, W);
		return x - v;
	}
#endif
	(void)lane;
	total = x;
	return x - v;
}
// the maximum of g over the lanes below this one and `carry` (the strips before); carry takes the whole strip in
template <int W> CS_HD inline int64_t wprefix_max(int64_t g, int lane, int64_t &carry)
{
	int64_t x = g;
#ifdef CSD_SYNC
	if constexpr (W > 1) {
		for (int d = 1; d < W; d <<= 1) { const int64_t y = (int64_t)CSD_SHFL_UP((long long)x, d, W); if (lane >= d) x = x > y ? x : y; }
		int64_t ex = (int64_t)CSD_SHFL_UP((long long)x, 1, W);
		if (lane == 0) ex = NO_G;
		ex = ex > carry ? ex : carry;
		const int64_t all = (int64_t)CSD_SHFL((long long)x, W - 1, W);
		carry = carry > all ? carry : all;
		return ex;
	}
#endif
	(void)lane;
	const int64_t ex = carry;
	carry = carry > x ? carry : x;
	return ex;
}
CS_HD inline uint64_t lanes_below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }
// the number of lanes in a ballot, unsigned as HIP's __popcll is: a list length that grows by it is computed as the chain filter's kernels
// always computed it (with a signed count the compiler proves the length non-negative and emits other compares)
CS_HD inline unsigned wcount(uint64_t m) { return (unsigned)__builtin_popcountll(m); }
} // namespace csdd
