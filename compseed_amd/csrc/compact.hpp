// compact.hpp -- the compaction of regions (align_gpu.hip: CS_ALN_DEV_COMPACT; dedup_pass.hpp: the survivors of a device
// de-duplication, whose kernels are not in the library yet): a flag per region, an exclusive scan over n + 1 flags (the last one 0: the total), then the flagged regions move as
// 8-byte words, a word per lane -- 7 words a region, so a wave reads 512 contiguous bytes and writes runs of them -- into a buffer of
// their own, and reg_off[r] becomes scan[reg_off[r]].  The bodies are plain functions indexed by region, word or read (a C++ program
// drives them without a GPU: tests/cpp/dedup_pass_check.cpp); the kernels are grid-stride loops around them, `inline` so that a second unit
// may include them (no device code crosses units).
#pragma once
#include "cs_internal.hpp"

namespace csa {
constexpr int REG_WORDS = (int)(sizeof(cs_alnreg_t) / 8);
static_assert(sizeof(cs_alnreg_t) == 56 && REG_WORDS * 8 == (int)sizeof(cs_alnreg_t), "cs_alnreg_t is seven 8-byte words");

CS_HD inline uint32_t live_flag(const cs_alnreg_t *regs, uint64_t n, uint64_t g) { return g < n && regs[g].qe > regs[g].qb ? 1u : 0u; }
CS_HD inline void move_word(const uint64_t *in, const uint32_t *live, const uint32_t *scan, uint64_t t, uint64_t *out)
{
	const uint64_t g = t / REG_WORDS;
	if (live[g]) out[(uint64_t)scan[g] * REG_WORDS + (t - g * REG_WORDS)] = in[t];
}
CS_HD inline void off_live(uint64_t *reg_off, const uint32_t *scan, int64_t r) { reg_off[r] = scan[reg_off[r]]; }   // in place: an entry is read and written by its own index

#ifdef __HIP__
// (`inline` gives the kernels the linkage of a template's instantiation -- one definition, whichever unit's -- and clang says it ignores it)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"
inline __global__ void live_kernel(const cs_alnreg_t *regs, uint64_t n, uint32_t *live)
{
	for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g <= n; g += (uint64_t)gridDim.x * blockDim.x) live[g] = live_flag(regs, n, g);
}
inline __global__ void scatter_kernel(const uint64_t *in, uint64_t n, const uint32_t *live, const uint32_t *scan, uint64_t *out)
{
	const uint64_t n_words = n * REG_WORDS;
	for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_words; t += (uint64_t)gridDim.x * blockDim.x) move_word(in, live, scan, t, out);
}
inline __global__ void reg_off_live_kernel(uint64_t *reg_off, int64_t n_reads, const uint32_t *scan, uint64_t n, unsigned long long *n_live)
{
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n_reads; r += (int64_t)gridDim.x * blockDim.x) off_live(reg_off, scan, r);
	if (blockIdx.x == 0 && threadIdx.x == 0) *n_live = scan[n];
}
#pragma clang diagnostic pop
#endif
} // namespace csa
