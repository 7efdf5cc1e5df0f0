// occ_math.hpp -- the arithmetic of one single-child backward extension over the device layout of the BWT (fm_device.hpp): counting the
// bases of a 32-byte record up to a row, and assembling child c of a bi-interval from the two (counts, planes) records that hold its
// two rows.  Plain functions of words, so that the kernel's arithmetic (extend1b, fm_device.hpp: the backward kernels of smem_bwd.hpp)
// is the arithmetic tests/cpp/occ_math_check.cpp checks without a GPU against counts made base by base and the cascade extend4 states.
//
// A record covers 64 rows: cnt[0..3] = occurrences of A, C, G, T before its first row (mod 2^32), then the low-bit plane of its 64 bases
// (lo0: rows 0..31, lo1: rows 32..63) and the high-bit plane (hi0, hi1).  Rows are the primary-adjusted ones (row_of).
#pragma once
#include <cstdint>

#ifndef CS_HD
#ifdef __HIP__
#define CS_HD __host__ __device__
#else
#define CS_HD
#endif
#endif

namespace csocc {

// the row of the stored BWT that holds position k of the BWT with its sentinel (bwt.c:176: k -= k >= primary); ge = k >= primary
CS_HD inline uint64_t row_of(uint64_t k, uint64_t primary, uint32_t &ge) { ge = k >= primary ? 1u : 0u; return k - ge; }

// occurrences of C, G, T among the bases 0 .. (row & 63) of a record, the row's own base included.  The mask of the bases BEHIND the
// row is one 64-bit shift of a constant by the row number as it stands (a shift takes the low six bits): the "first nb bits" form,
// ~0 >> (64 - nb), needs nb = (row & 63) + 1 and its complement to 64 first.  T = lo & hi, C = lo without T, G = hi without T.
CS_HD inline void count_cgt_upto(uint32_t lo0, uint32_t lo1, uint32_t hi0, uint32_t hi1, uint32_t row, uint32_t &c1, uint32_t &c2, uint32_t &c3)
{
	const uint64_t behind = ~1ull << (row & 63u);
	const uint32_t m0 = ~(uint32_t)behind, m1 = ~(uint32_t)(behind >> 32);
	c3 = (uint32_t)__builtin_popcount(lo0 & hi0 & m0) + (uint32_t)__builtin_popcount(lo1 & hi1 & m1);
	c1 = (uint32_t)__builtin_popcount(lo0 & m0) + (uint32_t)__builtin_popcount(lo1 & m1) - c3;
	c2 = (uint32_t)__builtin_popcount(hi0 & m0) + (uint32_t)__builtin_popcount(hi1 & m1) - c3;
}

struct Child { uint64_t ya, yb; uint32_t y2; }; // the searched coordinate, the other one, the size

// Child c (0..3) of the bi-interval whose searched coordinate covers positions k+1 .. l (k < l), bwt.c:262-275 for one child:
//   ya = L2[c] + 1 + Occ(c, k),  y2 = Occ(c, l) - Occ(c, k),  yb = xb + [k < primary <= l] + sum of y2 over the children above c.
// ck / cl: the counts of the records that hold rk and rl (the same record twice when the rows share one), k* / l*: their planes,
// rk / rl: the low words of the adjusted rows, gek / gel: row_of's flags, l2c1 = L2[c] + 1.
// Occ values and child sizes are below 2^32 (no base occurs 2^32 times: checked at engine creation), so everything up to the two
// coordinates is exact modulo 2^32, differences included.  The A counts are not counted: the children's sizes add up to the rows
// between k and l, so y2 of A is rl - rk less the three others, and Occ(A, k) is the row's place in its record less what was counted.
// k < primary <= l is gel - gek, from the two adjustments (k < l: gek <= gel).
CS_HD inline Child child1(const uint32_t ck[4], uint32_t klo0, uint32_t klo1, uint32_t khi0, uint32_t khi1,
                          const uint32_t cl[4], uint32_t llo0, uint32_t llo1, uint32_t lhi0, uint32_t lhi1,
                          uint32_t rk, uint32_t rl, uint32_t gek, uint32_t gel, uint32_t c, uint64_t l2c1, uint64_t xb)
{
	uint32_t k1, k2, k3, l1, l2, l3;
	count_cgt_upto(klo0, klo1, khi0, khi1, rk, k1, k2, k3);
	count_cgt_upto(llo0, llo1, lhi0, lhi1, rl, l1, l2, l3);
	const uint32_t tk1 = ck[1] + k1, tk2 = ck[2] + k2, tk3 = ck[3] + k3;
	const uint32_t tk0 = ck[0] + ((rk & 63u) + 1u - k1 - k2 - k3);
	const uint32_t s1 = cl[1] + l1 - tk1, s2 = cl[2] + l2 - tk2, s3 = cl[3] + l3 - tk3;
	const uint32_t a2 = s3 + s2, a1 = a2 + s1;     // the children above G, above C, above A
	const uint32_t s0 = rl - rk - a1;
	const bool c0 = c == 0, c1 = c == 1, c2 = c == 2;
	const uint32_t tkc = c0 ? tk0 : c1 ? tk1 : c2 ? tk2 : tk3;
	const uint32_t sc = c0 ? s0 : c1 ? s1 : c2 ? s2 : s3;
	const uint32_t above = c0 ? a1 : c1 ? a2 : c2 ? s3 : 0u; // (at most the parent's size: it fits)
	Child o;
	o.ya = l2c1 + tkc;
	o.yb = xb + (uint64_t)(gel - gek) + (uint64_t)above;
	o.y2 = sc;
	return o;
}

} // namespace csocc
