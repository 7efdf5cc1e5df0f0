// lane_sets.hpp -- a wave's 64 lanes handed out as SETS, not as aligned groups (bwd_win_run, smem_bwd.hpp): a call takes the lanes it
// needs, any free ones.  A set is a 64-bit mask; its members are ordered by lane number, and a member's RANK is its place in that order.
// The wave keeps one mask F of lanes that belong to no call; a call of w lanes gets the w lowest members of F, and gives lanes back to
// F when it ends (or earlier, where a lane can no longer matter).  Plain functions of masks, so that the kernel's arithmetic is the
// arithmetic tests/cpp/lane_sets_check.cpp checks without a GPU.  lane is 0..63 throughout.
#pragma once
#include <cstdint>

#ifndef CS_HD
#ifdef __HIP__
#define CS_HD __host__ __device__
#else
#define CS_HD
#endif
#endif

namespace csls {

CS_HD inline uint64_t below(uint32_t lane) { return (1ull << lane) - 1ull; }                       // the lanes under `lane`
CS_HD inline uint64_t above(uint32_t lane) { return ~1ull << lane; }                               // the lanes over it (one shift; none over lane 63)
CS_HD inline uint32_t count(uint64_t set) { return (uint32_t)__builtin_popcountll(set); }
CS_HD inline bool has(uint64_t set, uint32_t lane) { return ((set >> lane) & 1ull) != 0; }

// a lane's rank in a set: members under it (also defined for a lane outside the set)
CS_HD inline uint32_t rank_in(uint64_t set, uint32_t lane) { return count(set & below(lane)); }

// does `lane` belong to the w lowest members of F?  The ballot of this over a wave is take_lowest(F, w).
CS_HD inline bool takes(uint64_t F, uint32_t lane, uint32_t w) { return has(F, lane) && rank_in(F, lane) < w; }

// the w lowest members of F (all of F if it has fewer)
CS_HD inline uint64_t take_lowest(uint64_t F, uint32_t w)
{
	uint64_t rest = F;
	for (uint32_t q = 0; q < w && rest; ++q) rest &= rest - 1;
	return F & ~rest;
}

// the next higher member of a set as seen from `lane`, or `lane` itself if there is none
CS_HD inline uint32_t next_member(uint64_t set, uint32_t lane)
{
	const uint64_t a = set & above(lane);
	return a ? (uint32_t)__builtin_ctzll(a) : lane;
}

// a set after the lanes `gone` left it; the same AND serves every lane of the wave, whichever call it belongs to
CS_HD inline uint64_t release(uint64_t set, uint64_t gone) { return set & ~gone; }

} // namespace csls
