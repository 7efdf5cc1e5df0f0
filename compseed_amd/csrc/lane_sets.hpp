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

// ---- settling an end at the moment it stops (bwd_win_run, CS_WIN_SETTLE).  The ends of a call stop from the top of its set downward,
// ties within one iteration, so the first-survivor rule needs one value per lane: fup, the s of the nearest valid end above it that has
// already left the set (FUP_NONE: there is none).  stopv is the wave's ballot of "stopped in this iteration with valid == true".
constexpr int32_t FUP_NONE = 0x7fffffff;
// the valid ends of `lane`'s set above it that stop in this iteration
CS_HD inline uint64_t stops_above(uint64_t stopv, uint64_t gmask, uint32_t lane) { return stopv & gmask & above(lane); }
// the lane whose s a lane reads in this iteration: the nearest of stops_above, or itself
CS_HD inline uint32_t settle_src(uint64_t hi, uint32_t lane) { return hi ? (uint32_t)__builtin_ctzll(hi) : lane; }
// the s of the nearest valid end above: the one read from settle_src, or the carried one
CS_HD inline int32_t settle_fn(uint64_t hi, int32_t s_src, int32_t fup) { return hi ? s_src : fup; }
// does an end that stops valid at s report [s + 1, pend)?  The first-survivor rule as it stands (no valid end above, or it stopped
// strictly earlier: a larger s) and the length filter of emit_smem.
CS_HD inline bool settle_reports(int32_t s, int32_t fn, uint32_t pend, int32_t min_seed_len) { return s < fn && (int32_t)pend - (s + 1) >= min_seed_len; }
// what a lane carries on: the members of the set under a valid end that stopped take its s
CS_HD inline int32_t settle_carry(bool stopped, uint64_t hi, int32_t fn, int32_t fup) { return !stopped && hi ? fn : fup; }
// of the lanes that stopped in this iteration (`out`), those that go back to F at once: all but the ones that wait to report
CS_HD inline uint64_t settle_freed(uint64_t out, uint64_t reporting) { return out & ~reporting; }
// a lane's set after `out` left it: a lane that left holds no set, whether it is free or waits to report
CS_HD inline uint64_t settle_set(uint64_t gmask, uint64_t out, uint32_t lane) { return has(out, lane) ? 0ull : release(gmask, out); }
// Are the lanes P that wait to report flushed now?  When `thresh` of them have gathered; when the next placement (need lanes, 65: the
// queue is used up) is short of free lanes and they would make up for it; and when nothing else keeps the wave from its exit.
CS_HD inline bool settle_flush(uint64_t F, uint64_t P, uint32_t need, uint32_t thresh)
{
	if (P == 0) return false;
	if (count(P) >= thresh) return true;
	if (count(F) >= need) return false;
	return need > 64 ? (F | P) == ~0ull : count(F) + count(P) >= need;
}

} // namespace csls
