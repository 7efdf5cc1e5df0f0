// lane_sets_check.cpp -- compseed_amd/csrc/lane_sets.hpp (the mask arithmetic of bwd_win_run's dispenser, smem_bwd.hpp) as a plain C++
// program; tests/test_lane_sets_cpu.py builds and runs it.  No GPU and no Python in the process: it can be built with
// -fsanitize=address,undefined and run as it is.
//   lane_sets_check helpers          every helper against a naive loop: every w in 19..64 (and 0..18) over adversarial and random masks
//   lane_sets_check model SEED N R   a model of the dispenser, written lane by lane as the kernel is (64 copies of the per-lane state, a
//                                    ballot is a loop over them): N calls of random widths 19..64 and random lifetimes drawn 64 slots
//                                    at a time, foreign slots in between; R = 1: lanes other than a call's rank 0 also leave it early
//                                    (CS_WIN_RELEASE).  Every call must be placed, once, in queue order, on exactly w lanes that belong
//                                    to no other call; F must be the complement of the union of the calls' sets after every iteration;
//                                    a lane's rank in its set must never change while it stays; and the wave must come to its exit.
// Exit code 0 and one line "ok ..." on success; 1 and the failed check otherwise.
#include "../../compseed_amd/csrc/lane_sets.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint64_t rng_state = 1;
static uint64_t rnd()
{ // splitmix64
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

// ---------------------------------------------------------------------------------------------------------------------- naive forms
static uint32_t n_count(uint64_t m) { uint32_t c = 0; for (int b = 0; b < 64; ++b) if ((m >> b) & 1) ++c; return c; }
static uint32_t n_rank(uint64_t m, uint32_t lane) { uint32_t c = 0; for (uint32_t b = 0; b < lane; ++b) if ((m >> b) & 1) ++c; return c; }
static uint64_t n_take(uint64_t F, uint32_t w)
{
	uint64_t t = 0; uint32_t c = 0;
	for (int b = 0; b < 64 && c < w; ++b) if ((F >> b) & 1) { t |= 1ull << b; ++c; }
	return t;
}
static uint32_t n_next(uint64_t m, uint32_t lane) { for (uint32_t b = lane + 1; b < 64; ++b) if ((m >> b) & 1) return b; return lane; }

static int check_mask(uint64_t F, uint64_t other)
{
	CHECK(csls::count(F) == n_count(F), "F=%016llx", (unsigned long long)F);
	for (uint32_t lane = 0; lane < 64; ++lane) {
		uint64_t bel = 0, abv = 0;
		for (uint32_t b = 0; b < 64; ++b) { if (b < lane) bel |= 1ull << b; if (b > lane) abv |= 1ull << b; }
		CHECK(csls::below(lane) == bel && csls::above(lane) == abv, "lane %u", lane);
		CHECK(csls::has(F, lane) == (((F >> lane) & 1) != 0), "lane %u", lane);
		CHECK(csls::rank_in(F, lane) == n_rank(F, lane), "F=%016llx lane %u", (unsigned long long)F, lane);
		CHECK(csls::next_member(F, lane) == n_next(F, lane), "F=%016llx lane %u", (unsigned long long)F, lane);
	}
	for (uint32_t w = 0; w <= 64; ++w) {
		const uint64_t want = n_take(F, w);
		CHECK(csls::take_lowest(F, w) == want, "F=%016llx w=%u", (unsigned long long)F, w);
		uint64_t ballot = 0;
		for (uint32_t lane = 0; lane < 64; ++lane) if (csls::takes(F, lane, w)) ballot |= 1ull << lane;
		CHECK(ballot == want, "F=%016llx w=%u", (unsigned long long)F, w);
		CHECK((want & ~F) == 0 && n_count(want) == (n_count(F) < w ? n_count(F) : w), "F=%016llx w=%u", (unsigned long long)F, w);
		// the members of the taken set carry the ranks 0 .. w-1 in lane order
		uint32_t rk = 0;
		for (uint32_t lane = 0; lane < 64; ++lane) if ((want >> lane) & 1) { CHECK(csls::rank_in(want, lane) == rk, "F=%016llx w=%u lane %u", (unsigned long long)F, w, lane); ++rk; }
		const uint64_t rest = csls::release(F, want);
		CHECK((rest | want) == F && (rest & want) == 0, "F=%016llx w=%u", (unsigned long long)F, w);
	}
	uint64_t rel = 0;
	for (int b = 0; b < 64; ++b) if (((F >> b) & 1) && !((other >> b) & 1)) rel |= 1ull << b;
	CHECK(csls::release(F, other) == rel, "F=%016llx gone=%016llx", (unsigned long long)F, (unsigned long long)other);
	return 0;
}

static int helpers()
{
	std::vector<uint64_t> masks = {~0ull, 0ull, 0x5555555555555555ull, 0xAAAAAAAAAAAAAAAAull, 1ull, 1ull << 63, ~1ull, ~(1ull << 63), 0xFFFFFFFF00000000ull, 0x00000000FFFFFFFFull};
	for (uint32_t w = 1; w <= 64; ++w) {
		masks.push_back(w == 64 ? ~0ull : ~0ull << (64 - w));              // only the top w bits
		masks.push_back(w == 64 ? ~0ull : (1ull << w) - 1ull);             // only the low w bits
		masks.push_back((w == 64 ? ~0ull : ~0ull << (64 - w)) >> 1 | 1ull); // the top w bits but one, and lane 0
	}
	for (int q = 0; q < 2000; ++q) {
		uint64_t m = rnd();
		if (q % 3 == 1) m &= rnd();          // sparse
		if (q % 3 == 2) m |= rnd();          // dense
		masks.push_back(m);
	}
	for (size_t k = 0; k < masks.size(); ++k) if (check_mask(masks[k], masks[(k * 7 + 3) % masks.size()])) return 1;
	printf("ok helpers: %zu masks, w 0..64\n", masks.size());
	return 0;
}

// -------------------------------------------------------------------------------------------------------------------------- model
struct Lane { uint64_t gmask; uint32_t call, rank; int life; bool valid; };

static int model(uint64_t seed, int n_calls, bool early)
{
	rng_state = seed * 0x2545F4914F6CDD1Dull + 1;
	// the queue: n_calls calls of this kernel's classes among foreign slots; width 18 + n with n in 1..46, the boundaries often
	std::vector<int> slot_call; std::vector<uint32_t> width(n_calls); std::vector<int> life(n_calls);
	for (int c = 0; c < n_calls; ++c) {
		while (rnd() % 3 == 0) slot_call.push_back(-1);
		slot_call.push_back(c);
		const uint64_t k = rnd() % 8;
		const uint32_t n = k == 0 ? 1 : k == 1 ? 46 : k == 2 ? 14 + (uint32_t)(rnd() % 2) : k == 3 ? 45 : 1 + (uint32_t)(rnd() % 46);
		width[c] = 18 + n; life[c] = 1 + (int)(rnd() % 40);
	}
	const uint64_t n_tasks = slot_call.size();
	std::vector<int> placed(n_calls, 0), ended(n_calls, 0);
	std::vector<uint64_t> set_of(n_calls, 0);
	Lane L[64]; memset(L, 0, sizeof L);
	uint64_t F = ~0ull, batch_base = 0, avail_m = 0, ctr = 0; bool exhausted = false, place = true; uint32_t need = 19;
	uint8_t slot_w[64] = {0};
	int next_call = 0, max_live = 0; long iters = 0, attempts = 0;
	const long bound = 64L * (long)n_tasks + 64L * 41L * (long)n_calls + 1000;
	for (;;) {
		CHECK(++iters < bound, "no exit after %ld iterations", iters);
		if (place && csls::count(F) >= need) {
			++attempts;
			for (;;) {
				if (avail_m == 0) {
					if (exhausted) { need = 65; break; }
					const uint64_t base = ctr; ctr += 64;
					if (base >= n_tasks) { exhausted = true; need = 65; break; }
					avail_m = 0;
					for (uint32_t lane = 0; lane < 64; ++lane) {
						const uint64_t slot = base + lane;
						const int c = slot < n_tasks ? slot_call[slot] : -1;
						if (c >= 0) avail_m |= 1ull << lane;
						slot_w[lane] = (uint8_t)(c >= 0 ? width[c] : 0xff);
					}
					batch_base = base;
					continue;
				}
				const int k = __builtin_ctzll(avail_m);
				const uint32_t w = slot_w[k];
				CHECK(w >= 19 && w <= 64, "w=%u", w);
				if (csls::count(F) < w) { need = w; break; }
				uint64_t take = 0;
				for (uint32_t lane = 0; lane < 64; ++lane) if (csls::takes(F, lane, w)) take |= 1ull << lane;
				const int c = slot_call[batch_base + k];
				CHECK(c == next_call, "call %d placed, %d is next in the queue", c, next_call);
				++next_call; ++placed[c]; set_of[c] = take;
				CHECK(csls::count(take) == w, "call %d: %u lanes for w=%u", c, csls::count(take), w);
				for (uint32_t lane = 0; lane < 64; ++lane) if (csls::has(take, lane)) {
					CHECK(L[lane].gmask == 0, "lane %u given to call %d while call %u holds it", lane, c, L[lane].call);
					L[lane].gmask = take; L[lane].call = (uint32_t)c; L[lane].rank = csls::rank_in(take, lane); L[lane].life = life[c];
					L[lane].valid = true;
				}
				F = csls::release(F, take); avail_m &= avail_m - 1; need = 19;
			}
		}
		place = false;
		if (exhausted && avail_m == 0 && F == ~0ull) break;
		// one iteration of every live call: lanes lose `valid` at random (the equal-size rule), the call ends when its life is used up
		uint64_t gone = 0;
		for (uint32_t lane = 0; lane < 64; ++lane) if (L[lane].gmask) {
			Lane &l = L[lane];
			CHECK(csls::has(l.gmask, lane) && csls::rank_in(l.gmask, lane) <= l.rank, "lane %u", lane);
			CHECK((csls::rank_in(l.gmask, lane) == 0) == (l.rank == 0), "lane %u: rank 0 must stay the set's first lane", lane);
			if (rnd() % 6 == 0) l.valid = false;
			const bool end = --l.life == 0;
			if (end) ended[l.call] |= 1;
			if (end || (early && !l.valid && csls::rank_in(l.gmask, lane) != 0)) gone |= 1ull << lane;
		}
		if (gone) {
			CHECK((F & gone) == 0, "a free lane is released again");
			F |= gone; place = true;
			for (uint32_t lane = 0; lane < 64; ++lane) L[lane].gmask = csls::has(gone, lane) ? 0ull : csls::release(L[lane].gmask, gone);
		}
		// F is what no call holds; the lanes of a call agree on its set; sets are disjoint
		uint64_t held = 0; int live = 0; uint32_t seen[64]; int n_seen = 0;
		for (uint32_t lane = 0; lane < 64; ++lane) if (L[lane].gmask) {
			held |= 1ull << lane;
			for (uint32_t o = 0; o < 64; ++o) if (L[o].gmask) CHECK((L[o].call == L[lane].call) == csls::has(L[lane].gmask, o), "lanes %u and %u", lane, o);
			bool known = false;
			for (int q = 0; q < n_seen; ++q) known |= seen[q] == L[lane].call;
			if (!known) { seen[n_seen++] = L[lane].call; ++live; }
		}
		CHECK(F == ~held, "F=%016llx, held=%016llx", (unsigned long long)F, (unsigned long long)held);
		if (live > max_live) max_live = live;
	}
	for (int c = 0; c < n_calls; ++c) CHECK(placed[c] == 1 && ended[c] == 1, "call %d placed %d times, ended %d", c, placed[c], ended[c]);
	CHECK(ctr >= n_tasks, "queue not scanned");
	printf("ok model: %d calls in %zu slots, %ld iterations, %ld placement attempts, up to %d calls at once\n", n_calls, (size_t)n_tasks, iters, attempts, max_live);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && !strcmp(argv[1], "helpers")) return helpers();
	if (argc >= 5 && !strcmp(argv[1], "model")) return model(strtoull(argv[2], nullptr, 10), atoi(argv[3]), atoi(argv[4]) != 0);
	fprintf(stderr, "usage: lane_sets_check helpers | model SEED N_CALLS EARLY_RELEASE\n");
	return 2;
}
