// win_settle_check.cpp -- settling an end of bwd_win_run's wave loop (smem_bwd.hpp, CS_WIN_SETTLE) at the moment it stops, as a plain C++
// program over the functions of compseed_amd/csrc/lane_sets.hpp the kernel calls; tests/test_win_settle_cpu.py builds and runs it.  No
// GPU and no Python in the process: it can be built with -fsanitize=address,undefined and run as it is.
//   win_settle_check helpers        the settle_* helpers against naive loops over full, empty, alternating, top-only and random masks
//   win_settle_check model SEED N   a lane-by-lane model of the wave loop (64 copies of the per-lane state, a ballot is a loop over them)
//                                   on N synthetic calls: n = 1..46 stored LEPs, a random subset of valid window ends (none, only rank 0,
//                                   only rank 17, all 18 among them), per end the position f at which it stops -- non-increasing as the
//                                   end gets shorter, with ties, the read start among them --, equal-size stops sprinkled in, ends that
//                                   stop shorter than min_seed_len.  The same queue runs twice: with the first-survivor rule applied at
//                                   the call's end and rank 0 kept to it (the loop as it was), and settled at the stop.  Both must
//                                   report the same set for every call; every lane handed out returns to F exactly once; F is always the
//                                   complement of what calls and pending lanes hold; the calls of 64 lanes get placed; the wave reaches
//                                   its exit; and the settled loop needs fewer iterations, i.e. more calls share the wave.
// Exit code 0 and one line "ok ..." on success; 1 and the failed check otherwise.
#include "../../compseed_amd/csrc/lane_sets.hpp"

#include <algorithm>
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
#define LL(x) ((unsigned long long)(x))

constexpr int WIN = 18, K = 19, JK = 10; // window lanes, min_seed_len, jump_k (the defaults)
constexpr uint32_t PEND = 8;            // CS_WIN_PEND

// ------------------------------------------------------------------------------------------------------------------------ helpers
static int check_settle(uint64_t stopv, uint64_t gmask, uint64_t out)
{
	for (uint32_t lane = 0; lane < 64; ++lane) {
		uint64_t want = 0; int nearest = -1;
		for (uint32_t b = lane + 1; b < 64; ++b) if (((stopv >> b) & 1) && ((gmask >> b) & 1)) { want |= 1ull << b; if (nearest < 0) nearest = (int)b; }
		const uint64_t hi = csls::stops_above(stopv, gmask, lane);
		CHECK(hi == want, "stopv=%016llx gmask=%016llx lane %u", LL(stopv), LL(gmask), lane);
		CHECK(csls::settle_src(hi, lane) == (nearest < 0 ? lane : (uint32_t)nearest), "stopv=%016llx gmask=%016llx lane %u", LL(stopv), LL(gmask), lane);
		const int32_t s_src = (int32_t)(rnd() % 200) - 1, fup = rnd() % 3 ? (int32_t)(rnd() % 200) : csls::FUP_NONE;
		CHECK(csls::settle_fn(hi, s_src, fup) == (nearest < 0 ? fup : s_src), "lane %u", lane);
		for (int stopped = 0; stopped < 2; ++stopped)
			CHECK(csls::settle_carry(stopped != 0, hi, s_src, fup) == (!stopped && nearest >= 0 ? s_src : fup), "lane %u", lane);
		const uint64_t set = csls::settle_set(gmask, out, lane);
		uint64_t wset = 0;
		if (!((out >> lane) & 1)) for (uint32_t b = 0; b < 64; ++b) if (((gmask >> b) & 1) && !((out >> b) & 1)) wset |= 1ull << b;
		CHECK(set == wset, "gmask=%016llx out=%016llx lane %u", LL(gmask), LL(out), lane);
	}
	const uint64_t rep = out & stopv; // (those that wait to report are among the lanes that stopped)
	uint64_t freed = 0;
	for (uint32_t b = 0; b < 64; ++b) if (((out >> b) & 1) && !((rep >> b) & 1)) freed |= 1ull << b;
	CHECK(csls::settle_freed(out, rep) == freed && (freed | rep) == out && (freed & rep) == 0, "out=%016llx", LL(out));
	return 0;
}
static int check_flush(uint64_t F, uint64_t P)
{
	P &= ~F; // a lane that waits to report is not free
	uint32_t nf = 0, np = 0;
	for (int b = 0; b < 64; ++b) { nf += (F >> b) & 1; np += (P >> b) & 1; }
	for (uint32_t need = 19; need <= 65; ++need)
		for (uint32_t th = 1; th <= 64; th += (th < 9 ? 1 : 11)) {
			bool want = false;
			if (np > 0) {
				if (np >= th) want = true;
				else if (nf >= need) want = false;
				else want = need == 65 ? nf + np == 64 : nf + np >= need;
			}
			CHECK(csls::settle_flush(F, P, need, th) == want, "F=%016llx P=%016llx need=%u th=%u", LL(F), LL(P), need, th);
		}
	return 0;
}
static int helpers()
{
	std::vector<uint64_t> masks = {~0ull, 0ull, 0x5555555555555555ull, 0xAAAAAAAAAAAAAAAAull, 1ull, 1ull << 63, ~1ull, ~(1ull << 63), 0xFFFFFFFF00000000ull, 0x00000000FFFFFFFFull};
	for (uint32_t w = 1; w < 64; ++w) { masks.push_back(~0ull << (64 - w)); masks.push_back((1ull << w) - 1ull); }
	for (int q = 0; q < 600; ++q) {
		uint64_t m = rnd();
		if (q % 3 == 1) m &= rnd() & rnd();  // sparse
		if (q % 3 == 2) m |= rnd();          // dense
		masks.push_back(m);
	}
	const size_t n = masks.size();
	for (size_t k = 0; k < n; ++k) {
		if (check_settle(masks[k], masks[(k * 7 + 3) % n], masks[(k * 13 + 5) % n])) return 1;
		if (check_settle(masks[k] & masks[(k * 7 + 3) % n], masks[(k * 7 + 3) % n], masks[k])) return 1; // the stops inside the set
		if (check_flush(masks[k], masks[(k * 11 + 1) % n])) return 1;
	}
	// the rule: no valid end above (FUP_NONE) or a strictly larger s above, and at least min_seed_len bases
	for (int32_t s = -1; s < 60; ++s)
		for (int32_t fn = -1; fn < 62; ++fn)
			for (uint32_t pend = (uint32_t)(s + 1); pend < (uint32_t)(s + 40); ++pend) {
				CHECK(csls::settle_reports(s, fn, pend, K) == (s < fn && (int)pend - (s + 1) >= K), "s=%d fn=%d pend=%u", s, fn, pend);
				CHECK(csls::settle_reports(s, csls::FUP_NONE, pend, K) == ((int)pend - (s + 1) >= K), "s=%d pend=%u", s, pend);
			}
	printf("ok helpers: %zu masks\n", n);
	return 0;
}

// -------------------------------------------------------------------------------------------------------------------------- model
struct End { bool valid; int s0, f, eq; uint32_t pend; };                // an end: where it joins the clock, where it stops, from where on the equal-size rule takes it (-2: never)
struct Call { int x, n; std::vector<End> end; };                         // end[rank], rank 0..17 the window, 18 + j LEP j
struct Rep { int call; uint32_t pend; int beg; bool operator<(const Rep &o) const { return call != o.call ? call < o.call : pend != o.pend ? pend < o.pend : beg < o.beg; } bool operator==(const Rep &o) const { return call == o.call && pend == o.pend && beg == o.beg; } };
struct Lane { uint64_t gmask; int call; uint32_t rank; bool walking, valid; int s, clk, fup, eq, f; uint32_t pend; };
struct Run { std::vector<Rep> reps; long iters, call_iters; int max_live; long flushes; };

static void make_calls(uint64_t seed, int n_calls, std::vector<Call> &calls, std::vector<int> &slot_call)
{
	rng_state = seed * 0x2545F4914F6CDD1Dull + 1;
	calls.resize(n_calls);
	for (int c = 0; c < n_calls; ++c) {
		while (rnd() % 3 == 0) slot_call.push_back(-1); // foreign slots
		slot_call.push_back(c);
		Call &C = calls[c];
		const uint64_t kn = rnd() % 8;
		C.n = kn == 0 ? 1 : kn == 1 ? 46 : kn == 2 ? 14 + (int)(rnd() % 2) : kn == 3 ? 45 : 1 + (int)(rnd() % 46);
		C.x = 1 + (int)(rnd() % 120);
		C.end.resize(WIN + C.n);
		const uint64_t kw = rnd() % 6; // the window ends that pass the filter and the jump lookup
		uint64_t wm = kw == 0 ? 0 : kw == 1 ? 1 : kw == 2 ? 1ull << 17 : kw == 3 ? (1ull << 18) - 1 : rnd() & rnd() & ((1ull << 18) - 1);
		if (kw == 5) wm = rnd() & ((1ull << 18) - 1);
		// f from the top rank down: non-increasing, with ties; nothing stops in front of the pivot - 1 or past the read start
		const int style = (int)(rnd() % 4); // 0: mostly ties, 1: staggered by small steps, 2: long strides, 3: mixed
		int f = C.x - 1 - (int)(rnd() % 4 ? rnd() % 6 : 0);
		if (f < -1) f = -1;
		int t = C.x + K + C.n - 1 + (int)(rnd() % 5) + C.n; // LEP ends, ascending with rank
		for (int rk = WIN + C.n - 1; rk >= 0; --rk) {
			End &E = C.end[rk];
			if (rk >= WIN) { E.valid = true; E.s0 = C.x - 1; E.pend = (uint32_t)t; t -= 1 + (int)(rnd() % 2); if (t < C.x + K) t = C.x + K; if (rk > WIN && t < C.x + K + (rk - WIN - 1)) t = C.x + K + (rk - WIN - 1); }
			else { E.pend = (uint32_t)(C.x + 1 + rk); E.valid = ((wm >> rk) & 1) != 0 && (int)E.pend >= K; /* (the window must start inside the read) */ E.s0 = C.x + rk - JK; }
			E.f = std::min(f, E.s0);
			if (E.f < -1) E.f = -1;
			E.eq = rnd() % 5 == 0 ? E.s0 - (int)(rnd() % 12) : -2;
			const uint64_t d = rnd() % 8;
			const int stepd = style == 0 ? (d == 0) : style == 1 ? (int)(d % 3) : style == 2 ? (d < 3 ? 0 : (int)(rnd() % 25)) : (d < 4 ? 0 : (int)(rnd() % 9));
			f -= stepd;
			if (f < -1) f = -1;
		}
		// (LEP ends must ascend strictly with the rank: make them so from the bottom up)
		for (int rk = WIN + 1; rk < WIN + C.n; ++rk) if (C.end[rk].pend <= C.end[rk - 1].pend) C.end[rk].pend = C.end[rk - 1].pend + 1;
	}
}

// what the call reports by the rule as the reference states it, from the ends alone: who stopped valid (no equal-size stop took it
// first) is decided by the run; here only the rule over those
static int run(const std::vector<Call> &calls, const std::vector<int> &slot_call, bool settle, Run &R)
{
	const int n_calls = (int)calls.size();
	const uint64_t n_tasks = slot_call.size();
	std::vector<int> placed(n_calls, 0);
	Lane L[64]; memset(L, 0, sizeof L);
	int returned[64] = {0}, taken[64] = {0};
	uint64_t F = ~0ull, P = 0, batch_base = 0, avail_m = 0, ctr = 0; bool exhausted = false, place = true; uint32_t need = WIN + 1;
	uint8_t slot_w[64] = {0};
	int next_call = 0; long bound = 64L * (long)n_tasks + 400L * (long)n_calls + 1000;
	R.iters = 0; R.call_iters = 0; R.max_live = 0; R.flushes = 0; R.reps.clear();
	auto give_back = [&](uint64_t m) -> int {
		CHECK((F & m) == 0, "a free lane is released again: F=%016llx m=%016llx", LL(F), LL(m));
		for (uint32_t lane = 0; lane < 64; ++lane) if (csls::has(m, lane)) ++returned[lane];
		F |= m;
		return 0;
	};
	for (;;) {
		CHECK(++R.iters < bound, "no exit after %ld iterations", R.iters);
		while (place) {
			place = false;
			if (csls::count(F) >= need) {
				uint64_t fresh = 0;
				for (;;) {
					if (avail_m == 0) {
						if (exhausted) { need = 65; break; }
						const uint64_t base = ctr; ctr += 64;
						if (base >= n_tasks) { exhausted = true; need = 65; break; }
						for (uint32_t lane = 0; lane < 64; ++lane) {
							const uint64_t slot = base + lane;
							const int c = slot < n_tasks ? slot_call[slot] : -1;
							if (c >= 0) avail_m |= 1ull << lane;
							slot_w[lane] = (uint8_t)(c >= 0 ? WIN + calls[c].n : 0xff);
						}
						batch_base = base;
						continue;
					}
					const int k = __builtin_ctzll(avail_m);
					const uint32_t w = slot_w[k];
					if (csls::count(F) < w) { need = w; break; }
					uint64_t take = 0;
					for (uint32_t lane = 0; lane < 64; ++lane) if (csls::takes(F, lane, w)) take |= 1ull << lane;
					const int c = slot_call[batch_base + k];
					CHECK(c == next_call, "call %d placed, %d is next in the queue", c, next_call);
					CHECK(csls::count(take) == w && (take & P) == 0, "call %d: %u lanes for w=%u", c, csls::count(take), w);
					++next_call; ++placed[c];
					for (uint32_t lane = 0; lane < 64; ++lane) if (csls::has(take, lane)) {
						CHECK(L[lane].gmask == 0, "lane %u given to call %d while call %d holds it", lane, c, L[lane].call);
						Lane &l = L[lane]; const Call &C = calls[c];
						l.gmask = take; l.call = c; l.rank = csls::rank_in(take, lane); ++taken[lane];
						const End &E = C.end[l.rank];
						l.valid = E.valid; l.walking = E.valid; l.s = E.s0; l.f = E.f; l.eq = E.eq; l.pend = E.pend; l.fup = csls::FUP_NONE;
						l.clk = C.x + WIN - JK - 1; if (l.clk < C.x - 1) l.clk = C.x - 1;
					}
					fresh |= take;
					F = csls::release(F, take); avail_m &= avail_m - 1; need = WIN + 1;
				}
				if (settle) {
					uint64_t dud = 0;
					for (uint32_t lane = 0; lane < 64; ++lane) if (csls::has(fresh, lane) && !L[lane].valid) dud |= 1ull << lane;
					if (dud) {
						if (give_back(dud)) return 1;
						for (uint32_t lane = 0; lane < 64; ++lane) L[lane].gmask = csls::settle_set(L[lane].gmask, dud, lane);
						place = true;
					}
				}
			}
			if (settle && csls::settle_flush(F, P, need, PEND)) {
				for (uint32_t lane = 0; lane < 64; ++lane) if (csls::has(P, lane)) R.reps.push_back({L[lane].call, L[lane].pend, L[lane].s + 1});
				const uint64_t m = P; P = 0; ++R.flushes;
				if (give_back(m)) return 1;
				place = true;
			}
		}
		if (exhausted && avail_m == 0 && F == ~0ull) break;
		// ---- one iteration: the step
		bool step[64], stopv[64], surv[64];
		for (uint32_t lane = 0; lane < 64; ++lane) {
			Lane &l = L[lane];
			step[lane] = l.walking && l.s == l.clk;
			if (l.walking) CHECK(l.gmask != 0 && csls::has(l.gmask, lane), "lane %u walks without a set", lane);
			if (step[lane]) { if (l.s == l.f) l.walking = false; else --l.s; }
			stopv[lane] = step[lane] && !l.walking;
			surv[lane] = step[lane] && l.walking;
		}
		uint64_t surv_m = 0;
		for (uint32_t lane = 0; lane < 64; ++lane) if (surv[lane]) surv_m |= 1ull << lane;
		for (uint32_t lane = 0; lane < 64; ++lane) {
			Lane &l = L[lane];
			if ((l.clk & 3) == 0 && surv[lane] && (surv_m & l.gmask & csls::above(lane)) != 0 && l.clk <= l.eq) { l.walking = false; l.valid = false; }
		}
		for (uint32_t lane = 0; lane < 64; ++lane) --L[lane].clk;
		if (settle) {
			uint64_t out = 0, stopm = 0, pm = 0;
			for (uint32_t lane = 0; lane < 64; ++lane) { if (step[lane] && !L[lane].walking) out |= 1ull << lane; if (stopv[lane]) stopm |= 1ull << lane; }
			if (out) {
				int s_of[64]; for (uint32_t lane = 0; lane < 64; ++lane) s_of[lane] = L[lane].s;
				if (stopm) for (uint32_t lane = 0; lane < 64; ++lane) {
					Lane &l = L[lane];
					const uint64_t hi = csls::stops_above(stopm, l.gmask, lane);
					const int fn = csls::settle_fn(hi, s_of[csls::settle_src(hi, lane)], l.fup);
					if (stopv[lane]) {
						// the claim the change rests on: whatever valid end above has left did so at a strictly larger s
						CHECK(l.fup == csls::FUP_NONE || l.s < l.fup, "lane %u: fup %d, s %d", lane, l.fup, l.s);
						if (csls::settle_reports(l.s, fn, l.pend, K)) pm |= 1ull << lane;
					}
					l.fup = csls::settle_carry(stopv[lane], hi, fn, l.fup);
				}
				CHECK((P & out) == 0, "a pending lane stopped again");
				P |= pm;
				if (give_back(csls::settle_freed(out, pm))) return 1;
				place = true;
				for (uint32_t lane = 0; lane < 64; ++lane) L[lane].gmask = csls::settle_set(L[lane].gmask, out, lane);
			}
		} else {
			uint64_t walk_m = 0, valid_m = 0, gone = 0;
			for (uint32_t lane = 0; lane < 64; ++lane) { if (L[lane].walking) walk_m |= 1ull << lane; if (L[lane].gmask && L[lane].valid) valid_m |= 1ull << lane; }
			bool ending[64];
			for (uint32_t lane = 0; lane < 64; ++lane) {
				Lane &l = L[lane];
				ending[lane] = l.gmask != 0 && (walk_m & l.gmask) == 0;
				if (ending[lane] && l.valid) {
					const uint64_t hi = valid_m & l.gmask & csls::above(lane);
					const int fn = L[hi ? __builtin_ctzll(hi) : (int)lane].s;
					if ((hi == 0 || l.s < fn) && (int)l.pend - (l.s + 1) >= K) R.reps.push_back({l.call, l.pend, l.s + 1});
				}
			}
			for (uint32_t lane = 0; lane < 64; ++lane) {
				Lane &l = L[lane];
				if (ending[lane]) l.valid = false;
				if (l.gmask != 0 && !l.valid && (ending[lane] || l.rank != 0)) gone |= 1ull << lane; // (rank 0 stays for the successor)
			}
			if (gone) {
				if (give_back(gone)) return 1;
				place = true;
				for (uint32_t lane = 0; lane < 64; ++lane) L[lane].gmask = csls::has(gone, lane) ? 0ull : csls::release(L[lane].gmask, gone);
			}
		}
		// ---- F is the complement of what calls and pending lanes hold; the lanes of a call agree on its set
		uint64_t held = 0; int live = 0, seen[64], n_seen = 0;
		for (uint32_t lane = 0; lane < 64; ++lane) if (L[lane].gmask) {
			held |= 1ull << lane;
			CHECK(csls::has(L[lane].gmask, lane), "lane %u is not in its own set", lane);
			for (uint32_t o = 0; o < 64; ++o) if (L[o].gmask) CHECK((L[o].call == L[lane].call) == csls::has(L[lane].gmask, o), "lanes %u and %u", lane, o);
			bool known = false;
			for (int q = 0; q < n_seen; ++q) known |= seen[q] == L[lane].call;
			if (!known) { seen[n_seen++] = L[lane].call; ++live; }
		}
		CHECK((held & P) == 0, "a pending lane is in a set");
		CHECK(F == ~(held | P), "F=%016llx held=%016llx P=%016llx", LL(F), LL(held), LL(P));
		if (live > R.max_live) R.max_live = live;
		R.call_iters += live;
	}
	CHECK(P == 0, "pending lanes at the exit");
	for (int c = 0; c < n_calls; ++c) CHECK(placed[c] == 1, "call %d placed %d times", c, placed[c]);
	for (uint32_t lane = 0; lane < 64; ++lane) CHECK(taken[lane] == returned[lane], "lane %u taken %d times, returned %d times", lane, taken[lane], returned[lane]);
	CHECK(ctr >= n_tasks, "queue not scanned");
	std::sort(R.reps.begin(), R.reps.end());
	return 0;
}

static int model(uint64_t seed, int n_calls)
{
	std::vector<Call> calls; std::vector<int> slot_call;
	make_calls(seed, n_calls, calls, slot_call);
	if (n_calls >= 3) { calls[n_calls / 2].n = 46; calls[n_calls / 2].end.resize(WIN + 46, calls[n_calls / 2].end.back()); for (int rk = WIN + 1; rk < WIN + 46; ++rk) calls[n_calls / 2].end[rk].pend = calls[n_calls / 2].end[rk - 1].pend + 1; }
	// the input holds what it is meant to: f non-increasing as the rank falls, ends in staggered iterations, ties, short ends
	long staggered = 0, tied = 0, full = 0;
	for (const Call &C : calls) {
		for (size_t rk = 1; rk < C.end.size(); ++rk) CHECK(C.end[rk - 1].f <= C.end[rk].f && (!C.end[rk].valid || C.end[rk].f <= C.end[rk].s0) && C.end[rk - 1].f >= -1, "f is not monotone");
		for (int rk = WIN + 1; rk < WIN + C.n; ++rk) CHECK(C.end[rk].pend > C.end[rk - 1].pend, "LEP ends do not ascend");
		staggered += C.end.front().f + 30 <= C.end.back().f; tied += C.end[WIN].f == C.end.back().f && C.n > 1; full += C.n == 46;
	}
	if (n_calls >= 65) CHECK(staggered > 0 && tied > 0 && full > 0, "staggered %ld tied %ld full %ld", staggered, tied, full);
	Run A, B;
	if (run(calls, slot_call, false, A)) return 1;
	if (run(calls, slot_call, true, B)) return 1;
	CHECK(A.reps.size() == B.reps.size(), "%zu reports at the call's end, %zu settled at the stop", A.reps.size(), B.reps.size());
	for (size_t k = 0; k < A.reps.size(); ++k) CHECK(A.reps[k] == B.reps[k], "report %zu: call %d [%d, %u) vs call %d [%d, %u)", k, A.reps[k].call, A.reps[k].beg, A.reps[k].pend, B.reps[k].call, B.reps[k].beg, B.reps[k].pend);
	size_t short_ends = 0;
	for (const Call &C : calls) for (const End &E : C.end) short_ends += E.valid && (int)E.pend - (E.f + 1) < K;
	CHECK(B.iters <= A.iters, "%ld iterations settled at the stop, %ld at the call's end", B.iters, A.iters);
	printf("ok model: %d calls, %zu reports (%zu ends stop short), iterations %ld -> %ld, calls per iteration %.3f -> %.3f, up to %d -> %d calls at once, %ld flushes\n",
	       n_calls, A.reps.size(), short_ends, A.iters, B.iters, (double)A.call_iters / (double)A.iters, (double)B.call_iters / (double)B.iters, A.max_live, B.max_live, B.flushes);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && !strcmp(argv[1], "helpers")) return helpers();
	if (argc >= 4 && !strcmp(argv[1], "model")) return model(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
	fprintf(stderr, "usage: win_settle_check helpers | model SEED N_CALLS\n");
	return 2;
}
