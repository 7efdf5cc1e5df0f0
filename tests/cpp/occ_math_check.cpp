// occ_math_check.cpp -- compseed_amd/csrc/occ_math.hpp without a GPU (tests/test_occ_math_cpu.py builds and runs it).
//   count : count_cgt_upto for every row of a record against a count made base by base, over random records and the all-A, all-T,
//           low-plane-only (all C) and high-plane-only (all G) records
//   child : child1 on a random BWT of three records (192 rows; with its sentinel 193 positions), record counts continued from an
//           offset just under 2^32 so that counts wrap inside the text and every difference is taken across the wrap: every pair of
//           positions k < l, every child, both directions, the sentinel (primary) at every position -- against the child assembled
//           literally from Occ counts made base by base, by the cascade extend4 states (fm_device.hpp; bwt.c:262-275).
//           The one case left out is k = 0 with primary = 0: its adjusted row is -1, and a real index has primary >= 1 (position 0
//           of the BWT belongs to the empty suffix).
// g++ -std=c++17 -O2 occ_math_check.cpp -o occ_math_check && ./occ_math_check count && ./occ_math_check child
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../../compseed_amd/csrc/occ_math.hpp"

struct Rec { uint32_t cnt[4], lo0, lo1, hi0, hi1; };

static int base_at(const Rec &r, uint32_t j) // base of row j (0..63) of a record
{
	const uint32_t lo = j < 32 ? r.lo0 : r.lo1, hi = j < 32 ? r.hi0 : r.hi1;
	return (int)(((lo >> (j & 31)) & 1u) | (((hi >> (j & 31)) & 1u) << 1));
}

static int check_count()
{
	std::mt19937_64 rng(20261);
	std::vector<Rec> recs;
	const uint32_t special[4][4] = {{0, 0, 0, 0}, {~0u, ~0u, ~0u, ~0u}, {~0u, ~0u, 0, 0}, {0, 0, ~0u, ~0u}};
	for (auto &q : special) recs.push_back(Rec{{0, 0, 0, 0}, q[0], q[1], q[2], q[3]});
	for (int i = 0; i < 4000; ++i) {
		uint64_t a = rng(), b = rng();
		if (i % 5 == 1) a &= rng();            // sparse and dense planes as well
		if (i % 5 == 2) b |= rng();
		recs.push_back(Rec{{0, 0, 0, 0}, (uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)});
	}
	unsigned long long n = 0;
	for (const Rec &r : recs) {
		uint32_t want[4] = {0, 0, 0, 0};
		for (uint32_t nb = 1; nb <= 64; ++nb) {
			++want[base_at(r, nb - 1)];
			// the row number as the kernel passes it: any 32-bit value whose low six bits are nb - 1
			const uint32_t row = (nb - 1) | ((uint32_t)rng() & ~63u);
			uint32_t c1, c2, c3;
			csocc::count_cgt_upto(r.lo0, r.lo1, r.hi0, r.hi1, row, c1, c2, c3);
			if (c1 != want[1] || c2 != want[2] || c3 != want[3] || nb - c1 - c2 - c3 != want[0]) {
				printf("FAIL count: planes %08x %08x %08x %08x nb %u: got %u %u %u, want %u %u %u\n", r.lo0, r.lo1, r.hi0, r.hi1, nb, c1, c2, c3, want[1], want[2], want[3]);
				return 1;
			}
			++n;
		}
	}
	printf("ok count: %llu cases over %zu records\n", n, recs.size());
	return 0;
}

static int check_child(uint64_t seed)
{
	constexpr int ROWS = 192, NPOS = ROWS + 1;
	std::mt19937_64 rng(seed);
	uint8_t bwt[ROWS];
	for (int i = 0; i < ROWS; ++i) bwt[i] = (uint8_t)(rng() & 3u);
	for (int i = 60; i < 70; ++i) bwt[i] = 3;                                   // a run across the first record boundary
	// record counts continue from OFF: within the 192 rows the counts of every base pass 2^32
	const uint32_t OFF[4] = {0xffffffffu - 20u, 0xffffffffu - 3u, 0xffffffffu, 0xffffffffu - 40u};
	Rec rec[3];
	uint32_t run[4] = {OFF[0], OFF[1], OFF[2], OFF[3]};
	for (int j = 0; j < 3; ++j) {
		Rec &r = rec[j];
		memcpy(r.cnt, run, sizeof run);
		r.lo0 = r.lo1 = r.hi0 = r.hi1 = 0;
		for (int q = 0; q < 64; ++q) {
			const int b = bwt[64 * j + q];
			(q < 32 ? r.lo0 : r.lo1) |= (uint32_t)(b & 1) << (q & 31);
			(q < 32 ? r.hi0 : r.hi1) |= (uint32_t)(b >> 1) << (q & 31);
			++run[b];
		}
	}
	const uint64_t L2[4] = {0, 0x1234567890ull, 0x1f00000000ull - 5, 0xfffffffffull};
	unsigned long long n = 0;
	for (int primary = 0; primary < NPOS; ++primary) {
		// Occ(c, pos): occurrences of c at positions 0..pos of the BWT with its sentinel at `primary`, base by base
		static uint32_t occ[4][NPOS];
		uint32_t seen[4] = {0, 0, 0, 0};
		for (int pos = 0; pos < NPOS; ++pos) {
			if (pos != primary) ++seen[bwt[pos - (pos > primary)]];
			for (int c = 0; c < 4; ++c) occ[c][pos] = seen[c];
		}
		for (int k = 0; k < NPOS - 1; ++k) {
			if (primary == 0 && k == 0) continue;
			for (int l = k + 1; l < NPOS; ++l) {
				const uint64_t xa = (uint64_t)k + 1, x2 = (uint64_t)(l - k), xb = (rng() & 0xffffffffffull) + 1;
				// the cascade of extend4 (fm_device.hpp), child sizes and the shifted coordinate from naive counts
				uint64_t y2[4], yb[4];
				for (int c = 0; c < 4; ++c) y2[c] = (uint64_t)(occ[c][l] - occ[c][k]);
				yb[3] = xb + ((xa <= (uint64_t)primary && xa + x2 - 1 >= (uint64_t)primary) ? 1 : 0);
				yb[2] = yb[3] + y2[3];
				yb[1] = yb[2] + y2[2];
				yb[0] = yb[1] + y2[1];
				uint32_t gek, gel;
				const uint64_t rk = csocc::row_of((uint64_t)k, (uint64_t)primary, gek), rl = csocc::row_of((uint64_t)l, (uint64_t)primary, gel);
				const Rec &bk = rec[rk >> 6], &bl = rec[rl >> 6];
				for (int c = 0; c < 4; ++c) {
					const uint64_t ya = L2[c] + 1 + (uint64_t)(uint32_t)(OFF[c] + occ[c][k]); // (the kernel's Occ is a 32-bit word)
					const csocc::Child got = csocc::child1(bk.cnt, bk.lo0, bk.lo1, bk.hi0, bk.hi1, bl.cnt, bl.lo0, bl.lo1, bl.hi0, bl.hi1,
					                                       (uint32_t)rk, (uint32_t)rl, gek, gel, (uint32_t)c, L2[c] + 1, xb);
					// both directions: backward reports (x0, x1) = (ya, yb), forward the two swapped (extend1_rt); the child itself is the same
					for (int is_back = 0; is_back < 2; ++is_back) {
						const uint64_t w0 = is_back ? ya : yb[c], w1 = is_back ? yb[c] : ya;
						const uint64_t g0 = is_back ? got.ya : got.yb, g1 = is_back ? got.yb : got.ya;
						if (g0 != w0 || g1 != w1 || (uint64_t)got.y2 != y2[c]) {
							printf("FAIL child: primary %d k %d l %d c %d back %d: got %llx %llx %u, want %llx %llx %llu\n", primary, k, l, c, is_back,
							       (unsigned long long)g0, (unsigned long long)g1, got.y2, (unsigned long long)w0, (unsigned long long)w1, (unsigned long long)y2[c]);
							return 1;
						}
						++n;
					}
				}
			}
		}
	}
	printf("ok child: %llu cases (seed %llu)\n", n, (unsigned long long)seed);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && !strcmp(argv[1], "count")) return check_count();
	if (argc >= 2 && !strcmp(argv[1], "child")) return check_child(argc >= 3 ? strtoull(argv[2], nullptr, 10) : 1);
	fprintf(stderr, "usage: %s count | child [seed]\n", argv[0]);
	return 2;
}
