// lockstep.hpp -- what the CPU programs over the W-lane bodies share (chain_filter_scan_check.cpp, dedup_scan_check.cpp,
// dedup_pass_check.cpp, cigar_scan_check.cpp, align_scan_check.cpp): include it BEFORE the header under test.
// Built with -DCS_EMU_W=N (a power of two up to 64; -pthread) the CSD_ macros of compseed_amd/csrc/wave_lanes.hpp are defined over N
// threads in lockstep: a ballot or a shuffle is an exchange through a shared array between two barriers, so lanes that reach different
// collectives, or a different number of them, never finish (the tests' time limits) or differ in what they return.  Without it LANES
// is 1 and run_lanes calls its function once.
//   LANES           the lanes a program instantiates its bodies for
//   run_lanes(f)    f(lane) on LANES threads, joined; false: a thread could not be started
//   slurp / spill   a flat binary file into / out of a vector
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#ifdef CS_EMU_W
#include <pthread.h>
namespace emu {
constexpr int W = CS_EMU_W;
static_assert(W > 1 && W <= 64 && (W & (W - 1)) == 0, "lanes: a power of two up to 64");
static pthread_barrier_t bar;
static long long slot[64];
static thread_local int lane;
inline void sync() { pthread_barrier_wait(&bar); }
inline unsigned long long ballot(bool b)
{
	slot[lane] = b; sync();
	unsigned long long m = 0;
	for (int k = 0; k < W; ++k) if (slot[k]) m |= 1ull << k;
	sync();
	return m;
}
template <class T> inline T exchange(T v, int src) { slot[lane] = (long long)v; sync(); const T r = src >= 0 && src < W ? (T)slot[src] : v; sync(); return r; }
template <class F> struct Start { F *f; int lane; };
template <class F> void *start(void *p) { Start<F> *s = (Start<F> *)p; lane = s->lane; (*s->f)(s->lane); return nullptr; }
} // namespace emu
#define CSD_SYNC() emu::sync()
#define CSD_BALLOT(b) emu::ballot(b)
#define CSD_SHFL(v, src, W) emu::exchange(v, src)
#define CSD_SHFL_UP(v, d, W) emu::exchange(v, emu::lane - (d))
#define CSD_SHFL_XOR(v, d, W) emu::exchange(v, emu::lane ^ (d))
constexpr int LANES = emu::W;
template <class F> static bool run_lanes(F f)
{
	pthread_t th[64]; emu::Start<F> st[64];
	pthread_barrier_init(&emu::bar, nullptr, LANES);
	for (int x = 0; x < LANES; ++x) { st[x] = {&f, x}; if (pthread_create(&th[x], nullptr, emu::start<F>, &st[x])) return false; }
	for (int x = 0; x < LANES; ++x) pthread_join(th[x], nullptr);
	pthread_barrier_destroy(&emu::bar);
	return true;
}
#else
constexpr int LANES = 1;
template <class F> static bool run_lanes(F f) { f(0); return true; }
#endif

template <class T> static bool slurp(const std::string &path, std::vector<T> &v)
{
	FILE *fp = fopen(path.c_str(), "rb");
	if (!fp) { fprintf(stderr, "cannot read %s\n", path.c_str()); return false; }
	fseek(fp, 0, SEEK_END);
	const long sz = ftell(fp);
	fseek(fp, 0, SEEK_SET);
	v.resize((size_t)sz / sizeof(T));
	const size_t got = v.empty() ? 0 : fread(v.data(), sizeof(T), v.size(), fp);
	fclose(fp);
	return got == v.size() && (size_t)sz == v.size() * sizeof(T);
}
template <class T> static bool spill(const std::string &path, const std::vector<T> &v)
{
	FILE *fp = fopen(path.c_str(), "wb");
	if (!fp) return false;
	const size_t put = v.empty() ? 0 : fwrite(v.data(), sizeof(T), v.size(), fp);
	return fclose(fp) == 0 && put == v.size();
}
