// map_stream_check.cpp -- compseed_amd/csrc/map_stream.hpp alone, with stub parts of random short duration on the ring's real threads.
// Plain C++, no HIP, no GPU:  g++ -std=c++17 -O1 -pthread -o map_stream_check map_stream_check.cpp   (also built with -fsanitize=thread
// and with -fsanitize=address,undefined; it is a program of its own and needs nothing preloaded).
// Per schedule a fresh ring and a random sequence of submits and collects, checked against a model kept by the driver:
//   order     a collect hands out the OLDEST batch; each part sees the batches in submission order, one at a time, and a batch sees its
//             parts in order (front, de-duplication, tail)
//   cap       a submit succeeds exactly when fewer than CS_MAP_MAX_IN_FLIGHT batches are uncollected, and a refused one changes nothing;
//             a collect on an empty stream is NOTHING_IN_FLIGHT; finished <= submitted <= CS_MAP_MAX_IN_FLIGHT at every look
//   errors    a batch made to fail in part k fails at ITS collect with that part's code and text, its later parts never ran, the
//             batches behind it are as usual, and the result handed out before stays what it was
//   lifetime  the result of a successful collect keeps its address and its bytes until the next successful collect, whatever is
//             submitted, finishes or fails meanwhile -- looked at again after every later step and after waiting for all in flight
//   the end   a ring destroyed with batches uncollected waits for them and returns; drain() leaves the ring empty and usable
// A second family runs a submitting and a collecting thread against each other.  Over all schedules the three parts must have been seen
// running beside each other (de-duplication beside a front and beside a tail), or the ring is a queue and not a pipeline.
#include "../../compseed_amd/csrc/map_stream.hpp"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <random>
#include <vector>

namespace {
using map_stream::N_PARTS;
constexpr int CAP = CS_MAP_MAX_IN_FLIGHT, PAYLOAD = 48;

struct Job { int id = -1, fail_part = -1, us[N_PARTS] = {0, 0, 0}; int seen = 0; };   // seen: bit k set when part k ran
struct Result { int id = -1; std::vector<int> payload; int seen = 0; };
using Ring = map_stream::Ring<Job, Result>;

int differs = 0;
std::atomic<long> beside_front{0}, beside_tail{0}, part_runs{0};
void bad(const char *what, long a = 0, long b = 0) { ++differs; printf("  DIFFERS: %s (%ld, %ld)\n", what, a, b); }

// the stub parts of one ring, with what they observe of each other
struct Stubs {
	std::atomic<int> inside[N_PARTS], last_id[N_PARTS], faults{0};
	Stubs() { for (int k = 0; k < N_PARTS; ++k) { inside[k] = 0; last_id[k] = -1; } }
	int run(int k, Job &j, Result &r, std::string &err)
	{
		if (inside[k].fetch_add(1) != 0) ++faults;                         // a part runs one batch at a time
		if (last_id[k].exchange(j.id) >= j.id) ++faults;                   // ... in submission order
		if (j.seen != (1 << k) - 1) ++faults;                              // the batch's earlier parts, all of them, and nothing later
		j.seen |= 1 << k;
		if (k == map_stream::PART_DEDUP) { if (inside[map_stream::PART_FRONT]) ++beside_front; if (inside[map_stream::PART_TAIL]) ++beside_tail; }
		++part_runs;
		const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(j.us[k]);
		while (std::chrono::steady_clock::now() < until) std::this_thread::yield();
		int rc = CS_OK;
		if (j.fail_part == k) { rc = -(10 + k); err = "part " + std::to_string(k) + " of batch " + std::to_string(j.id); }
		else if (k == map_stream::PART_TAIL) { r.id = j.id; r.payload.assign(PAYLOAD, j.id * 7 + 1); r.seen = j.seen; }   // over whatever an older batch left
		inside[k].fetch_sub(1);
		return rc;
	}
};
struct Plan { int id, fail_part; };

bool result_is(const Result *r, int id)
{
	if (!r || r->id != id || (int)r->payload.size() != PAYLOAD || r->seen != 7) return false;
	for (int v : r->payload) if (v != id * 7 + 1) return false;
	return true;
}

// one thread submits and collects in a random order
void one_thread_schedule(std::mt19937 &rng, int steps, int max_us, int fail_every)
{
	Stubs S;
	std::vector<Plan> flight;                                             // the model: what is uncollected, oldest first
	const Result *kept = nullptr; const int *kept_data = nullptr; int kept_id = -1, next_id = 0;
	auto check_kept = [&](const char *when) { if (kept && (!result_is(kept, kept_id) || kept->payload.data() != kept_data)) bad(when, kept_id, kept->id); };
	{
		Ring R([&](Job &j, Result &r, std::string &e) { return S.run(0, j, r, e); }, [&](Job &j, Result &r, std::string &e) { return S.run(1, j, r, e); },
		       [&](Job &j, Result &r, std::string &e) { return S.run(2, j, r, e); });
		for (int s = 0; s < steps; ++s) {
			const int what = (int)(rng() % 8);
			if (what < 4) {                                                 // submit
				const Plan p = {next_id, fail_every && rng() % (unsigned)fail_every == 0 ? (int)(rng() % N_PARTS) : -1};
				int us[N_PARTS]; for (int &u : us) u = max_us ? (int)(rng() % (unsigned)max_us) : 0;
				bool filled = false;
				const bool ok = R.submit([&](Job &j) { filled = true; j = Job(); j.id = p.id; j.fail_part = p.fail_part; for (int k = 0; k < N_PARTS; ++k) j.us[k] = us[k]; });
				if (ok != ((int)flight.size() < CAP) || ok != filled) bad("the cap", (long)flight.size(), ok);
				if (ok) { flight.push_back(p); ++next_id; }
			} else if (what < 7) {                                          // collect
				Result *r = nullptr; std::string err;
				const int rc = R.collect(&r, err);
				if (flight.empty()) { if (rc != map_stream::NOTHING_IN_FLIGHT || r) bad("a collect on an empty stream", rc); }
				else {
					const Plan p = flight.front(); flight.erase(flight.begin());
					if (p.fail_part >= 0) {
						if (rc != -(10 + p.fail_part) || r || err != "part " + std::to_string(p.fail_part) + " of batch " + std::to_string(p.id)) bad("a failed batch's collect", rc, p.id);
						check_kept("the earlier result after a failed collect");
					} else {
						if (rc != CS_OK || !result_is(r, p.id)) bad("a collect", rc, p.id);
						kept = r; kept_id = p.id; kept_data = r ? r->payload.data() : nullptr;
					}
				}
			} else {                                                        // wait for everything in flight, without collecting
				for (;;) { int sub, fin; R.in_flight(&sub, &fin); if (sub != (int)flight.size() || fin > sub) { bad("in_flight", sub, fin); break; } if (fin == sub) break; std::this_thread::yield(); }
			}
			int sub, fin; R.in_flight(&sub, &fin);
			if (sub != (int)flight.size() || fin < 0 || fin > sub || sub > CAP || R.idle() != flight.empty()) bad("in_flight", sub, fin);
			check_kept("the collected result's lifetime");
		}
		if (rng() % 2) {                                                    // drain, then the ring is empty and takes a batch again
			R.drain();
			int sub, fin; R.in_flight(&sub, &fin);
			if (sub || fin || !R.idle()) bad("drain", sub, fin);
			check_kept("the collected result after drain");
			const int id = next_id;
			if (!R.submit([&](Job &j) { j = Job(); j.id = id; })) bad("a submit after drain");
			Result *r = nullptr; std::string err;
			if (R.collect(&r, err) != CS_OK || !result_is(r, id)) bad("a collect after drain");
		}
	}                                                                       // ~Ring with whatever is still uncollected
	if (S.faults) bad("the parts' order", S.faults);
	for (int k = 0; k < N_PARTS; ++k) if (S.inside[k]) bad("a part still running after the ring's end", k);
}

// a submitting and a collecting thread
void two_thread_schedule(std::mt19937 &rng, int n_batches, int max_us, int fail_every)
{
	Stubs S;
	std::vector<Plan> plan; std::vector<std::vector<int>> us;
	for (int i = 0; i < n_batches; ++i) {
		plan.push_back({i, fail_every && rng() % (unsigned)fail_every == 0 ? (int)(rng() % N_PARTS) : -1});
		us.push_back({(int)(rng() % (unsigned)max_us), (int)(rng() % (unsigned)max_us), (int)(rng() % (unsigned)max_us)});
	}
	std::atomic<int> wrong{0};
	{
		Ring R([&](Job &j, Result &r, std::string &e) { return S.run(0, j, r, e); }, [&](Job &j, Result &r, std::string &e) { return S.run(1, j, r, e); },
		       [&](Job &j, Result &r, std::string &e) { return S.run(2, j, r, e); });
		std::thread sub([&]() {
			for (int i = 0; i < n_batches; ++i)
				while (!R.submit([&](Job &j) { j = Job(); j.id = i; j.fail_part = plan[(size_t)i].fail_part; for (int k = 0; k < N_PARTS; ++k) j.us[k] = us[(size_t)i][(size_t)k]; })) std::this_thread::yield();
		});
		std::thread col([&]() {
			int kept_id = -1; const Result *kept = nullptr;
			for (int i = 0; i < n_batches;) {
				Result *r = nullptr; std::string err;
				const int rc = R.collect(&r, err);
				if (rc == map_stream::NOTHING_IN_FLIGHT) { std::this_thread::yield(); continue; }
				int s, f; R.in_flight(&s, &f);
				if (f > s || s > CAP) ++wrong;
				if (plan[(size_t)i].fail_part >= 0) { if (rc != -(10 + plan[(size_t)i].fail_part) || r || (kept && !result_is(kept, kept_id))) ++wrong; }
				else { if (rc != CS_OK || !result_is(r, i)) ++wrong; kept = r; kept_id = i; }
				++i;
			}
		});
		sub.join(); col.join();
		if (!R.idle()) ++wrong;
	}
	if (wrong) bad("two threads", wrong);
	if (S.faults) bad("the parts' order under two threads", S.faults);
}

void family(const char *name, int n, unsigned seed, void (*fn)(std::mt19937 &, int, int, int), int a, int max_us, int fail_every)
{
	const int before = differs;
	std::mt19937 rng(seed);
	for (int i = 0; i < n; ++i) fn(rng, a, max_us, fail_every);
	printf("%-58s %5d schedules%s\n", name, n, differs == before ? "  ok" : "");
}
} // namespace

int main()
{
	family("one thread, no errors, parts of up to 60 us", 1200, 1, one_thread_schedule, 24, 60, 0);
	family("one thread, one batch in four fails in a random part", 1200, 2, one_thread_schedule, 24, 60, 4);
	family("one thread, every batch fails", 200, 3, one_thread_schedule, 16, 40, 1);
	family("one thread, parts that take no time", 400, 4, one_thread_schedule, 40, 0, 5);
	family("one thread, long parts (up to 400 us)", 150, 5, one_thread_schedule, 16, 400, 6);
	family("submitting thread against collecting thread", 300, 6, two_thread_schedule, 20, 80, 0);
	family("submitting against collecting thread, one in five fails", 300, 7, two_thread_schedule, 20, 80, 5);
	{   // an error in each part at each position of a full stream, the others in order around it
		const int before = differs;
		int n = 0;
		for (int part = 0; part < N_PARTS; ++part) for (int pos = 0; pos < CAP; ++pos, ++n) {
			Stubs S;
			Ring R([&](Job &j, Result &r, std::string &e) { return S.run(0, j, r, e); }, [&](Job &j, Result &r, std::string &e) { return S.run(1, j, r, e); },
			       [&](Job &j, Result &r, std::string &e) { return S.run(2, j, r, e); });
			Result *r = nullptr; std::string err;
			R.submit([&](Job &j) { j = Job(); j.id = 0; j.us[1] = 50; });
			if (R.collect(&r, err) != CS_OK || !result_is(r, 0)) bad("the batch in front");
			const Result *kept = r;
			for (int i = 0; i < CAP; ++i) if (!R.submit([&](Job &j) { j = Job(); j.id = 1 + i; j.fail_part = i == pos ? part : -1; j.us[0] = j.us[1] = j.us[2] = 30; })) bad("a submit below the cap");
			if (R.submit([](Job &) {})) bad("a submit at the cap");
			for (int i = 0; i < CAP; ++i) {
				r = nullptr; err.clear();
				const int rc = R.collect(&r, err);
				if (i == pos) { if (rc != -(10 + part) || r || err != "part " + std::to_string(part) + " of batch " + std::to_string(1 + i)) bad("the failing batch", part, pos); if (!result_is(kept, i ? i : 0)) bad("the result before the failing batch", part, pos); }
				else { if (rc != CS_OK || !result_is(r, 1 + i)) bad("a batch beside the failing one", part, pos); kept = r; }
			}
			if (R.collect(&r, err) != map_stream::NOTHING_IN_FLIGHT) bad("the stream's end");
			if (S.faults) bad("the parts' order", S.faults);
		}
		printf("%-58s %5d schedules%s\n", "an error in each part at each position", n, differs == before ? "  ok" : "");
	}
	printf("part runs %ld; de-duplication seen beside a front %ld times, beside a tail %ld times\n", part_runs.load(), beside_front.load(), beside_tail.load());
	if (!beside_front || !beside_tail) bad("the parts never ran beside each other");
	printf("%d case(s) differ\n", differs);
	return differs ? 1 : 0;
}
