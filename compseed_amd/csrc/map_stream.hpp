// map_stream.hpp -- the queue behind cs_map_submit / cs_map_collect (mapper.hip): a ring of CS_MAP_MAX_IN_FLIGHT slots and the three worker
// threads that carry a batch through its three parts -- front (upload, seeding, chaining, filter, extension, download), de-duplication and
// tail (marking, CIGAR, SAM text).  Plain C++ with no HIP in it, so that tests/cpp/map_stream_check.cpp drives it alone with stub parts on
// real threads: which batch runs where and when decides how fast a stream is and never what it returns, which no parity test can see.
//
// A slot goes  free -> queued -> front done -> de-duplicated -> finished -> (collected) free.  Worker k owns part k and takes the batches in
// submission order: it waits until the slot of its next batch is in state queued + k, runs the part WITHOUT the lock, and moves the slot on.
// So the parts of one batch run one after the other, each part runs one batch at a time (a part's objects need no lock), and the three parts
// run beside each other on three different batches: de-duplication of batch n beside the front of n + 1 and the tail of n - 1.
// A part that returns an error marks its batch: the later parts pass that batch on without running, its collect returns the code and the
// text the part left, and nothing else is touched -- the batches behind it run as usual.
// Results: every slot has a Result of its own (three finished batches may wait for their collect) and the ring holds ONE more, `held`:
// a successful collect exchanges the slot's Result with `held` and hands `held` out, so a collected result is in no slot and stays as it
// is, whatever is submitted or finishes, until the next successful collect exchanges it again.  A part finds in its slot's Result
// whatever an older batch left there and overwrites it.
// Threads: one submitting and one collecting thread (they may be the same); in_flight() from either.  The workers start with the first
// submit -- a ring that is never submitted to owns no thread -- and call `on_thread_start` first (the mapper: hipSetDevice).
#pragma once
#include "../../include/compseed_amd.h"

#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <utility>

namespace map_stream {

enum State { FREE, QUEUED, FRONT_DONE, DEDUPED, FINISHED };
enum { PART_FRONT, PART_DEDUP, PART_TAIL, N_PARTS };
enum { NOTHING_IN_FLIGHT = 1 };                                        // collect(): no code of the library is positive

template <class Job, class Result> class Ring {
public:
	static constexpr int CAP = CS_MAP_MAX_IN_FLIGHT;
	using Part = std::function<int(Job &, Result &, std::string &err)>;   // CS_OK, or the code with the message in err

	Ring(Part front, Part dedup, Part tail, std::function<void()> on_thread_start = nullptr) : part_{std::move(front), std::move(dedup), std::move(tail)}, start_(std::move(on_thread_start)) {}
	Ring(const Ring &) = delete;
	Ring &operator=(const Ring &) = delete;
	~Ring()
	{
		drain();
		{ std::lock_guard<std::mutex> g(mu_); stop_ = true; }
		cv_.notify_all();
		for (std::thread &t : th_) if (t.joinable()) t.join();
	}

	// fill(job) sets the slot's job up; false, and fill is not called, with CAP batches uncollected
	template <class Fill> bool submit(Fill fill)
	{
		std::unique_lock<std::mutex> g(mu_);
		if (submitted_ - head_ >= (uint64_t)CAP) return false;
		Slot &s = slot_[submitted_ % CAP];
		fill(s.job);
		s.rc = CS_OK; s.err.clear(); s.st = QUEUED;
		++submitted_;
		if (!started_) { started_ = true; for (int k = 0; k < N_PARTS; ++k) th_[k] = std::thread([this, k]() { work(k); }); }
		g.unlock();
		cv_.notify_all();
		return true;
	}
	// Blocks until the OLDEST batch is finished.  CS_OK: *out is `held`, valid until the next successful collect.  NOTHING_IN_FLIGHT.
	// Otherwise the batch's code, with its message in err: nothing is handed out and `held` stays as it was.
	int collect(Result **out, std::string &err)
	{
		std::unique_lock<std::mutex> g(mu_);
		if (head_ == submitted_) return NOTHING_IN_FLIGHT;
		Slot &s = slot_[head_ % CAP];
		cv_.wait(g, [&]() { return s.st == FINISHED; });
		const int rc = s.rc;
		if (rc == CS_OK) { std::swap(s.res, held_); *out = &held_; } else err = s.err;
		s.st = FREE;
		++head_;
		return rc;
	}
	void in_flight(int *submitted, int *finished) const
	{
		std::lock_guard<std::mutex> g(mu_);
		*submitted = (int)(submitted_ - head_); *finished = (int)(next_[PART_TAIL] - head_);
	}
	bool idle() const { std::lock_guard<std::mutex> g(mu_); return head_ == submitted_; }
	// waits for everything submitted and drops it uncollected; `held` stays
	void drain()
	{
		std::unique_lock<std::mutex> g(mu_);
		cv_.wait(g, [&]() { return next_[PART_TAIL] == submitted_; });
		for (; head_ != submitted_; ++head_) slot_[head_ % CAP].st = FREE;
	}
	Result &held() { return held_; }                                    // the collecting thread's

private:
	struct Slot { State st = FREE; int rc = CS_OK; std::string err; Job job; Result res; };

	void work(int k)
	{
		if (start_) start_();
		std::unique_lock<std::mutex> g(mu_);
		for (;;) {
			cv_.wait(g, [&]() { return stop_ || (next_[k] < submitted_ && slot_[next_[k] % CAP].st == QUEUED + k); });
			if (stop_) return;                                            // (the destructor has drained: nothing is waiting)
			Slot &s = slot_[next_[k] % CAP];
			if (s.rc == CS_OK) {                                          // a batch an earlier part refused is passed on as it is
				g.unlock();
				std::string err;
				const int rc = part_[k](s.job, s.res, err);
				g.lock();
				if (rc != CS_OK) { s.rc = rc; s.err = std::move(err); }
			}
			s.st = (State)(QUEUED + k + 1);
			++next_[k];
			cv_.notify_all();
		}
	}

	Part part_[N_PARTS]; std::function<void()> start_;
	mutable std::mutex mu_; std::condition_variable cv_;
	Slot slot_[CAP]; Result held_;
	uint64_t head_ = 0, submitted_ = 0, next_[N_PARTS] = {0, 0, 0};       // batch numbers: the oldest uncollected, the next to submit, each worker's next
	bool started_ = false, stop_ = false;
	std::thread th_[N_PARTS];
};

} // namespace map_stream
