// host_parts.hpp -- the two pure steps of a host submit (pipelines.hip, pipe_submit): the check of the caller's offsets and the cut of a
// batch into parts.  Plain C++ with no HIP in it, so that tests/cpp/host_parts_check.cpp compiles it alone: the cut points decide how fast
// a blocking call is and never what it returns, which no parity test can see.
#pragma once
#include "../../include/compseed_amd.h"

#include <algorithm>
#include <cstdint>
#include <thread>
#include <vector>

namespace host_parts {

struct OffsetCheck { int rc; const char *msg; uint64_t max_len; }; // rc CS_OK: max_len is the longest read; else msg is the error text

// offsets[0 .. n_reads] of n_reads > 0 reads: starts at 0, never decreases, no read of 65535 bases or more
inline OffsetCheck check_offsets(const uint64_t *offsets, int64_t n_reads)
{
	if (offsets[0] != 0) return {CS_EINVAL, "offsets[0] must be 0", 0};
	// (10 M offsets are 6 ms on one thread, in front of everything else a blocking call does: four threads)
	const int vt = n_reads >= (1 << 20) ? 4 : 1;
	uint64_t vmax[4] = {0, 0, 0, 0}; bool vbad[4] = {false, false, false, false};
	auto vrange = [&](int t) {
		uint64_t m = 0; bool bad = false;
		for (int64_t r = n_reads * t / vt, r1 = n_reads * (t + 1) / vt; r < r1; ++r) { bad |= offsets[r + 1] < offsets[r]; m = std::max(m, offsets[r + 1] - offsets[r]); }
		vmax[t] = m; vbad[t] = bad;
	};
	if (vt == 1) vrange(0);
	else { std::thread th[3]; for (int t = 1; t < vt; ++t) th[t - 1] = std::thread(vrange, t); vrange(0); for (auto &t : th) t.join(); }
	uint64_t max_len = 0;
	for (int t = 0; t < vt; ++t) { if (vbad[t]) return {CS_EINVAL, "offsets must start at 0, be non-decreasing and end at n_bases", 0}; max_len = std::max(max_len, vmax[t]); }
	if (max_len >= 65535) return {CS_ERANGE, "read length exceeds the limit 65535 (MAX_READ_LEN)", max_len};
	return {CS_OK, nullptr, max_len};
}

// parts: contiguous read ranges of about pipeline_reads reads (one, if the batch is not much larger than that, or pipeline_reads is 0).
// Returns the cut points: part i is the reads [cut[i], cut[i + 1]); the first is 0, the last n_reads.
// streaming: two or more batches are in flight and the call does not expand.  Parts exist to overlap upload, seeding and download INSIDE
// one batch, and each part pays the fixed cost of a pass (two passes over 5 M reads take ~8 ms longer than one over 10 M).  When other
// batches are in flight the overlap comes from them -- upload of n+1 and download of n-1 beside the seeding of n -- so a batch submitted
// behind another one is seeded whole.  This needs THREE batches in flight to pay: with two, collect(n) returns when download(n) ends, only
// then can batch n+2 be submitted and uploaded, and download + upload (79 ms) is longer than the seeding of batch n+1 (55 ms): measured
// 92 ms per batch whole against 65 ms in parts.
inline std::vector<int64_t> cut_parts(int64_t n_reads, int64_t pipeline_reads, bool streaming)
{
	const int64_t per = pipeline_reads > 0 ? pipeline_reads : std::max<int64_t>(n_reads, 1);
	// part boundaries.  A batch that has the engine to itself (a blocking call, the first batch of a stream) cannot hide the upload of its
	// first part or the download of its last one behind anything, so those two are made small (0.2 of the nominal part) and the rest is
	// cut into parts of about 0.8: 10 M reads at 5 M nominal = 1 / 4 / 4 / 1 M (measured against 1.5 / 3.5 / 3.5 / 1.5: section 8 of DESIGN.md).
	std::vector<int64_t> cut(1, 0);
	const int64_t even = std::max<int64_t>(1, (n_reads + per / 2) / per);
	if (streaming || even < 2) cut.push_back(n_reads);
	else {
		const int64_t h = std::max<int64_t>(1, std::min<int64_t>(n_reads / 4, per * 2 / 10)), rest = n_reads - 2 * h;
		const int64_t km = std::max<int64_t>(1, (rest + per * 8 / 20) / std::max<int64_t>(1, per * 8 / 10));
		cut.push_back(h);
		for (int64_t i = 1; i <= km; ++i) cut.push_back(h + rest * i / km);
		cut.push_back(n_reads);
	}
	return cut;
}

} // namespace host_parts
