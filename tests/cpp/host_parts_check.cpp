// host_parts_check.cpp -- the two pure steps of a host submit (compseed_amd/csrc/host_parts.hpp) against cut points worked out by hand
// and offsets with known faults.  Prints every case and what it got; exit status 0 if all agree.  tests/test_host_parts.py compiles
// and runs it; no GPU, no library.
#include "../../compseed_amd/csrc/host_parts.hpp"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

static int n_bad = 0;

static void cut_case(int64_t n, int64_t per, bool streaming, const std::vector<int64_t> &want)
{
	const std::vector<int64_t> got = host_parts::cut_parts(n, per, streaming);
	printf("cut n=%lld per=%lld streaming=%d:", (long long)n, (long long)per, (int)streaming);
	for (int64_t c : got) printf(" %lld", (long long)c);
	const bool ok = got == want;
	printf(ok ? "  ok\n" : "  DIFFERS\n");
	n_bad += !ok;
}

static void offsets_case(const char *what, const std::vector<uint64_t> &off, int want_rc, const char *want_msg, uint64_t want_max)
{
	const host_parts::OffsetCheck v = host_parts::check_offsets(off.data(), (int64_t)off.size() - 1);
	const bool ok = v.rc == want_rc && (want_rc == CS_OK ? v.max_len == want_max : v.msg && !strcmp(v.msg, want_msg));
	printf("offsets %s: rc=%d max_len=%llu msg=%s  %s\n", what, v.rc, (unsigned long long)v.max_len, v.msg ? v.msg : "-", ok ? "ok" : "DIFFERS");
	n_bad += !ok;
}

int main()
{
	cut_case(10000000, 5000000, false, {0, 1000000, 5000000, 9000000, 10000000});
	cut_case(10000000, 5000000, true, {0, 10000000});
	cut_case(3000, 700, false, {0, 140, 684, 1228, 1772, 2316, 2860, 3000});
	cut_case(1350, 900, false, {0, 180, 1170, 1350});
	cut_case(1000, 900, false, {0, 1000});
	cut_case(200, 64, false, {0, 12, 70, 129, 188, 200});
	cut_case(5, 2, false, {0, 1, 2, 3, 4, 5});
	cut_case(5000, 0, false, {0, 5000});
	cut_case(0, 900, false, {0, 0});

	// any input: the cuts start at 0, end at n_reads and never decrease
	std::mt19937_64 rng(12345);
	int n_prop_bad = 0;
	for (int i = 0; i < 600; ++i) {
		const int64_t n = i < 40 ? i : (int64_t)(rng() % (i % 3 ? 20000 : 40000000));
		int64_t per = i % 7 == 0 ? 0 : i % 5 == 0 ? (int64_t)(rng() % 8) : (int64_t)(rng() % (2 * n + 10));
		if (per > 0 && per < n / 1000) per = n / 1000;   // (at most a few thousand parts: the vector is the test's time)
		const bool streaming = i % 11 == 0;
		const std::vector<int64_t> cut = host_parts::cut_parts(n, per, streaming);
		bool ok = cut.size() >= 2 && cut.front() == 0 && cut.back() == n;
		for (size_t k = 1; ok && k < cut.size(); ++k) ok = cut[k] >= cut[k - 1];
		if (!ok) { printf("cut property fails for n=%lld per=%lld streaming=%d\n", (long long)n, (long long)per, (int)streaming); ++n_prop_bad; }
	}
	printf("cut property over 600 random (n, per) pairs: %s\n", n_prop_bad ? "DIFFERS" : "ok");
	n_bad += n_prop_bad;

	const char *m_first = "offsets[0] must be 0", *m_order = "offsets must start at 0, be non-decreasing and end at n_bases", *m_long = "read length exceeds the limit 65535 (MAX_READ_LEN)";
	offsets_case("good", {0, 100, 100, 350, 351}, CS_OK, nullptr, 250);
	offsets_case("first not zero", {1, 100, 200}, CS_EINVAL, m_first, 0);
	offsets_case("one decreasing pair", {0, 100, 99, 200}, CS_EINVAL, m_order, 0);
	offsets_case("a read of 65534 bases", {0, 10, 65544}, CS_OK, nullptr, 65534);
	offsets_case("a read of 65535 bases", {0, 10, 65545}, CS_ERANGE, m_long, 0);
	{ // the four-thread scan: 2^20 + 3 reads of one base, good, then with one decreasing pair in the last quarter
		const size_t n = ((size_t)1 << 20) + 3;
		std::vector<uint64_t> off(n + 1);
		for (size_t r = 0; r <= n; ++r) off[r] = r;
		offsets_case("2^20 + 3 reads of one base", off, CS_OK, nullptr, 1);
		off[n - 1000] = off[n - 1001] - 1;
		offsets_case("... one decreasing pair in the last quarter", off, CS_EINVAL, m_order, 0);
	}
	printf("%d case(s) differ\n", n_bad);
	return n_bad ? 1 : 0;
}
