// Stand-alone check of the host bookkeeping around the matrix-adjustment kernel (csrc/cbs_core.h: cbs_slots_assign,
// cbs_patch_runs): which slot of the matrix store a pair of a planning step takes, which pairs go back to the host threads, and
// the runs of consecutive slots their tables are copied in. Built with -fsanitize=address,undefined by
// tests/test_cbs_device_emu.py; prints "ok" and returns 0, or says which step failed.
#include "../../diamond_amd/csrc/cbs_core.h"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace dmnd;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

// what extend_host.hip does with the two functions, the matrix store stood in by a vector of slot owners
static void step(int64_t before, const std::vector<int32_t>& rule, const std::vector<uint8_t>& status, const std::vector<uint8_t>& host_keeps)
{
	const int64_t n = (int64_t)rule.size();
	std::vector<int32_t> mat((size_t)n, 12345);
	std::vector<int64_t> handed((size_t)n, -7);
	int64_t by[4];
	const int64_t h = cbs_slots_assign(before, n, rule.data(), status.data(), mat.data(), handed.data(), by);
	CHECK(by[0] + by[1] + by[2] + by[3] == n && h == n - by[0]);
	int64_t x = 0;
	for (int64_t k = 0; k < n; ++k) {
		if (status[(size_t)k] != 0) { CHECK(x < h && handed[(size_t)x] == k); ++x; CHECK(mat[(size_t)k] == before + k); }
		else CHECK(mat[(size_t)k] == (rule[(size_t)k] == CBSD_RULE_NONE ? -1 : before + k));
	}
	CHECK(x == h);
	std::vector<uint8_t> keep((size_t)h);
	for (int64_t i = 0; i < h; ++i) keep[(size_t)i] = host_keeps[(size_t)handed[(size_t)i]];
	std::vector<CbsPatchRun> runs((size_t)h);
	const int64_t r = cbs_patch_runs(before, handed.data(), keep.data(), h, runs.data());
	CHECK(r <= h);
	// every kept handed-back pair is covered exactly once, by its own patch, and nothing else is written
	std::vector<int64_t> store((size_t)(before + n), -1);
	for (int64_t i = 0; i < r; ++i) {
		CHECK(runs[(size_t)i].n >= 1 && runs[(size_t)i].first_patch >= 0 && runs[(size_t)i].first_patch + runs[(size_t)i].n <= h);
		CHECK(runs[(size_t)i].first_slot >= before && runs[(size_t)i].first_slot + runs[(size_t)i].n <= before + n);
		if (failures) return;
		for (int64_t j = 0; j < runs[(size_t)i].n; ++j) {
			CHECK(store[(size_t)(runs[(size_t)i].first_slot + j)] == -1);
			store[(size_t)(runs[(size_t)i].first_slot + j)] = runs[(size_t)i].first_patch + j;
		}
		if (i > 0) CHECK(runs[(size_t)i - 1].first_slot + runs[(size_t)i - 1].n < runs[(size_t)i].first_slot || runs[(size_t)i - 1].first_patch + runs[(size_t)i - 1].n < runs[(size_t)i].first_patch);
	}
	for (int64_t i = 0; i < h; ++i) CHECK(store[(size_t)(before + handed[(size_t)i])] == (keep[(size_t)i] ? i : -1));
	for (int64_t k = 0; k < n; ++k) if (status[(size_t)k] == 0) CHECK(store[(size_t)(before + k)] == -1);
	for (int64_t s = 0; s < before; ++s) CHECK(store[(size_t)s] == -1);
}

int main()
{
	step(0, {}, {}, {});
	step(5, { 4 }, { 0 }, { 1 });
	step(5, { 4 }, { 2 }, { 1 });
	step(0, { -1, 4, 4, 0, 4, -1 }, { 0, 0, 1, 3, 2, 3 }, { 1, 1, 1, 1, 1, 0 });
	step(3, { 4, 4, 4, 4 }, { 1, 2, 3, 1 }, { 1, 1, 1, 1 });                  // one run over everything
	step(3, { 4, 4, 4, 4 }, { 1, 2, 3, 1 }, { 1, 0, 1, 1 });                  // a host rule of NONE splits it
	step(1, { 4, 4, 4 }, { 0, 9, 0 }, { 1, 1, 1 });                           // an unknown status counts as handed back
	// every combination of status and host decision for six pairs
	for (int code = 0; code < 4096; ++code) {
		std::vector<int32_t> rule; std::vector<uint8_t> status, keeps;
		for (int k = 0, c = code; k < 6; ++k, c >>= 2) { status.push_back((uint8_t)(c & 3)); rule.push_back((c & 3) == 0 && (code >> 11 & 1) ? -1 : 4); keeps.push_back((uint8_t)((code >> k) & 1)); }
		step(code % 7, rule, status, keeps);
	}
	if (failures) return 1;
	std::printf("ok\n");
	return 0;
}
