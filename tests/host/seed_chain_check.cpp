// Stand-alone check of the host arithmetic of the seed search's chain mode (diamond_amd/csrc/seed_chain.h): the layout of the
// counter block and the readback, and the decoding of the status word into the point where the host-driven code continues.
// Built and run by tests/test_seed_chain_host.py (with the address and undefined-behaviour sanitizers); exit status 0 = pass.
#include <string.h>
#include <string>
#include <vector>
#include "../../diamond_amd/csrc/seed_chain.h"

using namespace dmnd;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static std::string name_of(unsigned long long status, unsigned long long done, int S, bool sorted)
{
	char buf[128];
	memset(buf, 0x7f, sizeof(buf));
	chain_path_name(buf, sizeof(buf), chain_plan(status, done, S, sorted), status);
	return buf;
}

static bool same(const ChainResume& x, bool hits_done, bool phase1_again, bool dirty, int64_t cap_total, int p2_first, bool p2_keep, int deferred_sid,
	unsigned long long deferred_n, int64_t hit_cap, int64_t def_cap, bool discard_pairs_time)
{
	return x.hits_done == hits_done && x.phase1_again == phase1_again && x.dirty == dirty && x.cap_total == cap_total && x.p2_first == p2_first && x.p2_keep == p2_keep
		&& x.deferred_sid == deferred_sid && x.deferred_n == deferred_n && x.hit_cap == hit_cap && x.def_cap == def_cap && x.discard_pairs_time == discard_pairs_time;
}

int main()
{
	// layout: the chain's words lie behind the five counters, clear of the phase ticks, for every shape count
	for (int S = 1; S <= 64; ++S) {
		CHECK(chain_ctr_status(S) > S + 4 && chain_ctr_done(S) > chain_ctr_status(S) && chain_ctr_done(S) < S + 8);
		CHECK(chain_ctr_survivors_of(S) == S + 16 && chain_ctr_words(S) == chain_ctr_survivors_of(S) + S);
		CHECK(chain_ret_header_bytes(S) % 64 == 0 && chain_ret_header_bytes(S) >= (size_t)chain_ctr_words(S) * 8 && chain_ret_header_bytes(S) < (size_t)chain_ctr_words(S) * 8 + 64);
		// the header is read and written through a vector of that many words without leaving it
		std::vector<unsigned long long> ret(chain_ret_header_bytes(S) / 8, 0);
		ret[chain_ctr_status(S)] = CHAIN_DEFERRED; ret[chain_ctr_done(S)] = (unsigned long long)(S - 1); ret[chain_ctr_survivors_of(S) + S - 1] = 7;
		const ChainPlan p = chain_plan(ret[chain_ctr_status(S)], ret[chain_ctr_done(S)], S, true);
		CHECK(p.point == CHAIN_FROM_DEFERRED && p.shape == S - 1);
	}
	// hits in the readback
	CHECK(chain_ret_hits(1 << 20, 24, 1 << 16) == (1 << 20) / 24);
	CHECK(chain_ret_hits(1 << 20, 24, 1000) == 1000);
	CHECK(chain_ret_hits(64, 24, 1000) == 2 && chain_ret_hits(23, 24, 1000) == 0 && chain_ret_hits(0, 24, 1000) == 0);
	CHECK(chain_ret_hits(-5, 24, 1000) == 0 && chain_ret_hits(100, 0, 1000) == 0 && chain_ret_hits(100, 24, 0) == 0);
	CHECK(chain_ret_hits(INT64_MAX, 24, INT64_MAX) == INT64_MAX / 24);
	// the plan: one flag each, then the precedence of several
	CHECK(chain_plan(0, 2, 2, true).point == CHAIN_COMPLETE);
	CHECK(chain_plan(0, 2, 2, false).point == CHAIN_FROM_SORT);
	CHECK(chain_plan(CHAIN_SORT_OVER, 2, 2, true).point == CHAIN_FROM_SORT);
	CHECK(chain_plan(CHAIN_MATCHED_OVER, 0, 2, true).point == CHAIN_FROM_PHASE1);
	CHECK(chain_plan(CHAIN_HITS_OVER, 1, 2, true).point == CHAIN_FROM_PHASE2 && chain_plan(CHAIN_HITS_OVER, 1, 2, true).shape == 0);
	CHECK(chain_plan(CHAIN_TILED, 1, 2, true).point == CHAIN_FROM_PAIRS && chain_plan(CHAIN_TILED, 1, 2, true).shape == 1);
	CHECK(chain_plan(CHAIN_SURVIVORS_OVER, 0, 2, true).point == CHAIN_FROM_PAIRS && chain_plan(CHAIN_SURVIVORS_OVER, 0, 2, true).shape == 0);
	CHECK(chain_plan(CHAIN_DEFERRED, 1, 2, true).point == CHAIN_FROM_DEFERRED);
	CHECK(chain_plan(CHAIN_MATCHED_OVER | CHAIN_TILED | CHAIN_SORT_OVER, 0, 2, true).point == CHAIN_FROM_PHASE1);
	CHECK(chain_plan(CHAIN_HITS_OVER | CHAIN_SORT_OVER, 0, 2, true).point == CHAIN_FROM_PHASE2);
	CHECK(chain_plan(CHAIN_DEFERRED | CHAIN_SORT_OVER, 0, 1, true).point == CHAIN_FROM_DEFERRED);
	// a `done` word outside the shapes (never written by the kernels) does not lead outside them
	CHECK(chain_plan(CHAIN_DEFERRED, ~0ull, 3, true).shape == 2 && chain_plan(CHAIN_TILED, 3, 3, true).shape == 2);
	// the continuation (chain_resume): one check per point, every field. Two shapes; the chain ran with the capacities 1000 (joined
	// positions), 50 (hits) and 20 (deferred pairs) and left 300 + 400 joined positions, 40 hits and 7 deferred pairs
	{
		const int S = 2;
		unsigned long long r[2 * 2 + 16] = { 0 };
		r[0] = 300; r[1] = 700; r[S] = 40; r[S + 1] = 7;
		auto resume = [&](unsigned long long status, unsigned long long done) { return chain_resume(chain_plan(status, done, S, true), r, S, 1000, 50, 20); };
		CHECK(same(ChainResume(), false, true, false, 0, 0, false, -1, 0, 0, 0, false));          // no chain: everything is the host's
		CHECK(same(resume(0, 2), true, false, false, 1000, 0, false, -1, 0, 0, 0, false));         // CHAIN_COMPLETE
		CHECK(same(resume(CHAIN_SORT_OVER, 2), false, false, false, 1000, 2, true, -1, 0, 50, 20, false));      // CHAIN_FROM_SORT: no shape is left
		CHECK(same(resume(CHAIN_TILED, 1), false, false, false, 1000, 1, true, -1, 0, 50, 20, false));          // CHAIN_FROM_PAIRS
		CHECK(same(resume(CHAIN_SURVIVORS_OVER, 0), false, false, false, 1000, 0, true, -1, 0, 50, 20, false));
		CHECK(same(resume(CHAIN_DEFERRED, 0), false, false, false, 1000, 1, true, 0, 7, 50, 20, false));        // CHAIN_FROM_DEFERRED: the list is complete
		CHECK(same(resume(CHAIN_DEFERRED, 1), false, false, false, 1000, 2, true, 1, 7, 50, 20, false));
		r[S + 1] = 20;                                       // ... exactly full is complete
		CHECK(same(resume(CHAIN_DEFERRED, 1), false, false, false, 1000, 2, true, 1, 20, 50, 20, false));
		r[S + 1] = 21;                                       // ... over the capacity: phase 2 again with a grown list, nothing kept
		CHECK(same(resume(CHAIN_DEFERRED, 1), false, false, false, 1000, 0, false, -1, 21, 0, 21 + 1024, true));
		r[S] = 51;                                           // CHAIN_FROM_PHASE2: the hit list grows, nothing kept
		CHECK(same(resume(CHAIN_HITS_OVER, 1), false, false, false, 1000, 0, false, -1, 0, 51 + 1024, 0, true));
		r[1] = 1600;                                         // CHAIN_FROM_PHASE1: lists for the 1600 positions counted plus an eighth
		CHECK(same(resume(CHAIN_MATCHED_OVER, 0), false, true, true, 1600 + 200 + 1024, 0, false, -1, 0, 0, 0, true));
		// several flags: the earliest point wins and takes nothing from the later ones (no grown hit or deferred list behind phase 1,
		// no kept shapes behind phase 2)
		CHECK(same(resume(CHAIN_MATCHED_OVER | CHAIN_HITS_OVER | CHAIN_DEFERRED | CHAIN_TILED | CHAIN_SORT_OVER, 1), false, true, true, 1600 + 200 + 1024, 0, false, -1, 0, 0, 0, true));
		CHECK(same(resume(CHAIN_HITS_OVER | CHAIN_DEFERRED | CHAIN_TILED | CHAIN_SORT_OVER, 1), false, false, false, 1000, 0, false, -1, 0, 51 + 1024, 0, true));
		CHECK(same(resume(CHAIN_SURVIVORS_OVER | CHAIN_DEFERRED | CHAIN_SORT_OVER, 1), false, false, false, 1000, 1, true, -1, 0, 50, 20, false));
	}
	// names: what the DMND_TRACE summary prints and the tests read; the longest one fits the caller's 128 bytes
	CHECK(name_of(0, 1, 1, true) == "chain");
	CHECK(name_of(CHAIN_MATCHED_OVER, 0, 2, true) == "chain, then host from phase 1 (joined positions over capacity)");
	CHECK(name_of(CHAIN_SURVIVORS_OVER, 0, 2, true) == "chain, then host from the pair filter of shape 0 (survivors over capacity)");
	CHECK(name_of(CHAIN_TILED, 63, 64, true) == "chain, then host from the pair filter of shape 63 (tiled filter)");
	CHECK(name_of(CHAIN_DEFERRED, 1, 2, true) == "chain, then host from the deferred pass of shape 1");
	CHECK(name_of(CHAIN_HITS_OVER, 0, 2, true) == "chain, then host from phase 2 (hits over capacity)");
	CHECK(name_of(CHAIN_SORT_OVER, 2, 2, true) == "chain, then host from the hit sort");
	for (unsigned long long status = 0; status < 64; ++status)
		for (unsigned long long done = 0; done <= 64; done += 63) {
			char small[8];
			chain_path_name(small, sizeof(small), chain_plan(status, done, 64, true), status);      // truncated, terminated
			CHECK(strlen(small) < sizeof(small));
			CHECK(name_of(status, done, 64, true).size() < 127);
		}
	if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
	printf("seed_chain_check ok\n");
	return 0;
}
