// tests/emu/rank_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The arithmetic of diamond_amd/csrc/rank_core.h (the device form of the global ranking step) for tests/test_rank_core.py: the walk of
// one group exactly as the kernels run it -- stable sort by (diagonal, j), one rank_walk_run per run of equal diagonal, a maximum over
// the packed results of the runs -- the key packing and the record's cast.
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>
#include "../../diamond_amd/csrc/rank_core.h"

using namespace dmnd;

// One group. Per hit, in the planner's order (frame, then location): i, j (relative to the target), frame and its x-drop record
// (left, right, score). reverse != 0: the runs are reduced last to first (the result must not depend on it).
// out: [0] record score (uint16 cast), [1] context, [2] hits that were not skipped, [3] the uncast score
extern "C" void emu_rank_walk_group(int n, const int32_t* i, const int32_t* j, const int32_t* frame, const int32_t* left, const int32_t* right, const int32_t* score,
	int reverse, int64_t* out)
{
	std::vector<uint32_t> order((size_t)n);
	std::iota(order.begin(), order.end(), 0u);
	// what the device does: a stable pass by j, then a stable sort by the (group, diagonal) key
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return j[a] < j[b]; });
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rank_key(7, i[a] - j[a]) < rank_key(7, i[b] - j[b]); });
	std::vector<int32_t> sj((size_t)n), sj_end((size_t)n), ss((size_t)n);
	std::vector<uint64_t> keys((size_t)n);
	for (int p = 0; p < n; ++p) {
		const uint32_t k = order[(size_t)p];
		const RankSeg s = rank_seg(i[k], j[k], XdropSeg{ left[k], right[k], score[k] });
		sj[(size_t)p] = j[k]; sj_end[(size_t)p] = s.j_end; ss[(size_t)p] = s.score;
		keys[(size_t)p] = rank_key(7, s.diag);
	}
	std::vector<std::pair<uint32_t, uint32_t>> runs;
	for (uint32_t b = 0; b < (uint32_t)n;) {
		uint32_t e = b + 1;
		while (e < (uint32_t)n && keys[e] == keys[b]) ++e;
		runs.emplace_back(b, e);
		b = e;
	}
	if (reverse) std::reverse(runs.begin(), runs.end());
	uint64_t best = 0;
	int64_t counted = 0;
	for (const auto& r : runs) {
		int32_t s; uint32_t pos, c;
		rank_walk_run(sj.data(), sj_end.data(), ss.data(), r.first, r.second, s, pos, c);
		best = std::max(best, rank_pack_best(s, pos));
		counted += c;
	}
	out[0] = rank_record_score(rank_best_score(best));
	out[1] = n > 0 ? frame[order[rank_best_pos(best)]] : -1;
	out[2] = counted;
	out[3] = rank_best_score(best);
}

extern "C" uint64_t emu_rank_key(uint32_t group, int32_t diag) { return rank_key(group, diag); }
extern "C" uint32_t emu_rank_key_group(uint64_t key) { return rank_key_group(key); }
extern "C" int32_t emu_rank_key_diag(uint64_t key) { return rank_key_diag(key); }
extern "C" int emu_rank_skips(int32_t d_diag, int32_t d_j_end, int32_t diag, int32_t j) { return rank_skips(d_diag, d_j_end, diag, j) ? 1 : 0; }
extern "C" uint64_t emu_rank_cut_key(uint32_t query, uint16_t score) { return rank_cut_key(query, score); }
extern "C" int emu_rank_xdrop(double K, double lambda) { return rank_xdrop(K, lambda); }
