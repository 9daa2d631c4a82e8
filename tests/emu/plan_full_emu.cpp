// tests/emu/plan_full_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The full-matrix arithmetic of diamond_amd/csrc/plan_core.h (Extension::Mode::FULL: the band and the DP size of a unit, the sum of a
// (read, target) pair over its units) for tests/test_plan_full.py: the statements plan_full_kernel, plan_pairs_kernel and
// ext_mark_kernel compile, run on the CPU.
#include <cstdint>
#include "../../diamond_amd/csrc/plan_core.h"

using namespace dmnd;

extern "C" void emu_full_matrix_band(int qlen, int tlen, int* d_begin, int* d_end)
{
	const FullBand b = full_matrix_band(qlen, tlen);
	*d_begin = b.d_begin; *d_end = b.d_end;
}
extern "C" int64_t emu_full_matrix_dp_size(int qlen, int tlen) { return full_matrix_dp_size(qlen, tlen); }

// One (read, target) pair of a translated call in Mode::FULL as plan_full_kernel + plan_pairs_kernel plan it. The pair's seed hits
// come frame after frame (frame[k] ascending, score[k]); every frame with a hit is one unit with one band over the matrix of ITS
// context (qlen[frame]) and the target. Out: per unit its band and context (band_query = query0 + frame), the pair's band count, its
// ranking score and the ungapped score of context 0. Returns the number of units, -1 if the pair would go to the host.
extern "C" int emu_plan_full_pair(const int* frame, const int* score, int n_hits, const int* qlen, int tlen, uint32_t query0, uint32_t limit,
	int* d_begin, int* d_end, uint32_t* band_query, uint32_t* n_bands, int* pair_score, int* ungapped0)
{
	PairSum s = pair_sum_begin();
	int n_units = 0;
	for (int b = 0; b < n_hits;) {
		int e = b, best = 0;
		while (e < n_hits && frame[e] == frame[b]) { if (score[e] > best) best = score[e]; ++e; }
		const FullBand fb = full_matrix_band(qlen[frame[b]], tlen);
		d_begin[n_units] = fb.d_begin; d_end[n_units] = fb.d_end; band_query[n_units] = query0 + (uint32_t)frame[b];
		pair_sum_add(s, best, (uint32_t)frame[b], 1u, false);
		++n_units;
		b = e;
	}
	pair_sum_end(s, limit);
	*n_bands = s.n_bands; *pair_score = s.score; *ungapped0 = s.ungapped0;
	return s.on_host ? -1 : n_units;
}
