// tests/emu/top_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The --top arithmetic of diamond_amd/csrc/top_core.h (what the host path's output_range / append_hits and the --top kernels of the
// device half compute) against a literal transcription of the host path's earlier statement of it, for tests/test_top_core.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include "../../diamond_amd/csrc/top_core.h"
#include "../../diamond_amd/csrc/evalue.h"
#include "../../diamond_amd/csrc/score_matrices.h"

using namespace dmnd;

namespace {
Evaluer evaluer_of(double lambda, double K)
{
	Evaluer e{};
	e.lambda = lambda; e.K = K; e.ln_k = std::log(K);
	return e;
}
}

// Over all pairs (best, score) with 1 <= score <= best <= max_score, for one --top percentage:
//   out[0] pairs where top_pass differs from `bitscore(score) >= max((1 - top/100) * bitscore(best), 1.0)` with Evaluer::bitscore
//   out[1] scores 1 .. max_score where top_append_floor differs from (int)((1 - top/100) * score)
//   out[2] pairs where top_near fires
//   out[3] pairs checked
// and the smallest relative distance of a bit score to a cutoff above the 1.0 floor (score != best), with the pair it was found at
extern "C" void emu_top_check(double top, double lambda, double K, int max_score, int64_t* out, double* closest, int* closest_pair)
{
	const Evaluer ev = evaluer_of(lambda, K);
	const TopCfg tc = top_cfg(top, ev.lambda, ev.ln_k);
	out[0] = out[1] = out[2] = out[3] = 0;
	*closest = 1e300; closest_pair[0] = closest_pair[1] = 0;
	for (int best = 1; best <= max_score; ++best) {
		const double cutoff = std::max((1.0 - top / 100.0) * ev.bitscore(best), 1.0);
		for (int score = 1; score <= best; ++score) {
			const bool want = ev.bitscore(score) >= cutoff;
			out[0] += top_pass(tc, score, best) != want;
			out[2] += top_near(tc, score, best);
			++out[3];
			if (score != best && cutoff > 1.0) {
				const double b = ev.bitscore(score), rel = std::fabs(b - cutoff) / std::fmax(std::fabs(b), std::fabs(cutoff));
				if (rel < *closest) { *closest = rel; closest_pair[0] = best; closest_pair[1] = score; }
			}
		}
	}
	for (int score = 1; score <= max_score; ++score)
		out[1] += top_append_floor(tc, score) != (int)((1.0 - top / 100.0) * score) || top_append(tc, score, score) != (score >= (int)((1.0 - top / 100.0) * score));
}

// single values, for hand-made cases
extern "C" int emu_top_pass(double top, double lambda, double K, int score, int best) { return top_pass(top_cfg(top, lambda, std::log(K)), score, best); }
extern "C" int emu_top_near(double top, double lambda, double K, int score, int best) { return top_near(top_cfg(top, lambda, std::log(K)), score, best); }
extern "C" int emu_top_append(double top, double lambda, double K, int max_v, int min_a) { return top_append(top_cfg(top, lambda, std::log(K)), max_v, min_a); }
extern "C" double emu_top_bits(double lambda, double K, int score) { return top_bits(top_cfg(0.0, lambda, std::log(K)), score); }

// the project's Gumbel constants of BLOSUM62 with gap penalties 11 / 1 (score_matrices.h), what Evaluer::init reads; 0 = found
extern "C" int emu_top_blosum62_constants(double* lambda, double* K)
{
	for (const GumbelRow& r : BLOSUM62_ROWS)
		if (r.gap_open == 11 && r.gap_extend == 1) { *lambda = r.lambda; *K = r.K; return 0; }
	return 1;
}
