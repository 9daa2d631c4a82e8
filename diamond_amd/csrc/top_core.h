// top_core.h -- the arithmetic of the --top culling (config.toppercent), HIP-free: one statement of it for the host path
// (extend_host.hip output_range, append_hits), the --top kernels of the device half (extend_kernels.hip) and the CPU tests
// (tests/emu/top_emu.cpp). --top never orders by e-value: a list is cut by a threshold against the bit score of its best
// entry, and a ranking chunk is appended by an integer comparison against the lowest score that survived the cut.
//   top_cutoff_score<double> / <int>     src/basic/config.h:428-454
//   output_range, append_hits            src/align/culling.cpp:92-144
// The host's value is the one the output is judged by, so the bit score is spelled operation by operation -- a product, a
// difference, a quotient, each rounded once -- and no compiler may contract the first two into a fused multiply-add.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DMND_TOP_HD __host__ __device__
#else
#define DMND_TOP_HD
#endif

namespace dmnd {

// f = 1 - top / 100, computed once on the host; lambda and ln K of the scoring system (evalue.h)
struct TopCfg { double f, lambda, ln_k; };

inline TopCfg top_cfg(double top_percent, double lambda, double ln_k) { return TopCfg{ 1.0 - top_percent / 100.0, lambda, ln_k }; }

// ScoreMatrix::bitscore of an integer raw score (Evaluer::bitscore, evalue.h)
DMND_TOP_HD inline double top_bits(const TopCfg& c, int score)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double p = c.lambda * (double)score;
	const double d = p - c.ln_k;
	return d / 0.69314718055994530941723212145818;
}

// the bit score an entry needs beside a best entry of raw score `best`: max(f x bits(best), 1.0)
DMND_TOP_HD inline double top_cutoff(const TopCfg& c, int best)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double x = c.f * top_bits(c, best);
	return x < 1.0 ? 1.0 : x;
}

// the bit-score cutoff test of output_range: the entry stays in a list whose best entry has raw score `best`
DMND_TOP_HD inline bool top_pass(const TopCfg& c, int score, int best) { return top_bits(c, score) >= top_cutoff(c, best); }

// the integer append test of append_hits: a chunk whose best score is max_v joins aligned targets whose lowest score is min_a.
// One double product, truncated.
DMND_TOP_HD inline int top_append_floor(const TopCfg& c, int min_a)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double x = c.f * (double)min_a;
	return (int)x;
}
DMND_TOP_HD inline bool top_append(const TopCfg& c, int max_v, int min_a) { return max_v >= top_append_floor(c, min_a); }

// The entry's bit score lies within 1e-9 relative of the cutoff (the tolerance of the device half's e-value decisions, ext_near):
// the device half does not decide such a query, the host redoes it. Never for the best entry itself (f <= 1: it always stays) and
// never where the cutoff is the 1.0 floor, a constant that is the same on both sides.
DMND_TOP_HD inline bool top_near(const TopCfg& c, int score, int best)
{
	if (score == best) return false;
	const double cut = top_cutoff(c, best);
	if (cut <= 1.0) return false;
	const double b = top_bits(c, score);
	return fabs(b - cut) <= 1e-9 * fmax(fabs(b), fabs(cut));
}

}  // namespace dmnd
