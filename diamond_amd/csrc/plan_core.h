// plan_core.h -- the arithmetic that translated queries (six contexts per read) add to the device planner and the device half of the
// extension stage, HIP-free: one statement of it for the kernels (plan_kernels.hip, extend_kernels.hip) and the CPU tests
// (tests/emu/plan_core_emu.cpp).
//   the sort key that brings a call's seed hits from (context, location, seed offset) order into (read, target, ...) order: the
//   reference groups a read's hits by target over all six frames (src/align/load_hits.h:44-127)
//   the best HSP of a target over the DpTargets of all its contexts (src/align/target.h:105-113, src/basic/match.h:199)
//   the sum of a (read, target) pair over its (context, target) units
// and the arithmetic of full-matrix targets (Extension::Mode::FULL): band and DP size of a unit (tests/emu/plan_full_emu.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DMND_PLAN_HD __host__ __device__
#else
#define DMND_PLAN_HD
#endif

namespace dmnd {

// bits that hold every value below n (at least one)
inline int plan_bits_below(uint64_t n) { int b = 1; while (b < 64 && ((uint64_t)1 << b) < n) ++b; return b; }

// The key of a seed hit: its read above its target. Reads and targets are block sequence numbers below 2^32, so the two fields come to
// at most 64 bits whatever the blocks' sizes -- the key bounds no block, and a stable radix sort over its target_bits + read_bits low
// bits leaves the hits of a (read, target) pair together, in their earlier order: frame, location, seed offset.
struct PlanKeyBits { int target_bits, read_bits; };
inline PlanKeyBits plan_key_bits(uint64_t n_reads, uint64_t n_targets) { return PlanKeyBits{ plan_bits_below(n_targets), plan_bits_below(n_reads) }; }
DMND_PLAN_HD inline uint64_t plan_pair_key(uint32_t read, uint32_t target, int target_bits) { return ((uint64_t)read << target_bits) | (uint64_t)target; }
DMND_PLAN_HD inline uint32_t plan_key_read(uint64_t key, int target_bits) { return (uint32_t)(key >> target_bits); }
DMND_PLAN_HD inline uint32_t plan_key_target(uint64_t key, int target_bits) { return (uint32_t)(key & (((uint64_t)1 << target_bits) - 1)); }

// Target::add_hit + inner_culling over the reported DpTargets of a target, taken contexts ascending: the best context is the first one
// that reaches the highest score; inside it the higher score wins, of equal ones the band that starts first. True: the DpTarget
// (score, context, d_begin) replaces the best one so far. With one context that is (score descending, d_begin ascending).
DMND_PLAN_HD inline bool best_hsp_replaces(int score, int64_t context, int d_begin, int best_score, int64_t best_context, int best_d_begin)
{
	return score > best_score || (score == best_score && context == best_context && d_begin < best_d_begin);
}

// Extension::Mode::FULL (--ext full, and the final pass of --global-ranking): a (context, target) unit with a seed hit gets ONE
// DpTarget over the whole matrix, no x-drop stage, no chaining (src/align/ungapped.cpp:70-75, gapped_score.cpp:123-130). Its band in
// the diagonal coordinates of the banded sweeps (d = i - j) is every diagonal the matrix has; its DP size, what config.max_swipe_dp
// is held against, is the matrix itself (DP::Flags::FULL_MATRIX, src/dp/dp.h:121-124) and not the band's columns x width.
struct FullBand { int32_t d_begin, d_end; };
DMND_PLAN_HD inline FullBand full_matrix_band(int qlen, int tlen) { return FullBand{ -(tlen - 1), qlen }; }
DMND_PLAN_HD inline int64_t full_matrix_dp_size(int qlen, int tlen) { return (int64_t)qlen * (int64_t)tlen; }

// A (read, target) pair of a translated call summed up over its (context, target) units, which arrive contexts ascending: the bands of
// all units (they lie one after the other in the band list), the ranking score = the best over all frames, the score that travels into
// the record = context 0's (0 without a hit there); one unit left to the host leaves the pair to the host. limit: a band count from
// which on the pair is left to the host (the planner's PLAN_NEED_CHAIN).
struct PairSum { uint32_t n_bands; int score, ungapped0; bool on_host; };
DMND_PLAN_HD inline PairSum pair_sum_begin() { return PairSum{ 0u, 0, 0, false }; }
DMND_PLAN_HD inline void pair_sum_add(PairSum& s, int unit_score, uint32_t unit_context, uint32_t unit_bands, bool unit_on_host)
{
	if (unit_score > s.score) s.score = unit_score;
	if (unit_context == 0) s.ungapped0 = unit_score;
	if (unit_on_host) s.on_host = true; else s.n_bands += unit_bands;
}
DMND_PLAN_HD inline void pair_sum_end(PairSum& s, uint32_t limit) { if (s.n_bands >= limit) s.on_host = true; }

}  // namespace dmnd
