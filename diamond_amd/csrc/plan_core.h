// plan_core.h -- the arithmetic that translated queries (six contexts per read) add to the device planner and the device half of the
// extension stage, HIP-free: one statement of it for the kernels (plan_kernels.hip, extend_kernels.hip) and the CPU tests
// (tests/emu/plan_core_emu.cpp).
//   the sort key that brings a call's seed hits from (context, location, seed offset) order into (read, target, ...) order: the
//   reference groups a read's hits by target over all six frames (src/align/load_hits.h:44-127)
//   the best HSP of a target over the DpTargets of all its contexts (src/align/target.h:105-113, src/basic/match.h:199)
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

}  // namespace dmnd
