// linsearch_core.h -- the rules of the linearised search (--linsearch: "only consider seed hits against longest target for
// identical seeds", basic/config.cpp:425), HIP-free: one statement of them for the seed stage's reduction and pair filters
// (seed_kernels.hip), the checks of dmnd_seed_search (seed_api.hip), the CLI (cli.cpp) and the CPU tests (tests/emu/linsearch_emu.cpp).
//   stage 1 of a linearised shape          src/search/hamming/kernel_lin.h:132-153 (stage1_target_lin; dispatch stage1_2.cpp:38-39,52)
//   the order inside a joined group        src/util/algo/hash_join.h:98-111,157-169 (input order: ascending block position)
//   stage 2 of a batch of one              src/search/stage2.h:101,132 (the saturation rule of larger batches: seed_core.h, simd_batch_size_sorted)
//   the weight bound                       src/search/setup.cpp:365-366
//   the length sort of the reference       src/run/double_indexed.cpp:112-115 (Block::length_sorted; length_ratio_core.h)
// The reference compares all query positions of a seed with s[0] only, the first reference position of the joined group. Groups
// keep the block's order, so s[0] is the smallest position of the reference block that carries the seed -- after the length sort
// a position in the longest such target. Here the joined records (slot, position) of a shape arrive in no particular order, so
// the rule is stated over the set: a record takes part iff its position is the minimum over the records of its slot.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DMND_LIN_HD __host__ __device__
#else
#define DMND_LIN_HD
#endif

namespace dmnd {

// the per-slot state before any record of the slot has been seen: above every block position
constexpr int64_t LIN_NO_POSITION = INT64_MAX;

// selection rule, step 1: the state of a slot after one more of its records (commutative and associative: arrival order is immaterial)
DMND_LIN_HD inline int64_t lin_first_update(int64_t first_so_far, int64_t position) { return position < first_so_far ? position : first_so_far; }

// selection rule, step 2: whether a joined record reaches the Hamming test, `first` being the reduced state of its slot
DMND_LIN_HD inline bool lin_record_selected(int64_t position, int64_t first) { return position == first; }

// Scoring rule of a batch of one subject (search/stage2.h: a batch below four takes the scalar window score): the score is never
// saturated at 255, so nothing waits for the second pass that counts batch mates. lin = the switch.
DMND_LIN_HD inline bool lin_score_is_deferred(int score, bool lin) { return score > 255 && !lin; }

// ... and the left-most filter is not applied to such a pair (stage2.h:101,132)
DMND_LIN_HD inline bool lin_applies_left_most(bool lin) { return !lin; }

// search/setup.cpp:365-366: "Linearization is only supported for seed shapes of weight >= 10."
enum { LIN_MIN_SHAPE_WEIGHT = 10 };
DMND_LIN_HD inline bool lin_shape_weight_ok(int weight) { return weight >= LIN_MIN_SHAPE_WEIGHT; }

// host form of the reduction over n records: first[slot] for every slot that occurs (first: n_slots entries, any content)
inline void lin_first_positions(const uint32_t* slot, const int64_t* position, int64_t n, int64_t* first)
{
	for (int64_t i = 0; i < n; ++i) first[slot[i]] = LIN_NO_POSITION;
	for (int64_t i = 0; i < n; ++i) first[slot[i]] = lin_first_update(first[slot[i]], position[i]);
}

}  // namespace dmnd
