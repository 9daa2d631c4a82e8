// tests/emu/plan_core_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The arithmetic of diamond_amd/csrc/plan_core.h (the (read, target) sort key of the device planner's re-sort of translated hits,
// the best-HSP rule over the contexts of a read) for tests/test_plan_core.py.
#include <cstdint>
#include "../../diamond_amd/csrc/plan_core.h"

using namespace dmnd;

extern "C" int emu_plan_bits_below(uint64_t n) { return plan_bits_below(n); }
extern "C" void emu_plan_key_bits(uint64_t n_reads, uint64_t n_targets, int* target_bits, int* read_bits)
{
	const PlanKeyBits b = plan_key_bits(n_reads, n_targets);
	*target_bits = b.target_bits; *read_bits = b.read_bits;
}
extern "C" uint64_t emu_plan_pair_key(uint32_t read, uint32_t target, int target_bits) { return plan_pair_key(read, target, target_bits); }
extern "C" uint32_t emu_plan_key_read(uint64_t key, int target_bits) { return plan_key_read(key, target_bits); }
extern "C" uint32_t emu_plan_key_target(uint64_t key, int target_bits) { return plan_key_target(key, target_bits); }

// the best of n DpTargets (score, context, d_begin), taken in the order given (contexts ascending): its index, -1 for none
extern "C" int emu_best_hsp(const int* score, const int64_t* context, const int* d_begin, int n)
{
	int best = -1;
	for (int i = 0; i < n; ++i)
		if (best < 0 || best_hsp_replaces(score[i], context[i], d_begin[i], score[best], context[best], d_begin[best])) best = i;
	return best;
}
