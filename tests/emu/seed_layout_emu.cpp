// tests/emu/seed_layout_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The layout functions of the query side (diamond_amd/csrc/seed_core.h seed_order, bm1_word_of_key / _of_top, bm2_word_of_top)
// evaluated on the CPU for a batch of keys, so that tests/test_seed_layout_emu.py can check what the sort-driven build relies on.
#include <cstdint>
#include "../../diamond_amd/csrc/seed_core.h"

using namespace dmnd;

// per key: t (sort key = home slot), class, level-1 word in the stream's form and as a function of t, level-2 word
extern "C" void emu_seed_layout(const uint64_t* keys, int64_t n, int slot_bits, int classes, uint32_t bm1_words, int bm_log2,
	uint32_t* top, uint32_t* cls, uint32_t* w1_key, uint32_t* w1_top, uint32_t* w2)
{
	const uint32_t hmask = bm1_hmask_of(slot_bits, classes);
	for (int64_t i = 0; i < n; ++i) {
		const uint32_t h = seed_hash_a(keys[i]);
		const uint32_t t = seed_order(h, keys[i], classes) >> (32 - slot_bits);
		top[i] = t;
		cls[i] = seed_class(keys[i]);
		w1_key[i] = bm1_word_of_key(h, keys[i], classes, hmask, bm1_words);
		w1_top[i] = bm1_word_of_top(t, slot_bits, bm1_words);
		w2[i] = bm2_word_of_top(t, slot_bits, bm_log2);
	}
}
