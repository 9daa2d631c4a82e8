// CPU side of tests/test_seed_filter_rule_emu.py: the size of the level-1 filter that a search on the sliced long-seed stream builds
// (csrc/seed_slices_core.h: seed_slices_filter_words) and the slice count seed_slice_bits finds for it.
#include "../../diamond_amd/csrc/seed_slices_core.h"
#include <vector>

using namespace dmnd;

// words of the filter; *k3: 0 / 2 (bm1_bits) where the rule sets the bits per seed, -1 where it leaves the default geometry's
extern "C" uint64_t emu_slices_filter_words(uint64_t nq_pos, int slot_bits, uint64_t bm_words, uint64_t default_words, uint32_t max_slice_words, uint64_t forced_words, int* k3)
{
	uint32_t k = 0xffffffffu;
	const uint64_t w = seed_slices_filter_words(nq_pos, slot_bits, bm_words, default_words, max_slice_words, forced_words, &k);
	*k3 = k == 0xffffffffu ? -1 : (int)k;
	return w;
}

extern "C" int emu_slice_bits(uint64_t words, int slot_bits, uint32_t max_words) { return seed_slice_bits(words, slot_bits, max_words); }

extern "C" uint32_t emu_bm1_bits(uint32_t h, uint32_t k3) { return bm1_bits(h, k3); }

// share of n_probes random keys that a level-1 filter of `words` words over n_seeds other random keys lets pass (hash a of
// splitmix64 keys; word and bits as the build and the streams take them, without key classes)
extern "C" double emu_bm1_false_positive_rate(int64_t n_seeds, int64_t n_probes, uint32_t words, int slot_bits, uint32_t k3)
{
	std::vector<uint32_t> bm(words, 0u);
	const uint32_t hmask = bm1_hmask_of(slot_bits, 0);
	uint64_t state = 0x243F6A8885A308D3ull;
	auto next = [&]() {
		uint64_t z = (state += 0x9E3779B97F4A7C15ull);
		z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
		return seed_hash_a(z ^ (z >> 31));
	};
	for (int64_t i = 0; i < n_seeds; ++i) { const uint32_t h = next(); bm[seed_slice_word(h, hmask, words)] |= bm1_bits(h, k3); }
	int64_t pass = 0;
	for (int64_t i = 0; i < n_probes; ++i) { const uint32_t h = next(), need = bm1_bits(h, k3); pass += (bm[seed_slice_word(h, hmask, words)] & need) == need; }
	return (double)pass / (double)n_probes;
}

extern "C" uint64_t emu_slices_most_words() { return (uint64_t)SEED_SLICE_MAX_WORDS << SEED_SLICE_MAX_BITS; }
