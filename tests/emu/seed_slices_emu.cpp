// CPU side of tests/test_seed_slices_emu.py: the slice identity of the sliced long-seed stream and its routing rule
// (csrc/seed_slices_core.h), the latter against the plain stream's rule (seed_key_at inside the block's window range).
#include "../../diamond_amd/csrc/seed_slices_core.h"

using namespace dmnd;

// per key: hash a and level-1 word (no key classes); returns the slice count exponent of this geometry (-1: none)
extern "C" int emu_slice_words(const uint64_t* keys, int64_t n, int slot_bits, uint32_t words, uint32_t* h_out, uint32_t* word_out)
{
	const uint32_t hmask = bm1_hmask_of(slot_bits, 0);
	for (int64_t i = 0; i < n; ++i) {
		h_out[i] = seed_hash_a(keys[i]);
		word_out[i] = bm1_word_of_key(h_out[i], keys[i], 0, hmask, words);
	}
	return seed_slice_bits(words, slot_bits, SEED_SLICE_MAX_WORDS);
}

// Routing bytes of the windows [t_begin & ~15, ...) of a block as the cache build computes them -- class nibbles and flag words per
// group of 16 letters (seed_codes_kernel's), then seed_route_group -- and as the plain stream decides them: a window inside
// [t_begin, t_end) whose seed_key_at is valid, routed by the hash of that key. n_out = seed_ref_windows bytes each.
extern "C" int64_t emu_route_block(const SeedParams* cp, int sid, const int8_t* tdata, int64_t t_begin, int64_t t_end, int slice_bits, uint8_t* routed, uint8_t* plain)
{
	const SeedParams& c = *cp;
	const int64_t base = t_begin & ~(int64_t)15, n = seed_ref_windows(t_begin, t_end), groups = n / 16 + 2;
	uint64_t* codes = new uint64_t[groups];
	uint32_t* flags = new uint32_t[groups];
	for (int64_t g = 0; g < groups; ++g) {
		uint64_t code = 0;
		uint32_t delim = 0, bad = 0;
		for (int j = 0; j < 16; ++j) {
			const uint32_t l = (uint32_t)tdata[base + 16 * g + j] & LETTER_MASK;
			const uint32_t r = c.reduction[l] == L_MASK ? 15u : (uint32_t)c.reduction[l];
			code |= (uint64_t)r << (4 * j);
			delim |= (l == L_DELIM ? 1u : 0u) << j;
			bad |= (r == 15u ? 1u : 0u) << j;
		}
		codes[g] = code; flags[g] = delim | (bad << 16);
	}
	uint64_t care64 = 0;
	for (int k = 0; k < c.shape_weight[sid]; ++k) care64 |= (uint64_t)15 << (4 * c.shape_pos[sid][k]);
	for (int64_t g = 0; g < n / 16; ++g) {
		const int64_t p0 = base + 16 * g;
		seed_route_group(codes[g], codes[g + 1], flags[g], flags[g + 1], t_begin - p0, t_end - p0, c.shape_len[sid], c.shape_mask[sid], care64, slice_bits, routed + 16 * g);
		for (int w = 0; w < 16; ++w) {
			const int64_t p = p0 + w;
			uint64_t key;
			plain[16 * g + w] = p >= t_begin && p < t_end && seed_key_at(c, sid, tdata + p, key) ? (uint8_t)seed_slice_of(seed_hash_a(key), slice_bits) : (uint8_t)SEED_ROUTE_NONE;
		}
	}
	delete[] codes; delete[] flags;
	return n;
}
