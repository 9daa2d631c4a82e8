// CPU side of tests/test_seed_slices_hash_emu.py: the hashes the sliced long-seed stream keeps beside its list entries
// (csrc/seed_slices_core.h: seed_ref_hash_entry, seed_slice_word) against the keys of the windows themselves (seed_key_at).
#include "../../diamond_amd/csrc/seed_slices_core.h"
#include <vector>

using namespace dmnd;

// The cache of one shape over a block as the build makes it -- class nibbles and flag words per group of 16 letters, routing bytes
// (seed_route_group), the windows listed slice by slice in ascending order (a stable pass, the windows that are no seeds last), the
// hash of every list entry (seed_ref_hash_entry) -- and then, for EVERY listed seed window k of slice s, against the window's own key
// (seed_key_at, h = seed_hash_a(key)):
//   bad[0]  the stored hash is not h
//   bad[1]  the word probed from the stored hash is not bm1_word_of_key(h, key, classes = 0)
//   bad[2]  bm1_bits of the stored hash are not those of h
//   bad[3]  that word lies outside slice s, or the window is not one the plain rule probes
// list_out / hash_out: seed_ref_windows words each, counts_out: 2^slice_bits. Returns the number of seed windows checked.
extern "C" int64_t emu_hash_block(const SeedParams* cp, int sid, const int8_t* tdata, int64_t t_begin, int64_t t_end, int slice_bits, int slot_bits, uint32_t words, uint32_t k3,
	int64_t* bad, uint32_t* list_out, uint32_t* hash_out, uint32_t* counts_out)
{
	const SeedParams& c = *cp;
	const int64_t base = t_begin & ~(int64_t)15, n = seed_ref_windows(t_begin, t_end), groups = n / 16 + 2;
	std::vector<uint64_t> codes(groups);
	std::vector<uint32_t> flags(groups);
	for (int64_t g = 0; g < groups; ++g) {
		uint64_t code = 0;
		uint32_t delim = 0, unclassed = 0;
		for (int j = 0; j < 16; ++j) {
			const uint32_t l = (uint32_t)tdata[base + 16 * g + j] & LETTER_MASK;
			const uint32_t r = c.reduction[l] == L_MASK ? 15u : (uint32_t)c.reduction[l];
			code |= (uint64_t)r << (4 * j);
			delim |= (l == L_DELIM ? 1u : 0u) << j;
			unclassed |= (r == 15u ? 1u : 0u) << j;
		}
		codes[g] = code; flags[g] = delim | (unclassed << 16);
	}
	uint64_t care64 = 0;
	for (int k = 0; k < c.shape_weight[sid]; ++k) care64 |= (uint64_t)15 << (4 * c.shape_pos[sid][k]);
	std::vector<uint8_t> route(n);
	for (int64_t g = 0; g < n / 16; ++g) {
		const int64_t p0 = base + 16 * g;
		seed_route_group(codes[g], codes[g + 1], flags[g], flags[g + 1], t_begin - p0, t_end - p0, c.shape_len[sid], c.shape_mask[sid], care64, slice_bits, route.data() + 16 * g);
	}
	const uint32_t slices = 1u << slice_bits;
	std::vector<int64_t> at(slices + 1, 0);
	for (int64_t w = 0; w < n; ++w) ++at[route[w] == SEED_ROUTE_NONE ? slices : route[w]];
	int64_t sum = 0;
	for (uint32_t s = 0; s <= slices; ++s) { const int64_t x = at[s]; if (s < slices) counts_out[s] = (uint32_t)x; at[s] = sum; sum += x; }
	for (int64_t w = 0; w < n; ++w) list_out[at[route[w] == SEED_ROUTE_NONE ? slices : route[w]]++] = (uint32_t)w;
	for (int64_t k = 0; k < n; ++k) hash_out[k] = seed_ref_hash_entry(codes.data(), list_out[k], care64);

	const uint32_t hmask = bm1_hmask_of(slot_bits, 0), per = words >> slice_bits;
	bad[0] = bad[1] = bad[2] = bad[3] = 0;
	int64_t k = 0;
	for (uint32_t s = 0; s < slices; ++s)
		for (uint32_t i = 0; i < counts_out[s]; ++i, ++k) {
			const int64_t p = base + list_out[k];
			uint64_t key = 0;
			if (p < t_begin || p >= t_end || !seed_key_at(c, sid, tdata + p, key)) { ++bad[3]; continue; }
			const uint32_t h = seed_hash_a(key), stored = hash_out[k];
			const uint32_t word = seed_slice_word(stored, hmask, words);
			if (stored != h) ++bad[0];
			if (word != bm1_word_of_key(h, key, 0, hmask, words)) ++bad[1];
			if (bm1_bits(stored, k3) != bm1_bits(h, k3)) ++bad[2];
			if (word / per != s) ++bad[3];
		}
	return k;
}
