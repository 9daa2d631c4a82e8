// seed_slices_core.h -- the sliced long-seed reference stream: what the kernels, the host bookkeeping in
// seed_api.hip and the CPU tests (tests/emu) share. No HIP in here.
//
// The level-1 filter of a long-seed search (3 MB for C2 on the plain stream, 8 MB on this one) does not fit a CU's LDS; a slice of it does. Without key classes the word of
// a key is bm1_word(h & hmask, W) = ((h & hmask) * W) >> 32 with h = seed_hash_a(key): when 2^b divides W and hmask keeps the top b
// bits of h (slot_bits >= b), a key whose top b bits of h are s probes a word of [s W / 2^b, (s + 1) W / 2^b) -- slice s. The key is
// a function of the reference window and the shape alone, so the slice of every window is a reference-side fact: it is computed
// once per uploaded reference block (the routing: per slice the list of its windows, ascending) and kept over the searches of
// that block, and a workgroup that holds slice s in LDS walks list s.
#pragma once
#include <stdint.h>
#include <string.h>
#include "seed_core.h"
#include "seed_ref_state.h"

namespace dmnd {

enum { SEED_SLICE_MAX_WORDS = 32768, SEED_SLICE_MAX_BITS = 6 };      // 128 KB of a CU's 160 KB of LDS; at most 64 slices
enum : uint8_t { SEED_ROUTE_NONE = 0xff };                            // routing byte of a window that is no seed

// b: the smallest slice count 2^b with W / 2^b <= max_words words a slice, 2^b | W and the top b hash bits inside the filter's
// hash mask; -1: none (the search takes the plain stream)
DMND_HD int seed_slice_bits(uint64_t words, int slot_bits, uint32_t max_words)
{
	if (max_words > (uint32_t)SEED_SLICE_MAX_WORDS) max_words = SEED_SLICE_MAX_WORDS;
	for (int b = 0; b <= SEED_SLICE_MAX_BITS; ++b) {
		if (words == 0 || words % ((uint64_t)1 << b) != 0) return -1;
		if ((words >> b) <= max_words) return b <= slot_bits ? b : -1;
	}
	return -1;
}

// Words of the level-1 filter that a search on the sliced stream builds. The plain stream's filter is sized to stay in an XCD's L2
// beside the stream (seed_sizes); the sliced stream probes from LDS, where only the slice count bounds the filter: the largest
// power of two that SEED_SLICE_MAX_BITS slices of SEED_SLICE_MAX_WORDS words hold, and no more than the level-2 filter (bm_words).
// It stands in for default_words (seed_sizes' size) only where it is larger and seed_slice_bits finds it a slice count; otherwise
// the result is default_words. forced_words (DMND_SEED_SLICES_FILTER_WORDS; 0: none) replaces the rule's size, bound by the slice
// count alone. *k3 (bm1_bits) is written only where the result is not default_words: three bits per seed from four filter bits per
// query position up, seed_sizes' own bound, and two bits otherwise. The three bits are k3 = 2, the third bit from below the word
// index, for a power of two of words (the rule's sizes; at most 2^21 by the slice count), and the plain stream's k3 = 1 for a
// forced size that is none: its word index reaches below bit 11.
DMND_HD uint64_t seed_slices_filter_words(uint64_t nq_pos, int slot_bits, uint64_t bm_words, uint64_t default_words, uint32_t max_slice_words, uint64_t forced_words, uint32_t* k3)
{
	uint64_t w = forced_words;
	if (w == 0) {
		uint64_t most = (uint64_t)SEED_SLICE_MAX_WORDS << SEED_SLICE_MAX_BITS;
		if (bm_words < most) most = bm_words;
		for (w = 1; w * 2 <= most; w *= 2) {}
		if (w <= default_words) return default_words;
	}
	if (w == default_words || seed_slice_bits(w, slot_bits, max_slice_words) < 0) return default_words;
	if (k3) *k3 = nq_pos * 4 > w * 32 ? 0u : (w & (w - 1)) == 0 ? 2u : 1u;
	return w;
}

// slice of a key's hash a
DMND_HD uint32_t seed_slice_of(uint32_t h, int slice_bits) { return slice_bits ? h >> (32 - slice_bits) : 0u; }

// Without key classes the level-1 probe of a window is a function of h = seed_hash_a(key) alone -- the word below (bm1_word_of_key
// for classes = 0) and bm1_bits(h, k3) -- and h is a reference-side fact as the slice is: the cache keeps it beside every list entry
// (seed_ref_hash_entry), and the stream reads the hash instead of gathering the window's nibbles. Only a window that passes
// level 1 needs its list entry and its key again (level-2 word, table): seed_window_key from the kept nibbles.
DMND_HD uint32_t seed_slice_word(uint32_t h, uint32_t hmask, uint32_t words) { return bm1_word(h & hmask, words); }
// table key of the window that starts at nibble `at` (0..15) of c0, c0 / c1 the class nibbles of its group of 16 letters and the next
DMND_HD uint64_t seed_window_key(uint64_t c0, uint64_t c1, uint32_t at, uint64_t care64)
{
	const int sh = 4 * (int)at;
	return (sh == 0 ? c0 : (c0 >> sh) | (c1 << (64 - sh))) & care64;
}
// what the cache keeps beside a list entry (window offset `off` from the block's base): hash a of the window's key
DMND_HD uint32_t seed_ref_hash_entry(const uint64_t* codes, uint32_t off, uint64_t care64)
{
	return seed_hash_a(seed_window_key(codes[off >> 4], codes[(off >> 4) + 1], off & 15u, care64));
}

// The routing bytes of the 16 windows that start in one group of 16 reference letters: slice of the window's key, or SEED_ROUTE_NONE.
// c0 / c1: class nibbles of this group and the next one (seed_codes_kernel); f0 / f1: their flag words (delimiters low, letters
// without a class high); first / last: the block's window range relative to the group's first letter. A window is a seed exactly
// where the plain stream kernel probes it: inside the range, no delimiter among its len letters, no mask / stop letter at a care
// position (spaced seeds).
DMND_HD void seed_route_group(uint64_t c0, uint64_t c1, uint32_t f0, uint32_t f1, int64_t first, int64_t last, int len, uint32_t care, uint64_t care64, int slice_bits, uint8_t out[16])
{
	const uint32_t delim = (f0 & 0xffffu) | (f1 << 16), bad = (f0 >> 16) | (f1 & 0xffff0000u);
	const uint32_t span = (1u << len) - 1;                    // len <= 16
	for (int w = 0; w < 16; ++w) {
		const bool inside = w >= first && w < last && ((delim >> w) & span) == 0;
		const bool ok = inside && ((bad >> w) & care) == 0;
		const uint64_t key = seed_window_key(c0, c1, (uint32_t)w, care64);
		out[w] = ok ? (uint8_t)seed_slice_of(seed_hash_a(key), slice_bits) : (uint8_t)SEED_ROUTE_NONE;
	}
}

// ---- host bookkeeping of the per-block cache (dmnd_ctx::seed_ref) ----------------------------------------------------------------
// Everything the routing depends on. Kept and compared as bytes (SeedRefState::key): always made by seed_ref_key_of, which zeroes the padding.
struct SeedRefKey {
	uint64_t generation;                 // dmnd_ctx::target_generation: letters, limits, soft-mask view or alias of the reference block
	const void* tseed;                   // what the stream reads: the block, or its soft-masked view
	int64_t t_begin, t_end;
	int32_t n_shapes, slice_bits, seed_encoding, reduction_size;
	int8_t reduction[32];
	int32_t shape_len[SEED_MAX_SHAPES];
	uint32_t shape_mask[SEED_MAX_SHAPES];
};

inline SeedRefKey seed_ref_key_of(uint64_t generation, const void* tseed, int64_t t_begin, int64_t t_end, const SeedParams& sp, int slice_bits)
{
	SeedRefKey k;
	memset(&k, 0, sizeof(k));
	k.generation = generation; k.tseed = tseed; k.t_begin = t_begin; k.t_end = t_end;
	k.n_shapes = sp.n_shapes; k.slice_bits = slice_bits; k.seed_encoding = sp.seed_encoding; k.reduction_size = sp.reduction_size;
	memcpy(k.reduction, sp.reduction, sizeof(k.reduction));
	for (int i = 0; i < sp.n_shapes && i < SEED_MAX_SHAPES; ++i) { k.shape_len[i] = sp.shape_len[i]; k.shape_mask[i] = sp.shape_mask[i]; }
	return k;
}

inline std::string seed_ref_key_bytes(const SeedRefKey& k) { return std::string(reinterpret_cast<const char*>(&k), sizeof(SeedRefKey)); }

// letters the routing covers (from t_begin rounded down to 16, whole groups) and bytes the cache keeps for them: per shape one 32-bit
// list entry per window and the slice counts, once the class nibbles (8 bytes per group of 16; one group beyond the last window's)
inline int64_t seed_ref_windows(int64_t t_begin, int64_t t_end) { return ((t_end - (t_begin & ~(int64_t)15) + 15) / 16) * 16; }
inline uint64_t seed_ref_cache_bytes(int64_t t_begin, int64_t t_end, int n_shapes)
{
	const uint64_t n = (uint64_t)seed_ref_windows(t_begin, t_end);
	return (uint64_t)n_shapes * (n * sizeof(uint32_t) + 64 * sizeof(uint32_t)) + (n / 16 + 2) * sizeof(uint64_t);
}
// ... and for the hashes beside the list entries: per shape one 32-bit word per window more. The budget counts the sum of the two.
inline uint64_t seed_ref_hash_bytes(int64_t t_begin, int64_t t_end, int n_shapes)
{
	return (uint64_t)n_shapes * (uint64_t)seed_ref_windows(t_begin, t_end) * sizeof(uint32_t);
}

// What a search does about the cache. NONE: the plain stream, nothing built (the first search of a block generation, an ineligible
// search, a cache over the budget); BUILT: this search builds the cache and takes the sliced stream; KEPT: the cache is the one of an
// earlier search.
enum SeedRefUse { SEED_REF_NONE = 0, SEED_REF_BUILT = 1, SEED_REF_KEPT = 2 };
// force: -1 the default rule, 0 never, 1 always (builds on the first search). eligible: the search could take the sliced stream
// at all (and, under the default rule, the block is long enough); bytes / budget: seed_ref_cache_bytes and the context's cap.
// *drop: a cache built for another key is stale -- the caller releases its buffers. After SEED_REF_BUILT the caller reports how the
// build went with seed_ref_built.
inline SeedRefUse seed_ref_decide(SeedRefState& s, const SeedRefKey& k, int force, bool eligible, uint64_t bytes, uint64_t budget, bool* drop)
{
	const std::string kb = seed_ref_key_bytes(k);
	const bool same = s.seen != 0 && s.key == kb;
	*drop = s.seen == 2 && !same;
	if (!same) { s.seen = 0; }
	if (force == 0 || !eligible || bytes > budget) {
		// nothing is built for this key now; a cache of the same key stays for a later search that can use it
		return SEED_REF_NONE;
	}
	if (same && s.seen == 2) return SEED_REF_KEPT;
	if (force == 1 || same) { s.key = kb; return SEED_REF_BUILT; }
	s.key = kb; s.seen = 1;
	return SEED_REF_NONE;
}
inline void seed_ref_built(SeedRefState& s, bool ok) { s.seen = ok ? 2 : 0; }

}  // namespace dmnd
