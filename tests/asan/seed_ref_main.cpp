// Stand-alone check of the host bookkeeping of the sliced stream's reference cache (csrc/seed_slices_core.h): key comparison,
// the plain / built / kept sequence, the budget, invalidation and the forcing hook. Built with -fsanitize=address,undefined by
// tests/test_seed_slices_emu.py; prints "ok" and returns 0, or says which step failed.
#include "../../diamond_amd/csrc/seed_slices_core.h"
#include <cstdio>
#include <vector>

using namespace dmnd;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

static SeedParams params(int shapes)
{
	SeedParams p;
	memset(&p, 0, sizeof(p));
	p.n_shapes = shapes;
	for (int i = 0; i < shapes; ++i) { p.shape_len[i] = 12 + i; p.shape_weight[i] = 3; p.shape_mask[i] = 0x83u << i; }
	for (int l = 0; l < 32; ++l) p.reduction[l] = (int8_t)(l < 20 ? l % 11 : L_MASK);
	p.reduction_size = 11;
	return p;
}

// one search: what seed_api.hip does around seed_ref_decide, with buffers stood in by a vector
struct Ctx {
	SeedRefState st;
	std::vector<char> cache;
	uint64_t generation = 0;
	SeedRefUse search(const SeedParams& sp, const void* tseed, int64_t t_begin, int64_t t_end, int slice_bits, int force, bool eligible, uint64_t budget, bool alloc_ok = true)
	{
		bool drop = false;
		const uint64_t bytes = seed_ref_cache_bytes(t_begin, t_end, sp.n_shapes);
		SeedRefUse u = seed_ref_decide(st, seed_ref_key_of(generation, tseed, t_begin, t_end, sp, slice_bits), force, eligible, bytes, budget, &drop);
		if (drop) { cache.clear(); cache.shrink_to_fit(); }
		if (u == SEED_REF_BUILT) {
			if (alloc_ok) cache.assign(64, 1);
			seed_ref_built(st, alloc_ok);
			if (!alloc_ok) { cache.clear(); u = SEED_REF_NONE; }
		}
		if (u != SEED_REF_NONE) CHECK(!cache.empty());
		return u;
	}
};

int main()
{
	const SeedParams one = params(1), two = params(2);
	const uint64_t big = (uint64_t)1 << 40;
	char block_a[64], block_b[64];
	{
		Ctx c;                                               // the default rule: plain, built, kept
		CHECK(c.search(one, block_a, 256, 100000, 5, -1, true, big) == SEED_REF_NONE && c.cache.empty());
		CHECK(c.search(one, block_a, 256, 100000, 5, -1, true, big) == SEED_REF_BUILT);
		CHECK(c.search(one, block_a, 256, 100000, 5, -1, true, big) == SEED_REF_KEPT);
		// every part of the key starts over and drops the stale buffers
		++c.generation;
		CHECK(c.search(one, block_a, 256, 100000, 5, -1, true, big) == SEED_REF_NONE && c.cache.empty());
		CHECK(c.search(one, block_a, 256, 100000, 5, -1, true, big) == SEED_REF_BUILT);
		CHECK(c.search(one, block_b, 256, 100000, 5, -1, true, big) == SEED_REF_NONE && c.cache.empty());
		CHECK(c.search(one, block_b, 256, 100000, 5, -1, true, big) == SEED_REF_BUILT);
		CHECK(c.search(one, block_b, 272, 100000, 5, -1, true, big) == SEED_REF_NONE);
		CHECK(c.search(one, block_b, 272, 100001, 5, -1, true, big) == SEED_REF_NONE);
		CHECK(c.search(one, block_b, 272, 100001, 4, -1, true, big) == SEED_REF_NONE);
		CHECK(c.search(two, block_b, 272, 100001, 4, -1, true, big) == SEED_REF_NONE);
		CHECK(c.search(two, block_b, 272, 100001, 4, -1, true, big) == SEED_REF_BUILT);
		SeedParams other = two;
		other.shape_mask[1] ^= 4u;
		CHECK(c.search(other, block_b, 272, 100001, 4, -1, true, big) == SEED_REF_NONE && c.cache.empty());
		other = two; other.reduction[3] = 7;
		CHECK(c.search(other, block_b, 272, 100001, 4, -1, true, big) == SEED_REF_NONE);
		other = two; other.shape_len[0] += 1;
		CHECK(c.search(other, block_b, 272, 100001, 4, -1, true, big) == SEED_REF_NONE);
		CHECK(c.search(other, block_b, 272, 100001, 4, -1, true, big) == SEED_REF_BUILT);
		// a search that cannot use the cache leaves one of the same key alone
		CHECK(c.search(other, block_b, 272, 100001, 4, 0, true, big) == SEED_REF_NONE && !c.cache.empty());
		CHECK(c.search(other, block_b, 272, 100001, 4, -1, false, big) == SEED_REF_NONE && !c.cache.empty());
		CHECK(c.search(other, block_b, 272, 100001, 4, -1, true, big) == SEED_REF_KEPT);
	}
	{
		Ctx c;                                               // the budget: bytes of C2's block with one shape, and one byte less
		const int64_t t_begin = 256, t_end = 256 + 301000000;
		const uint64_t need = seed_ref_cache_bytes(t_begin, t_end, 1);
		CHECK(need > (uint64_t)1250 << 20 && need <= (uint64_t)2048 << 20);
		CHECK(seed_ref_cache_bytes(t_begin, t_end, 2) <= (uint64_t)3072 << 20 && seed_ref_cache_bytes(t_begin, t_end, 3) > (uint64_t)3072 << 20);
		for (int k = 0; k < 3; ++k) CHECK(c.search(one, block_a, t_begin, t_end, 5, -1, true, need - 1) == SEED_REF_NONE && c.cache.empty());
		CHECK(c.search(one, block_a, t_begin, t_end, 5, 1, true, 0) == SEED_REF_NONE && c.cache.empty());
		CHECK(c.search(one, block_a, t_begin, t_end, 5, -1, true, need) == SEED_REF_NONE);      // (over the budget nothing was remembered either)
		CHECK(c.search(one, block_a, t_begin, t_end, 5, -1, true, need) == SEED_REF_BUILT);
	}
	{
		Ctx c;                                               // forced: built by the first search; a failed allocation leaves the plain stream
		CHECK(c.search(one, block_a, 256, 5000, 0, 1, true, big) == SEED_REF_BUILT);
		CHECK(c.search(one, block_a, 256, 5000, 0, 1, true, big) == SEED_REF_KEPT);
		CHECK(c.search(one, block_a, 256, 5000, 0, 0, true, big) == SEED_REF_NONE);
		++c.generation;
		CHECK(c.search(one, block_a, 256, 5000, 0, 1, true, big, false) == SEED_REF_NONE && c.cache.empty());
		CHECK(c.search(one, block_a, 256, 5000, 0, -1, true, big) == SEED_REF_NONE);
		CHECK(c.search(one, block_a, 256, 5000, 0, -1, true, big) == SEED_REF_BUILT);
	}
	// slice counts
	CHECK(seed_slice_bits(786432, 23, SEED_SLICE_MAX_WORDS) == 5 && seed_slice_bits(524288, 23, SEED_SLICE_MAX_WORDS) == 4);
	CHECK(seed_slice_bits(32768, 10, SEED_SLICE_MAX_WORDS) == 0 && seed_slice_bits(32768, 10, 512) == 6 && seed_slice_bits(32768, 3, 512) == -1);
	CHECK(seed_slice_bits(4194304, 31, SEED_SLICE_MAX_WORDS) == -1 && seed_slice_bits(3 * 4096 + 1, 20, 64) == -1);
	if (!failures) std::printf("ok\n");
	return failures ? 1 : 0;
}
