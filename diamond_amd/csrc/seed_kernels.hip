// seed_kernels.hip -- gfx950 (MI355X) kernels of the seed stage: replaces
// Search::search_shape (/root/reference/src/search/stage0.cpp:101-217) and its SIMD stage-1/2 filters.
//
// Data flow (per-thread arithmetic in seed_core.h):
//   seed_qid_kernel     query position -> query id (for Hit::query_ and the seed offset); once per uploaded query block
//   launch_seed_build   the query side from ONE sort: every query position's seed in registers -> its sort key (top bits of
//                       its hash); a stable radix sort; then the open-addressing table in HBM, the per-seed lists of query
//                       positions and both filters of the stream are written in sorted order with plain stores
//   seed_stream_kernel  the reference block is streamed ONCE, coalesced; every position's seed is computed in
//                       registers and probed; a probe hit marks the slot "joined" and appends (slot, position)
//                       -- no reference seed array, no radix passes, no 9-byte scatter (the reference's #1 cost)
//   seed_mask_kernel    per joined seed: low-complexity test (mask_seeds), per-letter mask times
//   seed_pair_kernel    per (joined reference position x query list entry): 48-byte Hamming filter, left-most rule,
//                       Hit append with one atomic per surviving pair
// The table for the 10k-query workload (3e6 seeds, 8M slots, 96 MB) lives in the 256 MB Infinity Cache, so the
// stream kernel's only HBM traffic is the reference letters themselves.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "seed_core.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <rocprim/iterator/transform_output_iterator.hpp>
#include <rocprim/device/device_scan.hpp>
#include "seed_kernels.h"

namespace dmnd {

// launch_seed_clear: thread t owns the t-th 16-byte chunk of the concatenated ranges
struct SeedClearArgs { char* p[8]; uint64_t bytes[8]; uint64_t first_chunk[9]; uint32_t word[8]; int n; };
__global__ __launch_bounds__(256) void seed_clear_kernel(SeedClearArgs z)
{
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= z.first_chunk[8]) return;
	// (selects over constant indices: a dynamically indexed kernel argument would be copied to scratch memory)
	char* base = z.p[0];
	uint64_t bytes = z.bytes[0], first = 0;
	uint32_t w = z.word[0];
#pragma unroll
	for (int i = 1; i < 8; ++i)
		if (i < z.n && t >= z.first_chunk[i]) { base = z.p[i]; bytes = z.bytes[i]; first = z.first_chunk[i]; w = z.word[i]; }
	const uint64_t off = (t - first) * 16, left = bytes - off;
	char* q = base + off;
	if (left >= 16 && ((uintptr_t)q & 15) == 0) { *reinterpret_cast<uint4*>(q) = make_uint4(w, w, w, w); return; }
	for (uint64_t i = 0; i < (left < 16 ? left : 16); ++i) q[i] = (char)w;
}

hipError_t launch_seed_clear(const SeedClear& z, hipStream_t st)
{
	if (z.n == 0) return hipSuccess;
	SeedClearArgs a;
	uint64_t chunks = 0;
	for (int i = 0; i < 8; ++i) {
		a.p[i] = i < z.n ? static_cast<char*>(z.p[i]) : nullptr; a.bytes[i] = i < z.n ? z.bytes[i] : 0;
		a.word[i] = i < z.n ? (z.value[i] & 0xffu) * 0x01010101u : 0u;
		a.first_chunk[i] = chunks;
		if (i < z.n) chunks += (z.bytes[i] + 15) / 16;
	}
	for (int i = z.n; i <= 8; ++i) a.first_chunk[i] = chunks;
	a.n = z.n;
	hipLaunchKernelGGL(seed_clear_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, st, a);
	return hipGetLastError();
}

__global__ void seed_qid_kernel(const int64_t* __restrict__ limits, int64_t n_seqs, uint32_t* __restrict__ qid_of)
{
	// one wavefront per sequence
	const int64_t seq = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const int lane = threadIdx.x & 63;
	if (seq >= n_seqs) return;
	const int64_t b = limits[seq], e = limits[seq + 1];
	for (int64_t p = b + lane; p < e; p += 64)
		qid_of[p] = (uint32_t)seq;
}

// ---- query side: one sort, then plain stores ---------------------------------------------------------------
// The work area of launch_seed_build (32-bit words): [0, n) sort keys, later the placement scan's output (and the long runs'
// scratch before it); [n, 2n) list sizes by sorted index; [2n, 2n + 64) counters; [2n + 64, 3n + 64) the sorted indices of the keys
// placed past the last slot; then, 8-byte aligned, every query position's table key. The kernels behind the sort find a position's
// key there with ONE 8-byte load: recomputed from the letters at positions in hash order it took ~28 byte loads to as many random
// lines per element (0.38 ms per C2 build, bound by L2 requests).
enum { BUILD_SHORT = 8 };                     // runs of equal sort key up to this length are regrouped in one thread's registers
static const uint32_t BUILD_CONSUMED = 0xffffffffu;

// Per query position: its sort key t (top slot_bits bits of the order value), or 1 << slot_bits -- sorting last -- for a position
// without a seed. The query-indexed algorithm drops a low-complexity query seed and masks it when the query seeds are enumerated
// (enum_seeds_hashed, enum_seeds.h:141-145), whether or not it joins; one position per thread and shape: no race.
__global__ void seed_order_kernel(SeedArgs a, int sid, uint32_t* __restrict__ skey, uint64_t* __restrict__ keys, uint32_t* __restrict__ ctr)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < 4) ctr[i] = 0;
	const int64_t p = a.q_begin + i;
	if (p >= a.q_end) return;
	uint32_t k = 1u << a.slot_bits;
	uint64_t seed;                                     // table key (seed_key_at)
	if (seed_key_at(a.params, sid, a.qseed + p, seed)) {
		if (a.params.seed_encoding == SEED_HASHED && !seed_is_complex(a.params, sid, a.qseed + p)) {
			const uint8_t t = (uint8_t)(sid * a.params.index_chunks);
			if (t < a.mask_time[p]) a.mask_time[p] = t;
		}
		else {
			k = a.order(seed_hash_a(seed), seed) >> (32 - a.slot_bits);
			keys[i] = seed;
		}
	}
	skey[i] = k;
}

__device__ __forceinline__ uint32_t reduce4(uint32_t letter, uint64_t map_lo, uint64_t map_hi)
{
	const uint64_t m = (letter & 16) ? map_hi : map_lo;
	return (uint32_t)(m >> ((letter & 15) * 4)) & 15u;
}

// seed_order_kernel for shapes of up to 16 letters over at most 15 classes, 16 positions per thread: the letters decoded the way the
// plain branch of seed_stream_fast_kernel decodes the reference (two 16-byte loads, class nibbles, delimiter and bad-letter maps), a
// window's key one funnel shift and the care mask. One thread per position spent ~12 byte loads and as many table look-ups in the
// kernel arguments on it (62-117 us for the 3e6 positions of C2). The workgroup's 4096 (sort key, table key) pairs go through LDS,
// 17 entries per thread's 16 against bank conflicts, so that the stores are coalesced. HASHED: seed_key_hashed keeps the windows
// that hold a mask or stop letter; a low-complexity seed is masked here, as in seed_order_kernel.
template<bool HASHED>
__global__ __launch_bounds__(256) void seed_order16_kernel(SeedArgs a, int sid, uint64_t map_lo, uint64_t map_hi, int64_t base, uint64_t care64,
	uint32_t* __restrict__ skey, uint64_t* __restrict__ keys, uint32_t* __restrict__ ctr)
{
	__shared__ uint32_t s_top[256 * 17];
	__shared__ uint64_t s_key[256 * 17];
	if (blockIdx.x == 0 && threadIdx.x < 4) ctr[threadIdx.x] = 0;
	const int64_t wg_base = base + (int64_t)blockIdx.x * 4096;
	const int64_t p0 = wg_base + (int64_t)threadIdx.x * 16;
	const uint32_t none = 1u << a.slot_bits;
	if (p0 < a.q_end) {
		typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
		const u32x4 v0 = *reinterpret_cast<const u32x4*>(a.qseed + p0), v1 = *reinterpret_cast<const u32x4*>(a.qseed + p0 + 16);
		const uint32_t w[8] = { v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w };
		uint64_t codes[2] = { 0, 0 };
		uint32_t delim = 0, bad = 0;
#pragma unroll
		for (int j = 0; j < 32; ++j) {
			const uint32_t l = (w[j >> 2] >> ((j & 3) * 8)) & LETTER_MASK;
			const uint32_t c = reduce4(l, map_lo, map_hi);
			codes[j >> 4] |= (uint64_t)(HASHED && c == 15u ? 0u : c) << ((j & 15) * 4);
			delim |= (l == L_DELIM ? 1u : 0u) << j;
			bad |= (c == 15u ? 1u : 0u) << j;
		}
		const uint32_t care = a.params.shape_mask[sid], span = (1u << a.params.shape_len[sid]) - 1;      // length <= 16
		const int64_t first = a.q_begin - p0, last = a.q_end - p0;                                       // window starts of the block: first <= i < last
#pragma unroll
		for (int i = 0; i < 16; ++i) {
			const int sh = i * 4;
			uint64_t seed = (sh == 0 ? codes[0] : (codes[0] >> sh) | (codes[1] << (64 - sh))) & care64;
			const bool inside = i >= first && i < last && ((delim >> i) & span) == 0;
			// spaced seeds: no mask / stop letter at a care position; hashed seeds: none anywhere in the window, or seed_key_hashed decides
			bool ok = inside && ((bad >> i) & (HASHED ? span : care)) == 0;
			if (HASHED && inside && !ok) ok = seed_key_hashed(a.params, sid, a.qseed + p0 + i, seed);
			uint32_t k = none;
			if (ok) {
				if (HASHED && !seed_is_complex(a.params, sid, a.qseed + p0 + i)) {
					const uint8_t t = (uint8_t)(sid * a.params.index_chunks);
					if (t < a.mask_time[p0 + i]) a.mask_time[p0 + i] = t;
				}
				else k = a.order(seed_hash_a(seed), seed) >> (32 - a.slot_bits);
			}
			s_top[threadIdx.x * 17 + i] = k;
			s_key[threadIdx.x * 17 + i] = seed;
		}
	}
	__syncthreads();
#pragma unroll 4
	for (int r = 0; r < 16; ++r) {
		const int e = r * 256 + threadIdx.x;                             // the workgroup's e-th position
		const int64_t p = wg_base + e;
		if (p < a.q_begin || p >= a.q_end) continue;
		skey[p - a.q_begin] = s_top[e + (e >> 4)];
		keys[p - a.q_begin] = s_key[e + (e >> 4)];
	}
}

// After the stable sort by t (positions ascending within a run of equal t): a run holds the positions of every key whose t it is,
// interleaved. Its first thread regroups them in place into one position-ascending list per key, the keys in the order of their
// smallest positions, and writes every list's size at its start (0 elsewhere). Runs longer than BUILD_SHORT -- a seed repeated
// many times, mostly -- are regrouped by the whole wavefront, one pass over the run per distinct key.
__global__ __launch_bounds__(256) void seed_group_kernel(SeedArgs a, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ top, uint32_t* __restrict__ qlist,
	uint32_t* __restrict__ len, uint32_t* __restrict__ scratch, int64_t n)
{
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t none = 1u << a.slot_bits;
	const uint32_t t = j < n ? top[j] : none;
	const bool head = t != none && (j == 0 || top[j - 1] != t);
	int64_t e = j + 1;
	if (head) {
		while (e < n && e - j <= BUILD_SHORT && top[e] == t) ++e;
		if (e - j > BUILD_SHORT && e < n && top[e] == t) {      // long run: the end by galloping, then bisection
			int64_t lo = e, step = 1, hi = e + 1;                 // top[lo] == t
			while (hi < n && top[hi] == t) { lo = hi; step *= 2; hi = lo + step; }
			if (hi > n) hi = n;                                   // the end lies in (lo, hi]
			while (hi - lo > 1) { const int64_t mid = (lo + hi) / 2; if (top[mid] == t) lo = mid; else hi = mid; }
			e = hi;
		}
	}
	else if (t == none && j < n) len[j] = 0;
	const bool is_long = head && e - j > BUILD_SHORT;
	if (head && !is_long) {
		const int m = (int)(e - j);
		if (m == 1) len[j] = 1;
		else {
			uint32_t x[BUILD_SHORT];
			uint64_t k[BUILD_SHORT];
#pragma unroll
			for (int i = 0; i < BUILD_SHORT; ++i) {
				x[i] = i < m ? qlist[j + i] : 0u;
				k[i] = i < m ? keys[x[i]] : 0u;
			}
			uint32_t done = 0;                                    // bit i: element i is written
			int out = 0;
#pragma unroll
			for (int i = 0; i < BUILD_SHORT; ++i) {
				if (i >= m || ((done >> i) & 1u)) continue;
				const int start = out;
#pragma unroll
				for (int r = i; r < BUILD_SHORT; ++r)
					if (r < m && k[r] == k[i]) {
						qlist[j + out] = x[r];
						if (out != start) len[j + out] = 0;
						++out;
						done |= 1u << r;
					}
				len[j + start] = (uint32_t)(out - start);
			}
		}
	}
	// the long runs of this wavefront, one after the other by all its lanes; a lane always handles the run indices = its lane number
	// mod 64, so that it reads back only what it wrote itself
	uint64_t longs = __ballot(is_long);
	const int lane = threadIdx.x & 63;
	while (longs) {
		const int src = __builtin_ctzll(longs);
		longs &= longs - 1;
		const int64_t s = __shfl(j, src), m = __shfl(e, src) - s;
		for (int64_t i = lane; i < m; i += 64) scratch[s + i] = qlist[s + i];
		int64_t out = 0, first = 0;
		for (;;) {
			// the smallest unconsumed index: its key is the next list's
			int64_t c = first & ~(int64_t)63;
			uint64_t av = 0;
			uint32_t v = BUILD_CONSUMED;
			for (; c < m; c += 64) {
				v = c + lane < m ? scratch[s + c + lane] : BUILD_CONSUMED;
				av = __ballot(v != BUILD_CONSUMED);
				if (av) break;
			}
			if (c >= m) break;
			first = c + __builtin_ctzll(av);
			const uint64_t key = keys[(uint32_t)__shfl((int)v, __builtin_ctzll(av))];
			const int64_t start = out;
			for (; c < m; c += 64) {
				const int64_t i = c + lane;
				const uint32_t x = i < m ? scratch[s + i] : BUILD_CONSUMED;
				const bool mine = x != BUILD_CONSUMED && keys[x] == key;
				const uint64_t mb = __ballot(mine);
				if (mine) {
					const int64_t o = out + __builtin_popcountll(mb & ((1ull << lane) - 1));
					qlist[s + o] = x;
					if (o != start) len[s + o] = 0;
					scratch[s + i] = BUILD_CONSUMED;
				}
				out += __builtin_popcountll(mb);
			}
			if (lane == 0) len[s + start] = (uint32_t)(out - start);
		}
	}
}

// Placement of the distinct keys in table order (linear probing): slot = max(home, slot of the key before + 1). Over a stretch of
// the sorted array this is x -> max(A, x + B) of the slot x of the key before it; the scan composes these functions. A value holds
// B (keys) in its high word and A + 1 in its low word -- 0: no key, saturated: past every slot.
struct SeedPlaceOp {
	__host__ __device__ uint64_t operator()(uint64_t x, uint64_t y) const
	{
		const uint32_t ax = (uint32_t)x, ay = (uint32_t)y, by = (uint32_t)(y >> 32);
		uint32_t v = ax == 0 ? 0u : (ax + by < ax ? 0xffffffffu : ax + by);
		v = v > ay ? v : ay;
		return (((x >> 32) + (uint64_t)by) << 32) | v;
	}
};
struct SeedPlaceIn {
	const uint32_t* len; const uint32_t* top;
	__host__ __device__ uint64_t operator()(uint32_t j) const { return len[j] ? ((uint64_t)1 << 32) | (uint64_t)(top[j] + 1u) : 0ull; }
};
struct SeedPlaceOut {
	__host__ __device__ uint32_t operator()(uint64_t v) const { return (uint32_t)v; }
};

// (word, bits) of the sorted elements of a workgroup: every word is OR-reduced over its elements and stored once -- with an atomic
// only where its elements continue into the workgroup before or after
__device__ __forceinline__ void build_words(uint32_t* bm, uint32_t w, uint32_t bits, bool edge_lo, bool edge_hi, uint32_t* sw, uint32_t* sb)
{
	const int i = threadIdx.x;
	__syncthreads();
	sw[i] = w; sb[i] = bits;
	__syncthreads();
	if (w == 0xffffffffu || (i > 0 && sw[i - 1] == w)) return;
	int r = i + 1;
	uint32_t v = bits;
	for (; r < (int)blockDim.x && sw[r] == w; ++r) v |= sb[r];
	const bool shared = (i == 0 && edge_lo) || (r == (int)blockDim.x && edge_hi);
	if (!shared) bm[w] = v;
	else if (v) atomicOr(&bm[w], v);
}

// Per list start of the regrouped order: the key's slot (key, list head, size | LOWC) with plain stores, or -- past the last slot --
// a note for seed_wrap_kernel; its filter bits, reduced per word
__global__ __launch_bounds__(256) void seed_build_kernel(SeedArgs a, int sid, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ top, const uint32_t* __restrict__ qlist,
	const uint32_t* __restrict__ len, const uint32_t* __restrict__ place, uint32_t* __restrict__ ctr, uint32_t* __restrict__ wrap, int64_t n)
{
	__shared__ uint32_t sw[256], sb[256];
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t none = 1u << a.slot_bits;
	const uint32_t t = j < n ? top[j] : none;
	const uint32_t L = t != none ? len[j] : 0u;
	uint32_t b1 = 0, b2 = 0;
	if (L) {
		const uint32_t x = qlist[j];                      // the list's smallest position
		const uint64_t key = keys[x];
		const uint64_t h = seed_hash(key);
		b1 = bm1_bits((uint32_t)h, a.bitmap1_k3);
		b2 = 1u << (uint32_t)(h >> 59);
		// a list of one query position (most seeds): head IS the position -- the probe that finds the slot has it without a second
		// dependent random read. Search::mask_seeds evaluates the first query position of a joined group (seed_complexity.cpp:97-99):
		// the smallest. Whether that seed is complex does not depend on the join, so it is decided once here (only the fused stream
		// needs the answer before the join is known; otherwise seed_mask_kernel asks for the few joined groups).
		const bool lowc = a.fused && a.params.seed_encoding == SEED_SPACED && !seed_is_complex(a.params, sid, a.qdata + a.q_begin + x);
		const uint32_t pos = place[j] - 1u;
		if ((uint64_t)pos <= a.slot_mask) {
			SeedSlot sl;
			sl.key = key; sl.head = L == 1 ? x : (uint32_t)j; sl.flags = (L << 8) | (lowc ? SLOT_LOWC : 0u);
			a.slot(pos) = sl;
		}
		else wrap[atomicAdd(&ctr[1], 1u)] = (uint32_t)j;
	}
	const int64_t blk0 = (int64_t)blockIdx.x * blockDim.x, blk1 = blk0 + blockDim.x;
	const bool in = t != none;
	const uint32_t t_lo = blk0 > 0 ? top[blk0 - 1] : none, t_hi = blk1 < n ? top[blk1] : none;
	{
		const uint32_t w = in ? a.bm1_of_top(t) : 0xffffffffu;
		build_words(a.bitmap1, w, b1, t_lo != none && a.bm1_of_top(t_lo) == w, t_hi != none && a.bm1_of_top(t_hi) == w, sw, sb);
	}
	if (a.level2) {
		const uint32_t w = in ? a.bm2_of_top(t) : 0xffffffffu;
		build_words(a.bitmap, w, b2, t_lo != none && a.bm2_of_top(t_lo) == w, t_hi != none && a.bm2_of_top(t_hi) == w, sw, sb);
	}
}

// The keys whose placement ran past the last slot go in by the linear-probing insertion from slot 0 (every slot from their home to
// the last one is taken); none at the default sizes
__global__ __launch_bounds__(256) void seed_wrap_kernel(SeedArgs a, int sid, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ qlist, const uint32_t* __restrict__ len,
	const uint32_t* __restrict__ ctr, const uint32_t* __restrict__ wrap)
{
	const uint32_t nw = ctr[1];
	for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < nw; k += gridDim.x * blockDim.x) {
		const uint32_t j = wrap[k], L = len[j], x = qlist[j];
		const uint64_t key = keys[x];
		const bool lowc = a.fused && a.params.seed_encoding == SEED_SPACED && !seed_is_complex(a.params, sid, a.qdata + a.q_begin + x);
		uint64_t slot = 0;
		while (atomicCAS((unsigned long long*)&a.slot(slot).key, (unsigned long long)SEED_EMPTY, (unsigned long long)key) != (unsigned long long)SEED_EMPTY)
			slot = (slot + 1) & a.slot_mask;
		a.slot(slot).head = L == 1 ? x : j;
		a.slot(slot).flags = (L << 8) | (lowc ? SLOT_LOWC : 0u);
	}
}

__global__ void seed_fold_kernel(const int8_t* __restrict__ data, int64_t n, uint8_t* __restrict__ out)
{
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // output byte = letters 2j, 2j + 1
	if (2 * j >= n) return;
	const uint32_t a = (uint32_t)data[2 * j] & 15u, b = 2 * j + 1 < n ? (uint32_t)data[2 * j + 1] & 15u : 0u;
	out[j] = (uint8_t)(a | (b << 4));
}

__global__ void seed_reset_slots_kernel(SeedArgs a)
{
	const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (slot > a.slot_mask) return;
	const SeedSlot sl = a.slot(slot);
	if (sl.key == SEED_EMPTY || !(sl.flags & (SLOT_JOINED | SLOT_ERASED))) return;
	a.slot(slot).flags = sl.flags & ~(uint32_t)(SLOT_JOINED | SLOT_ERASED);
}

// hashed seeds: the part of seed_index_kernel that masks non-complex query seeds, without the insertion
__global__ void seed_hashed_lowc_kernel(SeedArgs a, int sid)
{
	const int64_t p = a.q_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= a.q_end) return;
	uint64_t seed;
	if (!seed_key_at(a.params, sid, a.qseed + p, seed) || seed_is_complex(a.params, sid, a.qseed + p)) return;
	const uint8_t t = (uint8_t)(sid * a.params.index_chunks);
	if (t < a.mask_time[p]) a.mask_time[p] = t;
}

// Motif soft masking on the query side: the seed positions whose window of shape sid (clipped at the end of the sequence)
// touches a soft-masked letter carry the SEED_MASK bit from the first index chunk of that shape on (MaskingTable::remove with
// template_len = the shape's length, after the query seeds of (shape, chunk 0) were enumerated: enum_seeds.h:255-260)
__global__ void seed_soft_time_kernel(SeedArgs a)
{
	const int64_t p = a.q_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= a.q_end || (a.qdata[p] & LETTER_MASK) == L_DELIM) return;
	int reach = 0;                                       // letters of the sequence from p on, up to the longest shape
	int first_soft = 1 << 30;                            // distance to the first soft-masked letter
	for (; reach < 32 && (a.qdata[p + reach] & LETTER_MASK) != L_DELIM; ++reach)
		if (first_soft > reach && a.qseed[p + reach] != a.qdata[p + reach]) first_soft = reach;
	if (first_soft >= 32) return;
	for (int sid = 0; sid < a.params.n_shapes; ++sid)
		if (first_soft < a.params.shape_len[sid]) {
			const uint8_t t = (uint8_t)(sid * a.params.index_chunks);
			if (t < a.mask_time[p]) a.mask_time[p] = t;
			return;
		}
}

// Wave-aggregated append: the lanes of the wavefront that have an element reserve their slots with ONE atomic on the
// shared counter (a per-element atomicAdd on one address serialises at the L2 atomic unit: with tens of millions of joined
// positions per shape that was > 90 % of the seed stage in the sensitive modes). Must be called by every active lane.
__device__ __forceinline__ unsigned long long wave_append(unsigned long long* counter, bool have)
{
	const unsigned long long mask = __ballot(have);
	if (mask == 0) return 0;
	const int lane = threadIdx.x & 63, leader = __builtin_ctzll(mask);
	unsigned long long base = 0;
	if (lane == leader) base = atomicAdd(counter, (unsigned long long)__builtin_popcountll(mask));
	base = (unsigned long long)__shfl((long long)base, leader);
	return base + (unsigned long long)__builtin_popcountll(mask & ((1ull << lane) - 1));
}

__global__ void seed_stream_kernel(SeedArgs a, int sid)
{
	const int64_t p = a.t_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint64_t seed = 0, slot = 0;
	uint32_t fl = 0;
	bool found = false;
	if (p < a.t_end && seed_key_at(a.params, sid, a.tseed + p, seed)) {
		slot = a.home(seed_hash(seed), seed);
		for (;;) {
			const SeedSlot sl = a.slot(slot);
			if (sl.key == SEED_EMPTY) break;
			if (sl.key == seed) { found = true; fl = sl.flags; break; }
			slot = (slot + 1) & a.slot_mask;
		}
	}
	const unsigned long long idx = wave_append(a.matched_count, found);
	if (!found) return;
	if (!(fl & SLOT_JOINED)) a.slot(slot).flags = fl | SLOT_JOINED;      // benign race: every writer stores the same value
	if (idx < (unsigned long long)a.matched_cap) {
		a.matched_slot[idx] = (uint32_t)slot;
		a.matched_loc[idx] = p;
	}
}

// matches of two 48-letter windows held as 12 words each (fingerprint_id, four letters per 32-bit operation)
__device__ __forceinline__ int window_identity(const uint32_t* a, const uint32_t* b)
{
	int n = 0;
#pragma unroll
	for (int w = 0; w < 12; ++w) {
		const uint32_t d = (a[w] ^ b[w]) & 0x1f1f1f1fu;
		n += 4 - __builtin_popcount((d + 0x7f7f7f7fu) & 0x80808080u);
	}
	return n;
}

// ---- fast reference stream: 16 positions per thread -------------------------------------------------------------
// Each thread loads 32 consecutive letters with two aligned 16-byte loads (coalesced: a wavefront reads 1 KiB + a
// 16-byte halo that hits L1), reduces them to 4-bit classes packed in two 64-bit registers, and forms the table key
// of each of its 16 window starts as (class nibbles >> 4 * start) & care-position mask (seed_key_at) -- no LDS, no
// per-position byte loads, no polynomial. A 2^k-bit Bloom-style bitmap of the query seeds (built by seed_index_kernel, resident
// in every XCD's L2) rejects most reference seeds before the open-addressing table in HBM/Infinity Cache is touched.
// Preconditions (checked by the host): shape length <= 16, reduction size <= 15.
// LEVEL2: consult the level-2 bitmap before the table. It pays when most level-1 positives are false (long seeds: --fast,
// default); with short seeds (weight <= 9: a third of the reference positions really join) it is a wasted random access.
// HASHED: seeds of the query-indexed algorithm (seed_key_hashed, seed_core.h). A window made of amino acids only has the same
// key as in the spaced-seed mode and takes the same path; a window that holds a mask or stop letter (the spaced mode's
// invalid windows) is keyed exactly by seed_key_hashed, which needs a look back for the start of the sequence -- a rare path
// next to the table probes.
// FUSED (short seeds): the Hamming filter of every (joined reference position, query position) pair runs right here, while
// the reference window is in L1 -- the pair filter that works from the list of joined positions re-reads a 48-byte window
// at a random place of the reference block per joined position (80 M of them per shape and 1.7 pairs each in --sensitive:
// ~14 GB of 128-byte line fills), after a radix sort of the list. The stream part only stages the joins (slot, position, list
// start and size) in LDS; then every thread takes staged joins in turn and filters their lists -- all lanes busy and as many
// independent loads in flight as there are lanes, instead of a chain of dependent loads in the few lanes that found a join.
// Lists longer than LIGHT are filtered by the whole workgroup. Pairs of a non-complex seed (SLOT_LOWC) are dropped: the seed
// only gets its JOINED mark for seed_mask_kernel. FUSED implies BYCLASS: seed_api.hip fails a fused search whose geometry
// has no key classes.
// Mutual-coverage search: the window of admissible query positions of the target that holds reference position sloc -- the last
// target that starts at or before it. Evaluated once per joined reference position; the pair test is then two integer compares.
__device__ __forceinline__ SeedQueryWindow seed_window_at(const SeedArgs& a, int64_t sloc)
{
	int64_t lo = 0, hi = a.n_targets;
	while (hi - lo > 1) {
		const int64_t mid = (lo + hi) >> 1;
		if (a.tlimits[mid] <= sloc) lo = mid; else hi = mid;
	}
	return a.qwin[lo];
}
__device__ __forceinline__ bool seed_window_holds(SeedQueryWindow w, uint32_t x) { return x >= w.first && x < w.end; }

enum { SEED_CLASS_TILES = 4 };      // tiles of 4096 window starts per class workgroup (kernel and launch)
// DMND_SEED_PHASES=1 (SeedArgs::phase_ticks): thread 0 of every workgroup adds the 100 MHz ticks between its phase boundaries
#define PHASE_MARK(i) do { if (a.phase_ticks && threadIdx.x == 0) { const uint64_t now_ = wall_clock64(); atomicAdd(&a.phase_ticks[i], (unsigned long long)(now_ - phase_t_)); phase_t_ = now_; } } while (0)
// MLR (FUSED only; mutual-coverage search, SeedArgs::qwin): the window of admissible query positions is found once per staged
// join and kept beside it in LDS; a pair whose query position lies outside it is dropped before any letter is read.
template<bool LEVEL2, bool HASHED, bool FUSED, bool BYCLASS = false, bool MLR = false>
__global__ __launch_bounds__(256) void seed_stream_fast_kernel(SeedArgs a, int sid, uint64_t map_lo, uint64_t map_hi, int64_t base, uint64_t care64)
{
	static_assert(!FUSED || BYCLASS, "the fused stream runs by key class");
	static_assert(!MLR || FUSED, "only the fused stream filters pairs");
	// Joined positions are staged in LDS and flushed with ONE atomic on the shared counter per workgroup: an atomicAdd per
	// match on a single address serialises at ~4.5 ns each (measured: 3.3 M matches = 14.8 ms per shape in default mode,
	// 22 M = 98 ms per shape in --sensitive), which dwarfed the 1.6 ms stream itself.
	// With short seeds (LEVEL2 off) a third of the positions join: the staging area then holds every position of the workgroup
	// (the direct-append fallback cost more than the whole rest of the kernel); positions are staged as 16-bit offsets.
	// (BYCLASS: a workgroup time is spent waiting for memory, phase after phase, and the kernel's time is the sum of the workgroup times
	// over the workgroups a CU holds -- which LDS decides: 58 KB allowed 2, these sizes allow 8, as many as the 62 VGPRs do)
	constexpr unsigned STAGE = BYCLASS ? 768 : LEVEL2 ? 1024 : 4096;
	__shared__ uint32_t st_slot[STAGE];
	__shared__ uint16_t st_loc[STAGE];
	__shared__ unsigned st_n;
	__shared__ unsigned long long st_base;
	constexpr uint32_t LIGHT = 8;
	constexpr unsigned SURV = FUSED ? 128 : 1, HEAVY = FUSED ? 64 : 1, FSTAGE = FUSED ? STAGE : 1;
	__shared__ uint32_t st_head[FSTAGE];
	__shared__ uint16_t st_count[FSTAGE];                    // saturated: a list that long is read back from its slot
	__shared__ SeedQueryWindow st_win[MLR ? FSTAGE : 1];
	__shared__ uint32_t sv_slot[SURV], sv_x[SURV];
	__shared__ uint16_t sv_loc[SURV], hv_k[HEAVY];
	__shared__ unsigned sv_n, hv_n;
	constexpr unsigned CQ = BYCLASS ? 2560 : 1, PQ = BYCLASS ? 1024 : 1;
	__shared__ uint16_t cq[CQ], pq[PQ];                      // BYCLASS: the workgroup's windows of its class (2048 expected); those that passed level 1
	__shared__ unsigned cq_n, pq_n;
	constexpr unsigned PAIRS = BYCLASS ? 1536 : 1;           // (join, list element) pairs of the light lists: in cq's place, which is done with by then
	uint16_t* const pr = cq;
	static_assert(PAIRS <= CQ, "the pair list lives in the class queue");
	__shared__ unsigned pr_n;
	uint64_t phase_t_ = a.phase_ticks ? wall_clock64() : 0;
	if (threadIdx.x == 0) { st_n = 0; sv_n = 0; hv_n = 0; cq_n = 0; pq_n = 0; pr_n = 0; }
	__syncthreads();
	PHASE_MARK(0);
	// (BYCLASS: eight workgroups per tile of 4096 positions, each looking at the windows of one key class only -- its own:
	// workgroup w is dispatched to XCD w mod 8, which is all the affinity there is; the result does not depend on it)
	constexpr bool by_class = BYCLASS;
	const uint32_t my_class = by_class ? blockIdx.x & 7u : 0u;
	// (a class workgroup covers CLASS_TILES tiles: it finds an eighth of a tile's joins, and the filter phase below wants as many
	// staged joins per workgroup as without classes -- measured with one tile per class workgroup: 11.5 ms per shape against 7.3)
	constexpr int CLASS_TILES = SEED_CLASS_TILES;
	const int64_t wg_base = base + (int64_t)(by_class ? (blockIdx.x >> 3) * CLASS_TILES : blockIdx.x) * blockDim.x * 16;
	const int64_t p0 = wg_base + (int64_t)threadIdx.x * 16;
	const bool in_range = p0 < a.t_end;
	auto survive = [&](uint32_t slot, uint32_t x, int64_t pos) {
		const unsigned k = atomicAdd(&sv_n, 1u);
		if (k < SURV) { sv_slot[k] = slot; sv_x[k] = x; sv_loc[k] = (uint16_t)(pos - wg_base); }
		else {                                                    // staging area full: direct append
			const unsigned long long idx = atomicAdd(a.survivor_count, 1ull);
			if (idx < (unsigned long long)a.survivor_cap) a.survivors[idx] = SeedSurvivor{ slot, x, pos };
		}
	};
	// Hamming filter of the reference window at pos against the entries first, first + step, ... of a list of query positions.
	// Pre-filter on letters folded to 4 bits (letter & 15: equal letters stay equal, so the folded identity count is an upper
	// bound of the real one): the query side is read from a 1.5 MB array with two 16-byte requests per pair instead of three
	// from the 3 MB block, which is what this kernel is short of (L2 capacity and fabric reads); the reference side from its
	// folded copy too, half the lines of the letters for the eight class workgroups that read around every tile's joins. The
	// ~2 % of the pairs that pass are counted exactly on the letters.
	auto filter_list = [&](uint32_t slot, uint32_t head, uint32_t count, int64_t pos, uint32_t first, uint32_t step, SeedQueryWindow win) {
		uint32_t tw[12], tf[6];
		{
			const int64_t t0 = pos - 16;
			typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(1)));
			const u32x4_u* src = reinterpret_cast<const u32x4_u*>(a.tfold + (t0 >> 1));
			const u32x4_u r0 = src[0], r1 = src[1];
			const uint32_t raw[8] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w };
			const uint32_t sh = (uint32_t)(t0 & 1) * 4;
#pragma unroll
			for (int w = 0; w < 6; ++w) tf[w] = __builtin_amdgcn_alignbit(raw[w + 1], raw[w], sh);
		}
		for (uint32_t i = first; i < count; i += step) {
			const uint32_t x = count == 1 ? head : a.qlist[head + i];
			if (MLR && (x < win.first || x >= win.end)) continue;
			const int64_t x0 = a.q_begin + (int64_t)x - 16;
			uint32_t raw[8];
			__builtin_memcpy(raw, a.qfold + (x0 >> 1), 32);
			const uint32_t sh = (uint32_t)(x0 & 1) * 4;
			int mism = 0;
#pragma unroll
			for (int w = 0; w < 6; ++w) {
				const uint32_t qf = __builtin_amdgcn_alignbit(raw[w + 1], raw[w], sh);
				const uint32_t d = tf[w] ^ qf;
				mism += __builtin_popcount((((d & 0x77777777u) + 0x77777777u) | d) & 0x88888888u);
			}
			if (48 - mism < a.params.hamming_filter_id) continue;
			uint32_t qw[12];
			__builtin_memcpy(qw, a.qdata + x0, 48);
			__builtin_memcpy(tw, a.tdata + pos - 16, 48);
			if (window_identity(tw, qw) >= a.params.hamming_filter_id) survive(slot, x, pos);
		}
	};
	// level-2 bitmap -> table -> staging, for a window whose key passed (or skipped) level 1
	// the probe chain of a key from `slot` on, whose content `sl` the caller has read already; a join is staged
	auto table_chain = [&](uint64_t seed, int64_t pos, uint64_t slot, SeedSlot sl) {
		bool found = false;
		uint32_t fl = 0, head = 0;
		for (;;) {
			if (sl.key == SEED_EMPTY) break;
			if (sl.key == seed) { found = true; fl = sl.flags; head = sl.head; break; }
			slot = (slot + 1) & a.slot_mask;
			sl = a.slot(slot);
		}
		if (!found) return;
		if (!(fl & SLOT_JOINED)) a.slot(slot).flags = fl | SLOT_JOINED;
		if (FUSED && (fl & SLOT_LOWC)) return;
		const unsigned k = atomicAdd(&st_n, 1u);                 // LDS atomic
		SeedQueryWindow win{ 0, 0 };
		if (MLR) win = seed_window_at(a, pos);
		if (k < STAGE) {
			st_slot[k] = (uint32_t)slot; st_loc[k] = (uint16_t)(pos - wg_base);
			if (FUSED) { st_head[k] = head; st_count[k] = (uint16_t)((fl >> 8) < 0xffffu ? (fl >> 8) : 0xffffu); }
			if (MLR) st_win[k] = win;
		}
		else {                                                    // staging area full (dense matches): direct append
			const unsigned long long idx = atomicAdd(a.matched_count, 1ull);
			if (idx < (unsigned long long)a.matched_cap) { a.matched_slot[idx] = (uint32_t)slot; a.matched_loc[idx] = pos; }
			if (FUSED) filter_list((uint32_t)slot, head, fl >> 8, pos, 0, 1, win);
		}
	};
	auto probe_table = [&](uint64_t seed, int64_t pos) {
		const uint64_t hh = seed_hash(seed);
		if (LEVEL2 && !((a.bitmap[a.bm2_index((uint32_t)hh, seed)] >> (uint32_t)(hh >> 59)) & 1u)) return;
		const uint64_t slot = a.home(hh, seed);
		table_chain(seed, pos, slot, a.slot(slot));
	};
	if (by_class) {
		// Eight workgroups look at every window, each at one class: what is done for all of them is kept to the key, its class and
		// the validity maps (the letters come decoded: seed_codes_kernel). A thread's own windows -- 2 of 16 on average, 7 for the
		// unluckiest lane of a wavefront -- are not probed where they are found: a lane's probes are a chain of dependent reads
		// (filter word -> slot -> next slot), and 8 x 7 such rounds per wavefront with most lanes idle took 9.3 ms per shape. They
		// are queued in LDS as 16-bit offsets; then all threads take queue entries in turn, first through the level-1 filter (four
		// independent probes per thread in flight), the survivors through the table.
		auto key_at = [&](uint32_t off) {
			const int64_t p = wg_base + off;
			const int64_t g = (p - base) >> 4;
			const int sh = (int)(p & 15) * 4;                             // base and wg_base are multiples of 16
			const uint64_t c0 = a.tcodes[g], c1 = a.tcodes[g + 1];
			return (sh == 0 ? c0 : (c0 >> sh) | (c1 << (64 - sh))) & care64;
		};
		// which of a group's 16 windows are valid and of this class: seed_classify_kernel's answer for this shape (one bit per window);
		// the maps of all the thread's groups are requested together
		uint32_t maps[CLASS_TILES], specials[CLASS_TILES];
#pragma unroll
		for (int sub = 0; sub < CLASS_TILES; ++sub) {
			const int64_t p0 = wg_base + ((int64_t)sub * 256 + threadIdx.x) * 16;
			const int64_t g = (p0 - base) >> 4;
			maps[sub] = p0 < a.t_end ? a.tclass[(int64_t)my_class * a.tclass_stride + g] : 0u;
			specials[sub] = HASHED && p0 < a.t_end && ((uint32_t)g & 7u) == my_class ? a.tclass[8 * a.tclass_stride + g] : 0u;
		}
#pragma unroll
		for (int sub = 0; sub < CLASS_TILES; ++sub) {
			const int64_t p0 = wg_base + ((int64_t)sub * 256 + threadIdx.x) * 16;
			uint32_t mine = maps[sub];
			if (mine) {
				const unsigned n_mine = (unsigned)__builtin_popcount(mine);
				unsigned k = atomicAdd(&cq_n, n_mine);
				while (mine) {
					const int w0 = __builtin_ctz(mine);
					mine &= mine - 1;
					if (k < CQ) cq[k] = (uint16_t)(p0 + w0 - wg_base);
					else {                                                    // queue full (never seen: 4096 expected, room for 6144): on the spot
						const uint64_t key = key_at((uint32_t)(p0 + w0 - wg_base));
						const uint32_t h = seed_hash_a(key);
						const uint32_t bw = a.bitmap1[a.bm1_index(h, key)], need = bm1_bits(h, a.bitmap1_k3);
						if ((bw & need) == need) probe_table(key, p0 + w0);
					}
					++k;
				}
			}
			// HASHED: windows holding a mask / stop letter are keyed by seed_key_hashed -- plane 8; each is looked at by ONE of the
			// eight workgroups (any will do: the classes are an affinity, not a partition of the work's correctness)
			uint32_t special = specials[sub];
			while (HASHED && special) {
				const int w0 = __builtin_ctz(special);
				special &= special - 1;
				uint64_t seed;
				if (!seed_key_hashed(a.params, sid, a.tseed + p0 + w0, seed)) continue;
				const uint32_t h = seed_hash_a(seed);
				const uint32_t bw = a.bitmap1[a.bm1_index(h, seed)], need = bm1_bits(h, a.bitmap1_k3);
				if ((bw & need) == need) probe_table(seed, p0 + w0);
			}
		}
		__syncthreads();
		PHASE_MARK(1);
		const unsigned n_cq = cq_n < CQ ? cq_n : CQ;
		constexpr int L1B = 8, TB = 4;                                // entries a thread has in flight: level-1 probes, first slot reads
		for (unsigned k0 = threadIdx.x; k0 < n_cq; k0 += L1B * 256) {
			uint32_t off[L1B], bw[L1B], need[L1B];
#pragma unroll
			for (int j = 0; j < L1B; ++j) {
				const unsigned k = k0 + (unsigned)j * 256;
				off[j] = k < n_cq ? cq[k] : 0xffffffffu;
				bw[j] = 0; need[j] = 1;
				if (k < n_cq) {
					const uint64_t key = key_at(off[j]);
					const uint32_t h = seed_hash_a(key);
					bw[j] = a.bitmap1[a.bm1_index(h, key)];
					need[j] = bm1_bits(h, a.bitmap1_k3);
				}
			}
#pragma unroll
			for (int j = 0; j < L1B; ++j)
				if ((bw[j] & need[j]) == need[j]) {
					const unsigned k = atomicAdd(&pq_n, 1u);
					if (k < PQ) pq[k] = (uint16_t)off[j];
					else probe_table(key_at(off[j]), wg_base + off[j]);
				}
		}
		__syncthreads();
		PHASE_MARK(2);
		const unsigned n_pq = pq_n < PQ ? pq_n : PQ;
		for (unsigned k0 = threadIdx.x; k0 < n_pq; k0 += TB * 256) {
			uint64_t key[TB], slot[TB];
			uint32_t off[TB];
			SeedSlot sl[TB];
#pragma unroll
			for (int j = 0; j < TB; ++j) {
				const unsigned k = k0 + (unsigned)j * 256;
				off[j] = k < n_pq ? pq[k] : 0xffffffffu;
				key[j] = k < n_pq ? key_at(off[j]) : 0;
			}
#pragma unroll
			for (int j = 0; j < TB; ++j)
				if (off[j] != 0xffffffffu) { slot[j] = a.home(seed_hash(key[j]), key[j]); sl[j] = a.slot(slot[j]); }
#pragma unroll
			for (int j = 0; j < TB; ++j)
				if (off[j] != 0xffffffffu) table_chain(key[j], wg_base + off[j], slot[j], sl[j]);
		}
	}
	else if (in_range) {
	typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
	const u32x4 v0 = *reinterpret_cast<const u32x4*>(a.tseed + p0), v1 = *reinterpret_cast<const u32x4*>(a.tseed + p0 + 16);
	const uint32_t w[8] = { v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w };
	uint64_t codes[2] = { 0, 0 };
	uint32_t delim = 0, bad = 0;
#pragma unroll
	for (int j = 0; j < 32; ++j) {
		const uint32_t l = (w[j >> 2] >> ((j & 3) * 8)) & LETTER_MASK;
		const uint32_t c = reduce4(l, map_lo, map_hi);
		codes[j >> 4] |= (uint64_t)(HASHED && c == 15u ? 0u : c) << ((j & 15) * 4);
		delim |= (l == L_DELIM ? 1u : 0u) << j;
		bad |= (c == 15u ? 1u : 0u) << j;
	}
	const int len = a.params.shape_len[sid];
	const uint32_t care = a.params.shape_mask[sid], span = (1u << len) - 1;      // len <= 16

	// The 16 window starts are handled as two batches of 8 (register pressure). The table key of a window is its 16
	// class nibbles ANDed with the care-position mask (seed_key_at): one funnel shift + one AND per window.
	const int64_t first = a.t_begin - p0, last = a.t_end - p0;                 // valid window starts: first <= i < last
	uint32_t special = 0;                                                        // HASHED: windows holding a mask / stop letter
#pragma unroll 1
	for (int half = 0; half < 2; ++half) {
		uint64_t key[8];
#pragma unroll
		for (int i = 0; i < 8; ++i) {
			const int sh = (8 * half + i) * 4;                                   // 0..60
			key[i] = (sh == 0 ? codes[0] : (codes[0] >> sh) | (codes[1] << (64 - sh))) & care64;
		}
		uint32_t pos_mask = 0;
		uint32_t word[8];
#pragma unroll
		for (int i = 0; i < 8; ++i) {
			const int w0 = 8 * half + i;
			const bool inside = w0 >= first && w0 < last && ((delim >> w0) & span) == 0;
			// spaced seeds: no mask / stop letter at a care position; hashed seeds: none anywhere in the window (else: special)
			const bool ok = inside && ((bad >> w0) & (HASHED ? span : care)) == 0;
			if (HASHED && inside && !ok) special |= 1u << w0;
			const uint32_t h = seed_hash_a(key[i]);                              // hash b is only needed past level 1
			const uint32_t bw = ok ? a.bitmap1[a.bm1_index(h, key[i])] : 0u;
			const uint32_t need = bm1_bits(h, a.bitmap1_k3);
			word[i] = (bw & need) == need ? 1u : 0u;
		}
#pragma unroll
		for (int i = 0; i < 8; ++i) pos_mask |= word[i] << i;
		// rare path: level-1 positives -> level-2 bitmap -> table
		while (pos_mask) {
			const int i = __builtin_ctz(pos_mask);
			pos_mask &= pos_mask - 1;
			uint64_t seed = 0;
#pragma unroll
			for (int x = 0; x < 8; ++x) if (x == i) seed = key[x];
			probe_table(seed, p0 + 8 * half + i);
		}
	}
	while (HASHED && special) {
		const int w0 = __builtin_ctz(special);
		special &= special - 1;
		uint64_t seed;
		if (!seed_key_hashed(a.params, sid, a.tseed + p0 + w0, seed)) continue;
		const uint32_t h = seed_hash_a(seed);
		const uint32_t bw = a.bitmap1[a.bm1_index(h, seed)], need = bm1_bits(h, a.bitmap1_k3);
		if ((bw & need) == need) probe_table(seed, p0 + w0);
	}
	}
	__syncthreads();
	PHASE_MARK(3);
	if (FUSED) {
		// Light lists (up to LIGHT query positions), one (join, list element) PAIR per thread and turn: a thread that walked its join's
		// whole list made the wavefront wait for the longest list of 64 -- two dependent reads per element (measured, DMND_SEED_PHASES:
		// 50 of 139 s of workgroup time over the 16 shapes of C3). The pairs are listed in LDS first (join << 3 | element).
		const unsigned n_joined = st_n < STAGE ? st_n : STAGE;
		for (unsigned k = threadIdx.x; k < n_joined; k += 256) {
			uint32_t count = st_count[k];
			if (count > LIGHT) {
				const unsigned hk = atomicAdd(&hv_n, 1u);
				if (hk < HEAVY) { hv_k[hk] = (uint16_t)k; continue; }
				if (count == 0xffffu) count = a.slot(st_slot[k]).flags >> 8;
				filter_list(st_slot[k], st_head[k], count, wg_base + st_loc[k], 0, 1, (MLR ? st_win[k] : SeedQueryWindow{ 0, 0 }));
				continue;
			}
			const unsigned at = atomicAdd(&pr_n, count);
			if (at + count <= PAIRS) for (uint32_t i = 0; i < count; ++i) pr[at + i] = (uint16_t)((k << 3) | i);
			else {                                                    // no room: on the spot (the slots of the reservation that exist are voided)
				for (unsigned i = at; i < PAIRS; ++i) pr[i] = 0xffffu;
				filter_list(st_slot[k], st_head[k], count, wg_base + st_loc[k], 0, 1, (MLR ? st_win[k] : SeedQueryWindow{ 0, 0 }));
			}
		}
		__syncthreads();
		const unsigned n_pairs = pr_n < PAIRS ? pr_n : PAIRS;
		for (unsigned e = threadIdx.x; e < n_pairs; e += 256) {       // (two pairs per thread in flight, their loads issued together: 108 -> 124 ms
			if (pr[e] == 0xffffu) continue;                            //  per 16 shapes -- the registers cost more wavefronts than the overlap returns)
			const unsigned k = pr[e] >> 3;
			filter_list(st_slot[k], st_head[k], st_count[k], wg_base + st_loc[k], pr[e] & 7u, 0x40000000u, (MLR ? st_win[k] : SeedQueryWindow{ 0, 0 }));
		}
		__syncthreads();
		PHASE_MARK(4);
		const unsigned n_heavy = hv_n < HEAVY ? hv_n : HEAVY;       // block-uniform
		for (unsigned h = 0; h < n_heavy; ++h) {
			const unsigned k = hv_k[h];
			uint32_t count = st_count[k];
			if (count == 0xffffu) count = a.slot(st_slot[k]).flags >> 8;
			filter_list(st_slot[k], st_head[k], count, wg_base + st_loc[k], threadIdx.x, 256, (MLR ? st_win[k] : SeedQueryWindow{ 0, 0 }));
		}
		__syncthreads();
		PHASE_MARK(5);
		const unsigned n_sv = sv_n < SURV ? sv_n : SURV;
		if (n_sv) {
			if (threadIdx.x == 0) st_base = atomicAdd(a.survivor_count, (unsigned long long)n_sv);
			__syncthreads();
			for (unsigned k = threadIdx.x; k < n_sv; k += blockDim.x) {
				const unsigned long long idx = st_base + k;
				if (idx < (unsigned long long)a.survivor_cap) a.survivors[idx] = SeedSurvivor{ sv_slot[k], sv_x[k], wg_base + sv_loc[k] };
			}
			__syncthreads();
		}
	}
	const unsigned n_staged = st_n < STAGE ? st_n : STAGE;
	if (n_staged == 0) return;
	if (threadIdx.x == 0) st_base = atomicAdd(a.matched_count, (unsigned long long)n_staged);
	__syncthreads();
	for (unsigned k = threadIdx.x; k < n_staged; k += blockDim.x) {
		const unsigned long long idx = st_base + k;
		if (idx < (unsigned long long)a.matched_cap) { a.matched_slot[idx] = st_slot[k]; a.matched_loc[idx] = wg_base + st_loc[k]; }
	}
}

// ---- sliced long-seed reference stream (seed_slices_core.h) -------------------------------------------------------
// The plain stream sends one 4-byte level-1 probe per window to L2, each lane's its own request, and runs at the rate the L2s accept
// requests. Here a workgroup loads ONE slice of the filter into LDS and walks the list of the windows whose keys fall into that
// slice (the routing, built once per uploaded reference block: seed_route_kernel + one stable radix pass): the probe is an LDS read,
// and what goes to L2 is a coalesced stream -- per window hash a of the window's key (seed_ref_hash_kernel: without key classes word
// and bits of the probe are functions of that hash alone), 16 bytes per lane and load. List entry and class nibbles are read for the
// level-1 positives only, which need the key for level 2 and the table: with the filter sized for the slices (seed_slices_filter_words,
// C2: 8 MB, 0.6 % positives) a positive's line of the list costs less than the list as a second stream. A sliced
// search that keeps seed_sizes' filter (a kept query index, a slice hook under which the larger size finds no slice count; C2's
// 3 MB: 3.1 % positives) fetches the same bytes either way -- 1.2 GB less stream, 1.2 GB of on-demand lines -- and ran 0.699 against 0.696 ms.
// Workgroup w serves slice w mod 2^b and the (w >> b)-th share of its list; no workgroup waits for another.
// One workgroup of 16 wavefronts fits a CU beside the slice, so nothing in the loop may make a wavefront wait for the others: behind
// the slice load there is no workgroup barrier (a barrier also drains the loads a wavefront has requested ahead). Every wavefront
// keeps its own queue of level-1 positives and its own staging area in LDS, addressed with ballots instead of atomics:
//  * hashes are requested SEED_SLICE_DEPTH rounds ahead of the round that is probed (C2's blocks, kernel alone: 0.709 ms
//    at 2 rounds, 0.696 at 4, 0.697 at 8);
//  * level-1 positives (3.1 % of the windows with the plain stream's 3 MB filter, seed_sizes) are queued by their list
//    indices, and 64 of them at a time read their list entries, form their keys from the nibbles and take the plain kernel's path -- level-2 bitmap,
//    table, SLOT_JOINED -- with all lanes busy, instead of a chain of dependent reads in the few lanes that found one;
//  * joins are staged and go out with one matched_count atomic per flush; direct append when the staging area is full.
// Spaced seeds only (hashed seeds stay on the plain kernel: their windows with a mask / stop letter are keyed from the raw letters).
enum { SEED_SLICE_THREADS = 1024, SEED_SLICE_BATCH = 4, SEED_SLICE_DEPTH = 4, SEED_SLICE_QUEUE = 128, SEED_SLICE_STAGE = 32 };
__global__ __launch_bounds__(SEED_SLICE_THREADS) void seed_stream_slices_kernel(SeedArgs a, int64_t base, uint64_t care64, const uint64_t* __restrict__ codes,
	const uint32_t* __restrict__ list, const uint32_t* __restrict__ hashes, const uint32_t* __restrict__ counts, int slice_bits, uint32_t slice_words)
{
	constexpr int B = SEED_SLICE_BATCH, DEPTH = SEED_SLICE_DEPTH;      // windows of a thread per round; rounds requested ahead
	constexpr unsigned WAVES = SEED_SLICE_THREADS / 64, QW = SEED_SLICE_QUEUE, ST = SEED_SLICE_STAGE;
	static_assert(QW >= 128, "a wavefront queues up to 63 + 64 positives before it probes 64");
	__shared__ uint32_t slice[SEED_SLICE_MAX_WORDS];
	__shared__ uint32_t q_off[WAVES][QW];
	__shared__ uint32_t st_slot[WAVES][ST], st_off[WAVES][ST];
	const unsigned s = blockIdx.x & ((1u << slice_bits) - 1), share = blockIdx.x >> slice_bits, shares = gridDim.x >> slice_bits;
	uint64_t begin = 0;
	for (unsigned i = 0; i < s; ++i) begin += counts[i];
	const uint64_t count = counts[s];
	const uint64_t lo = begin + count * share / shares, hi = begin + count * (share + 1) / shares;
	const uint32_t word0 = s * slice_words;
	for (uint32_t i = threadIdx.x; i < slice_words; i += blockDim.x) slice[i] = a.bitmap1[word0 + i];
	__syncthreads();
	const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	unsigned qn = 0, sn = 0;                                  // queued positives, staged joins of this wavefront (wavefront-uniform)
	auto rank_in = [&](unsigned long long ballot) { return (unsigned)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u)); };
	// LDS written by some lanes of the wavefront and read by others: the hardware runs a wavefront's LDS operations in order
	auto wave_sync = [&]() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); };
	auto flush = [&]() {
		const unsigned n = sn < ST ? sn : ST;
		unsigned long long at = 0;
		if (lane == 0) at = atomicAdd(a.matched_count, (unsigned long long)n);
		at = ((unsigned long long)(uint32_t)__shfl((int)(at >> 32), 0) << 32) | (uint32_t)__shfl((int)(uint32_t)at, 0);
		wave_sync();
		if (lane < n && at + lane < (unsigned long long)a.matched_cap) { a.matched_slot[at + lane] = st_slot[wave][lane]; a.matched_loc[at + lane] = base + st_off[wave][lane]; }
		wave_sync();
		sn = 0;
	};
	// level-2 bitmap -> table for one queued window per lane, the joins staged. This is probe_table / table_chain of
	// seed_stream_fast_kernel (same level-2 test, chain walk, SLOT_JOINED store and direct append) with the staging slot taken by ballot
	// instead of an LDS atomic and LEVEL2 read from the arguments: a change to either has to be made in both.
	auto probe = [&](bool active, uint64_t seed, uint32_t off) {
		bool found = false;
		uint64_t slot = 0;
		if (active) {
			const uint64_t hh = seed_hash(seed);
			if (!a.level2 || ((a.bitmap[a.bm2_index((uint32_t)hh, seed)] >> (uint32_t)(hh >> 59)) & 1u)) {
				slot = a.home(hh, seed);
				SeedSlot sl = a.slot(slot);
				uint32_t fl = 0;
				for (;;) {
					if (sl.key == SEED_EMPTY) break;
					if (sl.key == seed) { found = true; fl = sl.flags; break; }
					slot = (slot + 1) & a.slot_mask;
					sl = a.slot(slot);
				}
				if (found && !(fl & SLOT_JOINED)) a.slot(slot).flags = fl | SLOT_JOINED;
			}
		}
		const unsigned long long jb = __ballot(found);
		if (jb == 0) return;
		const unsigned k = sn + rank_in(jb);
		if (found) {
			if (k < ST) { st_slot[wave][k] = (uint32_t)slot; st_off[wave][k] = off; }
			else {                                                // staging area full (dense matches): direct append
				const unsigned long long idx = atomicAdd(a.matched_count, 1ull);
				if (idx < (unsigned long long)a.matched_cap) { a.matched_slot[idx] = (uint32_t)slot; a.matched_loc[idx] = base + off; }
			}
		}
		sn += (unsigned)__builtin_popcountll(jb);
		if (sn >= ST / 2) flush();
	};
	// a queued positive: the key of its window from the nibbles, then `probe`
	auto probe_queued = [&](bool active, uint32_t e) {
		const uint32_t off = active ? e : 0u;
		const uint64_t seed = seed_window_key(codes[off >> 4], codes[(off >> 4) + 1], off & 15u, care64);
		probe(active, seed, off);
	};
	// Rounds of B consecutive entries per lane, one 16-byte load each, from the list's last multiple of B at or below lo (the lists of
	// a shape start at a multiple of 16 entries and end at one: the loads are aligned and stay inside); what lies outside [lo, hi)
	// is dropped by `pass`. DEPTH rounds are requested ahead of the one that is probed.
	typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
	static_assert(B == 4, "one 16-byte load per round");
	const uint64_t stride = (uint64_t)B * blockDim.x, first = (lo & ~(uint64_t)(B - 1)) + (uint64_t)B * threadIdx.x;
	u32x4 hv[DEPTH];
	auto request = [&](uint64_t k, u32x4& h) {
		h = 0;
		if (k < hi) h = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(hashes + k));
	};
#pragma unroll
	for (int d = 0; d < DEPTH; ++d) request(first + (uint64_t)d * stride, hv[d]);
	for (uint64_t k0 = first; k0 < hi + (uint64_t)B * threadIdx.x; k0 += (uint64_t)DEPTH * stride) {      // (workgroup-uniform trip count: k0 - B * threadIdx.x < hi)
#pragma unroll
		for (int d = 0; d < DEPTH; ++d) {
			const u32x4 h4 = hv[d];
			const uint64_t k = k0 + (uint64_t)d * stride;
			request(k + (uint64_t)DEPTH * stride, hv[d]);
#pragma unroll
			for (int j = 0; j < B; ++j) {
				const uint32_t h = h4[j];
				// inside the slice by the slice identity (seed_slices_core.h; the launch checks its conditions). The clamp below is for
				// the entries outside [lo, hi) (another slice's, or none), which `pass` drops
				const uint32_t lw = seed_slice_word(h, a.bm1_hmask, a.bitmap1_words) - word0;
				const uint32_t bw = slice[lw < slice_words ? lw : 0u], need = bm1_bits(h, a.bitmap1_k3);
				const bool pass = k + j >= lo && k + j < hi && (bw & need) == need;
				const unsigned long long pb = __ballot(pass);
				if (pb) {
					if (pass) q_off[wave][qn + rank_in(pb)] = (uint32_t)(k + j);      // (list index: the cache holds fewer than 2^31 windows)
					qn += (unsigned)__builtin_popcountll(pb);
					if (qn >= 64) {                                      // (wavefront-uniform)
						wave_sync();
						qn -= 64;
						const uint32_t at = q_off[wave][qn + lane];
						wave_sync();
						probe_queued(true, list[at]);
					}
				}
			}
		}
	}
	wave_sync();
	probe_queued(lane < qn, lane < qn ? list[q_off[wave][lane]] : 0u);
	if (sn) flush();
}

// routing bytes of every window (seed_route_group) and the number of windows per slice
__global__ __launch_bounds__(256) void seed_route_kernel(const uint64_t* __restrict__ codes, const uint32_t* __restrict__ flags, int64_t base, int64_t n_groups, int64_t t_begin, int64_t t_end,
	int len, uint32_t care, uint64_t care64, int slice_bits, uint8_t* __restrict__ route, uint32_t* __restrict__ counts)
{
	__shared__ uint32_t hist[1 << SEED_SLICE_MAX_BITS];
	if (threadIdx.x < (1u << SEED_SLICE_MAX_BITS)) hist[threadIdx.x] = 0;
	__syncthreads();
	const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g < n_groups) {
		const int64_t p0 = base + 16 * g;
		uint8_t out[16];
		seed_route_group(codes[g], codes[g + 1], flags[g], flags[g + 1], t_begin - p0, t_end - p0, len, care, care64, slice_bits, out);
		uint32_t w[4] = { 0, 0, 0, 0 };
#pragma unroll
		for (int j = 0; j < 16; ++j) {
			w[j >> 2] |= (uint32_t)out[j] << ((j & 3) * 8);
			if (out[j] != SEED_ROUTE_NONE) atomicAdd(&hist[out[j]], 1u);
		}
		typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
		u32x4 v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
		*reinterpret_cast<u32x4*>(route + 16 * g) = v;
	}
	__syncthreads();
	if (threadIdx.x < (1u << slice_bits) && hist[threadIdx.x]) atomicAdd(&counts[threadIdx.x], hist[threadIdx.x]);
}

__global__ void seed_mask_kernel(SeedArgs a, int sid)
{
	const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (slot > a.slot_mask) return;
	const SeedSlot sl = a.slot(slot);
	if (sl.key == SEED_EMPTY || !(sl.flags & SLOT_JOINED)) return;          // a free slot is all ones
	const uint32_t count = sl.flags >> 8;
	// Search::mask_seeds evaluates the first query position of the joined group (seed_complexity.cpp:97-99) = the smallest one:
	// the lists are sorted by position. The fused pipeline has the answer in the slot (seed_lists_kernel).
	if (a.fused ? !(sl.flags & SLOT_LOWC) : seed_is_complex(a.params, sid, a.qdata + a.q_begin + (count == 1 ? sl.head : a.qlist[sl.head]))) return;
	a.slot(slot).flags = sl.flags | SLOT_ERASED;
	const int t = sid * a.params.index_chunks + seed_chunk(a.params, seed_of_key(a.params, sid, sl.key));
	for (uint32_t i = 0; i < count; ++i) {
		const uint32_t x = count == 1 ? sl.head : a.qlist[sl.head + i];
		const uint8_t old = a.mask_time[a.q_begin + x];
		if (t < old) a.mask_time[a.q_begin + x] = (uint8_t)t;       // one group per position and shape: no race within a launch
	}
}

// The same, driven by the list of joined reference positions instead of a scan over all table slots: with long seeds a block
// pair joins a few 10^4 positions against 8 M slots. Every joined position of a seed finds the same slot; the first one to set
// ERASED masks the seed's query positions.
// CHAIN (seed_chain.h): the shape's range of the shared lists comes from the counter block, walked by a bounded grid
template<bool CHAIN>
__global__ void seed_mask_joined_kernel(SeedArgs a, int sid, int64_t n_matched, SeedChain ch)
{
	int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, end = n_matched;
	if (CHAIN) {
		if (ch.ctr[chain_ctr_status(ch.S)] & CHAIN_MATCHED_OVER) return;      // incomplete lists: phase 1 runs again
		m += sid ? (int64_t)ch.ctr[sid - 1] : 0;
		end = (int64_t)ch.ctr[sid];
	}
	for (; m < end; m += (int64_t)gridDim.x * blockDim.x) {
		const uint32_t slot = a.matched_slot[m];
		const SeedSlot sl = a.slot(slot);
		if (sl.flags & SLOT_ERASED) continue;
		const uint32_t count = sl.flags >> 8;
		if (seed_is_complex(a.params, sid, a.qdata + a.q_begin + (count == 1 ? sl.head : a.qlist[sl.head]))) continue;
		if (atomicOr(&a.slot(slot).flags, (uint32_t)SLOT_ERASED) & SLOT_ERASED) continue;
		const int t = sid * a.params.index_chunks + seed_chunk(a.params, seed_of_key(a.params, sid, sl.key));
		for (uint32_t i = 0; i < count; ++i) {
			const uint32_t x = count == 1 ? sl.head : a.qlist[sl.head + i];
			const uint8_t old = a.mask_time[a.q_begin + x];
			if (t < old) a.mask_time[a.q_begin + x] = (uint8_t)t;
		}
		if (!CHAIN) return;                               // (the host-sized grid covers the list)
	}
}

// left-most rule + emission of one pair that passed the Hamming and ungapped-score filters
__device__ __forceinline__ void finish_pair(const SeedArgs& a, int sid, int chunk, const uint8_t* qmt, const int8_t* q, const int8_t* s,
	uint32_t qid, int seed_offset, int query_len, int64_t sloc, int score)
{
	if (lin_applies_left_most(a.lin_first != nullptr) && !left_most_pair(a.params, q, qmt, s, seed_offset, sid, chunk, query_len)) return;
	const unsigned long long idx = atomicAdd(a.hit_count, 1ull);
	if (idx < (unsigned long long)a.hit_cap) {
		dmnd_seed_hit h;
		h.query = qid; h.seed_offset = seed_offset; h.subject = sloc; h.score = score; h.pad = 0;
		a.hits[idx] = h;
	}
}

// everything after the Hamming filter for one (joined reference position m, query position x) pair
// q / s / qmt: the seed positions of the pair in the blocks and in mask_time[] -- or in staged copies of their surroundings
// ([-48, +80) letters, [-48, +48) mask times: everything the stage-2 code reads)
// stage-2 ungapped window score of one pair: -1 = dropped (below the cutoff, or deferred to the second pass), else the score that
// goes into the hit if the pair also passes the left-most rule
__device__ __forceinline__ int stage2_score(const SeedArgs& a, const int8_t* matrix, uint32_t slot, int64_t sloc, uint32_t x, const int8_t* q, const int8_t* s)
{
	const int64_t qp = a.q_begin + x;
	const uint32_t qid = a.qid_of[qp];
	const int query_len = (int)(a.qlimits[qid + 1] - a.qlimits[qid] - 1);
	if (!a.params.use_ungapped) return 0xFFFF;
	const int cutoff = ungapped_cutoff(a.params, query_len);
	if (!cutoff) return 0xFFFF;
	const int window = stage2_window(a.params, query_len);
	int cb, ce;
	clip_window(q - window, 2 * window, window, cb, ce);
	const int window_left = window - cb;
	const int score = ungapped_window_score(matrix, q - window_left, s - window_left, ce - cb);
	if (lin_score_is_deferred(score, a.lin_first != nullptr)) {
		// saturation depends on the SIMD batch of the reference: second pass (seed_deferred_kernel); a linearised search's batch of
		// one keeps its scalar score (linsearch_core.h)
		const unsigned long long d = atomicAdd(a.deferred_count, 1ull);
		if (d < (unsigned long long)a.deferred_cap) a.deferred[d] = SeedDeferred{ sloc, slot, x, score, 0 };
		atomicOr(&a.need_bits[slot >> 5], 1u << (slot & 31));
		return -1;
	}
	return score <= cutoff ? -1 : score;
}

__device__ __forceinline__ void post_hamming(const SeedArgs& a, int sid, uint32_t slot, uint32_t slot_flags, int chunk, int64_t sloc, uint32_t x,
	const int8_t* q, const int8_t* s, const uint8_t* qmt)
{
	const int64_t qp = a.q_begin + x;
	const uint32_t qid = a.qid_of[qp];
	const int seed_offset = (int)(qp - a.qlimits[qid]);
	int score = 0xFFFF;
	const int query_len = (int)(a.qlimits[qid + 1] - a.qlimits[qid] - 1);
	if (a.params.use_ungapped) {
		// stage-2 ungapped window score over the query window clipped at its sequence ends (stage2.h:92-113)
		const int cutoff = ungapped_cutoff(a.params, query_len);
		if (cutoff) {
			const int window = stage2_window(a.params, query_len);
			int cb, ce;
			clip_window(q - window, 2 * window, window, cb, ce);
			const int window_left = window - cb;
			score = ungapped_window_score(a.matrix, q - window_left, s - window_left, ce - cb);
			if (lin_score_is_deferred(score, a.lin_first != nullptr)) {
				// saturation depends on the SIMD batch of the reference: second pass (seed_deferred_kernel)
				const unsigned long long d = atomicAdd(a.deferred_count, 1ull);
				if (d < (unsigned long long)a.deferred_cap) a.deferred[d] = SeedDeferred{ sloc, slot, x, score, 0 };
				atomicOr(&a.need_bits[slot >> 5], 1u << (slot & 31));
				return;
			}
			if (score <= cutoff) return;
		}
	}
	finish_pair(a, sid, chunk, qmt, q, s, qid, seed_offset, query_len, sloc, score);
}

__device__ __forceinline__ void post_hamming(const SeedArgs& a, int sid, uint32_t slot, uint32_t slot_flags, int chunk, int64_t sloc, uint32_t x)
{
	post_hamming(a, sid, slot, slot_flags, chunk, sloc, x, a.qdata + a.q_begin + x, a.tdata + sloc, a.mask_time + a.q_begin + x);
}

__device__ __forceinline__ void filter_pair(const SeedArgs& a, int sid, uint32_t slot, uint32_t slot_flags, int chunk, int64_t sloc, uint32_t x)
{
	if (a.qwin && !seed_window_holds(seed_window_at(a, sloc), x)) return;
	if (fingerprint_id(a.qdata + a.q_begin + x, a.tdata + sloc) < a.params.hamming_filter_id) return;
	post_hamming(a, sid, slot, slot_flags, chunk, sloc, x);
}

// ---- linearised search (linsearch_core.h): the first joined reference position of every seed -----------------------------------
// Two kernels over the shape's joined records, on the search's stream in front of the pair filter that reads their result:
// STEP 0 writes LIN_NO_POSITION into lin_first[slot] of every slot that occurs (so the array needs no clear per search, per shape or
// per repeated phase 1: a slot is only ever read through one of the records that initialised it in this very pass), STEP 1 takes
// the 64-bit minimum of the positions per slot. Neither result depends on the order of the records. Erased seeds are reduced too
// (one read less than testing the flag; their records stop at the pair filter as ever).
// CHAIN (seed_chain.h): the shape's range of the shared lists comes from the counter block; the guard is seed_pair_kernel's.
template<bool CHAIN, int STEP>
__global__ __launch_bounds__(256) void seed_lin_first_kernel(SeedArgs a, int sid, int64_t n_matched, SeedChain ch)
{
	int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, end = n_matched;
	if (CHAIN) {
		if (ch.ctr[chain_ctr_status(ch.S)]) return;       // (incomplete lists among the reasons: nothing behind ctr[sid] is read)
		m += sid ? (int64_t)ch.ctr[sid - 1] : 0;
		end = (int64_t)ch.ctr[sid];
	}
	for (; m < end; m += (int64_t)gridDim.x * blockDim.x) {
		const uint32_t slot = a.matched_slot[m];
		if (STEP == 0) a.lin_first[slot] = LIN_NO_POSITION;
		else {
			// lin_first_update as one atomic: positions are non-negative, so the signed and the unsigned order agree
			const int64_t pos = a.matched_loc[m];
			if (lin_first_update(a.lin_first[slot], pos) == pos) atomicMin(reinterpret_cast<unsigned long long*>(&a.lin_first[slot]), (unsigned long long)pos);
		}
		if (!CHAIN) return;                               // (the host-sized grid covers the list)
	}
}

// One thread per joined reference position; the seed's query positions are a contiguous list. Work per position is the
// list length, which is heavily skewed (a frequent seed has thousands of query positions and thousands of joined reference
// positions): lists longer than LIGHT are processed by the whole wavefront, 64 query positions at a time, so that no lane
// runs a 10^4-iteration loop while the rest of the machine idles.
// The pairs that pass go to the survivor list (LDS-staged, one atomic per workgroup) for launch_seed_post -- scoring them in
// place left most lanes of a wavefront waiting for the few that passed.
// CHAIN (seed_chain.h): the shape's range of the shared lists comes from the counter block; a bounded grid walks it in tiles of
// one workgroup (a workgroup-uniform trip count: the staging area is flushed per tile)
// MLR (mutual-coverage search): the joined position's window of admissible query positions is looked up with its slot, once
// LIN (linearised search, linsearch_core.h): a joined position that is not the first of its seed has no pairs
template<bool CHAIN, bool MLR, bool LIN = false>
__global__ __launch_bounds__(128) void seed_pair_kernel(SeedArgs a, int sid, int64_t n_matched, SeedChain ch)
{
	constexpr uint32_t LIGHT = 8;
	constexpr unsigned STAGE = 1024;
	__shared__ SeedSurvivor stage[STAGE];
	__shared__ unsigned st_n;
	__shared__ unsigned long long st_base;
	int64_t first = 0, end = n_matched;
	if (CHAIN) {
		if (ch.ctr[chain_ctr_status(ch.S)]) return;       // (written by the one-thread kernels between the shapes only)
		first = sid ? (int64_t)ch.ctr[sid - 1] : 0;
		end = (int64_t)ch.ctr[sid];
	}
	auto filter = [&](uint32_t slot, int64_t sloc, uint32_t x, SeedQueryWindow win) {
		if (MLR && !seed_window_holds(win, x)) return;
		if (fingerprint_id(a.qdata + a.q_begin + x, a.tdata + sloc) < a.params.hamming_filter_id) return;
		const unsigned k = atomicAdd(&st_n, 1u);
		if (k < STAGE) stage[k] = SeedSurvivor{ slot, x, sloc };
		else {                                            // staging area full: direct append
			const unsigned long long idx = atomicAdd(a.survivor_count, 1ull);
			if (idx < (unsigned long long)a.survivor_cap) a.survivors[idx] = SeedSurvivor{ slot, x, sloc };
		}
	};
	const int lane = threadIdx.x & 63;
	for (int64_t tile = first + (int64_t)blockIdx.x * blockDim.x; tile < end; tile += (int64_t)gridDim.x * blockDim.x) {
		if (threadIdx.x == 0) st_n = 0;
		__syncthreads();
		const int64_t m = tile + threadIdx.x;
		uint32_t slot = 0, head = 0, count = 0;
		int64_t sloc = 0;
		SeedQueryWindow win{ 0, 0 };
		if (m < end) {
			slot = a.matched_slot[m];
			const SeedSlot sl = a.slot(slot);                // key, list start, size and state of the seed in one 16-byte read
			if (!(sl.flags & SLOT_ERASED)) {
				head = sl.head; count = sl.flags >> 8;
				sloc = a.matched_loc[m];
				if (MLR) win = seed_window_at(a, sloc);
				if (LIN && !lin_record_selected(sloc, a.lin_first[slot])) count = 0;
			}
		}
		if (count <= LIGHT)
			for (uint32_t i = 0; i < count; ++i) filter(slot, sloc, count == 1 ? head : a.qlist[head + i], win);
		unsigned long long heavy = __ballot(count > LIGHT);
		while (heavy) {
			const int src = __builtin_ctzll(heavy);
			heavy &= heavy - 1;
			const uint32_t h_slot = (uint32_t)__shfl((int)slot, src), h_head = (uint32_t)__shfl((int)head, src), h_count = (uint32_t)__shfl((int)count, src);
			const int64_t h_sloc = (int64_t)__shfl((long long)sloc, src);
			SeedQueryWindow h_win{ 0, 0 };
			if (MLR) { h_win.first = (uint32_t)__shfl((int)win.first, src); h_win.end = (uint32_t)__shfl((int)win.end, src); }
			for (uint32_t i = (uint32_t)lane; i < h_count; i += 64) filter(h_slot, h_sloc, a.qlist[h_head + i], h_win);
		}
		__syncthreads();
		const unsigned n = st_n < STAGE ? st_n : STAGE;
		if (n != 0) {
			if (threadIdx.x == 0) st_base = atomicAdd(a.survivor_count, (unsigned long long)n);
			__syncthreads();
			for (unsigned k = threadIdx.x; k < n; k += blockDim.x) {
				const unsigned long long idx = st_base + k;
				if (idx < (unsigned long long)a.survivor_cap) a.survivors[idx] = stage[k];
			}
		}
		if (!CHAIN) return;                               // (the host-sized grid covers the list)
		__syncthreads();
	}
}

// ---- tiled pair filter for the sensitive modes -------------------------------------------------------------------------
// With short seeds a third of the reference positions join and the Hamming filter sees ~3e9 (query, reference) window pairs
// per shape. The joined positions are first sorted by seed slot (radix sort), so that the 256 entries of a workgroup belong to
// a few seeds; per seed with a long query list the workgroup stages the 48-byte query windows in LDS, TQ at a time, and every
// thread compares them (broadcast LDS reads) with its own reference window held in 12 registers: the query windows are read
// from the cache hierarchy once per workgroup instead of once per pair.
// Pairs that pass the Hamming filter are NOT scored in place: in a wavefront only the ~10 % passing lanes would run the long
// stage-2 code while the others wait (measured: 3/4 of the kernel's time). They are staged in LDS, flushed to a compact
// survivor list with one global atomic per flush, and scored by seed_post_kernel with all lanes busy.
// MLR (mutual-coverage search): every thread holds its reference position's window of admissible query positions
// LIN (linearised search, linsearch_core.h): a thread whose joined position is not the first of its seed holds an empty entry; the one
// that is starts its seed's run wherever it stands among the entries of equal slot
template<bool MLR, bool LIN = false>
__global__ __launch_bounds__(256) void seed_pair_tiled_kernel(SeedArgs a, int sid, int64_t n_matched)
{
	constexpr uint32_t LIGHT = 8;
	constexpr int TQ = 64;
	constexpr unsigned STAGE = 1024;
	__shared__ uint32_t q_tile[TQ * 12];
	__shared__ uint32_t q_x[TQ];
	__shared__ uint32_t sh_slot[256], sh_head[256], sh_count[256], run_of[256];
	__shared__ SeedSurvivor stage[STAGE];
	__shared__ unsigned st_n;
	__shared__ unsigned long long st_base;
	__shared__ int n_runs;
	const int tid = threadIdx.x;
	const int64_t m = (int64_t)blockIdx.x * 256 + tid;
	uint32_t slot = LIST_END, head = 0, count = 0;
	int64_t sloc = 0;
	SeedQueryWindow win{ 0, 0 };
	uint32_t sw[12];
#pragma unroll
	for (int w = 0; w < 12; ++w) sw[w] = 0;
	if (m < n_matched) {
		slot = a.matched_slot[m];
		const SeedSlot sl = a.slot(slot);
		if (!(sl.flags & SLOT_ERASED)) {
			head = sl.head; count = sl.flags >> 8;
			sloc = a.matched_loc[m];
			__builtin_memcpy(sw, a.tdata + sloc - 16, 48);
			if (MLR) win = seed_window_at(a, sloc);
			if (LIN && !lin_record_selected(sloc, a.lin_first[slot])) { slot = LIST_END; head = 0; count = 0; }
		}
	}
	auto survive = [&](uint32_t x) {
		const unsigned k = atomicAdd(&st_n, 1u);
		if (k < STAGE) stage[k] = SeedSurvivor{ slot, x, sloc };
		else {                                             // staging area full between two flushes: direct append
			const unsigned long long idx = atomicAdd(a.survivor_count, 1ull);
			if (idx < (unsigned long long)a.survivor_cap) a.survivors[idx] = SeedSurvivor{ slot, x, sloc };
		}
	};
	auto flush = [&]() {                                   // block-uniform
		__syncthreads();
		const unsigned n = st_n < STAGE ? st_n : STAGE;
		if (n) {
			if (tid == 0) st_base = atomicAdd(a.survivor_count, (unsigned long long)n);
			__syncthreads();
			for (unsigned k = (unsigned)tid; k < n; k += 256) {
				const unsigned long long idx = st_base + k;
				if (idx < (unsigned long long)a.survivor_cap) a.survivors[idx] = stage[k];
			}
		}
		__syncthreads();
		if (tid == 0) st_n = 0;
		__syncthreads();
	};
	const bool heavy = count > LIGHT;
	sh_slot[tid] = heavy ? slot : LIST_END;
	sh_head[tid] = head; sh_count[tid] = count;
	if (tid == 0) { n_runs = 0; st_n = 0; }
	__syncthreads();
	if (heavy && (tid == 0 || sh_slot[tid - 1] != slot)) run_of[atomicAdd(&n_runs, 1)] = (uint32_t)tid;      // first entry of a run of equal slots
	if (count > 0 && count <= LIGHT)
		for (uint32_t i = 0; i < count; ++i) {
			const uint32_t x = count == 1 ? head : a.qlist[head + i];
			if (MLR && !seed_window_holds(win, x)) continue;
			uint32_t qw[12];
			__builtin_memcpy(qw, a.qdata + a.q_begin + x - 16, 48);
			if (window_identity(sw, qw) >= a.params.hamming_filter_id) survive(x);
		}
	flush();
	const int runs = n_runs;
	for (int r = 0; r < runs; ++r) {
		const uint32_t lt = run_of[r], r_slot = sh_slot[lt], r_head = sh_head[lt], r_count = sh_count[lt];
		for (uint32_t base = 0; base < r_count; base += TQ) {
			const int nt = (int)(r_count - base < (uint32_t)TQ ? r_count - base : (uint32_t)TQ);
			for (int idx = tid; idx < nt * 12; idx += 256) {
				const int w = idx / 12, d = idx - 12 * w;
				const uint32_t x = a.qlist[r_head + base + w];
				uint32_t v;
				__builtin_memcpy(&v, a.qdata + a.q_begin + x - 16 + 4 * d, 4);
				q_tile[idx] = v;
				if (d == 0) q_x[w] = x;
			}
			__syncthreads();
			if (heavy && slot == r_slot)
				for (int w = 0; w < nt; ++w)
					if ((!MLR || seed_window_holds(win, q_x[w])) && window_identity(sw, q_tile + 12 * w) >= a.params.hamming_filter_id) survive(q_x[w]);
			flush();
		}
	}
}

// Stage 2 for the compact list of pairs that passed the Hamming filter, in two kernels: seed_score_kernel computes the ungapped
// window score of every survivor and compacts those above the cutoff (~10 %) into a second list; seed_leftmost_kernel runs the
// left-most rule on that list and emits the hits. In one kernel the long left-most code ran for whole wavefronts in which a
// few lanes were still alive (the same divergence that the survivor list removed from the Hamming filter).
// The score kernel reads ~100 letters of both sequences one byte at a time with data-dependent bounds: from the blocks that
// was ~150 L2 requests per survivor; every thread first copies the [-48, +48) surroundings of its pair into LDS with 16-byte
// loads and the byte-wise code runs on the copies (generic pointers into LDS).
constexpr int POST_THREADS = 256, POST_BEFORE = 48, POST_LETTERS = 96;

// stage2_score for windows of at most POST_BEFORE letters to either side, on the 96 letters around the pair held in REGISTERS
// (qw / sw: 24 dwords each, letter -48 first). Until round 5 the windows were staged in LDS (53 KB per workgroup: three wavefronts
// per SIMD) and clip_window / ungapped_window_score walked them byte by byte -- three dependent LDS reads per letter, ~14 us of a
// wavefront's 28 us (profiles/r05_pmc_summary_C3.json: 15 000 x 4 cycles per wavefront for 3 000 instructions). Here the delimiter
// search is a 96-bit mask, and the score loop is unrolled over all 96 letters with the letters outside [begin, end) neutralised
// (before the window: +0 keeps the running score at its initial 0; behind it: a large negative resets it without touching the
// maximum) -- the matrix reads of a thread no longer wait for one another.
__device__ __forceinline__ int stage2_score_regs(const SeedArgs& a, const int8_t* matrix, uint32_t slot, int64_t sloc, uint32_t x, const uint32_t (&qw)[24], const uint32_t (&sw)[24])
{
	const int64_t qp = a.q_begin + x;
	const uint32_t qid = a.qid_of[qp];
	const int query_len = (int)(a.qlimits[qid + 1] - a.qlimits[qid] - 1);
	if (!a.params.use_ungapped) return 0xFFFF;
	const int cutoff = ungapped_cutoff(a.params, query_len);
	if (!cutoff) return 0xFFFF;
	const int window = stage2_window(a.params, query_len);               // <= POST_BEFORE (the caller's test)
	// clip_window(q - window, 2 window, window): delimiters of the query letters [48 - window, 48 + window) as bits
	uint64_t lo = 0, hi = 0;
#pragma unroll
	for (int i = 0; i < 96; ++i) {
		const uint64_t d = ((qw[i >> 2] >> (8 * (i & 3))) & 0xffu) == (uint32_t)L_DELIM ? 1u : 0u;
		if (i < 64) lo |= d << i; else hi |= d << (i - 64);
	}
	const uint64_t before = lo & (((uint64_t)1 << 48) - 1) & ~(((uint64_t)1 << (48 - window)) - 1);
	const int begin = before ? 64 - __builtin_clzll(before) : 48 - window;
	const uint64_t behind = ((lo >> 48) | (hi << 16)) & (window >= 48 ? ((uint64_t)1 << 48) - 1 : ((uint64_t)1 << window) - 1);
	const int end = behind ? 48 + __builtin_ctzll(behind) : 48 + window;
	int score = 0, st = 0;
#pragma unroll
	for (int n = 0; n < 96; ++n) {
		const uint32_t ql = (qw[n >> 2] >> (8 * (n & 3))) & LETTER_MASK, sl = (sw[n >> 2] >> (8 * (n & 3))) & LETTER_MASK;
		const int m = matrix[ql * 32 + sl];
		st += n < begin ? 0 : n < end ? m : -(1 << 20);
		st = imax(st, 0);
		score = imax(score, st);
	}
	if (lin_score_is_deferred(score, a.lin_first != nullptr)) {
		// saturation depends on the SIMD batch of the reference: second pass (seed_deferred_kernel); a linearised search's batch of
		// one keeps its scalar score (linsearch_core.h)
		const unsigned long long d = atomicAdd(a.deferred_count, 1ull);
		if (d < (unsigned long long)a.deferred_cap) a.deferred[d] = SeedDeferred{ sloc, slot, x, score, 0 };
		atomicOr(&a.need_bits[slot >> 5], 1u << (slot & 31));
		return -1;
	}
	return score <= cutoff ? -1 : score;
}

// CHAIN (seed_chain.h): the survivor count comes from the counter block; a bounded grid walks the list in tiles of one workgroup
template<bool CHAIN>
__global__ __launch_bounds__(POST_THREADS) void seed_score_kernel(SeedArgs a, int sid, int64_t n_survivors, SeedChain ch)
{
	constexpr unsigned STAGE = POST_THREADS;
	__shared__ int8_t matrix[32 * 32];
	__shared__ SeedScored stage[STAGE];
	__shared__ unsigned st_n;
	__shared__ unsigned long long st_base;
	if (CHAIN) {
		if (ch.ctr[chain_ctr_status(ch.S)]) return;
		n_survivors = (int64_t)*a.survivor_count;
		if (n_survivors > a.survivor_cap) return;          // an incomplete list: the host runs the shape's pair filter again
	}
	for (int i = threadIdx.x; i < 1024; i += blockDim.x) matrix[i] = a.matrix[i];
	for (int64_t tile = (int64_t)blockIdx.x * blockDim.x; tile < n_survivors; tile += (int64_t)gridDim.x * blockDim.x) {
		if (threadIdx.x == 0) st_n = 0;
		__syncthreads();
		const int64_t i = tile + threadIdx.x;
		// (the kernel argument is not modified: a private copy of the 3 KB struct would live in scratch memory)
		if (i < n_survivors) {
			const SeedSurvivor sv = a.survivors[i];
			const SeedSlot sl = a.slot(sv.slot);
			if (!(sl.flags & SLOT_ERASED)) {                  // (the fused stream kernel never lets a pair of a non-complex seed through)
				const int64_t qp = a.q_begin + sv.x;
				int score;
				// windows wider than the staged stretch (--ungapped-window above 48; short translated frames use their whole length): from the blocks
				if (a.params.query_translated || a.params.ungapped_window > POST_BEFORE) score = stage2_score(a, matrix, sv.slot, sv.sloc, sv.x, a.qdata + qp, a.tdata + sv.sloc);
				else {
					uint32_t qw[24], sw[24];
#pragma unroll
					for (int k = 0; k < POST_LETTERS / 16; ++k) {
						uint4 v, w;
						__builtin_memcpy(&v, a.qdata + qp - POST_BEFORE + 16 * k, 16);
						__builtin_memcpy(&w, a.tdata + sv.sloc - POST_BEFORE + 16 * k, 16);
						qw[4 * k] = v.x; qw[4 * k + 1] = v.y; qw[4 * k + 2] = v.z; qw[4 * k + 3] = v.w;
						sw[4 * k] = w.x; sw[4 * k + 1] = w.y; sw[4 * k + 2] = w.z; sw[4 * k + 3] = w.w;
					}
					score = stage2_score_regs(a, matrix, sv.slot, sv.sloc, sv.x, qw, sw);
				}
				if (score >= 0)
					stage[atomicAdd(&st_n, 1u)] = SeedScored{ sv.slot, sv.x, sv.sloc, score, seed_chunk(a.params, seed_of_key(a.params, sid, sl.key)) };
			}
		}
		__syncthreads();
		const unsigned n = st_n;
		if (n != 0) {
			if (threadIdx.x == 0) st_base = atomicAdd(a.scored_count, (unsigned long long)n);
			__syncthreads();
			if (threadIdx.x < n) a.scored[st_base + threadIdx.x] = stage[threadIdx.x];
		}
		if (!CHAIN) return;                               // (the host-sized grid covers the list)
		__syncthreads();
	}
}

// The left-most rule's windows with wide loads (LmBytewise's counterpart, seed_core.h). The byte-wise form walks up to 96 + 49 + 49
// + 49 letters with one dependent load each, and looks every letter's class up in the parameter block: ~150 us of latency per
// survivor however few there are (0.16 ms of every C2 step for 20 k survivors). Here a window is six or four 16-byte loads issued
// together, delimiters are found with a zero-byte test per dword, classes come from the two 64-bit nibble maps of the stream kernel.
struct LmWide {
	uint64_t map_lo, map_hi;
	int reduction_ok;                                              // classes fit a nibble (else the byte-wise form)
	// bit x of the result: byte x of the dword equals v (exact, no carries between bytes)
	static __device__ __forceinline__ uint32_t eq_bytes(uint32_t x, uint32_t v)
	{
		const uint32_t t = x ^ (v * 0x01010101u);
		const uint32_t y = ~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & 0x80808080u;
		return ((y >> 7) & 1u) | ((y >> 14) & 2u) | ((y >> 21) & 4u) | ((y >> 28) & 8u);
	}
	__device__ void clip(const int8_t* seq, int len, int anchor, int& b, int& e) const
	{
		if (len > 96 || anchor > 63) { clip_window(seq, len, anchor, b, e); return; }
		uint32_t w[24];
		__builtin_memcpy(w, seq, 96);                                // the blocks carry 256 padding letters: reading past len is safe
		uint64_t lo = 0;
		uint32_t hi = 0;
#pragma unroll
		for (int x = 0; x < 16; ++x) lo |= (uint64_t)eq_bytes(w[x], (uint32_t)L_DELIM) << (4 * x);
#pragma unroll
		for (int x = 16; x < 24; ++x) hi |= eq_bytes(w[x], (uint32_t)L_DELIM) << (4 * (x - 16));
		if (len < 64) { lo &= (1ull << len) - 1; hi = 0; }
		else if (len < 96) hi &= (1u << (len - 64)) - 1;
		b = 0; e = len;
		const uint64_t below = lo & ((1ull << anchor) - 1), above = lo >> anchor;
		if (below) b = 64 - __builtin_clzll(below);
		if (above) e = anchor + __builtin_ctzll(above);
		else if (hi) e = 64 + __builtin_ctz(hi);
	}
	__device__ void masks(const SeedParams& c, const int8_t* qq, const int8_t* ss, const uint8_t* mm, int w, int t_now, uint64_t& match, uint64_t& masked) const
	{
		if (!reduction_ok) { match = reduced_match(c, qq, ss, w); masked = seed_mask_bits(mm, w, t_now); return; }
		uint32_t qw[16], sw[16], mw[16];
		__builtin_memcpy(qw, qq, 64); __builtin_memcpy(sw, ss, 64); __builtin_memcpy(mw, mm, 64);
		uint64_t m = 0, k = 0;
#pragma unroll
		for (int x = 0; x < 16; ++x) {
			uint32_t eq = 0, ms = 0;
#pragma unroll
			for (int y = 0; y < 4; ++y) {
				const uint32_t lq = (qw[x] >> (8 * y)) & LETTER_MASK, ls = (sw[x] >> (8 * y)) & LETTER_MASK;
				const bool bad = lq == L_MASK || lq == L_STOP || lq == L_DELIM || ls == L_MASK || ls == L_STOP || ls == L_DELIM;
				const uint32_t cq = (uint32_t)(((lq & 16) ? map_hi : map_lo) >> ((lq & 15) * 4)) & 15u, cs = (uint32_t)(((ls & 16) ? map_hi : map_lo) >> ((ls & 15) * 4)) & 15u;
				eq |= (uint32_t)(!bad && cq == cs) << y;
				ms |= (uint32_t)((int)((mw[x] >> (8 * y)) & 0xffu) <= t_now) << y;
			}
			m |= (uint64_t)eq << (4 * x);
			k |= (uint64_t)ms << (4 * x);
		}
		const uint64_t keep = w >= 64 ? ~0ull : (1ull << (w < 0 ? 0 : w)) - 1;
		match = m & keep;
		masked = k & keep;
	}
};

// left-most rule + emission over the scored list, whose size is only known on the device (~10 % of the survivors): a bounded grid
// walks it in strides (up to round 6 the grid covered the upper bound, the number of survivors: on C3 70 000 workgroups per shape of
// which nine in ten read the count and left). 0.12-0.14 ms per C3 shape by itself; the 0.70 ms average of the committed C3 statistics
// is what a small kernel shows when it shares the chip with the other seed stage's stream kernel, not work (tools/gpu_r06ab.sh).
__global__ __launch_bounds__(256) void seed_leftmost_kernel(SeedArgs a, int sid, uint64_t map_lo, uint64_t map_hi, int reduction_ok)
{
	const int lane = threadIdx.x & 63;
	const unsigned long long n = *a.scored_count, stride = (unsigned long long)gridDim.x * blockDim.x;
	for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; (i & ~63ull) < n; i += stride) {      // (wavefront-uniform trip count)
		bool keep = false;
		SeedScored sc{};
		uint32_t qid = 0;
		int seed_offset = 0;
		if (i < n) {
			sc = a.scored[i];
			const int64_t qp = a.q_begin + sc.x;
			qid = a.qid_of[qp];
			seed_offset = (int)(qp - a.qlimits[qid]);
			const int query_len = (int)(a.qlimits[qid + 1] - a.qlimits[qid] - 1);
			// (a linearised search skips the rule, linsearch_core.h: every scored pair is a hit)
			keep = !lin_applies_left_most(a.lin_first != nullptr) || left_most_pair_t(LmWide{ map_lo, map_hi, reduction_ok }, a.params, a.qdata + qp, a.mask_time + qp, a.tdata + sc.sloc, seed_offset, sid, sc.chunk, query_len);
		}
		// one atomic on the hit counter per wavefront
		const unsigned long long mask = __ballot(keep);
		if (mask == 0) continue;
		unsigned long long base = 0;
		const int leader = __builtin_ctzll(mask);
		if (lane == leader) base = atomicAdd(a.hit_count, (unsigned long long)__builtin_popcountll(mask));
		base = (unsigned long long)__shfl((long long)base, leader);
		if (!keep) continue;
		const unsigned long long idx = base + (unsigned long long)__builtin_popcountll(mask & ((1ull << lane) - 1));
		if (idx < (unsigned long long)a.hit_cap) {
			dmnd_seed_hit h;
			h.query = qid; h.seed_offset = seed_offset; h.subject = sc.sloc; h.score = sc.score; h.pad = 0;
			a.hits[idx] = h;
		}
	}
}

// copies the joined positions of the seeds that have deferred pairs (need_bits) as sort keys slot << 40 | position.
// 4096 list entries per workgroup and ONE atomic on the shared counter for them: with the joined positions in stream order the
// wanted entries are spread over the whole list, and an atomic per wavefront that holds one (1.2 M of them per shape in
// --sensitive, ~4.5 ns each on one address) was 5 ms of a 0.3 ms scan.
__global__ __launch_bounds__(256) void seed_collect_kernel(SeedArgs a, int64_t n_matched)
{
	constexpr int PER = 16;
	__shared__ unsigned n_local;
	__shared__ unsigned long long base;
	if (threadIdx.x == 0) n_local = 0;
	__syncthreads();
	const int64_t m0 = (int64_t)blockIdx.x * (256 * PER) + threadIdx.x;
	uint32_t mine = 0;
#pragma unroll
	for (int j = 0; j < PER; ++j) {
		const int64_t m = m0 + (int64_t)j * 256;
		if (m < n_matched) {
			const uint32_t slot = a.matched_slot[m];
			mine |= ((a.need_bits[slot >> 5] >> (slot & 31)) & 1u) << j;
		}
	}
	unsigned off = mine ? atomicAdd(&n_local, (unsigned)__builtin_popcount(mine)) : 0u;
	__syncthreads();
	if (n_local == 0) return;
	if (threadIdx.x == 0) base = atomicAdd(a.e_count, (unsigned long long)n_local);
	__syncthreads();
	while (mine) {
		const int j = __builtin_ctz(mine);
		mine &= mine - 1;
		const int64_t m = m0 + (int64_t)j * 256;
		a.e_key[base + off++] = ((uint64_t)a.matched_slot[m] << 40) | (uint64_t)a.matched_loc[m];
	}
}

// The same for the 10^7-10^8 joined positions of a short-seed shape (C3: 8.1e7 per shape, of which the ~10^4 seeds with a deferred
// pair own a few thousand). One need_bits test per joined position is one L2 request per position -- the request rate of the L2s,
// not the 4 bytes per position, set the 0.42 ms the kernel above took there. Here the need map is first folded to 2^18 bits
// (seed_need_fold_kernel: bit b = OR of the map's bits b + k 2^18), every workgroup keeps the folded map in LDS and walks many
// tiles; only positions whose folded bit is set (a few per cent) go on to the exact test.
__global__ void seed_need_fold_kernel(const uint32_t* __restrict__ need_bits, uint64_t words, uint32_t* __restrict__ fold, uint32_t fold_words)
{
	const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
	if (w >= fold_words) return;
	uint32_t x = 0;
	for (uint64_t i = w; i < words; i += fold_words) x |= need_bits[i];
	fold[w] = x;
}

__global__ __launch_bounds__(256) void seed_collect_folded_kernel(SeedArgs a, int64_t n_matched, const uint32_t* __restrict__ fold, uint32_t fold_words)
{
	constexpr int PER = 16;
	constexpr unsigned HOLD = 1024;                        // wanted entries a workgroup keeps before it claims room in the output
	extern __shared__ uint32_t filt[];                     // fold_words (a power of two) words
	__shared__ uint64_t held[HOLD];
	__shared__ unsigned n_local, n_held;
	__shared__ unsigned long long base;
	for (uint32_t i = threadIdx.x * 4; i < fold_words; i += 256 * 4)
		*reinterpret_cast<uint4*>(&filt[i]) = *reinterpret_cast<const uint4*>(&fold[i]);
	if (threadIdx.x == 0) n_held = 0;
	// the held entries go out: ONE returning atomic on the shared counter (a memory-side round trip the whole workgroup waits for --
	// per tile, as the kernel above does it, that wait was most of a tile's time here: nearly every tile of a short-seed shape holds
	// a wanted position)
	auto flush = [&]() {                                   // (called by all threads)
		__syncthreads();
		const unsigned n = n_held;
		if (n == 0) return;
		if (threadIdx.x == 0) base = atomicAdd(a.e_count, (unsigned long long)n);
		__syncthreads();
		for (unsigned i = threadIdx.x; i < n; i += 256) a.e_key[base + i] = held[i];
		__syncthreads();
		if (threadIdx.x == 0) n_held = 0;
		__syncthreads();
	};
	const int64_t tiles = (n_matched + 256 * PER - 1) / (256 * PER);
	for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
		__syncthreads();                                   // the filter is filled; the previous tile's counters have been read
		if (threadIdx.x == 0) n_local = 0;
		__syncthreads();
		const int64_t m0 = tile * (256 * PER) + threadIdx.x;
		uint32_t slot[PER];
#pragma unroll
		for (int j = 0; j < PER; ++j) {
			const int64_t m = m0 + (int64_t)j * 256;
			slot[j] = m < n_matched ? a.matched_slot[m] : 0xffffffffu;
		}
		// folded test of all sixteen first, then the exact words of the few candidates as independent loads behind one wait
		uint32_t cand = 0;
#pragma unroll
		for (int j = 0; j < PER; ++j)
			cand |= (slot[j] != 0xffffffffu ? (filt[(slot[j] >> 5) & (fold_words - 1)] >> (slot[j] & 31)) & 1u : 0u) << j;
		uint32_t exact[PER];
#pragma unroll
		for (int j = 0; j < PER; ++j) exact[j] = (cand >> j) & 1u ? a.need_bits[slot[j] >> 5] : 0u;
		uint32_t mine = 0;
#pragma unroll
		for (int j = 0; j < PER; ++j) mine |= ((exact[j] >> (slot[j] & 31)) & 1u) << j;
		unsigned off = mine ? atomicAdd(&n_local, (unsigned)__builtin_popcount(mine)) : 0u;
		__syncthreads();
		const unsigned n = n_local;
		if (n == 0) continue;
		if (n > HOLD) {                                       // a tile of wanted positions only: straight to the output
			if (threadIdx.x == 0) base = atomicAdd(a.e_count, (unsigned long long)n);
			__syncthreads();
			while (mine) {
				const int j = __builtin_ctz(mine);
				mine &= mine - 1;
				a.e_key[base + off++] = ((uint64_t)slot[j] << 40) | (uint64_t)a.matched_loc[m0 + (int64_t)j * 256];
			}
			continue;
		}
		if (n_held + n > HOLD) flush();                     // (uniform: n_held only changes between barriers)
		const unsigned at = n_held;
		while (mine) {
			const int j = __builtin_ctz(mine);
			mine &= mine - 1;
			held[at + off++] = ((uint64_t)slot[j] << 40) | (uint64_t)a.matched_loc[m0 + (int64_t)j * 256];
		}
		__syncthreads();
		if (threadIdx.x == 0) n_held = at + n;
	}
	flush();
}

// One wavefront per deferred pair: the lanes share the scan over the tile of the seed's joined positions (up to tile_size
// Hamming comparisons at random places of the reference -- as one thread's loop that was a 0.7 ms tail per shape for 10^4 pairs).
// Same arithmetic as simd_batch_size_sorted (seed_core.h), which the CPU emulation of this kernel uses.
// MLR (mutual-coverage search): the reference forms its batches behind the length test, so a joined position of the tile whose target
// fails it against this query is no batch mate (the tiles are still cut over all joined positions of the seed). Deferred pairs are
// few: the target of every mate is searched for here.
template<bool MLR>
__global__ __launch_bounds__(256) void seed_deferred_kernel(SeedArgs a, int sid, int64_t n_deferred)
{
	const int lane = threadIdx.x & 63;
	const int64_t d = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	if (d >= n_deferred) return;                          // wave-uniform
	const SeedDeferred r = a.deferred[d];
	const uint32_t slot = r.slot;
	const int64_t sloc = r.sloc;
	// the seed's joined positions: range of `slot` in the sorted copy. The keys are sorted by (slot, position), so all three searches
	// are lower bounds of a 64-bit key; the 64 lanes probe 64 places of the range at a time (three rounds for 2.5e5 keys where the
	// one-probe-per-round search, which every lane used to repeat for itself, made eighteen dependent reads)
	const uint64_t LOC = ((uint64_t)1 << 40) - 1;
	auto lower_bound64 = [&](int64_t lo, int64_t hi, uint64_t key) -> int64_t {       // first index in [lo, hi) whose key is >= `key`
		while (hi - lo > 64) {
			const int64_t chunk = (hi - lo + 63) >> 6, at = lo + (int64_t)lane * chunk;
			const int c = __builtin_popcountll(__ballot(at < hi && a.e_key[at] < key));      // the first c probes lie below the key
			const int64_t new_hi = c < 64 ? (lo + (int64_t)c * chunk < hi ? lo + (int64_t)c * chunk : hi) : hi;
			lo = c > 0 ? lo + (int64_t)(c - 1) * chunk + 1 : lo;
			hi = c > 0 ? new_hi : lo;
		}
		return lo + __builtin_popcountll(__ballot(lo + lane < hi && a.e_key[lo + lane] < key));
	};
	const int64_t b = lower_bound64(0, a.e_n, (uint64_t)slot << 40);
	const int64_t e = lower_bound64(b, a.e_n, ((uint64_t)slot + 1) << 40);
	const uint64_t* locs = a.e_key + b;
	const int64_t n = e - b;
	const int64_t qp = a.q_begin + r.x;
	const int8_t* q = a.qdata + qp;
	const int8_t* s = a.tdata + sloc;
	const int64_t rank = lower_bound64(b, e, ((uint64_t)slot << 40) | (uint64_t)sloc) - b, T = a.params.tile_size;      // rank = number of positions < sloc
	int64_t t_lo = 0, t_hi = n;
	if (T > 0 && n > T) { t_lo = rank / T * T; t_hi = t_lo + T < n ? t_lo + T : n; }
	int L = 0, rr = 0;
	for (int64_t k = t_lo + lane; k < t_hi; k += 64) {
		if (MLR && !seed_window_holds(seed_window_at(a, (int64_t)(locs[k] & LOC)), r.x)) continue;
		if (fingerprint_id(q, a.tdata + (int64_t)(locs[k] & LOC)) < a.params.hamming_filter_id) continue;
		++L; rr += k < rank;
	}
	for (int o = 32; o > 0; o >>= 1) { L += __shfl_xor(L, o); rr += __shfl_xor(rr, o); }
	if (lane != 0) return;
	const int lanes = a.params.simd_lanes, left = L - rr / lanes * lanes;
	int score = r.score;
	if ((left < lanes ? left : lanes) >= 4) score = 255;
	const uint32_t qid = a.qid_of[qp];
	const int query_len = (int)(a.qlimits[qid + 1] - a.qlimits[qid] - 1);
	if (score <= ungapped_cutoff(a.params, query_len)) return;
	finish_pair(a, sid, seed_chunk(a.params, seed_of_key(a.params, sid, a.slot(slot).key)), a.mask_time + qp, q, s, qid, (int)(qp - a.qlimits[qid]), query_len, sloc, score);
}

// DMND_TRACE: number of (joined reference position, query position) pairs the Hamming filter sees
__global__ void seed_count_pairs_kernel(SeedArgs a, int64_t n_matched, unsigned long long* out)
{
	const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	unsigned long long n = 0;
	if (m < n_matched) {
		const SeedSlot sl = a.slot(a.matched_slot[m]);
		if (!(sl.flags & SLOT_ERASED)) n = sl.flags >> 8;
	}
	for (int o = 32; o > 0; o >>= 1) n += (unsigned long long)__shfl_down((long long)n, o);
	if ((threadIdx.x & 63) == 0 && n) atomicAdd(out, n);
}

static unsigned blocks_for(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

hipError_t launch_seed_qid(const int64_t* limits, int64_t n_seqs, uint32_t* qid_of, hipStream_t st)
{
	if (n_seqs == 0) return hipSuccess;
	hipLaunchKernelGGL(seed_qid_kernel, dim3(blocks_for(n_seqs * 64, 256)), dim3(256), 0, st, limits, n_seqs, qid_of);
	return hipGetLastError();
}

// Mutual-coverage search: one lane per target. Both blocks are length-sorted, so the queries whose length passes against the
// target's are a range of query ids (length_window_of: two binary searches over length_ratio_passes itself) and their letters a
// range of query positions.
__global__ void seed_qwin_kernel(const int64_t* __restrict__ qlimits, int64_t n_queries, const int64_t* __restrict__ tlimits, int64_t n_targets, double mlr, SeedQueryWindow* __restrict__ qwin)
{
	const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n_targets) return;
	int64_t first, end;
	length_window_of(LengthsOfLimits{ qlimits }, n_queries, tlimits[t + 1] - tlimits[t] - 1, mlr, &first, &end);
	const int64_t q_begin = qlimits[0];
	qwin[t] = first < end ? SeedQueryWindow{ (uint32_t)(qlimits[first] - q_begin), (uint32_t)(qlimits[end] - q_begin) } : SeedQueryWindow{ 0, 0 };
}

hipError_t launch_seed_qwin(const int64_t* qlimits, int64_t n_queries, const int64_t* tlimits, int64_t n_targets, double min_length_ratio, SeedQueryWindow* qwin, hipStream_t st)
{
	if (n_targets == 0) return hipSuccess;
	hipLaunchKernelGGL(seed_qwin_kernel, dim3(blocks_for(n_targets, 256)), dim3(256), 0, st, qlimits, n_queries, tlimits, n_targets, min_length_ratio, qwin);
	return hipGetLastError();
}

hipError_t launch_seed_soft_time(const SeedArgs& a, hipStream_t st)
{
	hipLaunchKernelGGL(seed_soft_time_kernel, dim3(blocks_for(a.q_end - a.q_begin, 256)), dim3(256), 0, st, a);
	return hipGetLastError();
}

// class nibbles and flag maps of 16 reference letters (the decode of seed_stream_fast_kernel, once per search instead of once per
// shape and class)
__global__ void seed_codes_kernel(const int8_t* __restrict__ tseed, int64_t base, int64_t n_groups, uint64_t map_lo, uint64_t map_hi, int hashed, uint64_t* __restrict__ codes, uint32_t* __restrict__ flags,
	uint64_t* __restrict__ planes)
{
	const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= n_groups) return;
	typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
	const u32x4 v = *reinterpret_cast<const u32x4*>(tseed + base + 16 * g);
	const uint32_t w[4] = { v.x, v.y, v.z, v.w };
	uint64_t code = 0;
	uint32_t delim = 0, bad = 0, p01 = 0, p23 = 0;          // bit planes 0 | 1 << 16 and 2 | 3 << 16 of the nibbles
#pragma unroll
	for (int j = 0; j < 16; ++j) {
		const uint32_t l = (w[j >> 2] >> ((j & 3) * 8)) & LETTER_MASK;
		const uint32_t c = reduce4(l, map_lo, map_hi);
		const uint32_t stored = hashed && c == 15u ? 0u : c;
		code |= (uint64_t)stored << (j * 4);
		p01 |= ((stored & 1u) | ((stored & 2u) << 15)) << j;
		p23 |= (((stored >> 2) & 1u) | ((stored & 8u) << 13)) << j;
		delim |= (l == L_DELIM ? 1u : 0u) << j;
		bad |= (c == 15u ? 1u : 0u) << j;
	}
	codes[g] = code;
	flags[g] = delim | (bad << 16);
	if (planes) planes[g] = (uint64_t)p01 | ((uint64_t)p23 << 32);      // (NULL: the sliced stream's cache wants the nibbles only)
}

hipError_t launch_seed_codes(const SeedParams& c, const int8_t* tseed, int64_t t_begin, int64_t t_end, uint64_t* codes, uint32_t* flags, uint64_t* planes, hipStream_t st)
{
	uint64_t lo = 0, hi = 0;
	for (int l = 0; l < 32; ++l) {
		const uint64_t code = c.reduction[l] == L_MASK ? 15u : (uint64_t)c.reduction[l];
		(l < 16 ? lo : hi) |= code << ((l & 15) * 4);
	}
	const int64_t n = seed_code_groups(t_begin, t_end);
	hipLaunchKernelGGL(seed_codes_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, tseed, t_begin & ~(int64_t)15, n, lo, hi, c.seed_encoding == SEED_HASHED ? 1 : 0, codes, flags, planes);
	return hipGetLastError();
}

// Per shape: which windows are valid seeds, and of which key class -- one 16-bit map per group of 16 window starts and class (plane c
// of `out`; plane 8: the HASHED mode's windows with a mask / stop letter). The eight class workgroups of the stream then read a map
// instead of each evaluating every window (that alone was 46 of 124 s of workgroup time over the 16 shapes of C3).
// Round 5: all 16 windows of a group at once, on bit planes. seed_class is GF(2)-linear in the key (shifts and XORs only), so the
// class of the window at w is the XOR over the shape's care positions i and the four nibble bits b of
// [bit b of letter w + i] * seed_class(1 << (4 i + b)): with the letters' nibbles bit-sliced (SeedArgs::tplanes), bit j of the class
// of all 16 windows is an XOR of shifted planes, and the "valid window" tests are ORs of shifted delimiter / bad-letter maps.
// ~150 integer operations per group where the window-by-window form spent ~1000; with the 8-byte stores below 0.335 -> 0.28 ms per
// shape and 3e8 letters (C3; neither change alone moved it by more than 0.03 ms).
// The care positions grouped by their coefficient word coef = seed_class(1 << (4 pos + b)) << (3 b), b = 0..3 (seed_class has two: nibbles
// 0 and 8 of the key, and the rest): the planes of a group's positions are XORed first, the coefficients applied once per group.
struct SeedClassCoef { int n, n_groups; int8_t pos[16]; int8_t start[17]; uint16_t coef[16]; };       // group t = pos[start[t] .. start[t + 1])
// Four consecutive groups per thread: a plane is written as one 8-byte store per thread (the planes' stride is a multiple of four
// groups, seed_api.hip) -- with the arithmetic gone the kernel is its stores, 16 B out against 12 B in per group.
__global__ __launch_bounds__(256) void seed_classify_kernel(SeedArgs a, int sid, int64_t base, int64_t n_groups, SeedClassCoef cc, int hashed, uint16_t* __restrict__ out)
{
	const int64_t g0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
	if (g0 >= n_groups) return;
	// the thread's four groups and the one behind them (their windows reach into it)
	uint64_t q[5];
	uint32_t f[5];
	if (g0 + 4 <= n_groups) {
		typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
		typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
		const u64x2 x = *reinterpret_cast<const u64x2*>(a.tplanes + g0), y = *reinterpret_cast<const u64x2*>(a.tplanes + g0 + 2);
		const u32x4 z = *reinterpret_cast<const u32x4*>(a.tflags + g0);
		q[0] = x.x; q[1] = x.y; q[2] = y.x; q[3] = y.y;
		f[0] = z.x; f[1] = z.y; f[2] = z.z; f[3] = z.w;
		q[4] = g0 + 4 < n_groups ? a.tplanes[g0 + 4] : 0;
		f[4] = g0 + 4 < n_groups ? a.tflags[g0 + 4] : 0xffffu;
	}
	else {
#pragma unroll
		for (int k = 0; k < 5; ++k) { q[k] = g0 + k < n_groups ? a.tplanes[g0 + k] : 0; f[k] = g0 + k < n_groups ? a.tflags[g0 + k] : 0xffffu; }
	}
	const int len = a.params.shape_len[sid];
	uint64_t m[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
	for (int t = 0; t < 4; ++t) {
		const int64_t p0 = base + 16 * (g0 + t);
		const uint64_t q0 = q[t], q1 = q[t + 1];
		const uint32_t f0 = f[t], f1 = f[t + 1];
		const uint32_t delim = (f0 & 0xffffu) | (f1 << 16), bad = (f0 >> 16) | (f1 & 0xffff0000u);
		uint32_t plane[4];                                  // bit u = bit b of the nibble of letter p0 + u, u < 32
#pragma unroll
		for (int b = 0; b < 4; ++b) plane[b] = (uint32_t)((q0 >> (16 * b)) & 0xffffu) | ((uint32_t)((q1 >> (16 * b)) & 0xffffu) << 16);
		uint32_t cls[3] = { 0, 0, 0 };
		uint32_t bad_any = 0;                               // bit w: a mask / stop letter at a care position of window w
		for (int grp = 0; grp < cc.n_groups; ++grp) {       // (uniform: scalar loop control and branches)
			uint32_t sum[4] = { 0, 0, 0, 0 };
			for (int k = cc.start[grp]; k < cc.start[grp + 1]; ++k) {
				const int i = cc.pos[k];
#pragma unroll
				for (int b = 0; b < 4; ++b) sum[b] ^= plane[b] >> i;
				bad_any |= bad >> i;
			}
			const uint32_t coef = cc.coef[grp];
#pragma unroll
			for (int b = 0; b < 4; ++b)
#pragma unroll
				for (int j = 0; j < 3; ++j) if ((coef >> (3 * b + j)) & 1u) cls[j] ^= sum[b];
		}
		// bit w: a delimiter / a bad letter among the window's len letters: [w, w + len) = [w, w + p) u [w + len - p, w + len), p = the
		// largest power of two <= len, and runs of p by doubling
		uint32_t delim_any = delim, bad_span = bad;
		int p = 1;
		while (2 * p <= len) { delim_any |= delim_any >> p; bad_span |= bad_span >> p; p *= 2; }
		delim_any |= delim_any >> (len - p); bad_span |= bad_span >> (len - p);
		const int64_t first = a.t_begin - p0, last = a.t_end - p0;
		const uint32_t from = first <= 0 ? 0xffffu : first >= 16 ? 0u : (0xffffu << first) & 0xffffu;
		const uint32_t to = last >= 16 ? 0xffffu : last <= 0 ? 0u : (1u << last) - 1;
		const uint32_t inside = g0 + t < n_groups ? from & to & ~delim_any & 0xffffu : 0u;
		const uint32_t ok = inside & ~(hashed ? bad_span : bad_any);
#pragma unroll
		for (int c = 0; c < 8; ++c) {
			const uint32_t eq = (c & 1 ? cls[0] : ~cls[0]) & (c & 2 ? cls[1] : ~cls[1]) & (c & 4 ? cls[2] : ~cls[2]);
			m[c] |= (uint64_t)(ok & eq) << (16 * t);
		}
		m[8] |= (uint64_t)(inside & ~ok) << (16 * t);
	}
	const bool whole = g0 + 4 <= n_groups && (a.tclass_stride & 3) == 0;
#pragma unroll
	for (int c = 0; c < 9; ++c) {
		if (c == 8 && !hashed) break;
		uint16_t* o = out + (int64_t)c * a.tclass_stride + g0;
		if (whole) *reinterpret_cast<uint64_t*>(o) = m[c];
		else for (int t = 0; t < 4 && g0 + t < n_groups; ++t) o[t] = (uint16_t)(m[c] >> (16 * t));
	}
}

hipError_t launch_seed_fold(const int8_t* data, int64_t n, uint8_t* out, hipStream_t st)
{
	if (n <= 0) return hipSuccess;
	hipLaunchKernelGGL(seed_fold_kernel, dim3(blocks_for((n + 1) / 2, 256)), dim3(256), 0, st, data, n, out);
	return hipGetLastError();
}

hipError_t launch_seed_reset(const SeedArgs& a, int sid, hipStream_t st)
{
	hipLaunchKernelGGL(seed_reset_slots_kernel, dim3(blocks_for((int64_t)a.slot_mask + 1, 256)), dim3(256), 0, st, a);
	if (a.params.seed_encoding == SEED_HASHED)
		hipLaunchKernelGGL(seed_hashed_lowc_kernel, dim3(blocks_for(a.q_end - a.q_begin, 256)), dim3(256), 0, st, a, sid);
	return hipGetLastError();
}

hipError_t launch_seed_build(const SeedArgs& a, int sid, uint32_t* qlist, uint32_t* work, uint32_t* top, void** tmp, size_t* tmp_bytes, hipStream_t st)
{
	const int64_t n = a.q_end - a.q_begin;
	if (n <= 0) return hipSuccess;
	uint32_t* skey = work;                      // sort keys; then the long runs' scratch; then the placement
	uint32_t* len = work + n;
	uint32_t* ctr = work + 2 * n;
	uint32_t* wrap = work + 2 * n + 64;
	uint64_t* keys = reinterpret_cast<uint64_t*>(work + ((3 * n + 65) & ~(int64_t)1));
	if (seed_nibble_mode(a.params, sid)) {
		uint64_t lo, hi, care64 = 0;
		seed_class_maps(a.params, lo, hi);
		for (int k = 0; k < a.params.shape_weight[sid]; ++k) care64 |= (uint64_t)15 << (4 * a.params.shape_pos[sid][k]);
		const int64_t base = a.q_begin & ~(int64_t)15;
		const dim3 grid(blocks_for(a.q_end - base, 4096));
		if (a.params.seed_encoding == SEED_HASHED) hipLaunchKernelGGL(seed_order16_kernel<true>, grid, dim3(256), 0, st, a, sid, lo, hi, base, care64, skey, keys, ctr);
		else hipLaunchKernelGGL(seed_order16_kernel<false>, grid, dim3(256), 0, st, a, sid, lo, hi, base, care64, skey, keys, ctr);
	}
	else hipLaunchKernelGGL(seed_order_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, a, sid, skey, keys, ctr);
	// the sentinel 1 << slot_bits must sort last: slot_bits + 1 key bits (C2: 24 = three radix passes)
	const unsigned end_bit = (unsigned)(a.slot_bits + 1);
	rocprim::counting_iterator<uint32_t> iota(0);
	rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, SeedPlaceIn, uint64_t> place_in(iota, SeedPlaceIn{ len, top });
	rocprim::transform_output_iterator<uint32_t*, SeedPlaceOut> place_out(skey, SeedPlaceOut());
	size_t need_sort = 0, need_scan = 0;
	hipError_t e = rocprim::radix_sort_pairs(nullptr, need_sort, skey, top, iota, qlist, (size_t)n, 0, end_bit, st);
	if (e != hipSuccess) return e;
	e = rocprim::inclusive_scan(nullptr, need_scan, place_in, place_out, (size_t)n, SeedPlaceOp(), st);
	if (e != hipSuccess) return e;
	const size_t need = std::max(need_sort, need_scan);
	if (need > *tmp_bytes) {
		if (*tmp) (void)hipFree(*tmp);
		*tmp = nullptr; *tmp_bytes = 0;
		e = hipMalloc(tmp, need);
		if (e != hipSuccess) return e;
		*tmp_bytes = need;
	}
	e = rocprim::radix_sort_pairs(*tmp, need_sort, skey, top, iota, qlist, (size_t)n, 0, end_bit, st);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(seed_group_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, a, (const uint64_t*)keys, (const uint32_t*)top, qlist, len, skey, n);
	e = rocprim::inclusive_scan(*tmp, need_scan, place_in, place_out, (size_t)n, SeedPlaceOp(), st);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(seed_build_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, a, sid, (const uint64_t*)keys, (const uint32_t*)top, (const uint32_t*)qlist,
		(const uint32_t*)len, (const uint32_t*)skey, ctr, wrap, n);
	hipLaunchKernelGGL(seed_wrap_kernel, dim3(16), dim3(256), 0, st, a, sid, (const uint64_t*)keys, (const uint32_t*)qlist, (const uint32_t*)len, (const uint32_t*)ctr, (const uint32_t*)wrap);
	return hipGetLastError();
}

bool seed_stream_can_fuse(const SeedParams& c)
{
	for (int sid = 0; sid < c.n_shapes; ++sid)
		if (!seed_nibble_mode(c, sid) || c.shape_weight[sid] >= 10) return false;
	return true;
}

// seed_stream_fast_kernel<LEVEL2, HASHED, FUSED, BYCLASS> for either seed encoding
template<bool LEVEL2, bool FUSED, bool BYCLASS>
static void launch_stream_fast(const SeedArgs& a, int sid, dim3 grid, hipStream_t st, uint64_t lo, uint64_t hi, int64_t base, uint64_t care64)
{
	if (FUSED && a.qwin) {                               // mutual-coverage search: the instances with the length test
		if (a.params.seed_encoding == SEED_HASHED) hipLaunchKernelGGL((seed_stream_fast_kernel<LEVEL2, true, FUSED, BYCLASS, FUSED>), grid, dim3(256), 0, st, a, sid, lo, hi, base, care64);
		else hipLaunchKernelGGL((seed_stream_fast_kernel<LEVEL2, false, FUSED, BYCLASS, FUSED>), grid, dim3(256), 0, st, a, sid, lo, hi, base, care64);
		return;
	}
	if (a.params.seed_encoding == SEED_HASHED) hipLaunchKernelGGL((seed_stream_fast_kernel<LEVEL2, true, FUSED, BYCLASS>), grid, dim3(256), 0, st, a, sid, lo, hi, base, care64);
	else hipLaunchKernelGGL((seed_stream_fast_kernel<LEVEL2, false, FUSED, BYCLASS>), grid, dim3(256), 0, st, a, sid, lo, hi, base, care64);
}

hipError_t launch_seed_stream(const SeedArgs& a, int sid, hipStream_t st, bool fused)
{
	const SeedParams& c = a.params;
	if (fused && !(seed_nibble_mode(c, sid) && c.shape_weight[sid] < 10 && a.classes)) return hipErrorInvalidValue;
	if (seed_nibble_mode(c, sid)) {
		// 4-bit class map: 15 = invalid (X, '*'); every other letter code -> its reduced class
		uint64_t lo = 0, hi = 0;
		for (int l = 0; l < 32; ++l) {
			const uint64_t code = c.reduction[l] == L_MASK ? 15u : (uint64_t)c.reduction[l];
			(l < 16 ? lo : hi) |= code << ((l & 15) * 4);
		}
		const int64_t base = a.t_begin & ~(int64_t)15;
		const int64_t threads = (a.t_end - base + 15) / 16;
		uint64_t care64 = 0;
		for (int k = 0; k < c.shape_weight[sid]; ++k) care64 |= (uint64_t)15 << (4 * c.shape_pos[sid][k]);
		const bool level2 = a.level2 != 0, hashed = c.seed_encoding == SEED_HASHED;
		const dim3 grid(a.classes ? blocks_for(threads, 256 * SEED_CLASS_TILES) * 8u : blocks_for(threads, 256));
		const bool by_class = a.classes != 0;               // the fused pipeline, or long seeds against a large query block (seed_api.hip)
		if (by_class) {
			const int64_t n_groups = seed_code_groups(a.t_begin, a.t_end);
			// seed_classify_kernel computes classes as XORs of shifted bit planes: only right while seed_class is GF(2)-linear in the key
			static const bool class_is_linear = [] {
				uint64_t x = 0x9e3779b97f4a7c15ull;
				for (int t = 0; t < 256; ++t) {
					x ^= x << 13; x ^= x >> 7; x ^= x << 17;
					uint32_t sum = 0;
					for (int bit = 0; bit < 64; ++bit) if ((x >> bit) & 1u) sum ^= seed_class((uint64_t)1 << bit);
					if (sum != seed_class(x)) return false;
				}
				return seed_class(0) == 0;
			}();
			if (!class_is_linear) { std::fprintf(stderr, "seed_classify_kernel: seed_class is no longer linear over GF(2); the bit-plane classifier does not apply\n"); return hipErrorInvalidValue; }
			SeedClassCoef cc;
			cc.n = 0; cc.n_groups = 0;
			for (int k = 0; k < 16; ++k) { cc.pos[k] = 0; cc.coef[k] = 0; cc.start[k] = 0; }
			cc.start[16] = 0;
			uint16_t coef_of[16];
			for (int i = 0; i < 16; ++i) {
				coef_of[i] = 0;
				for (int b = 0; b < 4; ++b) coef_of[i] |= (uint16_t)(seed_class((uint64_t)1 << (4 * i + b)) << (3 * b));
			}
			for (int i = 0; i < 16; ++i) {                      // a group per distinct coefficient word, in order of first appearance
				if (!((care64 >> (4 * i)) & 15u)) continue;
				bool seen = false;
				for (int t = 0; t < cc.n_groups; ++t) seen = seen || cc.coef[t] == coef_of[i];
				if (seen) continue;
				cc.coef[cc.n_groups] = coef_of[i];
				cc.start[cc.n_groups] = (int8_t)cc.n;
				for (int i2 = i; i2 < 16; ++i2)
					if (((care64 >> (4 * i2)) & 15u) && coef_of[i2] == coef_of[i]) cc.pos[cc.n++] = (int8_t)i2;
				cc.start[++cc.n_groups] = (int8_t)cc.n;
			}
			hipLaunchKernelGGL(seed_classify_kernel, dim3(blocks_for((n_groups + 3) / 4, 256)), dim3(256), 0, st, a, sid, base, n_groups, cc, hashed ? 1 : 0, const_cast<uint16_t*>(a.tclass));
		}
		// the fused pipeline (short seeds: by class, no level 2); by class without the fusion (long seeds against a large query
		// block, or short seeds with DMND_SEED_FUSED=0); the plain stream
		if (fused) launch_stream_fast<false, true, true>(a, sid, grid, st, lo, hi, base, care64);
		else if (by_class && level2) launch_stream_fast<true, false, true>(a, sid, grid, st, lo, hi, base, care64);
		else if (by_class) launch_stream_fast<false, false, true>(a, sid, grid, st, lo, hi, base, care64);
		else if (level2) launch_stream_fast<true, false, false>(a, sid, grid, st, lo, hi, base, care64);
		else launch_stream_fast<false, false, false>(a, sid, grid, st, lo, hi, base, care64);
		return hipGetLastError();
	}
	hipLaunchKernelGGL(seed_stream_kernel, dim3(blocks_for(a.t_end - a.t_begin, 256)), dim3(256), 0, st, a, sid);
	return hipGetLastError();
}

static uint64_t care64_of(const SeedParams& c, int sid)
{
	uint64_t care64 = 0;
	for (int k = 0; k < c.shape_weight[sid]; ++k) care64 |= (uint64_t)15 << (4 * c.shape_pos[sid][k]);
	return care64;
}

hipError_t launch_seed_route(const SeedParams& c, int sid, const uint64_t* codes, const uint32_t* flags, int64_t t_begin, int64_t t_end, int slice_bits,
	uint8_t* route, uint8_t* route_sorted, uint32_t* list, uint32_t* counts, void** tmp, size_t* tmp_bytes, hipStream_t st)
{
	if (!seed_nibble_mode(c, sid) || c.seed_encoding != SEED_SPACED || slice_bits < 0 || slice_bits > SEED_SLICE_MAX_BITS) return hipErrorInvalidValue;
	const int64_t base = t_begin & ~(int64_t)15, n = seed_ref_windows(t_begin, t_end);
	if (n <= 0 || n >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
	hipError_t e = hipMemsetAsync(counts, 0, ((size_t)1 << SEED_SLICE_MAX_BITS) * sizeof(uint32_t), st);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(seed_route_kernel, dim3(blocks_for(n / 16, 256)), dim3(256), 0, st, codes, flags, base, n / 16, t_begin, t_end, (int)c.shape_len[sid], c.shape_mask[sid], care64_of(c, sid),
		slice_bits, route, counts);
	// one stable radix pass over the routing bytes' low b + 1 bits lists the windows slice by slice, ascending in each; the windows that
	// are no seeds (all ones) come last
	rocprim::counting_iterator<uint32_t> iota(0);
	size_t need = 0;
	e = rocprim::radix_sort_pairs(nullptr, need, route, route_sorted, iota, list, (size_t)n, 0, (unsigned)slice_bits + 1, st);
	if (e != hipSuccess) return e;
	if (need > *tmp_bytes) {
		if (*tmp) (void)hipFree(*tmp);
		*tmp = nullptr; *tmp_bytes = 0;
		e = hipMalloc(tmp, need);
		if (e != hipSuccess) return e;
		*tmp_bytes = need;
	}
	e = rocprim::radix_sort_pairs(*tmp, need, route, route_sorted, iota, list, (size_t)n, 0, (unsigned)slice_bits + 1, st);
	if (e != hipSuccess) return e;
	return hipGetLastError();
}

hipError_t launch_seed_stream_slices(const SeedArgs& a, int sid, const uint64_t* codes, const uint32_t* list, const uint32_t* hashes, const uint32_t* counts, int slice_bits, hipStream_t st)
{
	const SeedParams& c = a.params;
	if (a.classes || a.fused || !seed_nibble_mode(c, sid) || c.seed_encoding != SEED_SPACED || slice_bits < 0 || slice_bits > SEED_SLICE_MAX_BITS) return hipErrorInvalidValue;
	if (a.bitmap1_words % (1u << slice_bits) != 0 || (a.bitmap1_words >> slice_bits) > (uint32_t)SEED_SLICE_MAX_WORDS || slice_bits > a.slot_bits) return hipErrorInvalidValue;
	// a workgroup per CU (the slice takes most of a CU's LDS), a whole number of shares per slice
	int dev = 0, n_cus = 0;
	hipError_t e = hipGetDevice(&dev);
	if (e != hipSuccess) return e;
	e = hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev);
	if (e != hipSuccess) return e;
	n_cus = std::max(n_cus, 1);
	const unsigned slices = 1u << slice_bits, shares = std::max(1u, (unsigned)n_cus / slices);
	hipLaunchKernelGGL(seed_stream_slices_kernel, dim3(slices * shares), dim3(SEED_SLICE_THREADS), 0, st, a, a.t_begin & ~(int64_t)15, care64_of(c, sid), codes, list, hashes,
		counts, slice_bits, a.bitmap1_words >> slice_bits);
	return hipGetLastError();
}

// hash a of the key of every list entry's window, in list order (seed_ref_hash_entry)
__global__ __launch_bounds__(256) void seed_ref_hash_kernel(const uint64_t* __restrict__ codes, const uint32_t* __restrict__ list, int64_t n, uint64_t care64, uint32_t* __restrict__ hashes)
{
	const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (k < n) hashes[k] = seed_ref_hash_entry(codes, list[k], care64);
}

hipError_t launch_seed_ref_hashes(const SeedParams& c, int sid, const uint64_t* codes, const uint32_t* list, int64_t t_begin, int64_t t_end, uint32_t* hashes, hipStream_t st)
{
	if (!seed_nibble_mode(c, sid) || c.seed_encoding != SEED_SPACED) return hipErrorInvalidValue;
	const int64_t n = seed_ref_windows(t_begin, t_end);
	if (n <= 0 || n >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
	hipLaunchKernelGGL(seed_ref_hash_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, codes, list, n, care64_of(c, sid), hashes);
	return hipGetLastError();
}

hipError_t launch_seed_mask(const SeedArgs& a, int sid, hipStream_t st, int64_t n_matched)
{
	if (!a.fused && n_matched >= 0 && n_matched * 4 < (int64_t)a.slot_mask) {
		if (n_matched == 0) return hipSuccess;
		hipLaunchKernelGGL(seed_mask_joined_kernel<false>, dim3(blocks_for(n_matched, 256)), dim3(256), 0, st, a, sid, n_matched, SeedChain{});
		return hipGetLastError();
	}
	hipLaunchKernelGGL(seed_mask_kernel, dim3(blocks_for((int64_t)a.slot_mask + 1, 256)), dim3(256), 0, st, a, sid);
	return hipGetLastError();
}

hipError_t launch_seed_lin_first(const SeedArgs& a, int64_t n_matched, hipStream_t st)
{
	if (n_matched == 0 || !a.lin_first) return hipSuccess;
	hipLaunchKernelGGL((seed_lin_first_kernel<false, 0>), dim3(blocks_for(n_matched, 256)), dim3(256), 0, st, a, 0, n_matched, SeedChain{});
	hipLaunchKernelGGL((seed_lin_first_kernel<false, 1>), dim3(blocks_for(n_matched, 256)), dim3(256), 0, st, a, 0, n_matched, SeedChain{});
	return hipGetLastError();
}

hipError_t launch_seed_pairs(const SeedArgs& a, int sid, int64_t n_matched, hipStream_t st)
{
	if (n_matched == 0) return hipSuccess;
	if (a.lin_first) {                                   // linearised search (never with a length ratio: dmnd_seed_search refuses the two together)
		const hipError_t e = launch_seed_lin_first(a, n_matched, st);
		if (e != hipSuccess) return e;
		hipLaunchKernelGGL((seed_pair_kernel<false, false, true>), dim3(blocks_for(n_matched, 128)), dim3(128), 0, st, a, sid, n_matched, SeedChain{});
	}
	else if (a.qwin) hipLaunchKernelGGL((seed_pair_kernel<false, true>), dim3(blocks_for(n_matched, 128)), dim3(128), 0, st, a, sid, n_matched, SeedChain{});
	else hipLaunchKernelGGL((seed_pair_kernel<false, false>), dim3(blocks_for(n_matched, 128)), dim3(128), 0, st, a, sid, n_matched, SeedChain{});
	return hipGetLastError();
}

hipError_t launch_seed_pairs_tiled(const SeedArgs& a, int sid, int64_t n_matched, hipStream_t st)
{
	if (n_matched == 0) return hipSuccess;
	if (a.lin_first) {
		const hipError_t e = launch_seed_lin_first(a, n_matched, st);
		if (e != hipSuccess) return e;
		hipLaunchKernelGGL((seed_pair_tiled_kernel<false, true>), dim3(blocks_for(n_matched, 256)), dim3(256), 0, st, a, sid, n_matched);
	}
	else if (a.qwin) hipLaunchKernelGGL(seed_pair_tiled_kernel<true>, dim3(blocks_for(n_matched, 256)), dim3(256), 0, st, a, sid, n_matched);
	else hipLaunchKernelGGL(seed_pair_tiled_kernel<false>, dim3(blocks_for(n_matched, 256)), dim3(256), 0, st, a, sid, n_matched);
	return hipGetLastError();
}

hipError_t launch_seed_count_pairs(const SeedArgs& a, int64_t n_matched, unsigned long long* out, hipStream_t st)
{
	if (n_matched == 0) return hipSuccess;
	hipLaunchKernelGGL(seed_count_pairs_kernel, dim3(blocks_for(n_matched, 256)), dim3(256), 0, st, a, n_matched, out);
	return hipGetLastError();
}

// the left-most kernel with the 4-bit class maps of the letters; reductions with more than 15 classes keep the byte-wise windows
static void launch_leftmost(const SeedArgs& a, int sid, dim3 grid, hipStream_t st)
{
	uint64_t lo, hi;
	seed_class_maps(a.params, lo, hi);
	hipLaunchKernelGGL(seed_leftmost_kernel, grid, dim3(256), 0, st, a, sid, lo, hi, a.params.reduction_size <= 15 ? 1 : 0);
}

hipError_t launch_seed_post(const SeedArgs& a, int sid, int64_t n_survivors, hipStream_t st, bool clear_scored)
{
	if (n_survivors == 0) return hipSuccess;
	if (clear_scored) {
		const hipError_t e = hipMemsetAsync(a.scored_count, 0, sizeof(unsigned long long), st);
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(seed_score_kernel<false>, dim3(blocks_for(n_survivors, POST_THREADS)), dim3(POST_THREADS), 0, st, a, sid, n_survivors, SeedChain{});
	launch_leftmost(a, sid, dim3(std::min<unsigned>(blocks_for(n_survivors, 256), 256 * 16)), st);
	return hipGetLastError();
}

// stable sort of the joined positions by slot: (slot_in, loc_in) -> (slot_out, loc_out)
hipError_t sort_matched_by_slot(const uint32_t* slot_in, uint32_t* slot_out, const int64_t* loc_in, int64_t* loc_out, int64_t n, int slot_bits,
	void** tmp, size_t* tmp_bytes, hipStream_t st)
{
	if (n <= 0) return hipSuccess;
	size_t need = 0;
	hipError_t e = rocprim::radix_sort_pairs(nullptr, need, slot_in, slot_out, loc_in, loc_out, (size_t)n, 0, slot_bits, st);
	if (e != hipSuccess) return e;
	if (need > *tmp_bytes) {
		if (*tmp) (void)hipFree(*tmp);
		*tmp = nullptr; *tmp_bytes = 0;
		e = hipMalloc(tmp, need);
		if (e != hipSuccess) return e;
		*tmp_bytes = need;
	}
	return rocprim::radix_sort_pairs(*tmp, need, slot_in, slot_out, loc_in, loc_out, (size_t)n, 0, slot_bits, st);
}

hipError_t launch_seed_collect(const SeedArgs& a, int64_t n_matched, hipStream_t st)
{
	if (n_matched == 0) return hipSuccess;
	const char* folded_env = getenv("DMND_SEED_COLLECT_FOLDED_FROM");                  // (tests: 1 = always)
	const int64_t folded_from = folded_env ? (int64_t)atoll(folded_env) : (int64_t)1 << 22;
	if (n_matched >= folded_from) {
		const uint64_t words = (a.slot_mask + 1) / 32;
		uint32_t* fold = a.need_bits + words;              // (seed_api.hip sizes the map's buffer for it)
		const uint32_t fold_words = SEED_NEED_FOLD_WORDS;
		hipLaunchKernelGGL(seed_need_fold_kernel, dim3(fold_words / 256), dim3(256), 0, st, (const uint32_t*)a.need_bits, words, fold, fold_words);
		const unsigned tiles = blocks_for(n_matched, 256 * 16);
		const unsigned per_cu = std::max(1u, std::min(4u, (150u * 1024u) / (fold_words * 4u + 64u)));
		hipLaunchKernelGGL(seed_collect_folded_kernel, dim3(std::min(tiles, 256u * per_cu)), dim3(256), fold_words * sizeof(uint32_t), st, a, n_matched, (const uint32_t*)fold, fold_words);
		return hipGetLastError();
	}
	hipLaunchKernelGGL(seed_collect_kernel, dim3(blocks_for(n_matched, 256 * 16)), dim3(256), 0, st, a, n_matched);
	return hipGetLastError();
}

hipError_t sort_keys_u64(const uint64_t* in, uint64_t* out, int64_t n, void** tmp, size_t* tmp_bytes, hipStream_t st)
{
	size_t need = 0;
	hipError_t e = rocprim::radix_sort_keys(nullptr, need, in, out, (size_t)n, 0, 64, st);
	if (e != hipSuccess) return e;
	if (need > *tmp_bytes) {
		if (*tmp) (void)hipFree(*tmp);
		*tmp = nullptr; *tmp_bytes = 0;
		e = hipMalloc(tmp, need);
		if (e != hipSuccess) return e;
		*tmp_bytes = need;
	}
	return rocprim::radix_sort_keys(*tmp, need, in, out, (size_t)n, 0, 64, st);
}

namespace {

// pass 0: key = score, identity permutation; pass 1: key = subject << 24 | seed_offset; pass 2: key = query.
// pass 3 = passes 1 and 2 in one key, query | subject | seed_offset in subject_bits and off_bits wide fields (when the three fit 64 bits)
__global__ void hit_keys_kernel(const dmnd_seed_hit* hits, const uint32_t* perm, int64_t n, int pass, uint64_t* keys, uint32_t* idx_out, int subject_bits, int off_bits)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t src = perm ? perm[i] : (uint32_t)i;
	const dmnd_seed_hit h = hits[src];
	keys[i] = pass == 0 ? (uint64_t)(uint32_t)h.score : pass == 1 ? ((uint64_t)h.subject << 24) | ((uint64_t)h.seed_offset & 0xffffffu) : pass == 2 ? (uint64_t)h.query
		: ((((uint64_t)h.query << subject_bits) | (uint64_t)h.subject) << off_bits) | ((uint64_t)h.seed_offset & 0xffffffu);
	if (idx_out) idx_out[i] = src;
}

__global__ void hit_gather_kernel(const dmnd_seed_hit* hits, const uint32_t* perm, int64_t n, dmnd_seed_hit* out)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) out[i] = hits[perm[i]];
}

hipError_t sort_pairs(const uint64_t* kin, uint64_t* kout, const uint32_t* vin, uint32_t* vout, int64_t n, int bits, void** tmp, size_t* tmp_bytes, hipStream_t st)
{
	size_t need = 0;
	hipError_t e = rocprim::radix_sort_pairs(nullptr, need, kin, kout, vin, vout, (size_t)n, 0, bits, st);
	if (e != hipSuccess) return e;
	if (need > *tmp_bytes) {
		if (*tmp) (void)hipFree(*tmp);
		*tmp = nullptr; *tmp_bytes = 0;
		e = hipMalloc(tmp, need);
		if (e != hipSuccess) return e;
		*tmp_bytes = need;
	}
	return rocprim::radix_sort_pairs(*tmp, need, kin, kout, vin, vout, (size_t)n, 0, bits, st);
}

}  // namespace

hipError_t sort_seed_hits(const dmnd_seed_hit* hits, dmnd_seed_hit* out, int64_t n, uint64_t* keys[2], uint32_t* idx[2],
	void** tmp, size_t* tmp_bytes, hipStream_t st, int query_bits, int subject_bits, int off_bits, bool equal_scores)
{
	if (n <= 0) return hipSuccess;
	const dim3 grid(blocks_for(n, 256)), block(256);
	hipError_t e;
	const bool one_key = off_bits >= 1 && off_bits <= 24 && query_bits + subject_bits + off_bits <= 64;
	if (equal_scores && one_key) {
		// round 5: without the ungapped filter every hit carries the same score (0xFFFF), the stable pass over the scores orders
		// nothing: ONE sort of the (query, subject, seed_offset) key from the identity permutation (C2: a key kernel and a sort less)
		hipLaunchKernelGGL(hit_keys_kernel, grid, block, 0, st, hits, (const uint32_t*)nullptr, n, 3, keys[0], idx[1], subject_bits, off_bits);
		if ((e = sort_pairs(keys[0], keys[1], idx[1], idx[0], n, query_bits + subject_bits + off_bits, tmp, tmp_bytes, st)) != hipSuccess) return e;
		hipLaunchKernelGGL(hit_gather_kernel, grid, block, 0, st, hits, (const uint32_t*)idx[0], n, out);
		return hipGetLastError();
	}
	// least significant criterion first; every pass is stable
	hipLaunchKernelGGL(hit_keys_kernel, grid, block, 0, st, hits, (const uint32_t*)nullptr, n, 0, keys[0], idx[0], 0, 0);
	if ((e = sort_pairs(keys[0], keys[1], idx[0], idx[1], n, 32, tmp, tmp_bytes, st)) != hipSuccess) return e;
	if (one_key) {
		// (query, subject, seed_offset) as ONE key: a sort less (80 of 250 us for the 2e4 hits of a C2 step)
		hipLaunchKernelGGL(hit_keys_kernel, grid, block, 0, st, hits, (const uint32_t*)idx[1], n, 3, keys[0], (uint32_t*)nullptr, subject_bits, off_bits);
		if ((e = sort_pairs(keys[0], keys[1], idx[1], idx[0], n, query_bits + subject_bits + off_bits, tmp, tmp_bytes, st)) != hipSuccess) return e;
		hipLaunchKernelGGL(hit_gather_kernel, grid, block, 0, st, hits, (const uint32_t*)idx[0], n, out);
		return hipGetLastError();
	}
	hipLaunchKernelGGL(hit_keys_kernel, grid, block, 0, st, hits, (const uint32_t*)idx[1], n, 1, keys[0], (uint32_t*)nullptr, 0, 0);
	if ((e = sort_pairs(keys[0], keys[1], idx[1], idx[0], n, 64, tmp, tmp_bytes, st)) != hipSuccess) return e;
	hipLaunchKernelGGL(hit_keys_kernel, grid, block, 0, st, hits, (const uint32_t*)idx[0], n, 2, keys[0], (uint32_t*)nullptr, 0, 0);
	if ((e = sort_pairs(keys[0], keys[1], idx[0], idx[1], n, 32, tmp, tmp_bytes, st)) != hipSuccess) return e;
	hipLaunchKernelGGL(hit_gather_kernel, grid, block, 0, st, hits, (const uint32_t*)idx[1], n, out);
	return hipGetLastError();
}

// ---- chain mode (seed_chain.h) -------------------------------------------------------------------------------------------
namespace {

// the gate of shape s's pair filter: a shape that reached the tiled-filter threshold is the host's
__device__ void chain_gate(const SeedChain& ch, int s)
{
	const unsigned long long n = ch.ctr[s] - (s ? ch.ctr[s - 1] : 0ull);
	if ((long long)n >= ch.tiled_from) ch.ctr[chain_ctr_status(ch.S)] |= CHAIN_TILED;
}

// One thread, between two kernels of the chain: what the host decided there when it read the counters.
// Behind the stream kernel of shape sid: ctr[sid] is the end of the shape's range of the shared lists and the start of the next one's.
__global__ void seed_chain_streamed_kernel(SeedChain ch, int sid)
{
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	const unsigned long long end = ch.ctr[sid];
	if ((long long)end > ch.matched_cap) ch.ctr[chain_ctr_status(ch.S)] |= CHAIN_MATCHED_OVER;
	if (sid + 1 < ch.S) { ch.ctr[sid + 1] = end; return; }      // (the stream kernels append with atomics on ctr[sid])
	if (!ch.ctr[chain_ctr_status(ch.S)]) chain_gate(ch, 0);
}

// Behind the left-most rule of shape sid
__global__ void seed_chain_shape_done_kernel(SeedChain ch, int sid)
{
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	unsigned long long& status = ch.ctr[chain_ctr_status(ch.S)];
	// the left-most kernel has consumed the scored list: behind a flag the scoring of the following shapes does nothing, and their
	// left-most kernels must not find this shape's list again
	ch.ctr[ch.S + 4] = 0;
	if (status) return;
	const unsigned long long ns = ch.ctr[ch.S + 3];
	ch.ctr[chain_ctr_survivors_of(ch.S) + sid] = ns;
	if ((long long)ns > ch.survivor_cap) { status |= CHAIN_SURVIVORS_OVER; return; }
	if ((long long)ch.ctr[ch.S] > ch.hit_cap) { status |= CHAIN_HITS_OVER; return; }
	if (ch.ctr[ch.S + 1] != 0) { status |= CHAIN_DEFERRED; return; }      // (deferred pairs over their capacity: the host sees the count)
	ch.ctr[chain_ctr_done(ch.S)] = (unsigned long long)(sid + 1);
	if (sid + 1 < ch.S) {
		ch.ctr[ch.S + 3] = 0; ch.ctr[ch.S + 4] = 0;        // the next shape's survivors and scored survivors
		chain_gate(ch, sid + 1);
	}
}

// hit_keys_kernel over a fixed capacity: entries from the hit count (device memory) on carry a key of all ones, which sorts last
// -- behind every real key even where the fields of one are all ones, since the radix sorts are stable and the padding starts behind the hits.
// (pass 0: scores; pass 3: query | subject | seed_offset)
__global__ void hit_keys_chain_kernel(const dmnd_seed_hit* hits, const uint32_t* perm, int64_t cap, int pass, uint64_t* keys, uint32_t* idx_out, int subject_bits, int off_bits, SeedChain ch)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= cap) return;
	int64_t n = (int64_t)ch.ctr[ch.S];
	if (n > cap || (ch.ctr[chain_ctr_status(ch.S)] & ~(unsigned long long)CHAIN_SORT_OVER)) n = 0;      // nothing to sort here: the host continues
	const uint32_t src = perm ? perm[i] : (uint32_t)i;
	uint64_t key = ~(uint64_t)0;
	if ((int64_t)src < n) {
		const dmnd_seed_hit h = hits[src];
		key = pass == 0 ? (uint64_t)(uint32_t)h.score : ((((uint64_t)h.query << subject_bits) | (uint64_t)h.subject) << off_bits) | ((uint64_t)h.seed_offset & 0xffffffu);
	}
	keys[i] = key;
	if (idx_out) idx_out[i] = src;
}

// the sorted hits, and the readback: the counter block, then the leading sorted hits
__global__ void hit_gather_chain_kernel(const dmnd_seed_hit* hits, const uint32_t* perm, int64_t cap, dmnd_seed_hit* out, SeedChain ch, unsigned long long* ret, int ret_words, dmnd_seed_hit* ret_hits, int64_t n_ret_hits)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const unsigned long long status = ch.ctr[chain_ctr_status(ch.S)];
	int64_t n = (int64_t)ch.ctr[ch.S];
	const bool over = n > cap;
	if (i < ret_words) ret[i] = i == chain_ctr_status(ch.S) && !status && (over || !perm) ? (unsigned long long)CHAIN_SORT_OVER : ch.ctr[i];
	if (over || status || !perm) return;
	if (i < n) {
		const dmnd_seed_hit h = hits[perm[i]];
		out[i] = h;
		if (i < n_ret_hits) ret_hits[i] = h;
	}
}

}  // namespace

hipError_t launch_seed_chain_streamed(const SeedChain& ch, int sid, hipStream_t st)
{
	hipLaunchKernelGGL(seed_chain_streamed_kernel, dim3(1), dim3(64), 0, st, ch, sid);
	return hipGetLastError();
}

// Grids of the chain's kernels: the host does not know the list sizes, every workgroup reads them and leaves, or strides over the
// list -- eight workgroups per CU cover the 10^4 - 10^5 entries of a long-seed block pair in one pass
enum { CHAIN_GRID = 256 * 8 };

hipError_t launch_seed_chain_mask(const SeedArgs& a, const SeedChain& ch, int sid, hipStream_t st)
{
	hipLaunchKernelGGL(seed_mask_joined_kernel<true>, dim3(CHAIN_GRID / 2), dim3(256), 0, st, a, sid, (int64_t)0, ch);
	return hipGetLastError();
}

hipError_t launch_seed_chain_shape(const SeedArgs& a, const SeedChain& ch, int sid, hipStream_t st)
{
	if (a.lin_first) {                                   // the reduction over the shape's range of the counter block, then the filter that reads it
		hipLaunchKernelGGL((seed_lin_first_kernel<true, 0>), dim3(CHAIN_GRID / 2), dim3(256), 0, st, a, sid, (int64_t)0, ch);
		hipLaunchKernelGGL((seed_lin_first_kernel<true, 1>), dim3(CHAIN_GRID / 2), dim3(256), 0, st, a, sid, (int64_t)0, ch);
		hipLaunchKernelGGL((seed_pair_kernel<true, false, true>), dim3(CHAIN_GRID), dim3(128), 0, st, a, sid, (int64_t)0, ch);
	}
	else if (a.qwin) hipLaunchKernelGGL((seed_pair_kernel<true, true>), dim3(CHAIN_GRID), dim3(128), 0, st, a, sid, (int64_t)0, ch);
	else hipLaunchKernelGGL((seed_pair_kernel<true, false>), dim3(CHAIN_GRID), dim3(128), 0, st, a, sid, (int64_t)0, ch);
	hipLaunchKernelGGL(seed_score_kernel<true>, dim3(CHAIN_GRID / 2), dim3(POST_THREADS), 0, st, a, sid, (int64_t)0, ch);
	// (a voided shape leaves the scored count zero: the left-most kernel reads it and leaves)
	launch_leftmost(a, sid, dim3(CHAIN_GRID / 2), st);
	hipLaunchKernelGGL(seed_chain_shape_done_kernel, dim3(1), dim3(64), 0, st, ch, sid);
	return hipGetLastError();
}

hipError_t launch_seed_chain_sort(const SeedChain& ch, bool sorted, const dmnd_seed_hit* hits, dmnd_seed_hit* out, int64_t sort_cap, uint64_t* keys[2], uint32_t* idx[2],
	void** tmp, size_t* tmp_bytes, hipStream_t st, int query_bits, int subject_bits, int off_bits, bool equal_scores, char* ret, int64_t ret_hits)
{
	const dim3 grid(blocks_for(std::max<int64_t>(sort_cap, chain_ctr_words(ch.S)), 256)), block(256);
	unsigned long long* ret_ctr = reinterpret_cast<unsigned long long*>(ret);
	dmnd_seed_hit* ret_h = reinterpret_cast<dmnd_seed_hit*>(ret + chain_ret_header_bytes(ch.S));
	if (!sorted || !sort_seed_hits_one_key(query_bits, subject_bits, off_bits)) {
		hipLaunchKernelGGL(hit_gather_chain_kernel, dim3(1), block, 0, st, hits, (const uint32_t*)nullptr, sort_cap, out, ch, ret_ctr, chain_ctr_words(ch.S), ret_h, ret_hits);
		return hipGetLastError();
	}
	hipError_t e;
	const int bits = query_bits + subject_bits + off_bits;
	const uint32_t* perm;
	if (equal_scores) {
		hipLaunchKernelGGL(hit_keys_chain_kernel, grid, block, 0, st, hits, (const uint32_t*)nullptr, sort_cap, 3, keys[0], idx[1], subject_bits, off_bits, ch);
		if ((e = sort_pairs(keys[0], keys[1], idx[1], idx[0], sort_cap, bits, tmp, tmp_bytes, st)) != hipSuccess) return e;
		perm = idx[0];
	}
	else {
		// least significant criterion first; every pass is stable
		hipLaunchKernelGGL(hit_keys_chain_kernel, grid, block, 0, st, hits, (const uint32_t*)nullptr, sort_cap, 0, keys[0], idx[0], 0, 0, ch);
		if ((e = sort_pairs(keys[0], keys[1], idx[0], idx[1], sort_cap, 32, tmp, tmp_bytes, st)) != hipSuccess) return e;
		hipLaunchKernelGGL(hit_keys_chain_kernel, grid, block, 0, st, hits, (const uint32_t*)idx[1], sort_cap, 3, keys[0], (uint32_t*)nullptr, subject_bits, off_bits, ch);
		if ((e = sort_pairs(keys[0], keys[1], idx[1], idx[0], sort_cap, bits, tmp, tmp_bytes, st)) != hipSuccess) return e;
		perm = idx[0];
	}
	hipLaunchKernelGGL(hit_gather_chain_kernel, grid, block, 0, st, hits, perm, sort_cap, out, ch, ret_ctr, chain_ctr_words(ch.S), ret_h, ret_hits);
	return hipGetLastError();
}

hipError_t launch_seed_deferred(const SeedArgs& a, int sid, int64_t n_deferred, hipStream_t st)
{
	if (n_deferred == 0) return hipSuccess;
	if (a.qwin) hipLaunchKernelGGL(seed_deferred_kernel<true>, dim3(blocks_for(n_deferred * 64, 256)), dim3(256), 0, st, a, sid, n_deferred);
	else hipLaunchKernelGGL(seed_deferred_kernel<false>, dim3(blocks_for(n_deferred * 64, 256)), dim3(256), 0, st, a, sid, n_deferred);
	return hipGetLastError();
}

}  // namespace dmnd

// dmnd_init: the first launch of a kernel of this translation unit loads its code object onto the device
namespace { __global__ void touch_seed_kernel() {} }
extern "C" hipError_t dmnd_touch_seed(hipStream_t st) { hipLaunchKernelGGL(touch_seed_kernel, dim3(1), dim3(64), 0, st); return hipGetLastError(); }
