// length_ratio_core.h -- the arithmetic of the mutual-coverage search (--min-len-ratio; equal --query-cover / --subject-cover of
// 50 and more), HIP-free: one statement of it for the CLI (cli.cpp), the seed stage's window kernel and pair filters
// (seed_kernels.hip), the checks of dmnd_seed_search (seed_api.hip) and the CPU tests (tests/emu/length_ratio_emu.cpp).
//   the ratio of a command line            src/run/config.cpp:156-165
//   Block::length_sorted                   src/data/block/block.cpp:229-255
//   the pair test of stage 1               src/search/hamming/kernel_mutual_cov.h (all_vs_all_mutual_cov)
// The reference walks two length-sorted seed lists with two pointers; over blocks sorted by (length, index) descending that
// walk admits exactly the pairs for which length_ratio_passes holds, so here the test is that predicate and nothing else.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define DMND_LR_HD __host__ __device__
#else
#define DMND_LR_HD
#endif

namespace dmnd {

// both quotients in double, as the reference forms them; symmetric in its two lengths
DMND_LR_HD inline bool length_ratio_passes(int64_t qlen, int64_t tlen, double mlr)
{
	return (double)qlen / (double)tlen >= mlr && (double)tlen / (double)qlen >= mlr;
}

// min_length_ratio of a protein search: equal covers of 50 and more stand for a ratio of their own unless one was given
inline double mutual_cover_ratio(double query_cover, double subject_cover, double min_len_ratio_given)
{
	if (query_cover >= 50 && query_cover == subject_cover && min_len_ratio_given == 0.0)
		return std::max(query_cover / 100 - 0.05, 0.0);
	return min_len_ratio_given;
}

// order[k] = index (in the block as loaded) of the k-th sequence of the length-sorted block: (length, index) descending.
// limits: n + 1 block offsets, each sequence followed by its delimiter.
inline void length_sort_order(const int64_t* limits, int64_t n, int64_t* order)
{
	std::vector<std::pair<int64_t, int64_t>> v((size_t)n);
	for (int64_t i = 0; i < n; ++i) v[(size_t)i] = std::make_pair(limits[i + 1] - limits[i] - 1, i);
	std::sort(v.begin(), v.end(), std::greater<std::pair<int64_t, int64_t>>());
	for (int64_t i = 0; i < n; ++i) order[i] = v[(size_t)i].second;
}

// lengths[i * stride] non-increasing in i (stride 1: plain lengths; the kernel walks block limits through length_at below).
// The indices whose length passes against `len` form one range [first, end): towards the front the lengths grow until
// len / length falls below the ratio, towards the back they shrink until length / len does. Both ends are found by binary
// search over predicates that are length_ratio_passes itself joined with an integer comparison (which side of `len` a length
// lies on), so that no rounding case can put an index inside the range that the pair test would refuse, or the reverse.
// 0 < mlr <= 1; len <= 0 gives the empty range.
template<typename LengthAt>
DMND_LR_HD inline void length_window_of(LengthAt length_at, int64_t n, int64_t len, double mlr, int64_t* first, int64_t* end)
{
	if (len <= 0) { *first = 0; *end = 0; return; }
	int64_t lo = 0, hi = n;                                // first index whose length is <= len or passes
	while (lo < hi) {
		const int64_t mid = (lo + hi) >> 1, l = length_at(mid);
		if (l <= len || length_ratio_passes(len, l, mlr)) hi = mid; else lo = mid + 1;
	}
	*first = lo;
	hi = n;                                                // first index behind it whose length is < len and fails
	while (lo < hi) {
		const int64_t mid = (lo + hi) >> 1, l = length_at(mid);
		if (l < len && !length_ratio_passes(len, l, mlr)) hi = mid; else lo = mid + 1;
	}
	*end = lo;
}

struct LengthsPlain { const int64_t* p; DMND_LR_HD int64_t operator()(int64_t i) const { return p[i]; } };
// lengths of the sequences of a block from its limits (every sequence is followed by one delimiter)
struct LengthsOfLimits { const int64_t* limits; DMND_LR_HD int64_t operator()(int64_t i) const { return limits[i + 1] - limits[i] - 1; } };

DMND_LR_HD inline void length_window(const int64_t* lengths_desc, int64_t n, int64_t len, double mlr, int64_t* first, int64_t* end)
{
	length_window_of(LengthsPlain{ lengths_desc }, n, len, mlr, first, end);
}

// a block's sequences are in non-increasing length order (what a ratio > 0 requires of both blocks)
inline bool lengths_non_increasing(const int64_t* limits, int64_t n)
{
	for (int64_t i = 1; i < n; ++i)
		if (limits[i + 1] - limits[i] > limits[i] - limits[i - 1]) return false;
	return true;
}

}  // namespace dmnd
