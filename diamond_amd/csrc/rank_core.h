// rank_core.h -- the arithmetic of the global ranking step (--global-ranking; reference: align/global_ranking/table.cpp:88-133,
// get_query_hits_reextend + target_score), HIP-free: one statement of it for the kernels (rank_kernels.hip), the host entry
// (extend_host.hip, dmnd_rank_targets' x-drop value) and the CPU tests (tests/emu/rank_emu.cpp).
//
// The walk rule, as dmnd_rank_targets states it. The seed hits of a (query, target) group -- for translated queries the (read, target)
// pair with all its frames -- are ordered by (diagonal = i - j, then j), j relative to the target. `d` is the segment of the hit
// computed LAST. A hit is skipped when d.diag() == i - j && d.j_end() >= j; the test compares the diagonal only, not the frame.
// Otherwise the hit's own x-drop segment becomes d, and d.score > score (strict) replaces the score and the context. No composition
// bias; the x-drop value is rank_xdrop. The segment of a hit is what dmnd_xdrop_ungapped makes of the kernel's XdropSeg:
// (i - left, j - left, left + right, score).
//
// Consequences the device form rests on:
//   - hits of another diagonal never match d's diagonal, so every run of equal (group, diagonal) is walked on its own, its first hit
//     is always computed, and the skipped hits behind a computed one are the stretch with j <= d.j_end() (j ascends inside a run): the
//     next computed hit is found by binary search (rank_walk_run);
//   - the group's result is the highest score and, of the computed hits that reach it, the first in the sorted order: a maximum over
//     the packed (score, reversed sorted position) of the runs, which no order of reduction changes (rank_pack_best).
//
// The tie-break (device rule). std::sort on the host is unstable: hits of one group with equal (diagonal, j) -- which can only be hits
// of different frames -- come in an order it does not determine. On the device they come frame ascending, then seed offset: what a
// stable sort of the planner's translated order (read, target, frame, location, seed offset) gives. Wherever the host is determined
// the two agree.
#pragma once
#include <stdint.h>
#include <math.h>
#include "xdrop_core.h"

namespace dmnd {

// config.raw_ungapped_xdrop: 12.3 bits in raw score units of the context's matrix (make_cfg)
inline int rank_xdrop(double K, double lambda) { return (int)ceil((12.3 * 0.69314718055994530941723212145818 + log(K)) / lambda); }

// the DiagonalSegment of a hit (i, j) from the kernel's record, reduced to what the walk reads
struct RankSeg { int32_t diag, j_end, score; };
DMND_XD RankSeg rank_seg(int32_t i, int32_t j, const XdropSeg& x)
{
	const int32_t si = i - x.left, sj = j - x.left, len = x.left + x.right;
	return RankSeg{ si - sj, sj + len, x.score };
}

// the skip test, as dmnd_rank_targets' loop applies it hit by hit; rank_walk_run below is the same test over a run that is sorted by j
DMND_XD bool rank_skips(int32_t d_diag, int32_t d_j_end, int32_t diag, int32_t j) { return d_diag == diag && d_j_end >= j; }

// The sort key (group, diagonal): the group above the diagonal biased by 2^31, so that unsigned order is (group, diagonal) order for
// every diagonal an int32 holds -- a target longer than 65 535 letters loses nothing.
DMND_XD uint64_t rank_key(uint32_t group, int32_t diag) { return ((uint64_t)group << 32) | (uint64_t)((uint32_t)diag ^ 0x80000000u); }
DMND_XD uint32_t rank_key_group(uint64_t key) { return (uint32_t)(key >> 32); }
DMND_XD int32_t rank_key_diag(uint64_t key) { return (int32_t)((uint32_t)key ^ 0x80000000u); }

// (score, first sorted position that reached it): larger = better score, then earlier position. Scores are never negative (the
// x-drop walk starts at 0), positions lie below 2^32 - 1, so every packed value of a hit is above 0 = "no hit yet".
DMND_XD uint64_t rank_pack_best(int32_t score, uint32_t pos) { return ((uint64_t)(uint32_t)score << 32) | (uint64_t)(0xffffffffu - pos); }
DMND_XD int32_t rank_best_score(uint64_t packed) { return (int32_t)(uint32_t)(packed >> 32); }
DMND_XD uint32_t rank_best_pos(uint64_t packed) { return 0xffffffffu - (uint32_t)packed; }

// One run of equal (group, diagonal), positions [b, e) of the sorted lists (j ascending): the skip rule over the run. After a computed
// hit the walk jumps to the first hit whose j lies beyond the segment's end. best / best_pos: the run's highest score and the first
// position that reached it; counted: hits that were not skipped.
DMND_XD void rank_walk_run(const int32_t* sj, const int32_t* sj_end, const int32_t* sscore, uint32_t b, uint32_t e, int32_t& best, uint32_t& best_pos, uint32_t& counted)
{
	best = -1; best_pos = b; counted = 0;
	for (uint32_t p = b; p < e;) {
		++counted;
		if (sscore[p] > best) { best = sscore[p]; best_pos = p; }
		const int32_t reach = sj_end[p];
		uint32_t lo = p + 1, hi = e;
		while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (sj[mid] <= reach) lo = mid + 1; else hi = mid; }
		p = lo;
	}
}

// the record's score: the int score as the host casts it
DMND_XD uint16_t rank_record_score(int32_t score) { return (uint16_t)score; }

// The cut's sort key: the query (its number among the call's queries) above 65535 - score. A stable sort of the records, which
// arrive in (query, target) order, leaves them in (query, score descending, target ascending) order.
DMND_XD uint64_t rank_cut_key(uint32_t query, uint16_t score) { return ((uint64_t)query << 16) | (uint64_t)(65535u - (uint32_t)score); }
DMND_XD uint32_t rank_cut_query(uint64_t key) { return (uint32_t)(key >> 16); }

}  // namespace dmnd
