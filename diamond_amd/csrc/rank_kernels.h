// rank_kernels.h -- launch interface of the device form of the global ranking step (--global-ranking; what dmnd_rank_targets does per
// block pair on host threads: load_query, a sort per (query, target) group and a scalar x-drop walk per hit). Everything stays in HBM
// between the seed stage's sorted hit list and the records; the arithmetic is rank_core.h, shared with the host and the CPU tests.
//   1. group     launch_plan_groups (plan_kernels.hip): the (query, target) groups of the hits -- six contexts: the (read, target) pairs
//                with all their frames, the hits permuted into (read, target, frame, location, seed offset) order
//   2. walk      launch_xdrop_segs with no bias over ALL hits in one launch (the caller runs it in front of the grouping, whose permute
//                step carries the results along)
//   3. order     rank_key_kernel + a stable rocPRIM radix sort of hit indices by (group, diagonal); one context: j already ascends
//                inside a group (the hits arrive by (query, subject, seed offset)); six: a stable pass by j runs first
//   4. rank_walk_kernel   one lane per run of equal (group, diagonal): the skip rule over the run with binary-search jumps, then an
//                atomic max of the packed (score, reversed position) per group -- independent of the order of the lanes
//   5. rank_records_kernel + cut   one dmnd_ranked_target per group; n_keep > 0: a stable sort by (query, 65535 - score), the rank of a
//                record inside its query (the planner's query records give the query's first group: no extra scan), a scan of the
//                keep flags and a compaction
//
// Why the cut loses nothing for dmnd_rank_update. Within one block every target occurs once per query. Take a record r of query q
// outside the first N of its block in (score descending, target ascending) order: N other targets of that block precede it, each with
// a score >= r's, ties at smaller targets. dmnd_rank_update keeps per target its best score, so in the merged table each of those N
// targets holds a score at least as high as in this block, while r's target -- a sequence of this block only -- holds r's score: all
// N still precede r in the table's order (score descending, target ascending; the offset that turns block ids into ordinals keeps the
// order of targets) whatever the other blocks bring. So r is never among the N entries of q's row, and feeding the update each
// block's first N gives the table that all records give (tests/test_rank_core.py checks it on random records with many equal scores).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/diamond_hip.h"
#include "plan_kernels.h"
#include "rank_core.h"

namespace dmnd {

struct RankCounters { uint32_t n_groups, unsorted, n_records, pad; unsigned long long n_walked; };

struct RankArgs {
	PlanArgs plan;                 // the grouping launch's arguments: plan.hits / plan.xd are the lists in grouped order
	int n_keep;                    // 0: every record
	uint32_t target_offset;
	int j_bits, key_bits, cut_bits;      // radix sort widths: j inside a target, (group, diagonal), (query number, 65535 - score)
	// work arrays in HBM, n_hits entries each (+ 1 where noted)
	uint64_t* keys; uint64_t* keys_sorted;       // (group, diagonal) of the hits, then the cut's keys of the records
	uint32_t* idx_a; uint32_t* idx_b;             // hit indices on their way through the sorts
	int32_t* sj; int32_t* sj_end; int32_t* sscore;      // per sorted position: j, end of the hit's segment, its score (six contexts: first the j pass's keys)
	uint64_t* best;                // per group: packed (score, reversed position)
	dmnd_ranked_target* recs;      // one per group, in (query, target) order
	uint32_t* keep; uint32_t* keep_off;          // (+ 1) the cut's flags in sorted order, their exclusive scan
	dmnd_ranked_target* recs_out;  // the kept records
	RankCounters* counters;
};

// records of the call: a.recs (n_keep == 0) or a.recs_out, counters->n_records of them
hipError_t launch_rank(const RankArgs& a, hipStream_t st);

}  // namespace dmnd
