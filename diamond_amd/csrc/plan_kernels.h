// plan_kernels.h -- launch interface of the device planner of the extension stage (round 6): what load_hits + ungapped_stage +
// Chaining::run + add_dp_targets do per query on the reference's host threads
// (/root/reference/src/align/load_hits.h:44-127, align/ungapped.cpp:62-126, chaining/greedy_align.cpp:482-497,
// align/gapped_score.cpp:107-180), done for ALL seed hits of a block pair in a handful of launches: the hits are grouped by
// (query, target), every group's hits become diagonal segments (from the x-drop kernel's results), the segments are chained
// (chain_graph.h, the same source the host compiles) and the chains' bands merged into the DpTargets of round 1.
// Extension::Mode::FULL (--ext full, the final pass of --global-ranking; PlanArgs::ext_full): behind the grouping every group gets one
// band over its whole matrix (plan_full_kernel; align/ungapped.cpp:70-75, gapped_score.cpp:123-130) -- no x-drop results, segments or chains.
// The host path, for the queries that take it, keeps the ranking logic (which groups of a query are extended when) and only looks bands up.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/diamond_hip.h"
#include "xdrop_core.h"
#include "plan_core.h"

namespace dmnd {

enum {
	PLAN_ON_HOST = 255,        // PlanGroup::n_bands: the group is planned by the host (too many hits / segments for a lane's arrays)
	PLAN_NEED_CHAIN = 254,     // between the two planning kernels: segments written, chaining still to do
	PLAN_MAX_HITS = 32,
	PLAN_MAX_SEGS = 16
};

struct PlanGroup {             // the seed hits of one (query, target) pair = SeedHitList entry of load_hits
	uint32_t target;           // block sequence id
	uint32_t hit_begin;        // first hit of the group in the call's hit list
	uint32_t n_hits;
	uint32_t band_begin;       // first of its n_bands entries in the band list
	uint16_t score;            // best stage-1 score of its hits (TargetScore::score; WorkTarget::ungapped_score for one context)
	uint8_t pass;              // some hit passed the gapped filter (1 everywhere when the filter is off)
	uint8_t n_bands;           // DpTargets of round 1, or PLAN_ON_HOST
};
struct PlanBand { int32_t d_begin, d_end; };
struct PlanQuery { uint32_t query, group_begin, hit_begin; };      // one per query that has hits, in hit order; one sentinel entry behind the last (translated queries: the read, its first PAIR)
struct PlanCounters { uint32_t n_groups, n_queries, n_bands, unsorted, n_on_host, n_chain, n_chain_big, n_relisted, n_pairs, n_pairs_on_host; };      // n_chain / n_chain_big: groups with two to PLAN_SMALL_SEGS / more segments (plan_chain_list_kernel); n_relisted: small ones listed again for the large workspace (counted in n_chain_big too)

struct PlanArgs {
	const int8_t* qblock; const int8_t* tblock;
	const int64_t* qlimits; const int64_t* tlimits;
	int64_t n_targets;
	const int8_t* matrix;          // 32 x 32 int8
	const dmnd_seed_hit* hits; int64_t n_hits;
	const uint8_t* gf_flags;       // gapped filter flag per hit, or NULL (filter off)
	const XdropSeg* xd;            // x-drop extension of every hit (xdrop_seg_kernel)
	int gap_open, gap_extend, band_fast;
	int small_segs;                // groups with at most this many segments are chained with the small workspace (0: none; plan_kernels.hip)
	int ext_full;                  // Extension::Mode::FULL: every group gets one band, the whole matrix (plan_full_kernel); xd is not read
	// work and output arrays, all in HBM, sized for n_hits entries (+ 1 where a sentinel follows)
	uint32_t* tgt;                 // target of every hit
	uint64_t* heads;               // group head flag | query head flag << 32, then their inclusive scan
	uint64_t* head_scan;
	PlanGroup* groups;
	PlanQuery* queries;
	int32_t* segs;                 // 4 ints per hit slot: the sorted segments of a multi-segment group, from its first hit slot on
	PlanBand* band_slots;          // bands of a group, from its first hit slot on
	uint32_t* chain_list; uint32_t chain_cap;      // the groups that need chaining (at most one per two hits): small ones from the front, the others from the back
	uint32_t* band_count;          // per group, then its exclusive scan in band_off
	uint32_t* band_off;
	PlanBand* bands;               // dense
	PlanCounters* counters;
	void** scan_tmp; size_t* scan_tmp_bytes;
	// Translated queries (contexts = 6; every pointer below NULL otherwise). The call's hits arrive context after context; a stable radix
	// sort by (read, target) (plan_core.h) brings them into (read, target, frame, location, seed offset) order, and hits / gf_flags / xd
	// above are the permuted copies. `groups` stay the (context, target) units that segments, chaining and bands are made for; one
	// level above them the (read, target) PAIRS of up to six consecutive units are what the device half ranks and reports.
	int contexts;
	const dmnd_seed_hit* hits_in; const uint8_t* gf_in; const XdropSeg* xd_in;      // the call's lists as they arrive
	dmnd_seed_hit* hits_sorted; uint8_t* gf_sorted; XdropSeg* xd_sorted;
	uint64_t* keys; uint64_t* keys_sorted; uint32_t* perm_in; uint32_t* perm;         // perm[k]: where sorted hit k lay in the call's list
	int target_bits, key_bits;
	uint32_t* pheads; uint32_t* phead_scan;        // pair head flag of every hit, inclusive scan
	PlanGroup* pairs;              // (+ 1) score: the best over all frames; pass: some hit of the pair passed; n_bands: all its units' bands, which lie one after the other
	uint32_t* pair_unit;           // (+ 1) first unit of every pair
	uint32_t* unit_pair;
	uint16_t* ungapped0;           // per pair: best stage-1 score of context 0, 0 without a hit there (the record's ungapped_score)
	uint32_t* band_query;          // per band of the dense list: the context (block sequence id) it belongs to
};

hipError_t launch_plan(const PlanArgs& a, hipStream_t st);
// its grouping half alone (groups / pairs / queries of the hits; plan_kernels.hip): what the device form of the global ranking needs
hipError_t launch_plan_groups(const PlanArgs& a, hipStream_t st, size_t extra_tmp);

}  // namespace dmnd
