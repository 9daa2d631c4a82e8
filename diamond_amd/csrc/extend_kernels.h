// extend_kernels.h -- launch interface of the device half of the extension stage behind the planner (round 6). Everything between
// the planner's band list and the match records happens in HBM, ranking chunk by ranking chunk (/root/reference/src/align/extend.cpp:
// 289-336: a query's targets are taken ranking_chunk_size at a time in the order of their seed-hit scores until a chunk brings no new
// hit and the tail rule says stop); most queries have one chunk:
//   DpTargets of round 1 from the bands, their launch order (band class ascending, longest first), trace offsets and item pairs
//                         (what api.hip's dmnd_swipe_keep prepares on the host: DP::BandedSwipe::bin, /root/reference/src/dp/swipe/swipe_wrapper.cpp:75-102)
//   best HSP per target, report cutoff          (/root/reference/src/align/gapped_score.cpp:182-268, target.h:97-113)
//   culling: sort by (e-value, score, target), first -k targets            (/root/reference/src/align/culling.cpp:97-113, 189-203)
//   round 2 = a walk of the kept traces of the survivors                     (/root/reference/src/align/gapped_final.cpp:66-160)
//   match records in (query, e-value, score, target) order                   (/root/reference/src/align/extend.h:51-56, extend.cpp:341)
//   with a transcript arena: the walk's packed transcripts kept in a dense store, gathered in record order (TrArgs below)
// The e-value is double arithmetic with exp / erfc (evalue.h); the device's versions of those differ from the host library's in the
// last bits, so the device value only DECIDES (cutoff, order, first k) and a decision that two values closer than 1e-9 relative
// could flip marks the query `ambiguous`: the host redoes that query (two values that are 0.0 on both sides are ordered by score and
// target exactly; next to the underflow two tiny values are always flagged). The records leave with the device value; the host overwrites
// it with its own (and the bit score) and checks the order. Queries with a group the planner left to the host, with an item the
// traceback path cannot take or with more than EXT_MAX_GROUPS groups stay on the host path (extend_host.hip extend_range).
// The bands are the planner's: chained and merged ones of a banded search, or -- Extension::Mode::FULL: --ext full, the final pass of
// --global-ranking -- one band over the whole matrix per target and context with a seed hit; there an item is held against max_swipe_dp
// with query length x target length (ExtArgs::ext_full), everything behind ext_mark_kernel is the same.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/diamond_hip.h"
#include "extend_core.h"
#include "extend_cbs_core.h"
#include "filter_core.h"
#include "top_core.h"
#include "transcript_core.h"
#include "plan_kernels.h"
#include "swipe_kernels.h"

namespace dmnd {

static_assert(sizeof(SwipeEnd) == EXT_SWIPE_END_BYTES, "extend_core.h lays the per-item ends out with this size");

struct ExtEvalue {             // Evaluer (evalue.h) as plain data + the report cutoff
	double lambda, K, ln_k, db_letters, a, b, alpha, beta, sigma, tau, v_thr, c_thr, max_evalue;
};

struct ExtArgs {
	// planner output (HBM) and the blocks' limits
	const PlanGroup* groups; const PlanQuery* queries; const PlanBand* bands;
	uint32_t n_groups, n_queries, n_bands;
	const dmnd_seed_hit* hits;
	const int64_t* qlimits; const int64_t* tlimits;
	// translated queries (contexts = 6; NULL otherwise): a group is a (read, target) pair, a query a read; every band carries its
	// context, and the record's ungapped score is context 0's
	int contexts;
	const uint32_t* band_query; const uint16_t* ungapped0;
	const int32_t* source_lens;    // translated queries with HSP filters: the DNA length of every read of the block (--query-cover is measured on it); NULL otherwise
	int use_cbs;
	uint32_t row_min_items;        // items of an iteration from which on the row classes of the packed 16-bit sweeps are used (sweep_rows_min_items)
	uint32_t chunk_size;           // ranking_chunk_size
	int k;                         // max_target_seqs
	int64_t max_swipe_dp;
	int ext_full;                  // Extension::Mode::FULL: max_swipe_dp is held against query length x target length (plan_core.h full_matrix_dp_size)
	ExtEvalue ev;
	double min_bit_score;          // --min-score: != 0 replaces the e-value cutoff (ScoreMatrix::report_cutoff)
	FilterCfg filt; int filt_on;   // the HSP filters (filter_core.h); filt_on: the filter arrays exist (without top_on: the call runs the filtered ranking loop, the f-kernels)
	TopCfg top; int top_on;        // --top (top_core.h); top_on: the call runs the --top kernels, -k plays no part
	// per query
	uint8_t* qstate;               // EXT_Q_*
	uint8_t* q_active;             // still ranking: its window [q_i0, q_i1) of the order below is the next chunk
	uint32_t* q_i0; uint32_t* q_i1;
	int32_t* q_tail; int32_t* q_prev;        // tail_score / previous_tail_score of the ranking loop
	uint32_t* q_swept;             // targets of its current window that are swept (0: none, or not active)
	uint32_t* q_matched; uint32_t* q_removed;      // filt_on: matches of the rounds so far (Extension::extend's `matches`), records a filter removed
	// per group
	uint64_t* okeys; uint64_t* okeys_sorted; uint32_t* oidx;      // ranking order: sort keys (query, 0xffff - score), group numbers
	uint32_t* gorder;              // groups of a query in ranking order (TargetScore::operator<: score descending, then load order)
	uint8_t* aligned;              // the target is in the query's aligned_targets
	uint32_t* g_first; uint32_t* g_cnt;      // its round-1 items (once its chunk has been swept)
	uint32_t* cnt; uint32_t* item_off;       // (+ 1) items of the current iteration per group, exclusive scan
	uint32_t* kept; uint32_t* kept_pos;      // (+ 1) survives the final culling / its record slot
	uint32_t* cand_item;           // the item of its best HSP
	double* cand_ev;
	uint8_t* fverdict;             // filt_on: the filters' verdict on the target's best HSP (EXT_F_*)
	uint8_t* matched;              // filt_on: the target is one of the query's matches of an earlier round
	int32_t* cand_score;           // top_on: the score of its best reported HSP (0: none, or not swept yet)
	// per item: all iterations' items one after the other (a group is swept once, so n_bands bounds them)
	uint32_t item_base;            // first item of the current iteration
	uint32_t item_cap;             // room in the per-item arrays: n_bands + one copy of every survivor (round 2 sweeps those again whose traces were not kept)
	dmnd_dp_target* items;
	int64_t* off_item;             // trace offset: inside the iteration's arena for its sweeps, from the first arena on afterwards
	int32_t* p_of_item;
	SwipeEnd* ends;
	dmnd_hsp* hsps;
	// per item of the current iteration (indices relative to item_base)
	uint32_t* keys; uint32_t* keys_sorted; uint32_t* idx; uint32_t* order;      // launch order: slot -> item
	int64_t* rows; int64_t* rows_slot; int64_t* off_slot;
	int32_t* pairs;
	// round 2 and output
	uint32_t r2_cap;               // room in the round-2 arrays and the records (ExtLayout::nR)
	uint32_t r2_tr_clear;          // entries of r2_tr that launch_ext_begin zeroes (ExtLayout::r2_tr_clear)
	int32_t* r2_order; int32_t* r2_p; int64_t* r2_off; int64_t* r2_tr;       // slot -> item, band class, trace offset, (zero) transcript offsets
	uint32_t* r2_group;            // slot -> group
	uint32_t* rperm;               // top_on: record -> slot of the walked list (a query's records by score descending, target ascending)
	dmnd_match* records;
	ExtCounters* ctr;
	void** scan_tmp; size_t* scan_tmp_bytes;
	// --comp-based-stats 2 - 5 (extend_cbs_core.h; layout: ext_cbs_layout): g_mat == NULL -- every other call -- and none of these is read
	int32_t* g_mat;                // per group: EXT_MAT_UNSET until the group is listed as a pair, then EXT_MAT_STANDARD or its slot of the matrix store
	uint32_t* g_row;               // per group: its planned query
	double* q_comp; int32_t* q_true_aa;      // per planned query: composition (20 doubles), true amino acids
	uint32_t* c_flag; uint32_t* c_pos;       // (+ 1) per group: a new pair of this iteration, exclusive scan
	uint32_t* pair_group; int32_t* pair_qidx; int64_t* pair_toff; int32_t* pair_tlen; int64_t* pair_qoff; int32_t* pair_qlen;      // per pair of this iteration
	int32_t* pair_rule; uint8_t* pair_status; uint8_t* pair_keep;
	ExtCbsCounters* cbs_ctr;
	int tr_on;                     // the call returns transcripts: a record leaves the records kernels with its GROUP in hsp.transcript_off
	                               // (launch_tr_gather turns it into the offset); 0: -1, as ever
};

// The transcripts of a call with a transcript arena (transcript_core.h; layout: extend_core.h tr_layout). The trace walk writes each
// walked entry's packed transcript into a raw slot; the KEEP step behind every walk copies them into a dense, append-only store
// (a chunk's trace rows are gone once the next chunk is swept, its transcripts stay); the GATHER step, once the records exist,
// copies each record's transcript from the store into the output in record order. One wavefront per entry, byte copies, offsets
// from scans: no atomics, the same layout in every run. Raw slots, store and output are three allocations, each addressed from its
// own base by offsets >= 0.
struct TrArgs {
	int64_t* g_store;              // per group: offset of its transcript in the store
	int64_t* k_len; int64_t* k_off;          // per entry of the current piece (+ 1)
	int64_t* r_len; int64_t* r_off;          // per record (+ 1)
	uint32_t* pieces;              // first entry of each piece of the current walk (+ 1: the list's end)
	TrCounters* ctr;
};

// before a walk of the first n entries of the round-2 list: a.r2_tr[0 .. n] = exclusive scan of the entries' slot widths
// (tr_slot_bytes), and the list cut into consecutive pieces of at most `limit` raw bytes (at least one entry): t.pieces, t.ctr
hipError_t launch_tr_slots(const ExtArgs& a, const TrArgs& t, uint32_t n, int64_t limit, hipStream_t st);
// behind the walk of the piece [s0, s0 + m): the kept lengths of its entries and their scan, t.k_off[m] = the piece's bytes in the store ...
hipError_t launch_tr_keep_sizes(const ExtArgs& a, const TrArgs& t, uint32_t s0, uint32_t m, hipStream_t st);
// ... and the copy raw -> store + base (store holds base + t.k_off[m] bytes at least), the store offset of each entry's group
hipError_t launch_tr_keep(const ExtArgs& a, const TrArgs& t, uint32_t s0, uint32_t m, const uint8_t* raw, uint8_t* store, int64_t base, hipStream_t st);
// behind the records kernels (a.tr_on): the records' output sizes and their scan, t.r_off[n] = bytes of the output ...
hipError_t launch_tr_gather_sizes(const ExtArgs& a, const TrArgs& t, uint32_t n, hipStream_t st);
// ... and the copy store -> out (t.r_off[n] bytes at least), records[r].hsp.transcript_off = t.r_off[r]
hipError_t launch_tr_gather(const ExtArgs& a, const TrArgs& t, uint32_t n, const uint8_t* store, uint8_t* out, hipStream_t st);

enum { EXT_F_PASS = 0, EXT_F_FAIL = 1, EXT_F_THRESHOLD = 2 };
enum { EXT_Q_HOST = 0, EXT_Q_DEVICE = 1, EXT_Q_AMBIGUOUS = 2, EXT_Q_CAPPED = 3 };      // CAPPED: still ranking after the last allowed chunk

// once per call: which queries run here, their ranking order, the state of their ranking loops
hipError_t launch_ext_begin(const ExtArgs& a, hipStream_t st);
// one iteration, before its sweeps: the DpTargets of every active query's current chunk, launch order, trace offsets, pairs
// (a.item_base = items of the earlier iterations); the counts stay in ctr
hipError_t launch_ext_prepare(const ExtArgs& a, hipStream_t st);
// The same in three steps for a call with matrix adjustment (a.g_mat != NULL; --comp-based-stats 2 - 5). launch_ext_cbs_begin,
// once per call behind launch_ext_begin: the composition of every planned query (one wavefront each, the counting and the single
// division of cbsd_pair's target side), every group's query row, g_mat = EXT_MAT_UNSET. launch_ext_cbs_window: the windows (cnt per
// group) and the iteration's new pairs -- every group with cnt > 0 and no matrix number yet, in group order: pair k -> group, query
// row, target offset and length (the lists cbs_adjust_kernel takes), cbs_ctr->n_pairs. The host has the kernel fill the slots
// before + k of the matrix store (dmnd_cbs_adjust_lists), computes the pairs it hands back and patches their slots.
// launch_ext_cbs_matrices: g_mat of the pairs' groups from rule, status and -- keep != 0 -- pair_keep (ext_pair_matrix).
// launch_ext_cbs_items: the rest of launch_ext_prepare; an item of a group with a matrix carries its code (ext_matrix_code) and
// is counted in a launch class of its own (cbs_ctr->class_count: 32-bit kernels only, never a row class).
hipError_t launch_ext_cbs_begin(const ExtArgs& a, const int8_t* qblock, hipStream_t st);
hipError_t launch_ext_cbs_window(const ExtArgs& a, hipStream_t st);
hipError_t launch_ext_cbs_matrices(const ExtArgs& a, int64_t before, uint32_t n_pairs, bool keep, hipStream_t st);
hipError_t launch_ext_cbs_items(const ExtArgs& a, hipStream_t st);
// ... behind its sweeps: best HSP per target, append_hits, the next chunk or the end of the query's ranking. kept: the sweeps ran in
// traceback mode and their trace rows stay (rel = the iteration's arena relative to the first one); else round 2 sweeps the
// survivors of this iteration again. Then -- speculatively: it only counts if ctr->n_active comes back 0 -- the final culling and
// the round-2 list. last: no further chunk is allowed -- a query that would go on is handed back to the host (EXT_Q_CAPPED)
hipError_t launch_ext_append(const ExtArgs& a, uint32_t n_items, bool kept, int64_t rel, bool last, hipStream_t st);
// round 2, first half, for the survivors without kept trace rows: copies of their items as one more iteration (launch order, trace
// offsets, pairs); then, behind its traceback-mode sweeps, launch_ext_rewalk points the round-2 list at the copies
hipError_t launch_ext_resweep(const ExtArgs& a, uint32_t n_kept, hipStream_t st);
hipError_t launch_ext_rewalk(const ExtArgs& a, uint32_t n_items, uint32_t n_kept, int64_t rel, hipStream_t st);
// With HSP filters (a.filt_on; src/align/extend.cpp:226-344 with have_filters, src/align/gapped_final.cpp:105-152) a chunk takes
// three steps behind its sweeps instead of launch_ext_append: launch_ext_fcand lists the chunk's targets past the report cutoff
// in the round-2 arrays (ctr->n_kept of them, ctr->n_resweep without kept trace rows: launch_ext_resweep / _rewalk as in round 2);
// the host has their traces walked; launch_ext_fappend then filters them (ext_filter_kernel, one lane per listed target) and runs
// the query's ranking step: append_hits without culling and -- where the chunk loop ends -- round 2's stepping over the sorted
// aligned targets, in which a target that fails a filter takes no place, and the outer loop's decision to rank on.
// launch_ext_ffinal, once no query is left ranking: the first -k of every query's matches, record slots.
hipError_t launch_ext_fcand(const ExtArgs& a, uint32_t n_items, bool kept, int64_t rel, hipStream_t st);
hipError_t launch_ext_fappend(const ExtArgs& a, uint32_t n_listed, uint32_t list_need, bool last, hipStream_t st);      // list_need: ctr->list_need as launch_ext_fcand left it
hipError_t launch_ext_ffinal(const ExtArgs& a, hipStream_t st);
// after the walk: the records
hipError_t launch_ext_records(const ExtArgs& a, uint32_t n_kept, hipStream_t st);
// --top (a.top_on; src/align/culling.cpp:92-144 with config.toppercent, extend.cpp:272, 331, gapped_final.cpp:103-154). The culling
// never orders by e-value: the aligned targets are cut by a threshold against the bit score of the best one, and a chunk is appended
// by an integer comparison against the lowest score left -- wavefront reductions over the query's `aligned` flags in HBM, no LDS
// list and no limit on the number of aligned targets. launch_ext_top_append stands where launch_ext_append stands (and lists the
// survivors of the last cut for the walk, speculatively); a score within the tolerance of the cutoff hands the query back.
// launch_ext_top_records, after the walk of all n_walked survivors: with HSP filters their verdicts (ext_filter_kernel) and the
// cut against the best match that PASSED (a filtered match is a placeholder of score 0: it sorts last and drops out); then one
// stable device-wide sort of the walked list by (query, 0xffffffff - score) -- the list is in load order, ascending target, so
// that is Match::cmp_score order -- and the records written through that permutation; ctr->n_records of them.
hipError_t launch_ext_top_append(const ExtArgs& a, uint32_t n_items, bool kept, int64_t rel, bool last, hipStream_t st);
hipError_t launch_ext_top_records(const ExtArgs& a, uint32_t n_walked, hipStream_t st);

// the host's (e-value, bit score) pairs into the records where they lie in HBM; records of a context gathered for a join with
// their block-local target ids turned into database-wide ordinals
hipError_t launch_ext_patch(dmnd_match* records, const double* ev_bits, uint32_t n, hipStream_t st);
hipError_t launch_ext_gather(dmnd_match* dst, const dmnd_match* src, uint32_t n, uint32_t target_offset, hipStream_t st);

}  // namespace dmnd
