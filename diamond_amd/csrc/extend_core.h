// extend_core.h -- the HIP-free part of the device half of the extension stage (extend_kernels.h): its constants, its counters and
// the layout of its work arrays in one buffer (extend_on_device, extend_device.hip). Plain C++, so that the CPU tests
// (tests/emu/extend_layout_emu.cpp) check the same numbers the launchers use: every array, and every extent the device half clears,
// inside its region of the buffer. The arrays of a call that returns transcripts have a layout of their own (tr_layout, below).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/diamond_hip.h"

namespace dmnd {

enum { EXT_CLASSES = 16, EXT_MAX_CHUNK = 1024, EXT_MAX_GROUPS = 1 << 16, EXT_MAX_ITERATIONS = 64 };
enum { EXT_FILTER_LIST = 2048 };          // with HSP filters: aligned targets of one query the LDS list of ext_fappend_kernel holds (a query with more goes back to the host)
enum { EXT_SWIPE_END_BYTES = 32 };      // sizeof(SwipeEnd) (swipe_kernels.h; checked in extend_kernels.h)

struct ExtCounters {
	uint32_t n_items;                        // of the current iteration
	uint32_t n_active;                       // queries that go on to another ranking chunk
	uint32_t n_saturated, n_kept, n_ambiguous, n_resweep;      // n_resweep: survivors whose round-1 sweep kept no trace
	int32_t tb_status;                       // traceback_kernel's status word (0 = every walk ended at a cell with score 0)
	uint32_t n_capped;                       // queries still ranking after the last allowed chunk: handed back to the host
	// (the arrays and the 64-bit counters below lie back to back: reset_iteration clears them in one go)
	uint32_t class_count[EXT_CLASSES];       // items of the current iteration per launch class c (P = class_of_index(c), swipe_core.h)
	uint32_t class_max_steps[EXT_CLASSES];
	unsigned long long total_rows;           // trace bytes of the current iteration's items
	unsigned long long cells1, cells2;       // DP cells of all round-1 items / of the items walked in round 2 (the reference's round-2 targets)
	unsigned long long cells_again;          // ... of those of them that round 2 swept again (their round-1 sweep kept no trace rows)
	unsigned long long window_targets, window_bound;      // of the current iteration: targets in the active queries' windows, and sum over the queries of min(-k, targets): what can survive the culling
	unsigned long long diag_steps, lane_steps;   // over the round-1 items: band diagonals x anti-diagonal steps, and the 128 P diagonals the item's wavefront holds x steps (lane use of the sweeps)
	uint32_t list_need, list_pad;            // with HSP filters, of the current iteration: the most targets one active query has had swept so far = what its aligned targets and the chunk's can come to (sizes the LDS list of ext_fappend_kernel)
	uint32_t n_filtered, n_threshold;        // with HSP filters: records a filter removed (of the queries done here), queries handed back for a value on a threshold
	uint32_t n_records, n_records_pad;       // --top: entries of the walked list that are records (with HSP filters fewer than n_kept)
};

// Byte offsets of the work arrays in the buffer (each 64-byte aligned), for nG groups, nQ queries, nB bands and -k k
struct ExtLayout {
	size_t nG, nQ, nB;
	bool filters;           // the layout of a call with HSP filters (--id, --approx-id, covers): the arrays below marked so exist
	bool top;               // the layout of a --top call: the arrays below marked so exist
	size_t nR;              // round-2 capacity: survivors = records (at most -k per query, at most one per group); --top: nG -- the
	                        // cut is a threshold against the best score, so every group of a query can become a record
	size_t nS;              // capacity of the trace walk's list: nR; with HSP filters nG -- every target of a chunk that passes the report
	                        // cutoff is walked BEFORE the culling (a group is swept once, so the groups bound all chunks' candidates)
	size_t nI;              // items: every band once + a copy of every walked target (round 2 without kept traces)
	size_t r2_tr_clear;     // entries of r2_tr that launch_ext_begin zeroes (the transcript offsets of the round-2 list)
	size_t o_qstate, o_qactive, o_qi0, o_qi1, o_qtail, o_qprev, o_qswept;
	size_t o_okeys, o_okeys2, o_oidx, o_gorder, o_aligned, o_gfirst, o_gcnt, o_cnt, o_item_off, o_kept, o_kept_pos, o_cand_item, o_cand_ev;
	size_t o_fverdict, o_matched, o_qmatched, o_qremoved;      // with HSP filters only (empty otherwise)
	size_t o_cand_score, o_rperm;                              // --top only (empty otherwise): best reported score per group, record order of the walked list
	size_t o_items, o_off_item, o_p, o_ends, o_hsps, o_keys, o_keys_sorted, o_idx, o_order, o_rows, o_rows_slot, o_off_slot, o_pairs;
	size_t o_r2_order, o_r2_p, o_r2_off, o_r2_tr, o_r2_group, o_records, o_ctr;
	size_t bytes;           // the whole buffer
};

inline ExtLayout ext_layout(size_t nG, size_t nQ, size_t nB, int k, bool filters = false, bool top = false)
{
	ExtLayout L;
	L.nG = nG; L.nQ = nQ; L.nB = nB; L.filters = filters; L.top = top;
	const size_t kk = k > 1 ? (size_t)k : 1;
	L.nR = top || nG < nQ * kk ? nG : nQ * kk;
	L.nS = filters || top ? nG : L.nR;
	L.nI = nB + L.nS;
	L.r2_tr_clear = L.nS + 1;
	const size_t nI = L.nI, nR = L.nR, nS = L.nS;
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 63) & ~(size_t)63; return o; };
	L.o_qstate = take(nQ); L.o_qactive = take(nQ); L.o_qi0 = take(nQ * 4); L.o_qi1 = take(nQ * 4); L.o_qtail = take(nQ * 4); L.o_qprev = take(nQ * 4); L.o_qswept = take(nQ * 4);
	L.o_okeys = take(nG * 8); L.o_okeys2 = take(nG * 8); L.o_oidx = take(nG * 4); L.o_gorder = take(nG * 4); L.o_aligned = take(nG); L.o_gfirst = take(nG * 4); L.o_gcnt = take(nG * 4);
	L.o_cnt = take((nG + 1) * 4); L.o_item_off = take((nG + 1) * 4); L.o_kept = take((nG + 1) * 4); L.o_kept_pos = take((nG + 1) * 4); L.o_cand_item = take(nG * 4); L.o_cand_ev = take(nG * 8);
	L.o_fverdict = take(filters ? nG : 0); L.o_matched = take(filters ? nG : 0); L.o_qmatched = take(filters ? nQ * 4 : 0); L.o_qremoved = take(filters ? nQ * 4 : 0);
	L.o_cand_score = take(top ? nG * 4 : 0); L.o_rperm = take(top ? nS * 4 : 0);
	L.o_items = take(nI * sizeof(dmnd_dp_target)); L.o_off_item = take(nI * 8); L.o_p = take(nI * 4); L.o_ends = take(nI * EXT_SWIPE_END_BYTES); L.o_hsps = take(nI * sizeof(dmnd_hsp));
	L.o_keys = take(nI * 4); L.o_keys_sorted = take(nI * 4); L.o_idx = take(nI * 4); L.o_order = take(nI * 4); L.o_rows = take(nI * 8); L.o_rows_slot = take((nI + 1) * 8); L.o_off_slot = take((nI + 1) * 8);
	L.o_pairs = take((nI + 8 * EXT_CLASSES) * 4);
	L.o_r2_order = take(nS * 4); L.o_r2_p = take(nS * 4); L.o_r2_off = take(nS * 8); L.o_r2_tr = take((nS + 1) * 8); L.o_r2_group = take(nS * 4);
	L.o_records = take(nR * sizeof(dmnd_match)); L.o_ctr = take(sizeof(ExtCounters));
	L.bytes = at;
	return L;
}

// What the device half touches of each array, from the array's offset on: its reads and writes by the sizes the kernels index with
// (n_groups, item_cap = nI, r2_cap = nR), and its memset clears. In layout order; returns the number of regions. Under --top the
// record order of the walked list is sorted in okeys / okeys_sorted / oidx (free once the ranking order stands; nS = nG entries).
struct ExtRegion { const char* name; size_t off, used; };
enum { EXT_REGIONS = 46 };

inline int ext_regions(const ExtLayout& L, ExtRegion* r)
{
	const size_t nG = L.nG, nQ = L.nQ, nI = L.nI, nR = L.nR, nS = L.nS;
	const bool filters = L.filters, top = L.top;
	int n = 0;
	auto add = [&](const char* name, size_t off, size_t used) { r[n++] = ExtRegion{ name, off, used }; };
	add("qstate", L.o_qstate, nQ); add("q_active", L.o_qactive, nQ); add("q_i0", L.o_qi0, nQ * 4); add("q_i1", L.o_qi1, nQ * 4);
	add("q_tail", L.o_qtail, nQ * 4); add("q_prev", L.o_qprev, nQ * 4); add("q_swept", L.o_qswept, nQ * 4);
	add("okeys", L.o_okeys, nG * 8); add("okeys_sorted", L.o_okeys2, nG * 8); add("oidx", L.o_oidx, nG * 4); add("gorder", L.o_gorder, nG * 4);
	add("aligned", L.o_aligned, nG); add("g_first", L.o_gfirst, nG * 4); add("g_cnt", L.o_gcnt, nG * 4);
	add("cnt", L.o_cnt, (nG + 1) * 4); add("item_off", L.o_item_off, (nG + 1) * 4);         // (entry n_groups: ext_window_kernel, the scans)
	add("kept", L.o_kept, (nG + 1) * 4); add("kept_pos", L.o_kept_pos, (nG + 1) * 4);
	add("cand_item", L.o_cand_item, nG * 4); add("cand_ev", L.o_cand_ev, nG * 8);
	add("fverdict", L.o_fverdict, filters ? nG : 0); add("matched", L.o_matched, filters ? nG : 0);
	add("q_matched", L.o_qmatched, filters ? nQ * 4 : 0); add("q_removed", L.o_qremoved, filters ? nQ * 4 : 0);
	add("cand_score", L.o_cand_score, top ? nG * 4 : 0); add("rperm", L.o_rperm, top ? nS * 4 : 0);
	add("items", L.o_items, nI * sizeof(dmnd_dp_target)); add("off_item", L.o_off_item, nI * 8); add("p_of_item", L.o_p, nI * 4);
	add("ends", L.o_ends, nI * EXT_SWIPE_END_BYTES); add("hsps", L.o_hsps, nI * sizeof(dmnd_hsp));
	add("keys", L.o_keys, nI * 4); add("keys_sorted", L.o_keys_sorted, nI * 4); add("idx", L.o_idx, nI * 4); add("order", L.o_order, nI * 4);
	add("rows", L.o_rows, nI * 8);
	add("rows_slot", L.o_rows_slot, (nI + 1) * 8); add("off_slot", L.o_off_slot, (nI + 1) * 8);      // (ext_slots_kernel, the scan: n_left + 1)
	add("pairs", L.o_pairs, (nI + 8 * EXT_CLASSES) * 4);          // (the last wavefront of each class filled up with -1: < 8 per class)
	add("r2_order", L.o_r2_order, nS * 4); add("r2_p", L.o_r2_p, nS * 4); add("r2_off", L.o_r2_off, nS * 8);
	add("r2_tr", L.o_r2_tr, L.r2_tr_clear * 8);                   // (launch_ext_begin's clear)
	add("r2_group", L.o_r2_group, nS * 4); add("records", L.o_records, nR * sizeof(dmnd_match));
	add("ctr", L.o_ctr, sizeof(ExtCounters));                     // (launch_ext_begin's clear, reset_iteration's)
	return n;
}

// ---- transcripts (a call with a transcript arena; transcript_core.h) ----
// The arrays between the trace walk and the caller's arena live in a buffer of their own, laid out here the same way: nG groups,
// nS = the capacity of the walked list, nR = the capacity of the records (ExtLayout::nS, nR of the same call).
struct TrCounters {
	uint32_t n_pieces;                       // of the current walk: its pieces (tr_piece_end), their bounds in `pieces`
	uint32_t missing;                        // != 0: the gather step met a record whose group has no transcript in the store (the call fails)
	long long raw_total, raw_max;            // ... raw-slot bytes of the whole list and of its largest piece
	long long pad2[5];
};

struct TrLayout {
	size_t nG, nS, nR;
	size_t o_g_store;       // per group: where its transcript lies in the store (valid once its chunk has been walked)
	size_t o_k_len, o_k_off;        // (+ 1) per entry of the current piece: slot widths before the walk, kept lengths behind it / their scan
	size_t o_r_len, o_r_off;        // (+ 1) per record: bytes in the output / their scan = the records' transcript offsets
	size_t o_pieces;        // (+ 1) first entry of each piece of the current walk
	size_t o_ctr;
	size_t bytes;
};

inline TrLayout tr_layout(size_t nG, size_t nS, size_t nR)
{
	TrLayout T;
	T.nG = nG; T.nS = nS; T.nR = nR;
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 63) & ~(size_t)63; return o; };
	T.o_g_store = take(nG * 8);
	T.o_k_len = take((nS + 1) * 8); T.o_k_off = take((nS + 1) * 8);
	T.o_r_len = take((nR + 1) * 8); T.o_r_off = take((nR + 1) * 8);
	T.o_pieces = take((nS + 1) * 4);
	T.o_ctr = take(sizeof(TrCounters));
	T.bytes = at;
	return T;
}

enum { TR_REGIONS = 7 };

inline int tr_regions(const TrLayout& T, ExtRegion* r)
{
	int n = 0;
	auto add = [&](const char* name, size_t off, size_t used) { r[n++] = ExtRegion{ name, off, used }; };
	add("g_store", T.o_g_store, T.nG * 8);
	add("k_len", T.o_k_len, (T.nS + 1) * 8); add("k_off", T.o_k_off, (T.nS + 1) * 8);      // (the scans: entries + 1)
	add("r_len", T.o_r_len, (T.nR + 1) * 8); add("r_off", T.o_r_off, (T.nR + 1) * 8);
	add("pieces", T.o_pieces, (T.nS + 1) * 4);                                              // (a piece has at least one entry)
	add("tr_ctr", T.o_ctr, sizeof(TrCounters));
	return n;
}

}  // namespace dmnd
