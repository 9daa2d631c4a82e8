// extend_cbs_core.h -- the HIP-free part of the matrix adjustment (--comp-based-stats 2 - 5) inside the device half of the extension
// stage: the index arithmetic the kernels of extend_kernels.hip and the launchers of extend_device.hip share with the CPU emulator
// (tests/emu/extend_cbs_emu.cpp), and the layout of the step's work arrays in a buffer of their own (the way tr_layout does it;
// ext_layout stays as it is).
//   * the matrix code of an item: dmnd_dp_target::cbs_off of a group that owns matrix number `mat` of the work context's store
//     (swipe_kernels.h own_matrix_number reads it back), or the Hauser bias / none for a group on the standard matrix;
//   * the launch class of an item with a matrix of its own: its band class -- never a row class, never one of the packed 16-bit
//     launches -- counted EXT_OWN_CLASS above the classes of the standard matrix (api.hip's host scheme counts them 16 above, too);
//   * pair k of a ranking iteration -> slot before + k of the store (cbs_slots_assign, cbs_core.h, says the same on the host);
//   * the matrix number of a pair's group from the kernel's rule and status and -- for a pair the kernel handed back -- whether the
//     host form ended with a table.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "cbs_core.h"
#include "swipe_core.h"

#if defined(__HIPCC__)
#define EXTC_FN __host__ __device__ inline
#else
#define EXTC_FN inline
#endif

namespace dmnd {

enum { EXT_OWN_CLASS = 16, EXT_ALL_CLASSES = 32 };      // launch classes of the device scheme: [0, 16) standard matrix (EXT_CLASSES), [16, 32) own matrix
enum { EXT_MAT_UNSET = -2, EXT_MAT_STANDARD = -1 };     // g_mat: no pair listed for the group yet / the group keeps the standard matrix; >= 0: its slot

// cbs_off of a banded item (extend_host.hip item_of): own matrix -> -2 - mat, swept without the bias; else the bias row of the
// query (query_off) where the mode has the Hauser bias, or -1
EXTC_FN int64_t ext_matrix_code(int32_t mat, bool hauser, int64_t query_off)
{
	return mat >= 0 ? (int64_t)-2 - (int64_t)mat : hauser ? query_off : (int64_t)-1;
}

// launch class P of an item (api.hip sweep_class): the row classes take what the packed 16-bit kernels take, and those never take
// an item with a matrix of its own
EXTC_FN int ext_item_class(bool rows, bool own, int band, int64_t steps, int64_t max_pair_steps)
{
	return rows && !own && steps <= 2 * max_pair_steps ? band_class_rows(band) : band_class(band);
}

// ... and its number among the device scheme's launch classes (the sort key, the counters)
EXTC_FN int ext_class_slot(int P, bool own) { return class_index(P) + (own ? (int)EXT_OWN_CLASS : 0); }

EXTC_FN int64_t ext_pair_slot(int64_t before, int64_t k) { return before + k; }

// matrix number of pair k's group. keep: the host form's verdict on a handed-back pair (0 = its rule was NONE: no table), unused
// for a pair the kernel decided
EXTC_FN int32_t ext_pair_matrix(int64_t before, int64_t k, int32_t rule, uint8_t status, uint8_t keep)
{
	if (status != CBS_ST_DEVICE) return keep ? (int32_t)ext_pair_slot(before, k) : (int32_t)EXT_MAT_STANDARD;
	return rule == CBSD_RULE_NONE ? (int32_t)EXT_MAT_STANDARD : (int32_t)ext_pair_slot(before, k);
}

// the step's counters: the pairs of the current iteration and the launch classes of its own-matrix items (ExtCounters keeps its shape)
struct ExtCbsCounters {
	uint32_t n_pairs, pad[15];
	uint32_t class_count[EXT_OWN_CLASS];
	uint32_t class_max_steps[EXT_OWN_CLASS];
};

// Byte offsets of the step's arrays (each 64-byte aligned) for nG groups and nQ planned queries. A group is listed as a pair once
// in a call, so nG bounds the pairs of an iteration.
struct ExtCbsLayout {
	size_t nG, nQ;
	size_t o_g_mat;         // per group: EXT_MAT_* or its slot; lives for the whole call
	size_t o_g_row;         // per group: its planned query (row of the compositions)
	size_t o_comp, o_true_aa;       // per planned query: 20 doubles, count of true amino acids
	size_t o_flag, o_pos;   // (+ 1) per group: listed in this iteration / exclusive scan
	size_t o_pair_group, o_qidx, o_toff, o_tlen, o_qoff, o_qlen;      // per pair: group, query row, target offset / length, query offset / length
	size_t o_rule, o_status, o_keep;        // per pair: the kernel's answers, the host's verdict on the handed-back ones
	size_t o_model, o_ctr;
	size_t bytes;
};

inline ExtCbsLayout ext_cbs_layout(size_t nG, size_t nQ)
{
	ExtCbsLayout L;
	L.nG = nG; L.nQ = nQ;
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 63) & ~(size_t)63; return o; };
	L.o_g_mat = take(nG * 4); L.o_g_row = take(nG * 4);
	L.o_comp = take(nQ * CBSD_N * 8); L.o_true_aa = take(nQ * 4);
	L.o_flag = take((nG + 1) * 4); L.o_pos = take((nG + 1) * 4);
	L.o_pair_group = take(nG * 4); L.o_qidx = take(nG * 4); L.o_toff = take(nG * 8); L.o_tlen = take(nG * 4); L.o_qoff = take(nG * 8); L.o_qlen = take(nG * 4);
	L.o_rule = take(nG * 4); L.o_status = take(nG); L.o_keep = take(nG);
	L.o_model = take(sizeof(CbsDevModel)); L.o_ctr = take(sizeof(ExtCbsCounters));
	L.bytes = at;
	return L;
}

struct ExtCbsRegion { const char* name; size_t off, used; };
enum { EXT_CBS_REGIONS = 17 };

// what the kernels and copies touch of each array, from its offset on, in layout order; returns the number of regions
inline int ext_cbs_regions(const ExtCbsLayout& L, ExtCbsRegion* r)
{
	const size_t nG = L.nG, nQ = L.nQ;
	int n = 0;
	auto add = [&](const char* name, size_t off, size_t used) { r[n++] = ExtCbsRegion{ name, off, used }; };
	add("g_mat", L.o_g_mat, nG * 4); add("g_row", L.o_g_row, nG * 4);
	add("comp", L.o_comp, nQ * CBSD_N * 8); add("true_aa", L.o_true_aa, nQ * 4);
	add("flag", L.o_flag, (nG + 1) * 4); add("pos", L.o_pos, (nG + 1) * 4);      // (the scan: entries + 1)
	add("pair_group", L.o_pair_group, nG * 4); add("qidx", L.o_qidx, nG * 4); add("toff", L.o_toff, nG * 8); add("tlen", L.o_tlen, nG * 4);
	add("qoff", L.o_qoff, nG * 8); add("qlen", L.o_qlen, nG * 4);
	add("rule", L.o_rule, nG * 4); add("status", L.o_status, nG); add("keep", L.o_keep, nG);
	add("model", L.o_model, sizeof(CbsDevModel)); add("cbs_ctr", L.o_ctr, sizeof(ExtCbsCounters));
	return n;
}

}  // namespace dmnd
