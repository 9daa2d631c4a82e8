// tests/emu/extend_cbs_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The index arithmetic of the matrix adjustment inside the device half of the extension stage (diamond_amd/csrc/extend_cbs_core.h)
// as the kernels of extend_kernels.hip compute it, for tests/test_extend_cbs_core.py: the layout of the step's work arrays, the
// matrix code of an item and what the sweep kernels read back of it, the launch class of an item with a matrix of its own, the
// slots and matrix numbers of an iteration's pairs beside what the host's bookkeeping (cbs_slots_assign, cbs_core.h) says.
#include <cstdint>
#include "../../include/diamond_hip.h"
#include "../../diamond_amd/csrc/extend_cbs_core.h"
#include "../../diamond_amd/csrc/swipe16_core.h"

using namespace dmnd;

// the two readers of swipe_kernels.h (a HIP header), restated on the constant they share
static int64_t emu_own_matrix_number(int64_t cbs_off) { return (-2 - cbs_off) & (DMND_CBS_MATRIX_WITH_BIAS - 1); }
static bool emu_own_matrix_biased(int64_t cbs_off) { return cbs_off <= -2 && ((-2 - cbs_off) & DMND_CBS_MATRIX_WITH_BIAS) != 0; }

extern "C" int emu_ext_cbs_layout(uint64_t n_groups, uint64_t n_queries, int cap, const char** names, uint64_t* off, uint64_t* used, uint64_t* bytes)
{
	const ExtCbsLayout L = ext_cbs_layout((size_t)n_groups, (size_t)n_queries);
	ExtCbsRegion r[EXT_CBS_REGIONS];
	const int n = ext_cbs_regions(L, r);
	for (int i = 0; i < n && i < cap; ++i) { names[i] = r[i].name; off[i] = r[i].off; used[i] = r[i].used; }
	*bytes = L.bytes;
	return n;
}

// cbs_off of an item, and what a sweep kernel makes of it: out[0] = the code, out[1] = own matrix (1 / 0), out[2] = the matrix
// number read back, out[3] = swept with the bias row of the query (1 / 0)
extern "C" void emu_ext_matrix_code(int32_t mat, int hauser, int64_t query_off, int64_t* out)
{
	const int64_t code = ext_matrix_code(mat, hauser != 0, query_off);
	out[0] = code;
	out[1] = code <= -2 ? 1 : 0;
	out[2] = code <= -2 ? emu_own_matrix_number(code) : -1;
	out[3] = code >= 0 || emu_own_matrix_biased(code) ? 1 : 0;
}

// launch class of an item: out[0] = P, out[1] = its number among the device scheme's classes, out[2] = P is a row class,
// out[3] = the class goes to the packed 16-bit kernels as dmnd_sweep_classes decides it (api.hip)
extern "C" void emu_ext_item_class(int rows, int own, int band, int64_t steps, int* out)
{
	const int P = ext_item_class(rows != 0, own != 0, band, steps, (int64_t)SW16_MAX_PAIRS);
	const int slot = ext_class_slot(P, own != 0);
	out[0] = P; out[1] = slot; out[2] = row_class(P) ? 1 : 0;
	out[3] = slot < EXT_OWN_CLASS && sw16_class(P) && steps <= 2 * (int64_t)SW16_MAX_PAIRS ? 1 : 0;
}

// One iteration's pairs: slot[k] and g_mat[k] as the device computes them (keep: per pair, read for the handed-back ones), and
// beside them the host's bookkeeping: mat_host[k] (cbs_slots_assign, with the handed-back pairs without a table set to -1 as
// extend_range does), handed[0 .. return value), by_status[4]
extern "C" int64_t emu_ext_pair_matrices(int64_t before, int64_t n, const int32_t* rule, const uint8_t* status, const uint8_t* keep, int64_t* slot, int32_t* g_mat,
	int32_t* mat_host, int64_t* handed, int64_t* by_status)
{
	for (int64_t k = 0; k < n; ++k) { slot[k] = ext_pair_slot(before, k); g_mat[k] = ext_pair_matrix(before, k, rule[k], status[k], keep[k]); }
	const int64_t h = cbs_slots_assign(before, n, rule, status, mat_host, handed, by_status);
	for (int64_t x = 0; x < h; ++x) if (!keep[handed[x]]) mat_host[handed[x]] = -1;
	return h;
}

extern "C" void emu_ext_cbs_constants(int* out)
{
	out[0] = EXT_OWN_CLASS; out[1] = EXT_ALL_CLASSES; out[2] = EXT_MAT_UNSET; out[3] = EXT_MAT_STANDARD; out[4] = CLASS_INDICES; out[5] = (int)sizeof(ExtCbsCounters);
}
