// tests/emu/filter_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The filter arithmetic of diamond_amd/csrc/filter_core.h (what the host path, the device filter kernel and the approx_pident column
// compute) and the layout of the device half's work arrays under filters (extend_core.h), for tests/test_filter_core.py.
#include <cstdint>
#include "../../diamond_amd/csrc/filter_core.h"
#include "../../diamond_amd/csrc/extend_core.h"

using namespace dmnd;

extern "C" double emu_hsp_approx_id(int score, int q_range, int s_range, int identities, int length) { return hsp_approx_id(score, q_range, s_range, identities, length); }
extern "C" double emu_approx_id(int score, int range1, int range2) { return approx_id(score, range1, range2); }
extern "C" unsigned emu_hamming_id_cutoff(double approx_min_id) { return hamming_id_cutoff(approx_min_id); }

// 0 = passes, 1 = removed, 2 = a value on a threshold
extern "C" int emu_filter_verdict(double min_id, double approx_min_id, double query_cover, double subject_cover, int score, int identities, int length,
	int q_begin, int q_end, int s_begin, int s_end, int qlen, int tlen)
{
	FilterCfg f;
	f.min_id = min_id; f.approx_id = approx_min_id; f.query_cover = query_cover; f.subject_cover = subject_cover;
	const FilterValues v = filter_values(score, identities, length, q_begin, q_end, s_begin, s_end, q_end - q_begin, qlen, tlen);
	return filter_on_threshold(f, v) ? 2 : filter_fails(f, v) ? 1 : 0;
}

// as emu_ext_layout (extend_layout_emu.cpp), for a call with HSP filters; also the capacity of the walked list
extern "C" int emu_ext_layout_filters(uint64_t n_groups, uint64_t n_queries, uint64_t n_bands, int k, int cap, const char** names, uint64_t* off,
	uint64_t* used, uint64_t* bytes, uint64_t* r2_cap, uint64_t* item_cap, uint64_t* walk_cap)
{
	const ExtLayout L = ext_layout((size_t)n_groups, (size_t)n_queries, (size_t)n_bands, k, true);
	ExtRegion r[EXT_REGIONS];
	const int n = ext_regions(L, r);
	for (int i = 0; i < n && i < cap; ++i) { names[i] = r[i].name; off[i] = r[i].off; used[i] = r[i].used; }
	*bytes = L.bytes; *r2_cap = L.nR; *item_cap = L.nI; *walk_cap = L.nS;
	return n;
}
