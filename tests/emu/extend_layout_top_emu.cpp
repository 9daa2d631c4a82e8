// tests/emu/extend_layout_top_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The work-array layout of the device half of the extension stage under --top (diamond_amd/csrc/extend_core.h ext_layout(.., top),
// ext_regions) for one shape, for tests/test_extend_layout_top.py: as emu_ext_layout (extend_layout_emu.cpp), also the capacity of
// the walked list.
#include <cstdint>
#include "../../diamond_amd/csrc/extend_core.h"

using namespace dmnd;

extern "C" int emu_ext_layout_top(uint64_t n_groups, uint64_t n_queries, uint64_t n_bands, int k, int filters, int cap, const char** names, uint64_t* off,
	uint64_t* used, uint64_t* bytes, uint64_t* r2_cap, uint64_t* item_cap, uint64_t* walk_cap)
{
	const ExtLayout L = ext_layout((size_t)n_groups, (size_t)n_queries, (size_t)n_bands, k, filters != 0, true);
	ExtRegion r[EXT_REGIONS];
	const int n = ext_regions(L, r);
	for (int i = 0; i < n && i < cap; ++i) { names[i] = r[i].name; off[i] = r[i].off; used[i] = r[i].used; }
	*bytes = L.bytes; *r2_cap = L.nR; *item_cap = L.nI; *walk_cap = L.nS;
	return n;
}
