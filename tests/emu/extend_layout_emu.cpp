// tests/emu/extend_layout_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The work-array layout of the device half of the extension stage (diamond_amd/csrc/extend_core.h ext_layout, ext_regions) for
// one shape, so that tests/test_extend_layout.py can check that what the kernels touch and clear stays inside each region.
#include <cstdint>
#include "../../diamond_amd/csrc/extend_core.h"

using namespace dmnd;

// per region (layout order): name, offset, bytes the device half touches from there on; returns the number of regions (at most
// cap), and the buffer's size, the round-2 capacity and the item capacity
extern "C" int emu_ext_layout(uint64_t n_groups, uint64_t n_queries, uint64_t n_bands, int k, int cap, const char** names, uint64_t* off,
	uint64_t* used, uint64_t* bytes, uint64_t* r2_cap, uint64_t* item_cap)
{
	const ExtLayout L = ext_layout((size_t)n_groups, (size_t)n_queries, (size_t)n_bands, k);
	ExtRegion r[EXT_REGIONS];
	const int n = ext_regions(L, r);
	for (int i = 0; i < n && i < cap; ++i) { names[i] = r[i].name; off[i] = r[i].off; used[i] = r[i].used; }
	*bytes = L.bytes; *r2_cap = L.nR; *item_cap = L.nI;
	return n;
}
