"""CPU checks of the work-array layout of the device half of the extension stage under --top (diamond_amd/csrc/extend_core.h
ext_layout(.., top) and ext_regions, via tests/emu/libswipe_emu.so), over the grid of tests/test_extend_layout.py: the --top cut is a
threshold against the best score, so every group of a query can become a record -- the records, the walked list and the copies swept
again are sized for the groups whatever -k is; every array and every clear lies inside its region; the record order is sorted in
the arrays of the ranking order, which hold one entry per group; the layouts without --top keep their sizes."""
import ctypes

import numpy as np
import pytest

import emu_py as emu
from test_extend_layout import SHAPES, MAX_REGIONS, layout


def layout_top(n_groups, n_queries, n_bands, k, filters=False):
    lib = emu.lib()
    u64 = ctypes.c_uint64
    names = (ctypes.c_char_p * MAX_REGIONS)()
    off, used = np.zeros(MAX_REGIONS, np.uint64), np.zeros(MAX_REGIONS, np.uint64)
    total, r2_cap, item_cap, walk_cap = u64(0), u64(0), u64(0), u64(0)
    lib.emu_ext_layout_top.argtypes = [u64, u64, u64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    n = lib.emu_ext_layout_top(n_groups, n_queries, n_bands, k, int(filters), MAX_REGIONS, ctypes.cast(names, ctypes.c_void_p), off.ctypes.data, used.ctypes.data,
                               ctypes.byref(total), ctypes.byref(r2_cap), ctypes.byref(item_cap), ctypes.byref(walk_cap))
    assert 0 < n <= MAX_REGIONS
    return [(names[i].decode(), int(off[i]), int(used[i])) for i in range(n)], total.value, r2_cap.value, item_cap.value, walk_cap.value


@pytest.mark.parametrize("filters", [False, True], ids=["plain", "filters"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_top_layout_is_sized_for_every_group(shape, filters):
    n_groups, n_queries, n_bands, k = SHAPES[shape]
    regions, total, r2_cap, item_cap, walk_cap = layout_top(n_groups, n_queries, n_bands, k, filters)
    assert r2_cap == n_groups                              # records: every group, whatever -k is (also -k 1)
    assert walk_cap == n_groups
    assert item_cap == n_bands + n_groups                  # ... each with room for a copy swept again with traceback
    names = [r[0] for r in regions]
    assert len(set(names)) == len(names)
    for i, (name, off, used) in enumerate(regions):
        end = regions[i + 1][1] if i + 1 < len(regions) else total
        assert off % 64 == 0, name
        assert off <= end, name
        assert off + used <= end, f"{name}: {off + used - end} bytes past its region ({used} used, {end - off} there)"
    assert regions[-1][1] + regions[-1][2] <= total
    got = dict((r[0], r[2]) for r in regions)
    assert got["records"] >= n_groups * 104
    for name, per in (("r2_order", 4), ("r2_p", 4), ("r2_off", 8), ("r2_group", 4), ("rperm", 4), ("cand_score", 4)):
        assert got[name] >= n_groups * per, name
    assert got["r2_tr"] >= (n_groups + 1) * 8              # the walk reads a (zero) transcript offset for every slot, launch_ext_begin clears them
    # the record order of the walked list is sorted in the arrays of the ranking order: 64-bit keys twice, 32-bit values
    assert got["okeys"] >= walk_cap * 8 and got["okeys_sorted"] >= walk_cap * 8 and got["oidx"] >= walk_cap * 4
    assert got["items"] >= item_cap * 32 and got["ends"] >= item_cap * 32 and got["hsps"] >= item_cap * 56
    assert got["cnt"] >= (n_groups + 1) * 4 and got["kept"] >= (n_groups + 1) * 4 and got["kept_pos"] >= (n_groups + 1) * 4
    assert (got["fverdict"] >= n_groups) if filters else (got["fverdict"] == 0)
    assert got["ctr"] > 0


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_layout_without_top_has_no_top_arrays(shape):
    n_groups, n_queries, n_bands, k = SHAPES[shape]
    regions, total, r2_cap, item_cap = layout(n_groups, n_queries, n_bands, k)
    got = dict((r[0], r[2]) for r in regions)
    assert got["cand_score"] == got["rperm"] == 0
    assert r2_cap == min(n_groups, n_queries * k)
    _, total_top, _, _, _ = layout_top(n_groups, n_queries, n_bands, k)
    assert total_top >= total


def test_k1_records_are_bounded_by_the_groups_not_by_k():
    """-k 1 with 100 groups per query: the -k layout holds one record per query, the --top layout one per group."""
    _, _, r2_k, _ = layout(3000, 30, 30_000, 1)
    regions, _, r2_top, _, walk = layout_top(3000, 30, 30_000, 1)
    assert r2_k == 30 and r2_top == walk == 3000
    assert dict((r[0], r[2]) for r in regions)["r2_tr"] == 3001 * 8
