"""CPU checks of the work-array layout of the device half of the extension stage (diamond_amd/csrc/extend_core.h ext_layout and
ext_regions, via tests/emu/libswipe_emu.so): over a grid of shapes, what the kernels index and what the launchers clear (the
transcript offsets of the round-2 list, the counters) lies inside each array's region, and the last region ends inside the buffer.
extend_on_device allocates exactly ext_layout's size, so a clear sized by another count -- the bands instead of the round-2
capacity, as launch_ext_begin once did -- runs into the arrays behind it or past the allocation."""
import ctypes

import numpy as np
import pytest

import emu_py as emu

MAX_REGIONS = 64


def layout(n_groups, n_queries, n_bands, k):
    lib = emu.lib()
    u64 = ctypes.c_uint64
    names = (ctypes.c_char_p * MAX_REGIONS)()
    off, used = np.zeros(MAX_REGIONS, np.uint64), np.zeros(MAX_REGIONS, np.uint64)
    total, r2_cap, item_cap = u64(0), u64(0), u64(0)
    lib.emu_ext_layout.argtypes = [u64, u64, u64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    n = lib.emu_ext_layout(n_groups, n_queries, n_bands, k, MAX_REGIONS, ctypes.cast(names, ctypes.c_void_p), off.ctypes.data, used.ctypes.data,
                           ctypes.byref(total), ctypes.byref(r2_cap), ctypes.byref(item_cap))
    assert 0 < n <= MAX_REGIONS
    regions = [(names[i].decode(), int(off[i]), int(used[i])) for i in range(n)]
    return regions, total.value, r2_cap.value, item_cap.value


# (groups, queries, bands, -k)
SHAPES = {
    "k1_10000_bands_per_query": (3000, 30, 300_000, 1),          # bands >> round-2 capacity (-k 1: 30 records, 10 000 bands per query)
    "k1_k1_test_block": (18_000, 300, 18_000, 1),                  # the -k 1 case of tests/test_gpu_extend_device.py, about
    "queries_times_k_above_groups": (500, 1000, 800, 25),          # most queries have fewer targets than -k
    "k_above_the_chunk": (5000, 10, 6000, 200),                    # -k 200 (ranking chunk 224)
    "k_far_above_the_chunk": (5000, 10, 5000, 2000),
    "one_band_per_group": (100_000, 1000, 100_000, 25),
    "one_of_each": (1, 1, 1, 1),
    "c2_like": (200_000, 6700, 260_000, 25),
    "many_bands_per_group": (100, 100, 60_000, 25),
}


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_every_array_and_clear_lies_inside_its_region(shape):
    n_groups, n_queries, n_bands, k = SHAPES[shape]
    regions, total, r2_cap, item_cap = layout(n_groups, n_queries, n_bands, k)
    assert r2_cap == min(n_groups, n_queries * k)
    assert item_cap == n_bands + r2_cap
    names = [r[0] for r in regions]
    assert len(set(names)) == len(names)
    for i, (name, off, used) in enumerate(regions):
        end = regions[i + 1][1] if i + 1 < len(regions) else total
        assert off % 64 == 0, name
        assert off <= end, name
        assert off + used <= end, f"{name}: {off + used - end} bytes past its region ({used} used, {end - off} there)"
    assert regions[-1][1] + regions[-1][2] <= total
    got = dict((r[0], r[2]) for r in regions)
    # what the kernels need at the least: the traceback reads a transcript offset for every round-2 slot (up to the capacity), the
    # per-item arrays hold every band and a copy of every survivor, the group arrays one entry more for the scans
    assert got["r2_tr"] >= r2_cap * 8
    assert got["records"] >= r2_cap * 104
    assert got["items"] >= item_cap * 32 and got["ends"] >= item_cap * 32
    assert got["cnt"] >= (n_groups + 1) * 4 and got["kept_pos"] >= (n_groups + 1) * 4
    assert got["ctr"] > 0


def test_the_layout_grows_with_the_bands_but_the_round2_clear_does_not():
    """-k 1: ten times the bands per query leaves the round-2 list and its clear where they were."""
    a, _, r2a, _ = layout(3000, 30, 30_000, 1)
    b, _, r2b, _ = layout(3000, 30, 300_000, 1)
    assert r2a == r2b == 30
    assert dict((r[0], r[2]) for r in a)["r2_tr"] == dict((r[0], r[2]) for r in b)["r2_tr"] == 31 * 8
