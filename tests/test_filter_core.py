"""CPU checks of the HSP filter arithmetic (diamond_amd/csrc/filter_core.h: what the host path, the device filter kernel and the
approx_pident column compute) and of the device half's work-array layout under filters (extend_core.h ext_layout(.., filters)),
via tests/emu/libswipe_emu.so.
 * approx_id against tests/golden/approx_id_ref.tsv: score, coordinates, identities, length and approx_pident as the reference binary
   printed them (-f 6 score qstart qend sstart send nident length approx_pident; the last ten rows are self hits, where the value is
   100 whatever the score). The column is printed with one decimal, so the recomputed value may differ by half a unit of it.
 * the Hamming identities an --approx-id threshold asks of the seed stage: 0 below 50, 20 from 50, 30 from 90.
 * the filter verdict on hand-made HSPs, with the value on a threshold marked as undecided.
 * the layout over the grid of tests/test_extend_layout.py: every array inside its region, the walked list and the item arrays sized
   for every group (the statistics exist for every target of a chunk BEFORE the -k culling), the unfiltered layout unchanged."""
import ctypes
import os

import numpy as np
import pytest

import emu_py as emu
from test_extend_layout import SHAPES, MAX_REGIONS, layout

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _lib():
    lib = emu.lib()
    lib.emu_hsp_approx_id.restype = ctypes.c_double
    lib.emu_hsp_approx_id.argtypes = [ctypes.c_int] * 5
    lib.emu_approx_id.restype = ctypes.c_double
    lib.emu_approx_id.argtypes = [ctypes.c_int] * 3
    lib.emu_hamming_id_cutoff.restype = ctypes.c_uint
    lib.emu_hamming_id_cutoff.argtypes = [ctypes.c_double]
    lib.emu_filter_verdict.argtypes = [ctypes.c_double] * 4 + [ctypes.c_int] * 9
    return lib


def test_approx_id_equals_the_reference_column():
    lib = _lib()
    rows = [l.split("\t") for l in open(os.path.join(GOLDEN, "approx_id_ref.tsv")).read().splitlines()]
    assert len(rows) == 160
    n_identical = 0
    for score, qs, qe, ss, se, nident, length, printed in rows:
        got = lib.emu_hsp_approx_id(int(score), int(qe) - int(qs) + 1, int(se) - int(ss) + 1, int(nident), int(length))
        assert abs(got - float(printed)) <= 0.05 + 1e-9, (score, qs, qe, ss, se, printed, got)
        if nident == length:
            n_identical += 1
            assert got == 100.0
    assert n_identical >= 10
    # a score that would give less than 100 is still 100 for identical ranges, and the estimate is clamped to [0, 100]
    assert lib.emu_hsp_approx_id(100, 50, 50, 50, 50) == 100.0 and lib.emu_hsp_approx_id(100, 50, 50, 49, 50) < 100.0
    assert lib.emu_approx_id(10000, 10, 10) == 100.0 and lib.emu_approx_id(-500, 10, 300) == 0.0 and lib.emu_approx_id(7, 0, 0) == 100.0
    assert abs(lib.emu_approx_id(300, 100, 120) - (300 / 120 * 16.56 + 11.41)) < 1e-12      # (one fused multiply-add: a last-bit difference)


@pytest.mark.parametrize("approx_id,want", [(0.0, 0), (10.0, 0), (49.999, 0), (50.0, 20), (75.0, 20), (89.9, 20), (90.0, 30), (100.0, 30)])
def test_hamming_id_cutoff(approx_id, want):
    assert _lib().emu_hamming_id_cutoff(approx_id) == want


def test_filter_verdict():
    lib = _lib()
    # score 200, 60 identities over 100 columns, query 10..110 of 200, subject 0..90 of 120
    hsp = (200, 60, 100, 10, 110, 0, 90, 200, 120)
    assert lib.emu_filter_verdict(0, 0, 0, 0, *hsp) == 0
    assert lib.emu_filter_verdict(59.9, 0, 0, 0, *hsp) == 0 and lib.emu_filter_verdict(60.1, 0, 0, 0, *hsp) == 1
    assert lib.emu_filter_verdict(60.0, 0, 0, 0, *hsp) == 2                                      # on the threshold: not decided on the device
    assert lib.emu_filter_verdict(0, 0, 49.0, 0, *hsp) == 0 and lib.emu_filter_verdict(0, 0, 51.0, 0, *hsp) == 1      # query cover 50 %
    assert lib.emu_filter_verdict(0, 0, 0, 74.0, *hsp) == 0 and lib.emu_filter_verdict(0, 0, 0, 76.0, *hsp) == 1      # subject cover 75 %
    approx = lib.emu_approx_id(200, 100, 90)                                                   # 44.53
    assert 44 < approx < 45
    assert lib.emu_filter_verdict(0, 44.0, 0, 0, *hsp) == 0 and lib.emu_filter_verdict(0, 45.0, 0, 0, *hsp) == 1
    assert lib.emu_filter_verdict(0, approx, 0, 0, *hsp) == 2
    assert lib.emu_filter_verdict(59.0, 44.0, 49.0, 74.0, *hsp) == 0 and lib.emu_filter_verdict(59.0, 44.0, 49.0, 76.0, *hsp) == 1


def layout_filters(n_groups, n_queries, n_bands, k):
    lib = emu.lib()
    u64 = ctypes.c_uint64
    names = (ctypes.c_char_p * MAX_REGIONS)()
    off, used = np.zeros(MAX_REGIONS, np.uint64), np.zeros(MAX_REGIONS, np.uint64)
    total, r2_cap, item_cap, walk_cap = u64(0), u64(0), u64(0), u64(0)
    lib.emu_ext_layout_filters.argtypes = [u64, u64, u64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    n = lib.emu_ext_layout_filters(n_groups, n_queries, n_bands, k, MAX_REGIONS, ctypes.cast(names, ctypes.c_void_p), off.ctypes.data, used.ctypes.data,
                                   ctypes.byref(total), ctypes.byref(r2_cap), ctypes.byref(item_cap), ctypes.byref(walk_cap))
    assert 0 < n <= MAX_REGIONS
    return [(names[i].decode(), int(off[i]), int(used[i])) for i in range(n)], total.value, r2_cap.value, item_cap.value, walk_cap.value


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_filtered_layout_holds_the_statistics_of_every_group(shape):
    n_groups, n_queries, n_bands, k = SHAPES[shape]
    regions, total, r2_cap, item_cap, walk_cap = layout_filters(n_groups, n_queries, n_bands, k)
    assert r2_cap == min(n_groups, n_queries * k)          # records: still at most -k per query
    assert walk_cap == n_groups                            # walked before the culling: every group once, over all chunks
    assert item_cap == n_bands + n_groups                  # ... each with room for a copy swept again with traceback
    names = [r[0] for r in regions]
    assert len(set(names)) == len(names)
    for i, (name, off, used) in enumerate(regions):
        end = regions[i + 1][1] if i + 1 < len(regions) else total
        assert off % 64 == 0, name
        assert off + used <= end, f"{name}: {off + used - end} bytes past its region ({used} used, {end - off} there)"
    got = dict((r[0], r[2]) for r in regions)
    assert got["fverdict"] >= n_groups and got["matched"] >= n_groups
    assert got["q_matched"] >= n_queries * 4 and got["q_removed"] >= n_queries * 4
    for name, per in (("r2_order", 4), ("r2_p", 4), ("r2_off", 8), ("r2_group", 4)):
        assert got[name] >= walk_cap * per, name
    assert got["r2_tr"] >= (walk_cap + 1) * 8              # the walk reads a (zero) transcript offset for every slot
    assert got["records"] >= r2_cap * 104
    assert got["items"] >= item_cap * 32 and got["ends"] >= item_cap * 32 and got["hsps"] >= item_cap * 56


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_unfiltered_layout_has_no_filter_arrays_and_its_old_size(shape):
    n_groups, n_queries, n_bands, k = SHAPES[shape]
    regions, total, r2_cap, item_cap = layout(n_groups, n_queries, n_bands, k)
    got = dict((r[0], r[2]) for r in regions)
    assert got["fverdict"] == got["matched"] == got["q_matched"] == got["q_removed"] == 0
    assert item_cap == n_bands + r2_cap
    _, total_f, _, _, _ = layout_filters(n_groups, n_queries, n_bands, k)
    assert total_f >= total
