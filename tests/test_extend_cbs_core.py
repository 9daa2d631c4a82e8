"""CPU checks of the index arithmetic of the matrix adjustment inside the device half of the extension stage
(diamond_amd/csrc/extend_cbs_core.h, via tests/emu/libswipe_emu.so: tests/emu/extend_cbs_emu.cpp): the layout of the step's work
arrays, the matrix code of an item and what the sweep kernels read back of it, the launch class of an item with a matrix of its
own, and the slots and matrix numbers of an iteration's pairs against the host's bookkeeping (cbs_slots_assign, cbs_core.h)."""
import ctypes

import numpy as np
import pytest

import emu_py as emu
from test_extend_layout import SHAPES

MAX_REGIONS = 32
u64, i64 = ctypes.c_uint64, ctypes.c_int64
RULE_NONE, RULE_SCALE_OLD, RULE_REL_ENTROPY = -1, 0, 4
ST_DEVICE, ST_ROUNDING, ST_ITERATIONS, ST_RULE = 0, 1, 2, 3
WITH_BIAS = 1 << 40          # DMND_CBS_MATRIX_WITH_BIAS (include/diamond_hip.h): only the full-matrix sweeps of the host path set it


def constants():
    out = (ctypes.c_int * 6)()
    emu.lib().emu_ext_cbs_constants(out)
    return dict(own_class=out[0], all_classes=out[1], unset=out[2], standard=out[3], class_indices=out[4], counters_bytes=out[5])


def layout(n_groups, n_queries):
    lib = emu.lib()
    names = (ctypes.c_char_p * MAX_REGIONS)()
    off, used = np.zeros(MAX_REGIONS, np.uint64), np.zeros(MAX_REGIONS, np.uint64)
    total = u64(0)
    lib.emu_ext_cbs_layout.argtypes = [u64, u64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(u64)]
    n = lib.emu_ext_cbs_layout(n_groups, n_queries, MAX_REGIONS, ctypes.cast(names, ctypes.c_void_p), off.ctypes.data, used.ctypes.data, ctypes.byref(total))
    assert 0 < n <= MAX_REGIONS
    return [(names[i].decode(), int(off[i]), int(used[i])) for i in range(n)], total.value


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_every_array_of_the_step_lies_inside_its_region(shape):
    n_groups, n_queries, _, _ = SHAPES[shape]
    regions, total = layout(n_groups, n_queries)
    names = [r[0] for r in regions]
    assert len(set(names)) == len(names)
    for i, (name, off, used) in enumerate(regions):
        end = regions[i + 1][1] if i + 1 < len(regions) else total
        assert off % 64 == 0, name
        assert off + used <= end, f"{name}: {off + used - end} bytes past its region ({used} used, {end - off} there)"
    got = dict((r[0], r[2]) for r in regions)
    # a group is listed as a pair once per call: the groups bound an iteration's pairs; the scan takes one entry more
    assert got["g_mat"] >= n_groups * 4 and got["g_row"] >= n_groups * 4
    assert got["comp"] >= n_queries * 20 * 8 and got["true_aa"] >= n_queries * 4
    assert got["flag"] >= (n_groups + 1) * 4 and got["pos"] >= (n_groups + 1) * 4
    for name, width in (("pair_group", 4), ("qidx", 4), ("toff", 8), ("tlen", 4), ("qoff", 8), ("qlen", 4), ("rule", 4), ("status", 1), ("keep", 1)):
        assert got[name] >= n_groups * width, name
    assert got["model"] > 400 * 8 + 1024 and got["cbs_ctr"] == constants()["counters_bytes"] >= 4 + 2 * 16 * 4


def code(mat, hauser, query_off):
    out = (i64 * 4)()
    lib = emu.lib()
    lib.emu_ext_matrix_code.argtypes = [ctypes.c_int32, ctypes.c_int, i64, ctypes.POINTER(i64)]
    lib.emu_ext_matrix_code(mat, hauser, query_off, out)
    return dict(code=out[0], own=bool(out[1]), number=out[2], biased=bool(out[3]))


@pytest.mark.parametrize("hauser", [0, 1])
def test_matrix_codes_round_trip(hauser):
    for mat in (0, 1, 2, 1023, 1024, 2**20 + 7, 2**31 - 1):
        for query_off in (0, 1, 12345, 2**33):
            c = code(mat, hauser, query_off)
            # a banded item of an adjusted target: its own matrix, read back as the same number, swept without the bias in every mode
            assert c["code"] == -2 - mat and c["own"] and c["number"] == mat and not c["biased"], (mat, query_off, c)
            assert (-2 - c["code"]) & WITH_BIAS == 0
    c = constants()
    for mat in (c["standard"], c["unset"]):          # no matrix: the bias row of the query where the mode has the Hauser bias, or none
        for query_off in (0, 77, 2**33):
            got = code(mat, hauser, query_off)
            assert not got["own"] and got["number"] == -1
            assert got["code"] == (query_off if hauser else -1) and got["biased"] == bool(hauser)


def item_class(rows, own, band, steps):
    out = (ctypes.c_int * 4)()
    lib = emu.lib()
    lib.emu_ext_item_class.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, i64, ctypes.POINTER(ctypes.c_int)]
    lib.emu_ext_item_class(rows, own, band, steps, out)
    return dict(P=out[0], slot=out[1], row=bool(out[2]), k16=bool(out[3]))


def test_an_own_matrix_item_never_takes_a_row_class_or_a_packed_launch():
    c = constants()
    assert c["own_class"] == 16 and c["all_classes"] == 32 and c["class_indices"] <= c["own_class"]
    seen_rows = 0
    for band in range(1, 4097):
        for steps in (1, 500, 2 * 65535, 2 * 65535 + 1, 10**6):
            for rows in (0, 1):
                own = item_class(rows, 1, band, steps)
                std = item_class(rows, 0, band, steps)
                # its band class: a power of two wide enough for the band, counted in a class of its own above the standard ones
                P = own["P"]
                assert P & (P - 1) == 0 and 128 * P >= band and (P == 1 or 64 * P < band), (band, own)
                assert not own["row"] and not own["k16"], (band, steps, rows, own)
                assert c["own_class"] <= own["slot"] < c["all_classes"] and own["slot"] - c["own_class"] == P.bit_length() - 1
                # the standard item beside it: below the own-matrix classes, a row class only with rows on and inside the packed kernels' reach
                assert 0 <= std["slot"] < c["class_indices"]
                if std["row"]:
                    assert rows and std["k16"] and band <= 160 and steps <= 2 * 65535
                    seen_rows += 1
                else:
                    assert std["P"] == P
    assert seen_rows > 100


def pair_matrices(before, rule, status, keep):
    n = len(rule)
    rule, status, keep = np.asarray(rule, np.int32), np.asarray(status, np.uint8), np.asarray(keep, np.uint8)
    slot, handed, by_status = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64), np.zeros(4, np.int64)
    g_mat, mat_host = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    lib = emu.lib()
    lib.emu_ext_pair_matrices.restype = i64
    lib.emu_ext_pair_matrices.argtypes = [i64, i64] + [ctypes.c_void_p] * 8
    # (n = 0: no array is touched; numpy hands out a valid pointer all the same)
    rule, status, keep = (np.concatenate([a, np.zeros(1, a.dtype)]) for a in (rule, status, keep))
    h = lib.emu_ext_pair_matrices(before, n, rule.ctypes.data, status.ctypes.data, keep.ctypes.data,
                                  slot.ctypes.data, g_mat.ctypes.data, mat_host.ctypes.data, handed.ctypes.data, by_status.ctypes.data)
    return slot[:n], g_mat[:n], mat_host[:n], handed[:h], by_status


PAIR_CASES = {
    "none": ([], [], []),
    "one_adjusted": ([RULE_REL_ENTROPY], [ST_DEVICE], [1]),
    "one_standard": ([RULE_NONE], [ST_DEVICE], [1]),
    "one_handed_back_without_a_table": ([RULE_REL_ENTROPY], [ST_RULE], [0]),
    "all_none": ([RULE_NONE] * 7, [ST_DEVICE] * 7, [1] * 7),
    "all_handed_back": ([RULE_REL_ENTROPY, RULE_SCALE_OLD, RULE_NONE, RULE_REL_ENTROPY, RULE_SCALE_OLD, RULE_REL_ENTROPY],
                        [ST_ROUNDING, ST_RULE, ST_RULE, ST_ITERATIONS, ST_RULE, 200], [1, 1, 0, 1, 0, 1]),
    "alternating": ([RULE_REL_ENTROPY, RULE_NONE] * 40, [ST_DEVICE, ST_DEVICE, ST_ITERATIONS, ST_RULE] * 20, [1, 1, 1, 0] * 20),
    "mixed": ([RULE_REL_ENTROPY, RULE_REL_ENTROPY, RULE_NONE, RULE_SCALE_OLD, RULE_NONE, RULE_REL_ENTROPY, RULE_SCALE_OLD],
              [ST_DEVICE, ST_ROUNDING, ST_DEVICE, ST_RULE, ST_RULE, ST_DEVICE, ST_RULE], [0, 1, 0, 1, 0, 1, 0]),
}


@pytest.mark.parametrize("case", list(PAIR_CASES), ids=list(PAIR_CASES))
@pytest.mark.parametrize("before", [0, 1, 128, 2**31 - 200])
def test_slots_and_matrix_numbers_equal_the_hosts_bookkeeping(case, before):
    rule, status, keep = PAIR_CASES[case]
    slot, g_mat, mat_host, handed, by_status = pair_matrices(before, rule, status, keep)
    n = len(rule)
    assert list(slot) == [before + k for k in range(n)]
    # the matrix number of every pair's group is the one extend_range ends up with (cbs_slots_assign, then -1 for a handed-back pair
    # whose host rule is NONE), and never the `unset` mark: a listed group is not listed again
    assert list(g_mat) == list(mat_host)
    assert all(m == -1 or m == before + k for k, m in enumerate(g_mat))
    assert list(handed) == [k for k in range(n) if status[k] != ST_DEVICE] and int(by_status.sum()) == n
    for k in range(n):
        if status[k] == ST_DEVICE:
            assert (g_mat[k] == -1) == (rule[k] == RULE_NONE)
        else:
            assert (g_mat[k] == -1) == (keep[k] == 0)
