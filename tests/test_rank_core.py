"""CPU checks of diamond_amd/csrc/rank_core.h, via tests/emu/libswipe_emu.so: the arithmetic of the device form of the global ranking
step (--global-ranking; dmnd_rank_targets_device).
 * The walk rule on hand-made segment lists against a literal transcription of the host loop of dmnd_rank_targets: hits in
   (diagonal, j) order, a hit skipped when the segment computed LAST lies on its diagonal and reaches its j (the frame plays no part),
   a strictly higher score replaces score and context. The emulator runs the form the kernels run: one binary-search walk per run of
   equal diagonal, a maximum over the packed (score, reversed position) of the runs, taken in either order.
 * The sort key (group, diagonal biased by 2^31) round-trips and orders like the pair for every diagonal an int32 can hold.
 * The cut lemma without a device: feeding dmnd_rank_update each block's first N records per query gives the table that all records
   give.
"""
import ctypes

import numpy as np
import pytest

import emu_py as emu
from diamond_amd import hip


def _lib():
    lib = emu.lib()
    p, i32, u32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64
    lib.emu_rank_walk_group.restype, lib.emu_rank_walk_group.argtypes = None, [ctypes.c_int, p, p, p, p, p, p, ctypes.c_int, p]
    lib.emu_rank_key.restype, lib.emu_rank_key.argtypes = u64, [u32, i32]
    lib.emu_rank_key_group.restype, lib.emu_rank_key_group.argtypes = u32, [u64]
    lib.emu_rank_key_diag.restype, lib.emu_rank_key_diag.argtypes = i32, [u64]
    lib.emu_rank_skips.restype, lib.emu_rank_skips.argtypes = ctypes.c_int, [i32, i32, i32, i32]
    lib.emu_rank_cut_key.restype, lib.emu_rank_cut_key.argtypes = u64, [u32, ctypes.c_uint16]
    lib.emu_rank_xdrop.restype, lib.emu_rank_xdrop.argtypes = ctypes.c_int, [ctypes.c_double, ctypes.c_double]
    return lib


def host_walk(hits):
    """dmnd_rank_targets' loop over one group, literally. hits: (i, j, frame, left, right, score) in load order (frame ascending);
    Python's sort is stable, so hits with equal (diagonal, j) stay frame ascending: the device rule, where the host's unstable sort
    decides nothing. Returns (uint16 score, context, computed hits)."""
    seg = lambda h: (h[0] - h[3], h[1] - h[3], h[3] + h[4], h[5])          # DiagonalSegment(i - left, j - left, left + right, score)
    diag = lambda d: d[0] - d[1]
    j_end = lambda d: d[1] + d[2]
    sh = sorted(hits, key=lambda h: (h[0] - h[1], h[1]))
    d = seg(sh[0])
    score, context, computed = d[3], sh[0][2], 1
    for x in sh[1:]:
        if diag(d) == x[0] - x[1] and j_end(d) >= x[1]:
            continue
        d = seg(x)
        computed += 1
        if d[3] > score:
            score, context = d[3], x[2]
    return score & 0xffff, context, computed


def emu_walk(lib, hits, reverse):
    a = np.array(hits, dtype=np.int32).reshape(-1, 6)
    cols = [np.ascontiguousarray(a[:, k]) for k in range(6)]
    out = np.zeros(4, dtype=np.int64)
    lib.emu_rank_walk_group(len(a), *[c.ctypes.data for c in cols], int(reverse), out.ctypes.data)
    return int(out[0]), int(out[1]), int(out[2])


CASES = {
    # one diagonal; the first segment reaches every later hit
    "all_covered": [(10, 10, 0, 10, 90, 50), (20, 20, 0, 20, 80, 50), (60, 60, 0, 60, 40, 50), (100, 100, 0, 100, 0, 50)],
    # the second computed segment ends before the third hit: that one is computed again, and scores highest
    "second_ends_early": [(5, 5, 0, 5, 10, 30), (20, 20, 0, 12, 3, 30), (40, 40, 0, 3, 8, 31), (45, 45, 0, 8, 3, 31), (60, 60, 0, 2, 9, 44)],
    # the same diagonal in two frames: frame 0's segment covers frame 1's hit whose own walk would score higher; the frame is not compared
    "frames_share_diagonal": [(10, 30, 0, 4, 40, 25), (30, 50, 1, 6, 30, 90), (80, 100, 1, 5, 5, 26)],
    # equal (diagonal, j) in two frames: frame ascending (the device rule)
    "frames_equal_position": [(10, 30, 0, 4, 2, 25), (10, 30, 1, 4, 2, 40), (50, 70, 2, 1, 1, 41)],
    # the same best score on two diagonals: the smaller diagonal is walked first, its context stays (strict >)
    "equal_best_two_diagonals": [(50, 10, 3, 5, 5, 77), (10, 50, 1, 5, 5, 77), (30, 30, 2, 5, 5, 60)],
    "single_hit": [(7, 1234, 4, 7, 0, 13)],
    # scores through the uint16 cast
    "score_65535": [(3, 3, 0, 3, 9000, 65535), (3, 900, 0, 3, 5, 100)],
    "score_65536": [(3, 3, 0, 3, 9000, 65536), (3, 900, 1, 3, 5, 100)],
    "score_66000": [(3, 3, 2, 3, 9000, 66000), (3, 900, 1, 3, 5, 65535)],
    # negative and positive diagonals far apart, a long target
    "far_diagonals": [(5, 69990, 0, 5, 9, 33), (2999, 3, 0, 3, 0, 33), (0, 0, 0, 0, 1, 4)],
    "zero_scores": [(4, 9, 2, 0, 0, 0), (4, 2, 1, 0, 0, 0)],
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_walk_rule_matches_the_host_loop(name):
    lib = _lib()
    hits = CASES[name]
    want = host_walk(hits)
    assert emu_walk(lib, hits, 0) == want
    assert emu_walk(lib, hits, 1) == want          # the order in which the runs are reduced changes nothing


def test_walk_rule_cases_do_what_their_names_say():
    assert host_walk(CASES["all_covered"]) == (50, 0, 1)
    assert host_walk(CASES["second_ends_early"]) == (44, 0, 4)
    assert host_walk(CASES["frames_share_diagonal"]) == (26, 1, 2)          # not 90: that hit is covered by frame 0's segment
    assert host_walk(CASES["frames_equal_position"]) == (41, 2, 2)
    assert host_walk(CASES["equal_best_two_diagonals"]) == (77, 1, 3)       # diagonal -40 (context 1) before +40 (context 3)
    assert host_walk(CASES["single_hit"]) == (13, 4, 1)
    assert host_walk(CASES["score_65535"]) == (65535, 0, 2)
    assert host_walk(CASES["score_65536"]) == (0, 0, 2)
    assert host_walk(CASES["score_66000"]) == (66000 - 65536, 2, 2)
    assert host_walk(CASES["zero_scores"]) == (0, 2, 2)                      # all scores 0: the first hit in walk order keeps the context


def test_walk_rule_random_groups():
    lib = _lib()
    rng = np.random.default_rng(20261019)
    for _ in range(300):
        n = int(rng.integers(1, 60))
        n_diag = int(rng.integers(1, 5))
        hits = []
        for _k in range(n):
            j = int(rng.integers(0, 200))
            d = int(rng.integers(0, n_diag)) * 7 - 10
            i = j + d
            left = int(rng.integers(0, 12))
            right = int(rng.integers(0, 40))
            hits.append((i, j, int(rng.integers(0, 6)), left, right, int(rng.integers(0, 50))))
        # no ties in (diagonal, j) across frames: there the host's order is not determined; load order is frame ascending
        seen, uniq = set(), []
        for h in sorted(hits, key=lambda h: h[2]):
            if (h[0] - h[1], h[1]) not in seen:
                seen.add((h[0] - h[1], h[1]))
                uniq.append(h)
        want = host_walk(uniq)
        assert emu_walk(lib, uniq, 0) == want and emu_walk(lib, uniq, 1) == want


def test_skip_rule_reads_the_diagonal_only():
    lib = _lib()
    assert lib.emu_rank_skips(5, 100, 5, 100) == 1 and lib.emu_rank_skips(5, 100, 5, 101) == 0
    assert lib.emu_rank_skips(5, 100, 6, 50) == 0 and lib.emu_rank_skips(-5, 100, -5, 0) == 1


def test_key_packing_round_trips_and_orders():
    lib = _lib()
    top = 2 ** 31 - 2
    diags = [-top, -top + 1, -70000, -65536, -65535, -1, 0, 1, 65535, 65536, 70000, top - 1, top]
    groups = [0, 1, 65535, 65536, 2 ** 32 - 2]
    pairs = [(g, d) for g in groups for d in diags]
    keys = [int(lib.emu_rank_key(g, d)) for g, d in pairs]
    for (g, d), k in zip(pairs, keys):
        assert (int(lib.emu_rank_key_group(k)), int(lib.emu_rank_key_diag(k))) == (g, d)
    assert keys == sorted(keys) and len(set(keys)) == len(keys)      # pairs were listed in (group, diagonal) order
    rng = np.random.default_rng(5)
    rnd = [(int(g), int(d)) for g, d in zip(rng.integers(0, 2 ** 32 - 1, 2000), rng.integers(-top, top + 1, 2000))]
    assert sorted(rnd) == [p for _, p in sorted((int(lib.emu_rank_key(g, d)), (g, d)) for g, d in rnd)]


def test_cut_key_orders_by_query_then_score_descending():
    lib = _lib()
    recs = [(q, s) for q in (0, 1, 70000) for s in (65535, 65534, 300, 1, 0)]
    keys = [int(lib.emu_rank_cut_key(q, s)) for q, s in recs]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_xdrop_value_is_the_reference_default():
    # BLOSUM62 11/1: lambda 0.267, K 0.041 -> ceil((12.3 ln 2 + ln K) / lambda) = 20
    assert _lib().emu_rank_xdrop(0.041, 0.267) == 20


@pytest.mark.parametrize("n", [1, 3, 8])
def test_cut_is_lossless_for_rank_update(n):
    """3 blocks x 50 queries, many equal scores: the table from each block's first n records per query in (score descending, target
    ascending) order equals the table from every record."""
    rng = np.random.default_rng(100 + n)
    n_queries, per_block = 50, 40
    full = np.zeros(n_queries * n, hip.RANKED_DTYPE)
    cut = np.zeros(n_queries * n, hip.RANKED_DTYPE)
    for b in range(3):
        rows = []
        for q in range(n_queries):
            k = int(rng.integers(0, 30))
            targets = np.sort(rng.choice(per_block, size=k, replace=False)) + b * per_block      # every target once per query, in its own block only
            for t in targets:
                rows.append((q, int(t), int(rng.integers(1, 6)), int(rng.integers(0, 6)), 0))
        recs = np.array(rows, hip.RANKED_DTYPE)
        hip.rank_update(full, n, recs)
        order = np.lexsort((recs["target"], 65535 - recs["score"].astype(np.int64), recs["query"]))
        s = recs[order]
        first = np.searchsorted(s["query"], s["query"], side="left")
        kept = s[np.arange(len(s)) - first < n]
        assert len(kept) < len(recs)
        hip.rank_update(cut, n, kept)
    assert full.tobytes() == cut.tobytes()
    assert (full["score"] > 0).any()
