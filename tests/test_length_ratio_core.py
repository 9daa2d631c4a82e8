"""CPU checks of the mutual-coverage search's arithmetic (diamond_amd/csrc/length_ratio_core.h) through tests/emu/libswipe_emu.so
(tests/emu/length_ratio_emu.cpp):
 * length_window -- the contiguous index range of a descending length list that passes against one length -- against the pairwise
   predicate, brute force, on random lists with long runs of ties, single sequences and empty windows;
 * mutual_cover_ratio against the literals the reference's expression yields in double (run/config.cpp:156-165);
 * length_sort_order against sorted(key=(length, index), reverse=True);
 * the seed stage's data flow with the length test (pair filter + batch count of the deferred pass) against the reference's hits
   tapped with --min-len-ratio 0.75 (tests/golden/ext_mutual_*.tap, minted by tests/golden/make_mutual_golden.sh): the default
   sensitivity's golden holds deferred pairs whose batch loses a mate to the length test, and counting batch mates without the test
   gives other hits there."""
import ctypes
import os

import numpy as np
import pytest

import emu_py as emu
import mutual_sets
from tapfile import read_ext_tap
from test_oracle_seed import blosum62_matrix8, hit_multiset

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RATIOS = [0.45, 0.5499999999999999, 0.75, 0.95, 1.0, 1e-9]


def _lib():
    lib = emu.lib()
    i64, d, v = ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    lib.emu_length_ratio_passes.restype = ctypes.c_int
    lib.emu_length_ratio_passes.argtypes = [i64, i64, d]
    lib.emu_mutual_cover_ratio.restype = d
    lib.emu_mutual_cover_ratio.argtypes = [d, d, d]
    lib.emu_length_sort_order.restype = None
    lib.emu_length_sort_order.argtypes = [v, i64, v]
    lib.emu_length_window.restype = None
    lib.emu_length_window.argtypes = [v, i64, i64, d, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.emu_query_window.restype = None
    lib.emu_query_window.argtypes = [v, i64, i64, d, v]
    lib.emu_mutual_seed_search.restype = i64
    lib.emu_mutual_seed_search.argtypes = [v, v, v, v, i64, v, v, i64, d, v, i64, v]
    return lib


def length_window(lengths, length, mlr):
    a = np.ascontiguousarray(lengths, np.int64)
    first, end = ctypes.c_int64(-1), ctypes.c_int64(-1)
    _lib().emu_length_window(a.ctypes.data, len(a), int(length), mlr, ctypes.byref(first), ctypes.byref(end))
    return first.value, end.value


def query_window(qlimits, tlen, mlr):
    ql = np.ascontiguousarray(qlimits, np.int64)
    out = np.zeros(2, np.uint32)
    _lib().emu_query_window(ql.ctypes.data, len(ql) - 1, int(tlen), mlr, out.ctypes.data)
    return int(out[0]), int(out[1])


def mutual_seed_search(c, matrix8, qd, ql, td, tl, mlr, cap=1 << 21):
    qd, td = np.ascontiguousarray(qd, np.int8), np.ascontiguousarray(td, np.int8)
    ql, tl = np.ascontiguousarray(ql, np.int64), np.ascontiguousarray(tl, np.int64)
    m = np.ascontiguousarray(matrix8, np.int8)
    hits = np.zeros(cap, emu.HIT_DTYPE)
    stats = np.zeros(5, np.int64)
    n = _lib().emu_mutual_seed_search(ctypes.addressof(c), m.ctypes.data, qd.ctypes.data, ql.ctypes.data, len(ql) - 1, td.ctypes.data, tl.ctypes.data, len(tl) - 1,
                                      float(mlr), hits.ctypes.data, cap, stats.ctypes.data)
    assert n >= 0
    return hits[:n].copy(), dict(zip(("length_removed", "deferred", "batch_differs", "saturation_differs", "hamming_pairs"), stats.tolist()))


def test_python_and_core_predicate_agree():
    lib = _lib()
    rng = np.random.default_rng(3)
    for mlr in RATIOS:
        for a, b in rng.integers(1, 2000, (2000, 2)).tolist() + [[90, 120], [120, 90], [3, 4], [55, 100], [100, 55], [1, 1]]:
            assert bool(lib.emu_length_ratio_passes(a, b, mlr)) == mutual_sets.passes(a, b, mlr)
    assert mutual_sets.passes(90, 120, 0.75) and not mutual_sets.passes(89, 120, 0.75)


@pytest.mark.parametrize("mlr", RATIOS)
def test_length_window_equals_the_pairwise_predicate(mlr):
    rng = np.random.default_rng(int(mlr * 1000) + 7)
    lists = [np.array([300]), np.array([7, 7, 7, 7, 7, 7]), np.array([], np.int64)]
    for _ in range(60):
        n = int(rng.integers(1, 120))
        few = rng.integers(20, 900, int(rng.integers(1, 8)))              # few distinct values: long runs of ties
        lists.append(np.sort(rng.choice(few, n))[::-1])
        lists.append(np.sort(rng.integers(20, 900, n))[::-1])
    empty = 0
    for lens in lists:
        probes = set(lens.tolist()) | {1, 19, 20, 450, 901, 5000} | set(rng.integers(1, 2500, 12).tolist())
        for length in probes:
            first, end = length_window(lens, length, mlr)
            want = [mutual_sets.passes(length, int(l), mlr) for l in lens]
            assert [first <= i < end for i in range(len(lens))] == want, (lens, length, mlr)
            empty += first == end
    assert empty > 0 or mlr < 1e-6                                        # empty windows occurred


def test_length_window_of_no_length_is_empty():
    assert length_window([5, 4, 3], 0, 0.75) == (0, 0)


def test_query_windows_are_position_ranges_of_the_passing_queries():
    db, doff, q, qoff = mutual_sets.generate(families=12, members=3, queries=3, seed=5)
    qd, ql, td, tl = mutual_sets.sorted_blocks(db, doff, q, qoff)
    qlen = np.diff(ql) - 1
    for tlen in sorted(set((np.diff(tl) - 1).tolist())) + [1, 10000]:
        first, end = query_window(ql, tlen, 0.75)
        ok = [i for i in range(len(qlen)) if mutual_sets.passes(int(qlen[i]), tlen, 0.75)]
        assert (first, end) == ((int(ql[ok[0]] - ql[0]), int(ql[ok[-1] + 1] - ql[0])) if ok else (0, 0))


def test_mutual_cover_ratio_literals():
    f = _lib().emu_mutual_cover_ratio
    want = {50: 0.45, 60: 0.5499999999999999, 70: 0.6499999999999999, 75: 0.7, 80: 0.75, 85: 0.7999999999999999, 90: 0.85, 95: 0.8999999999999999, 100: 0.95}
    for cover, ratio in want.items():
        assert f(cover, cover, 0.0) == ratio == max(cover / 100 - 0.05, 0.0), cover
    assert f(49.9, 49.9, 0.0) == 0.0
    assert f(80, 70, 0.0) == 0.0 and f(70, 80, 0.0) == 0.0 and f(0, 0, 0.0) == 0.0
    assert f(80, 80, 0.3) == 0.3 and f(80, 70, 0.9) == 0.9 and f(0, 0, 0.6) == 0.6


def test_length_sort_order_is_length_then_index_descending():
    rng = np.random.default_rng(11)
    for n in (0, 1, 2, 17, 400):
        lens = rng.choice(rng.integers(1, 300, 9), n) if n else np.zeros(0, np.int64)          # many ties
        limits = 256 + np.concatenate([[0], np.cumsum(lens + 1)]).astype(np.int64)
        order = np.full(n, -1, np.int64)
        _lib().emu_length_sort_order(limits.ctypes.data, n, order.ctypes.data)
        assert order.tolist() == sorted(range(n), key=lambda i: (int(lens[i]), i), reverse=True)
        if n:
            assert order.tolist() == mutual_sets.length_sorted(np.zeros(int(lens.sum()), np.int8), np.concatenate([[0], np.cumsum(lens)]))[2].tolist()
    ties = np.array([5, 9, 5, 9, 5])
    limits = np.concatenate([[0], np.cumsum(ties + 1)]).astype(np.int64)
    order = np.zeros(5, np.int64)
    _lib().emu_length_sort_order(limits.ctypes.data, 5, order.ctypes.data)
    assert order.tolist() == [3, 1, 4, 2, 0]                           # not the stable order [1, 3, 0, 2, 4]


def removed_share(cfg, recs, c):
    """Share of the ratio-off run's hits that the length test removes, for the condition every input of these tests must meet."""
    ref = np.concatenate([r["hits"] for r in recs])
    off, _ = mutual_seed_search(c, blosum62_matrix8(), cfg["query"]["data"], cfg["query"]["limits"], cfg["target"]["data"], cfg["target"]["limits"], 0.0)
    return 1.0 - len(ref) / len(off)


@pytest.mark.parametrize("tap", ["ext_mutual_fast.tap", "ext_mutual_default.tap", "ext_mutual_sensitive.tap"])
def test_emulated_hits_with_the_length_test_equal_reference(tap):
    cfg, recs = read_ext_tap(os.path.join(GOLDEN, tap))
    ql, tl = cfg["query"]["limits"], cfg["target"]["limits"]
    assert (np.diff(np.diff(ql)) <= 0).all() and (np.diff(np.diff(tl)) <= 0).all()          # the tap's blocks arrive length-sorted
    assert (np.diff(np.diff(ql)) == 0).any() and (np.diff(np.diff(tl)) == 0).any()           # ... with ties
    c = emu.seed_params_from_tap(cfg)
    hits, stats = mutual_seed_search(c, blosum62_matrix8(), cfg["query"]["data"], ql, cfg["target"]["data"], tl, 0.75)
    ref = np.concatenate([r["hits"] for r in recs])
    assert len(hits) == len(ref) and hit_multiset(hits) == hit_multiset(ref)
    share = removed_share(cfg, recs, c)
    print("%s: %d hits, the length test removes %.1f %% of the ratio-off hits, %s" % (tap, len(ref), 100 * share, stats))
    assert 0.2 <= share <= 0.8
    assert stats["length_removed"] > 0


def test_deferred_batches_lose_mates_to_the_length_test():
    """The default-sensitivity golden holds deferred pairs (window score above 255) whose SIMD batch loses a mate to the length
    test, some with another saturation decision for it; counting every Hamming survivor as a mate gives other hits than the reference's."""
    cfg, recs = read_ext_tap(os.path.join(GOLDEN, "ext_mutual_default.tap"))
    c = emu.seed_params_from_tap(cfg)
    args = (blosum62_matrix8(), cfg["query"]["data"], cfg["query"]["limits"], cfg["target"]["data"], cfg["target"]["limits"])
    hits, stats = mutual_seed_search(c, *args, 0.75)
    assert stats["deferred"] > 0 and stats["batch_differs"] >= 1 and stats["saturation_differs"] >= 1, stats
    ref = np.concatenate([r["hits"] for r in recs])
    assert (ref["score"] == 255).any() and (ref["score"] > 255).any()
    # the pair filter alone (ratio-off search, hits filtered by the predicate afterwards) is not the reference's answer here
    off, _ = mutual_seed_search(c, *args, 0.0)
    qlen, tlen = np.diff(cfg["query"]["limits"]) - 1, np.diff(cfg["target"]["limits"]) - 1
    t_of = np.searchsorted(cfg["target"]["limits"], off["subject"], side="right") - 1
    keep = np.array([mutual_sets.passes(int(qlen[h["query"]]), int(tlen[t]), 0.75) for h, t in zip(off, t_of)], bool)
    assert hit_multiset(off[keep]) != hit_multiset(ref)
