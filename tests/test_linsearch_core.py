"""CPU checks of the linearised search's rules (diamond_amd/csrc/linsearch_core.h) through tests/emu/libswipe_emu.so
(tests/emu/linsearch_emu.cpp):
 * the selection rule -- a joined record reaches the Hamming test iff its position is the smallest of its slot -- against brute
   force on random record lists with repeated slots, equal positions in different slots and shuffled arrival orders;
 * the scoring rule of a batch of one and the weight bound;
 * the seed stage's data flow with the rule (reduction, pair filter, no deferral, no left-most filter) against the reference's
   hits tapped with --linsearch (tests/golden/ext_lin_*.tap, minted by tests/golden/make_linsearch_golden.sh). Every golden meets
   the conditions the tests of the device code rely on: the rule drops at least 10 % of the joined reference positions, and the
   default sensitivity's golden holds hits with a window score above 255."""
import ctypes
import os

import numpy as np
import pytest

import emu_py as emu
from tapfile import read_ext_tap
from test_oracle_seed import blosum62_matrix8, hit_multiset

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAPS = ["ext_lin_fast.tap", "ext_lin_default.tap", "ext_lin_hashed.tap"]
STATS = ("joined", "selected", "hamming_pairs", "above_255", "dropped_though_passing", "left_most_would_drop")


def _lib():
    lib = emu.lib()
    i64, v = ctypes.c_int64, ctypes.c_void_p
    lib.emu_lin_select.restype = None
    lib.emu_lin_select.argtypes = [v, v, i64, i64, v]
    lib.emu_lin_score_is_deferred.restype = ctypes.c_int
    lib.emu_lin_score_is_deferred.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.emu_lin_applies_left_most.restype = ctypes.c_int
    lib.emu_lin_applies_left_most.argtypes = [ctypes.c_int]
    lib.emu_lin_shape_weight_ok.restype = ctypes.c_int
    lib.emu_lin_shape_weight_ok.argtypes = [ctypes.c_int]
    lib.emu_lin_seed_search.restype = i64
    lib.emu_lin_seed_search.argtypes = [v, v, v, v, i64, v, v, i64, v, i64, v]
    return lib


def lin_select(slot, position, n_slots):
    slot, position = np.ascontiguousarray(slot, np.uint32), np.ascontiguousarray(position, np.int64)
    out = np.zeros(len(slot), np.uint8)
    _lib().emu_lin_select(slot.ctypes.data, position.ctypes.data, len(slot), int(n_slots), out.ctypes.data)
    return out.astype(bool)


def lin_seed_search(c, matrix8, qd, ql, td, tl, cap=1 << 21):
    """The emulated linearised seed search: (hits, statistics)."""
    qd, td = np.ascontiguousarray(qd, np.int8), np.ascontiguousarray(td, np.int8)
    ql, tl = np.ascontiguousarray(ql, np.int64), np.ascontiguousarray(tl, np.int64)
    m = np.ascontiguousarray(matrix8, np.int8)
    hits = np.zeros(cap, emu.HIT_DTYPE)
    stats = np.zeros(6, np.int64)
    n = _lib().emu_lin_seed_search(ctypes.addressof(c), m.ctypes.data, qd.ctypes.data, ql.ctypes.data, len(ql) - 1, td.ctypes.data, tl.ctypes.data, len(tl) - 1,
                                   hits.ctypes.data, cap, stats.ctypes.data)
    assert n >= 0, n
    return hits[:n].copy(), dict(zip(STATS, stats.tolist()))


def test_selection_rule_equals_brute_force():
    rng = np.random.default_rng(5)
    some_dropped = 0
    for trial in range(200):
        n_slots = int(rng.integers(1, 40))
        n = int(rng.integers(0, 300))
        slot = rng.integers(0, n_slots, n)
        # few distinct positions: the same position in several slots; a (slot, position) pair occurs once, as in the joined lists
        position = rng.integers(256, 256 + int(rng.integers(2, 400)), n)
        _, keep = np.unique(slot * (1 << 20) + position, return_index=True)
        keep = rng.permutation(keep)
        slot, position = slot[keep], position[keep]
        got = lin_select(slot, position, n_slots)
        want = np.array([position[i] == position[slot == slot[i]].min() for i in range(len(slot))], bool)
        assert np.array_equal(got, want), trial
        # exactly one record per slot that occurs, whatever the arrival order
        assert got.sum() == len(set(slot.tolist()))
        perm = rng.permutation(len(slot))
        assert np.array_equal(lin_select(slot[perm], position[perm], n_slots), want[perm])
        some_dropped += int((~got).sum())
    assert some_dropped > 1000
    # positions beyond 2^31 and up to 2^40 (the sort key of the deferred pass allows that many)
    slot = np.array([0, 0, 1, 1, 0])
    position = np.array([(1 << 40) - 1, (1 << 31) + 5, 1 << 33, (1 << 33) - 1, (1 << 31) + 6])
    assert lin_select(slot, position, 2).tolist() == [False, True, False, True, False]


def test_scoring_rule_and_weight_bound():
    lib = _lib()
    for score in (0, 100, 255, 256, 1000, 0xFFFF):
        assert lib.emu_lin_score_is_deferred(score, 0) == (1 if score > 255 else 0)
        assert lib.emu_lin_score_is_deferred(score, 1) == 0
    assert lib.emu_lin_applies_left_most(0) == 1 and lib.emu_lin_applies_left_most(1) == 0
    assert [w for w in range(1, 20) if lib.emu_lin_shape_weight_ok(w)] == list(range(10, 20))


@pytest.mark.parametrize("tap", TAPS)
def test_emulated_linearised_hits_equal_reference(tap):
    cfg, recs = read_ext_tap(os.path.join(GOLDEN, tap))
    assert os.path.getsize(os.path.join(GOLDEN, tap)) <= os.path.getsize(os.path.join(GOLDEN, "ext_default_synth.tap"))
    ql, tl = cfg["query"]["limits"], cfg["target"]["limits"]
    assert (np.diff(np.diff(tl)) <= 0).all() and (np.diff(np.diff(tl)) == 0).any()           # the reference block arrives length-sorted, with ties
    assert (np.diff(np.diff(ql)) > 0).any()                                                    # ... the query block as it was
    c = emu.seed_params_from_tap(dict(cfg, seed_encoding=1) if tap == "ext_lin_hashed.tap" else cfg)
    hits, stats = lin_seed_search(c, blosum62_matrix8(), cfg["query"]["data"], ql, cfg["target"]["data"], tl)
    ref = np.concatenate([r["hits"] for r in recs])
    dropped = 1.0 - stats["selected"] / stats["joined"]
    print("%s: %d hits, the rule drops %.1f %% of %d joined positions, %s" % (tap, len(ref), 100 * dropped, stats["joined"], stats))
    assert len(hits) == len(ref) and hit_multiset(hits) == hit_multiset(ref)
    assert dropped >= 0.10
    if tap == "ext_lin_default.tap":
        assert stats["above_255"] > 0 and (ref["score"] > 255).sum() == stats["above_255"]      # kept as they are, none deferred
        assert stats["left_most_would_drop"] > 0               # the left-most filter is skipped, and that shows
