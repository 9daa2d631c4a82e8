"""CPU checks of the query-side layout (seed_core.h seed_order and the filter-word functions, via tests/emu/libswipe_emu.so): the
home slot, the level-1 word and the level-2 word are non-decreasing functions of the build's sort key t, the stream's form of the
level-1 word equals the one the build derives from t, and with key classes class c owns the c-th eighth of slots and words."""
import ctypes

import numpy as np
import pytest

import emu_py as emu


def layout(keys, slot_bits, classes, bm1_words, bm_log2):
    lib = emu.lib()
    n = len(keys)
    out = [np.zeros(n, np.uint32) for _ in range(5)]
    lib.emu_seed_layout.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int] + [ctypes.c_void_p] * 5
    lib.emu_seed_layout(keys.ctypes.data, n, slot_bits, classes, bm1_words, bm_log2, *[o.ctypes.data for o in out])
    return out


def nondecreasing_in(t, w):
    o = np.argsort(t, kind="stable")
    return bool((np.diff(w[o].astype(np.int64)) >= 0).all())


# (slot_bits, level-1 words, level-2 log2): C2's geometry, a short-seed one, a tiny block's, the largest table
@pytest.mark.parametrize("slot_bits,bm1_words,bm_log2", [(23, 786432, 21), (24, 262144, 22), (10, 524288, 15), (31, 4194304, 22)])
@pytest.mark.parametrize("classes", [0, 8])
def test_layout_is_monotone_in_the_sort_key(slot_bits, bm1_words, bm_log2, classes):
    rng = np.random.default_rng(slot_bits + classes)
    keys = rng.integers(0, 2**63, 300_000, dtype=np.uint64) & np.uint64(0x0FFFFFFFFFFFFFFF)
    t, cls, w1k, w1t, w2 = layout(keys, slot_bits, classes, bm1_words, bm_log2)
    assert (t < 2**slot_bits).all()
    assert np.array_equal(w1k, w1t)                      # the stream probes the word the build filled
    assert (w1t < bm1_words).all() and (w2 < 2**bm_log2).all()
    assert nondecreasing_in(t, w1t) and nondecreasing_in(t, w2)
    if classes:
        eighth = 2 ** (slot_bits - 3)
        assert np.array_equal(t // eighth, cls)
        assert np.array_equal(w1t // (bm1_words // 8), cls)
        assert np.array_equal(w2 // (2 ** bm_log2 // 8), cls)
    else:
        # the home slot spreads over the whole table
        assert len(np.unique(t >> max(slot_bits - 8, 0))) == min(256, 2**slot_bits)
