"""CPU checks of the hashes the sliced long-seed stream keeps beside its list entries (csrc/seed_slices_core.h, restated for ctypes in
tests/emu/seed_slices_hash_emu.cpp): the cache of a block is built as the library builds it, and for every listed window -- not a
sample -- the stored hash is hash a of the window's own key (seed_key_at), and the level-1 probe from the stored hash (word and
bits) is the probe from the key, on the four filter geometries of test_seed_slices_emu.py."""
import ctypes
import os

import numpy as np
import pytest

from diamond_amd import hip, workload

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libswipe_emu.so")


def block():
    """delimiters, mask and stop letters, sequences shorter than the shapes (test_routing_rule_equals_the_plain_streams' block, longer)"""
    rng = np.random.default_rng(8)
    lens = rng.integers(1, 120, 1500)
    lens[::7] = rng.integers(1, 12, len(lens[::7]))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    letters = rng.integers(0, 20, int(off[-1])).astype(np.int8)
    letters[rng.random(len(letters)) < 0.03] = 23
    letters[rng.random(len(letters)) < 0.01] = 24
    return workload.sequence_set(letters, off)


_block = block()


@pytest.mark.parametrize("slot_bits,words,slices", [(23, 786_432, 32), (23, 524_288, 16), (10, 524_288, 16), (31, 4_194_304, 32)])
def test_stored_hash_probes_as_the_key_does(slot_bits, words, slices):
    lib = ctypes.CDLL(EMU)
    lib.emu_hash_block.restype = ctypes.c_int64
    lib.emu_hash_block.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_route_block.restype = ctypes.c_int64
    lib.emu_route_block.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    td, tl = _block
    b = slices.bit_length() - 1
    sp = hip.seed_params_fast(threads=1)
    sp2, _ = hip.seed_params_preset("default", hip.default_params(), threads=1)
    checked = 0
    for params in (sp, sp2):
        for sid in range(params.n_shapes):
            for (first, last) in ((0, len(tl) - 1), (3, len(tl) - 4)):
                t_begin, t_end = int(tl[first]), int(tl[last])
                n = ((t_end - (t_begin & ~15) + 15) // 16) * 16
                bad = np.zeros(4, np.int64)
                lst, hashes, counts = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(slices, np.uint32)
                for k3 in (0, 1):
                    seeds = lib.emu_hash_block(ctypes.byref(params), sid, td.ctypes.data, t_begin, t_end, b, slot_bits, words, k3,
                                               bad.ctypes.data, lst.ctypes.data, hashes.ctypes.data, counts.ctypes.data)
                    assert bad.tolist() == [0, 0, 0, 0]
                    # every window the plain stream probes is listed once, each slice's ascending, the others behind them
                    routed, plain = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
                    assert lib.emu_route_block(ctypes.byref(params), sid, td.ctypes.data, t_begin, t_end, b, routed.ctypes.data, plain.ctypes.data) == n
                    assert seeds == int(counts.sum()) == int((plain != 0xff).sum()) and seeds > n // 3
                    assert np.array_equal(np.sort(lst), np.arange(n, dtype=np.uint32))
                    ends = np.cumsum(counts)
                    for s in range(slices):
                        part = lst[ends[s] - counts[s]:ends[s]]
                        assert np.all(plain[part] == s) and np.all(np.diff(part.astype(np.int64)) > 0)
                    checked += seeds
    assert checked > 200_000
