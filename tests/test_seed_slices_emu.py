"""CPU checks of the sliced long-seed stream (csrc/seed_slices_core.h, restated for ctypes in tests/emu/seed_slices_emu.cpp):
the slice identity -- a key whose hash a has the top b bits s probes a level-1 word of slice s -- over the filter geometries the
stream meets, the balance of the slices on realistic keys, the routing rule against the plain stream's rule, and the host
bookkeeping of the reference cache as a stand-alone program under AddressSanitizer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from diamond_amd import hip, workload

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libswipe_emu.so")


def realistic_keys(rng, n):
    """care-masked nibble windows of reduced letters, with the class frequencies of test_seed_classes_emu.py"""
    p = np.array([0.16, 0.13, 0.12, 0.11, 0.10, 0.09, 0.08, 0.07, 0.06, 0.05, 0.03])
    nib = rng.choice(11, size=(n, 16), p=p).astype(np.uint64)
    keys = np.zeros(n, np.uint64)
    for k in [0, 1, 2, 4, 5, 7, 8, 10, 11, 13, 14, 15]:
        keys |= nib[:, k] << np.uint64(4 * k)
    return keys


def slice_words(keys, slot_bits, words):
    lib = ctypes.CDLL(EMU)
    n = len(keys)
    h, word = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    lib.emu_slice_words.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_slice_words.restype = ctypes.c_int
    b = lib.emu_slice_words(keys.ctypes.data, n, slot_bits, words, h.ctypes.data, word.ctypes.data)
    return b, h, word


@pytest.mark.parametrize("slot_bits,words,slices,fits", [(23, 786_432, 32, True), (23, 524_288, 16, True), (10, 524_288, 16, True), (31, 4_194_304, 32, False)])
def test_slice_identity(slot_bits, words, slices, fits):
    """(slot_bits 23, 786 432 words, 32 slices) is C2's geometry; slot_bits 10 leaves ten hash bits in the word's mask; the last
    one's slices do not fit LDS (the stream would not take it) -- the identity holds all the same."""
    rng = np.random.default_rng(slot_bits * 1000 + slices)
    n = 300_000
    b = slices.bit_length() - 1
    per = words // slices
    assert words % slices == 0 and slot_bits >= b
    for keys in (rng.integers(0, 1 << 63, n, dtype=np.int64).astype(np.uint64), realistic_keys(rng, n)):
        got_b, h, word = slice_words(keys, slot_bits, words)
        assert got_b == (b if fits else -1)
        s = h >> np.uint32(32 - b)
        assert np.array_equal(word // np.uint32(per), s)
        assert word.max() < words
        # the words of a slice span it (where the hash mask leaves a slice more than a handful of words)
        local = word - s * np.uint32(per)
        distinct = min(per, 1 << (slot_bits - b))
        for k in (0, slices // 2, slices - 1):
            w = local[s == k]
            assert w.min() < max(per // 50, per // distinct + 1) and w.max() >= per - max(per // 50, per // distinct + 1)
    # realistic keys: the slices' shares within a sixth of equal
    share = np.bincount(s, minlength=slices) / n
    assert share.min() > (1 - 1 / 6) / slices and share.max() < (1 + 1 / 6) / slices, share


def test_routing_rule_equals_the_plain_streams():
    """Delimiters, mask letters at care and at other positions, stop letters, sequences shorter than the shape, and a window
    range that starts and ends off a multiple of 16: the routing byte of every window is the plain rule's."""
    lib = ctypes.CDLL(EMU)
    lib.emu_route_block.restype = ctypes.c_int64
    lib.emu_route_block.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    rng = np.random.default_rng(8)
    sp = hip.seed_params_fast(threads=1)
    sp2, _ = hip.seed_params_preset("default", hip.default_params(), threads=1)
    lens = rng.integers(1, 120, 300)
    lens[::7] = rng.integers(1, 12, len(lens[::7]))                    # shorter than the shapes
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    letters = rng.integers(0, 20, int(off[-1])).astype(np.int8)
    letters[rng.random(len(letters)) < 0.03] = 23                      # mask letters: some at care positions of a window, some not
    letters[rng.random(len(letters)) < 0.01] = 24                      # stop letters
    td, tl = workload.sequence_set(letters, off)
    checked = 0
    for params in (sp, sp2):
        for sid in range(params.n_shapes):
            care = params.shape_mask[sid]
            assert care != (1 << params.shape_len[sid]) - 1           # a spaced shape: it has positions that do not count
            for (a, b) in ((0, len(tl) - 1), (3, len(tl) - 4), (5, 9)):
                t_begin, t_end = int(tl[a]), int(tl[b])
                if (a, b) == (3, len(tl) - 4):
                    assert t_begin % 16 and t_end % 16
                for bits in (0, 5):
                    n = ((t_end - (t_begin & ~15) + 15) // 16) * 16
                    routed, plain = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
                    assert lib.emu_route_block(ctypes.byref(params), sid, td.ctypes.data, t_begin, t_end, bits, routed.ctypes.data, plain.ctypes.data) == n
                    assert np.array_equal(routed, plain)
                    valid = routed != 0xff
                    assert 0.3 < valid.mean() < 0.98 and routed[valid].max() < (1 << bits)
                    checked += 1
    assert checked == 3 * 2 * 3


def test_cache_bookkeeping_under_address_sanitizer(tmp_path):
    """Key comparison, budget, invalidation and the forcing hook of the reference cache: a stand-alone program over the same header
    the library uses, compiled with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the host compiler that built tests/emu"
    exe = str(tmp_path / "seed_ref_main")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, os.path.join(HERE, "asan", "seed_ref_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
