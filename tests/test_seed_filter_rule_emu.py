"""CPU checks of the rule that sizes the level-1 filter of a search on the sliced long-seed stream (csrc/seed_slices_core.h
seed_slices_filter_words, restated for ctypes in tests/emu/seed_filter_rule_emu.cpp): it never goes below the plain stream's size nor
above the level-2 filter or 64 slices of 32 768 words, seed_slice_bits accepts whatever it changes, and it gives C2's block
64 slices of 128 KB."""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MOST = 64 * 32768


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(os.path.join(HERE, "emu", "libswipe_emu.so"))
    lib.emu_slices_filter_words.restype = ctypes.c_uint64
    lib.emu_slices_filter_words.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int)]
    lib.emu_slice_bits.restype = ctypes.c_int
    lib.emu_slice_bits.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32]
    lib.emu_slices_most_words.restype = ctypes.c_uint64
    lib.emu_bm1_bits.restype = ctypes.c_uint32
    lib.emu_bm1_bits.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    lib.emu_bm1_false_positive_rate.restype = ctypes.c_double
    lib.emu_bm1_false_positive_rate.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32]
    assert lib.emu_slices_most_words() == MOST
    return lib


def rule(lib, nq_pos, slot_bits, bm_words, default_words, max_slice_words=32768, forced=0):
    k3 = ctypes.c_int(-2)
    w = lib.emu_slices_filter_words(nq_pos, slot_bits, bm_words, default_words, max_slice_words, forced, ctypes.byref(k3))
    return int(w), k3.value


def plain_geometry(nq_pos):
    """seed_sizes for long seeds and a query block of up to 2^24 positions: (slot_bits, level-2 words, level-1 words)"""
    assert nq_pos <= 1 << 24
    slots = 1024
    while slots * 8 < nq_pos * 16:
        slots <<= 1
    bm = 1 << 15
    while bm * 32 < nq_pos * 16 and bm < 1 << 22:
        bm <<= 1
    bm1 = min((1 << 24) // 32, bm)
    if bm >= 3 * bm1 // 2:
        bm1 = 3 * bm1 // 2
    return slots.bit_length() - 1, bm, bm1


def test_bounds_and_slice_count_over_block_sizes(lib):
    rng = np.random.default_rng(4)
    sizes = sorted(set([1, 1000, 65_535, 65_536, 65_537, 131_072, 131_073, 1 << 20, (1 << 20) + 1, 3_019_757, 1 << 22, (1 << 22) + 1, 1 << 23, (1 << 24) - 1, 1 << 24]
                       + [int(x) for x in np.exp(rng.uniform(np.log(100), np.log(1 << 24), 400))]))
    changed = 0
    for nq in sizes:
        slot_bits, bm, bm1 = plain_geometry(nq)
        for max_words in (32768, 8192, 512, 64):
            w, k3 = rule(lib, nq, slot_bits, bm, bm1, max_words)
            assert bm1 <= w <= min(bm, MOST), (nq, max_words, w)
            if w != bm1:
                changed += 1
                b = lib.emu_slice_bits(w, slot_bits, max_words)
                assert 0 <= b <= 6 and w % (1 << b) == 0 and (w >> b) <= max_words and b <= slot_bits, (nq, max_words, w, b)
                assert w & (w - 1) == 0
                assert k3 == (2 if nq * 4 <= w * 32 else 0)      # (2: the third bit from below the word index, bm1_bits)
            else:
                assert k3 == -1                       # the default geometry keeps its own bits per seed
    assert changed > 100


def test_c2_block_gets_64_slices_of_128_kb(lib):
    nq = 3_019_757
    assert plain_geometry(nq) == (23, 1 << 21, 786_432)
    assert rule(lib, nq, 23, 1 << 21, 786_432) == (2_097_152, 2)
    assert lib.emu_slice_bits(2_097_152, 23, 32768) == 6
    assert lib.emu_slice_bits(786_432, 23, 32768) == 5      # today's 32 x 96 KB


@pytest.mark.parametrize("nq", [1, 600, 15_000, 65_536])
def test_small_block_keeps_the_default(lib, nq):
    slot_bits, bm, bm1 = plain_geometry(nq)
    assert bm == bm1 == 32768
    assert rule(lib, nq, slot_bits, bm, bm1) == (bm1, -1)


def test_slice_hook_without_a_slice_count_falls_back(lib):
    # 2^21 words in slices of at most 512 would be 4096 slices
    assert lib.emu_slice_bits(2_097_152, 23, 512) == -1
    assert rule(lib, 3_019_757, 23, 1 << 21, 786_432, max_slice_words=512) == (786_432, -1)
    # ... and too few hash bits inside the filter's hash mask for the slice count
    assert rule(lib, 3_019_757, 5, 1 << 21, 786_432) == (786_432, -1)


def test_forced_size_is_bound_by_the_slice_count_alone(lib):
    slot_bits, bm, bm1 = plain_geometry(15_000)
    assert bm == 32768
    assert rule(lib, 15_000, slot_bits, bm, bm1, forced=65_536) == (65_536, 2)          # above the level-2 size
    assert lib.emu_slice_bits(65_536, slot_bits, 32768) == 1
    assert rule(lib, 15_000, slot_bits, bm, bm1, forced=MOST) == (MOST, 2)
    assert lib.emu_slice_bits(MOST, slot_bits, 32768) == 6
    assert rule(lib, 15_000, slot_bits, bm, bm1, forced=98_304) == (98_304, 1)          # no power of two: the third bit by the plain stream's rule
    assert rule(lib, 3_019_757, 23, 1 << 21, 786_432, forced=65_536) == (65_536, 0)     # under four filter bits per position: two bits
    assert rule(lib, 15_000, slot_bits, bm, bm1, forced=2 * MOST) == (bm1, -1)           # more than 64 slices
    assert rule(lib, 15_000, slot_bits, bm, bm1, forced=65_537) == (bm1, -1)             # odd: no slice count divides it


def test_third_bit_of_a_sliced_filter_comes_from_below_the_word_index(lib):
    """bm1_bits(h, 2): the two bits of k3 = 0 / 1 and a third that depends on h's low eleven bits alone -- the word index of a
    power of two of at most 2^21 words is h >> 11 and above"""
    rng = np.random.default_rng(6)
    for h in rng.integers(0, 1 << 32, 3000):
        h = int(h)
        two, three = lib.emu_bm1_bits(h, 0), lib.emu_bm1_bits(h, 2)
        assert three & two == two and bin(three).count("1") <= 3
        assert three == lib.emu_bm1_bits(h & 0x7ff, 2)
        assert lib.emu_bm1_bits(h, 1) == two | (1 << ((h >> 10) & 31))      # the plain stream's rule stays what it was
    places = {lib.emu_bm1_bits(x, 2) & ~lib.emu_bm1_bits(x, 0) for x in range(1 << 11)}
    assert len([p for p in places if p]) == 32                              # every place of the word is some key's third


def test_modelled_false_positives_of_c2s_filter(lib):
    """3e6 random seeds in 2^21 words (C2's sliced filter): the blocked filter's ideal rates are 1.2 % with two bits and 0.58 % with
    three independent ones. k3 = 2 must reach the three-bit rate within a fifth; k3 = 1, whose third bit follows the word index,
    does not (printed, not required)."""
    rate = {k3: lib.emu_bm1_false_positive_rate(3_000_000, 2_000_000, 1 << 21, 23, k3) for k3 in (0, 1, 2)}
    print("modelled false positives, 2^21 words, k3 = 0 / 1 / 2: %.4f %.4f %.4f" % (rate[0], rate[1], rate[2]))
    assert 0.010 < rate[0] < 0.014
    assert rate[2] < 0.0058 * 1.2
