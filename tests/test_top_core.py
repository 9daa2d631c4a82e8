"""CPU checks of the --top arithmetic (diamond_amd/csrc/top_core.h: what the host path's output_range / append_hits and the --top
kernels of the device half compute), via tests/emu/libswipe_emu.so, with the project's own Gumbel constants of BLOSUM62 11/1
(score_matrices.h -> Evaluer). For --top in {0, 5, 10, 33.3, 60} and every pair of best score and score in 1..4000:
 * the bit-score cutoff test equals a literal transcription of output_range: bitscore(score) >= max((1 - top/100) * bitscore(best), 1.0)
   with Evaluer::bitscore;
 * the integer append test equals (int)((1 - top/100) * score);
 * the near predicate (1e-9 relative, the tolerance of the device half's decisions) fires for none of these pairs -- the percentages
   lie off the values a score can take, so the GPU tests can hold the device half to a low share of queries handed back. The
   closest pair lies 9.2e-8 away (--top 33.3, scores 3952 and 2632; the other four values: 4.8e-7 and more). 33.3 is kept although that
   is a little under 1e-7: the GPU tests are set with it, and the margin that matters is the one to the tolerance, asserted here as ten
   tolerances (1e-8)."""
import ctypes

import numpy as np
import pytest

import emu_py as emu

TOPS = [0.0, 5.0, 10.0, 33.3, 60.0]
MAX_SCORE = 4000


def _lib():
    lib = emu.lib()
    d, i = ctypes.c_double, ctypes.c_int
    lib.emu_top_check.restype = None
    lib.emu_top_check.argtypes = [d, d, d, i, ctypes.c_void_p, ctypes.POINTER(d), ctypes.c_void_p]
    for f in (lib.emu_top_pass, lib.emu_top_near, lib.emu_top_append):
        f.restype = i
        f.argtypes = [d, d, d, i, i]
    lib.emu_top_bits.restype = d
    lib.emu_top_bits.argtypes = [d, d, i]
    return lib


def constants():
    lam, K = ctypes.c_double(0), ctypes.c_double(0)
    assert emu.lib().emu_top_blosum62_constants(ctypes.byref(lam), ctypes.byref(K)) == 0
    return lam.value, K.value


def test_constants_are_blosum62_11_1():
    assert constants() == (0.267, 0.041)


@pytest.mark.parametrize("top", TOPS)
def test_cutoff_append_and_near_over_all_score_pairs(top):
    lib = _lib()
    lam, K = constants()
    out = np.zeros(4, np.int64)
    closest = ctypes.c_double(0)
    pair = np.zeros(2, np.int32)
    lib.emu_top_check(top, lam, K, MAX_SCORE, out.ctypes.data, ctypes.byref(closest), pair.ctypes.data)
    print("top %g: closest relative distance of a bit score to a cutoff %.3g at (best, score) = %s" % (top, closest.value, pair.tolist()))
    assert out[3] == MAX_SCORE * (MAX_SCORE + 1) // 2
    assert out[0] == 0, "cutoff test differs from output_range"
    assert out[1] == 0, "append test differs from (int)(f * score)"
    assert out[2] == 0, "the near predicate fires"
    assert closest.value >= 1e-8


def test_hand_made_cases():
    lib = _lib()
    lam, K = constants()
    bits = lambda s: (lam * s - np.log(K)) / np.log(2.0)
    assert abs(lib.emu_top_bits(lam, K, 100) - bits(100)) < 1e-12
    # --top 10, best 500 (197.2 bits): the cutoff is 177.5 bits, which raw score 448 misses (177.2) and 449 reaches (177.6)
    assert lib.emu_top_pass(10.0, lam, K, 449, 500) == 1 and lib.emu_top_pass(10.0, lam, K, 448, 500) == 0
    # --top 0: only the best score itself; the best entry always stays and is never `near`
    assert lib.emu_top_pass(0.0, lam, K, 500, 500) == 1 and lib.emu_top_pass(0.0, lam, K, 499, 500) == 0
    assert lib.emu_top_near(0.0, lam, K, 500, 500) == 0 and lib.emu_top_near(33.3, lam, K, 77, 77) == 0
    # the 1.0 floor: --top 100 makes the cutoff 0 x bits -> 1.0; score 1 has 4.99 bits. Never `near` at the floor
    assert lib.emu_top_pass(100.0, lam, K, 1, 4000) == 1 and lib.emu_top_near(100.0, lam, K, 1, 4000) == 0
    # a cutoff that a score meets exactly is `near`: f = 1 (--top 0) against an equal score is excluded, so build one with f = 0.5
    # and K = 1 (ln K = 0): bits(best 200) x 0.5 = bits(100) up to rounding
    assert lib.emu_top_near(50.0, lam, 1.0, 100, 200) == 1 and lib.emu_top_near(50.0, lam, 1.0, 101, 200) == 0
    # append: (int)(0.9 x 100) = 90, (int)(0.667 x 100) = 66, truncation not rounding
    assert lib.emu_top_append(10.0, lam, K, 90, 100) == 1 and lib.emu_top_append(10.0, lam, K, 89, 100) == 0
    assert lib.emu_top_append(33.3, lam, K, 66, 100) == 1 and lib.emu_top_append(33.3, lam, K, 65, 100) == 0
    assert lib.emu_top_append(0.0, lam, K, 100, 100) == 1 and lib.emu_top_append(0.0, lam, K, 99, 100) == 0
