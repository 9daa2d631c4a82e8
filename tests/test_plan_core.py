"""CPU checks of diamond_amd/csrc/plan_core.h, via tests/emu/libswipe_emu.so: the sort key that brings the seed hits of a translated
call into (read, target) order on the device, and the rule that picks a target's best HSP over the contexts of a read.
 * The key is the read above the target, each in the bits its block needs. Both are block sequence numbers below 2^32, so the key
   has at most 64 bits: it bounds no block size, and no call falls back to the host path because of it (the planner's own bound is
   the 2^31 hits of a call, as for protein queries). Checked at the limits of all three fields: read 0 and 2^32 / 6 - 1 (the last
   read a block of 2^32 - 4 contexts can hold), target 0 and 2^32 - 1, frames 0 and 5 of one read mapping to the same key.
 * Keys order as (read, target) pairs do, and a stable sort by them keeps (frame, location, seed offset) inside a pair.
 * The tie rule on hand-made triples (score, context, d_begin), contexts ascending: the highest score; of equal scores the FIRST
   context that reaches it; inside that context the band that starts first."""
import ctypes

import numpy as np

import emu_py as emu


def _lib():
    lib = emu.lib()
    u64, u32, i = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    lib.emu_plan_bits_below.restype, lib.emu_plan_bits_below.argtypes = i, [u64]
    lib.emu_plan_key_bits.restype, lib.emu_plan_key_bits.argtypes = None, [u64, u64, ctypes.POINTER(i), ctypes.POINTER(i)]
    lib.emu_plan_pair_key.restype, lib.emu_plan_pair_key.argtypes = u64, [u32, u32, i]
    lib.emu_plan_key_read.restype, lib.emu_plan_key_read.argtypes = u32, [u64, i]
    lib.emu_plan_key_target.restype, lib.emu_plan_key_target.argtypes = u32, [u64, i]
    lib.emu_best_hsp.restype, lib.emu_best_hsp.argtypes = i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, i]
    return lib


def _bits(lib, n_reads, n_targets):
    t, r = ctypes.c_int(0), ctypes.c_int(0)
    lib.emu_plan_key_bits(n_reads, n_targets, ctypes.byref(t), ctypes.byref(r))
    return t.value, r.value


def test_bits_hold_every_value_below_n():
    lib = _lib()
    for n, want in [(1, 1), (2, 1), (3, 2), (4, 2), (5, 3), (1500, 11), (2 ** 31, 31), (2 ** 31 + 1, 32), (2 ** 32, 32)]:
        assert lib.emu_plan_bits_below(n) == want, n
        assert n - 1 < 2 ** want


def test_key_packing_at_the_limits_of_read_target_and_frame():
    lib = _lib()
    n_targets, n_contexts = 2 ** 32, 2 ** 32 - 4            # the largest blocks 32-bit sequence numbers allow (contexts: a multiple of 6)
    n_reads = n_contexts // 6
    tb, rb = _bits(lib, n_reads, n_targets)
    assert (tb, rb) == (32, 30) and tb + rb <= 64              # the bound: none below the 32-bit sequence numbers themselves
    for read in (0, 1, n_reads - 1):
        for target in (0, 1, n_targets - 1):
            key = lib.emu_plan_pair_key(read, target, tb)
            assert key == (read << tb) | target and key < 2 ** (tb + rb)
            assert (lib.emu_plan_key_read(key, tb), lib.emu_plan_key_target(key, tb)) == (read, target)
    # the key is built from context // 6: the six frames of a read share it
    last = n_contexts - 6
    assert {lib.emu_plan_pair_key((last + f) // 6, 7, tb) for f in range(6)} == {lib.emu_plan_pair_key(n_reads - 1, 7, tb)}
    # small blocks take few bits: the golden blastx block (120 reads, 1 500 targets) sorts over 18
    assert _bits(lib, 120, 1500) == (11, 7)


def test_keys_order_as_read_target_pairs_and_a_stable_sort_keeps_the_frames_in_order():
    lib = _lib()
    rng = np.random.default_rng(5)
    n_reads, n_targets = 37, 1000
    tb, _ = _bits(lib, n_reads, n_targets)
    # hits as a seed search leaves them: by (context, location)
    ctxs = np.sort(rng.integers(0, 6 * n_reads, 4000))
    tgt = rng.integers(0, n_targets, 4000)
    order = np.lexsort((tgt, ctxs))
    ctxs, tgt = ctxs[order], tgt[order]
    keys = np.array([lib.emu_plan_pair_key(int(c) // 6, int(t), tb) for c, t in zip(ctxs, tgt)], np.uint64)
    perm = np.argsort(keys, kind="stable")
    got = list(zip((ctxs[perm] // 6).tolist(), tgt[perm].tolist(), (ctxs[perm] % 6).tolist()))
    assert got == sorted(got)                                   # (read, target, frame): what load_hits' sort gives


def _best(lib, triples):
    s = np.array([t[0] for t in triples], np.int32)
    c = np.array([t[1] for t in triples], np.int64)
    d = np.array([t[2] for t in triples], np.int32)
    return lib.emu_best_hsp(s.ctypes.data, c.ctypes.data, d.ctypes.data, len(triples))


def test_best_hsp_tie_rule_on_hand_made_triples():
    lib = _lib()
    assert _best(lib, []) == -1
    assert _best(lib, [(50, 0, 3)]) == 0
    assert _best(lib, [(50, 0, 3), (60, 1, 9)]) == 1                            # the higher score, whatever the context
    assert _best(lib, [(60, 0, 3), (60, 1, -9)]) == 0                           # equal scores: the first context, even if the other band starts first
    assert _best(lib, [(60, 1, 3), (60, 4, -9), (60, 5, -20)]) == 0
    assert _best(lib, [(60, 2, 3), (60, 2, -9)]) == 1                           # inside one context: the band that starts first
    assert _best(lib, [(60, 2, -9), (60, 2, 3)]) == 0
    assert _best(lib, [(40, 0, 0), (60, 1, 5), (60, 1, 2), (60, 3, -7), (61, 5, 8), (61, 5, 9)]) == 4
    assert _best(lib, [(60, 0, 5), (70, 1, 5), (60, 0, 1)]) == 1                # a later, lower DpTarget of an earlier context does not come back
    # one context (a protein query): score descending, d_begin ascending
    assert _best(lib, [(60, 0, 5), (60, 0, 1), (59, 0, -30)]) == 1
