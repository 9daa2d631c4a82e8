"""CPU: the full-matrix arithmetic of csrc/plan_core.h (Extension::Mode::FULL -- --ext full, the final pass of --global-ranking), the
statements plan_full_kernel, plan_pairs_kernel and ext_mark_kernel compile, through tests/emu/plan_full_emu.cpp.
 * the band of a unit is [-(tlen - 1), qlen): every diagonal of the matrix, so the banded sweep over it has tlen columns
   (oracle_py.banded_cols) and qlen + tlen - 1 diagonals -- at the band-class edges 128 / 129 and 4096 / 4097 too;
 * its DP size is qlen x tlen, the rule of dp_size in csrc/extend_host.hip (DP::Flags::FULL_MATRIX), NOT columns x band width -- at
   10^6 (kept on the device under the default max_swipe_dp) and 10^6 + 1000 (handed back);
 * a (read, target) pair of six contexts: one band per frame with a hit, each over its own context's matrix, band_query = that
   context, n_bands = the frames with hits, ungapped0 = context 0's best stage-1 score or 0."""
import ctypes

import numpy as np
import pytest

import emu_py
import oracle_py

MAX_SWIPE_DP = 1000000


def _band(qlen, tlen):
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    emu_py.lib().emu_full_matrix_band(int(qlen), int(tlen), ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def _dp_size(qlen, tlen):
    f = emu_py.lib().emu_full_matrix_dp_size
    f.restype = ctypes.c_int64
    return f(int(qlen), int(tlen))


def _host_dp_size(qlen, tlen, d_begin, d_end, full):
    """dp_size of csrc/extend_host.hip extend_range"""
    return qlen * tlen if full else oracle_py.banded_cols(qlen, tlen, d_begin, d_end) * (d_end - d_begin)


def _lengths():
    rng = np.random.default_rng(41)
    pairs = [(1, 1), (1, 5000), (5000, 1), (1, 2), (2, 1), (5000, 5000)]
    for band in (128, 129, 4096, 4097):                 # qlen + tlen - 1 on both sides of a band-class edge, short side either way
        for q in (1, 7, band // 2, band - 6, band):
            pairs.append((q, band + 1 - q))
    pairs += [(1000, 1000), (1000, 1001), (1001, 1000), (200, 5000), (5000, 200), (250, 4000), (250, 4004)]      # 10^6 and 10^6 + 1000 cells
    pairs += [(int(a), int(b)) for a, b in rng.integers(1, 5001, (300, 2))]
    return pairs


def test_the_band_of_a_full_matrix_unit_is_every_diagonal():
    for qlen, tlen in _lengths():
        d0, d1 = _band(qlen, tlen)
        assert (d0, d1) == (-(tlen - 1), qlen)
        assert d1 - d0 == qlen + tlen - 1
        assert oracle_py.banded_cols(qlen, tlen, d0, d1) == tlen      # the sweep visits every target column
        # one diagonal less on either side loses a corner cell
        if tlen > 1:
            assert oracle_py.banded_cols(qlen, tlen, d0 + 1, d1) <= tlen
    assert _band(100, 29)[1] - _band(100, 29)[0] == 128 and _band(100, 30)[1] - _band(100, 30)[0] == 129
    assert _band(97, 4000)[1] - _band(97, 4000)[0] == 4096 and _band(98, 4000)[1] - _band(98, 4000)[0] == 4097


def test_the_dp_size_is_the_matrix_not_the_band():
    seen_keep = seen_back = 0
    for qlen, tlen in _lengths():
        d0, d1 = _band(qlen, tlen)
        size = _dp_size(qlen, tlen)
        assert size == qlen * tlen == _host_dp_size(qlen, tlen, d0, d1, True)
        banded = _host_dp_size(qlen, tlen, d0, d1, False)
        assert banded == tlen * (qlen + tlen - 1) >= size
        seen_keep += size <= MAX_SWIPE_DP < banded            # the two rules decide differently: the full rule keeps it
        seen_back += size > MAX_SWIPE_DP
    assert seen_keep > 0 and seen_back > 0
    assert _dp_size(1000, 1000) == MAX_SWIPE_DP and _dp_size(1000, 1001) == MAX_SWIPE_DP + 1000
    assert _dp_size(250, 4000) == MAX_SWIPE_DP and _dp_size(250, 4004) == MAX_SWIPE_DP + 1000
    assert _dp_size(5000, 5000) == 25000000                   # (64-bit: 46341^2 is the first square past 2^31)
    assert _dp_size(70000, 70000) == 4900000000


def _pair(frames_scores, qlen, tlen, query0=12, limit=254):
    frames = np.array([f for f, _ in frames_scores], np.int32)
    scores = np.array([s for _, s in frames_scores], np.int32)
    ql = np.array(qlen, np.int32)
    d0, d1, bq = np.zeros(6, np.int32), np.zeros(6, np.int32), np.zeros(6, np.uint32)
    nb, ps, ug = ctypes.c_uint32(0), ctypes.c_int(0), ctypes.c_int(0)
    v = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n = emu_py.lib().emu_plan_full_pair(v(frames), v(scores), len(frames), v(ql), int(tlen), ctypes.c_uint32(query0), ctypes.c_uint32(limit),
                                        v(d0), v(d1), v(bq), ctypes.byref(nb), ctypes.byref(ps), ctypes.byref(ug))
    return n, list(zip(d0[:max(n, 0)].tolist(), d1[:max(n, 0)].tolist(), bq[:max(n, 0)].tolist())), nb.value, ps.value, ug.value


QLEN = [50, 49, 49, 50, 48, 49]          # the six frames of a 150-base read


@pytest.mark.parametrize("hits", [
    [(0, 31)],
    [(3, 44)],
    [(1, 27), (1, 35), (4, 30)],
    [(0, 20), (0, 22), (1, 50), (2, 21), (3, 33), (4, 19), (5, 60), (5, 58)],
], ids=["frame0", "frame3", "frames1and4", "all_six"])
def test_a_pair_of_six_contexts_gets_one_band_per_frame_with_a_hit(hits):
    tlen = 333
    n, units, n_bands, score, ungapped0 = _pair(hits, QLEN, tlen)
    frames = sorted(set(f for f, _ in hits))
    # the host form (csrc/extend_host.hip plan_groups, Mode::FULL): per frame its best score; a band where that is non-zero
    best = {f: max(s for g, s in hits if g == f) for f in frames}
    assert n == len(frames) == n_bands
    assert units == [(-(tlen - 1), QLEN[f], 12 + f) for f in frames]
    assert score == max(best.values())
    assert ungapped0 == best.get(0, 0)


def test_a_pair_is_never_left_to_the_host_in_full_mode():
    # six units of one band each stay far below the planner's limit; only a unit that IS left to the host (banded planning) marks the pair
    assert _pair([(f, 10 + f) for f in range(6)], QLEN, 100)[0] == 6
    assert _pair([(f, 10 + f) for f in range(6)], QLEN, 100, limit=6)[0] == -1
