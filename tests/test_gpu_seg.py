"""-m gpu tests of SEG masking on the device (dmnd_seg_mask_block_device and its kin; diamond_amd/csrc/seg_kernels.hip) against the
reference's own SEG (the goldens minted from oracle/_ref/seg_ref) and against the host form (dmnd_seg_mask_block), on one block of 867 sequences built
from the three SEG fixtures: the reference's ctest proteins, the synthetic cases, and the device cases (left-remainder searches,
overlapping neighbours, lengths around one and two wavefronts, windows with 2 and 3 non-standard letters, the hand-back)."""
import functools
import os

import numpy as np
import pytest

from diamond_amd import hip
from test_seg_core import fixtures

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def block():
    """(data, limits, golden ranges per sequence, host-masked data, host n_masked): computed once, never modified."""
    data = [np.full(256, 31, np.int8)]
    limits = [256]
    for _, s, _ in fixtures():
        data += [s, np.array([31], np.int8)]
        limits.append(limits[-1] + len(s) + 1)
    data = np.concatenate(data + [np.full(256, 31, np.int8)])
    limits = np.array(limits, np.int64)
    want = data.copy()
    n_masked = hip.seg_mask_block(want, limits, threads=4)
    for a in (data, limits, want):
        a.setflags(write=False)
    return data, limits, [g for _, _, g in fixtures()], want, n_masked


@pytest.fixture
def ctx():
    c = hip.Context(device=0)
    yield c
    c.close()


def _by_sequence(ranges, n):
    out = [[] for _ in range(n)]
    for s, b, e in ranges.tolist():
        out[s].append((b, e))
    return out


def test_device_ranges_equal_the_reference_seg(ctx):
    data, limits, golden, _, _ = block()
    assert len(golden) == len(fixtures()) > 800
    ctx.upload_block(hip.TARGET, data, limits)
    ctx.seg_mask_block(hip.TARGET)
    ranges = ctx.seg_ranges(hip.TARGET)
    assert np.all(np.diff(ranges[:, 0]) >= 0)                              # sorted by sequence
    got = _by_sequence(ranges, len(golden))
    for i, (name, _, want) in enumerate(fixtures()):
        assert got[i] == want, name
    st = ctx.seg_stats()
    assert st["ranges"] == sum(len(g) for g in golden) > 1800
    assert st["work"] >= sum(1 for g in golden if g) and st["work"] < len(golden)
    assert st["kernel_ms"] > 0


def test_masked_block_equals_the_host_form_byte_for_byte(ctx):
    data, limits, _, want, n_want = block()
    ctx.upload_block(hip.TARGET, data, limits)
    host = data.copy()
    n = ctx.seg_mask_block(hip.TARGET, host)
    assert n == n_want > 20000
    assert np.array_equal(host, want)                                      # the patched host copy
    assert np.array_equal(ctx.download_block(hip.TARGET, data.size), want)      # the block in HBM
    # without a host copy: the same block
    ctx.upload_block(hip.TARGET, data, limits)
    assert ctx.seg_mask_block(hip.TARGET) == n_want
    assert np.array_equal(ctx.download_block(hip.TARGET, data.size), want)


def test_handed_back_sequences_are_counted_and_come_out_right(ctx):
    data, limits, golden, want, _ = block()
    long_raw = [i for i, (_, s, g) in enumerate(fixtures()) if any(e - b + 1 > 10000 for b, e in g)]
    # (a raw segment is never shorter than the trimmed one, and the fixtures hold no other sequence of 10 000 letters)
    assert len(long_raw) == 1 == sum(1 for _, s, _ in fixtures() if len(s) > 10000)
    for host in (data.copy(), None):                                       # unmasked letters from the host copy / copied from HBM
        ctx.upload_block(hip.TARGET, data, limits)
        ctx.seg_mask_block(hip.TARGET, host)
        assert ctx.seg_stats()["handed_back"] == len(long_raw)
        got = _by_sequence(ctx.seg_ranges(hip.TARGET), len(golden))
        for i in long_raw:
            assert got[i] == golden[i]
            lo, hi = limits[i], limits[i + 1] - 1
            assert np.array_equal(ctx.download_block(hip.TARGET, data.size)[lo:hi], want[lo:hi])


def test_subset_in_shuffled_order_leaves_the_other_sequences_alone(ctx):
    data, limits, golden, want, _ = block()
    rng = np.random.default_rng(5)
    n = len(golden)
    ids = rng.permutation(n)[: n // 3].astype(np.int32)
    ids = np.unique(np.concatenate([ids, np.array([i for i, (_, s, _) in enumerate(fixtures()) if len(s) > 10000], np.int32)]))
    rng.shuffle(ids)
    chosen = np.zeros(n, bool)
    chosen[ids] = True
    expect = data.copy()
    for i in ids:
        expect[limits[i]:limits[i + 1]] = want[limits[i]:limits[i + 1]]
    ctx.upload_block(hip.TARGET, data, limits)
    host = data.copy()
    n_masked = ctx.seg_mask_sequences(hip.TARGET, host, ids)
    assert n_masked == sum(e - b + 1 for i in ids for b, e in golden[i])
    assert np.array_equal(host, expect) and np.array_equal(ctx.download_block(hip.TARGET, data.size), expect)
    assert not np.array_equal(expect, want)                               # sequences outside the subset have segments too
    got = _by_sequence(ctx.seg_ranges(hip.TARGET), n)
    assert all(got[i] == (golden[i] if chosen[i] else []) for i in range(n))
    assert ctx.seg_mask_sequences(hip.TARGET, host, np.zeros(0, np.int32)) == 0


def test_a_range_list_forced_small_is_grown_and_gives_the_same_bytes(ctx, monkeypatch):
    data, limits, golden, want, n_want = block()
    ctx.upload_block(hip.TARGET, data, limits)
    monkeypatch.setenv("DMND_SEG_RANGE_CAP", "7")
    host = data.copy()
    assert ctx.seg_mask_block(hip.TARGET, host) == n_want
    monkeypatch.delenv("DMND_SEG_RANGE_CAP")
    assert np.array_equal(host, want) and np.array_equal(ctx.download_block(hip.TARGET, data.size), want)
    assert _by_sequence(ctx.seg_ranges(hip.TARGET), len(golden)) == golden
    assert ctx.seg_stats()["ranges"] == sum(len(g) for g in golden)


def test_shared_block_is_refused(ctx):
    data, limits, _, _, _ = block()
    ctx.upload_block(hip.TARGET, data, limits)
    other = hip.Context(device=0)
    try:
        other.share_block(hip.TARGET, ctx)
        with pytest.raises(hip.DiamondHipError, match="shared"):
            other.seg_mask_block(hip.TARGET)
        with pytest.raises(hip.DiamondHipError, match="shared"):
            other.seg_mask_sequences(hip.TARGET, None, np.array([0], np.int32))
        assert np.array_equal(ctx.download_block(hip.TARGET, data.size), data)      # nothing was written
    finally:
        other.close()


def test_block_of_short_sequences_masks_nothing(ctx):
    seqs = [np.zeros(k, np.int8) for k in (1, 2, 5, 9, 9, 3, 9)]          # homopolymers, all below the window of 10
    data = [np.full(256, 31, np.int8)]
    limits = [256]
    for s in seqs:
        data += [s, np.array([31], np.int8)]
        limits.append(limits[-1] + len(s) + 1)
    data = np.concatenate(data + [np.full(256, 31, np.int8)])
    ctx.upload_block(hip.TARGET, data, np.array(limits, np.int64))
    host = data.copy()
    assert ctx.seg_mask_block(hip.TARGET, host) == 0
    assert np.array_equal(host, data) and np.array_equal(ctx.download_block(hip.TARGET, data.size), data)
    st = ctx.seg_stats()
    assert (st["work"], st["handed_back"], st["ranges"]) == (0, 0, 0) and len(ctx.seg_ranges(hip.TARGET)) == 0


def test_masking_twice_keeps_every_mask_and_reports_the_second_pass_alone(ctx):
    data, limits, golden, want, _ = block()
    ctx.upload_block(hip.TARGET, data, limits)
    ctx.seg_mask_block(hip.TARGET)
    n2 = ctx.seg_mask_block(hip.TARGET)                                    # second pass: over the masked block
    twice = ctx.download_block(hip.TARGET, data.size)
    assert np.all(twice[want == 23] == 23)                                 # no letter unmasked that the first pass masked
    expect = want.copy()
    assert hip.seg_mask_block(expect, limits, threads=2) == n2             # the host form on the masked block
    assert np.array_equal(twice, expect)
    # the statistics and the range list are the second pass's own, not sums over the calls
    again = [hip.seg_ranges(want[limits[i]:limits[i + 1] - 1]) for i in range(len(golden))]
    assert _by_sequence(ctx.seg_ranges(hip.TARGET), len(golden)) == again
    st = ctx.seg_stats()
    assert st["ranges"] == sum(len(r) for r in again) < sum(len(g) for g in golden)
    assert st["handed_back"] == 0                                          # the homopolymer is all X now: no window at all
