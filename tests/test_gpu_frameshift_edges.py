"""-m gpu tests of dmnd_frameshift_swipe (frameshift_api.hip, frameshift_kernels.hip, frameshift_core.h) outside the one regime
tests/test_gpu_frameshift.py runs it in. Every comparison is exact -- integers, transcripts byte for byte -- against
oracle/frameshift_swipe.c; every precondition is computed from the inputs and the oracle, never from the device's answers.
  1. the chunk loop of run_launch under a small trace budget (DMND_TRACE_ARENA_MB=8): per-chunk trace / transcript offsets,
     wave_off / wave_rows, the copy back to results + c0, the transcript gather;
  2. its 1 GiB limit on the interleaved state of a score-only pass (the 4 Mi-item limit is not tested);
  3. the int16 saturation at 65535 and the re-run of such an item alone on its own band;
  4. letters 0-25 (X, stops, the hard-mask letter), four matrices / gap penalties, frameshift penalties 1, 15, 50;
  5. reads of 3-14 nucleotides against targets of 1-4 letters on every band, enumerated;
  6. the entry's refusals, each followed by a valid call on the same context;
(7. the CLI under a small trace budget and with another matrix: tests/test_gpu_cli.py.)"""
import ctypes
import time
import numpy as np
import pytest
import torch

import oracle_py as orc
from diamond_amd import hip
from test_frameshift import (KEYS, MATRICES, _random_case, degenerate_items, edge_cols, end_frame, oracle_score_only, own_geometry,
                             saturation_groups, wide_items)
from test_gpu_frameshift import MAP, _pack

pytestmark = pytest.mark.gpu
SCORE_FIELDS = ("score", "max_col", "q_begin", "q_end", "read_begin", "read_end", "frame")
MiB = 1 << 20


def _context(params=None, arena_mb=None):
    """A context; arena_mb: DMND_TRACE_ARENA_MB while dmnd_create reads it"""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    with pytest.MonkeyPatch.context() as mp:
        if arena_mb is None:
            mp.delenv("DMND_TRACE_ARENA_MB", raising=False)
        else:
            mp.setenv("DMND_TRACE_ARENA_MB", str(arena_mb))
        return hip.Context(params=params)


@pytest.fixture(scope="module")
def ctx():
    c = _context()
    yield c
    c.close()


def _items(meta, groups, cols):
    """meta: [(frames, strand, dna_len, target, d_begin, d_end)] -> query block, target block, FS_TARGET_DTYPE items"""
    return _pack([(m[0], m[1], m[2], int(g), [(m[3], m[4], m[5], int(c))]) for m, g, c in zip(meta, groups, cols)])


def _upload(c, meta, groups, cols):
    qb, tb, items = _items(meta, groups, cols)
    c.upload_block(hip.QUERY, qb)
    c.upload_block(hip.TARGET, tb)
    return items


def _tracebacks(meta, M, go, ge, fs):
    want = []
    for frames, strand, dna_len, t, d0, d1 in meta:
        rc, o, otr = orc.frameshift_traceback(frames, strand, dna_len, t, d0, d1, M, go, ge, fs)
        assert rc == 0
        want.append((o, otr))
    return want


def _assert_tracebacks(out, tr, want, tag=""):
    """every field the oracle has, the transcript and its terminator; an item without an alignment reports zeros and no transcript"""
    assert len(out) == len(want)
    for k, (o, otr) in enumerate(want):
        g = out[k]
        assert g["score"] == o["score"], (tag, k, g, o)
        if o["score"] > 0:
            assert all(g[MAP.get(x, x)] == o[x] for x in KEYS) and g["transcript_len"] == o["transcript_len"] == len(otr), (tag, k, g, o)
            assert np.array_equal(tr[g["transcript_off"]: g["transcript_off"] + g["transcript_len"]], otr), (tag, k)
            assert tr[g["transcript_off"] + g["transcript_len"]] == 0, (tag, k)
        else:
            assert g["transcript_off"] == -1 and g["transcript_len"] == 0 and g["length"] == 0, (tag, k, g)
    # the arena holds the transcripts in item order, one terminator each, and nothing else
    assert len(tr) == sum(len(otr) + 1 for o, otr in want if o["score"] > 0), tag


def _assert_scores(out, want, tag=""):
    assert len(out) == len(want)
    for k, w in enumerate(want):
        assert tuple(int(out[k][x]) for x in SCORE_FIELDS) == w, (tag, k, out[k], w)


# ---- 1. chunked traceback launches ---------------------------------------------------------------------------------------------

def _trace_bytes(m):
    """kept columns of a traceback item: (cols + 2) * (3 band + 1) int32 (f3_trace_cols restated)"""
    frames, _, _, t, d0, d1 = m
    band, i0, i1, pos0 = own_geometry(d0, d1)
    j1 = min(len(frames[0]) - 1 - d0, len(t) - 1) + 1
    return (max(j1 - pos0, 0) + 2) * (3 * band + 1) * 4


@pytest.fixture(scope="module")
def chunked():
    rng = np.random.default_rng(21)
    M = hip.matrix_of(hip.default_params())
    meta = []
    while len(meta) < 840:
        frames, dna_len, t, d0, d1 = _random_case(rng, M)
        meta.append((frames, len(meta) % 2, dna_len, t, d0, d1))
    small, large = _context(arena_mb=8), _context()
    for c in (small, large):
        items = _upload(c, meta, np.arange(len(meta)) // 5, edge_cols(len(meta)))
    yield dict(meta=meta, items=items, want=_tracebacks(meta, M, 11, 1, 15), need=np.array([_trace_bytes(m) for m in meta], np.int64), small=small, large=large)
    small.close()
    large.close()


@pytest.mark.parametrize("count", [1, 63, 64, 65, 128, 333, 840])
def test_chunked_traceback_launches_are_transparent(chunked, count):
    """A three-frame trace budget of 4 MiB (DMND_TRACE_ARENA_MB=8, halved) cuts the call into chunks of whole wavefronts; the
    subsets are the `count` items that keep most columns, so that all but the first three are cut, with chunk ends on (64, 128) and
    off (65, 333, 840) a wavefront boundary of the call."""
    need, meta = chunked["need"], chunked["meta"]
    pick = np.sort(np.argsort(-need, kind="stable")[:count])
    sub, sub_need = [meta[k] for k in pick], need[pick]
    # the launch order: band descending, then target length descending (a stable sort of the call's order)
    order = sorted(range(count), key=lambda k: (-(sub[k][5] - sub[k][4]), -len(sub[k][3])))
    waves = [int(sub_need[order[w:w + 64]].sum()) for w in range(0, count, 64)]
    if count == 840:
        assert need.sum() >= 8 * 4 * MiB, need.sum()
        assert max(waves) > 4 * MiB                         # the `c1 > c0` exception: a first wavefront always goes
    if count >= 65:
        assert sum(waves) > 4 * MiB and len(waves) >= 2      # more than one chunk
    items = chunked["items"][pick]
    out, tr = chunked["small"].frameshift_swipe(items, 0, 15)
    _assert_tracebacks(out, tr, [chunked["want"][k] for k in pick], count)
    out2, tr2 = chunked["large"].frameshift_swipe(items, 0, 15)
    assert out.tobytes() == out2.tobytes() and tr.tobytes() == tr2.tobytes()


# ---- 2. the 1 GiB state limit of a score-only pass -----------------------------------------------------------------------------

def test_score_only_pass_is_cut_at_1_GiB_of_state(ctx):
    """20 wavefronts of items with a nominal band of 50 000 diagonals -- (2 * 150 000 + 5) * 64 * 4 B = 77 MB of interleaved state
    each, the chunk ends once 1 GiB is exceeded: after 14 -- and 100 narrow items at the end of the launch order, in the last
    chunk. The reads are 30-100 codons, so the sweep itself is small. Needs about 1.2 GB of HBM for the state buffer."""
    rng = np.random.default_rng(12)
    M = hip.matrix_of(ctx.params)
    meta = []
    for k in range(1280 + 100):
        n = int(rng.integers(30, 101))
        dna_len = 3 * n + int(rng.integers(0, 3))
        frames = [rng.integers(0, 21, (dna_len - f) // 3).astype(np.int8) for f in range(3)]
        f, at = int(rng.integers(0, 3)), int(rng.integers(0, n - 10))
        t = np.concatenate([rng.integers(0, 20, int(rng.integers(0, 20))), frames[f][at:at + int(rng.integers(8, 100))]]).astype(np.int8)
        mut = rng.random(len(t)) < 0.2
        t[mut] = rng.integers(0, 20, int(mut.sum()))
        d1 = min(at + int(rng.integers(1, 20)), n)
        meta.append((frames, k % 2, dna_len, t, d1 - (50000 if k < 1280 else int(rng.integers(1, 91))), d1))
    assert all(30 <= len(m[0][0]) <= 100 and len(m[3]) <= 120 for m in meta)
    wave = (2 * 3 * 50000 + 5) * 64 * 4
    assert 14 * wave > (1 << 30) >= 13 * wave and 20 * wave > (1 << 30) + wave      # two chunks, the second with the narrow items
    groups, cols = np.arange(len(meta)) // 5, edge_cols(len(meta))
    items = _upload(ctx, meta, groups, cols)
    want, again, _ = oracle_score_only(meta, groups, cols, M, 11, 1, 15, 4)
    assert not any(again) and sum(w[0] > 0 for w in want) > len(meta) // 2
    out, _ = ctx.frameshift_swipe(items, 1, 15, channels=4)
    _assert_scores(out, want)


# ---- 3. saturation at 65535 -----------------------------------------------------------------------------------------------------

def test_saturated_items_are_swept_again_on_their_own_band(ctx, capsys):
    """Reads of about 6 000 tryptophans against themselves, each in a score-only batch of four with three short targets of wider
    bands and smaller d_end: an item whose batch-geometry score reaches 65535 reports the score, max_col and ranges of its own
    geometry, one at 65534 and all batch mates those of the batch geometry. The same items in traceback mode: exact int32 scores
    and transcripts of about 6 000 operations. One lane walks the long item's columns alone; the call times are printed."""
    M = hip.matrix_of(ctx.params)
    sat = saturation_groups()
    meta = [m for _, _, g in sat for m in g]
    groups, cols = np.arange(len(meta)) // 4, np.zeros(len(meta), np.int64)
    want, again, first = oracle_score_only(meta, groups, cols, M, 11, 1, 15, 4)
    long_ = list(range(0, len(meta), 4))
    assert [first[k] for k in long_] == [s for _, s, _ in sat]
    assert sum(again) >= 3 and all(again[k] == (first[k] >= 65535) for k in range(len(meta))) and not any(again[k] for k in range(len(meta)) if k % 4)
    assert any(first[k] == 65535 and again[k] for k in long_) and any(first[k] == 65534 and not again[k] for k in long_)
    assert {meta[k][1] for k in long_ if again[k]} == {0, 1} and {meta[k][1] for k in long_ if not again[k]} == {0, 1}
    for k in long_:                                          # the batch geometry is not the long item's own: the re-run shows
        own = oracle_score_only([meta[k]], [0], [0], M, 11, 1, 15, 4)[0][0]
        assert (own == want[k]) == again[k], k
    items = _upload(ctx, meta, groups, cols)
    t0 = time.perf_counter()
    out, _ = ctx.frameshift_swipe(items, 1, 15, channels=4)
    t1 = time.perf_counter()
    _assert_scores(out, want)
    tb = _tracebacks(meta, M, 11, 1, 15)
    assert [tb[k][0]["score"] for k in long_] == [s for _, s, _ in sat] and all(len(tb[k][1]) > 5900 for k in long_)
    t2 = time.perf_counter()
    out, tr = ctx.frameshift_swipe(items, 0, 15)
    t3 = time.perf_counter()
    _assert_tracebacks(out, tr, tb)
    t4 = time.perf_counter()
    one, _ = ctx.frameshift_swipe(items[4:5], 1, 15, channels=4)      # the 65535 item alone: swept twice on the same band
    t5 = time.perf_counter()
    _assert_scores(one, oracle_score_only([meta[4]], [0], [0], M, 11, 1, 15, 4)[0])
    with capsys.disabled():
        print("\n[frameshift saturation] score-only call of %d items %.1f ms, traceback call %.1f ms, one saturated item alone (two sweeps) %.1f ms"
              % (len(meta), 1e3 * (t1 - t0), 1e3 * (t3 - t2), 1e3 * (t5 - t4)))


# ---- 4. letters above 20, other matrices, other penalties -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def wide():
    return wide_items(240)


@pytest.mark.parametrize("name,go,ge", MATRICES)
def test_letters_above_20_matrices_and_penalties(wide, name, go, ge):
    """Frames and targets with letters 0-25 -- X = 23, stops = 24 at about 1 in 20, the hard-mask letter 25, which is also the
    column a channel scores before its target begins -- under four matrices with their gap penalties (c->params) and frameshift
    penalties 1, 15, 50, traceback and score-only. Letters with bit 7 set (the soft-mask flag) are left out: the reference's
    three-frame sweep indexes its profile (SwipeProfile::get, `data_[(int)letter]`) and the matrix rows of TargetIterator
    (`&matrix8()[32 * letter]`) with the letter as it is, without letter_mask, so a flagged letter would read outside its tables;
    its pipeline hands the sweep translated frames and unmasked targets, and there is nothing in it to agree with."""
    c = _context(params=hip.matrix_params(name, go, ge))
    try:
        M = hip.matrix_of(c.params)
        assert (c.params.gap_open, c.params.gap_extend) == (go, ge)
        groups, cols = np.arange(len(wide)) // 5, edge_cols(len(wide))
        items = _upload(c, wide, groups, cols)
        for fs in (1, 15, 50):
            tb = _tracebacks(wide, M, go, ge, fs)
            want, _, _ = oracle_score_only(wide, groups, cols, M, go, ge, fs, 4)
            assert sum(o["score"] > 0 for o, _ in tb) >= 0.4 * len(wide) and sum(w[0] > 0 for w in want) >= 0.4 * len(wide), (name, fs)
            out, tr = c.frameshift_swipe(items, 0, fs)
            _assert_tracebacks(out, tr, tb, (name, fs))
            out, _ = c.frameshift_swipe(items, 1, fs, channels=4)
            _assert_scores(out, want, (name, fs))
    finally:
        c.close()


# ---- 5. degenerate geometry -----------------------------------------------------------------------------------------------------

def test_degenerate_geometry_enumerated(ctx):
    """Reads of 3-14 nucleotides (frames of 1/0/0, 1/1/0, 1/1/1 .. 4/4/4 letters), targets of 1-4 letters, both strands, every band
    inside the matrix (one-diagonal bands, bands touching either corner), the match planted in each frame: one launch per mode."""
    M = hip.matrix_of(ctx.params)
    meta = degenerate_items()
    tb = _tracebacks(meta, M, 11, 1, 15)
    assert sum(o["score"] > 0 for o, _ in tb) >= len(meta) / 3
    short_end = 0
    for (frames, strand, dna_len, t, d0, d1), (o, _) in zip(meta, tb):
        if o["score"] > 0:
            f = end_frame(o, strand, dna_len)
            short_end += f > 0 and len(frames[f]) < len(frames[0]) and o["q_end"] == len(frames[f])
    assert short_end >= 20
    groups, cols = np.arange(len(meta)) // 7, edge_cols(len(meta))
    items = _upload(ctx, meta, groups, cols)
    out, tr = ctx.frameshift_swipe(items, 0, 15)
    _assert_tracebacks(out, tr, tb)
    for channels in (1, 16):
        want, _, _ = oracle_score_only(meta, groups, cols, M, 11, 1, 15, channels)
        out, _ = ctx.frameshift_swipe(items, 1, 15, channels=channels)
        _assert_scores(out, want, channels)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def valid65():
    rng = np.random.default_rng(33)
    M = hip.matrix_of(hip.default_params())
    meta = []
    while len(meta) < 65:
        frames, dna_len, t, d0, d1 = _random_case(rng, M)
        meta.append((frames, len(meta) % 2, dna_len, t, d0, d1))
    qb, tb, items = _items(meta, np.arange(65) // 5, edge_cols(65))
    return dict(qb=qb, tb=tb, items=items, want=_tracebacks(meta, M, 11, 1, 15))


def _raw_call(c, items, score_only=0, frame_shift=15, channels=16, cap=None):
    """dmnd_frameshift_swipe as the C caller sees it -> (code, out, transcript arena, transcript_used)"""
    out = np.zeros(max(len(items), 1), dtype=hip.FS_HSP_DTYPE)
    full = int((2 * items["target_len"].astype(np.int64) + items["frame_len"][:, 0] + 65).sum()) + 16
    tr = np.zeros(full, np.uint8)
    used = ctypes.c_int64(99)
    rc = c.lib.dmnd_frameshift_swipe(c.h, items.ctypes.data, len(items), score_only, frame_shift, channels, out.ctypes.data, tr.ctypes.data,
                                     full if cap is None else cap, ctypes.byref(used))
    return rc, out[:len(items)], tr, used.value


def _change(field, value, f=None):
    def apply(items, v65):
        it = items[7:8]
        if f is None:
            it[field] = value(it, v65)
        else:
            it[field][:, f] = value(it, v65)
    return apply


REFUSALS = {
    "target range leaves its block": (dict(), _change("target_off", lambda it, v: len(v["tb"]) - it["target_len"] + 1), -1, "item 7 out of range"),
    "frame range leaves its block": (dict(), _change("frame_off", lambda it, v: len(v["qb"]) - it["frame_len"][:, 2] + 1, 2), -1, "item 7 out of range"),
    "d_end <= d_begin": (dict(), _change("d_end", lambda it, v: it["d_begin"]), -1, "item 7 out of range"),
    "band of 65537": (dict(), _change("d_begin", lambda it, v: it["d_end"] - 65537), -4, "Band size"),
    "channels = 0": (dict(score_only=1, channels=0), None, -1, "bad argument"),
    "frame_shift = 0": (dict(frame_shift=0), None, -1, "bad argument"),
    "frame lengths two apart": (dict(), _change("frame_len", lambda it, v: it["frame_len"][:, 0] - 2, 2), -1, "item 7 out of range"),
}


@pytest.mark.parametrize("case", list(REFUSALS) + ["transcript arena one byte short"])
def test_refusals_leave_the_context_usable(ctx, valid65, case):
    """The documented code (DMND_E_ARG -1, DMND_E_BAND -4, DMND_E_CAP -5) and a message; then a valid 65-item call on the same
    context equals the oracle. All refusals are host-side checks before a launch or after the last one."""
    ctx.upload_block(hip.QUERY, valid65["qb"])
    ctx.upload_block(hip.TARGET, valid65["tb"])
    items = valid65["items"].copy()
    assert items["frame_len"][7, 0] >= 2 and items["target_len"][7] >= 1
    if case in REFUSALS:
        kw, change, code, msg = REFUSALS[case]
        if change:
            change(items, valid65)
            assert items[7].tobytes() != valid65["items"][7].tobytes() and items[:7].tobytes() == valid65["items"][:7].tobytes()
        rc, _, _, used = _raw_call(ctx, items, **kw)
    else:
        rc, out, tr, full = _raw_call(ctx, items)
        assert rc == 0 and full == sum(len(otr) + 1 for o, otr in valid65["want"] if o["score"] > 0)
        assert _raw_call(ctx, items, cap=full)[0] == 0         # exactly enough is enough
        code, msg = -5, "transcript arena too small"
        rc, _, _, used = _raw_call(ctx, items, cap=full - 1)
    assert rc == code and used == 0, (case, rc, used)
    assert msg in ctx.lib.dmnd_last_error().decode(), ctx.lib.dmnd_last_error()
    rc, out, tr, used = _raw_call(ctx, valid65["items"])
    assert rc == 0
    _assert_tracebacks(out, tr[:used], valid65["want"], case)


def test_call_without_blocks_is_refused_and_empty_call_is_ok(valid65):
    c = _context()
    try:
        rc, _, _, used = _raw_call(c, valid65["items"])
        assert rc == -1 and used == 0 and "sequence blocks not uploaded" in c.lib.dmnd_last_error().decode()
        c.upload_block(hip.QUERY, valid65["qb"])
        rc, _, _, used = _raw_call(c, valid65["items"])        # one of the two is not enough
        assert rc == -1 and used == 0 and "sequence blocks not uploaded" in c.lib.dmnd_last_error().decode()
        c.upload_block(hip.TARGET, valid65["tb"])
        for score_only in (0, 1):
            rc, _, _, used = _raw_call(c, valid65["items"][:0], score_only=score_only)
            assert rc == 0 and used == 0
        rc, out, tr, used = _raw_call(c, valid65["items"])
        assert rc == 0
        _assert_tracebacks(out, tr[:used], valid65["want"])
    finally:
        c.close()
