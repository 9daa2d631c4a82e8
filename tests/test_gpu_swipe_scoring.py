"""-m gpu: the banded Smith-Waterman kernels (csrc/swipe16_kernels.hip, csrc/swipe_kernels.hip with traceback_walk_wave) under the 14
scoring systems of tests/scoring_schemes.py -- the eight matrices with their default gap costs and six rows at the edges of the gap
table -- one context per system. What only the .hip files hold and no CPU emulator runs: the LDS score tables built from the context's
matrix, the launchers' class routing, the 32-bit re-run of saturated items, the sweep over several wavefronts and the wave walk's own
gap accounting and stop rule. Every comparison is integer-exact against oracle/banded_swipe.c called with the same matrix and gap
costs: score, coordinate, traceback and statistics (510) modes, every field, every transcript byte and the terminator. A failure
names the system, the item's class tag and the field. Every count a test relies on is asserted in it from the oracle's results."""
import functools
import itertools

import numpy as np
import pytest
import torch

import oracle_py as orc
import scoring_schemes as ss
from diamond_amd import hip
from gpu_util import pack_records_m
from test_gpu_swipe import STAT_KEYS

pytestmark = pytest.mark.gpu

KEYS = "score q_begin q_end s_begin s_end length identities mismatches positives gap_openings gaps transcript_len".split()
INS, DEL = 1, 2
W = 17
# (tag, narrowest band, widest band, class without the row classes, class with them)
CLASSES = (("rows 3", 1, 96, 1, 3), ("P 1", 97, 128, 1, 1), ("rows 5", 129, 160, 2, 5), ("P 2", 161, 256, 2, 2), ("P 4", 257, 512, 4, 4),
           ("32-bit 8", 513, 1024, 8, 8), ("32-bit 16", 1025, 2048, 16, 16), ("32-bit 32", 2049, 4096, 32, 32))
PER_CLASS = 31
WAVEFRONTS_BAND, WAVEFRONTS_LEN = 4200, 2200
ORDER_SCHEMES = (("blosum80", 25, 2), ("pam250", 11, 3))
SAT_SCORES = (32766, 32767, 32768)
SAT_BANDS = ((-20, 21), (-60, 60), (-70, 80), (-150, 150))       # rows 3 / P 1 / rows 5 / P 4: the 32-bit re-run in classes 1, 1, 2, 4


@pytest.fixture(scope="module", params=ss.GPU, ids=ss.scheme_id)
def system(request):
    """(scheme, context on its params, its matrix)"""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    scheme = request.param
    x = hip.Context(params=ss.params(scheme))
    yield scheme, x, ss.matrix(scheme[0])
    x.close()


def _rec(q, t, d0, d1, tag, cbs=None, matrix=None, related=False):
    return {"query": q, "cbs": cbs, "tag": tag, "related": related, "targets": [{"seq": t, "d_begin": int(d0), "d_end": int(d1), "matrix": matrix}]}


def _dress(rng, k, q, t, own):
    """a third of the items with a bias, a quarter with a matrix of their own (those take no bias), a fifth with odd letters"""
    if k % 5 == 2:
        ss.odd_letters(rng, q, t)
    matrix = own if k % 4 == 3 else None
    cbs = ss.bias(rng, len(q)) if k % 9 < 4 and matrix is None else None        # 4/9 of the three quarters that are left
    return cbs, matrix


@functools.lru_cache(maxsize=None)
def class_items(scheme):
    """About 250 items of 150 - 400 letters, PER_CLASS per band class: two of three by the gapped recipe (its band [-40, 41) widened
    to the class), one of three an unrelated pair with a band anywhere; and one pair of 2200 letters on a band of 4200 diagonals"""
    name = scheme[0]
    rng = np.random.default_rng(ss.row_seed(*scheme))
    own = np.array(ss.matrix(ss.other_matrix(name)))
    recs, k = [], 0
    for tag, lo, hi, _, _ in CLASSES:
        for n in range(PER_CLASS):
            if n % 3 != 2:
                q, t = ss.gapped_pair(rng)
                need = ss.GAPPED_BAND[1] - ss.GAPPED_BAND[0]
                w = int(rng.integers(max(lo, need), hi + 1))
                d0 = ss.GAPPED_BAND[0] - int(rng.integers(0, w - need + 1))
                kind = "related"
            else:
                q, t = ss.unrelated_pair(rng)
                w = int(rng.integers(lo, hi + 1))
                d0 = int(rng.integers(-(len(t) - 1) - w + 1, len(q)))                # any band that meets the matrix
                kind = "unrelated"
            cbs, matrix = _dress(rng, k, q, t, own)
            what = "own " + ss.other_matrix(name) if matrix is not None else "bias" if cbs is not None else "plain"
            recs.append(_rec(q, t, d0, d0 + w, "%s/%s/%s/%d" % (tag, kind, what, n), cbs, matrix, kind == "related"))
            k += 1
    n = WAVEFRONTS_LEN
    q = rng.integers(0, 20, n).astype(np.int8)
    t = q.copy()
    mut = rng.random(n) < 0.15
    t[mut] = rng.integers(0, 20, int(mut.sum()))
    t = np.concatenate([t[:700], rng.integers(0, 20, 6).astype(np.int8), t[700:1500], t[1507:]])
    recs.append(_rec(q, t, -WAVEFRONTS_BAND // 2, WAVEFRONTS_BAND // 2, "several wavefronts/related/bias/0", ss.bias(rng, n), None, True))
    return tuple(recs)


def _oracle(recs, scheme):
    M, (_, go, ge) = ss.matrix(scheme[0]), scheme
    out = []
    for rec in recs:
        t = rec["targets"][0]
        m = M if t["matrix"] is None else t["matrix"]
        rc, o, tr = orc.banded_swipe(rec["query"], rec["cbs"], t["seq"], t["d_begin"], t["d_end"], m, go, ge, orc.TRACEBACK)
        assert rc == 0, rec["tag"]
        rc, st = orc.swipe_stats(rec["query"], rec["cbs"], t["seq"], t["d_begin"], t["d_end"], m, go, ge, 510)
        assert rc == 0, rec["tag"]
        out.append((o, tr, st))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def class_oracle(scheme):
    return _oracle(class_items(scheme), scheme)


def _upload(ctx, recs):
    qb, tb, cbs, items, _, mats = pack_records_m(recs)
    ctx.upload_block(hip.QUERY, qb)
    ctx.upload_block(hip.TARGET, tb)
    ctx.upload_cbs(cbs)
    ctx.upload_matrices(mats)
    return items


def _check_traceback(recs, ref, out, tr, what):
    for k, rec in enumerate(recs):
        o, otr, _ = ref[k]
        g, tag = out[k], rec["tag"]
        assert g["score"] == o["score"], (what, tag, "score", int(g["score"]), o["score"])
        off, n = int(g["transcript_off"]), int(g["transcript_len"])
        if o["score"] > 0:
            for key in KEYS:
                assert g[key] == o[key], (what, tag, key, int(g[key]), o[key])
            assert np.array_equal(tr[off: off + n], otr), (what, tag, "transcript", tr[off: off + n].tolist(), otr.tolist())
        else:
            assert n == 0, (what, tag, "transcript_len", n)
        assert tr[off + n] == 0, (what, tag, "terminator")


def _check_all_modes(ctx, recs, ref, what):
    """the four modes of dmnd_banded_swipe on the uploaded records against the oracle; returns the traceback result"""
    items = _upload(ctx, recs)
    score, _ = ctx.banded_swipe(items, hip.SWIPE_SCORE)
    coords, _ = ctx.banded_swipe(items, hip.SWIPE_COORDS)
    out, tr = ctx.banded_swipe(items, hip.SWIPE_TRACEBACK)
    stats, _ = ctx.banded_swipe(items, hip.SWIPE_STATS, 510)
    ctx.upload_matrices(np.zeros((0, 32, 32), np.int8))
    for k, rec in enumerate(recs):
        o, _, st = ref[k]
        tag = rec["tag"]
        assert score[k]["score"] == o["score"], (what, tag, "score-only score", int(score[k]["score"]), o["score"])
        assert coords[k]["score"] == o["score"], (what, tag, "coordinate-mode score", int(coords[k]["score"]), o["score"])
        assert stats[k]["score"] == st["score"], (what, tag, "statistics score", int(stats[k]["score"]), st["score"])
        if o["score"] > 0:
            assert (coords[k]["q_end"], coords[k]["s_end"]) == (o["q_end"], o["s_end"]), (what, tag, "end cell", coords[k], o)
            for key in STAT_KEYS:
                assert stats[k][key] == st[key], (what, tag, "statistics " + key, int(stats[k][key]), st[key])
    _check_traceback(recs, ref, out, tr, what)
    return items, out, tr


def _class_of(width, rows):
    for _, lo, hi, p, pr in CLASSES:
        if lo <= width <= hi:
            return pr if rows else p
    return 64


def assert_class_corpus(recs, ref):
    """From the oracle alone: every class has four items and more with a positive score, nine of ten related items open a gap, both
    gap directions occur, and items with a bias, a matrix of their own and odd letters are all there"""
    positive = {}
    for rec, (o, _, _) in zip(recs, ref):
        tag = rec["tag"].split("/")[0]
        positive[tag] = positive.get(tag, 0) + (o["score"] > 0)
    assert set(positive) == {c[0] for c in CLASSES} | {"several wavefronts"}, positive
    assert all(n >= 4 for t, n in positive.items() if t != "several wavefronts") and positive["several wavefronts"] == 1, positive
    related = [(rec, o, tr) for rec, (o, tr, _) in zip(recs, ref) if rec["related"]]
    assert len(related) >= 150 and all(o["score"] > 0 for _, o, _ in related)
    gapped = sum(o["gap_openings"] > 0 for _, o, _ in related)
    assert 10 * gapped >= 9 * len(related), (gapped, len(related))
    ops = {int(b) >> 6 for _, _, tr in related for b in tr}
    assert {INS, DEL} <= ops, ops
    assert sum(r["cbs"] is not None for r in recs) >= 75 and sum(r["targets"][0]["matrix"] is not None for r in recs) >= 60
    assert sum(bool((r["query"] < 0).any()) for r in recs) >= 40
    wide = recs[-1]["targets"][0]
    assert wide["d_end"] - wide["d_begin"] > 4096 and ref[-1][0]["gap_openings"] >= 2, ref[-1][0]


@pytest.mark.parametrize("rows", ["0", "1"])
def test_every_band_class_equals_the_oracle(system, rows, monkeypatch):
    """Every launch class -- the packed sweeps' 1, 2, 4 and the row classes 3, 5, the 32-bit kernels' 8, 16, 32 (and 1 - 32 for
    the items with a matrix of their own, another standard matrix under the context's gap costs), one band of several
    wavefronts; the statistics call sweeps bands from 2049 with several wavefronts"""
    scheme, ctx, _ = system
    monkeypatch.setenv("DMND_SWEEP_ROWS", rows)
    recs, ref = class_items(scheme), class_oracle(scheme)
    assert_class_corpus(recs, ref)
    want = {3, 1, 5, 2, 4, 8, 16, 32, 64} if rows == "1" else {1, 2, 4, 8, 16, 32, 64}
    assert {_class_of(r["targets"][0]["d_end"] - r["targets"][0]["d_begin"], rows == "1") for r in recs} == want
    _check_all_modes(ctx, recs, ref, "%s, rows %s" % (ss.scheme_id(scheme), rows))


# ---- saturation --------------------------------------------------------------------------------------------------------------------

def saturating_pair(M, score):
    """Identical sequences of the exact self score `score`: a run of W (the matrix's W:W entry per column) and at most three
    further letters behind it, found by search over the matrix's diagonal"""
    d = int(M[W, W])
    diag = [int(M[a, a]) for a in range(20)]
    for n_extra in range(4):
        for extra in itertools.combinations_with_replacement(range(20), n_extra):
            rest = score - sum(diag[a] for a in extra)
            if rest > 0 and rest % d == 0 and W not in extra:
                s = np.array([W] * (rest // d) + list(extra), np.int8)
                return s, s.copy()
    raise AssertionError("no run of W and three letters scores %d" % score)


@functools.lru_cache(maxsize=None)
def saturation_items(scheme):
    M = ss.matrix(scheme[0])
    rng = np.random.default_rng(ss.row_seed(*scheme) + 7)
    recs = []
    for k in range(9):
        q, t = ss.gapped_pair(rng) if k % 3 else ss.unrelated_pair(rng, 20, 200)
        w = int(rng.integers(81, 200))
        recs.append(_rec(q, t, -40 - (w - 81) // 2, -40 - (w - 81) // 2 + w, "neighbour/%d" % k, ss.bias(rng, len(q)) if k % 2 else None, None, k % 3 != 0))
    big = np.full(3400, W, np.int8)
    sat = [saturating_pair(M, s) for s in SAT_SCORES] + [(big, big.copy())]
    for k, ((q, t), (d0, d1), at) in enumerate(zip(sat, SAT_BANDS, (2, 3, 7, 9))):
        recs.insert(at + k, _rec(q, t, d0, d1, "sat/%s" % (SAT_SCORES + ("above",))[k]))
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def saturation_oracle(scheme):
    return _oracle(saturation_items(scheme), scheme)


@pytest.mark.parametrize("rows", ["0", "1"])
def test_scores_around_the_16_bit_limit(system, rows, monkeypatch):
    """Self scores of exactly 32766 (the largest the packed sweep holds), 32767 and 32768 (both re-run in 32 bits) and one far
    above, built from the matrix's own W:W entry, in one batch with nine ordinary items, which must not be disturbed"""
    scheme, ctx, M = system
    monkeypatch.setenv("DMND_SWEEP_ROWS", rows)
    recs, ref = saturation_items(scheme), saturation_oracle(scheme)
    assert int(M[W, W]) in (11, 13, 15, 17)
    got = {rec["tag"]: o["score"] for rec, (o, _, _) in zip(recs, ref) if rec["tag"].startswith("sat/")}
    assert [got["sat/%d" % s] for s in SAT_SCORES] == list(SAT_SCORES) and got["sat/above"] >= 35000, got
    assert len(recs) == 13 and sum(o["score"] > 0 for _, (o, _, _) in zip(recs, ref)) >= 10
    for rec in recs:
        if rec["tag"].startswith("sat/") and rec["tag"] != "sat/above":
            assert len(rec["query"]) - int((rec["query"] == W).sum()) <= 3
    _check_all_modes(ctx, recs, ref, "%s, rows %s" % (ss.scheme_id(scheme), rows))


# ---- order and arena ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scheme", ORDER_SCHEMES, ids=ss.scheme_id)
def test_shuffled_order_and_a_small_trace_arena(scheme, monkeypatch):
    """The class batch in another order (other items share a wavefront and a launch) gives the same records; a context with a
    trace arena of 64 MB (more chunks) gives the same bytes"""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    recs, ref = class_items(scheme), class_oracle(scheme)
    order = np.random.default_rng(5).permutation(len(recs))
    shuffled, sref = [recs[k] for k in order], [ref[k] for k in order]
    what = ss.scheme_id(scheme)
    ctx = hip.Context(params=ss.params(scheme))
    try:
        items = _upload(ctx, recs)
        out, tr = ctx.banded_swipe(items, hip.SWIPE_TRACEBACK)
        _check_traceback(recs, ref, out, tr, what)
        sitems = _upload(ctx, shuffled)
        sout, str_ = ctx.banded_swipe(sitems, hip.SWIPE_TRACEBACK)
        _check_traceback(shuffled, sref, sout, str_, what + ", shuffled")
        for name in out.dtype.names:
            if name != "transcript_off":
                assert np.array_equal(sout[name], out[name][order]), (what, "shuffled", name)
    finally:
        ctx.close()
    monkeypatch.setenv("DMND_TRACE_ARENA_MB", "64")
    small = hip.Context(params=ss.params(scheme))
    monkeypatch.delenv("DMND_TRACE_ARENA_MB")
    try:
        items = _upload(small, recs)
        aout, atr = small.banded_swipe(items, hip.SWIPE_TRACEBACK)
    finally:
        small.close()
    assert np.array_equal(aout, out) and np.array_equal(atr, tr), (what, "64 MB arena")
