"""-m gpu: the Hauser bias dmnd_extend keeps in HBM between calls (extend_front, csrc/extend_host.hip: reused while cbs_generation ==
query_generation and cbs_len == the query block's end). Every entry that changes the query block's letters, or puts another bias
into the buffer, has to invalidate it -- dmnd_upload_block, dmnd_share_block, dmnd_copy_block, the masking entries, dmnd_upload_cbs,
dmnd_xdrop_ungapped -- and a stale bias gives plausible, wrong scores. One long-lived context goes through all of them on the
block pair of tests/golden/ext_default.tap; after every step its dmnd_extend records equal, field for field, those of a fresh
context that has seen only the step's final state. The first records also equal the reference's Match lists (as test_gpu_extend.py).
That a stale bias would show: the records without bias differ, the other block's bias differs at most positions, and the cached
buffer is read directly through dmnd_gapped_filter's first-stage score against the oracle with the host's bias."""
import os
import numpy as np
import pytest
import torch

import oracle_py as orc
from tapfile import read_ext_tap
from diamond_amd import hip, workload
from test_gpu_seed import to_hip_params
from test_oracle_seed import blosum62_matrix8

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HSP_KEYS = "score q_begin q_end s_begin s_end length identities mismatches gap_openings gaps".split()


class State:
    """what a context is given before dmnd_extend: the two blocks, the seed hits, --comp-based-stats"""

    def __init__(self, qd, ql, td, tl, hits, mode=1):
        self.qd, self.ql, self.td, self.tl, self.hits, self.mode = qd, ql, td, tl, hits, mode

    def but(self, **kw):
        s = State(self.qd, self.ql, self.td, self.tl, self.hits, self.mode)
        for k, v in kw.items():
            setattr(s, k, v)
        return s


def _settings(ctx, s):
    ctx.set_db_letters(float(s.tl[-1] - s.tl[0] - (len(s.tl) - 1)))
    ctx.set_gapped_filter(0.0)
    ctx.set_query_contexts(1)
    ctx.set_comp_based_stats(s.mode)


def _give(ctx, s):
    ctx.upload_block(hip.QUERY, s.qd, s.ql)
    ctx.upload_block(hip.TARGET, s.td, s.tl)
    _settings(ctx, s)


def _fresh(s):
    ctx = hip.Context()
    try:
        _give(ctx, s)
        return ctx.extend(s.qd, s.td, s.hits, threads=4)[0]
    finally:
        ctx.close()


def _fields(a, b, dtype, path=""):
    for name in dtype.names:
        if dtype[name].names:
            yield from _fields(a[name], b[name], dtype[name], path + name + ".")
        else:
            yield path + name, a[name], b[name]


def _equal(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for name, g, w in _fields(got, want, got.dtype):
        if name.endswith("transcript_off"):                  # no transcript arena in these calls: the field has no meaning
            continue
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: field %s of %d records differs from a fresh context's; first: record %d (query %d, target %d): %s, fresh %s" % (
            what, name, len(bad), bad[0], got["query"][bad[0]], got["target"][bad[0]], g[bad[0]], w[bad[0]])


def _step(ctx, s, what):
    """dmnd_extend on the long-lived context (already in state s) against a fresh context given s"""
    got = ctx.extend(s.qd, s.td, s.hits, threads=4)[0]
    _equal(got, _fresh(s), what)
    assert len(got) > 100, what
    return got


def _reversed(data, limits):
    out = data.copy()
    for a, b in zip(limits[:-1], limits[1:]):
        out[a:b - 1] = data[a:b - 1][::-1]
    return out


def _other_queries(data, limits):
    """A query block of the same limits and other letters: every sequence reversed, and three letters in ten replaced by the
    sequence's most frequent residue. Reversal alone moves the bias at 27 % of the positions of this block (83 % of them have
    bias 0 either way); the skewed composition moves it at 63 %, and the mirrored targets still align."""
    out = _reversed(data, limits)
    rng = np.random.default_rng(9)
    for a, b in zip(limits[:-1], limits[1:]):
        seq = out[a:b - 1]
        std = seq[(seq & 31) < 20] & 31
        seq[rng.random(len(seq)) < 0.3] = np.bincount(std, minlength=20).argmax() if len(std) else 0
    return out


def _mirror(base):
    """the other query block, every target reversed, and the seed hits in the reversed coordinates: the mirror images of the alignments"""
    return base.but(qd=_other_queries(base.qd, base.ql), td=_reversed(base.td, base.tl), hits=_mirrored(base.hits, base.ql, base.tl))


def _mirrored(hits, ql, tl):
    """the same seed hits in the coordinates of the blocks with every sequence reversed"""
    out = hits.copy()
    q = hits["query"].astype(np.int64)
    t = np.searchsorted(tl, hits["subject"], side="right") - 1
    out["seed_offset"] = (ql[q + 1] - ql[q] - 1) - 1 - hits["seed_offset"]
    out["subject"] = tl[t] + (tl[t + 1] - 1 - 1 - hits["subject"])
    return out[np.lexsort((out["seed_offset"], out["subject"], out["query"]))]


def _host_bias(s):
    return hip.extend_plan(hip.default_params(), s.qd, s.ql, s.td, s.tl, np.zeros(0, hip.SEED_HIT_DTYPE))[0]


@pytest.fixture(scope="module")
def world():
    assert torch.cuda.is_available()
    cfg, recs = read_ext_tap(os.path.join(GOLDEN, "ext_default.tap"))
    assert cfg["gapped_filter_evalue"] == 0 and cfg["query_contexts"] == 1
    qd, ql, td, tl = cfg["query"]["data"], cfg["query"]["limits"], cfg["target"]["data"], cfg["target"]["limits"]
    ctx = hip.Context()
    base = State(np.ascontiguousarray(qd, np.int8), np.asarray(ql, np.int64), np.ascontiguousarray(td, np.int8), np.asarray(tl, np.int64), None)
    _give(ctx, base)
    base.hits = ctx.seed_search(to_hip_params(cfg))
    yield ctx, base, recs
    ctx.close()


def test_first_call_equals_the_reference_and_a_second_call_reuses_the_bias(world):
    ctx, base, recs = world
    _give(ctx, base)
    m = _step(ctx, base, "first call")
    pos = 0
    for r in sorted(recs, key=lambda x: x["query_id"]):
        for ref in r["matches"]:
            got = m[pos]
            pos += 1
            assert (got["query"], got["target"]) == (r["query_id"], ref["target_block_id"])
            for k in HSP_KEYS:
                assert got["hsp"][k] == ref["hsps"][0][k], (k, r["query_id"], ref["target_block_id"])
            assert got["ungapped_score"] == ref["ungapped_score"]
    assert pos == len(m) > 300
    again = _step(ctx, base, "the same call again")
    _equal(again, m, "the same call again, against the first")


def test_a_stale_bias_would_be_seen(world):
    ctx, base, _ = world
    _give(ctx, base)
    with_bias = _step(ctx, base, "mode 1")
    ctx.set_comp_based_stats(0)
    without = _step(ctx, base.but(mode=0), "--comp-based-stats 0")
    ctx.set_comp_based_stats(1)
    back = _step(ctx, base, "--comp-based-stats 1 again")
    _equal(back, with_bias, "--comp-based-stats 1 again, against the call before")
    key = lambda m: set(zip(m["query"].tolist(), m["target"].tolist(), m["hsp"]["score"].tolist(), m["hsp"]["q_begin"].tolist(), m["hsp"]["q_end"].tolist()))
    assert len(key(with_bias) ^ key(without)) >= 20
    a, b = _host_bias(base), _host_bias(_mirror(base))
    letters = (base.qd & 31) != 31
    assert int((a[letters] != b[letters]).sum()) > letters.sum() // 2


def _gapped_first_stage(ctx, s, n=200):
    """the cached buffer read directly: the gapped filter's first-stage score (window 64, band 100) with the bias in HBM"""
    ctx.set_gapped_filter(1.0)
    try:
        index = np.random.default_rng(5).permutation(len(s.hits))[:n]
        index.sort()
        hits = s.hits[index]
        _, scores = ctx.gapped_filter(hits, use_cbs=True, with_scores=True)
    finally:
        ctx.set_gapped_filter(0.0)
    cbs = _host_bias(s)
    m8 = blosum62_matrix8()
    changed = 0
    for x, h in enumerate(hits):
        qi = int(h["query"])
        ti = int(np.searchsorted(s.tl, h["subject"], side="right") - 1)
        q, c = s.qd[s.ql[qi]:s.ql[qi + 1] - 1], cbs[s.ql[qi]:s.ql[qi + 1] - 1]
        t = s.td[s.tl[ti]:s.tl[ti + 1] - 1]
        hi, hj = int(h["seed_offset"]), int(h["subject"] - s.tl[ti])
        want = orc.gapped_filter_hit(m8, q, c, t, hi, hj, 64, 100, 20)
        assert scores[x, 0] == want, (x, qi, ti, hi, hj)
        changed += int(want != orc.gapped_filter_hit(m8, q, None, t, hi, hj, 64, 100, 20))
    assert changed > n // 4                                 # the bias matters to these scores


def test_another_block_of_the_same_shape_then_the_first_again(world):
    ctx, base, _ = world
    _give(ctx, base)
    _step(ctx, base, "original block")
    _gapped_first_stage(ctx, base)
    # every sequence of both blocks reversed: the alignments are the mirror images, the limits are the same, the bias is another
    mirror = _mirror(base)
    ctx.upload_block(hip.QUERY, mirror.qd, mirror.ql)
    ctx.upload_block(hip.TARGET, mirror.td, mirror.tl)
    _step(ctx, mirror, "both blocks reversed")
    _gapped_first_stage(ctx, mirror)
    # the reversed queries alone, against the targets as they were
    half = base.but(qd=mirror.qd)
    ctx.upload_block(hip.TARGET, base.td, base.tl)
    got = ctx.extend(half.qd, half.td, half.hits, threads=4)[0]
    _equal(got, _fresh(half), "query block reversed")
    ctx.upload_block(hip.QUERY, base.qd, base.ql)
    _step(ctx, base, "original block restored")
    _gapped_first_stage(ctx, base)


def test_a_longer_and_a_shorter_query_block(world):
    ctx, base, _ = world
    _give(ctx, base)
    _step(ctx, base, "original block")
    n = len(base.ql) - 1
    seqs = [base.qd[a:b - 1] for a, b in zip(base.ql[:-1], base.ql[1:])]

    def block(seqs):
        off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
        return workload.sequence_set(np.concatenate(seqs).astype(np.int8), off)

    extra = n // 2 + 7
    qd, ql = block(seqs + [x[::-1] for x in seqs[:extra]])                  # the bias buffer has to grow
    assert np.array_equal(ql[:n + 1], base.ql)
    longer = base.but(qd=qd, ql=ql)
    ctx.upload_block(hip.QUERY, qd, ql)
    _step(ctx, longer, "longer query block")
    keep = n // 2
    qd, ql = block([x[::-1] if k % 2 else x for k, x in enumerate(seqs[:keep])])      # same limits as far as it goes, other letters
    shorter = base.but(qd=qd, ql=ql, hits=base.hits[base.hits["query"] < keep])
    ctx.upload_block(hip.QUERY, qd, ql)
    _step(ctx, shorter, "shorter query block")
    ctx.upload_block(hip.QUERY, base.qd, base.ql)
    _step(ctx, base, "original block restored")


def test_a_bias_of_the_callers_and_other_users_of_the_buffer(world):
    ctx, base, _ = world
    _give(ctx, base)
    first = _step(ctx, base, "original block")
    ctx.upload_cbs(np.full(int(base.ql[-1]), 5, np.int8))
    _step(ctx, base, "after dmnd_upload_cbs of a vector of +5")
    ctx.upload_cbs(np.zeros(0, np.int8))
    _step(ctx, base, "after dmnd_upload_cbs of nothing")
    some = base.hits[:: max(1, len(base.hits) // 3000)]
    ctx.xdrop_ungapped(some, use_bias=True)
    _step(ctx, base, "after dmnd_xdrop_ungapped with the bias")
    ctx.xdrop_ungapped(some, use_bias=False)
    _step(ctx, base, "after dmnd_xdrop_ungapped without the bias")
    ctx.set_gapped_filter(1.0)
    ctx.gapped_filter(some, use_cbs=True)
    ctx.gapped_filter(some, use_cbs=False)
    ctx.set_gapped_filter(0.0)
    last = _step(ctx, base, "after dmnd_gapped_filter")
    _equal(last, first, "after dmnd_gapped_filter, against the first call")


def test_masking_the_query_block_in_place(world):
    ctx, base, _ = world
    # tandem repeats planted into the twenty queries with the most seed hits: tantan has something to mask where the extension looks
    counts = np.bincount(base.hits["query"], minlength=len(base.ql) - 1)
    lens = np.diff(base.ql) - 1
    ids = [int(q) for q in np.argsort(-counts) if lens[q] >= 120][:20]
    qd = base.qd.copy()
    for q in ids:
        qd[base.ql[q] + 30: base.ql[q] + 90] = np.resize(np.array([5, 15, 9], np.int8), 60)
    planted = base.but(qd=qd)
    _give(ctx, planted)
    _step(ctx, planted, "repeats planted")
    host = qd.copy()
    n1 = ctx.mask_sequences(hip.QUERY, host, np.array(ids[:7], np.int32))
    assert n1 >= 7 * 30
    masked = ctx.download_block(hip.QUERY, len(qd))
    assert np.array_equal(masked, host) and int((masked != qd).sum()) == n1
    some = planted.but(qd=masked)
    assert int((_host_bias(some) != _host_bias(planted)).sum()) >= 100
    _step(ctx, some, "after dmnd_mask_sequences")
    n2 = ctx.mask_block(hip.QUERY, host)
    assert n2 >= 20 * 30
    masked = ctx.download_block(hip.QUERY, len(qd))
    assert np.array_equal(masked, host)
    every = planted.but(qd=masked)
    assert int((_host_bias(every) != _host_bias(some)).sum()) >= 100
    _step(ctx, every, "after dmnd_mask_block")
    ctx.soft_mask_block(hip.QUERY)                           # builds the view seeds are drawn from; the block itself stays
    assert np.array_equal(ctx.download_block(hip.QUERY, len(qd)), masked)
    _step(ctx, every, "after dmnd_soft_mask_block")
    # SEG on the device writes into the block as well: the planted block again, its runs of three residues are low-complexity
    ctx.upload_block(hip.QUERY, qd, base.ql)
    _step(ctx, planted, "repeats planted again")
    host = qd.copy()
    n3 = ctx.seg_mask_block(hip.QUERY, host)
    assert n3 >= 20 * 30
    masked = ctx.download_block(hip.QUERY, len(qd))
    assert np.array_equal(masked, host)
    seg = planted.but(qd=masked)
    assert int((_host_bias(seg) != _host_bias(planted)).sum()) >= 100
    _step(ctx, seg, "after dmnd_seg_mask_block_device")
    ctx.upload_block(hip.QUERY, base.qd, base.ql)
    _step(ctx, base, "original block restored")


def test_a_query_block_copied_and_shared_from_another_context(world):
    ctx, base, _ = world
    _give(ctx, base)
    _step(ctx, base, "original block")
    mirror = _mirror(base)
    other, third = hip.Context(), hip.Context()
    try:
        other.upload_block(hip.QUERY, mirror.qd, mirror.ql)                  # a different block of the same shape
        third.upload_block(hip.QUERY, base.qd, base.ql)
        for entry, take in (("dmnd_copy_block", ctx.copy_block), ("dmnd_share_block", ctx.share_block)):
            take(hip.QUERY, other)
            assert np.array_equal(ctx.download_block(hip.QUERY, len(base.qd)), mirror.qd)
            ctx.upload_block(hip.TARGET, mirror.td, mirror.tl)               # the mirrored targets: as many alignments as before
            _step(ctx, mirror, "after %s of the reversed block" % entry)
            take(hip.QUERY, third)
            ctx.upload_block(hip.TARGET, base.td, base.tl)
            _step(ctx, base, "after %s of the original block" % entry)
            ctx.upload_block(hip.QUERY, base.qd, base.ql)                    # its own block again (a shared one is read-only)
            _step(ctx, base, "original block uploaded again")
    finally:
        other.close()
        third.close()
