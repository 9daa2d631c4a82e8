"""-m gpu: the device planner of the extension stage (csrc/plan_kernels.hip) read out through dmnd_extend_plan_device and compared,
group by group and exactly, with the host planner (hip.extend_plan, pinned on the reference's taps by tests/test_extend_plan.py):
 (a) the seed hits of the golden configurations: same rows for the planned groups, in both forms of the chaining (one kernel; the
     small workspace first, DMND_PLAN_SMALL_HITS=0), the gapped filter's pass flags included;
 (b) WHICH groups the device leaves to the host is predicted on the CPU (more than 32 hits, more than 16 segments, the fixed
     16 / 96 / 16 chaining instance overflowing: tests/emu/chain_emu.cpp) and must match in both directions, with the counters;
 (c) a constructed block of a few thousand (query, target) pairs that holds the edges of the planner's arrays and rules -- each
     asserted present from the CPU prediction (_constructed_block / _assert_edges_present run without a GPU) -- under
     DMND_EXTEND_GUARD, in both forms and both band modes, as a whole and as prefixes whose group and chaining-list counts sit on
     the kernels' workgroup boundaries; and a second, small block searched without composition based statistics, whose groups of at
     most 16 segments outgrow the 96 links of the fixed workspace (_overflow_block says why the bias has to be off for that);
 (d) a list with two hits swapped is reported as not planned, and dmnd_extend on it equals the host-planned run.
Every comparison is equality. The expected rows of the slow band mode (the host entry plans in the fast one) come from _bands below,
a restatement of add_dp_targets over the emulator's chains that is itself compared with the host planner's rows in the fast mode.

One edge of the issue's list cannot exist: "a left x-drop walk that carries a later hit's segment in front of an earlier one".
Hits of a diagonal are walked in ascending j, and a kept hit lies behind the end of the segment before it. Walking left from it,
the running best on arrival at the earlier hit is at least what the earlier hit's own walk started from, so the later walk stops no
further left than the earlier one did: its segment begins at or behind the earlier segment's begin, and the second sort of
plan_segments_kernel (a stable sort by (diagonal, begin)) never moves anything. _assert_edges_present checks exactly that on every
group of the block (the emulator's segments with and without the sort are the same lists)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import emu_py as emu
from tapfile import read_ext_tap
from diamond_amd import hip, workload
from test_chain_graph import _run, _pair, _hits
from test_gpu_seed import to_hip_params

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
TAPS = ["ext_fast_synth.tap", "ext_default_synth.tap", "ext_default.tap", "ext_rank.tap", "ext_bjz.tap", "ext_long.tap", "ext_sensitive.tap"]
MAX_HITS, MAX_SEGS, SMALL_SEGS = 32, 16, 4          # plan_kernels.h PLAN_MAX_HITS, PLAN_MAX_SEGS; plan_kernels.hip PLAN_SMALL_SEGS
RESORT = 16                                         # emu_chain: sort the segments again before chaining, as the extension stage does


def _band_for(n, fast):                             # Extension::band (extend_host.hip band_for)
    if fast:
        return 12 if n < 50 else 16 if n < 100 else 30 if n < 250 else 40 if n < 350 else 64
    return 15 if n < 50 else 20 if n < 100 else 30 if n < 150 else 50 if n < 200 else 60 if n < 250 else 100 if n < 350 else 120 if n < 500 else 150


def _bands(chains, band, qlen, tlen):
    """add_dp_targets: the chains' bands [d_min - band, d_max + 1 + band) clipped to the matrix, in d_min order (stable), a band
    that overlaps the running one by at least one diagonal merged into it. Returns (bands, gaps): gaps = begin of every later band
    minus the end of the running one before it (0: they touch, -1: they overlap by one)."""
    out, gaps, cur = [], [], None
    for k in sorted(range(len(chains)), key=lambda k: int(chains[k][0])):
        b0, b1 = max(int(chains[k][0]) - band, -(tlen - 1)), min(int(chains[k][1]) + 1 + band, qlen)
        if cur is None:
            cur = [b0, b1]
            continue
        gaps.append(b0 - cur[1])
        if min(cur[1], b1) - max(cur[0], b0) > 0:
            cur = [min(cur[0], b0), max(cur[1], b1)]
        else:
            out.append(tuple(cur))
            cur = [b0, b1]
    if cur is not None:
        out.append(tuple(cur))
    return out, gaps


def _predict(qd, ql, td, tl, hits, cbs, M, fast=True, every_group=False):
    """Per (query, target) group of a sorted hit list, on the CPU: hits, segments, whether the device must plan it, whether the
    small chaining instance fits, and (every_group, or two hits and more) its bands by _bands. every_group = False skips the
    emulator for one-hit groups: the device always plans those."""
    tgt = np.searchsorted(tl, hits["subject"], "right") - 1
    head = np.ones(len(hits), bool)
    head[1:] = (hits["query"][1:] != hits["query"][:-1]) | (tgt[1:] != tgt[:-1])
    begin = np.flatnonzero(head)
    end = np.append(begin[1:], len(hits))
    groups = []
    for b, e in zip(begin, end):
        qi, ti, n = int(hits["query"][b]), int(tgt[b]), int(e - b)
        g = dict(query=qi, target=ti, n_hits=n, begin=int(b), score=int(hits["score"][b:e].astype(np.uint16).max()), n_segs=None, on_host=n > MAX_HITS,
                 need_chain=False, small=False, relist=False, bands=None, gaps=[], same_order=True,
                 qlen=int(ql[qi + 1] - ql[qi] - 1), tlen=int(tl[ti + 1] - tl[ti] - 1))
        groups.append(g)
        if n == 1 and not every_group:
            continue
        q, t = qd[ql[qi]: ql[qi + 1] - 1], td[tl[ti]: tl[ti + 1] - 1]
        bias = cbs[ql[qi]: ql[qi + 1] - 1] if cbs is not None else None
        ij = sorted(((int(h["seed_offset"]), int(h["subject"] - tl[ti])) for h in hits[b:e]), key=lambda x: (x[0] - x[1], x[1]))
        s0, c0 = _run(0 | RESORT, q, bias, t, M, ij)
        g["n_segs"] = len(s0)
        g["same_order"] = np.array_equal(s0, _run(0, q, bias, t, M, ij)[0])
        if n > MAX_HITS:
            continue
        if len(s0) > MAX_SEGS:
            g["on_host"] = True
            continue
        if len(s0) >= 2:
            g["need_chain"] = True
            g["small"] = len(s0) <= SMALL_SEGS
            s2, c2 = _run(2 | RESORT, q, bias, t, M, ij)
            assert np.array_equal(s0, s2)
            if c2 is None:
                g["on_host"] = True
            else:
                assert np.array_equal(c0, c2)
            if g["small"]:
                g["relist"] = _run(3 | RESORT, q, bias, t, M, ij)[1] is None
        if not g["on_host"]:
            g["bands"], g["gaps"] = _bands(c0 if len(s0) else [], _band_for(g["qlen"], fast), g["qlen"], g["tlen"])
    return groups


def _host_rows(p, qd, ql, td, tl, hits):
    """(bias, rows of the host planner in (query, target) order, the order inside a pair kept)"""
    cbs, plan = hip.extend_plan(p, qd, ql, td, tl, hits, threads=4)
    order = np.lexsort((plan["target"], plan["query"]))          # (stable)
    return cbs, plan[order]


def _rows_of(plan, pairs):
    """the rows of `plan` whose (query, target) is in `pairs`"""
    key = plan["query"].astype(np.int64) << 32 | plan["target"]
    want = np.array(sorted(q << 32 | t for q, t in pairs), np.int64)
    return plan[np.isin(key, want)]


def _compare(ctx, hits, pred, host_plan, small_form, passes=None, band_rows=None):
    """One planner call on `hits` against the prediction for exactly these groups. passes: per group, the gapped filter's verdict
    (None: the filter is off). band_rows: take the expected rows from the prediction's bands instead of the host plan."""
    rows, groups, info = ctx.extend_plan_device(hits)
    assert info["planned"] and not info["unsorted"]
    assert info["n_groups"] == len(pred) == len(groups)
    assert info["n_queries"] == len({g["query"] for g in pred})
    assert [(int(a), int(b), int(c)) for a, b, c in zip(groups["query"], groups["target"], groups["n_hits"])] == [(g["query"], g["target"], g["n_hits"]) for g in pred]
    ok = [True] * len(pred) if passes is None else [bool(x) for x in passes]
    assert groups["pass"].astype(bool).tolist() == ok
    want_host = {(g["query"], g["target"]) for g, p in zip(pred, ok) if p and g["on_host"]}
    got_host = {(int(a), int(b)) for a, b, h in zip(groups["query"], groups["target"], groups["on_host"]) if h}
    assert got_host == want_host, (sorted(got_host - want_host)[:5], sorted(want_host - got_host)[:5])
    assert info["n_on_host"] == len(want_host)
    need = [g for g, p in zip(pred, ok) if p and g["need_chain"]]
    relisted = sum(g["relist"] for g in need) if small_form else 0
    assert info["n_relisted"] == relisted
    assert info["n_chain"] + info["n_chain_big"] == len(need) + relisted
    assert info["n_chain"] == (sum(g["small"] for g in need) if small_form else 0)
    planned = [g for g, p in zip(pred, ok) if p and not g["on_host"]]
    if band_rows:
        want = np.array([(g["query"], g["target"], d0, d1, g["score"]) for g in planned for d0, d1 in g["bands"]], dtype=hip.PLAN_DTYPE)
    else:
        want = _rows_of(host_plan, [(g["query"], g["target"]) for g in planned])
    assert info["n_bands"] == len(rows) == len(want)
    assert rows.tobytes() == want.tobytes(), np.flatnonzero(rows != want)[:5]
    for g, passed, r in zip(pred, ok, groups):
        if not passed or g["on_host"]:
            assert r["n_bands"] == 0
    assert int(groups["n_bands"].sum()) == len(rows)
    return rows, groups, info


def _assert_bands_equal_host_rows(pred, host_plan):
    """_bands against the host planner (fast band mode), for every group the prediction chained"""
    key = host_plan["query"].astype(np.int64) << 32 | host_plan["target"]
    lo, hi = np.searchsorted(key, [g["query"] << 32 | g["target"] for g in pred], "left"), np.searchsorted(key, [g["query"] << 32 | g["target"] for g in pred], "right")
    n = 0
    for g, a, b in zip(pred, lo, hi):
        if g["bands"] is not None:
            assert [(int(x["d_begin"]), int(x["d_end"])) for x in host_plan[a:b]] == g["bands"], g
            assert all(int(x["ungapped_score"]) == g["score"] for x in host_plan[a:b])
            n += 1
    return n


def _bias_of(p, q):
    """Hauser bias of one query (the host entry on a block of this one sequence, no hits)"""
    d, lim = workload.sequence_set(np.asarray(q, np.int8), np.array([0, len(q)], np.int64))
    cbs, _ = hip.extend_plan(p, d, lim, d, lim, np.zeros(0, hip.SEED_HIT_DTYPE))
    return cbs[lim[0]: lim[0] + len(q)]


def _matrix():
    p = hip.default_params()
    assert int(np.ceil((12.3 * np.log(2.0) + np.log(p.K)) / p.lambda_)) == 20      # the x-drop the emulator walks with
    return p, hip.matrix_of(p)


# ---- (a), (b): real hits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tap", TAPS)
def test_device_plan_of_real_hits_equals_the_host_plan(tap, monkeypatch):
    assert torch.cuda.is_available()
    cfg, _ = read_ext_tap(os.path.join(GOLDEN, tap))
    assert cfg["query_contexts"] == 1
    qd, ql, td, tl = cfg["query"]["data"], cfg["query"]["limits"], cfg["target"]["data"], cfg["target"]["limits"]
    # (an extension tap carries the seed-stage settings, the gapped filter's e-value and the query contexts, all applied below; it has no
    # gap costs, x-drop or composition mode of its own -- the goldens were minted with the default scoring, which default_params gives)
    p, M = _matrix()
    p.db_letters = float(tl[-1] - tl[0] - (len(tl) - 1))
    gf_on = cfg["gapped_filter_evalue"] > 0
    assert gf_on == (tap == "ext_sensitive.tap")
    seen = []
    for small_form in (False, True):
        if small_form:
            monkeypatch.setenv("DMND_PLAN_SMALL_HITS", "0")
        ctx = hip.Context(params=p)
        try:
            ctx.upload_block(hip.QUERY, qd, ql)
            ctx.upload_block(hip.TARGET, td, tl)
            ctx.set_db_letters(p.db_letters)
            ctx.set_gapped_filter(cfg["gapped_filter_evalue"])
            ctx.set_query_contexts(1)
            hits = ctx.seed_search(to_hip_params(cfg))
            assert len(hits) > 0
            if not seen:
                cbs, host_plan = _host_rows(p, qd, ql, td, tl, hits)
                pred = _predict(qd, ql, td, tl, hits, cbs, M)
                _assert_bands_equal_host_rows(pred, host_plan)
            rows, groups, info = ctx.extend_plan_device(hits)     # (leaves the queries' bias in HBM for the filter below)
            passes = None
            if gf_on:
                flags = ctx.gapped_filter(hits, use_cbs=True)
                passes = [bool(flags[g["begin"]: g["begin"] + g["n_hits"]].any()) for g in pred]
                assert 0 < sum(passes) < len(passes)
            rows, groups, info = _compare(ctx, hits, pred, host_plan, small_form, passes)
            print("%s small_form=%d: %d hits, %d groups, %d on the host, lists %d + %d, %d re-listed, %d bands" % (
                tap, small_form, len(hits), info["n_groups"], info["n_on_host"], info["n_chain"], info["n_chain_big"], info["n_relisted"], info["n_bands"]))
            seen.append((rows.tobytes(), groups.tobytes()))
        finally:
            ctx.close()
    assert seen[0] == seen[1]


# ---- (c): constructed hit lists at the edges -------------------------------------------------------------------------------------
BOUNDARY_LENGTHS = [49, 50, 99, 100, 149, 150, 199, 200, 249, 250, 349, 350, 499, 500]


def _constructed_block():
    """(qd, ql, td, tl, hits, special): pair k = query k and target k; query k's hits lie in target k (every 9th query has one more
    hit in the next target). special: name -> list of pair numbers built for that edge."""
    p, M = _matrix()
    rng = np.random.default_rng(20260)
    pairs, special = [], {}

    def add(q, t, ij, name=None):
        assert all(0 <= i < len(q) and 0 <= j < len(t) for i, j in ij)
        pairs.append((np.asarray(q, np.int8), np.asarray(t, np.int8), list(ij)))
        if name:
            special.setdefault(name, []).append(len(pairs) - 1)

    def seg_of(q, t, h):
        s, _ = _run(0, q, _bias_of(p, q), t, M, [h])
        return s[0] if len(s) else None

    def repeats(qlen, tlen, unit_len):
        unit = rng.integers(0, 20, unit_len).astype(np.int8)
        return np.resize(unit, qlen).copy(), np.resize(unit, tlen).copy()

    # a call of exactly one hit = the first pair; hits on the first and on the last letter of a sequence
    s = rng.integers(0, 20, 60).astype(np.int8)
    add(s, s.copy(), [(30, 30)], "one_hit")
    add(s, s.copy(), [(0, 0), (59, 59)], "first_last_letter")
    # hit counts around PLAN_MAX_HITS, on exact repeats (every (i, j) with i = j mod unit is a match)
    for n in (1, 2, 31, 32, 33, 31, 32, 33):
        q, t = repeats(120, 130, 7)
        cand = [(i, j) for i in range(0, 110) for j in range(0, 120) if (i - j) % 7 == 0]
        pick = rng.choice(len(cand), n, replace=False)
        add(q, t, [cand[k] for k in pick], "hits_%d" % n)
    # segment counts: k hits on k different diagonals of unrelated repeats of two units (short segments that do not reach each other)
    for k in (1, 2, 4, 5, 16, 17, 16, 17, 12, 14, 15):
        unit = rng.integers(0, 20, 6).astype(np.int8)
        q = np.concatenate([np.concatenate([unit, rng.integers(0, 20, 9).astype(np.int8)]) for _ in range(k + 2)])
        t = np.concatenate([np.concatenate([rng.integers(0, 20, 5 + x % 3).astype(np.int8), unit]) for x in range(k + 2)])
        qpos = [15 * x for x in range(k + 2)]
        tpos, at = [], 0
        for x in range(k + 2):
            at += 5 + x % 3
            tpos.append(at)
            at += 6
        ij, diags = [], set()
        for x in rng.permutation((k + 2) * (k + 2)):
            i, j = qpos[x // (k + 2)], tpos[x % (k + 2)]
            if i - j not in diags and len(ij) < k:
                diags.add(i - j)
                ij.append((i, j))
        add(q, t, ij, "segs_%d" % k)
    # the same (i, j) twice, as two shapes give it
    for _ in range(4):
        q, t = _pair(rng, 0)
        h = _hits(rng, q, t, w=4)[:6]
        add(q, t, h + [h[0], h[-1]], "same_hit_twice")
    # a later hit exactly at the end of the kept segment (skipped) and one past it (walked)
    while len(special.get("hit_at_j_end", [])) < 4:
        q, t = _pair(rng, 0)
        h = _hits(rng, q, t, w=5)[0]
        sg = seg_of(q, t, h)
        if sg is None:
            continue
        i_end, j_end = int(sg[0] + sg[2]), int(sg[1] + sg[2])
        if i_end + 1 < len(q) and j_end + 1 < len(t):
            add(q, t, [h, (i_end, j_end)], "hit_at_j_end")
            add(q, t, [h, (i_end + 1, j_end + 1)], "hit_past_j_end")
    # two one-diagonal chains whose bands touch (0) or overlap by one diagonal (-1): query lengths of 100 - 149 have a band of 30 in
    # both modes, the gap between the diagonals costs more than either segment scores
    for gap in (0, -1, 0, -1):
        q = rng.integers(0, 20, 140).astype(np.int8)
        t = rng.integers(0, 20, 140).astype(np.int8)
        a = -40
        c = a + 61 + gap
        t[10 - a: 18 - a] = q[10:18]
        t[60 - c: 68 - c] = q[60:68]                                 # (behind the first in the query, before it in the target: no join)
        add(q, t, [(12, 12 - a), (63, 63 - c)], "bands_gap_%d" % gap)
    # bands clipped at both edges of the matrix
    for n in (10, 8, 12):
        s = rng.integers(0, 20, n).astype(np.int8)
        add(s, s.copy(), [(n // 2, n // 2)], "clipped_both")
    # query lengths on both sides of every length class of the band, the target long enough that nothing is clipped
    for n in BOUNDARY_LENGTHS:
        q = rng.integers(0, 20, n).astype(np.int8)
        t = np.concatenate([rng.integers(0, 20, 170).astype(np.int8), q, rng.integers(0, 20, 170).astype(np.int8)])
        add(q, t, [(n // 2, 170 + n // 2), (5, 175)], "len_%d" % n)
    # the bulk: colinear, repetitive, swapped and unrelated pairs with 1 - 40 of their word matches
    while len(pairs) < 2600:
        k = len(pairs)
        q, t = _pair(rng, k % 4)
        h = _hits(rng, q, t, w=(3, 4, 5)[k % 3])
        n = int(rng.integers(1, 41)) if k % 4 == 1 else int(rng.integers(1, 13))
        pick = np.sort(rng.choice(len(h), min(n, len(h)), replace=False))
        add(q, t, [h[x] for x in pick])
    add(s, s.copy(), [(3, 3)], "last_sequence")
    return _assemble(pairs, rng) + (special,)


def _assemble(pairs, rng):
    """the two blocks and the sorted hit list of (query, target, [(i, j)]) pairs"""
    qoff = np.concatenate([[0], np.cumsum([len(x[0]) for x in pairs])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(x[1]) for x in pairs])]).astype(np.int64)
    qd, ql = workload.sequence_set(np.concatenate([x[0] for x in pairs]), qoff)
    td, tl = workload.sequence_set(np.concatenate([x[1] for x in pairs]), toff)
    recs = []
    for k, (q, t, ij) in enumerate(pairs):
        for i, j in ij:
            recs.append((k, i, int(tl[k]) + j, int(rng.integers(15, 200)), 0))
        if k % 9 == 4 and k + 1 < len(pairs):
            recs.append((k, int(rng.integers(0, len(q))), int(tl[k + 1]) + int(rng.integers(0, len(pairs[k + 1][1]))), int(rng.integers(15, 200)), 0))
    hits = np.array(recs, dtype=hip.SEED_HIT_DTYPE)
    hits = hits[np.lexsort((hits["seed_offset"], hits["subject"], hits["query"]))]
    return qd, ql, td, tl, hits


def _overflow_block():
    """(qd, ql, td, tl, hits, special) for a search WITHOUT composition based statistics: groups of at most 16 segments that outgrow the
    96 links of the fixed workspace, among ordinary pairs. A query and a longer target of the same two-letter repeat, one hit on each
    of sixteen diagonals two apart: every segment runs the length of the query and overlaps every other; runs of changed letters, too
    short to stop the x-drop walk, cost each diagonal score at rows of its own, so that leaving one segment for another pays, for
    most pairs of them and in both directions (up to 2 * 120 links). Drawn until the emulator says so. With the Hauser bias the
    segments of such a repeat score too little against the links' letter scores, which carry no bias: a search of the same family
    with the bias on reached 68 links, so these groups are run with --comp-based-stats 0, where the bias is none."""
    _, M = _matrix()
    rng = np.random.default_rng(20261)
    pairs, special = [], {"workspace_overflow": []}
    for _ in range(20000):
        if len(pairs) % 16 != 5:
            q, t = _pair(rng, len(pairs) % 4)
            h = _hits(rng, q, t, w=4)
            pairs.append((q, t, [h[x] for x in np.sort(rng.choice(len(h), min(int(rng.integers(1, 13)), len(h)), replace=False))]))
            continue
        if len(special["workspace_overflow"]) == 4:
            break
        qlen = int(rng.integers(40, 140))
        unit = rng.choice(20, 2, replace=False).astype(np.int8)
        q, t = np.resize(unit, qlen).copy(), np.resize(unit, qlen + 32 + int(rng.integers(0, 10))).copy()
        width, step = int(rng.integers(2, 5)), int(rng.integers(10, 40))
        for x in ((t,), (t, q))[int(rng.integers(0, 2))]:
            at = int(rng.integers(0, step))
            while at + width < len(x):
                x[at:at + width] = rng.integers(0, 20, width)
                at += int(rng.integers(step // 2 + 4, step + 5))
        ij = sorted(((i, i + 2 * k) for k, i in enumerate(rng.integers(0, qlen, 16).tolist())), key=lambda h: (h[0] - h[1], h[1]))
        sg, ch = _run(2 | RESORT, q, None, t, M, ij)
        if 2 <= len(sg) <= MAX_SEGS and ch is None:
            special["workspace_overflow"].append(len(pairs))
            pairs.append((q, t, ij))
    return _assemble(pairs, rng) + (special,)


def _lanes():
    return int(emu.lib().emu_chain_lanes(1)), int(emu.lib().emu_chain_lanes(0))


def _assert_edges_present(qd, ql, td, tl, hits, special, pred, cbs, M):
    """Every edge the block was built for, from the CPU prediction alone."""
    by_pair = {}
    for g in pred:
        if g["query"] == g["target"]:
            by_pair[g["query"]] = g
    n_hits = {g["n_hits"] for g in pred}
    n_segs = {g["n_segs"] for g in pred if g["n_hits"] <= MAX_HITS}
    assert {1, 2, 31, 32, 33} <= n_hits, sorted(n_hits)
    assert {0, 1, 2, 4, 5, 16, 17} <= n_segs, sorted(n_segs)
    assert any(g["on_host"] and g["n_hits"] > MAX_HITS for g in pred) and any(g["on_host"] and g["n_hits"] <= MAX_HITS and g["n_segs"] > MAX_SEGS for g in pred)
    # (the fixed 16 / 96 / 16 workspace overflowing with at most 16 segments: _overflow_block and its test -- not reachable with the bias on)
    for k in special["same_hit_twice"]:
        g = by_pair[k]
        ij = [(int(h["seed_offset"]), int(h["subject"])) for h in hits[g["begin"]: g["begin"] + g["n_hits"]]]
        assert len(set(ij)) < len(ij)
    for name, past in (("hit_at_j_end", 0), ("hit_past_j_end", 1)):
        for k in special[name]:
            g = by_pair[k]
            assert g["n_hits"] == 2
            h = hits[g["begin"]: g["begin"] + 2]
            q, t = qd[ql[k]: ql[k + 1] - 1], td[tl[k]: tl[k + 1] - 1]
            first = (int(h[0]["seed_offset"]), int(h[0]["subject"] - tl[k]))
            sg = _run(0, q, cbs[ql[k]: ql[k + 1] - 1], t, M, [first])[0][0]
            assert (int(h[1]["seed_offset"]), int(h[1]["subject"] - tl[k])) == (int(sg[0] + sg[2]) + past, int(sg[1] + sg[2]) + past)
    # (the re-sort: see the module's docstring -- it cannot change the order, on any group)
    assert all(g["same_order"] for g in pred)
    for k in special["first_last_letter"]:
        g = by_pair[k]
        h = hits[g["begin"]: g["begin"] + g["n_hits"]]
        assert int(h[0]["seed_offset"]) == 0 and int(h[0]["subject"]) == tl[k] and int(h[-1]["seed_offset"]) == g["qlen"] - 1 and int(h[-1]["subject"]) == tl[k + 1] - 2
    last = len(ql) - 2
    assert pred[0]["query"] == 0 and pred[0]["target"] == 0 and pred[-1]["query"] == last and pred[-1]["target"] == len(tl) - 2
    per_query = np.bincount(hits["query"], minlength=last + 1)
    assert (per_query == 1).any() and pred[0]["n_hits"] == 1
    gaps = [x for g in pred if not g["on_host"] for x in g["gaps"]]
    assert 0 in gaps and -1 in gaps
    for k in special["bands_gap_0"]:
        assert by_pair[k]["gaps"] == [0] and len(by_pair[k]["bands"]) == 2, by_pair[k]
    for k in special["bands_gap_-1"]:
        assert by_pair[k]["gaps"] == [-1] and len(by_pair[k]["bands"]) == 1, by_pair[k]
    for k in special["clipped_both"]:
        g = by_pair[k]
        assert g["bands"] == [(-(g["tlen"] - 1), g["qlen"])]
    for n in BOUNDARY_LENGTHS:
        (k,) = special["len_%d" % n]
        g = by_pair[k]
        assert g["qlen"] == n and g["bands"] and all(d0 > -(g["tlen"] - 1) and d1 < n for d0, d1 in g["bands"]), g
    assert len(pred) > 2000 and sum(g["need_chain"] for g in pred) > 500


def _prefixes(pred, small_form):
    """Numbers of leading groups whose calls put the group count and the two chaining lists on the workgroup boundaries of the
    kernels: 64 lanes (plan_segments_kernel), 256 (list, count, gather), ChainLanes<...>::value of either chaining kernel."""
    ls, lb = _lanes()
    assert 2 <= lb < ls <= 64
    want = {1, 63, 64, 65, 255, 256, 257}
    need = np.cumsum([g["need_chain"] for g in pred])
    small = np.cumsum([g["need_chain"] and g["small"] for g in pred])
    big = np.cumsum([g["need_chain"] and (not g["small"] or g["relist"]) for g in pred])
    counts = [(small, ls), (big, lb)] if small_form else [(need, lb)]
    for cum, lanes in counts:
        for v in (lanes - 1, lanes, lanes + 1, 2 * lanes, 2 * lanes + 1):
            at = np.flatnonzero(cum == v)
            assert len(at), "no prefix of the block lists %d groups" % v
            want.add(int(at[0]) + 1)
    return sorted(want)


def test_constructed_block_at_the_edges_equals_the_host_plan(monkeypatch):
    assert torch.cuda.is_available()
    monkeypatch.setenv("DMND_EXTEND_GUARD", "1")
    p, M = _matrix()
    qd, ql, td, tl, hits, special = _constructed_block()
    p.db_letters = float(tl[-1] - tl[0] - (len(tl) - 1))
    cbs, host_plan = _host_rows(p, qd, ql, td, tl, hits)
    pred = {True: _predict(qd, ql, td, tl, hits, cbs, M, fast=True, every_group=True)}
    pred[False] = _predict(qd, ql, td, tl, hits, cbs, M, fast=False, every_group=True)
    _assert_edges_present(qd, ql, td, tl, hits, special, pred[True], cbs, M)
    # the restatement of the band merge equals the host planner on every group (fast mode: the one the host entry plans in)
    assert _assert_bands_equal_host_rows(pred[True], host_plan) > 2000
    assert any(a["bands"] != b["bands"] for a, b in zip(pred[True], pred[False]))
    whole = {}
    for small_form in (False, True):
        if small_form:
            monkeypatch.setenv("DMND_PLAN_SMALL_HITS", "0")
        for fast in (True, False):
            ctx = hip.Context(params=p)
            try:
                ctx.upload_block(hip.QUERY, qd, ql)
                ctx.upload_block(hip.TARGET, td, tl)
                ctx.set_db_letters(p.db_letters)
                ctx.lib.dmnd_set_extension_mode.argtypes = [ctypes.c_void_p, ctypes.c_int]
                assert ctx.lib.dmnd_set_extension_mode(ctx.h, 0 if fast else 1) == 0      # DMND_EXT_BANDED_FAST / DMND_EXT_BANDED_SLOW
                rows, groups, info = _compare(ctx, hits, pred[fast], host_plan, small_form, band_rows=not fast)
                print("constructed block small_form=%d fast=%d: %d hits, %d groups, %d on the host, lists %d + %d, %d re-listed, %d bands" % (
                    small_form, fast, len(hits), info["n_groups"], info["n_on_host"], info["n_chain"], info["n_chain_big"], info["n_relisted"], info["n_bands"]))
                whole[(small_form, fast)] = (rows.tobytes(), groups.tobytes())
                if fast:
                    for n in _prefixes(pred[True], small_form):
                        cut = pred[True][n]["begin"] if n < len(pred[True]) else len(hits)
                        _compare(ctx, hits[:cut], pred[True][:n], host_plan, small_form)
            finally:
                ctx.close()
    assert whole[(False, True)] == whole[(True, True)] and whole[(False, False)] == whole[(True, False)]


def test_groups_that_outgrow_the_fixed_workspace_are_left_to_the_host(monkeypatch):
    """The second hand-over of plan_chain_kernel<16, 96, 16, false>: at most 32 hits and at most 16 segments, and the links do not fit.
    Present by the CPU prediction alone; the device must leave exactly these groups to the host, in both forms, and plan the others
    as _bands does from the emulator's chains (the host planner's entry always applies the bias, so it is no reference here)."""
    assert torch.cuda.is_available()
    monkeypatch.setenv("DMND_EXTEND_GUARD", "1")
    p, M = _matrix()
    qd, ql, td, tl, hits, special = _overflow_block()
    p.db_letters = float(tl[-1] - tl[0] - (len(tl) - 1))
    pred = _predict(qd, ql, td, tl, hits, None, M, fast=True, every_group=True)
    _assert_overflow_present(special, pred)
    seen = []
    for small_form in (False, True):
        if small_form:
            monkeypatch.setenv("DMND_PLAN_SMALL_HITS", "0")
        ctx = hip.Context(params=p)
        try:
            ctx.upload_block(hip.QUERY, qd, ql)
            ctx.upload_block(hip.TARGET, td, tl)
            ctx.set_db_letters(p.db_letters)
            ctx.set_comp_based_stats(0)
            rows, groups, info = _compare(ctx, hits, pred, None, small_form, band_rows=True)
            print("overflow block small_form=%d: %d hits, %d groups, %d on the host, lists %d + %d, %d re-listed, %d bands" % (
                small_form, len(hits), info["n_groups"], info["n_on_host"], info["n_chain"], info["n_chain_big"], info["n_relisted"], info["n_bands"]))
            seen.append((rows.tobytes(), groups.tobytes()))
        finally:
            ctx.close()
    assert seen[0] == seen[1]


def _assert_overflow_present(special, pred):
    assert len(special["workspace_overflow"]) == 4
    by_pair = {g["query"]: g for g in pred if g["query"] == g["target"]}
    for k in special["workspace_overflow"]:
        g = by_pair[k]
        assert g["on_host"] and g["n_hits"] == 16 and 2 <= g["n_segs"] <= MAX_SEGS and g["need_chain"] and not g["small"], g
    assert any(g["on_host"] and g["n_hits"] <= MAX_HITS and g["n_segs"] <= MAX_SEGS for g in pred)
    assert sum(not g["on_host"] and g["need_chain"] for g in pred) > 20 and all(g["same_order"] for g in pred)


# ---- (d): order ----------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from diamond_amd import hip
z = np.load(sys.argv[2])
p = hip.default_params()
p.db_letters = float(z["db_letters"])
ctx = hip.Context(params=p)
try:
    ctx.upload_block(hip.QUERY, z["qd"], z["ql"])
    ctx.upload_block(hip.TARGET, z["td"], z["tl"])
    ctx.set_db_letters(p.db_letters)
    m = ctx.extend(z["qd"], z["td"], z["hits"].view(hip.SEED_HIT_DTYPE), threads=4)[0]
    plan = ctx.extend_plan_stats()
    open(sys.argv[3], "wb").write(m.tobytes())
    print("groups", plan["groups"], "records", len(m))
finally:
    ctx.close()
"""


def test_a_list_out_of_order_is_not_planned_and_extends_as_on_the_host(tmp_path):
    assert torch.cuda.is_available()
    cfg, _ = read_ext_tap(os.path.join(GOLDEN, "ext_fast_synth.tap"))
    qd, ql, td, tl = cfg["query"]["data"], cfg["query"]["limits"], cfg["target"]["data"], cfg["target"]["limits"]
    p, _ = _matrix()
    p.db_letters = float(tl[-1] - tl[0] - (len(tl) - 1))
    ctx = hip.Context(params=p)
    try:
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, td, tl)
        ctx.set_db_letters(p.db_letters)
        hits = ctx.seed_search(to_hip_params(cfg))
        rows, groups, info = ctx.extend_plan_device(hits)
        assert info["planned"] and len(rows) > 0
        same_query = np.flatnonzero((hits["query"][1:] == hits["query"][:-1]) & (hits["subject"][1:] != hits["subject"][:-1]))
        k = int(same_query[len(same_query) // 2])
        swapped = hits.copy()
        swapped[[k, k + 1]] = swapped[[k + 1, k]]
        rows, groups, info = ctx.extend_plan_device(swapped)
        assert not info["planned"] and info["unsorted"] and len(rows) == 0 and len(groups) == 0 and info["n_groups"] == 0 and info["n_bands"] == 0
        rows, groups, info = ctx.extend_plan_device(hits)         # (and the context plans the next, sorted list as before)
        assert info["planned"] and len(rows) > 0
    finally:
        ctx.close()
    np.savez(tmp_path / "in.npz", qd=qd, ql=ql, td=td, tl=tl, hits=swapped.view(np.uint8), db_letters=p.db_letters)
    out = {}
    for name, env in (("device", {}), ("host", {"DMND_EXTEND_PLAN_GPU": "0"})):
        r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(HERE), str(tmp_path / "in.npz"), str(tmp_path / (name + ".bin"))],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-1500:]
        assert r.stdout.split()[:2] == ["groups", "0"], r.stdout            # neither run used a device plan
        out[name] = open(tmp_path / (name + ".bin"), "rb").read()
    assert len(out["host"]) > 100 * hip.MATCH_DTYPE.itemsize and out["device"] == out["host"]
