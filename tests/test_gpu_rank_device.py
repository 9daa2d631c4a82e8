"""-m gpu: the device form of the global ranking step (dmnd_rank_targets_device; csrc/rank_kernels.hip, arithmetic in rank_core.h)
against two yardsticks on the same hits: dmnd_rank_targets (the host form), both outputs in (query, target) order, and a numpy
restatement of the walk over Context.xdrop_ungapped(hits, use_bias=False), which also gives the expected count of hits that were not
skipped (stats [1]).
The hit lists are built here: arbitrary in-bounds positions, sorted as dmnd_seed_hits sorts them. Hits that would tie in
(diagonal, j) across frames are removed before every call -- there the host's unstable sort decides nothing (rank_core.h has the
device rule) --, so every comparison covers all records.
blastp: 0 and 1 hit; 70 000 groups of one hit; group sizes cycling 1, 255, 256, 257; one pair with 5 000 hits, 3 000 of them on one
diagonal of an identical 4 000-letter pair; a 70 000-letter target with hits in its last 1 000 letters against a 40- and a
3 000-letter query; an all-tryptophan pair whose score passes 65 535. Translated (six contexts): hits in all frames; a frame's hit
covered by an earlier frame's segment on the same diagonal; equal best scores on two diagonals. n_keep and target_offset against the
host records cut in numpy (one context and six), and through rank_update. Hits resident in HBM after a real seed search, also one
made under set_seed_hits_resident. Refusals. The CLI with and without
DMND_RANK_HOST=1."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from diamond_amd import hip, synth, workload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "diamond")
CLI = os.path.join(ROOT, "diamond_amd", "diamond-hip")
W = 17                                     # tryptophan in the reference's letter order ARNDCQEGHILKMFPSTWYV: W/W scores 11


def _block(seqs):
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return workload.sequence_set(np.concatenate(seqs).astype(np.int8), off)


def _hits(tl, rows, contexts=1):
    """rows: (context id, i, target, j) -> SEED_HIT_DTYPE in dmnd_seed_hits' order, duplicates and cross-frame ties in
    (read, target, diagonal, j) removed (the lowest frame stays)"""
    a = np.array(sorted(set(rows)), dtype=np.int64).reshape(-1, 4)
    read, diag = a[:, 0] // contexts, a[:, 1] - a[:, 3]
    order = np.lexsort((a[:, 0], a[:, 3], diag, a[:, 2], read))
    key = np.stack([read, a[:, 2], diag, a[:, 3]], 1)[order]
    first = np.ones(len(a), bool)
    first[1:] = (key[1:] != key[:-1]).any(1)
    a = a[order[first]]
    h = np.zeros(len(a), hip.SEED_HIT_DTYPE)
    h["query"], h["seed_offset"], h["subject"] = a[:, 0], a[:, 1], tl[a[:, 2]] + a[:, 3]
    return h[np.lexsort((h["seed_offset"], h["subject"], h["query"]))]


def _restate(ctx, hits, tl, contexts=1, skip=True):
    """The walk of dmnd_rank_targets over the device's x-drop segments. Returns (records in (query, target) order, computed hits,
    uncast scores)."""
    seg = ctx.xdrop_ungapped(hits, use_bias=False)
    tgt = np.searchsorted(tl, hits["subject"], "right") - 1
    read, frame = hits["query"].astype(np.int64) // contexts, hits["query"].astype(np.int64) % contexts
    j = hits["subject"] - tl[tgt]
    diag = hits["seed_offset"].astype(np.int64) - j
    assert np.array_equal(seg["i"].astype(np.int64) - (seg["j"] - tl[tgt]), diag)
    j_end = seg["j"] - tl[tgt] + seg["len"]
    order = np.lexsort((frame, j, diag, tgt, read))
    recs, raw, computed = [], [], 0
    cur, d = None, None
    for k in order.tolist():
        g = (int(read[k]), int(tgt[k]))
        if g != cur:
            if cur is not None:
                recs.append((cur[0], cur[1], score & 0xffff, context, 0)); raw.append(score)
            cur, d, score, context = g, (int(diag[k]), int(j_end[k])), int(seg["score"][k]), int(frame[k])
            computed += 1
            continue
        if skip and d[0] == diag[k] and d[1] >= j[k]:
            continue
        d = (int(diag[k]), int(j_end[k]))
        computed += 1
        if seg["score"][k] > score:
            score, context = int(seg["score"][k]), int(frame[k])
    if cur is not None:
        recs.append((cur[0], cur[1], score & 0xffff, context, 0)); raw.append(score)
    return np.array(recs, hip.RANKED_DTYPE), computed, raw


def _check(ctx, world, hits, contexts=1):
    qd, ql, td, tl = world
    got = ctx.rank_targets_device(hits)
    st = ctx.rank_device_stats()
    host = ctx.rank_targets(qd, td, hits, threads=4)
    want, computed, raw = _restate(ctx, hits, tl, contexts)
    assert len(got) == len(host) == len(want)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:5]
    assert got.tobytes() == host.tobytes(), np.flatnonzero(got != host)[:5]
    assert st == [float(len(want)), float(computed), float(len(want)), 0.0]
    return got, raw


# ---- blastp ----------------------------------------------------------------------------------------------------------------------
N_Q, N_T = 280, 250                         # 70 000 pairs of short sequences
Q_SAME, Q_3000, Q_W, Q_A, Q_B = 280, 281, 282, 283, 284
T_SAME, T_LONG, T_W, T_A = 250, 251, 252, 253          # T_A .. T_A + 3: four targets of 300 letters


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(20261019)
    r = lambda n: rng.integers(0, 20, n).astype(np.int8)
    same = r(4000)
    q3000 = r(3000)
    long_t = r(70000)
    long_t[69000:70000] = q3000[2000:3000]                  # the long target ends in the long query's last 1 000 letters
    qs = [r(40) for _ in range(N_Q)] + [same, q3000, np.full(6100, W, np.int8), r(300), r(300)]
    ts = [r(41) for _ in range(N_T)] + [same.copy(), long_t, np.full(6100, W, np.int8)] + [r(300) for _ in range(4)]
    qd, ql = _block(qs)
    td, tl = _block(ts)
    return qd, ql, td, tl


@pytest.fixture(scope="module")
def ctx(world):
    assert torch.cuda.is_available()
    qd, ql, td, tl = world
    c = hip.Context(params=hip.default_params())
    c.upload_block(hip.QUERY, qd, ql)
    c.upload_block(hip.TARGET, td, tl)
    yield c
    c.close()


def test_no_hit_and_one_hit(ctx, world):
    tl = world[3]
    got = ctx.rank_targets_device(np.zeros(0, hip.SEED_HIT_DTYPE))
    assert len(got) == 0 and ctx.rank_device_stats() == [0.0, 0.0, 0.0, 0.0]
    got, _ = _check(ctx, world, _hits(tl, [(3, 7, 5, 9)]))
    assert (int(got["query"][0]), int(got["target"][0])) == (3, 5)


def test_70000_groups_of_one_hit(ctx, world):
    rng = np.random.default_rng(1)
    rows = [(q, int(i), t, int(j)) for q in range(N_Q) for t, i, j in zip(range(N_T), rng.integers(0, 40, N_T), rng.integers(0, 41, N_T))]
    hits = _hits(world[3], rows)
    got, _ = _check(ctx, world, hits)
    assert len(hits) == len(got) == 70000


def test_group_sizes_around_a_workgroup(ctx, world):
    rng = np.random.default_rng(2)
    rows = []
    for g, size in enumerate([1, 255, 256, 257] * 2):
        q, t = (Q_A, Q_B)[g // 4], T_A + g % 4
        cells = rng.choice(300 * 300, size=size, replace=False)
        rows += [(q, int(c) // 300, t, int(c) % 300) for c in cells]
    hits = _hits(world[3], rows)
    got, _ = _check(ctx, world, hits)
    assert len(got) == 8 and len(hits) == 2 * (1 + 255 + 256 + 257)


def test_5000_hits_of_one_pair_3000_on_one_diagonal(ctx, world):
    rng = np.random.default_rng(3)
    rows = [(Q_SAME, int(p), T_SAME, int(p)) for p in rng.choice(4000, size=3000, replace=False)]
    diags = np.concatenate([np.arange(-200, 0), np.arange(1, 201)])           # 400 diagonals, both signs
    for k in range(2000):
        d = int(diags[k % len(diags)])
        j = int(rng.integers(max(0, -d), min(4000, 4000 - d)))
        rows.append((Q_SAME, j + d, T_SAME, j))
    hits = _hits(world[3], rows)
    assert len(hits) >= 4900
    got, raw = _check(ctx, world, hits)
    st = ctx.rank_device_stats()
    assert len(got) == 1 and st[0] == 1.0
    assert st[1] <= len(hits) - 2990                       # the identical pair: one walk covers the whole main diagonal
    assert len(np.unique(hits["seed_offset"] - (hits["subject"] - world[3][T_SAME]))) > 256


@pytest.mark.parametrize("query", [5, Q_3000], ids=["40-letter-query", "3000-letter-query"])
def test_hits_at_the_end_of_a_70000_letter_target(ctx, world, query):
    rng = np.random.default_rng(4)
    qlen = 40 if query == 5 else 3000
    rows = [(query, int(rng.integers(0, qlen)), T_LONG, int(rng.integers(69000, 70000))) for _ in range(600)]
    if query == Q_3000:                                     # and along the planted copy: diagonal 2000 - 69000
        rows += [(query, 2000 + int(p), T_LONG, 69000 + int(p)) for p in rng.choice(1000, size=200, replace=False)]
    hits = _hits(world[3], rows)
    got, raw = _check(ctx, world, hits)
    diag = hits["seed_offset"] - (hits["subject"] - world[3][T_LONG])
    assert diag.min() < -65536 and len(got) == 1
    if query == Q_3000:
        assert raw[0] > 3000                                # the copy's walk, found on a diagonal beyond 16 bits


def test_score_beyond_65535_is_cast_like_the_host(ctx, world):
    hits = _hits(world[3], [(Q_W, 100, T_W, 100), (Q_W, 5000, T_W, 5000), (Q_W, 10, T_W, 50)])
    got, raw = _check(ctx, world, hits)
    assert raw == [6100 * 11] and int(got["score"][0]) == 6100 * 11 - 65536


# ---- translated ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def xworld():
    """22 reads x 6 contexts. Reads 0..19: random 60-letter frames against 8 shared targets. Read 20: context 0 is the first 50 letters of
    target 8, context 1 all 120 of them. Read 21: context 2 is ten letters of tryptophan, then the 30 letters of target 9; context 3
    those 30 letters alone."""
    rng = np.random.default_rng(77)
    r = lambda n: rng.integers(0, 17, n).astype(np.int8)    # (no tryptophan)
    ts = [r(80) for _ in range(8)] + [r(120), r(30)]
    qs = [r(60) for _ in range(20 * 6)]
    qs += [ts[8][:50].copy(), ts[8].copy(), r(20), r(20), r(20), r(20)]
    qs += [r(20), r(20), np.concatenate([np.full(10, W, np.int8), ts[9]]), ts[9].copy(), r(20), r(20)]
    qd, ql = _block(qs)
    td, tl = _block(ts)
    return qd, ql, td, tl


@pytest.fixture(scope="module")
def xctx(xworld):
    qd, ql, td, tl = xworld
    c = hip.Context(params=hip.default_params())
    c.upload_block(hip.QUERY, qd, ql)
    c.upload_block(hip.TARGET, td, tl)
    c.set_query_contexts(6)
    yield c
    c.close()


def test_translated_hits_in_all_six_frames(xctx, xworld):
    rng = np.random.default_rng(5)
    rows = [(int(rng.integers(0, 120)), int(rng.integers(0, 60)), int(rng.integers(0, 8)), int(rng.integers(0, 80))) for _ in range(6000)]
    rows += [(read * 6 + f, 10 + f, 3, 20 + f) for read in range(20) for f in range(6)]      # every frame of every read on one diagonal of target 3
    hits = _hits(xworld[3], rows, 6)
    got, _ = _check(xctx, xworld, hits, 6)
    assert len(got) == 160 and len(set(got["context"].tolist())) == 6
    frames = {(int(q) // 6, int(q) % 6) for q in hits["query"]}
    assert len(frames) == 120


def test_translated_hit_covered_by_another_frames_segment(xctx, xworld):
    tl = xworld[3]
    hits = _hits(tl, [(20 * 6 + 0, 5, 8, 5), (20 * 6 + 1, 30, 8, 30)], 6)
    got, raw = _check(xctx, xworld, hits, 6)
    no_skip, _, raw_no_skip = _restate(xctx, hits, tl, 6, skip=False)
    assert (int(got["context"][0]), int(got["query"][0]), int(got["target"][0])) == (0, 20, 8)
    assert int(no_skip["context"][0]) == 1 and raw_no_skip[0] > raw[0]      # without the skip rule frame 1's own walk would win
    assert xctx.rank_device_stats()[1] == 1.0


def test_translated_equal_best_scores_on_two_diagonals(xctx, xworld):
    tl = xworld[3]
    hits = _hits(tl, [(21 * 6 + 2, 15, 9, 5), (21 * 6 + 3, 5, 9, 5)], 6)
    seg = xctx.xdrop_ungapped(hits, use_bias=False)
    assert seg["score"][0] == seg["score"][1] > 0
    got, _ = _check(xctx, xworld, hits, 6)
    assert int(got["context"][0]) == 3                      # diagonal 0 (frame 3) is walked before diagonal 10 (frame 2); a tie changes nothing
    assert xctx.rank_device_stats()[1] == 2.0


# ---- n_keep, target_offset -------------------------------------------------------------------------------------------------------
def _cut(recs, n_keep, offset=0):
    order = np.lexsort((recs["target"], 65535 - recs["score"].astype(np.int64), recs["query"]))
    s = recs[order].copy()
    first = np.searchsorted(s["query"], s["query"], "left")
    s = s[np.arange(len(s)) - first < n_keep]
    s["target"] = (s["target"].astype(np.int64) + offset).astype(np.uint32)
    return s


def _keep_hits(world, seed):
    rng = np.random.default_rng(seed)
    rows = [(int(rng.integers(0, 30)), int(rng.integers(0, 40)), int(rng.integers(0, 40)), int(rng.integers(0, 41))) for _ in range(1500)]
    return _hits(world[3], rows)


@pytest.fixture(scope="module")
def keep_case(ctx, world):
    hits = _keep_hits(world, 6)
    return hits, ctx.rank_targets(world[0], world[2], hits, threads=4)


def test_n_keep_equals_the_host_records_cut_in_numpy(ctx, world, keep_case):
    hits, host = keep_case
    counts = np.bincount(host["query"])
    exact = int(counts.min())                               # the exact record count of some query, one more than it, and beyond every query's
    assert 2 < exact < counts.max()
    for n_keep in (1, exact, exact + 1, int(counts.max()), int(counts.max()) + 5):
        for offset in (0, 2 ** 31 - 10):
            got = ctx.rank_targets_device(hits, n_keep=n_keep, target_offset=offset)
            want = _cut(host, n_keep, offset)
            assert got.tobytes() == want.tobytes(), (n_keep, offset)
            assert ctx.rank_device_stats()[2] == float(len(want)) and ctx.rank_device_stats()[0] == float(len(host))
    assert len(_cut(host, int(counts.max()))) == len(host)
    all_off = ctx.rank_targets_device(hits, n_keep=0, target_offset=2 ** 31 - 10)
    assert np.array_equal(all_off["target"].astype(np.int64), host["target"].astype(np.int64) + 2 ** 31 - 10)


def test_equal_scores_at_the_cut_keep_the_smaller_target(ctx, world, keep_case):
    hits, host = keep_case
    found = 0
    for n_keep in (1, 2, 3, 5):
        got = ctx.rank_targets_device(hits, n_keep=n_keep)
        for q in np.unique(host["query"]):
            mine, kept = host[host["query"] == q], got[got["query"] == q]
            if len(mine) <= n_keep:
                continue
            dropped = mine[~np.isin(mine["target"], kept["target"])]
            tied = dropped[dropped["score"] == kept["score"][-1]]
            if len(tied):
                found += 1
                assert tied["target"].min() > kept["target"][kept["score"] == kept["score"][-1]].max()
    assert found >= 3, "no query whose cut falls between equal scores"


@pytest.mark.parametrize("n", [1, 4])
def test_rank_update_over_three_cut_blocks_equals_the_uncut_host_table(ctx, world, n):
    full, cut = np.zeros(30 * n, hip.RANKED_DTYPE), np.zeros(30 * n, hip.RANKED_DTYPE)
    for b in range(3):
        hits = _keep_hits(world, 10 + b)
        host = ctx.rank_targets(world[0], world[2], hits, threads=4)
        host["target"] += b * 1000
        hip.rank_update(full, n, host)
        hip.rank_update(cut, n, ctx.rank_targets_device(hits, n_keep=n, target_offset=b * 1000))
    assert full.tobytes() == cut.tobytes() and (full["score"] > 0).all()


def test_translated_n_keep_equals_the_host_records_cut_in_numpy(xctx, xworld):
    """the cut over the (read, target) pairs: a read's first pair and its number come from the planner's translated lists"""
    rng = np.random.default_rng(8)
    rows = [(int(rng.integers(0, 120)), int(rng.integers(0, 60)), int(rng.integers(0, 8)), int(rng.integers(0, 80))) for _ in range(3000)]
    rows = [r for r in rows if not (r[0] // 6 == 4 and r[2] > 2)]            # read 4 has three targets only
    hits = _hits(xworld[3], rows, 6)
    host = xctx.rank_targets(xworld[0], xworld[2], hits, threads=4)
    counts = np.bincount(host["query"])
    assert counts.min() == 3 and counts.max() == 8 and len(counts) == 20
    for n_keep, offset in ((1, 0), (3, 5), (4, 2 ** 31 - 10), (8, 0), (9, 1)):
        got = xctx.rank_targets_device(hits, n_keep=n_keep, target_offset=offset)
        want = _cut(host, n_keep, offset)
        assert got.tobytes() == want.tobytes(), (n_keep, offset)
        assert xctx.rank_device_stats()[0] == float(len(host))
    assert len(set(_cut(host, 3)["context"].tolist())) > 1


# ---- resident hits ---------------------------------------------------------------------------------------------------------------
def test_hits_resident_after_a_seed_search():
    db, doff, q, qoff = synth.generate(300, members=10, queries=300, seed=5, sub=(0.05, 0.6), qsub=(0.05, 0.5))
    qd, ql = workload.sequence_set(q, qoff)
    td, tl = workload.sequence_set(db, doff)
    p = hip.default_params()
    p.db_letters = float(doff[-1])
    sp, _ = hip.seed_params_preset("fast", p, threads=4)
    c = hip.Context(params=p)
    try:
        c.upload_block(hip.QUERY, qd, ql)
        c.upload_block(hip.TARGET, td, tl)
        c.set_db_letters(p.db_letters)
        assert c.seed_hit_count() == 0 and len(c.seed_hits()) == 0
        hits = c.seed_search(sp)
        assert len(hits) > 1000
        resident = c.rank_targets_device(None)
        assert c.rank_device_stats()[3] == 1.0
        uploaded = c.rank_targets_device(c.seed_hits())
        assert c.rank_device_stats()[3] == 0.0
        host = c.rank_targets(qd, td, hits, threads=4)
        assert len(host) > 300 and resident.tobytes() == uploaded.tobytes() == host.tobytes()
        kept = c.rank_targets_device(None, n_keep=3, target_offset=7)
        assert kept.tobytes() == _cut(host, 3, 7).tobytes()
        # a search whose hits stay in HBM (the seed search's own readback carries none): the same hits, read where they lie
        c.set_seed_hits_resident(True)
        assert c.seed_search(sp, fetch=False) == len(hits) == c.seed_hit_count()
        assert c.rank_targets_device(None).tobytes() == host.tobytes() and c.rank_device_stats()[3] == 1.0
        assert c.seed_hits().tobytes() == hits.tobytes()           # (dmnd_seed_hits downloads them then)
        c.set_seed_hits_resident(False)
        assert c.seed_search(sp).tobytes() == hits.tobytes()
    finally:
        c.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _raw_call(c, hits, n_keep, cap):
    out = np.zeros(max(1, cap), hip.RANKED_DTYPE)
    n = ctypes.c_int64(-1)
    v = ctypes.c_void_p
    c.lib.dmnd_rank_targets_device.argtypes = [v, v, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32, v, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    rc = c.lib.dmnd_rank_targets_device(c.h, hits.ctypes.data, ctypes.c_int64(hits.size), n_keep, 0, out.ctypes.data, ctypes.c_int64(cap), ctypes.byref(n))
    return rc, n.value


def test_refusals(ctx, world):
    qd, ql, td, tl = world
    hits = _keep_hits(world, 6)
    bad = hits.copy()
    k = next(i for i in range(len(bad) - 1) if bad["query"][i] == bad["query"][i + 1])
    bad[[k, k + 1]] = bad[[k + 1, k]]
    assert _raw_call(ctx, bad, 0, len(bad))[0] == -1                         # DMND_E_ARG: out of order
    n_recs = len(ctx.rank_targets(qd, td, hits, threads=4))
    assert _raw_call(ctx, hits, 0, n_recs - 1) == (-5, n_recs)               # DMND_E_CAP, *n_out set
    assert _raw_call(ctx, hits, 0, n_recs) == (0, n_recs)
    assert _raw_call(ctx, hits, -1, n_recs)[0] == -1                         # a negative n_keep
    outside = hits[:1].copy()
    outside["subject"] = tl[-1]
    assert _raw_call(ctx, outside, 0, 1)[0] == -1
    c = hip.Context(params=hip.default_params())
    try:
        c.upload_block(hip.QUERY, qd)                                        # no limits
        c.upload_block(hip.TARGET, td, tl)
        with pytest.raises(hip.DiamondHipError, match="limits"):
            c.rank_targets_device(hits)
    finally:
        c.close()


# ---- CLI -------------------------------------------------------------------------------------------------------------------------
def test_cli_global_ranking_device_and_host_forms_give_the_same_bytes(tmp_path):
    db, doff, q, qoff = synth.generate(150, members=12, queries=200, seed=31, decoy_frac=0.3)
    synth.write_fasta(str(tmp_path / "db.faa"), "t", db, doff)
    synth.write_fasta(str(tmp_path / "q.faa"), "q", q, qoff)
    args = ["blastp", "-q", str(tmp_path / "q.faa"), "-d", str(tmp_path / "db.faa"), "-p", "4", "--global-ranking", "8", "-b0.00002"]
    out = {}
    for form, env in (("device", {}), ("host", {"DMND_RANK_HOST": "1"})):
        e = {k: v for k, v in os.environ.items() if k != "DMND_RANK_HOST"}
        e.update(env, DMND_CLI_TIMELINE="1")
        r = subprocess.run([CLI] + args + ["-o", str(tmp_path / (form + ".out"))], capture_output=True, text=True, timeout=600, env=e)
        assert r.returncode == 0, r.stderr[-2000:]
        marks = [l for l in r.stderr.splitlines() if "ranked (on the " in l]
        assert len(marks) > 1 and all(("ranked (on the %s)" % form) in l for l in marks), marks[:3]      # several reference blocks, all in this form
        out[form] = open(tmp_path / (form + ".out")).read()
    assert len(out["device"].splitlines()) > 50 and out["device"] == out["host"]
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/diamond is missing: the two forms agree; the comparison with the reference binary was not made")
    r = subprocess.run([REF] + args + ["-o", str(tmp_path / "ref.out")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "ref.out").read() == out["device"]
