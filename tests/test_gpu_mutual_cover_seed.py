"""-m gpu tests of the mutual-coverage search in the seed stage (dmnd_set_min_length_ratio, include/diamond_hip.h): the length test
of length_ratio_core.h at every place of seed_kernels.hip where the Hamming identity decides.

Goldens: tests/golden/ext_mutual_*.tap, the reference's stage-2 hits tapped with --min-len-ratio 0.75 on inputs whose families
hold members of 45-100 % of their base (tests/mutual_sets.py; tests/golden/make_mutual_golden.sh). Which parameter reaches which
site (GOLDEN_CASES; the lists longer than 8 query positions -- the wave-cooperative / LDS-tiled / whole-workgroup paths -- are
reached by the crowded inputs of test_hits_equal_filtered_ratio_off_hits, whose near-identical queries share their seeds):
  fast, default                       seed_pair_kernel, light path, as the search runs by default
  DMND_SEED_CHAIN=0 / 1               seed_pair_kernel<CHAIN = false / true>: host-driven launches / the device chain (seed_chain.h)
  DMND_SEED_TILED=1                   seed_pair_tiled_kernel (joined positions sorted by seed)
  sensitive                           the fused short-seed stream (seed_stream_fast_kernel<FUSED>, filter_list)
  sensitive, DMND_SEED_FUSED=0        short seeds through seed_pair_kernel
  DMND_SEED_CLASSES_LONG=1            long seeds streamed by key class, then seed_pair_kernel
  DMND_SEED_SLICES=1                  the sliced long-seed stream, then seed_pair_kernel
  default (any of the above)          seed_deferred_kernel: its golden holds deferred pairs whose batch loses a mate to the length
                                      test (tests/test_length_ratio_core.py counts them with the emulator)
  hashed                              seed_encoding = 1 (the query-indexed algorithm's keys), golden minted with --algo 1
Every input meets the condition that the length test removes between 20 % and 80 % of what the ratio-off run finds."""
import os

import numpy as np
import pytest
import torch

import emu_py as emu
import mutual_sets
from tapfile import read_ext_tap
from diamond_amd import hip
from test_oracle_seed import hit_multiset
from test_length_ratio_core import query_window

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOOKS = ("DMND_SEED_TILED", "DMND_SEED_CHAIN", "DMND_SEED_FUSED", "DMND_SEED_CLASSES_LONG", "DMND_SEED_SLICES")


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    c = hip.Context()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def ratio_off_afterwards(ctx):
    yield
    ctx.set_min_length_ratio(0.0)


def to_hip_params(cfg):
    import ctypes
    e = emu.seed_params_from_tap(cfg)
    p = hip.SeedParams()
    assert ctypes.sizeof(p) == ctypes.sizeof(e)
    ctypes.memmove(ctypes.byref(p), ctypes.byref(e), ctypes.sizeof(p))
    return p


def set_hooks(monkeypatch, env):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def upload(ctx, qd, ql, td, tl):
    ctx.upload_block(hip.QUERY, qd, ql)
    ctx.upload_block(hip.TARGET, td, tl)


def filtered(hits, ql, tl, mlr):
    """The hits whose (query, target) lengths pass length_ratio_passes."""
    qlen, tlen = np.diff(ql) - 1, np.diff(tl) - 1
    t_of = np.searchsorted(tl, hits["subject"], side="right") - 1
    keep = np.array([mutual_sets.passes(int(qlen[q]), int(tlen[t]), mlr) for q, t in zip(hits["query"].tolist(), t_of.tolist())], bool)
    return hits[keep]


GOLDEN_CASES = [("ext_mutual_fast.tap", 0, {}), ("ext_mutual_fast.tap", 0, {"DMND_SEED_CHAIN": "0"}), ("ext_mutual_fast.tap", 0, {"DMND_SEED_CHAIN": "1"}),
                ("ext_mutual_fast.tap", 0, {"DMND_SEED_TILED": "1"}), ("ext_mutual_fast.tap", 0, {"DMND_SEED_CLASSES_LONG": "1"}),
                ("ext_mutual_fast.tap", 0, {"DMND_SEED_SLICES": "1"}), ("ext_mutual_hashed.tap", 1, {}), ("ext_mutual_hashed.tap", 1, {"DMND_SEED_TILED": "1"}),
                ("ext_mutual_default.tap", 0, {}), ("ext_mutual_default.tap", 0, {"DMND_SEED_CHAIN": "0"}), ("ext_mutual_default.tap", 0, {"DMND_SEED_CHAIN": "1"}),
                ("ext_mutual_default.tap", 0, {"DMND_SEED_TILED": "1"}), ("ext_mutual_default.tap", 0, {"DMND_SEED_TILED": "1", "DMND_SEED_CHAIN": "0"}),
                ("ext_mutual_default.tap", 0, {"DMND_SEED_CLASSES_LONG": "1"}), ("ext_mutual_default.tap", 0, {"DMND_SEED_SLICES": "1"}),
                ("ext_mutual_sensitive.tap", 0, {}), ("ext_mutual_sensitive.tap", 0, {"DMND_SEED_FUSED": "0"}),
                ("ext_mutual_sensitive.tap", 0, {"DMND_SEED_FUSED": "0", "DMND_SEED_TILED": "1"}), ("ext_mutual_sensitive.tap", 0, {"DMND_SEED_FUSED": "0", "DMND_SEED_CHAIN": "1"})]


@pytest.mark.parametrize("tap,enc,env", GOLDEN_CASES, ids=lambda v: v if isinstance(v, str) else ",".join("%s=%s" % (k[10:], x) for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_hit_multisets_equal_reference(ctx, tap, enc, env, monkeypatch):
    cfg, recs = read_ext_tap(os.path.join(GOLDEN, tap))
    ql, tl = cfg["query"]["limits"], cfg["target"]["limits"]
    upload(ctx, cfg["query"]["data"], ql, cfg["target"]["data"], tl)
    sp = to_hip_params(dict(cfg, seed_encoding=enc))
    set_hooks(monkeypatch, env)
    ctx.set_min_length_ratio(0.75)
    if env.get("DMND_SEED_SLICES") == "1":
        ctx.seed_search(sp)                                             # (the routing of the sliced stream is kept from here on)
    hits = ctx.seed_search(sp)
    ctx.set_min_length_ratio(0.0)
    off = ctx.seed_search(sp)
    ref = np.concatenate([r["hits"] for r in recs])
    removed = 1.0 - len(ref) / len(off)
    print("%s %s: %d hits, ratio off %d, removed %.1f %%" % (tap, env, len(hits), len(off), 100 * removed))
    assert 0.2 <= removed <= 0.8
    assert len(hits) == len(ref) and hit_multiset(hits) == hit_multiset(ref)
    assert (np.diff(hits["query"].astype(np.int64)) >= 0).all()
    if tap == "ext_mutual_default.tap":
        assert (hits["score"] == 255).any() and (hits["score"] > 255).any()      # both outcomes of the deferred pass


@pytest.fixture(scope="module")
def crowded():
    """Sorted blocks whose near-identical families put more than eight query positions on a seed (the cooperative paths of the pair
    filters) and many equal lengths on both sides; with the --fast and the --sensitive shapes, window scores off."""
    db, doff, q, qoff = mutual_sets.generate(families=30, members=5, queries=2, near=3, near_members=14, near_queries=14, seed=41, hi=400)
    return mutual_sets.sorted_blocks(db, doff, q, qoff)


def preset_without_scores(name, enc):
    params = hip.default_params()
    sp, _ = hip.seed_params_preset(name, params, threads=1)
    if enc:
        hip.set_query_indexed(sp, threads=1)
    sp.use_ungapped = 0                                                    # no window scores: the length test is a pure per-pair predicate
    return sp


FREE_CASES = [("fast", 0, {}), ("fast", 0, {"DMND_SEED_CHAIN": "0"}), ("fast", 0, {"DMND_SEED_CHAIN": "1"}), ("fast", 0, {"DMND_SEED_TILED": "1"}),
              ("fast", 0, {"DMND_SEED_TILED": "1", "DMND_SEED_CHAIN": "0"}), ("fast", 1, {}), ("fast", 0, {"DMND_SEED_SLICES": "1"}),
              ("sensitive", 0, {}), ("sensitive", 0, {"DMND_SEED_FUSED": "0"}), ("sensitive", 0, {"DMND_SEED_FUSED": "0", "DMND_SEED_TILED": "1"}), ("sensitive", 1, {})]


@pytest.mark.parametrize("preset,enc,env", FREE_CASES, ids=lambda v: v if isinstance(v, str) else ",".join("%s=%s" % (k[10:], x) for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_hits_equal_filtered_ratio_off_hits(ctx, crowded, preset, enc, env, monkeypatch):
    """Without window scores the hits with ratio r are the ratio-off hits on the same blocks filtered by length_ratio_passes, for
    r in {0.45, 0.75, 0.95, 1.0}; with r = 1e-9 they are the ratio-off hits. Setting the ratio back to 0 reproduces them exactly."""
    qd, ql, td, tl = crowded
    upload(ctx, qd, ql, td, tl)
    sp = preset_without_scores(preset, enc)
    set_hooks(monkeypatch, env)
    ctx.set_min_length_ratio(0.0)
    off = ctx.seed_search(sp)
    assert len(off) > 2000
    for r in (0.45, 0.75, 0.95, 1.0):
        ctx.set_min_length_ratio(r)
        hits = ctx.seed_search(sp)
        want = filtered(off, ql, tl, r)
        assert len(hits) == len(want) and hit_multiset(hits) == hit_multiset(want), r
        if r == 0.75:
            assert 0.2 <= 1.0 - len(hits) / len(off) <= 0.8
    ctx.set_min_length_ratio(1e-9)
    assert np.array_equal(ctx.seed_search(sp), off)
    ctx.set_min_length_ratio(0.0)
    assert np.array_equal(ctx.seed_search(sp), off)


def test_crowded_blocks_reach_the_cooperative_paths(crowded):
    """The inputs above hold seeds with more than eight query positions (LIGHT in seed_kernels.hip) in both seed geometries."""
    qd, ql, td, tl = crowded
    for preset in ("fast", "sensitive"):
        sp = preset_without_scores(preset, 0)
        w, L = sp.shape_weight[0], sp.shape_len[0]
        pos = [sp.shape_pos[0][k] for k in range(w)]
        red = np.array([sp.reduction[i] for i in range(32)])
        keys = {}
        for i in range(len(ql) - 1):
            s = red[qd[ql[i]:ql[i + 1] - 1] & 31]
            for p in range(len(s) - L + 1):
                k = tuple(s[p + x] for x in pos)
                keys[k] = keys.get(k, 0) + 1
        assert max(keys.values()) > 8, preset


def test_query_index_reuse_rebuilds_the_windows_per_reference_block(ctx, crowded):
    qd, ql, td, tl = crowded
    sp = preset_without_scores("fast", 0)
    # a second reference block: the shorter half of the targets
    n = (len(tl) - 1) // 2
    td2 = np.concatenate([np.full(256, 31, np.int8), td[tl[n]:tl[-1]], np.full(256, 31, np.int8)])
    tl2 = tl[n:] - tl[n] + 256
    want = []
    for t, l in ((td, tl), (td2, tl2)):
        upload(ctx, qd, ql, t, l)
        ctx.set_min_length_ratio(0.0)
        want.append(filtered(ctx.seed_search(sp), ql, l, 0.75))
    ctx.set_query_index_reuse(True)
    try:
        ctx.set_min_length_ratio(0.75)
        ctx.upload_block(hip.QUERY, qd, ql)
        for (t, l), w in zip(((td, tl), (td2, tl2), (td, tl)), (want[0], want[1], want[0])):
            ctx.upload_block(hip.TARGET, t, l)
            hits = ctx.seed_search(sp)
            assert len(hits) == len(w) and hit_multiset(hits) == hit_multiset(w)
    finally:
        ctx.set_query_index_reuse(False)


def test_unsorted_blocks_and_bad_ratios_are_refused(ctx, crowded):
    qd, ql, td, tl = crowded
    sp = preset_without_scores("fast", 0)
    for bad in (-0.1, 1.0000001, float("nan")):
        with pytest.raises(hip.DiamondHipError, match="ratio"):
            ctx.set_min_length_ratio(bad)
    db, doff, q, qoff = mutual_sets.generate(families=6, members=3, queries=2, seed=9)
    from diamond_amd import workload
    uq, uql = workload.sequence_set(q, qoff)
    ut, utl = workload.sequence_set(db, doff)
    assert (np.diff(np.diff(uql)) > 0).any() and (np.diff(np.diff(utl)) > 0).any()
    ctx.set_min_length_ratio(0.75)
    for blocks, what in (((uq, uql, td, tl), "query"), ((qd, ql, ut, utl), "reference")):
        upload(ctx, *blocks)
        with pytest.raises(hip.DiamondHipError, match="%s block must be length-sorted" % what):
            ctx.seed_search(sp)
        assert ctx.seed_hit_count() == 0                                     # nothing ran
    ctx.set_query_contexts(6)
    upload(ctx, qd, ql, td, tl)
    try:
        with pytest.raises(hip.DiamondHipError, match="translated"):
            ctx.seed_search(sp)
    finally:
        ctx.set_query_contexts(1)
    # the ratio off takes unsorted blocks as ever
    ctx.set_min_length_ratio(0.0)
    upload(ctx, uq, uql, ut, utl)
    assert len(ctx.seed_search(sp)) > 0


def test_length_sort_order_binding():
    limits = np.concatenate([[256], 256 + np.cumsum(np.array([5, 9, 5, 9, 5]) + 1)])
    assert hip.length_sort_order(limits).tolist() == [3, 1, 4, 2, 0]
    assert hip.length_sort_order(np.array([256])).tolist() == []


@pytest.mark.parametrize("mlr", [0.45, 0.75, 0.8999999999999999, 1.0])
def test_device_windows_equal_length_window(ctx, crowded, mlr):
    """seed_qwin_kernel's window of every target equals length_window (the host's two binary searches over length_ratio_passes), on
    blocks with many equal lengths."""
    qd, ql, td, tl = crowded
    upload(ctx, qd, ql, td, tl)
    ctx.set_min_length_ratio(mlr)
    ctx.seed_search(preset_without_scores("fast", 0))
    win = ctx.seed_query_windows(len(tl) - 1)
    tlen = np.diff(tl) - 1
    assert (np.diff(tlen) == 0).sum() > 10
    for t in range(len(tlen)):
        assert tuple(win[t].tolist()) == query_window(ql, int(tlen[t]), mlr), t
    assert (win[:, 0] == win[:, 1]).any() or mlr < 0.9                       # short targets that no query passes against


def test_no_admissible_query_gives_no_hits(ctx):
    """Queries all much longer than every target: every window is empty and the search returns nothing, though the ratio-off search has hits."""
    rng = np.random.default_rng(17)
    base = rng.integers(0, 20, 600).astype(np.int8)
    q = [base[:600 - i].copy() for i in range(6)]
    t = [base[a:a + 200 - i].copy() for i, a in enumerate((0, 100, 200, 300, 390))]
    off = lambda s: np.concatenate([[0], np.cumsum([len(x) for x in s])]).astype(np.int64)
    from diamond_amd import workload
    qd, ql = workload.sequence_set(np.concatenate(q), off(q))
    td, tl = workload.sequence_set(np.concatenate(t), off(t))
    upload(ctx, qd, ql, td, tl)
    sp = preset_without_scores("fast", 0)
    assert len(ctx.seed_search(sp)) > 0
    ctx.set_min_length_ratio(0.75)
    assert len(ctx.seed_search(sp)) == 0
    assert (ctx.seed_query_windows(len(tl) - 1) == 0).all()
    with pytest.raises(hip.DiamondHipError):
        ctx.seed_query_windows(len(tl))
