"""-m gpu tests of the linearised search in the seed stage (dmnd_set_linsearch, include/diamond_hip.h): the reduction of a shape's
joined records to the first reference position per seed (seed_lin_first_kernel) and its readers, on every long-seed path that
reaches the pair filter.

Goldens: tests/golden/ext_lin_*.tap, the reference's stage-2 hits tapped with --linsearch (tests/golden/make_linsearch_golden.sh);
tests/test_linsearch_core.py shows with the emulator that the rule drops 48-63 % of their joined positions. Which parameter
reaches which site:
  DMND_SEED_CHAIN=0 / 1               host-driven launches / the device chain (the shape's range comes from the counter block)
  DMND_SEED_TILED=1                   seed_pair_tiled_kernel (joined positions sorted by seed; the first one starts its seed's run)
  DMND_SEED_CLASSES_LONG=1            long seeds streamed by key class, then seed_pair_kernel
  DMND_SEED_SLICES=1                  the sliced long-seed stream (joined positions listed slice by slice, not in block order)
  hashed                              seed_encoding = 1 (the query-indexed algorithm's keys), golden minted with --algo 1
  DMND_SEED_MATCHED_CAP               phase 1 runs again after a joined-position overflow
Hand-made blocks (the smallest shapes that can go wrong) are checked against the emulator (tests/emu/linsearch_emu.cpp)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import emu_py as emu
import mutual_sets
from tapfile import read_ext_tap
from diamond_amd import hip, workload
from test_oracle_seed import blosum62_matrix8, hit_multiset
from test_linsearch_core import lin_seed_search

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOOKS = ("DMND_SEED_TILED", "DMND_SEED_CHAIN", "DMND_SEED_FUSED", "DMND_SEED_CLASSES_LONG", "DMND_SEED_SLICES", "DMND_SEED_MATCHED_CAP")
PATHS = [{}, {"DMND_SEED_CHAIN": "0"}, {"DMND_SEED_CHAIN": "1"}, {"DMND_SEED_TILED": "1"}, {"DMND_SEED_TILED": "1", "DMND_SEED_CHAIN": "0"},
         {"DMND_SEED_CLASSES_LONG": "1"}, {"DMND_SEED_SLICES": "1"}]
ids = lambda v: v if isinstance(v, str) else ",".join("%s=%s" % (k[10:], x) for k, x in v.items()) if isinstance(v, dict) else str(v)


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    c = hip.Context()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def switch_off_afterwards(ctx):
    yield
    ctx.set_linsearch(False)
    ctx.set_min_length_ratio(0.0)


def copy_params(src, cls):
    p = cls()
    assert ctypes.sizeof(p) == ctypes.sizeof(src)
    ctypes.memmove(ctypes.byref(p), ctypes.byref(src), ctypes.sizeof(p))
    return p


def set_hooks(monkeypatch, env):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def upload(ctx, qd, ql, td, tl):
    ctx.upload_block(hip.QUERY, qd, ql)
    ctx.upload_block(hip.TARGET, td, tl)


def preset(name, hashed=False):
    sp, _ = hip.seed_params_preset(name, hip.default_params(), threads=1)
    if hashed:
        hip.set_query_indexed(sp, threads=1)
    return sp


_golden = {}


def golden(tap):
    """(cfg, the reference's hits) of a golden, read once."""
    if tap not in _golden:
        cfg, recs = read_ext_tap(os.path.join(GOLDEN, tap))
        _golden[tap] = (cfg, np.concatenate([r["hits"] for r in recs]))
    return _golden[tap]


GOLDEN_CASES = [("ext_lin_fast.tap", 0, env) for env in PATHS] + [("ext_lin_default.tap", 0, env) for env in PATHS] \
    + [("ext_lin_hashed.tap", 1, {}), ("ext_lin_hashed.tap", 1, {"DMND_SEED_CHAIN": "0"}), ("ext_lin_hashed.tap", 1, {"DMND_SEED_TILED": "1"})]


@pytest.mark.parametrize("tap,enc,env", GOLDEN_CASES, ids=ids)
def test_hit_multisets_equal_reference(ctx, tap, enc, env, monkeypatch):
    cfg, ref = golden(tap)
    upload(ctx, cfg["query"]["data"], cfg["query"]["limits"], cfg["target"]["data"], cfg["target"]["limits"])
    sp = copy_params(emu.seed_params_from_tap(dict(cfg, seed_encoding=enc)), hip.SeedParams)
    set_hooks(monkeypatch, env)
    ctx.set_linsearch(True)
    if env.get("DMND_SEED_SLICES") == "1":
        ctx.seed_search(sp)                                             # (the routing of the sliced stream is kept from here on)
    hits = ctx.seed_search(sp)
    again = ctx.seed_search(sp)
    ctx.set_linsearch(False)
    off = ctx.seed_search(sp)
    print("%s %s: %d hits, switch off %d" % (tap, env, len(hits), len(off)))
    assert len(hits) == len(ref) and hit_multiset(hits) == hit_multiset(ref)
    assert (np.diff(hits["query"].astype(np.int64)) >= 0).all()          # sorted by query
    assert hit_multiset(again) == hit_multiset(hits)                    # two consecutive searches
    assert len(off) != len(hits)
    if tap == "ext_lin_default.tap":
        assert (hits["score"] > 255).any()                               # emitted with their scalar score, not deferred


def test_switch_off_after_on_equals_a_fresh_search(ctx):
    """A context that has searched with the switch on gives, with the switch off again, exactly what a context gives that never had it on."""
    cfg, _ = golden("ext_lin_default.tap")
    blocks = (cfg["query"]["data"], cfg["query"]["limits"], cfg["target"]["data"], cfg["target"]["limits"])
    sp = copy_params(emu.seed_params_from_tap(cfg), hip.SeedParams)
    upload(ctx, *blocks)
    ctx.set_linsearch(True)
    on = ctx.seed_search(sp)
    ctx.set_linsearch(False)
    off = ctx.seed_search(sp)
    fresh = hip.Context()
    try:
        upload(fresh, *blocks)
        want = fresh.seed_search(sp)
    finally:
        fresh.close()
    assert len(on) != len(off) and np.array_equal(off, want)
    assert (off["score"] == 255).any() or (off["score"] > 255).any()      # the deferred pass is back


# ---- hand-made blocks -----------------------------------------------------------------------------------------------------------

def rnd(rng, n):
    return rng.integers(0, 20, n).astype(np.int8)


def planted(rng, n, *motifs):
    """n random letters with every (offset, motif) written over them."""
    s = rnd(rng, n)
    for at, m in motifs:
        assert 0 <= at and at + len(m) <= n
        s[at:at + len(m)] = m
    return s


def sets_of(queries, targets):
    """SequenceSet blocks of the given sequences; the targets must come in non-increasing length order."""
    off = lambda seqs: np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    assert (np.diff([len(t) for t in targets]) <= 0).all()
    qd, ql = workload.sequence_set(np.concatenate(queries).astype(np.int8), off(queries))
    td, tl = workload.sequence_set(np.concatenate(targets).astype(np.int8), off(targets))
    return qd, ql, td, tl


def check_against_emulator(ctx, monkeypatch, sp, blocks, paths=PATHS):
    """The linearised search of the blocks on every path equals the emulator's; returns (its hits, its statistics, the switch-off hits)."""
    want, stats = lin_seed_search(copy_params(sp, emu.SeedParams), blosum62_matrix8(), *blocks)
    upload(ctx, *blocks)
    for env in paths:
        set_hooks(monkeypatch, env)
        ctx.set_linsearch(True)
        hits = ctx.seed_search(sp)
        assert len(hits) == len(want) and hit_multiset(hits) == hit_multiset(want), env
    set_hooks(monkeypatch, {})
    ctx.set_linsearch(False)
    return want, stats, ctx.seed_search(sp)


def target_of(tl, subject):
    return np.searchsorted(tl, subject, side="right") - 1


def whole(hits, at, n):
    """The hits whose seed window of up to 16 letters lies inside the n planted letters at block position `at` (a window that
    reaches into the random letters beside them may or may not be a seed of another copy: chance, which the emulator shares)."""
    return hits[(hits["subject"] >= at) & (hits["subject"] <= at + n - 16)]


def near(hits, at, n):
    """The hits whose seed window touches those letters (the switch-off search keeps the left-most window of a diagonal only)."""
    return hits[(hits["subject"] > at - 16) & (hits["subject"] < at + n)]


@pytest.mark.parametrize("name,hashed", [("fast", False), ("default", False), ("fast", True)], ids=["fast", "default-two-shapes", "hashed"])
def test_one_seed_in_three_workgroups_of_the_stream(ctx, monkeypatch, name, hashed):
    """A 40-letter stretch at three reference positions that three different workgroups of the stream read (4096 window starts
    each: a block above 8192 letters), the first one in the longest target: all hits lie there. With the default sensitivity's two
    shapes, window scores on."""
    rng = np.random.default_rng(1)
    m = rnd(rng, 40)
    targets = [planted(rng, 4200, (100, m)), planted(rng, 4100, (500, m)), planted(rng, 4000, (300, m))]
    queries = [planted(rng, 300, (120, m)), rnd(rng, 200), planted(rng, 250, (7, m))]
    blocks = sets_of(queries, targets)
    tl = blocks[3]
    at = [int(tl[0]) + 100, int(tl[1]) + 500, int(tl[2]) + 300]
    assert at[0] - tl[0] < 4096 <= at[1] - tl[0] < 8192 <= at[2] - tl[0]
    sp = preset(name, hashed)
    want, stats, off = check_against_emulator(ctx, monkeypatch, sp, blocks)
    per_copy = 2 * (40 - 16 + 1) * sp.n_shapes                             # two queries, every whole window, every shape
    assert [len(whole(want, a, 40)) for a in at] == [per_copy, 0, 0]
    assert all(0 < len(near(off, a, 40)) < per_copy for a in at)         # (the switch-off search: every copy, thinned by the left-most filter)
    assert set(target_of(tl, off["subject"]).tolist()) == {0, 1, 2} and stats["selected"] < stats["joined"]


def test_the_same_seed_twice_inside_one_target(ctx, monkeypatch):
    rng = np.random.default_rng(2)
    m = rnd(rng, 30)
    blocks = sets_of([planted(rng, 200, (50, m))], [planted(rng, 900, (200, m), (600, m)), rnd(rng, 500)])
    tl = blocks[3]
    want, stats, off = check_against_emulator(ctx, monkeypatch, preset("fast"), blocks)
    assert len(whole(want, tl[0] + 200, 30)) == 30 - 16 + 1 and len(near(off, tl[0] + 600, 30)) > 0
    assert len(whole(want, tl[0] + 600, 30)) == 0                          # the later occurrence in the same target is dropped


def test_first_position_fails_the_hamming_test_where_a_later_one_passes(ctx, monkeypatch):
    """The longest target carries the query's seed in other letters of the same reduced classes amid random letters (the pair fails
    the Hamming identity), a shorter target carries the query's stretch letter for letter: the switch-off search reports the
    second, the linearised search nothing."""
    rng = np.random.default_rng(3)
    sp = preset("fast")
    red = [sp.reduction[i] for i in range(20)]
    classes = [2, 6, 1, 7, 9, 2, 6, 7, 1, 9, 6, 2, 7, 6, 2, 9]            # classes with at least two letters each
    pick = lambda c, k: [l for l in range(20) if red[l] == c][k]
    seed_q = np.array([pick(c, 0) for c in classes], np.int8)
    seed_t = np.array([pick(c, 1) for c in classes], np.int8)
    stretch = np.concatenate([rnd(rng, 16), seed_q, rnd(rng, 16)])        # the whole Hamming window [-16, +32)
    # the shorter target's copy differs in the four letters on either side of the seed, by class: no shifted window is a seed of both
    # (any four consecutive places of the shape hold one that counts), and 40 of the 48 letters still agree
    other = lambda l: next(x for x in range(20) if red[x] != red[l])
    copy = stretch.copy()
    for i in list(range(12, 16)) + list(range(32, 36)):
        copy[i] = other(int(stretch[i]))
    query = planted(rng, 200, (60, stretch))
    blocks = sets_of([query], [planted(rng, 700, (300, seed_t)), planted(rng, 600, (100, copy))])
    want, stats, off = check_against_emulator(ctx, monkeypatch, sp, blocks)
    assert len(want) == 0 and stats["selected"] == 1 and stats["joined"] == 2 and stats["dropped_though_passing"] == 1
    assert len(off) == 1 and target_of(blocks[3], off["subject"])[0] == 1


def test_seeds_at_the_first_and_the_last_window_of_the_block(ctx, monkeypatch):
    rng = np.random.default_rng(4)
    m1, m2 = rnd(rng, 20), rnd(rng, 20)
    targets = [planted(rng, 800, (0, m1)), planted(rng, 700, (350, m1)), planted(rng, 600, (580, m2))]
    blocks = sets_of([planted(rng, 150, (10, m1), (100, m2))], targets)
    tl = blocks[3]
    want, stats, off = check_against_emulator(ctx, monkeypatch, preset("fast"), blocks)
    subjects = set(want["subject"].tolist())
    assert int(tl[0]) in subjects and int(tl[3]) - 1 - 16 in subjects     # the block's first window, and its last one of 16 letters
    assert [len(whole(want, a, 20)) for a in (tl[0], tl[1] + 350, tl[2] + 580)] == [5, 0, 5]
    assert all(len(near(off, a, 20)) > 0 for a in (tl[0], tl[1] + 350, tl[2] + 580))


def test_query_lists_of_nine_and_of_more_than_sixty_four(ctx, monkeypatch):
    """Seeds with 9 query positions (above the light path's 8) and with 70 (more than one wavefront of the cooperative path)."""
    rng = np.random.default_rng(5)
    a, b = rnd(rng, 20), rnd(rng, 20)
    queries = [planted(rng, 80, (int(rng.integers(0, 60)), a)) for _ in range(9)] + [planted(rng, 80, (int(rng.integers(0, 60)), b)) for _ in range(70)]
    targets = [planted(rng, 900 - 50 * i, (100 + 10 * i, a), (400 + 10 * i, b)) for i in range(3)]
    blocks = sets_of(queries, targets)
    tl = blocks[3]
    want, stats, off = check_against_emulator(ctx, monkeypatch, preset("fast"), blocks)
    for i in range(3):
        for at, n in ((tl[i] + 100 + 10 * i, 9), (tl[i] + 400 + 10 * i, 70)):
            assert len(whole(want, at, 20)) == (5 * n if i == 0 else 0) and len(near(off, at, 20)) >= n


def test_a_low_complexity_group_stays_erased(ctx, monkeypatch):
    rng = np.random.default_rng(6)
    low, m = np.zeros(24, np.int8), rnd(rng, 20)
    blocks = sets_of([planted(rng, 200, (20, low), (100, m))], [planted(rng, 600, (50, low), (300, m)), planted(rng, 500, (200, low), (400, m))])
    tl = blocks[3]
    want, stats, off = check_against_emulator(ctx, monkeypatch, preset("fast"), blocks)
    assert len(whole(want, tl[0] + 300, 20)) == 5 and len(whole(want, tl[1] + 400, 20)) == 0 and len(near(off, tl[1] + 400, 20)) > 0
    for hits in (want, off):                                               # nothing from the erased group, in either search
        assert len(whole(hits, tl[0] + 50, 24)) == 0 and len(whole(hits, tl[1] + 200, 24)) == 0


@pytest.mark.parametrize("env", [{"DMND_SEED_CHAIN": "0"}, {"DMND_SEED_CHAIN": "1"}], ids=ids)
@pytest.mark.parametrize("tap", ["ext_lin_fast.tap", "ext_lin_default.tap"])
def test_phase_one_runs_again_after_a_joined_position_overflow(ctx, monkeypatch, tap, env):
    cfg, ref = golden(tap)
    upload(ctx, cfg["query"]["data"], cfg["query"]["limits"], cfg["target"]["data"], cfg["target"]["limits"])
    sp = copy_params(emu.seed_params_from_tap(cfg), hip.SeedParams)
    set_hooks(monkeypatch, dict(env, DMND_SEED_MATCHED_CAP="64"))
    ctx.set_linsearch(True)
    hits = ctx.seed_search(sp)
    assert len(hits) == len(ref) and hit_multiset(hits) == hit_multiset(ref)


def test_query_index_reuse_over_two_reference_blocks(ctx, monkeypatch):
    """First positions are per reference block: with the query side kept, block A, then its shorter half B (where the seeds' first
    positions are others), then A again."""
    cfg, ref = golden("ext_lin_fast.tap")
    qd, ql, td, tl = cfg["query"]["data"], cfg["query"]["limits"], cfg["target"]["data"], cfg["target"]["limits"]
    n = (len(tl) - 1) // 2
    td2 = np.concatenate([np.full(256, 31, np.int8), td[tl[n]:tl[-1]], np.full(256, 31, np.int8)])
    tl2 = tl[n:] - tl[n] + 256
    sp = copy_params(emu.seed_params_from_tap(cfg), hip.SeedParams)
    want2, stats2 = lin_seed_search(emu.seed_params_from_tap(cfg), blosum62_matrix8(), qd, ql, td2, tl2)
    assert 0 < len(want2) and stats2["selected"] < stats2["joined"]
    set_hooks(monkeypatch, {})
    ctx.set_query_index_reuse(True)
    try:
        ctx.set_linsearch(True)
        ctx.upload_block(hip.QUERY, qd, ql)
        for (t, l), w in zip(((td, tl), (td2, tl2), (td, tl)), (ref, want2, ref)):
            ctx.upload_block(hip.TARGET, t, l)
            hits = ctx.seed_search(sp)
            assert len(hits) == len(w) and hit_multiset(hits) == hit_multiset(w)
    finally:
        ctx.set_query_index_reuse(False)


def test_refusals(ctx, monkeypatch):
    """DMND_E_ARG before any launch: a shape of weight below 10, an unsorted reference block, a length ratio beside the switch."""
    set_hooks(monkeypatch, {})
    db, doff, q, qoff = mutual_sets.generate(families=6, members=3, queries=2, seed=9)
    qd, ql, td, tl = mutual_sets.sorted_blocks(db, doff, q, qoff)
    ut, utl = workload.sequence_set(db, doff)
    assert (np.diff(np.diff(utl)) > 0).any()
    ctx.set_linsearch(True)
    upload(ctx, qd, ql, td, tl)
    assert len(ctx.seed_search(preset("fast"))) > 0
    with pytest.raises(hip.DiamondHipError, match="seed shapes of weight >= 10"):
        ctx.seed_search(preset("sensitive"))
    assert ctx.seed_hit_count() == 0                                       # nothing ran
    upload(ctx, qd, ql, ut, utl)
    with pytest.raises(hip.DiamondHipError, match="reference block length-sorted"):
        ctx.seed_search(preset("fast"))
    assert ctx.seed_hit_count() == 0
    upload(ctx, qd, ql, td, tl)
    ctx.set_min_length_ratio(0.75)
    with pytest.raises(hip.DiamondHipError, match="minimum length ratio"):
        ctx.seed_search(preset("fast"))
    assert ctx.seed_hit_count() == 0
    ctx.set_min_length_ratio(0.0)
    # the switch off takes the unsorted block and the short shapes as ever
    ctx.set_linsearch(False)
    upload(ctx, qd, ql, ut, utl)
    assert len(ctx.seed_search(preset("fast"))) > 0 and len(ctx.seed_search(preset("sensitive"))) > 0
