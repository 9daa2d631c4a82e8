"""-m gpu tests of the chain mode of the long-seed seed search (csrc/seed_chain.h): the search enqueued without a host wait,
its sizes read from device memory, one readback -- and the host-driven code as its continuation where the status word asks
for one. Every case compares chain on, chain off (DMND_SEED_CHAIN) and the reference's tapped hits; the path taken is read
from the DMND_TRACE summary line."""
import os
import re
import numpy as np
import pytest
import torch

from tapfile import read_ext_tap
from diamond_amd import hip, workload
from test_oracle_seed import hit_multiset
from test_gpu_seed import to_hip_params, GOLDEN

pytestmark = pytest.mark.gpu

HOOKS = ("DMND_SEED_CHAIN", "DMND_SEED_MATCHED_CAP", "DMND_SEED_SURVIVOR_CAP", "DMND_SEED_HIT_CAP", "DMND_SEED_DEFERRED_CAP", "DMND_SEED_TILED", "DMND_SEED_SORT_CAP",
         "DMND_SEED_READBACK_BYTES", "DMND_SEED_FUSED", "DMND_SEED_CLASSES_LONG")


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    c = hip.Context()
    yield c
    c.close()


_taps = {}


def tap_of(name, hashed=False):
    """(config, seed parameters, reference hits) of a golden tap, read once"""
    if (name, hashed) not in _taps:
        cfg, recs = read_ext_tap(os.path.join(GOLDEN, name))
        _taps[(name, hashed)] = (cfg, to_hip_params(dict(cfg, seed_encoding=1) if hashed else cfg), np.concatenate([r["hits"] for r in recs]))
    return _taps[(name, hashed)]


def tap_without_deferred_pairs(name="ext_default_synth.tap"):
    """A two-shape tap with the ungapped filter, cut down to the queries that have no hit scoring 200 or more: no pair of it
    reaches the 255 that defers a pair to the second pass, so the whole search -- both shapes' pair filters, scoring and
    left-most rule on device-side offsets, and the sort with its pass over the scores -- stays on the chain. A query's hits do
    not depend on the other queries of the block: the reference hits are the tap's, restricted and renumbered."""
    if ("no deferred", name) not in _taps:
        cfg, sp, ref = tap_of(name)
        qd, ql = cfg["query"]["data"], cfg["query"]["limits"]
        nq = len(ql) - 1
        bad = np.zeros(nq, bool)
        bad[np.unique(ref["query"][ref["score"] >= 200])] = True
        keep = np.flatnonzero(~bad)
        seqs = [qd[ql[i]:ql[i + 1] - 1] for i in keep]
        off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
        data, limits = workload.sequence_set(np.concatenate(seqs), off)
        new_id = np.full(nq, -1, np.int64)
        new_id[keep] = np.arange(len(keep))
        r = ref[~bad[ref["query"]]].copy()
        r["query"] = new_id[r["query"]]
        assert sp.n_shapes == 2 and sp.use_ungapped and len(r) > 100 and len(np.unique(r["score"])) > 10
        _taps[("no deferred", name)] = (dict(cfg, query=dict(n=len(keep), data=data, limits=limits)), sp, r)
    return _taps[("no deferred", name)]


def upload(c, cfg):
    c.upload_block(hip.QUERY, cfg["query"]["data"], cfg["query"]["limits"])
    c.upload_block(hip.TARGET, cfg["target"]["data"], cfg["target"]["limits"])


def search(c, sp, monkeypatch, capfd, **env):
    """One search with the given hooks set; returns (hits, path named by the trace line, joined positions per shape); the
    deferred pairs per shape that the trace line reports are left in search.deferred"""
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("DMND_SEED_" + k, str(v))
    monkeypatch.setenv("DMND_TRACE", "1")
    capfd.readouterr()
    hits = c.seed_search(sp)
    err = capfd.readouterr().err
    monkeypatch.delenv("DMND_TRACE")
    for k in env:
        monkeypatch.delenv("DMND_SEED_" + k)
    m = re.search(r"joined reference positions per shape:((?: \d+)+) \|.*\| deferred:((?: \d+)+) \|.*\| path: (.*)", err)
    assert m, err[-2000:]
    search.deferred = [int(x) for x in m.group(2).split()]
    return hits, m.group(3).strip(), [int(x) for x in m.group(1).split()]


def check(c, sp, ref, monkeypatch, capfd, want_path, **env):
    """chain (with the hooks) == host-driven path == the reference's hits; returns the chain's hits"""
    off, path_off, _ = search(c, sp, monkeypatch, capfd, CHAIN=0, **{k: v for k, v in env.items() if k == "FUSED"})
    assert path_off == "host"
    check.deferred = search.deferred
    on, path_on, counts = search(c, sp, monkeypatch, capfd, CHAIN=1, **env)
    assert np.array_equal(on, off)
    assert len(on) == len(ref) and hit_multiset(on) == hit_multiset(ref)
    if callable(want_path):
        assert want_path(path_on), path_on
    else:
        assert path_on == want_path
    return on, counts


@pytest.mark.parametrize("tap,hashed", [("ext_fast.tap", False), ("ext_fast_synth.tap", False), ("ext_default_synth.tap", False), ("ext_default.tap", False),
                                        ("ext_bjz.tap", False), ("ext_hashed.tap", True)])
def test_chain_equals_host_path_and_reference(ctx, tap, hashed, monkeypatch, capfd):
    """One long shape, two shapes (device-side offsets between the shapes), query-indexed keys. An input without deferred pairs
    stays on the chain; ext_default.tap has scores above 255: its deferred pass is the host's."""
    cfg, sp, ref = tap_of(tap, hashed)
    upload(ctx, cfg)
    if tap in ("ext_default.tap", "ext_default_synth.tap"):
        assert sp.n_shapes == 2
    hits, _ = check(ctx, sp, ref, monkeypatch, capfd, lambda p: p.startswith("chain"))
    _, path, _ = search(ctx, sp, monkeypatch, capfd, CHAIN=1)
    first_deferred = [i for i, d in enumerate(check.deferred) if d]      # (counted by the host-driven path)
    if tap == "ext_default.tap":
        assert first_deferred and (ref["score"] > 255).any()
    assert path == ("chain, then host from the deferred pass of shape %d" % first_deferred[0] if first_deferred else "chain")
    assert (np.diff(hits["query"].astype(np.int64)) >= 0).all()
    # the default (no DMND_SEED_CHAIN) is the chain; a context that just met deferred pairs leaves it out for a few searches
    c = hip.Context()
    try:
        upload(c, cfg)
        for k in range(3):
            got, path_k, _ = search(c, sp, monkeypatch, capfd)
            assert path_k == (path if k == 0 or not first_deferred else "host") and np.array_equal(got, hits)
    finally:
        c.close()


def test_two_shapes_with_the_ungapped_filter_stay_on_the_chain(ctx, monkeypatch, capfd):
    """No deferred pairs: shape 0's end-of-shape kernel, the gate, shape 1's pair filter / scoring / left-most rule on its
    device-side range, and the two-pass device sort all run, and nothing is left to the host."""
    cfg, sp, ref = tap_without_deferred_pairs()
    upload(ctx, cfg)
    hits, counts = check(ctx, sp, ref, monkeypatch, capfd, "chain")
    assert check.deferred == [0, 0] and min(counts) > 0
    assert (np.diff(hits["query"].astype(np.int64)) >= 0).all()
    got, path, _ = search(ctx, sp, monkeypatch, capfd)      # the default
    assert path == "chain" and np.array_equal(got, hits)


def test_by_class_stream_on_the_chain(ctx, monkeypatch, capfd):
    """Long seeds by key class (DMND_SEED_CLASSES_LONG=1): the by-class stream kernel appends through the same cumulative
    counters. The default leaves the chain out there; forced, it gives the host path's hits."""
    for cfg, sp, ref in (tap_of("ext_fast_synth.tap"), tap_without_deferred_pairs()):
        upload(ctx, cfg)
        off, path_off, _ = search(ctx, sp, monkeypatch, capfd, CHAIN=0, CLASSES_LONG=1)
        on, path_on, _ = search(ctx, sp, monkeypatch, capfd, CHAIN=1, CLASSES_LONG=1)
        assert path_off == "host" and path_on == "chain"
        assert np.array_equal(on, off) and len(on) == len(ref) and hit_multiset(on) == hit_multiset(ref)
        _, path, _ = search(ctx, sp, monkeypatch, capfd, CLASSES_LONG=1)
        assert path == "host"


def test_forced_continuations_at_tiny_capacities(ctx, monkeypatch, capfd):
    """Every buffer of the chain too small in turn (the existing hooks), on a two-shape tap: same hits, the fallback point named
    in the trace line, and the call after it, without the hook, takes the chain again."""
    cfg, sp, ref = tap_without_deferred_pairs()
    upload(ctx, cfg)
    _, clean, counts = search(ctx, sp, monkeypatch, capfd, CHAIN=1)
    assert clean == "chain" and len(counts) == 2 and counts[1] >= 2
    between = counts[0] + counts[1] // 2                     # the first shape fits, the second one overflows
    cases = [(dict(MATCHED_CAP=1), "chain, then host from phase 1 (joined positions over capacity)"),
             (dict(MATCHED_CAP=between), "chain, then host from phase 1 (joined positions over capacity)"),
             (dict(SURVIVOR_CAP=5), "chain, then host from the pair filter of shape 0 (survivors over capacity)"),
             (dict(HIT_CAP=10), "chain, then host from phase 2 (hits over capacity)"),
             (dict(TILED=1), "chain, then host from the pair filter of shape 0 (tiled filter)")]
    for env, want in cases:
        check(ctx, sp, ref, monkeypatch, capfd, want, **env)
        got, path, _ = search(ctx, sp, monkeypatch, capfd, CHAIN=1)
        assert path == clean and hit_multiset(got) == hit_multiset(ref)


def test_deferred_pairs_in_an_early_shape_of_many(ctx, monkeypatch, capfd):
    """Sixteen short shapes through the list-based path (DMND_SEED_FUSED=0) with deferred pairs in an early shape: the kernels of
    the shapes behind it do nothing -- the left-most rule of a later shape does not find the earlier shape's scored list again --
    and the host continues with the deferred pass of that shape and the pair filters of the following ones."""
    cfg, sp, ref = tap_of("ext_sensitive.tap")
    upload(ctx, cfg)
    check(ctx, sp, ref, monkeypatch, capfd, lambda p: p.startswith("chain"), FUSED=0)
    first_deferred = [i for i, d in enumerate(check.deferred) if d]
    assert first_deferred and first_deferred[0] < sp.n_shapes - 1
    _, path, _ = search(ctx, sp, monkeypatch, capfd, CHAIN=1, FUSED=0)
    assert path == "chain, then host from the deferred pass of shape %d" % first_deferred[0]


def test_deferred_pairs_over_the_chains_capacity_run_phase_2_again(ctx, monkeypatch, capfd):
    """The chain's deferred list one entry long (DMND_SEED_DEFERRED_CAP=1) on a tap whose first shape with deferred pairs has
    more than one: the list the chain left is incomplete, so nothing of it is kept and the host runs phase 2 again for every
    shape with a list that has grown to the count the chain read back."""
    cfg, sp, ref = tap_of("ext_default.tap")
    upload(ctx, cfg)
    assert (ref["score"] > 255).any()
    check(ctx, sp, ref, monkeypatch, capfd, lambda p: p.startswith("chain, then host from the deferred pass of shape"), DEFERRED_CAP=1)
    first_deferred = [d for d in check.deferred if d]        # (counted by the host-driven path)
    assert first_deferred and first_deferred[0] > 1


def masked_query_block():
    """three sequences of masked letters: no position has a seed"""
    q = np.full(180, 23, np.int8)
    return workload.sequence_set(q, np.array([0, 60, 120, 180], np.int64))


def test_empty_and_repeated_searches_read_no_stale_count(ctx, monkeypatch, capfd):
    many_cfg, many_sp, many_ref = tap_of("ext_default_synth.tap")
    few_cfg, few_sp, few_ref = tap_of("ext_bjz.tap")
    assert len(many_ref) > len(few_ref) > 0
    # a fresh context's first call
    c = hip.Context()
    try:
        upload(c, few_cfg)
        got, path, _ = search(c, few_sp, monkeypatch, capfd, CHAIN=1)
        assert path.startswith("chain") and len(got) == len(few_ref) and hit_multiset(got) == hit_multiset(few_ref)
        first = got
    finally:
        c.close()
    # a search right after one with more hits on the same context
    upload(ctx, many_cfg)
    got, path, _ = search(ctx, many_sp, monkeypatch, capfd, CHAIN=1)
    assert path.startswith("chain") and hit_multiset(got) == hit_multiset(many_ref)
    upload(ctx, few_cfg)
    got, path, _ = search(ctx, few_sp, monkeypatch, capfd, CHAIN=1)
    assert path.startswith("chain") and np.array_equal(got, first)
    # a query block that joins nothing: no hits, and the previous search's are not left behind
    qd, ql = masked_query_block()
    ctx.upload_block(hip.QUERY, qd, ql)
    for chain in (1, 0):
        got, path, counts = search(ctx, few_sp, monkeypatch, capfd, CHAIN=chain)
        assert len(got) == 0 and sum(counts) == 0
        assert path == ("chain" if chain else "host")


def test_readback_budget_spills_to_a_second_copy(ctx, monkeypatch, capfd):
    cfg, sp, ref = tap_of("ext_fast_synth.tap")
    upload(ctx, cfg)
    assert len(ref) * hip.SEED_HIT_DTYPE.itemsize > 64
    check(ctx, sp, ref, monkeypatch, capfd, "chain", READBACK_BYTES=64)
    check(ctx, sp, ref, monkeypatch, capfd, "chain", READBACK_BYTES=0)


def test_padded_sort_at_its_capacity_edges(ctx, monkeypatch, capfd):
    """The device-sized sort runs over a fixed capacity padded with keys that sort last: hit counts of capacity - 1, capacity
    and capacity + 1 (the last one is sorted by the host's launches); with and without the pass over the scores."""
    for cfg, sp, ref in (tap_of("ext_fast_synth.tap"), tap_without_deferred_pairs()):
        upload(ctx, cfg)
        n = len(ref)
        assert n > 2
        _, clean, _ = search(ctx, sp, monkeypatch, capfd, CHAIN=1)
        assert clean == "chain"
        check(ctx, sp, ref, monkeypatch, capfd, "chain", SORT_CAP=n + 1)
        check(ctx, sp, ref, monkeypatch, capfd, "chain", SORT_CAP=n)
        check(ctx, sp, ref, monkeypatch, capfd, "chain, then host from the hit sort", SORT_CAP=n - 1)
