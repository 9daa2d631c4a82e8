"""-m gpu tests of the sliced long-seed reference stream (csrc/seed_slices_core.h, seed_stream_slices_kernel): the level-1 filter
probed from LDS slices over a routing of the reference windows that a context keeps per uploaded block. The sliced stream finds
the joins of the plain one, so the sorted hits must be identical; which stream ran and what the call did about the cache is read
from the second DMND_TRACE summary line."""
import ctypes
import os
import re
import numpy as np
import pytest
import torch

from tapfile import read_ext_tap
from diamond_amd import hip, synth, workload
from test_oracle_seed import hit_multiset
from test_gpu_seed import to_hip_params, GOLDEN

pytestmark = pytest.mark.gpu

HOOKS = ("DMND_SEED_CHAIN", "DMND_SEED_MATCHED_CAP", "DMND_SEED_SLICES", "DMND_SEED_SLICES_BUDGET_MB", "DMND_SEED_SLICES_MIN_LETTERS", "DMND_SEED_SLICE_WORDS")


def search(c, sp, monkeypatch, capfd, **env):
    """One search with the given DMND_SEED_* hooks; returns (hits, path, stream, cache, bytes held by the cache)"""
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
    m = re.search(r"\| path: (.*)", err)
    s = re.search(r"stream: (plain|slices)( \((\d+) x [0-9.]+ KB\))?, reference cache: (none|built|kept), (\d+) bytes held", err)
    assert m and s, err[-2000:]
    search.slices = int(s.group(3)) if s.group(3) else 0
    return hits, m.group(1).strip(), s.group(1), s.group(4), int(s.group(5))


def plain_hits(cfg_or_blocks, sp, monkeypatch, capfd, **env):
    """the plain stream's hits, in a fresh context"""
    c = hip.Context()
    try:
        upload(c, cfg_or_blocks)
        hits, _, stream, cache, held = search(c, sp, monkeypatch, capfd, SLICES=0, **env)
        assert (stream, cache, held) == ("plain", "none", 0)
        return hits
    finally:
        c.close()


def upload(c, b):
    if isinstance(b, dict):
        c.upload_block(hip.QUERY, b["query"]["data"], b["query"]["limits"])
        c.upload_block(hip.TARGET, b["target"]["data"], b["target"]["limits"])
    else:
        qd, ql, td, tl = b
        c.upload_block(hip.QUERY, qd, ql)
        c.upload_block(hip.TARGET, td, tl)


_taps = {}


def tap_of(name):
    if name not in _taps:
        cfg, recs = read_ext_tap(os.path.join(GOLDEN, name))
        _taps[name] = (cfg, to_hip_params(cfg), np.concatenate([r["hits"] for r in recs]))
    return _taps[name]


@pytest.mark.parametrize("tap", ["ext_fast.tap", "ext_fast_synth.tap", "ext_default_synth.tap", "ext_bjz.tap"])
def test_sliced_stream_equals_plain_and_reference(tap, monkeypatch, capfd):
    """The long-seed golden taps (ext_default_synth.tap: two shapes, two routings in one cache), host-driven and as a chain, the
    filter as one slice and cut into slices of 1024 words."""
    assert torch.cuda.is_available()
    cfg, sp, ref = tap_of(tap)
    if tap == "ext_default_synth.tap":
        assert sp.n_shapes == 2
    for chain, want_path in ((0, "host"), (1, "chain")):
        plain = plain_hits(cfg, sp, monkeypatch, capfd, CHAIN=chain)
        assert len(plain) == len(ref) and hit_multiset(plain) == hit_multiset(ref)
        for words in (None, 1024):
            c = hip.Context()
            try:
                upload(c, cfg)
                env = dict(CHAIN=chain, SLICES=1, **({} if words is None else dict(SLICE_WORDS=words)))
                got, path, stream, cache, held = search(c, sp, monkeypatch, capfd, **env)
                assert (stream, cache) == ("slices", "built") and held > 0
                assert words is None or search.slices > 1
                assert path == want_path or (chain and path.startswith("chain"))
                assert np.array_equal(got, plain)
                again, path2, stream, cache, _ = search(c, sp, monkeypatch, capfd, **env)
                assert (stream, cache) == ("slices", "kept") and np.array_equal(again, plain)
                if chain:
                    _, path_plain, _, _, _ = search(c, sp, monkeypatch, capfd, CHAIN=1, SLICES=0)
                    assert path2 == path_plain
            finally:
                c.close()


def random_block(rng, lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return workload.sequence_set(rng.integers(0, 20, int(off[-1])).astype(np.int8), off)


def family_blocks(families, members, queries, seed):
    db, doff, q, qoff = synth.generate(families, members=members, queries=queries, seed=seed)
    qd, ql = workload.sequence_set(q, qoff)
    td, tl = workload.sequence_set(db, doff)
    return qd, ql, td, tl


def check_blocks(blocks, sp, monkeypatch, capfd, min_hits=1, **env):
    """forced sliced stream == plain stream on a block pair, with 1 slice and with 64; returns the hits"""
    plain = plain_hits(blocks, sp, monkeypatch, capfd, **{k: v for k, v in env.items() if k != "SLICE_WORDS"})
    assert len(plain) >= min_hits
    for words in (None, 512):
        c = hip.Context()
        try:
            upload(c, blocks)
            e = dict(env, SLICES=1, **({} if words is None else dict(SLICE_WORDS=words)))
            for want in ("built", "kept"):
                got, _, stream, cache, _ = search(c, sp, monkeypatch, capfd, **e)
                assert (stream, cache) == ("slices", want)
                assert np.array_equal(got, plain)
        finally:
            c.close()
    return plain


def test_structural_edges(monkeypatch, capfd):
    """A block shorter than one tile; 64 slices of which at least 59 receive no window; a window range that begins and ends off
    every multiple of 16; sequences shorter than the shape."""
    assert torch.cuda.is_available()
    sp = hip.seed_params_fast(threads=1)
    qd, ql, td, tl = family_blocks(6, 4, 12, seed=5)
    # shorter than a tile of 4096 letters
    few = 6
    assert tl[few] - tl[0] < 4096
    check_blocks((qd, ql, td, tl[:few + 1].copy()), sp, monkeypatch, capfd)
    # fewer windows than slices: two sequences barely longer than the shape, searched with themselves. Most of the 64 slices receive
    # no window (counted on the CPU with the routing rule of the cache build): their workgroups have an empty list
    L = int(sp.shape_len[0])
    db0, doff0, _, _ = synth.generate(6, members=4, queries=12, seed=5)
    tiny = [db0[doff0[0]:doff0[0] + L + 2], db0[doff0[1]:doff0[1] + L + 1]]
    td1, tl1 = workload.sequence_set(np.concatenate(tiny), np.array([0, L + 2, 2 * L + 3], np.int64))
    emu = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libswipe_emu.so"))
    emu.emu_route_block.restype = ctypes.c_int64
    emu.emu_route_block.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    n_win = ((int(tl1[-1]) - (int(tl1[0]) & ~15) + 15) // 16) * 16
    routed, plain_rule = np.zeros(n_win, np.uint8), np.zeros(n_win, np.uint8)
    assert emu.emu_route_block(ctypes.byref(sp), 0, td1.ctypes.data, int(tl1[0]), int(tl1[-1]), 6, routed.ctypes.data, plain_rule.ctypes.data) == n_win
    used = np.unique(routed[routed != 0xff])
    assert 1 <= len(used) <= 5 and np.array_equal(routed, plain_rule)      # 3 + 2 windows: at least 59 of the 64 slices are empty
    check_blocks((td1, tl1, td1, tl1), sp, monkeypatch, capfd, min_hits=0)
    assert search.slices == 64
    # the window range starts and ends off a multiple of 16 (and of the tile): the block's limits without its first sequences
    n = len(tl) - 1
    k, m = next((k, m) for k in range(1, n // 2) for m in range(n, n // 2, -1) if tl[k] % 16 and tl[m] % 16 and (tl[m] - tl[k]) % 16 and (tl[m] - tl[k]) % 4096)
    check_blocks((qd, ql, td, tl[k:m + 1].copy()), sp, monkeypatch, capfd)
    # sequences shorter than the shape between the others
    rng = np.random.default_rng(11)
    db, doff, q, qoff = synth.generate(6, members=4, queries=12, seed=5)
    seqs = []
    for i in range(len(doff) - 1):
        seqs.append(db[doff[i]:doff[i + 1]])
        seqs.append(rng.integers(0, 20, int(rng.integers(1, sp.shape_len[0]))).astype(np.int8))
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    td2, tl2 = workload.sequence_set(np.concatenate(seqs), off)
    check_blocks((qd, ql, td2, tl2), sp, monkeypatch, capfd)


def test_dense_joins_fill_the_staging_area(monkeypatch, capfd):
    """The query block is the reference block: every window joins. A workgroup's share of 2.6e6 windows is several rounds of its
    loop, each with more joins than the staging area holds -- the flush inside the loop and the direct append."""
    assert torch.cuda.is_available()
    sp = hip.seed_params_fast(threads=1)
    rng = np.random.default_rng(3)
    d, l = random_block(rng, np.full(2600, 1000))
    plain = plain_hits((d, l, d, l), sp, monkeypatch, capfd)
    assert len(plain) >= 2600
    c = hip.Context()
    try:
        upload(c, (d, l, d, l))
        got, _, stream, cache, _ = search(c, sp, monkeypatch, capfd, SLICES=1)
        assert (stream, cache) == ("slices", "built") and np.array_equal(got, plain)
    finally:
        c.close()


def test_joined_position_overflow_continues(monkeypatch, capfd):
    """DMND_SEED_MATCHED_CAP=1: phase 1 runs again after the joined-position list overflowed, host-driven and after a chain"""
    assert torch.cuda.is_available()
    sp = hip.seed_params_fast(threads=1)
    blocks = family_blocks(40, 6, 60, seed=9)
    for chain in (0, 1):
        check_blocks(blocks, sp, monkeypatch, capfd, min_hits=50, CHAIN=chain, MATCHED_CAP=1)


def test_default_policy_builds_on_the_second_search(monkeypatch, capfd):
    """No DMND_SEED_SLICES: the first search of a block takes the plain stream and builds nothing, the second builds, the third keeps"""
    assert torch.cuda.is_available()
    sp = hip.seed_params_fast(threads=1)
    blocks = family_blocks(40, 6, 60, seed=9)
    c = hip.Context()
    try:
        upload(c, blocks)
        # the shipped threshold leaves a block of this size on the plain stream
        for _ in range(3):
            _, _, stream, cache, held = search(c, sp, monkeypatch, capfd)
            assert (stream, cache, held) == ("plain", "none", 0)
        seen = []
        hits = []
        for _ in range(3):
            h, _, stream, cache, _ = search(c, sp, monkeypatch, capfd, SLICES_MIN_LETTERS=1)
            seen.append((stream, cache))
            hits.append(h)
        assert seen == [("plain", "none"), ("slices", "built"), ("slices", "kept")]
        assert len(hits[0]) > 50 and np.array_equal(hits[0], hits[1]) and np.array_equal(hits[0], hits[2])
    finally:
        c.close()


def two_searches_follow(c, blocks, sp, monkeypatch, capfd, want, what):
    seen = []
    for _ in range(2):
        h, _, stream, cache, _ = search(c, sp, monkeypatch, capfd, SLICES_MIN_LETTERS=1)
        seen.append((stream, cache))
        assert np.array_equal(h, want), what
    assert seen == [("plain", "none"), ("slices", "built")], what


def test_cache_follows_the_reference_block(monkeypatch, capfd):
    """Whatever changes the letters the stream reads starts the cache over: another block of the same length, an alias of another
    context's block, masking in place, the soft-mask view. The hits follow the new content."""
    assert torch.cuda.is_available()
    sp = hip.seed_params_fast(threads=1)
    qd, ql, td, tl = family_blocks(40, 6, 60, seed=9)
    rng = np.random.default_rng(2)
    # a tandem repeat for tantan and a motif for the soft-mask view, inside sequences that the queries hit
    td = td.copy()
    td[tl[3] + 20: tl[3] + 70] = np.resize(np.array([5, 15, 5, 15, 9], np.int8), 50)
    motif = rng.integers(0, 20, 8).astype(np.int8)
    for i in range(0, len(tl) - 1, 4):
        td[tl[i] + 30: tl[i] + 38] = motif
    # another block of the same shape: the same sequences, in another order of the families' members
    lens = np.diff(tl) - 1
    perm = np.arange(len(lens)).reshape(-1, 6)[:, ::-1].reshape(-1)
    seqs = [td[tl[i]:tl[i + 1] - 1] for i in perm]
    assert sorted(lens[perm]) == sorted(lens)
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    td_b, tl_b = workload.sequence_set(np.concatenate(seqs), off)
    assert len(td_b) == len(td) and not np.array_equal(td_b, td)
    c = hip.Context()
    other = hip.Context()
    try:
        upload(c, (qd, ql, td, tl))
        want_a = plain_hits((qd, ql, td, tl), sp, monkeypatch, capfd)
        two_searches_follow(c, None, sp, monkeypatch, capfd, want_a, "first block")
        # 1. another block of the same length
        c.upload_block(hip.TARGET, td_b, tl_b)
        want_b = plain_hits((qd, ql, td_b, tl_b), sp, monkeypatch, capfd)
        assert not np.array_equal(want_a, want_b)
        two_searches_follow(c, None, sp, monkeypatch, capfd, want_b, "upload")
        # 2. an alias of another context's block
        other.upload_block(hip.TARGET, td, tl)
        c.share_block(hip.TARGET, other)
        two_searches_follow(c, None, sp, monkeypatch, capfd, want_a, "share_block")
        # 3. masked in place
        c.upload_block(hip.TARGET, td, tl)
        two_searches_follow(c, None, sp, monkeypatch, capfd, want_a, "upload again")
        masked = td.copy()
        assert c.mask_block(hip.TARGET, masked) > 10
        want_m = plain_hits((qd, ql, masked, tl), sp, monkeypatch, capfd)
        two_searches_follow(c, None, sp, monkeypatch, capfd, want_m, "mask_block")
        # 4. the soft-mask view, with a motif table of the one planted motif
        code = 0
        for x in motif:
            code = code * 20 + int(x)
        c.set_motif_table([code])
        covered = c.soft_mask_block(hip.TARGET)
        assert covered >= 8
        fresh = hip.Context()
        try:
            upload(fresh, (qd, ql, masked, tl))
            fresh.set_motif_table([code])
            assert fresh.soft_mask_block(hip.TARGET) == covered
            want_s, _, stream, _, _ = search(fresh, sp, monkeypatch, capfd, SLICES=0)
            assert stream == "plain"
        finally:
            fresh.close()
        two_searches_follow(c, None, sp, monkeypatch, capfd, want_s, "soft_mask_block")
    finally:
        c.close()
        other.close()


def test_changed_seed_params_get_their_own_routing(monkeypatch, capfd):
    """Other shapes on the same block: the routing of the first parameters is not used for the second"""
    assert torch.cuda.is_available()
    blocks = family_blocks(40, 6, 60, seed=9)
    params = hip.default_params()
    sp_fast = hip.seed_params_fast(threads=1)
    sp_two, _ = hip.seed_params_preset("default", params, threads=1)
    assert sp_two.n_shapes == 2
    want_fast = plain_hits(blocks, sp_fast, monkeypatch, capfd)
    want_two = plain_hits(blocks, sp_two, monkeypatch, capfd)
    c = hip.Context()
    try:
        upload(c, blocks)
        two_searches_follow(c, None, sp_fast, monkeypatch, capfd, want_fast, "fast")
        two_searches_follow(c, None, sp_two, monkeypatch, capfd, want_two, "default")
        h, _, stream, cache, _ = search(c, sp_two, monkeypatch, capfd, SLICES_MIN_LETTERS=1)
        assert (stream, cache) == ("slices", "kept") and np.array_equal(h, want_two)
        two_searches_follow(c, None, sp_fast, monkeypatch, capfd, want_fast, "fast again")
    finally:
        c.close()


def test_budget_zero_keeps_the_plain_stream(monkeypatch, capfd):
    """DMND_SEED_SLICES_BUDGET_MB=0: every search is plain, and the cache holds no byte -- forced or not"""
    assert torch.cuda.is_available()
    sp = hip.seed_params_fast(threads=1)
    blocks = family_blocks(40, 6, 60, seed=9)
    want = plain_hits(blocks, sp, monkeypatch, capfd)
    c = hip.Context()
    try:
        upload(c, blocks)
        for env in (dict(SLICES=1), dict(SLICES_MIN_LETTERS=1), dict(SLICES_MIN_LETTERS=1), dict(SLICES_MIN_LETTERS=1)):
            h, _, stream, cache, held = search(c, sp, monkeypatch, capfd, SLICES_BUDGET_MB=0, **env)
            assert (stream, cache, held) == ("plain", "none", 0) and np.array_equal(h, want)
    finally:
        c.close()
