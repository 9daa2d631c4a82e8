"""-m gpu tests of the sliced long-seed stream's stored hashes (csrc/seed_slices_core.h: the cache keeps hash a of every listed
window's key, seed_stream_slices_kernel probes the level-1 filter from it and forms the key only for the positives). The hits are
exact: sorted, they must be identical to the plain stream's of a fresh context, host-driven and as a chain."""
import numpy as np
import pytest
import torch

from diamond_amd import hip, workload
from test_gpu_seed_slices import search, plain_hits, upload

pytestmark = pytest.mark.gpu


def check(blocks, sp, monkeypatch, capfd, words=(None,), min_hits=0, max_hits=None):
    """forced sliced stream (built, then kept) == plain stream, for every slice size of `words`; returns the plain hits"""
    plain = None
    for chain in (0, 1):
        plain = plain_hits(blocks, sp, monkeypatch, capfd, CHAIN=chain)
        assert len(plain) >= min_hits and (max_hits is None or len(plain) <= max_hits)
        for w in words:
            c = hip.Context()
            try:
                upload(c, blocks)
                env = dict(CHAIN=chain, SLICES=1, **({} if w is None else dict(SLICE_WORDS=w)))
                for want in ("built", "kept"):
                    got, _, stream, cache, held = search(c, sp, monkeypatch, capfd, **env)
                    assert (stream, cache) == ("slices", want) and held > 0
                    assert np.array_equal(got, plain)
            finally:
                c.close()
    return plain


def blocks_of(seqs_q, seqs_t):
    def one(seqs):
        off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
        return workload.sequence_set(np.concatenate(seqs), off)
    qd, ql = one(seqs_q)
    td, tl = one(seqs_t)
    return qd, ql, td, tl


def random_seqs(rng, n, length):
    return [rng.integers(0, 20, length).astype(np.int8) for _ in range(n)]


def test_every_window_is_a_positive(monkeypatch, capfd):
    """(a) the reference is the query sequences, twelve times: nearly every window passes level 1 and joins -- whole queues of
    positives inside the loop, more joins per probe than the staging area holds (direct append); a wrong stored hash loses a hit"""
    assert torch.cuda.is_available()
    sp = hip.seed_params_fast(threads=1)
    q = random_seqs(np.random.default_rng(1), 150, 100)
    blocks = blocks_of(q, q * 12)
    assert blocks[3][-1] - blocks[3][0] <= 200_000
    check(blocks, sp, monkeypatch, capfd, words=(None, 512), min_hits=150 * 12)


def test_no_positive_at_all(monkeypatch, capfd):
    """(b) an unrelated random reference: nothing joins, and an empty result equals an empty result"""
    assert torch.cuda.is_available()
    sp = hip.seed_params_fast(threads=1)
    rng = np.random.default_rng(2)
    blocks = blocks_of(random_seqs(rng, 20, 100), random_seqs(rng, 500, 300))
    check(blocks, sp, monkeypatch, capfd, words=(None, 512), max_hits=0)


def test_fewer_positives_than_one_queue(monkeypatch, capfd):
    """(c) one reference sequence of 40 letters, equal to a query: fewer than 64 positives in all -- only the probe behind the loop"""
    assert torch.cuda.is_available()
    sp = hip.seed_params_fast(threads=1)
    q = random_seqs(np.random.default_rng(3), 12, 40)
    check(blocks_of(q, [q[5]]), sp, monkeypatch, capfd, words=(None, 512), min_hits=1)


@pytest.mark.parametrize("filler", [300, 301, 307, 315])
def test_joins_at_both_ends_of_the_block(filler, monkeypatch, capfd):
    """(d) the block's first sequence begins with the first window of a query and its last one ends with the last window of another:
    the only joins of the two are at the block's first and last window, whose key takes the nibbles of the group behind it -- for the
    last window those behind the block's end. The filler moves that end over the positions of a group of 16."""
    assert torch.cuda.is_available()
    sp = hip.seed_params_fast(threads=1)
    rng = np.random.default_rng(4)
    L = int(sp.shape_len[0])
    q = random_seqs(rng, 10, 60)
    head = np.concatenate([q[2][:L], rng.integers(0, 20, 40).astype(np.int8)])
    tail = np.concatenate([rng.integers(0, 20, 40).astype(np.int8), q[7][-L:]])
    blocks = blocks_of(q, [head] + random_seqs(rng, 3, filler) + [tail])
    tl = blocks[3]
    plain = check(blocks, sp, monkeypatch, capfd, words=(None, 512), min_hits=2)
    assert sorted(plain["subject"].tolist()) == [int(tl[0]), int(tl[-1]) - 1 - L]


def test_empty_slices_and_lists_shorter_than_a_round(monkeypatch, capfd):
    """(e) 64 slices on a 200-letter block: most slices receive no window, no list fills one round of its workgroup.
    (DMND_SEED_SLICE_WORDS=512: the smallest filter has 32 768 words and a search has at most 64 slices -- with 64-word slices
    seed_slice_bits finds no slice count and the search takes the plain stream.)"""
    assert torch.cuda.is_available()
    sp = hip.seed_params_fast(threads=1)
    rng = np.random.default_rng(5)
    q = random_seqs(rng, 8, 50)
    blocks = blocks_of(q, [q[1], q[6]] + random_seqs(rng, 2, 48))
    assert blocks[3][-1] - blocks[3][0] <= 200 + 4
    check(blocks, sp, monkeypatch, capfd, words=(512,), min_hits=2)
    assert search.slices == 64


def test_kept_until_another_block_is_uploaded(monkeypatch, capfd):
    """(g) the second search of a context keeps the cache -- list, hashes and nibbles, all counted in the bytes held -- and returns the
    same hits; after another block is uploaded the search builds again and follows the new letters"""
    assert torch.cuda.is_available()
    sp = hip.seed_params_fast(threads=1)
    rng = np.random.default_rng(6)
    q = random_seqs(rng, 40, 80)
    a = blocks_of(q, q[:20] + random_seqs(rng, 30, 90))
    b = blocks_of(q, random_seqs(rng, 30, 90) + q[20:])
    want_a, want_b = (plain_hits(x, sp, monkeypatch, capfd) for x in (a, b))
    assert len(want_a) >= 20 and len(want_b) >= 20 and not np.array_equal(want_a, want_b)
    c = hip.Context()
    try:
        upload(c, a)
        seen = []
        for want in (want_a, want_a, want_a):
            got, _, stream, cache, held = search(c, sp, monkeypatch, capfd, SLICES=1)
            seen.append((stream, cache))
            assert np.array_equal(got, want)
            # nibbles + per window a list entry and a hash, + the slice counts: more than 8 bytes per window
            windows = ((int(a[3][-1]) - (int(a[3][0]) & ~15) + 15) // 16) * 16
            assert held >= 8 * windows
        assert seen == [("slices", "built"), ("slices", "kept"), ("slices", "kept")]
        c.upload_block(hip.TARGET, b[2], b[3])
        for want_cache in ("built", "kept"):
            got, _, stream, cache, _ = search(c, sp, monkeypatch, capfd, SLICES=1)
            assert (stream, cache) == ("slices", want_cache) and np.array_equal(got, want_b)
    finally:
        c.close()
