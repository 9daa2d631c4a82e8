"""-m gpu: the sort-driven build of the query side (seed_kernels.hip launch_seed_build) against the oracle's seed search on blocks
made to reach its rare paths -- distinct seeds with equal order values, a seed repeated 10^5 times among seeds of the same home
slot (the long-run regrouping), and a table so full that placements run past the last slot (the wrap-around insertion)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle_py as orc
from diamond_amd import hip

pytestmark = pytest.mark.gpu
M32 = np.uint64(0xFFFFFFFF)


def hash_a(keys):
    lo, hi = keys & M32, keys >> np.uint64(32)
    a = (lo * np.uint64(0x9E3779B1) + hi * np.uint64(0x85EBCA6B)) & M32
    a ^= a >> np.uint64(15)
    a = (a * np.uint64(0x2C1B3C6D)) & M32
    a ^= a >> np.uint64(13)
    return a


def shape(p):
    pos = np.array([p.shape_pos[0][k] for k in range(p.shape_weight[0])])
    red = np.array([p.reduction[i] for i in range(32)])
    inv = np.array([int(np.flatnonzero(red[:20] == c)[0]) for c in range(p.reduction_size)])
    return pos, inv, int(p.shape_len[0])


def random_keys(rng, p, n):
    pos, _, _ = shape(p)
    cls = rng.integers(0, p.reduction_size, (n, len(pos))).astype(np.uint64)
    return (cls << (np.uint64(4) * pos.astype(np.uint64))[None, :]).sum(axis=1, dtype=np.uint64), cls


def window(p, cls_row):
    pos, inv, L = shape(p)
    w = np.zeros(L, np.int8)                              # non-care positions: letter 0
    w[pos] = inv[cls_row]
    return w


def blocks(seqs):
    """SequenceSet layout: 256 delimiters, then each sequence followed by one, then 256 more."""
    lens = np.array([len(s) for s in seqs])
    limits = 256 + np.concatenate([[0], np.cumsum(lens + 1)])
    out = np.full(int(limits[-1]) + 256, 31, np.int8)
    for s, b in zip(seqs, limits[:-1]):
        out[b:b + len(s)] = s
    return out, limits.astype(np.int64)


def oracle_cfg(p):
    oc = orc.SeedCfg()
    oc.seedp_bits, oc.index_chunks, oc.hamming_filter_id, oc.n_shapes = p.seedp_bits, p.index_chunks, p.hamming_filter_id, p.n_shapes
    oc.shape_len[0], oc.shape_weight[0], oc.shape_mask[0] = p.shape_len[0], p.shape_weight[0], p.shape_mask[0]
    for k in range(p.shape_weight[0]):
        oc.shape_pos[0][k] = p.shape_pos[0][k]
    for i in range(32):
        oc.reduction[i] = p.reduction[i]
    oc.reduction_size, oc.ungapped_window, oc.left_most_interval, oc.seed_complexity_cut = p.reduction_size, 48, 32, p.seed_complexity_cut
    oc.tile_size, oc.simd_lanes = p.tile_size, p.simd_lanes
    return oc


def hit_set(h):
    return set(zip(h["query"].tolist(), h["subject"].tolist(), h["seed_offset"].tolist(), h["score"].tolist()))


def search_both(p, qseqs, tseqs):
    qd, ql = blocks(qseqs)
    td, tl = blocks(tseqs)
    ctx = hip.Context()
    try:
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, td, tl)
        got = ctx.seed_search(p)
    finally:
        ctx.close()
    want = orc.seed_search(oracle_cfg(p), qd, ql, td, tl)
    return got, want


def slot_bits_of(qseqs):
    """log2 of the table's slots for a long-seed block (seed_api.hip seed_sizes: two slots per query position, at least 1024)."""
    n = sum(len(s) + 1 for s in qseqs)
    b = 10
    while (1 << b) < 2 * n:
        b += 1
    return b


def embed(rng, w, flank=12):
    return np.concatenate([rng.integers(0, 20, flank), w, rng.integers(0, 20, flank)]).astype(np.int8)


def test_distinct_seeds_with_equal_order_values():
    assert torch.cuda.is_available()
    p = hip.seed_params_fast(threads=8)
    rng = np.random.default_rng(11)
    keys, cls = random_keys(rng, p, 200_000)
    keys, first = np.unique(keys, return_index=True)
    cls = cls[first]
    h = hash_a(keys)
    _, inv, cnt = np.unique(h, return_inverse=True, return_counts=True)
    pair = np.flatnonzero(cnt[inv] > 1)                   # distinct keys whose hash a (the order value) is the same
    assert len(pair) >= 4
    background = rng.choice(len(keys), 2000, replace=False)
    qseqs = [embed(rng, window(p, cls[i])) for i in np.concatenate([pair, background])]
    rng.shuffle(qseqs)
    tseqs = [s.copy() for s in qseqs[::3]] + [embed(rng, window(p, cls[i])) for i in pair]
    got, want = search_both(p, qseqs, tseqs)
    assert len(got) == len(want) > 500 and hit_set(got) == hit_set(want)


def test_a_seed_repeated_1e5_times_among_seeds_of_its_home_slot():
    p = hip.seed_params_fast(threads=8)
    rng = np.random.default_rng(12)
    keys, cls = random_keys(rng, p, 1)
    rep = embed(rng, window(p, cls[0]), flank=4)
    n_rep = 100_000
    bits = slot_bits_of([rep] * (n_rep + 8))
    t0 = hash_a(keys)[0] >> np.uint64(32 - bits)
    mates = []
    for _ in range(16):                                   # keys of the same home slot, by brute force
        k, c = random_keys(rng, p, 4_000_000)
        same = np.flatnonzero((hash_a(k) >> np.uint64(32 - bits)) == t0)
        mates += [c[i] for i in same if k[i] != keys[0]]
        if len(mates) >= 3:
            break
    assert len(mates) >= 2
    mate_seqs = [embed(rng, window(p, c), flank=4) for c in mates]
    qseqs = [rep] * n_rep
    for i, s in enumerate(mate_seqs):                     # among the repeats: their positions interleave in the sorted run
        for at in (1000 + 7 * i, 50_000 + 11 * i, 99_000 + i):
            qseqs.insert(at, s)
    assert slot_bits_of(qseqs) == bits
    tseqs = [rep] + mate_seqs
    got, want = search_both(p, qseqs, tseqs)
    assert len(got) == len(want) >= n_rep and hit_set(got) == hit_set(want)


FULL_TABLE = r"""
import sys
sys.path[:0] = {paths!r}
import numpy as np
import test_gpu_seed_build as t
from diamond_amd import hip
p = hip.seed_params_fast(threads=8)
rng = np.random.default_rng(13)
q = [rng.integers(0, 20, 300).astype(np.int8) for _ in range(405)]    # 122 310 positions for 131 072 slots
tseqs = []
for s in q[::2]:
    m = s.copy()
    flip = rng.random(len(m)) < 0.1
    m[flip] = rng.integers(0, 20, int(flip.sum()))
    tseqs.append(m)
got, want = t.search_both(p, q, tseqs)
assert len(got) == len(want) > 1000 and t.hit_set(got) == t.hit_set(want), (len(got), len(want))
print("ok", len(got))
"""


def test_a_full_table_takes_the_wrap_around_insertion():
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, DMND_SEED_SLOTS_X8="8")        # one slot per query position (tuning is read once per process)
    code = FULL_TABLE.format(paths=[here, root, os.path.join(root, "oracle")])
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
