"""-m gpu tests of the kernels around the reference stream of a long-seed search, at their structural edges: the query keys taken 16
positions per thread (seed_order16_kernel), the left-most rule's wide windows (LmWide), the padded hit sort sized by the context's last
hit count, and the query ids filled at the upload. Every case compares the device's hits with the oracle's (oracle_py.seed_search)
on small crafted block pairs."""
import numpy as np
import pytest
import torch

import oracle_py as orc
from diamond_amd import hip, workload
from test_oracle_seed import hit_multiset
from test_gpu_seed import to_hip_params
from test_gpu_seed_chain import tap_of, search

pytestmark = pytest.mark.gpu

MURPHY10 = np.array([0, 1, 2, 2, 3, 2, 2, 4, 5, 6, 6, 1, 6, 7, 8, 9, 9, 7, 7, 6], np.int8)      # class of the 20 amino acids
CARE, NO_CARE = 3, 2                                         # a care and a non-care position of the --fast shape 1101110101101111
X, STOP, B, J, Z = 23, 24, 20, 21, 22


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    c = hip.Context()
    yield c
    c.close()


def cfg_of(tap, **over):
    cfg = {k: v for k, v in tap_of(tap)[0].items() if k not in ("query", "target")}
    cfg.update(over)
    if cfg.get("seed_encoding"):
        cfg["index_chunks"] = 1                              # the query-indexed mode runs with one index chunk
    return cfg


def fast(**over):
    return cfg_of("ext_fast.tap", **over)


def default(**over):
    return cfg_of("ext_default.tap", **over)


def blocks(seqs):
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    return workload.sequence_set(np.concatenate(seqs).astype(np.int8), off)


_matrix = []


def both_params(cfg, window=None, translated=None):
    """the device's and the oracle's parameters of one configuration"""
    if not _matrix:
        _matrix.append(hip.matrix_of(hip.default_params()))
    p, o = to_hip_params(cfg), orc.seed_cfg_from_tap(cfg, _matrix[0])
    o.seed_encoding = int(cfg.get("seed_encoding", 0))
    for x in (p, o):
        if window is not None:
            x.ungapped_window = window
        if translated is not None:
            x.query_translated = translated
    return p, o


def compare(c, cfg, qseqs, tseqs, **kw):
    """uploads the two blocks, searches, and checks the hits against the oracle's; returns the hits"""
    (qd, ql), (td, tl) = blocks(qseqs), blocks(tseqs)
    p, o = both_params(cfg, **kw)
    c.upload_block(hip.QUERY, qd, ql)
    c.upload_block(hip.TARGET, td, tl)
    hits = c.seed_search(p)
    want = orc.seed_search(o, qd, ql, td, tl)
    assert len(hits) == len(want) and hit_multiset(hits) == hit_multiset(want)
    return hits


def protein(rng, n):
    return rng.integers(0, 20, n).astype(np.int8)


def mutated(rng, seq, rate):
    out = seq.copy()
    m = rng.random(len(seq)) < rate
    out[m] = rng.integers(0, 20, int(m.sum()))
    return out


def other_class(rng, seq):
    """letters of another reduced class than the given ones: no window over them shares a seed with the original"""
    out = seq.copy()
    for i, l in enumerate(seq):
        while MURPHY10[out[i]] == MURPHY10[l]:
            out[i] = rng.integers(0, 20)
    return out


def offsets_of(hits, query):
    return sorted(hits["seed_offset"][hits["query"] == query].tolist())


# ---- query keys ---------------------------------------------------------------------------------------------------------

def edge_block(rng):
    """Sequences of 15, 16 and 17 letters (no, one and two windows of a 16-letter shape), one that ends on a 16-position group edge,
    one that ends on the edge of a workgroup's 4096 positions, and a block length that is a multiple of neither"""
    lens = [15, 16, 17]
    at = 256 + sum(n + 1 for n in lens)                      # block offset of the next sequence
    lens.append(44 + (-(at + 45)) % 16)                      # ... ends on a group edge
    at += lens[-1] + 1
    assert at % 16 == 0
    while at + 300 < 256 + 4096:
        lens.append(int(rng.integers(30, 200)))
        at += lens[-1] + 1
    lens.append(256 + 4096 - at - 1)                         # ... ends on the workgroup's edge
    at += lens[-1] + 1
    assert at == 256 + 4096 and lens[-1] >= 17
    for n in (23, 61, 130, 18):
        lens.append(n)
        at += n + 1
    assert at % 16 != 0 and (at - 256) % 4096 != 0
    return [protein(rng, n) for n in lens], len(lens) - 5


@pytest.mark.parametrize("name,cfg", [("fast", fast()), ("fast, query-indexed", fast(seed_encoding=1)), ("default: shapes of 12 and 15 letters", default()),
                                      ("default, query-indexed", default(seed_encoding=1))], ids=lambda x: x if isinstance(x, str) else "")
def test_query_keys_at_sequence_and_group_edges(ctx, name, cfg):
    rng = np.random.default_rng(11)
    qs, wg_edge = edge_block(rng)
    ts = [q.copy() if len(q) < 20 else mutated(rng, q, 0.06) for q in qs] + [protein(rng, 90) for _ in range(5)]
    hits = compare(ctx, cfg, qs, ts)
    found = set(hits["query"].tolist())
    if name.startswith("fast"):
        assert 0 not in found and 1 in found and 2 in found      # 15, 16 and 17 letters
        assert offsets_of(hits, 1) == [0]
    assert 3 in found and wg_edge in found and wg_edge + 1 in found and len(found) > len(qs) // 2
    # the last window of the sequence that ends on the workgroup's edge, and the first one of the next sequence
    last = compare(ctx, cfg, [qs[wg_edge], qs[wg_edge + 1]], [qs[wg_edge][-16:], qs[wg_edge + 1][:16]])
    if name.startswith("fast"):
        assert offsets_of(last, 0) == [len(qs[wg_edge]) - 16] and offsets_of(last, 1) == [0]


@pytest.mark.parametrize("hashed", [0, 1])
def test_query_keys_with_mask_stop_and_ambiguity_letters(ctx, hashed):
    """X, '*', B, J and Z at a care and at a non-care position of the window, in the query alone and in both sequences; runs of
    masked letters at the start of a sequence (the query-indexed iterator reduces those blindly)"""
    rng = np.random.default_rng(12 + hashed)
    qs, ts = [], []
    for letter in (X, STOP, B, J, Z):
        for pos in (CARE, NO_CARE):
            for both in (False, True):
                q = protein(rng, 50)
                t = q.copy()
                q[20 + pos] = letter
                if both:
                    t[20 + pos] = letter
                qs.append(q); ts.append(t)
    for run in (1, 3, 17):
        q = protein(rng, 60)
        q[:run] = X
        qs.append(q); ts.append(q.copy())
    q = protein(rng, 60)
    q[-2:] = STOP
    qs.append(q); ts.append(q.copy())
    for _ in range(10):
        q = protein(rng, 80)
        for l in (X, STOP, B, J, Z):
            q[rng.integers(0, 80, 2)] = l
        qs.append(q); ts.append(mutated(rng, q, 0.05))
    hits = compare(ctx, fast(seed_encoding=hashed), qs, ts)
    assert len(set(hits["query"].tolist())) > 20


def test_low_complexity_seed_of_the_query_indexed_mode_masks_its_letters(ctx):
    """A repetitive stretch inside a conserved region: the query-indexed algorithm drops its seeds and masks their letters when it
    enumerates them, which the left-most rule of the neighbouring seeds then sees. The rule reads letters, not the index: dropping
    the seeds alone leaves their windows standing as left neighbours. So a pair behind the stretch that the oracle keeps with the
    complexity filter and drops without it is kept only because the key kernel lowered mask_time under its left neighbours."""
    rng = np.random.default_rng(13)
    qs = []
    for k in range(12):
        q = protein(rng, 120)
        q[40:40 + 18 + k] = [0, 15][k % 2]                   # A or S, one class
        qs.append(q)
    cfg = fast(seed_encoding=1)
    hits = compare(ctx, cfg, qs, qs)
    qd, ql = blocks(qs)
    unfiltered = orc.seed_search(both_params(dict(cfg, seed_complexity_cut=0.0))[1], qd, ql, qd, ql)
    pairs = lambda h: set(zip(h["query"].tolist(), h["subject"].tolist(), h["seed_offset"].tolist()))
    kept_by_mask = pairs(hits) - pairs(unfiltered)
    assert len({q for q, _, _ in kept_by_mask}) >= 4         # (the stretches of 24 letters and more)
    assert all(40 < off < 80 and sub == ql[q] + off for q, sub, off in kept_by_mask)      # behind the stretch, on the main diagonal


def test_parameters_outside_the_preconditions_take_the_one_position_kernel(ctx):
    """a shape of 20 letters: neither the 16-position key kernel nor the stream's fast form applies, the hits are the oracle's"""
    pos = [0, 1, 3, 4, 6, 9, 10, 13, 15, 17, 18, 19]
    shape = dict(length=20, weight=len(pos), mask=sum(1 << k for k in pos), positions=pos)
    rng = np.random.default_rng(14)
    qs, _ = edge_block(rng)
    ts = [mutated(rng, q, 0.04) for q in qs]
    hits = compare(ctx, fast(shapes=[shape]), qs, ts)
    assert len(set(hits["query"].tolist())) > len(qs) // 2


def test_query_ids_follow_a_second_upload(ctx):
    """a different query block uploaded into the same context: its own limits, so its own position -> query id map"""
    rng = np.random.default_rng(15)
    first = [protein(rng, n) for n in (70, 200, 31, 90)]
    second = [protein(rng, n) for n in (25, 26, 150, 40, 40, 88, 300)]
    ts = [mutated(rng, q, 0.05) for q in first + second]
    a = compare(ctx, fast(), first, ts)
    b = compare(ctx, fast(), second, ts)
    assert set(a["query"].tolist()) == set(range(4)) and set(b["query"].tolist()) == set(range(7))
    # ... and a block of the same length with other limits
    third = [np.concatenate([second[0], second[1]])] + second[2:]
    c = compare(ctx, fast(), third, ts)
    assert set(c["query"].tolist()) <= set(range(6)) and len(c) > 0


# ---- left-most rule -----------------------------------------------------------------------------------------------------

def left_most_block(rng):
    """pairs whose first common seed lies at query offset 0, 1 and 31, short pairs whose windows are clipped by the delimiters on
    either side, long ones, and one with a masked and a stop letter beside the seeds"""
    qs, ts = [], []
    q = protein(rng, 120); qs.append(q); ts.append(q.copy())                                  # 0: offset 0 kept, 1 ... dropped
    q = protein(rng, 110); q[0] = X; qs.append(q); ts.append(q.copy())                        # 1: offset 1 kept
    q = protein(rng, 100); t = q.copy(); t[:31] = other_class(rng, q[:31]); qs.append(q); ts.append(t)      # 2: offset 31 kept
    for n in (16, 17, 20, 33, 40, 48, 49):                                                    # 3-9: clipped on both sides
        q = protein(rng, n); qs.append(q); ts.append(q.copy())
    q = protein(rng, 85); qs.append(q); ts.append(np.concatenate([protein(rng, 7), q[10:60], protein(rng, 9)]))      # 10: the subject clipped, another diagonal
    q = protein(rng, 400); qs.append(q); ts.append(mutated(rng, q, 0.1))                      # 11
    q = protein(rng, 90); q[30] = X; q[52] = STOP; qs.append(q); ts.append(q.copy())          # 12
    return qs, ts


@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("name,kw", [("fast", {}), ("default", {}), ("default, ungapped window 64: clips of 128 letters", dict(window=64)),
                                     ("fast, translated frames", dict(translated=1))], ids=lambda x: x if isinstance(x, str) else "")
def test_left_most_rule_keeps_and_drops(ctx, name, kw, chunks):
    rng = np.random.default_rng(16)
    qs, ts = left_most_block(rng)
    cfg = (fast if name.startswith("fast") else default)(index_chunks=chunks)
    hits = compare(ctx, cfg, qs, ts, **kw)
    first = {q: offsets_of(hits, q)[:1] for q in range(len(qs))}
    # every window of these pairs is a seed hit: some are kept, most are dropped
    for q in (0, 1, 2, 11):
        assert 0 < len(offsets_of(hits, q)) < (len(qs[q]) - 15) // 2
    if chunks == 1:                                          # (with index chunks the first seed in chunk order is kept, not the first by offset)
        assert first[0] == [0] and first[1] == [1]
        assert 1 not in offsets_of(hits, 0) and 2 not in offsets_of(hits, 1)      # seeds to the right of a kept one, same interval
        if name.startswith("fast"):
            assert first[2] == [31] and 32 in offsets_of(hits, 2)                # the interval's next one starts at 32
            assert all(first[q] == [0] for q in range(3, 10))


def single_window_pairs(rng, n, pool={}):
    """n pairs of 16-letter sequences with one seed hit each (the --fast shape): the sequences are drawn once, the oracle says which
    of them give a hit (a low-complexity seed gives none), and the first n of those are used -- hit count = n"""
    if "good" not in pool:
        seqs = [protein(rng, 16) for _ in range(2300)]
        qd, ql = blocks(seqs)
        want = orc.seed_search(both_params(fast())[1], qd, ql, qd, ql)
        diagonal = want[want["subject"] == ql[want["query"]]]
        assert len(diagonal) == len(want)                    # no chance hits between different sequences
        pool["good"] = [seqs[i] for i in sorted(set(diagonal["query"].tolist()))]
        assert len(pool["good"]) > 2100
    return pool["good"][:n]


def two_window_pairs(rng, n, pool={}):
    """n pairs of 17-letter sequences with two seed hits each on the main diagonal, of which the left-most rule keeps one and
    drops the other: sequences whose two windows each give a hit as a 16-letter sequence of their own (no low-complexity seed)"""
    if "good" not in pool:
        seqs = [protein(rng, 17) for _ in range(120)]
        qd, ql = blocks([s[:16] for s in seqs] + [s[1:] for s in seqs])
        want = orc.seed_search(both_params(fast())[1], qd, ql, qd, ql)
        alone = set(want["query"][want["subject"] == ql[want["query"]]].tolist())
        pool["good"] = [s for i, s in enumerate(seqs) if i in alone and i + len(seqs) in alone]
        assert len(pool["good"]) >= 32
    return pool["good"][:n]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_left_most_rule_list_sizes(ctx, n, monkeypatch, capfd):
    """n pairs reach the left-most rule, around the wavefront's 64: n // 2 of them are kept and n // 2 dropped (the two windows of
    identical 17-letter sequences, in neighbouring list entries), an odd one is kept"""
    rng = np.random.default_rng(17)
    seqs = two_window_pairs(rng, n // 2) + single_window_pairs(rng, n % 2) + [np.full(20, X, np.int8)]      # (a block needs a sequence: one that has no seed)
    (qd, ql) = blocks(seqs)
    ctx.upload_block(hip.QUERY, qd, ql)
    ctx.upload_block(hip.TARGET, qd, ql)
    p, o = both_params(fast())
    hits, path, joined = search(ctx, p, monkeypatch, capfd, CHAIN=1)
    assert path.startswith("chain") and sum(joined) == n
    assert len(hits) == n // 2 + n % 2                       # (which of a pair's two windows is kept follows the index chunks' order)
    assert hit_multiset(hits) == hit_multiset(orc.seed_search(o, qd, ql, qd, ql))


# ---- the padded sort ----------------------------------------------------------------------------------------------------

def test_sort_pad_follows_the_last_hit_count(monkeypatch, capfd):
    """The padded sort is sized by the context's last hit count plus a quarter, rounded up to a power of two: a first call (the
    ceiling), hit counts one below, at and one above the pad, no hits at all, and the call after an overflow."""
    rng = np.random.default_rng(17)
    p, o = both_params(fast())
    c = hip.Context()
    try:
        def run(n):
            seqs = single_window_pairs(rng, n) + [np.full(20, X, np.int8)]
            qd, ql = blocks(seqs)
            c.upload_block(hip.QUERY, qd, ql)
            c.upload_block(hip.TARGET, qd, ql)
            hits, path, _ = search(c, p, monkeypatch, capfd)
            assert len(hits) == n and hit_multiset(hits) == hit_multiset(orc.seed_search(o, qd, ql, qd, ql))
            assert (np.diff(hits["query"].astype(np.int64)) >= 0).all()
            return path
        over = "chain, then host from the hit sort"
        assert run(1500) == "chain"                          # a fresh context: the ceiling
        assert run(2047) == "chain"                          # 1500 + 375 -> a pad of 2048
        assert run(1500) == "chain"
        assert run(2048) == "chain"
        assert run(1500) == "chain"
        assert run(2049) == over                             # the host's launches sort, and the next pad is sized for them
        assert run(2049) == "chain"
        assert run(0) == "chain"
        assert run(1024) == "chain"                          # the smallest pad
        assert run(0) == "chain"
        assert run(1025) == over
        assert run(1500) == "chain"                          # an overflow below the ceiling does not make the chain rest
        monkeypatch.setenv("DMND_SEED_SORT_CAP", "1024")     # the ceiling stays the ceiling
        hits = c.seed_search(p)
        monkeypatch.delenv("DMND_SEED_SORT_CAP")
        assert len(hits) == 1500
    finally:
        c.close()
