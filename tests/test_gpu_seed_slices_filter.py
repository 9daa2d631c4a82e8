"""-m gpu tests of the level-1 filter that a search on the sliced long-seed stream builds (csrc/seed_slices_core.h
seed_slices_filter_words, seed_api.hip seed_sizes_sliced / SeedRun::ref_decide): sized for LDS slices -- up to 64 slices of 128 KB --
where the plain stream's is sized for L2. Level 1 is a pre-filter without false negatives, so whatever its size the sorted hits are
those of a fresh context on the plain stream; the geometry is read from the DMND_TRACE line `stream: slices (N x K KB)`."""
import re

import numpy as np
import pytest
import torch

from diamond_amd import hip, workload
from test_gpu_seed_slices import search, plain_hits, upload

pytestmark = pytest.mark.gpu


class Keep:
    """capfd for `search`, keeping what the search wrote: the geometry of the trace line"""

    def __init__(self, capfd):
        self.capfd, self.last = capfd, None

    def readouterr(self):
        self.last = self.capfd.readouterr()
        return self.last

    def geometry(self):
        m = re.search(r"stream: slices \((\d+) x ([0-9.]+) KB\)", self.last.err)
        return (int(m.group(1)), float(m.group(2))) if m else None


def blocks_of(rng, n_queries, length, copies, random_letters):
    """n_queries random queries; the reference: `copies` (a list of query ranges, each one sequence per query) and random sequences
    of the queries' length"""
    q = rng.integers(0, 20, n_queries * length).astype(np.int8)
    qoff = np.arange(n_queries + 1, dtype=np.int64) * length
    parts = [q[a * length:b * length] for a, b in copies]
    parts.append(rng.integers(0, 20, random_letters // length * length).astype(np.int8))
    t = np.concatenate(parts)
    toff = np.arange(len(t) // length + 1, dtype=np.int64) * length
    qd, ql = workload.sequence_set(q, qoff)
    td, tl = workload.sequence_set(t, toff)
    return qd, ql, td, tl


SMALL = {
    # the reference is the queries twelve times: every window joins -- whole queues of positives, the staging area full
    "copies": dict(copies=[(0, 150)] * 12, random_letters=0, min_hits=150 * 12),
    "unrelated": dict(copies=[], random_letters=200_000, min_hits=0),
    "mix": dict(copies=[(0, 150)] * 3 + [(20, 90)] * 4, random_letters=100_000, min_hits=150 * 3),
}


@pytest.mark.parametrize("case", list(SMALL))
def test_forced_filter_sizes_on_a_small_block(case, monkeypatch, capfd):
    """DMND_SEED_SLICES_FILTER_WORDS on 150 queries x 100 letters: 65 536 words are 2 slices of 32 768 -- the whole LDS array --,
    2 097 152 are 64 slices of 32 768, both maxima at once. Host-driven and as a chain, built and kept."""
    assert torch.cuda.is_available()
    spec = SMALL[case]
    blocks = blocks_of(np.random.default_rng(17), 150, 100, spec["copies"], spec["random_letters"])
    assert blocks[3][-1] - blocks[3][0] <= 200_000 + 2000
    sp = hip.seed_params_fast(threads=1)
    keep = Keep(capfd)
    for chain in (0, 1):
        plain = plain_hits(blocks, sp, monkeypatch, capfd, CHAIN=chain)
        assert len(plain) >= spec["min_hits"] and (spec["min_hits"] or len(plain) == 0)
        for words, geometry in ((65_536, (2, 128.0)), (2_097_152, (64, 128.0))):
            c = hip.Context()
            try:
                upload(c, blocks)
                for want in ("built", "kept"):
                    got, path, stream, cache, _ = search(c, sp, monkeypatch, keep, CHAIN=chain, SLICES=1, SLICES_FILTER_WORDS=words)
                    assert (stream, cache) == ("slices", want) and keep.geometry() == geometry
                    assert path.startswith("chain") if chain else path == "host"
                    assert np.array_equal(got, plain)
            finally:
                c.close()


_large = {}


def large_blocks():
    """About 7400 random queries of 300 letters -- more than 2^21 positions: the level-2 filter has 2^21 words --, a reference of
    <= 3e5 letters that holds 300 of them. The plain stream's hits, once."""
    if not _large:
        _large["blocks"] = blocks_of(np.random.default_rng(23), 7400, 300, [(1000, 1200), (7300, 7400)], 200_000)
        _large["sp"] = hip.seed_params_fast(threads=1)
    return _large["blocks"], _large["sp"]


def large_plain(monkeypatch, capfd):
    blocks, sp = large_blocks()
    if "plain" not in _large:
        _large["plain"] = plain_hits(blocks, sp, monkeypatch, capfd)
        assert len(_large["plain"]) >= 300
    return _large["plain"]


def test_rule_gives_a_large_query_block_64_slices_of_128_kb(monkeypatch, capfd):
    assert torch.cuda.is_available()
    blocks, sp = large_blocks()
    qd, ql, td, tl = blocks
    assert ql[-1] - ql[0] > 1 << 21 and tl[-1] - tl[0] <= 300_000
    plain = large_plain(monkeypatch, capfd)
    keep = Keep(capfd)
    c = hip.Context()
    try:
        upload(c, blocks)
        got, _, stream, cache, _ = search(c, sp, monkeypatch, keep, SLICES=1)
        assert (stream, cache) == ("slices", "built")
        assert "stream: slices (64 x 128 KB)" in keep.last.err
        assert np.array_equal(got, plain)
    finally:
        c.close()


def test_one_context_through_its_states(monkeypatch, capfd):
    """Plain first search with the plain stream's filter, built and kept with the large one, plain again after the reference block
    is uploaded again, built again; a kept query index keeps the plain stream's geometry on the sliced stream."""
    assert torch.cuda.is_available()
    blocks, sp = large_blocks()
    qd, ql, td, tl = blocks
    plain = large_plain(monkeypatch, capfd)
    keep = Keep(capfd)
    c = hip.Context()
    try:
        upload(c, blocks)
        seen = []

        def step(**env):
            got, _, stream, cache, _ = search(c, sp, monkeypatch, keep, **env)
            assert np.array_equal(got, plain), seen
            seen.append((stream, cache, keep.geometry()))

        for _ in range(3):
            step(SLICES_MIN_LETTERS=1)
        c.upload_block(hip.TARGET, td, tl)
        for _ in range(2):
            step(SLICES_MIN_LETTERS=1)
        large = (64, 128.0)
        assert seen == [("plain", "none", None), ("slices", "built", large), ("slices", "kept", large), ("plain", "none", None), ("slices", "built", large)]
        c.set_query_index_reuse(True)
        step(SLICES=1)
        step(SLICES=1)
        assert seen[-2:] == [("slices", "built", (32, 96.0)), ("slices", "kept", (32, 96.0))]
    finally:
        c.close()


def test_failed_cache_allocation_falls_back_to_the_plain_stream(monkeypatch, capfd):
    """DMND_SEED_SLICES_ALLOC_FAIL=1: a search that decided to build finds no memory for the cache and takes the plain stream with
    the plain stream's geometry -- after the larger filter of the rule and after a forced smaller one were cleared for it, and with
    a kept query index, whose filters must stay as they are. The hits are the plain stream's every time, and a later search builds."""
    assert torch.cuda.is_available()
    blocks, sp = large_blocks()
    plain = large_plain(monkeypatch, capfd)
    keep = Keep(capfd)
    c = hip.Context()
    try:
        upload(c, blocks)
        for env in (dict(), dict(SLICES_FILTER_WORDS=65_536), dict()):
            got, _, stream, cache, held = search(c, sp, monkeypatch, keep, SLICES=1, SLICES_ALLOC_FAIL=1, **env)
            assert (stream, cache, held) == ("plain", "none", 0) and np.array_equal(got, plain), env
        got, _, stream, cache, _ = search(c, sp, monkeypatch, keep, SLICES=1)
        assert (stream, cache, keep.geometry()) == ("slices", "built", (64, 128.0)) and np.array_equal(got, plain)
    finally:
        c.close()
    c = hip.Context()
    try:
        c.set_query_index_reuse(True)
        upload(c, blocks)
        seen = []
        for env in (dict(SLICES=0), dict(SLICES=1, SLICES_ALLOC_FAIL=1), dict(SLICES=0), dict(SLICES=1), dict(SLICES=1)):
            got, _, stream, cache, _ = search(c, sp, monkeypatch, keep, **env)
            seen.append((stream, cache, keep.geometry()))
            assert np.array_equal(got, plain), seen       # (from the second search on the query index is the kept one)
        assert seen == [("plain", "none", None)] * 3 + [("slices", "built", (32, 96.0)), ("slices", "kept", (32, 96.0))]
    finally:
        c.close()
