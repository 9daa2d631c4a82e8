"""-m gpu: the device planner on translated queries (six contexts per read; csrc/plan_kernels.hip: the hits re-sorted by (read, target),
units and pairs) read out through dmnd_extend_plan_device and compared exactly, pair by pair and context by context, with the host
planner (hip.extend_plan with six contexts: rows in (read, target, frame) order, `query` = the context, the ungapped score of
context 0): on tests/golden/ext_blastx.tap and on the constructed read set of tests/translated_sets.py, as a whole and as prefixes
cut at read boundaries so that the pair counts sit on the kernels' 64- and 256-wide workgroup boundaries, in both forms of the
chaining (DMND_PLAN_SMALL_HITS=0), under DMND_EXTEND_GUARD. Compared too: the pairs' hit counts, the gapped filter's pass flag per
pair (the OR over all its hits, whatever their frame; the constructed set is searched with the filter on), the counters, and the set
of pairs left to the host -- predicted per (context, target) unit on the CPU by tests/test_gpu_plan_device.py's _predict (more than
32 hits, more than 16 segments, a chaining workspace outgrown), a pair being left where one of its units is; empty for the golden.
A list with two hits swapped comes back as not planned."""
import os

import numpy as np
import pytest
import torch

import translated_sets as ts
from tapfile import read_ext_tap
from diamond_amd import hip, workload
from test_gpu_seed import to_hip_params
from test_gpu_plan_device import _matrix, _predict

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _expect(p, M, qd, ql, td, tl, hits, flags):
    """per (read, target) pair in (read, target) order: (read, target, n_hits, pass, on_host, host rows)"""
    cbs, plan = hip.extend_plan(p, qd, ql, td, tl, hits, threads=4, query_contexts=6)
    rows = {}
    for r in plan:
        rows.setdefault((int(r["query"]) // 6, int(r["target"])), []).append(r)
    for key, v in rows.items():                           # the host's own order inside a pair: frame by frame
        assert [int(r["query"]) for r in v] == sorted(int(r["query"]) for r in v), key
    units = {(g["query"], g["target"]): g for g in _predict(qd, ql, td, tl, hits, cbs, M)}
    out = []
    for (read, target), v in sorted(ts.pairs_of(hits, tl).items()):
        idx = [k for _, k in v]
        passed = bool(flags[idx].any()) if flags is not None else True
        on_host = len(v) > 1 and any(units[(read * 6 + f, target)]["on_host"] for f in {f for f, _ in v})
        out.append((read, target, len(v), passed, on_host, rows.get((read, target), [])))
    return out


def _compare(ctx, hits, want):
    rows, groups, info = ctx.extend_plan_device(hits)
    assert info["planned"] and not info["unsorted"]
    assert info["n_groups"] == len(groups) == len(want)
    assert info["n_queries"] == len({w[0] for w in want})
    assert [(int(g["query"]), int(g["target"]), int(g["n_hits"])) for g in groups] == [(w[0] * 6, w[1], w[2]) for w in want]
    assert groups["pass"].astype(bool).tolist() == [w[3] for w in want]
    assert [bool(g["on_host"]) for g in groups] == [w[3] and w[4] for w in want]
    assert info["n_on_host"] == sum(w[3] and w[4] for w in want)
    pos = 0
    for g, w in zip(groups, want):
        n = int(g["n_bands"])
        got = rows[pos:pos + n]
        pos += n
        if not w[3] or w[4]:
            assert n == 0
            continue
        exp = np.array([tuple(r) for r in w[5]], dtype=hip.PLAN_DTYPE) if w[5] else np.zeros(0, hip.PLAN_DTYPE)
        assert got.tobytes() == exp.tobytes(), (w[0], w[1], got, exp)
    assert pos == len(rows) == info["n_bands"]
    return groups, info


def _context(p, qd, ql, td, tl, gf):
    ctx = hip.Context(params=p)
    ctx.upload_block(hip.QUERY, qd, ql)
    ctx.upload_block(hip.TARGET, td, tl)
    ctx.set_db_letters(p.db_letters)
    ctx.set_gapped_filter(gf)
    ctx.set_query_contexts(6)
    return ctx


@pytest.mark.parametrize("small_form", [False, True], ids=["one-kernel", "small-first"])
def test_device_plan_of_the_blastx_golden_equals_the_host_plan(small_form, monkeypatch):
    assert torch.cuda.is_available()
    monkeypatch.setenv("DMND_EXTEND_GUARD", "1")
    if small_form:
        monkeypatch.setenv("DMND_PLAN_SMALL_HITS", "0")
    cfg, _ = read_ext_tap(os.path.join(GOLDEN, "ext_blastx.tap"))
    assert cfg["query_contexts"] == 6 and cfg["gapped_filter_evalue"] == 0
    qd, ql, td, tl = cfg["query"]["data"], cfg["query"]["limits"], cfg["target"]["data"], cfg["target"]["limits"]
    p, M = _matrix()
    p.db_letters = float(tl[-1] - tl[0] - (len(tl) - 1))
    ctx = _context(p, qd, ql, td, tl, 0.0)
    try:
        hits = ctx.seed_search(to_hip_params(cfg))
        want = _expect(p, M, qd, ql, td, tl, hits, None)
        assert len(want) == 365 and not any(w[4] for w in want)
        groups, info = _compare(ctx, hits, want)
        assert info["n_on_host"] == 0 and int(groups["n_bands"].sum()) > 300
        # two hits swapped: not planned
        bad = hits.copy()
        k = next(i for i in range(len(bad) - 1) if bad["query"][i] == bad["query"][i + 1])
        bad[[k, k + 1]] = bad[[k + 1, k]]
        rows, groups, info = ctx.extend_plan_device(bad)
        assert not info["planned"] and info["unsorted"] and len(rows) == 0 and len(groups) == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("small_form", [False, True], ids=["one-kernel", "small-first"])
def test_device_plan_of_the_constructed_reads_equals_the_host_plan(small_form, monkeypatch):
    monkeypatch.setenv("DMND_EXTEND_GUARD", "1")
    if small_form:
        monkeypatch.setenv("DMND_PLAN_SMALL_HITS", "0")
    db, doff, dna, off, kinds = ts.constructed_set()
    xd, xl = hip.translated_block(dna, off)
    td, tl = workload.sequence_set(db, doff)
    p, M = _matrix()
    p.db_letters = float(doff[-1])
    sp, gf = hip.seed_params_preset("sensitive", p, threads=4)
    sp.query_translated = 1
    assert gf > 0
    ctx = _context(p, xd, xl, td, tl, gf)
    try:
        hits = ctx.seed_search(sp)
        ts.assert_cases_present(hits, tl, kinds)
        ctx.extend_plan_device(hits)                       # (leaves the bias in HBM for the filter)
        flags = ctx.gapped_filter(hits, use_cbs=True)
        want = _expect(p, M, xd, xl, td, tl, hits, flags)
        assert 0 < sum(w[3] for w in want) < len(want), "the filter passes every pair or none"
        _compare(ctx, hits, want)
        # prefixes cut at read boundaries: pair counts on and around the 64- and 256-wide workgroup boundaries
        reads = hits["query"] // 6
        ends = np.flatnonzero(np.append(reads[1:] != reads[:-1], True)) + 1
        n_pairs = np.searchsorted(np.array([w[0] for w in want]), reads[ends - 1], "right")
        cuts = set()
        for bound in (64, 256, 1024):
            below, above = np.flatnonzero(n_pairs <= bound), np.flatnonzero(n_pairs > bound)
            if len(below):
                cuts.add(int(ends[below[-1]]))
            if len(above):
                cuts.add(int(ends[above[0]]))
        assert len(cuts) >= 4
        for e in sorted(cuts):
            last = int(reads[e - 1])
            _compare(ctx, hits[:e], [w for w in want if w[0] <= last])
    finally:
        ctx.close()
