"""-m gpu: --comp-based-stats 2 - 5 searches through the device half of the extension stage (diamond_amd/csrc/extend_device.hip,
extend_kernels.hip, extend_cbs_core.h): per ranking iteration the new (query, target) pairs are listed in HBM, cbs_adjust_kernel fills
their slots of the matrix store, the host form patches the pairs the kernel hands back, and the items carry their matrix codes into
the 32-bit sweeps and the trace walk. Every comparison is the default call against DMND_EXTEND_DEVICE=0 (the host path's ranking loop
with the same kernel) in one process: all record fields and the transcript bytes."""
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from diamond_amd import hip, synth, workload  # noqa: E402
from test_gpu_cbs_device import Env, _block, _fields, _stats_ok  # noqa: E402

pytestmark = pytest.mark.gpu
HOST = dict(DMND_EXTEND_DEVICE=0)
SEED = 5          # the block of tests/test_gpu_cbs_device.py: at most one of its 40 queries goes back to the host path in every mode


def _extend(blk, mode, k, env, top=None, filters=None, transcripts=True, ext=None):
    qd, ql, td, tl, params, gf, hits = blk
    with Env(**env):          # (the trace budget is read when the context is made, the other switches per call)
        ctx = hip.Context(params=params)
        try:
            ctx.upload_block(hip.QUERY, qd, ql)
            ctx.upload_block(hip.TARGET, td, tl)
            ctx.set_gapped_filter(gf)
            ctx.set_comp_based_stats(mode)
            ctx.set_max_target_seqs(k)
            if top is not None:
                ctx.set_top_percent(top)
            if filters:
                ctx.set_filters(**filters)
            if ext is not None:
                ctx.set_extension_mode(ext)
            m, tr = ctx.extend(qd, td, hits, threads=4, with_transcripts=transcripts)
            return m, tr, ctx.cbs_device_stats(), ctx.extend_device_stats()
        finally:
            ctx.close()


def _same(got, want, what, at_least=51):
    m, tr, m0, tr0 = got[0], got[1], want[0], want[1]
    assert len(m) == len(m0) and len(m) >= at_least, (what, len(m), len(m0))
    with_tr = tr is not None
    for name, g, w in _fields(m, m0, m.dtype):
        if not with_tr and name == "hsp.transcript_off":
            assert (g == -1).all() and (w == -1).all(), what
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: field %s of %d records differs from the host path's; first: record %d (query %d, target %d): %s, host path %s" % (
            what, name, len(bad), bad[0], m["query"][bad[0]], m["target"][bad[0]], g[bad[0]], w[bad[0]])
    if with_tr:
        end = int((m["hsp"]["transcript_off"] + m["hsp"]["transcript_len"] + 1).max())
        assert end > 0 and np.array_equal(tr[:end], tr0[:end]), what


def _on_device(got, what):
    """the device half took the call and kept its queries: the project's cap on what goes back"""
    st = got[3]
    print("%s: %s %s" % (what, st, got[2]))
    assert st["queries"] > 0, (what, st)
    assert st["queries_back_to_host"] <= max(1, st["queries"] // 50), (what, st)


_host = {}


def _host_path(key, blk, mode, k, **kw):
    """the DMND_EXTEND_DEVICE=0 answer of a configuration, computed once"""
    if key not in _host:
        _host[key] = _extend(blk, mode, k, HOST, **kw)
        assert _host[key][3]["queries"] == 0
    return _host[key]


@pytest.mark.parametrize("mode", [2, 3, 4, 5])
def test_modes_through_the_device_half(mode):
    blk = _block(40, 10, SEED)
    what = "mode %d" % mode
    host = _host_path(("k25", mode), blk, mode, 25)
    dev = _extend(blk, mode, 25, {})
    _same(dev, host, what)
    _on_device(dev, what)
    _stats_ok(dev[2], mode, what)
    # both halves offered the kernel the same pairs, whichever half ended up with a query
    assert dev[2]["pairs"] == host[2]["pairs"], (dev[2], host[2])
    if mode == 4:          # every pair is adjusted
        assert dev[2]["rule"] == 0
    else:                  # the conditional test takes both branches: own-matrix items beside standard ones
        assert host[2]["pairs"] > 0


@pytest.mark.parametrize("mode", [3, 4, 5])
def test_several_ranking_chunks_append_to_the_store(mode):
    """-k 1 over 300 targets per query: later chunks append their pairs to the store and find the earlier chunks' matrix numbers.
    With an iteration cap of 1 every relative-entropy pair is patched by the host form, and the queries stay on the device."""
    blk = _block(4, 300, 6)
    what = "mode %d, -k 1" % mode
    host = _host_path(("k1", mode), blk, mode, 1)
    dev = _extend(blk, mode, 1, {})
    _same(dev, host, what, at_least=3)
    print("%s: %s %s" % (what, dev[3], dev[2]))
    assert dev[3]["queries"] > 0 and dev[2]["pairs"] > 4 * 128, (dev[3], dev[2])
    assert dev[2]["pairs"] == host[2]["pairs"]
    # one survivor of 128 swept targets per query: round 1 sweeps for scores only (extend_device.hip few_survive), so round 2 sweeps
    # copies of the survivors' items -- with their matrix codes -- and the walk reads those matrices
    assert dev[3]["round2_cells_swept_again"] > 0, dev[3]
    back = _extend(blk, mode, 1, dict(DMND_CBS_DEVICE_MAX_ITS=1))
    _same(back, host, what + ", iteration cap 1", at_least=3)
    assert back[2]["pairs"] == dev[2]["pairs"] and back[3]["queries"] > 0 and back[2]["iterations"] > 0, (back[2], back[3])


@pytest.mark.parametrize("env", [dict(DMND_EXTEND_KEEP_TRACE=0), dict(DMND_TRACE_ARENA_MB=8)], ids=["no_kept_rows", "arena_8mb"])
@pytest.mark.parametrize("mode", [3, 4])
def test_round_2_sweeps_again_with_the_matrix_codes(mode, env):
    blk = _block(40, 10, SEED)
    what = "mode %d, %s" % (mode, env)
    host = _host_path(("k25", mode), blk, mode, 25)
    dev = _extend(blk, mode, 25, env)
    _same(dev, host, what)
    _on_device(dev, what)
    if "DMND_EXTEND_KEEP_TRACE" in env:          # every survivor is swept again as a copy of its item, matrix code included
        assert dev[3]["round2_cells_swept_again"] == dev[3]["round2_cells"] > 0, dev[3]


def test_row_classes_forced_on():
    blk = _block(40, 10, SEED)
    host = _host_path(("k25", 3), blk, 3, 25)
    dev = _extend(blk, 3, 25, dict(DMND_SWEEP_ROWS=1))          # (a row class outside the 16-bit kernels fails the call)
    _same(dev, host, "mode 3, row classes")
    _on_device(dev, "mode 3, row classes")


@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("cfg", ["top10", "filters"])
def test_top_and_filters(mode, cfg):
    blk = _block(40, 10, SEED)
    kw = dict(top=10.0) if cfg == "top10" else dict(filters=dict(min_id=30, query_cover=30))
    what = "mode %d, %s" % (mode, cfg)
    host = _host_path((cfg, mode), blk, mode, 25, **kw)
    dev = _extend(blk, mode, 25, {}, **kw)
    _same(dev, host, what, at_least=20)
    print("%s: %s" % (what, dev[3]))
    assert dev[3]["queries"] > dev[3]["queries_back_to_host"], dev[3]


def test_without_a_transcript_arena():
    blk = _block(40, 10, SEED)
    host = _extend(blk, 4, 25, HOST, transcripts=False)
    dev = _extend(blk, 4, 25, {}, transcripts=False)
    _same(dev, host, "mode 4, no transcripts")
    _on_device(dev, "mode 4, no transcripts")


def _one_pair():
    rng = np.random.default_rng(17)
    q = rng.integers(0, 20, 150).astype(np.int8)
    t = q.copy()
    mut = rng.random(len(t)) < 0.2
    t[mut] = rng.integers(0, 20, int(mut.sum()))
    qd, ql = workload.sequence_set(q, np.array([0, len(q)]))
    td, tl = workload.sequence_set(t, np.array([0, len(t)]))
    params = hip.default_params()
    params.db_letters = float(len(t))
    ctx = hip.Context(params=params)
    try:
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, td, tl)
        sp, gf = hip.seed_params_preset("default", params, threads=1)
        ctx.set_gapped_filter(gf)
        hits = ctx.seed_search(sp)
    finally:
        ctx.close()
    assert len(hits) >= 1
    return qd, ql, td, tl, params, gf, hits


@pytest.mark.parametrize("mode", [4, 2])
def test_one_query_one_target(mode):
    blk = _one_pair()
    host = _extend(blk, mode, 25, HOST)
    dev = _extend(blk, mode, 25, {})
    _same(dev, host, "one pair, mode %d" % mode, at_least=1)
    assert len(dev[0]) == 1 and dev[3]["queries"] == 1 and dev[3]["queries_back_to_host"] == 0, dev[3]
    assert dev[2]["pairs"] == 1 and dev[2]["kernel_ms"] > 0, dev[2]


def test_gates():
    blk = _block(40, 10, SEED)
    host = _host_path(("k25", 4), blk, 4, 25)
    # the host arithmetic on the host path
    off = _extend(blk, 4, 25, dict(DMND_CBS_DEVICE=0))
    assert off[3]["queries"] == 0 and off[2]["pairs"] == 0
    _same(off, host, "DMND_CBS_DEVICE=0")
    # the store bound: more groups than slots of one pass -> the host path and its passes
    bound = _extend(blk, 4, 25, dict(DMND_CBS_PASS_HITS=1))
    assert bound[3]["queries"] == 0
    _same(bound, host, "DMND_CBS_PASS_HITS=1")
    # the full-matrix sweep cannot trace back on an adjusted matrix: the reference's refusal
    for env in ({}, HOST):
        with pytest.raises(hip.DiamondHipError, match="Traceback with adjusted matrix not supported"):
            _extend(blk, 4, 25, env, ext=hip.EXT_FULL)


def _write_files(d):
    """ordinary families and a few whose composition lies far from the matrix background"""
    rng = np.random.default_rng(44)
    db, doff, q, qoff = synth.generate(30, members=4, queries=30, seed=45)
    ts = [db[doff[i]:doff[i + 1]] for i in range(len(doff) - 1)]
    qs = [q[qoff[i]:qoff[i + 1]] for i in range(len(qoff) - 1)]
    pools = [np.array([0, 10, 19, 9, 12, 13], np.int8), np.array([3, 6, 11, 1, 15, 5], np.int8), np.array([7, 14, 15, 16, 2], np.int8)]
    for k in range(9):
        pool = pools[k % 3]
        n = int(rng.integers(80, 250))
        anc = np.where(rng.random(n) < 0.7, rng.choice(pool, n), rng.integers(0, 20, n)).astype(np.int8)
        for j in range(5):
            m = anc.copy()
            mut = rng.random(n) < rng.uniform(0.1, 0.35)
            m[mut] = rng.integers(0, 20, int(mut.sum()))
            (qs if j == 0 else ts).append(m)

    def write(path, prefix, seqs):
        off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
        synth.write_fasta(path, prefix, np.concatenate(seqs), off)
    write(str(d / "db.faa"), "t", ts)
    write(str(d / "q.faa"), "q", qs)


def test_cli_outputs_are_byte_identical(tmp_path):
    from test_gpu_cli import CLI, _run
    assert os.path.exists(CLI), "diamond-hip not built (make product)"
    _write_files(tmp_path)
    base = [CLI, "blastp", "-q", str(tmp_path / "q.faa"), "-d", str(tmp_path / "db.faa"), "-p", "4"]
    for extra in (["3", "-f", "6"], ["4", "-f", "0"]):
        _run(base + ["--comp-based-stats"] + extra + ["-o", str(tmp_path / "dev.out")])
        with Env(**HOST):
            _run(base + ["--comp-based-stats"] + extra + ["-o", str(tmp_path / "host.out")])
        dev, host = open(tmp_path / "dev.out").read(), open(tmp_path / "host.out").read()
        assert len(host) > 2000 and dev == host, extra
