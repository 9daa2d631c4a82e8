"""-m gpu: translated queries (blastx, six contexts per read) in the device half of the extension stage (csrc/plan_kernels.hip:
the hits re-sorted per (read, target) pair; csrc/extend_kernels.hip: ranking, best HSP and records per read).
 1. tests/golden/ext_blastx.tap (120 reads = 720 contexts, 1 500 targets; 365 (read, target) pairs, 210 of them with one seed hit, at
    most 10 hits per pair -- counted below on the CPU, so no pair can reach the planner's 32-hit / 16-segment limits) is planned and
    extended in HBM and equals the Match lists of the reference, frame included.
 2. The same block, device half against host path (DMND_EXTEND_DEVICE=0) in one process: every field of every record, the arena
    bytes of every transcript, for -k 25, -k 1 and --top 10.
 3. The constructed read set of tests/translated_sets.py (pairs with hits in two frames, equal scores in two contexts, single-hit
    pairs, reads ranked in several chunks, a band width taken from context 0 -- cases a, c and d asserted from the seed hits, b and e
    hold by construction, see there) under DMND_EXTEND_GUARD: records equal to the host path's, and the CLI's output byte-identical
    to the reference binary's for default -k, -k 1, --top 10, --sensitive and a BTOP column.
 4. A translated call with --id stays on the host path as a whole.
 5. Reads that come back from a device-planned call -- the whole call declined (-k 2000), reads at the chunk cap, with and without the
    gapped filter -- on a fresh context: records and transcripts equal the host path's."""
import os
import subprocess

import numpy as np
import pytest
import torch

import translated_sets as ts
from tapfile import read_ext_tap
from diamond_amd import hip, synth, workload
from test_gpu_seed import to_hip_params
from test_gpu_extend_device import HSP_KEYS, _check, _search

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
REF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "diamond")
CLI = os.path.join(os.path.dirname(HERE), "diamond_amd", "diamond-hip")
_cache = {}


def _golden():
    if "golden" not in _cache:
        _cache["golden"] = read_ext_tap(os.path.join(GOLDEN, "ext_blastx.tap"))
    return _cache["golden"]


def _upload(ctx, cfg):
    qd, ql, td, tl = cfg["query"]["data"], cfg["query"]["limits"], cfg["target"]["data"], cfg["target"]["limits"]
    ctx.upload_block(hip.QUERY, qd, ql)
    ctx.upload_block(hip.TARGET, td, tl)
    ctx.set_db_letters(float(tl[-1] - tl[0] - (len(tl) - 1)))
    ctx.set_gapped_filter(cfg["gapped_filter_evalue"])
    ctx.set_query_contexts(cfg["query_contexts"])
    return ctx.seed_search(to_hip_params(cfg))


def _same_records(a, b, tra=None, trb=None):
    """every field of every dmnd_match; with arenas the bytes of each record's transcript"""
    assert len(a) == len(b)
    for name in a.dtype.names:
        if name == "hsp":
            for k in a["hsp"].dtype.names:
                if k != "transcript_off":
                    assert np.array_equal(a["hsp"][k], b["hsp"][k]), k
        else:
            assert np.array_equal(a[name], b[name]), name
    if tra is None:
        assert (a["hsp"]["transcript_off"] == -1).all() and (b["hsp"]["transcript_off"] == -1).all()
        return
    for x, y in zip(a, b):
        n = int(x["hsp"]["transcript_len"]) + 1
        ox, oy = int(x["hsp"]["transcript_off"]), int(y["hsp"]["transcript_off"])
        assert ox >= 0 and oy >= 0
        assert np.array_equal(tra[ox:ox + n], trb[oy:oy + n])


@pytest.mark.parametrize("arena_mb,rows", [(None, None), ("8", None), (None, "1"), ("8", "1")])
def test_blastx_golden_is_planned_and_extended_in_hbm_and_equals_the_reference(arena_mb, rows, monkeypatch):
    assert torch.cuda.is_available()
    if arena_mb:
        monkeypatch.setenv("DMND_TRACE_ARENA_MB", arena_mb)
    if rows:
        monkeypatch.setenv("DMND_SWEEP_ROWS", rows)
    cfg, recs = _golden()
    assert cfg["query_contexts"] == 6
    ctx = hip.Context()
    try:
        m = _search(ctx, cfg)
        plan, dev = ctx.extend_plan_stats(), ctx.extend_device_stats()
        assert plan["groups"] > 0 and plan["bands"] > 0, "the planner did not run on the device"
        assert dev["queries"] > 0 and dev["records"] > 0, "no read was extended on the device"
        assert dev["queries_back_to_host"] <= max(1, dev["queries"] // 50)
        _check(m, recs)
        pos = 0
        for r in sorted(recs, key=lambda x: x["query_id"]):
            for ref in r["matches"]:
                assert int(m[pos]["frame"]) == ref["hsps"][0]["frame"], r["query_id"]
                pos += 1
        assert len(np.unique(m["frame"])) == 6
    finally:
        ctx.close()


def test_blastx_golden_pairs_stay_below_the_planner_limits():
    """(no GPU work: the condition under which test 1 may hold the device half to a 2 % hand-back rate)"""
    cfg, _ = _golden()
    ctx = hip.Context()
    try:
        hits = _upload(ctx, cfg)
    finally:
        ctx.close()
    pairs = ts.pairs_of(hits, cfg["target"]["limits"])
    assert len(pairs) == 365 and sum(len(v) == 1 for v in pairs.values()) == 210
    assert max(len(v) for v in pairs.values()) == 10
    assert all(len({f for f, _ in v}) == 1 for v in pairs.values())
    assert len({r for r, _ in pairs}) == 99


@pytest.mark.parametrize("k,top", [(25, None), (1, None), (25, 10.0)], ids=["k25", "k1", "top10"])
@pytest.mark.parametrize("with_tr", [False, True], ids=["records", "transcripts"])
def test_blastx_golden_device_half_equals_host_path(k, top, with_tr, monkeypatch):
    cfg, _ = _golden()
    ctx = hip.Context()
    try:
        hits = _upload(ctx, cfg)
        qd, td = cfg["query"]["data"], cfg["target"]["data"]
        ctx.set_max_target_seqs(k)
        ctx.set_top_percent(top)
        a, tra = ctx.extend(qd, td, hits, threads=4, with_transcripts=with_tr)
        dev = ctx.extend_device_stats()
        assert dev["queries"] > 0 and dev["records"] > 0
        monkeypatch.setenv("DMND_EXTEND_DEVICE", "0")
        b, trb = ctx.extend(qd, td, hits, threads=4, with_transcripts=with_tr)
        assert ctx.extend_device_stats()["queries"] == 0
        assert len(a) > 60                                  # (99 reads have hits; --top 10 leaves 165 records, -k 1 fewer than 99)
        _same_records(a, b, tra, trb)
    finally:
        ctx.close()


def _constructed():
    if "set" not in _cache:
        db, doff, dna, off, kinds = ts.constructed_set()
        xd, xl = hip.translated_block(dna, off)
        td, tl = workload.sequence_set(db, doff)
        _cache["set"] = (db, doff, dna, off, kinds, xd, xl, td, tl)
    return _cache["set"]


def test_constructed_reads_device_half_equals_host_path(monkeypatch):
    """Cases (b) and (e) hold by construction (tests/translated_sets.py): a doubled read gives contexts 0 and 1 the same score on its
    protein, and a 300-base read with its gene in frame 1 has 100 letters in context 0 and 99 in the frame of its hits."""
    monkeypatch.setenv("DMND_EXTEND_GUARD", "1")
    db, doff, dna, off, kinds, xd, xl, td, tl = _constructed()
    params = hip.default_params()
    params.db_letters = float(doff[-1])
    ctx = hip.Context(params=params)
    try:
        ctx.upload_block(hip.TARGET, td, tl)
        ctx.upload_block(hip.QUERY, xd, xl)
        ctx.set_query_contexts(6)
        sp, gf = hip.seed_params_preset("default", params, threads=4)
        sp.query_translated = 1
        ctx.set_gapped_filter(gf)
        hits = ctx.seed_search(sp)
        ts.assert_cases_present(hits, tl, kinds)
        for k, top in ((25, None), (1, None), (25, 10.0)):
            ctx.set_max_target_seqs(k)
            ctx.set_top_percent(top)
            monkeypatch.delenv("DMND_EXTEND_DEVICE", raising=False)
            a, tra = ctx.extend(xd, td, hits, threads=4, with_transcripts=True)
            plan, dev = ctx.extend_plan_stats(), ctx.extend_device_stats()
            assert plan["groups"] > 0 and dev["queries"] > dev["queries_back_to_host"] and dev["records"] > 0, (k, top)
            monkeypatch.setenv("DMND_EXTEND_DEVICE", "0")
            b, trb = ctx.extend(xd, td, hits, threads=4, with_transcripts=True)
            assert ctx.extend_device_stats()["queries"] == 0
            _same_records(a, b, tra, trb)
            # the lower context wins where two reach the same score: every doubled read reports its own protein in frame 0
            if top is None and k == 25:
                for r, t in zip([i for i, kind in enumerate(kinds) if kind == "b"], ts.doubled_targets(doff)):
                    assert a["frame"][(a["query"] == r) & (a["target"] == t)].tolist() == [0], (r, t)
    finally:
        ctx.close()


@pytest.mark.parametrize("preset,k,max_chunks", [("default", 2000, None), ("default", 25, "1"), ("sensitive", 25, "1")],
                         ids=["declined-k2000", "capped", "capped-gapped-filter"])
def test_reads_that_come_back_to_the_host_path_on_a_fresh_context(preset, k, max_chunks, monkeypatch):
    """A translated call that was planned on the device and whose reads -- all of them: -k 2000 outgrows the LDS lists and the device half
    declines the call; some of them: DMND_EXTEND_MAX_CHUNKS=1 hands back the reads of the large family -- take the host path: there they
    are planned from the call's own hits, x-drop results and (--sensitive) filter flags, which are fetched only then. On a FRESH
    context, so that no earlier call has left a host buffer behind; records and transcripts equal the host path's (DMND_EXTEND_DEVICE=0,
    where the host plans as ever)."""
    monkeypatch.setenv("DMND_EXTEND_GUARD", "1")
    if max_chunks:
        monkeypatch.setenv("DMND_EXTEND_MAX_CHUNKS", max_chunks)
    db, doff, dna, off, kinds, xd, xl, td, tl = _constructed()
    params = hip.default_params()
    params.db_letters = float(doff[-1])
    out = []
    for device in (True, False):
        if not device:
            monkeypatch.setenv("DMND_EXTEND_DEVICE", "0")
        ctx = hip.Context(params=params)
        try:
            ctx.upload_block(hip.TARGET, td, tl)
            ctx.upload_block(hip.QUERY, xd, xl)
            ctx.set_query_contexts(6)
            sp, gf = hip.seed_params_preset(preset, params, threads=4)
            sp.query_translated = 1
            assert (gf > 0) == (preset == "sensitive")
            ctx.set_gapped_filter(gf)
            ctx.set_max_target_seqs(k)
            hits = ctx.seed_search(sp)
            out.append(ctx.extend(xd, td, hits, threads=4, with_transcripts=True))
            plan, dev = ctx.extend_plan_stats(), ctx.extend_device_stats()
            if not device:
                assert plan["groups"] == 0 and dev["queries"] == 0
            elif max_chunks:
                assert plan["groups"] > 0 and dev["queries_capped"] > 0 and dev["queries"] > dev["queries_back_to_host"]
            else:
                assert plan["groups"] > 0 and dev["queries"] == 0, "the device half took a call it was expected to decline"
        finally:
            ctx.close()
    assert len(out[0][0]) > 300
    _same_records(out[0][0], out[1][0], out[0][1], out[1][1])


@pytest.mark.parametrize("extra", [[], ["-k", "1"], ["--top", "10"], ["--sensitive"], ["-f", "6", "qseqid", "sseqid", "qstart", "qend", "btop"]],
                         ids=["default", "k1", "top10", "sensitive", "btop"])
def test_constructed_reads_cli_equals_the_reference_binary(tmp_path, extra):
    if not os.path.exists(REF):
        pytest.fail("oracle/_ref/diamond is missing: under -m gpu the reference binary is the checker, its absence is a failure")
    db, doff, dna, off, kinds, xd, xl, td, tl = _constructed()
    synth.write_fasta(str(tmp_path / "db.faa"), "t", db, doff)
    synth.write_dna_fasta(str(tmp_path / "reads.fna"), "r", dna, off)
    common = ["blastx", "-q", str(tmp_path / "reads.fna"), "-d", str(tmp_path / "db.faa"), "-p", "4"] + extra
    r = subprocess.run([REF] + common + ["--algo", "0", "--masking", "0", "--motif-masking", "0", "-o", str(tmp_path / "ref.tsv")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1000:]
    h = subprocess.run([CLI] + common + ["--masking", "0", "-o", str(tmp_path / "hip.tsv")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, DMND_TRACE="1", DMND_EXTEND_GUARD="1"))
    assert h.returncode == 0, h.stderr[-1500:]
    assert "dmnd_extend (device half)" in h.stderr, "the call did not reach the device half"
    assert open(tmp_path / "hip.tsv", "rb").read() == open(tmp_path / "ref.tsv", "rb").read()
    assert os.path.getsize(tmp_path / "ref.tsv") > 5000


def test_translated_call_with_id_filter_stays_on_the_host_path(monkeypatch):
    cfg, _ = _golden()
    ctx = hip.Context()
    try:
        hits = _upload(ctx, cfg)
        qd, td = cfg["query"]["data"], cfg["target"]["data"]
        ctx.set_filters(min_id=50.0)
        a, _ = ctx.extend(qd, td, hits, threads=4)
        assert ctx.extend_device_stats()["queries"] == 0 and ctx.extend_plan_stats()["groups"] == 0
        monkeypatch.setenv("DMND_EXTEND_DEVICE", "0")
        b, _ = ctx.extend(qd, td, hits, threads=4)
        assert len(a) > 50
        _same_records(a, b)
        ctx.set_filters()
        c, _ = ctx.extend(qd, td, hits, threads=4)
        assert len(c) > len(a)
    finally:
        ctx.close()
