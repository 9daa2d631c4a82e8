"""-m gpu: the device half of the extension stage (csrc/plan_kernels.hip, csrc/extend_kernels.hip; round 6) against the Match lists
the genuine reference's Extension::extend returned (tests/golden/ext_*.tap), with the checks on WHICH path produced the records:
 * the default search of a protein block is planned and extended in HBM (dmnd_extend_plan_stats / dmnd_extend_device_stats);
 * with a trace budget of 8 MB (DMND_TRACE_ARENA_MB, read when the context is made) round 1 sweeps for scores only and round 2
   sweeps the survivors again with traceback -- same records;
 * the same with the row classes of the sweeps forced on (DMND_SWEEP_ROWS=1: small blocks would not take them);
 * a skewed block whose queries have more targets than a ranking chunk (/root/reference/src/align/extend.cpp:79-92: 128 with -k 25)
   is ranked in chunks on the device -- same records as the reference binary on the same files (tests/test_gpu_skew.py holds the
   big case; here a small one that also runs with a tiny budget);
 * the limits the device half was sized for, each byte-identical to the reference binary: -k 1 with many bands per record under
   DMND_EXTEND_GUARD (a reused and a reserved buffer too), the chunk cap (lowered, and the natural one of 64 chunks) handing queries
   back to the host path, and e-values that underflow to 0.0 ordered on the device."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tapfile import read_ext_tap
from diamond_amd import hip, synth, workload
from test_gpu_seed import to_hip_params

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
REF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "diamond")
HSP_KEYS = "score q_begin q_end s_begin s_end length identities mismatches gap_openings gaps".split()


def _search(ctx, cfg):
    qd, ql, td, tl = cfg["query"]["data"], cfg["query"]["limits"], cfg["target"]["data"], cfg["target"]["limits"]
    ctx.upload_block(hip.QUERY, qd, ql)
    ctx.upload_block(hip.TARGET, td, tl)
    ctx.set_db_letters(float(tl[-1] - tl[0] - (len(tl) - 1)))
    ctx.set_gapped_filter(cfg["gapped_filter_evalue"])
    ctx.set_query_contexts(cfg["query_contexts"])
    hits = ctx.seed_search(to_hip_params(cfg))
    return ctx.extend(qd, td, hits, threads=4)[0]


def _check(m, recs):
    pos = 0
    for r in sorted(recs, key=lambda x: x["query_id"]):
        for ref in r["matches"]:
            got = m[pos]
            pos += 1
            assert (got["query"], got["target"]) == (r["query_id"], ref["target_block_id"])
            for k in HSP_KEYS:
                assert got["hsp"][k] == ref["hsps"][0][k], (k, r["query_id"])
            assert got["evalue"] == pytest.approx(ref["hsps"][0]["evalue"], rel=1e-6, abs=0)
            assert got["bit_score"] == pytest.approx(ref["hsps"][0]["bit_score"], rel=1e-12)
    assert pos == len(m)


@pytest.mark.parametrize("tap", ["ext_fast_synth.tap", "ext_default_synth.tap", "ext_sensitive.tap", "ext_long.tap"])
@pytest.mark.parametrize("arena_mb,rows", [(None, None), ("8", None), (None, "1"), ("8", "1")])
def test_protein_search_is_extended_in_hbm_and_equals_the_reference(tap, arena_mb, rows, monkeypatch):
    """rows = "1": the row classes of the packed 16-bit sweeps (eight items per wavefront, swipe16_kernels.hip) whatever the number
    of items -- by default only iterations of 131 072 items and more take them (tests/test_gpu_skew.py has such a block)."""
    assert torch.cuda.is_available()
    if arena_mb:
        monkeypatch.setenv("DMND_TRACE_ARENA_MB", arena_mb)
    if rows:
        monkeypatch.setenv("DMND_SWEEP_ROWS", rows)
    ctx = hip.Context()
    try:
        cfg, recs = read_ext_tap(os.path.join(GOLDEN, tap))
        m = _search(ctx, cfg)
        plan, dev = ctx.extend_plan_stats(), ctx.extend_device_stats()
        assert plan["groups"] > 0 and plan["bands"] > 0, "the planner did not run on the device"
        if tap != "ext_long.tap":      # (its 30 000-letter sequences give matrices above max_swipe_dp: those queries take the host path by design)
            assert dev["queries"] > 0 and dev["records"] > 0, "no query was extended on the device"
            # all but the queries handed back (ambiguous e-value order, saturation, groups the planner left to the host) came from HBM
            assert dev["queries_back_to_host"] <= max(1, dev["queries"] // 50)
        _check(m, recs)
    finally:
        ctx.close()


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/diamond missing")
@pytest.mark.parametrize("arena_mb", [None, "8"])
def test_queries_ranked_in_chunks_equal_the_reference_binary(tmp_path, arena_mb):
    """300 queries against 3 families of 400 members: every query has ~400 targets = four ranking chunks of 128. The CLI's records
    (device path; with arena_mb = 8 every chunk is swept for scores only) must equal the reference binary's output on the same files."""
    db, doff, q, qoff = synth.generate(3, members=400, queries=300, seed=11, sub=(0.1, 0.3), qsub=(0.1, 0.3))
    synth.write_fasta(str(tmp_path / "db.faa"), "t", db, doff)
    synth.write_fasta(str(tmp_path / "q.faa"), "q", q, qoff)
    assert subprocess.run([REF, "makedb", "--in", str(tmp_path / "db.faa"), "-d", str(tmp_path / "db")], capture_output=True).returncode == 0
    common = ["blastp", "--fast", "--algo", "0", "--masking", "0", "--motif-masking", "0", "-q", str(tmp_path / "q.faa"), "-d", str(tmp_path / "db.dmnd")]
    r = subprocess.run([REF] + common + ["-o", str(tmp_path / "ref.tsv"), "-p", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1000:]
    env = dict(os.environ, DMND_TRACE="1")
    if arena_mb:
        env["DMND_TRACE_ARENA_MB"] = arena_mb
    cli = os.path.join(os.path.dirname(HERE), "diamond_amd", "diamond-hip")
    h = subprocess.run([cli] + common + ["-o", str(tmp_path / "hip.tsv")], capture_output=True, text=True, timeout=600, env=env)
    assert h.returncode == 0, h.stderr[-1000:]
    chunks = [l for l in h.stderr.splitlines() if "dmnd_extend (device half): chunk" in l]
    assert any("chunk 1:" in l for l in chunks), "no query was ranked in more than one chunk on the device:\n" + h.stderr[-1500:]
    if arena_mb:
        assert any("scores only" in l for l in chunks)
    assert open(tmp_path / "hip.tsv", "rb").read() == open(tmp_path / "ref.tsv", "rb").read()
    assert os.path.getsize(tmp_path / "ref.tsv") > 10000


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/diamond missing")
@pytest.mark.parametrize("extra", [["-k", "1"], ["-k", "5"], ["-k", "200"], ["--comp-based-stats", "0"], ["-e", "1e-20"], ["--sensitive"]],
                         ids=["k1", "k5", "k200", "cbs0", "e1e-20", "sensitive"])
def test_device_extension_options_equal_the_reference_binary(tmp_path, extra):
    """The options that change what the device half decides -- -k below and above the ranking chunk (with -k 200 the chunk is 224 and
    a first chunk may have to grow: those queries stay on the host), no composition bias, a strict e-value cutoff, the gapped filter of
    --sensitive -- on queries with several ranking chunks and on queries with none: byte-identical to the reference binary."""
    db, doff, q, qoff = synth.generate(40, members=60, queries=300, seed=23, sub=(0.1, 0.4), qsub=(0.1, 0.4))
    synth.write_fasta(str(tmp_path / "db.faa"), "t", db, doff)
    synth.write_fasta(str(tmp_path / "q.faa"), "q", q, qoff)
    assert subprocess.run([REF, "makedb", "--in", str(tmp_path / "db.faa"), "-d", str(tmp_path / "db")], capture_output=True).returncode == 0
    common = ["blastp", "--algo", "0", "--masking", "0", "--motif-masking", "0", "-q", str(tmp_path / "q.faa"), "-d", str(tmp_path / "db.dmnd")] + extra
    if "--sensitive" not in extra:
        common.append("--fast")
    r = subprocess.run([REF] + common + ["-o", str(tmp_path / "ref.tsv"), "-p", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1000:]
    cli = os.path.join(os.path.dirname(HERE), "diamond_amd", "diamond-hip")
    h = subprocess.run([cli] + common + ["-o", str(tmp_path / "hip.tsv")], capture_output=True, text=True, timeout=600, env=dict(os.environ, DMND_TRACE="1"))
    assert h.returncode == 0, h.stderr[-1000:]
    assert "dmnd_extend (device half)" in h.stderr
    assert open(tmp_path / "hip.tsv", "rb").read() == open(tmp_path / "ref.tsv", "rb").read()
    assert os.path.getsize(tmp_path / "ref.tsv") > 1000


# ---- the limits the device half was sized for ---------------------------------------------------------------------------------
# Every case runs the CLI and the reference binary on the same files and compares the tabular output byte for byte; the DMND_TRACE
# summary of each device-half call says which path the queries took.
SUMMARY = re.compile(r"dmnd_extend \(device half\): (\d+) queries, (\d+) handed back to the host \((\d+) ambiguous, (\d+) saturated, (\d+) at the "
                     r"chunk cap of (\d+)\), (\d+) records; (\d+) groups, (\d+) bands, (\d+) bytes of work arrays")
FIELDS = "queries back ambiguous saturated capped cap records groups bands bytes".split()


def _summaries(stderr):
    return [dict(zip(FIELDS, map(int, m.groups()))) for m in SUMMARY.finditer(stderr)]


def _total(sums, key):
    return sum(s[key] for s in sums)


def _write_fasta(tmp_path, db, doff, q, qoff):
    synth.write_fasta(str(tmp_path / "db.faa"), "t", db, doff)
    synth.write_fasta(str(tmp_path / "q.faa"), "q", q, qoff)
    assert subprocess.run([REF, "makedb", "--in", str(tmp_path / "db.faa"), "-d", str(tmp_path / "db")], capture_output=True).returncode == 0


def _cli_equals_reference(tmp_path, args, env_extra, min_bytes=1000):
    """The CLI (DMND_TRACE=1 and env_extra) and the reference binary on tmp_path's files: byte-identical output; returns the CLI's
    stderr."""
    common = ["blastp", "--algo", "0", "--masking", "0", "--motif-masking", "0", "-q", str(tmp_path / "q.faa"), "-d", str(tmp_path / "db.dmnd")] + args
    r = subprocess.run([REF] + common + ["-o", str(tmp_path / "ref.tsv"), "-p", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1000:]
    env = dict(os.environ, DMND_TRACE="1", **env_extra)
    cli = os.path.join(os.path.dirname(HERE), "diamond_amd", "diamond-hip")
    h = subprocess.run([cli] + common + ["-o", str(tmp_path / "hip.tsv")], capture_output=True, text=True, timeout=600, env=env)
    assert h.returncode == 0, h.stderr[-1500:]
    assert open(tmp_path / "hip.tsv", "rb").read() == open(tmp_path / "ref.tsv", "rb").read()
    assert os.path.getsize(tmp_path / "ref.tsv") > min_bytes
    return h.stderr


def _concat(*sets):
    """(db, doff, q, qoff) of several synth.generate sets, one after the other"""
    db = np.concatenate([s[0] for s in sets])
    q = np.concatenate([s[2] for s in sets])
    doff, qoff, d0, q0 = [np.zeros(1, np.int64)], [np.zeros(1, np.int64)], 0, 0
    for s in sets:
        doff.append(s[1][1:] + d0)
        qoff.append(s[3][1:] + q0)
        d0 += int(s[1][-1]); q0 += int(s[3][-1])
    return db, np.concatenate(doff), q, np.concatenate(qoff)


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/diamond missing")
def test_k1_with_many_targets_per_query_stays_inside_the_work_arrays(tmp_path):
    """-k 1 with about 70 targets per query: round 2 holds one record per query, while the bands are many times more. Under
    DMND_EXTEND_GUARD every byte of the device buffers behind the call's layout (planner and device half) is checked at the end of
    the call: a clear sized by the bands (as launch_ext_begin's clear of the transcript offsets once was) fails the call."""
    db, doff, q, qoff = synth.generate(40, members=80, queries=300, seed=23, sub=(0.05, 0.25), qsub=(0.05, 0.25))
    _write_fasta(tmp_path, db, doff, q, qoff)
    err = _cli_equals_reference(tmp_path, ["--fast", "-k", "1"], {"DMND_EXTEND_GUARD": "1"})
    sums = _summaries(err)
    assert sums, err[-1500:]
    assert _total(sums, "queries") > _total(sums, "back") and _total(sums, "records") > 0, "no query was extended on the device"
    assert _total(sums, "groups") >= 50 * _total(sums, "queries"), "fewer than 50 targets per query"
    assert _total(sums, "bands") > 14 * _total(sums, "records")      # (where a clear by the bands left the layout)


def _search_block(ctx, db, doff, q, qoff):
    qd, ql = workload.sequence_set(q, qoff)
    td, tl = workload.sequence_set(db, doff)
    ctx.upload_block(hip.QUERY, qd, ql)
    ctx.upload_block(hip.TARGET, td, tl)
    hits = ctx.seed_search(hip.seed_params_fast(threads=4))
    m = ctx.extend(qd, td, hits, threads=4)[0].copy()
    return m, ctx.extend_plan_stats(), ctx.extend_device_stats(), len(np.unique(hits["query"]))


def _layout_bytes(groups, queries, bands, k):
    from test_extend_layout import layout
    return layout(groups, queries, bands, k)[1]


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/diamond missing")
def test_reused_and_reserved_work_arrays_at_k1_equal_the_reference_binary(tmp_path, monkeypatch):
    """One context, two calls, as a blocked run makes them: a -k 25 block with ~10 targets per query sizes the device buffers, then
    dmnd_set_max_target_seqs(1) and a block with ~150 targets per query whose layout is smaller -- the buffers are reused, with the
    bands many times the records. Then the second block alone on a fresh context after dmnd_extend_reserve with a small hint. Both
    under DMND_EXTEND_GUARD; both give the same records, and those equal the reference binary's -k 1 output on the same files."""
    monkeypatch.setenv("DMND_EXTEND_GUARD", "1")
    a = synth.generate(200, members=10, queries=1000, seed=5, sub=(0.1, 0.3), qsub=(0.1, 0.3))
    b = synth.generate(4, members=150, queries=60, seed=31, sub=(0.1, 0.3), qsub=(0.1, 0.3))
    params = hip.default_params()
    params.db_letters = float(b[1][-1])
    ctx = hip.Context(params=params)
    try:
        ma, plan_a, dev_a, nq_a = _search_block(ctx, *a)
        assert dev_a["queries"] > 0 and dev_a["records"] > 0
        ctx.set_max_target_seqs(1)
        mb, plan_b, dev_b, nq_b = _search_block(ctx, *b)
        assert dev_b["queries"] > 0 and dev_b["records"] > 0, "the second call did not extend on the device"
        assert dev_b["queries_back_to_host"] <= max(1, dev_b["queries"] // 50)
        assert plan_b["bands"] > 50 * dev_b["records"]
        assert _layout_bytes(plan_b["groups"], nq_b, plan_b["bands"], 1) < _layout_bytes(plan_a["groups"], nq_a, plan_a["bands"], 25), \
            "the second call's layout does not fit the first one's buffer"
    finally:
        ctx.close()
    fresh = hip.Context(params=params)
    try:
        fresh.set_max_target_seqs(1)
        qd, ql = workload.sequence_set(b[2], b[3])
        fresh.upload_block(hip.QUERY, qd, ql)
        fresh.extend_reserve(64)
        mr, _, dev_r, _ = _search_block(fresh, *b)
        assert dev_r["queries"] > 0 and dev_r["records"] > 0
    finally:
        fresh.close()
    assert mr.tobytes() == mb.tobytes()
    _write_fasta(tmp_path, *b)
    common = ["blastp", "--fast", "--algo", "0", "--masking", "0", "--motif-masking", "0", "-k", "1", "-q", str(tmp_path / "q.faa"), "-d", str(tmp_path / "db.dmnd")]
    r = subprocess.run([REF] + common + ["-o", str(tmp_path / "ref.tsv"), "-p", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1000:]
    qids = ["q%d" % i for i in range(len(b[3]) - 1)]
    tids = ["t%d" % i for i in range(len(b[1]) - 1)]
    assert hip.format_tab(mb, qids, tids) == open(tmp_path / "ref.tsv").read()


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/diamond missing")
@pytest.mark.parametrize("max_chunks", [1, 2])
def test_queries_past_the_chunk_cap_go_back_to_the_host_and_equal_the_reference_binary(tmp_path, max_chunks):
    """The block of test_queries_ranked_in_chunks_equal_the_reference_binary (300 queries of four ranking chunks each) plus 100
    queries of ~20 targets (one chunk), with the device's chunk cap lowered to 1 or 2 (DMND_EXTEND_MAX_CHUNKS): a query still
    ranking after its last allowed chunk is handed back to the host path, which ranks it to the end; the one-chunk queries stay
    on the device. Byte-identical to the reference binary."""
    big = synth.generate(3, members=400, queries=300, seed=11, sub=(0.1, 0.3), qsub=(0.1, 0.3))
    small = synth.generate(30, members=20, queries=100, seed=12, sub=(0.1, 0.3), qsub=(0.1, 0.3))
    _write_fasta(tmp_path, *_concat(big, small))
    err = _cli_equals_reference(tmp_path, ["--fast"], {"DMND_EXTEND_MAX_CHUNKS": str(max_chunks)}, min_bytes=10000)
    sums = _summaries(err)
    assert sums and all(s["cap"] == max_chunks for s in sums), err[-1500:]
    assert _total(sums, "capped") > 0, "no query was handed back at the chunk cap"
    assert _total(sums, "queries") - _total(sums, "back") >= 50, "the one-chunk queries did not stay on the device"
    chunks = [l for l in err.splitlines() if "dmnd_extend (device half): chunk" in l]
    assert not any("chunk %d:" % max_chunks in l for l in chunks), "a chunk past the cap ran on the device"


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/diamond missing")
def test_ranking_past_64_chunks_goes_back_to_the_host_and_equals_the_reference_binary(tmp_path):
    """A few queries against 8 500 identical copies of one target: every chunk of 128 brings hits as good as the k-th (equal
    e-values count as new, culling.cpp append_hits), so the reference ranks all 67 chunks. The device takes its 64 (the trace shows
    chunk 63), then hands the queries back to the host path instead of failing the call."""
    rng = np.random.default_rng(7)
    base = rng.integers(0, 20, 250).astype(np.int8)
    n_copies = 8500
    db = np.tile(base, n_copies)
    doff = np.arange(n_copies + 1, dtype=np.int64) * len(base)
    qs = [base.copy() for _ in range(3)]
    for i, s in enumerate(qs[1:]):
        pos = rng.choice(len(s), 10 * (i + 1), replace=False)
        s[pos] = (s[pos] + 1 + rng.integers(0, 19, len(pos))) % 20
    q = np.concatenate(qs)
    qoff = np.arange(4, dtype=np.int64) * len(base)
    _write_fasta(tmp_path, db, doff, q, qoff)
    err = _cli_equals_reference(tmp_path, ["--fast", "-k", "25"], {}, min_bytes=1000)
    chunks = [l for l in err.splitlines() if "dmnd_extend (device half): chunk" in l]
    assert any("chunk 63:" in l for l in chunks), err[-1500:]
    sums = _summaries(err)
    assert _total(sums, "capped") == 3 and all(s["cap"] == 64 for s in sums)


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/diamond missing")
def test_evalues_that_underflow_to_zero_stay_on_the_device_and_equal_the_reference_binary(tmp_path):
    """20 queries of 900 letters, each against 40 copies of itself with 0 - 5 substitutions: raw scores of ~4 500 (lambda x score
    far past the underflow of exp), so every e-value is 0.0 on the host and on the device, while the scores differ. -k 25 culls
    by (e-value, score, target): 0.0 against 0.0 is decided by the score, exactly -- no query goes back to the host."""
    rng = np.random.default_rng(17)
    qs, ts = [], []
    for _ in range(20):
        base = rng.integers(0, 20, 900).astype(np.int8)
        qs.append(base)
        for c in range(40):
            t = base.copy()
            pos = rng.choice(len(t), c % 6, replace=False)
            t[pos] = (t[pos] + 1 + rng.integers(0, 19, len(pos))) % 20
            ts.append(t)
    order = rng.permutation(len(ts))
    ts = [ts[i] for i in order]
    db, q = np.concatenate(ts), np.concatenate(qs)
    doff = np.arange(len(ts) + 1, dtype=np.int64) * 900
    qoff = np.arange(len(qs) + 1, dtype=np.int64) * 900
    _write_fasta(tmp_path, db, doff, q, qoff)
    err = _cli_equals_reference(tmp_path, ["--fast"], {}, min_bytes=10000)
    sums = _summaries(err)
    assert _total(sums, "queries") == 20, err[-1500:]
    assert _total(sums, "back") == 0, sums
    assert _total(sums, "records") == 20 * 25
    out = open(tmp_path / "ref.tsv").read().splitlines()
    assert len(out) == 500 and all(l.split("\t")[10] == "0.0" for l in out)
