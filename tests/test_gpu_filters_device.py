"""-m gpu: --approx-id, and the HSP filters (--id, --approx-id, --query-cover, --subject-cover, --min-score) applied by the device
half of the extension stage (csrc/extend_kernels.hip: ext_fcand_kernel, ext_filter_kernel, ext_fappend_kernel, ext_ffinal_kernel).
 * --approx-id through the CLI against the reference binary, --fast / default / --sensitive, a low and a high threshold, with
   approx_pident in the output; the refusal together with --id.
 * through hip.Context: under each filter combination queries are extended on the device, and the records equal those of the same
   call on the host path (DMND_EXTEND_DEVICE=0) exactly.
 * the CLI against the reference binary for the same combinations at -k 1, 5 and 25, on a block whose queries have dozens of
   targets, and on one whose best-scoring targets all fail --id, so that the ranking has to go on past them.
 * the edges of the layout: -k 1 with a filter under DMND_EXTEND_GUARD, and DMND_EXTEND_MAX_CHUNKS=1.
Thresholds are chosen off the values an HSP can take (61.37 % identity needs a length that is a multiple of 10 000), so a correct
device half hands no query back for a value on a threshold; the share of queries it may hand back for any reason is capped at 2 %,
the cap of the unfiltered device tests (tests/test_gpu_extend_device.py).
The cover filters are run on a block of partial-length targets (pieces of the query: query cover 50 .. 100 %; the query between
random flanks: subject cover 50 .. 100 %), where each of the two thresholds removes some targets and keeps others, and where a
cover measured against the other sequence's length gives another answer."""
import os
import subprocess

import numpy as np
import pytest
import torch

from diamond_amd import hip, synth, workload

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "diamond")
CLI = os.path.join(os.path.dirname(HERE), "diamond_amd", "diamond-hip")
FIELDS = "6 qseqid sseqid pident approx_pident length evalue bitscore".split()
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/diamond missing")

COMBOS = {
    "id": ["--id", "61.37"],
    "covers": ["--query-cover", "80.13", "--subject-cover", "70.29"],
    "approx_id": ["--approx-id", "45.77"],
    "min_score": ["--min-score", "99.73"],
    "all": ["--approx-id", "41.19", "--query-cover", "60.13", "--subject-cover", "50.29", "--min-score", "60.31"],
}
CTX_FILTERS = {       # the same through the C ABI: (min_id, query_cover, subject_cover, min_bit_score), approx_id
    "id": ((61.37, 0, 0, 0), 0), "covers": ((0, 80.13, 70.29, 0), 0), "approx_id": ((0, 0, 0, 0), 45.77), "min_score": ((0, 0, 0, 99.73), 0),
    "all": ((0, 60.13, 50.29, 60.31), 41.19),
}


def _run(binary, args, out, env=None):
    r = subprocess.run([binary] + args + ["-o", out] + (["-p", "4"] if binary == REF else []), capture_output=True, text=True, timeout=600, env=env)
    return r


@pytest.fixture(scope="module")
def families(tmp_path_factory):
    """300 queries against 300 families of 10 (a few targets per query), as the CLI tests use"""
    d = tmp_path_factory.mktemp("fam")
    db, doff, q, qoff = synth.generate(300, members=10, queries=300, seed=5, sub=(0.05, 0.6), qsub=(0.05, 0.5))
    synth.write_fasta(str(d / "db.faa"), "t", db, doff)
    synth.write_fasta(str(d / "q.faa"), "q", q, qoff)
    if os.path.exists(REF):
        assert subprocess.run([REF, "makedb", "--in", str(d / "db.faa"), "-d", str(d / "db")], capture_output=True).returncode == 0
    return d


@pytest.fixture(scope="module")
def chunks(tmp_path_factory):
    """120 queries against 6 families of 200: dozens of targets per query, several times -k"""
    d = tmp_path_factory.mktemp("chunks")
    db, doff, q, qoff = synth.generate(6, members=200, queries=120, seed=7, sub=(0.05, 0.6), qsub=(0.05, 0.5))
    synth.write_fasta(str(d / "db.faa"), "t", db, doff)
    synth.write_fasta(str(d / "q.faa"), "q", q, qoff)
    if os.path.exists(REF):
        assert subprocess.run([REF, "makedb", "--in", str(d / "db.faa"), "-d", str(d / "db")], capture_output=True).returncode == 0
    return d, (db, doff, q, qoff)


@pytest.fixture(scope="module")
def best_fail(tmp_path_factory):
    """12 queries of 300 random letters; per query 280 targets that are the query with 30 % of its letters substituted (no indels: a
    high seed-hit score and a high alignment score, about 70 % identity) and 5 targets that are 50-letter pieces of it, unchanged
    (a low score, 100 % identity). With --id 90 every target of the first two ranking chunks fails."""
    d = tmp_path_factory.mktemp("bestfail")
    rng = np.random.default_rng(3)
    aa = "ARNDCQEGHILKMFPSTWYV"
    with open(d / "db.faa", "w") as fdb, open(d / "q.faa", "w") as fq:
        for qi in range(12):
            s = rng.integers(0, 20, 300)
            fq.write(">q%d\n%s\n" % (qi, "".join(aa[x] for x in s)))
            for m in range(280):
                t = s.copy()
                pos = rng.choice(300, 90, replace=False)
                t[pos] = (t[pos] + rng.integers(1, 20, 90)) % 20
                fdb.write(">long%d_%d\n%s\n" % (qi, m, "".join(aa[x] for x in t)))
            for m in range(5):
                fdb.write(">piece%d_%d\n%s\n" % (qi, m, "".join(aa[x] for x in s[40 * m + 10: 40 * m + 60])))
    if os.path.exists(REF):
        assert subprocess.run([REF, "makedb", "--in", str(d / "db.faa"), "-d", str(d / "db")], capture_output=True).returncode == 0
    return d


@pytest.fixture(scope="module")
def partial(tmp_path_factory):
    """60 queries of 300 random letters, 16 targets each: 8 pieces of the query that span 50 .. 100 % of it, 15 % of their letters
    substituted (query cover = the span, subject cover about 100 %), and 8 whole copies between random flanks that make up 0 .. 50 % of
    the target (query cover about 100 %, subject cover 50 .. 100 %) -- 5 % substituted where the subject cover is below 70 %, 25 %
    above, so that a query's best-scoring targets fail the subject cover."""
    d = tmp_path_factory.mktemp("partial")
    rng = np.random.default_rng(17)
    qs, ts = [], []
    for qi in range(60):
        s = rng.integers(0, 20, 300).astype(np.int8)
        qs.append(s)
        for f in np.linspace(0.5, 1.0, 8):
            n = int(round(300 * f))
            a = int(rng.integers(0, 300 - n + 1))
            t = s[a:a + n].copy()
            pos = rng.choice(n, int(0.15 * n), replace=False)
            t[pos] = (t[pos] + rng.integers(1, 20, len(pos))) % 20
            ts.append(t)
        for f in np.linspace(0.5, 1.0, 8):
            flank = int(round(300 / f)) - 300
            t = s.copy()
            pos = rng.choice(300, 15 if f < 0.7 else 75, replace=False)      # (the copies that will fail the subject cover score best)
            t[pos] = (t[pos] + rng.integers(1, 20, len(pos))) % 20
            left = flank // 2
            ts.append(np.concatenate([rng.integers(0, 20, left), t, rng.integers(0, 20, flank - left)]).astype(np.int8))
    pack = lambda seqs: (np.concatenate(seqs).astype(np.int8), np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64))
    (db, doff), (q, qoff) = pack(ts), pack(qs)
    synth.write_fasta(str(d / "db.faa"), "t", db, doff)
    synth.write_fasta(str(d / "q.faa"), "q", q, qoff)
    if os.path.exists(REF):
        assert subprocess.run([REF, "makedb", "--in", str(d / "db.faa"), "-d", str(d / "db")], capture_output=True).returncode == 0
    return d, (db, doff, q, qoff)


def _common(d, extra):
    return ["blastp", "--algo", "0", "--masking", "0", "--motif-masking", "0", "-q", str(d / "q.faa"), "-d", str(d / "db.dmnd"), "-f"] + FIELDS + extra


@needs_ref
@pytest.mark.parametrize("mode", ["--fast", None, "--sensitive"], ids=["fast", "default", "sensitive"])
@pytest.mark.parametrize("x", ["40", "60"])
def test_approx_id_equals_the_reference_binary(families, tmp_path, mode, x):
    d = families
    sens = [mode] if mode else []
    plain = _run(REF, _common(d, sens), str(tmp_path / "plain.tsv"))
    ref = _run(REF, _common(d, sens + ["--approx-id", x]), str(tmp_path / "ref.tsv"))
    assert plain.returncode == 0 and ref.returncode == 0, ref.stderr[-1000:]
    want = open(tmp_path / "ref.tsv", "rb").read()
    assert len(want) > 0 and want != open(tmp_path / "plain.tsv", "rb").read()       # the threshold removes some records and leaves some
    h = _run(CLI, _common(d, sens + ["--approx-id", x]), str(tmp_path / "hip.tsv"))
    assert h.returncode == 0, h.stderr[-1000:]
    assert open(tmp_path / "hip.tsv", "rb").read() == want


def test_approx_id_with_id_is_refused(families, tmp_path):
    h = _run(CLI, _common(families, ["--approx-id", "50", "--id", "50"]), str(tmp_path / "hip.tsv"))
    assert h.returncode != 0
    assert "Incompatible options: --approx-id, --id." in h.stderr + h.stdout


def _extend(data, name, k, device, monkeypatch):
    db, doff, q, qoff = data
    monkeypatch.setenv("DMND_EXTEND_DEVICE", "1" if device else "0")
    qd, ql = workload.sequence_set(q, qoff)
    td, tl = workload.sequence_set(db, doff)
    params = hip.default_params()
    params.db_letters = float(doff[-1])
    ctx = hip.Context(device=0, params=params)
    try:
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, td, tl)
        sp, gf = hip.seed_params_preset("fast", params, threads=1)
        ctx.set_gapped_filter(gf)
        ctx.set_max_target_seqs(k)
        f, approx = CTX_FILTERS[name]
        ctx.set_filters(*f)
        ctx.set_approx_id(approx)
        hits = ctx.seed_search(sp)
        m, _ = ctx.extend(qd, td, hits, threads=4)
        return m.copy(), dict(ctx.extend_device_stats(), plan=ctx.extend_plan_stats())
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(COMBOS))
def test_filtered_queries_are_extended_on_the_device_and_equal_the_host_path(chunks, partial, name, monkeypatch):
    assert torch.cuda.is_available()
    _, data = partial if name == "covers" else chunks
    host, hs = _extend(data, name, 5, False, monkeypatch)
    dev, ds = _extend(data, name, 5, True, monkeypatch)
    print(name, "host records", len(host), "device stats", ds)
    assert hs["queries"] == 0 and len(host) > 0
    assert ds["queries"] > 0, "no query was extended on the device"
    assert ds["queries_back_to_host"] <= ds["queries"] // 50
    assert ds["queries_on_filter_threshold"] == 0
    if name != "min_score":                     # (--min-score is a cutoff, not a filter)
        assert ds["records_filtered"] > 0
    assert dev.tobytes() == host.tobytes()


@needs_ref
@pytest.mark.parametrize("k", ["1", "5", "25"])
@pytest.mark.parametrize("name", list(COMBOS))
def test_filters_equal_the_reference_binary(chunks, tmp_path, name, k):
    d, _ = chunks
    args = _common(d, ["--fast", "-k", k] + COMBOS[name])
    ref = _run(REF, args, str(tmp_path / "ref.tsv"))
    assert ref.returncode == 0, ref.stderr[-1000:]
    h = _run(CLI, args, str(tmp_path / "hip.tsv"), env=dict(os.environ, DMND_TRACE="1"))
    assert h.returncode == 0, h.stderr[-1000:]
    assert "dmnd_extend (device half)" in h.stderr
    want = open(tmp_path / "ref.tsv", "rb").read()
    assert len(want) > 1000
    assert open(tmp_path / "hip.tsv", "rb").read() == want


@needs_ref
@pytest.mark.parametrize("k", ["1", "5", "25"])
def test_cover_filters_on_partial_targets_equal_the_reference_binary(partial, tmp_path, k):
    d, _ = partial
    plain = _run(REF, _common(d, ["--fast", "-k", k]), str(tmp_path / "plain.tsv"))
    args = _common(d, ["--fast", "-k", k] + COMBOS["covers"])
    ref = _run(REF, args, str(tmp_path / "ref.tsv"))
    assert plain.returncode == 0 and ref.returncode == 0, ref.stderr[-1000:]
    want = open(tmp_path / "ref.tsv", "rb").read()
    assert len(want) > 1000 and want != open(tmp_path / "plain.tsv", "rb").read()      # the covers remove some records and leave some
    h = _run(CLI, args, str(tmp_path / "hip.tsv"), env=dict(os.environ, DMND_TRACE="1"))
    assert h.returncode == 0, h.stderr[-1000:]
    assert "dmnd_extend (device half)" in h.stderr
    assert open(tmp_path / "hip.tsv", "rb").read() == want


@needs_ref
@pytest.mark.parametrize("k", ["1", "5"])
def test_ranking_goes_on_past_targets_that_fail_the_filter(best_fail, tmp_path, k):
    d = best_fail
    plain = _run(REF, _common(d, ["--fast", "-k", k]), str(tmp_path / "plain.tsv"))
    args = _common(d, ["--fast", "-k", k, "--id", "90"])
    ref = _run(REF, args, str(tmp_path / "ref.tsv"))
    assert plain.returncode == 0 and ref.returncode == 0, ref.stderr[-1000:]
    # from the reference alone: unfiltered, every query reports the long targets; filtered, every query still reports hits -- pieces
    assert all(l.split("\t")[1].startswith("long") for l in open(tmp_path / "plain.tsv"))
    rows = [l.split("\t") for l in open(tmp_path / "ref.tsv")]
    assert set(r[0] for r in rows) == set("q%d" % i for i in range(12)) and all(r[1].startswith("piece") for r in rows)
    h = _run(CLI, args, str(tmp_path / "hip.tsv"), env=dict(os.environ, DMND_TRACE="1"))
    assert h.returncode == 0, h.stderr[-1000:]
    assert "dmnd_extend (device half): chunk 1:" in h.stderr, "the device half did not rank past the first chunk"
    assert open(tmp_path / "hip.tsv", "rb").read() == open(tmp_path / "ref.tsv", "rb").read()


@needs_ref
@pytest.mark.parametrize("env", [{"DMND_EXTEND_GUARD": "1"}, {"DMND_EXTEND_MAX_CHUNKS": "1"}], ids=["guard_k1", "max_chunks_1"])
def test_layout_edges_under_filters(best_fail, tmp_path, env):
    """-k 1 under the guard, 285 targets per query: the walked list (every group) is at its largest next to the record capacity (one
    per query). One chunk allowed: the queries, which all rank on past their first chunk, go back to the host with the filters on."""
    d = best_fail
    args = _common(d, ["--fast", "-k", "1", "--id", "90"])
    ref = _run(REF, args, str(tmp_path / "ref.tsv"))
    assert ref.returncode == 0, ref.stderr[-1000:]
    h = _run(CLI, args, str(tmp_path / "hip.tsv"), env=dict(os.environ, DMND_TRACE="1", **env))
    assert h.returncode == 0, h.stderr[-1500:]
    assert "dmnd_extend (device half)" in h.stderr
    if "DMND_EXTEND_MAX_CHUNKS" in env:
        assert "at the chunk cap of 1" in h.stderr and " 0 at the chunk cap" not in h.stderr
    want = open(tmp_path / "ref.tsv", "rb").read()
    assert len(want.splitlines()) == 12 and open(tmp_path / "hip.tsv", "rb").read() == want
