"""-m gpu: --top searches through the device half of the extension stage (csrc/extend_kernels.hip: ext_top_append_kernel,
ext_top_final_kernel, ext_top_ffinal_kernel, ext_top_keys_kernel, ext_top_records_kernel; the arithmetic in csrc/top_core.h).
 * through hip.Context, queries of several ranking chunks (128 targets each under --top), --top 0 / 10 / 33.3, default and
   --sensitive seeds: queries are extended on the device, at most 2 % of them are handed back (the cap of the other device tests),
   and the records equal those of the same call on the host path (DMND_EXTEND_DEVICE=0) field for field and in order.
 * both branches of the append rule on a block whose scores fall steadily: --top 5 refuses the second chunk, --top 60 appends it.
 * ties at --top 0, more than 2 048 aligned targets of one query (what the -k filter path hands back), the chunk cap, the layout
   under DMND_EXTEND_GUARD fresh and after dmnd_extend_reserve.
 * with the HSP filters and --min-score, on the block of partial targets of tests/test_gpu_filters_device.py (rebuilt here) and on a
   block whose best-scoring targets all fail --id 90: the cut is taken against the best match that passed.
 * the CLI against the reference binary, three sensitivities, one and two database blocks; --top with -k is refused.
The percentages lie off the values a score can take (tests/test_top_core.py), so a correct device half hands no query back for a
score on the --top cutoff."""
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
FIELDS = "6 qseqid sseqid pident length evalue bitscore".split()
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/diamond missing")

FILTERS = {       # CLI flags, and the same through the C ABI: (min_id, query_cover, subject_cover, min_bit_score), approx_id
    "id": (["--id", "61.37"], (61.37, 0, 0, 0), 0),
    "covers": (["--query-cover", "80.13", "--subject-cover", "70.29"], (0, 80.13, 70.29, 0), 0),
    "approx_id": (["--approx-id", "45.77"], (0, 0, 0, 0), 45.77),
    "min_score": (["--min-score", "99.73"], (0, 0, 0, 99.73), 0),
    "id90": (["--id", "90"], (90, 0, 0, 0), 0),
}


def _pack(seqs):
    return np.concatenate(seqs).astype(np.int8), np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)


def _substituted(rng, s, n):
    t = s.copy()
    pos = rng.choice(len(s), n, replace=False)
    t[pos] = (t[pos] + rng.integers(1, 20, n)) % 20
    return t


def _files(d, data):
    db, doff, q, qoff = data
    synth.write_fasta(str(d / "db.faa"), "t", db, doff)
    synth.write_fasta(str(d / "q.faa"), "q", q, qoff)
    if os.path.exists(REF):
        assert subprocess.run([REF, "makedb", "--in", str(d / "db.faa"), "-d", str(d / "db")], capture_output=True).returncode == 0
    return d, data


@pytest.fixture(scope="module")
def chunks(tmp_path_factory):
    """120 queries against 6 families of 200: two ranking chunks of 128 per query"""
    return _files(tmp_path_factory.mktemp("chunks"), synth.generate(6, members=200, queries=120, seed=7, sub=(0.05, 0.6), qsub=(0.05, 0.5)))


@pytest.fixture(scope="module")
def families(tmp_path_factory):
    """300 queries against 300 families of 10, as the CLI tests use"""
    return _files(tmp_path_factory.mktemp("fam"), synth.generate(300, members=10, queries=300, seed=5, sub=(0.05, 0.6), qsub=(0.05, 0.5)))


@pytest.fixture(scope="module")
def gradient(tmp_path_factory):
    """12 queries of 300 random letters, 300 targets each: the query with a share of its letters substituted that rises steadily from
    5 % to 60 %, no indels -- the seed-hit score and the alignment score fall together, target after target."""
    rng = np.random.default_rng(23)
    qs, ts = [], []
    for qi in range(12):
        s = rng.integers(0, 20, 300).astype(np.int8)
        qs.append(s)
        for f in np.linspace(0.05, 0.60, 300):
            ts.append(_substituted(rng, s, int(round(300 * f))))
    return _files(tmp_path_factory.mktemp("gradient"), _pack(ts) + _pack(qs))


@pytest.fixture(scope="module")
def ties(tmp_path_factory):
    """20 queries of 200 letters; per query 6 targets with 20 % substitutions around four byte-identical ones with 5 %"""
    rng = np.random.default_rng(29)
    qs, ts = [], []
    for qi in range(20):
        s = rng.integers(0, 20, 200).astype(np.int8)
        qs.append(s)
        best = _substituted(rng, s, 10)
        for m in range(10):
            ts.append(best.copy() if m in (1, 4, 5, 8) else _substituted(rng, s, 40))
    return _files(tmp_path_factory.mktemp("ties"), _pack(ts) + _pack(qs))


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    """1 query of 300 letters, 2 600 copies of one target (the query with 10 % substitutions) with 2 % substitutions each"""
    rng = np.random.default_rng(31)
    s = rng.integers(0, 20, 300).astype(np.int8)
    t = _substituted(rng, s, 30)
    return _files(tmp_path_factory.mktemp("many"), _pack([_substituted(rng, t, 6) for _ in range(2600)]) + _pack([s]))


@pytest.fixture(scope="module")
def partial(tmp_path_factory):
    """The block of partial targets of tests/test_gpu_filters_device.py: 60 queries of 300 random letters, 16 targets each -- 8 pieces of
    the query that span 50 .. 100 % of it with 15 % substitutions, and 8 whole copies between random flanks that make up 0 .. 50 % of the
    target, 5 % substituted where the subject cover is below 70 %, 25 % above."""
    rng = np.random.default_rng(17)
    qs, ts = [], []
    for qi in range(60):
        s = rng.integers(0, 20, 300).astype(np.int8)
        qs.append(s)
        for f in np.linspace(0.5, 1.0, 8):
            n = int(round(300 * f))
            a = int(rng.integers(0, 300 - n + 1))
            ts.append(_substituted(rng, s[a:a + n], int(0.15 * n)))
        for f in np.linspace(0.5, 1.0, 8):
            flank = int(round(300 / f)) - 300
            t = _substituted(rng, s, 15 if f < 0.7 else 75)
            left = flank // 2
            ts.append(np.concatenate([rng.integers(0, 20, left), t, rng.integers(0, 20, flank - left)]).astype(np.int8))
    return _files(tmp_path_factory.mktemp("partial"), _pack(ts) + _pack(qs))


@pytest.fixture(scope="module")
def best_fail(tmp_path_factory):
    """30 queries of 300 random letters; per query 4 whole copies with 30 % substitutions (the best scores, about 70 % identity: they
    fail --id 90), 4 pieces of 150 letters with 3 % (lower scores inside --top 33.3 of the copies', they pass) and 4 pieces of 60
    letters (outside)."""
    rng = np.random.default_rng(37)
    qs, ts = [], []
    for qi in range(30):
        s = rng.integers(0, 20, 300).astype(np.int8)
        qs.append(s)
        for m in range(4):
            ts.append(_substituted(rng, s, 90))
            ts.append(_substituted(rng, s[20 * m: 20 * m + 150], 4))
            ts.append(_substituted(rng, s[50 * m: 50 * m + 60], 2))
    return _files(tmp_path_factory.mktemp("bestfail"), _pack(ts) + _pack(qs))


def _extend(data, top, device, monkeypatch, mode="fast", filters=None, env=None, reserve=False):
    """(records, device statistics, stage statistics) of one search of the block pair with --top"""
    db, doff, q, qoff = data
    monkeypatch.setenv("DMND_EXTEND_DEVICE", "1" if device else "0")
    for k in ("DMND_EXTEND_GUARD", "DMND_EXTEND_MAX_CHUNKS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    qd, ql = workload.sequence_set(q, qoff)
    td, tl = workload.sequence_set(db, doff)
    params = hip.default_params()
    params.db_letters = float(doff[-1])
    ctx = hip.Context(device=0, params=params)
    try:
        ctx.upload_block(hip.QUERY, qd, ql)
        if reserve:
            ctx.extend_reserve(64)
        ctx.upload_block(hip.TARGET, td, tl)
        sp, gf = hip.seed_params_preset(mode, params, threads=1)
        ctx.set_gapped_filter(gf)
        ctx.set_top_percent(top)
        if filters:
            _, f, approx = FILTERS[filters]
            ctx.set_filters(*f)
            ctx.set_approx_id(approx)
        hits = ctx.seed_search(sp)
        m, _ = ctx.extend(qd, td, hits, threads=4)
        return m.copy(), ctx.extend_device_stats(), ctx.extend_stats()
    finally:
        ctx.close()


def _device_equals_host(data, top, monkeypatch, **kw):
    host, hs, _ = _extend(data, top, False, monkeypatch, **{k: v for k, v in kw.items() if k != "env" and k != "reserve"})
    dev, ds, st = _extend(data, top, True, monkeypatch, **kw)
    print("--top", top, kw, "host records", len(host), "device stats", ds)
    assert hs["queries"] == 0 and len(host) > 0
    assert ds["queries"] > 0, "no query was extended on the device"
    assert dev.tobytes() == host.tobytes()
    return dev, ds, st


@pytest.mark.parametrize("mode", ["default", "sensitive"])
@pytest.mark.parametrize("top", [0, 10, 33.3])
def test_top_queries_of_several_chunks_are_extended_on_the_device_and_equal_the_host_path(chunks, top, mode, monkeypatch):
    assert torch.cuda.is_available()
    dev, ds, _ = _device_equals_host(chunks[1], top, monkeypatch, mode=mode)
    assert ds["queries_back_to_host"] <= ds["queries"] // 50
    assert 0 < ds["records"] <= len(dev)


def test_both_branches_of_the_append_rule(gradient, monkeypatch):
    """--top 5: the second chunk's best score lies under (int)(0.95 x lowest score left) -- refused, the tail rule ends the ranking.
    --top 60: it is appended and the ranking goes on to the last chunk. (--sensitive seeds: they find more than 256 of a query's 300
    targets, so there is a third chunk to go on to.)"""
    d5, s5, st5 = _device_equals_host(gradient[1], 5, monkeypatch, mode="sensitive")
    d60, s60, st60 = _device_equals_host(gradient[1], 60, monkeypatch, mode="sensitive")
    assert s5["queries_back_to_host"] == 0 and s60["queries_back_to_host"] == 0
    print("swept items: --top 5", st5["round1_targets"], "--top 60", st60["round1_targets"])
    assert st5["round1_targets"] >= 12 * 129              # the second chunk was swept ...
    assert st60["round1_targets"] > st5["round1_targets"]      # ... and only --top 60 went on past it
    assert len(d60) > 12 * 128 > len(d5)                  # --top 60 reports targets of the second chunk


@needs_ref
@pytest.mark.parametrize("top", ["5", "60"])
def test_both_branches_equal_the_reference_binary(gradient, tmp_path, top):
    _cli_equals_reference(gradient[0], tmp_path, ["--sensitive", "--top", top])


def test_ties_at_top_0_are_reported_in_target_order(ties, monkeypatch):
    dev, ds, _ = _device_equals_host(ties[1], 0, monkeypatch)
    assert ds["queries"] == 20 and ds["queries_back_to_host"] == 0
    assert len(dev) == 80
    for qi in range(20):
        r = dev[dev["query"] == qi]
        assert r["target"].tolist() == [10 * qi + m for m in (1, 4, 5, 8)]
        assert len(set(r["hsp"]["score"].tolist())) == 1


def test_more_than_2048_aligned_targets_stay_on_the_device(many, monkeypatch):
    dev, ds, _ = _device_equals_host(many[1], 50, monkeypatch)
    assert ds["queries"] == 1 and ds["queries_back_to_host"] == 0 and ds["queries_capped"] == 0
    assert ds["records"] == 2600 and len(dev) == 2600
    s = dev["hsp"]["score"]
    assert np.all(s[:-1] >= s[1:])
    capped, cs, _ = _extend(many[1], 50, True, monkeypatch, env={"DMND_EXTEND_MAX_CHUNKS": "2"})
    assert cs["queries"] == 1 and cs["queries_capped"] == 1 and cs["queries_back_to_host"] == 1 and cs["records"] == 0
    assert capped.tobytes() == dev.tobytes()


def test_top_layout_under_the_guard_fresh_and_reserved(chunks, monkeypatch):
    fresh, fs, _ = _device_equals_host(chunks[1], 10, monkeypatch, env={"DMND_EXTEND_GUARD": "1"})
    res, rs, _ = _extend(chunks[1], 10, True, monkeypatch, env={"DMND_EXTEND_GUARD": "1"}, reserve=True)
    assert fs["queries"] > 0 and rs["queries"] == fs["queries"] and rs["records"] == fs["records"] > 0
    assert res.tobytes() == fresh.tobytes()


@pytest.mark.parametrize("name", ["id", "covers", "approx_id", "min_score"])
def test_top_with_filters_equals_the_host_path(partial, name, monkeypatch):
    dev, ds, _ = _device_equals_host(partial[1], 33.3, monkeypatch, filters=name)
    assert ds["queries_back_to_host"] <= ds["queries"] // 50
    assert ds["queries_on_filter_threshold"] == 0
    if name == "covers":
        assert ds["records_filtered"] > 0


def test_top_cut_is_taken_against_the_best_match_that_passed(best_fail, monkeypatch):
    plain, _, _ = _extend(best_fail[1], 33.3, True, monkeypatch)
    dev, ds, _ = _device_equals_host(best_fail[1], 33.3, monkeypatch, filters="id90")
    assert ds["queries_back_to_host"] == 0 and ds["records_filtered"] >= 3 * 30      # (nearly all of the 4 x 30 whole copies lie inside the first cut)
    for qi in range(30):
        # unfiltered the whole copies (targets 12 qi + 0, 3, 6, 9) lead; filtered every query still reports -- the long pieces
        assert plain[plain["query"] == qi]["target"][0] % 3 == 0
        t = dev[dev["query"] == qi]["target"]
        assert len(t) > 0 and np.all(t % 3 == 1)


def _common(d, extra):
    return ["blastp", "--algo", "0", "--masking", "0", "--motif-masking", "0", "-q", str(d / "q.faa"), "-d", str(d / "db.dmnd"), "-f"] + FIELDS + extra


def _run(binary, args, out, env=None):
    return subprocess.run([binary] + args + ["-o", out] + (["-p", "4"] if binary == REF else []), capture_output=True, text=True, timeout=600, env=env)


def _cli_equals_reference(d, tmp_path, extra, min_bytes=1000):
    args = _common(d, extra)
    ref = _run(REF, args, str(tmp_path / "ref.tsv"))
    assert ref.returncode == 0, ref.stderr[-1000:]
    h = _run(CLI, args, str(tmp_path / "hip.tsv"), env=dict(os.environ, DMND_TRACE="1"))
    assert h.returncode == 0, h.stderr[-1000:]
    assert "dmnd_extend (device half):" in h.stderr and "queries, " in h.stderr, "the device half did not extend the call"
    want = open(tmp_path / "ref.tsv", "rb").read()
    assert len(want) > min_bytes
    assert open(tmp_path / "hip.tsv", "rb").read() == want
    return h.stderr


@needs_ref
@pytest.mark.parametrize("name", ["id", "covers", "approx_id", "min_score"])
def test_top_with_filters_equals_the_reference_binary(partial, tmp_path, name):
    _cli_equals_reference(partial[0], tmp_path, ["--fast", "--top", "33.3"] + FILTERS[name][0])


@needs_ref
def test_best_targets_fail_the_filter_equals_the_reference_binary(best_fail, tmp_path):
    _cli_equals_reference(best_fail[0], tmp_path, ["--fast", "--top", "33.3", "--id", "90"])
    rows = [l.split("\t") for l in open(tmp_path / "ref.tsv")]
    assert set(r[0] for r in rows) == set("q%d" % i for i in range(30)) and all(int(r[1][1:]) % 3 == 1 for r in rows)


@needs_ref
@pytest.mark.parametrize("mode", ["--fast", None, "--sensitive"], ids=["fast", "default", "sensitive"])
def test_top_10_equals_the_reference_binary(families, tmp_path, mode):
    _cli_equals_reference(families[0], tmp_path, ([mode] if mode else []) + ["--top", "10"])


@needs_ref
def test_top_10_over_two_database_blocks_equals_the_reference_binary(families, tmp_path):
    """a block size of 0.6 of the database's letters: two blocks, whose device-resident --top records the device join merges"""
    d, (db, doff, q, qoff) = families
    err = _cli_equals_reference(d, tmp_path, ["--top", "10", "-b", "%.9f" % (0.6 * float(doff[-1]) / 1e9), "-c1"])
    assert err.count(" handed back to the host (") >= 2


def test_top_with_k_is_refused(families, tmp_path):
    h = _run(CLI, _common(families[0], ["--top", "10", "-k", "5"]), str(tmp_path / "hip.tsv"))
    assert h.returncode != 0
    assert "--top and -k/--max-target-seqs are mutually exclusive" in h.stderr + h.stdout
