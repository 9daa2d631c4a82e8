"""-m gpu: the HSP filters (--id, --approx-id, --query-cover, --subject-cover, with --min-score) on translated (blastx) queries in
the device half of the extension stage. The filter kernel (csrc/extend_kernels.hip ext_filter_kernel) measures the query cover in bases
on the DNA read, whose lengths the device half keeps in HBM (Context.set_query_source_lengths); every test runs under DMND_EXTEND_GUARD.
 1. Device half against host path (DMND_EXTEND_DEVICE=0) in one process: every field of every record, with an arena the bytes of every
    transcript; the filter combinations of tests/test_gpu_filters_device.py at -k 25, -k 1 and --top 10, on the constructed read set
    of tests/translated_sets.py and on the cover set of tests/translated_filter_sets.py.
 2. --id 90 on reads whose best-scoring targets -- more than two ranking chunks of them -- all fail: the ranking goes on past them.
 3. Two query blocks in turn on one context, with other reads and read lengths; then other lengths for the same block.
 4. The gate from both sides: --query-cover without read lengths is refused, --id without them stays on the host path, with them it
    runs on the device.
 5. DMND_EXTEND_MAX_CHUNKS=1 with a filter on a fresh context: the reads handed back are planned by the host.
 6. The CLI against the reference binary, byte for byte.
Thresholds have two decimals that no value can reach: 61.37 %, 80.13 %, 70.29 % or 45.77 % of an integer count needs a length that is
a multiple of 10 000 (asserted: every read is shorter), so a correct device half hands no read back for a value on a threshold."""
import os
import subprocess

import numpy as np
import pytest
import torch

import translated_sets as ts
import translated_filter_sets as tfs
from diamond_amd import hip, synth, workload
from test_gpu_extend_translated import _same_records
from test_gpu_filters_device import COMBOS, CTX_FILTERS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "diamond")
CLI = os.path.join(os.path.dirname(HERE), "diamond_amd", "diamond-hip")
MODES = {"k25": (25, None), "k1": (1, None), "top10": (25, 10.0)}
_sets = {}


@pytest.fixture(autouse=True)
def _guard(monkeypatch):
    monkeypatch.setenv("DMND_EXTEND_GUARD", "1")
    monkeypatch.delenv("DMND_EXTEND_DEVICE", raising=False)


def _data(name):
    """(db, doff, dna, off, query block, its limits, target block, its limits) of a read set, made once"""
    if name not in _sets:
        db, doff, dna, off = {"constructed": lambda: ts.constructed_set()[:4], "cover": tfs.cover_set, "best_fail": lambda: tfs.best_fail_set()[:4]}[name]()
        assert int(np.diff(off).max()) < 10000, "a read long enough for a filter value to lie on a two-decimal threshold"
        xd, xl = hip.translated_block(dna, off)
        td, tl = workload.sequence_set(db, doff)
        _sets[name] = (db, doff, dna, off, xd, xl, td, tl)
    return _sets[name]


def _context(name, lengths=True, reads=None):
    """a context with the set's blocks uploaded (reads: a slice of its reads) and its seed hits"""
    db, doff, dna, off, xd, xl, td, tl = _data(name)
    params = hip.default_params()
    params.db_letters = float(doff[-1])
    ctx = hip.Context(params=params)
    try:
        ctx.upload_block(hip.TARGET, td, tl)
        ctx.set_query_contexts(6)
        sp, gf = hip.seed_params_preset("default", params, threads=4)
        sp.query_translated = 1
        ctx.set_gapped_filter(gf)
        hits, xd = _query_block(ctx, sp, name, lengths, reads)
    except Exception:
        ctx.close()
        raise
    return ctx, sp, hits, xd


def _query_block(ctx, sp, name, lengths=True, reads=None):
    db, doff, dna, off, xd, xl, td, tl = _data(name)
    if reads is not None:
        sub = off[reads.start:reads.stop + 1] - off[reads.start]
        xd, xl = hip.translated_block(dna[off[reads.start]:off[reads.stop]], sub)
        off = sub
    ctx.upload_block(hip.QUERY, xd, xl)
    if lengths:
        ctx.set_query_source_lengths(np.diff(off))
    return ctx.seed_search(sp), xd


@pytest.fixture(scope="module")
def searched():
    """one context per read set for the comparisons of test 1: blocks, read lengths and seed hits stay, the options change per case"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = _context(name)
        return made[name]
    yield get
    for ctx, _, _, _ in made.values():
        ctx.close()


def _set_options(ctx, name, mode):
    k, top = MODES[mode]
    f, approx = CTX_FILTERS[name]
    ctx.set_max_target_seqs(k)
    ctx.set_top_percent(top)
    ctx.set_filters(*f)
    ctx.set_approx_id(approx)


def _both_paths(ctx, xd, td, hits, with_tr, monkeypatch):
    monkeypatch.delenv("DMND_EXTEND_DEVICE", raising=False)
    a, tra = ctx.extend(xd, td, hits, threads=4, with_transcripts=with_tr)
    a, tra = a.copy(), (tra.copy() if with_tr else None)
    plan, dev = ctx.extend_plan_stats(), ctx.extend_device_stats()
    monkeypatch.setenv("DMND_EXTEND_DEVICE", "0")
    b, trb = ctx.extend(xd, td, hits, threads=4, with_transcripts=with_tr)
    assert ctx.extend_device_stats()["queries"] == 0 and ctx.extend_plan_stats()["groups"] == 0
    monkeypatch.delenv("DMND_EXTEND_DEVICE", raising=False)
    return a, tra, b, trb, plan, dev


def test_cover_set_thresholds_decide_and_reads_stay_below_a_ranking_chunk(searched, monkeypatch):
    """From the unfiltered host-path records of the cover set: each cover threshold of the tests removes some HSPs and keeps others.
    From its seed hits: no read has more than 128 targets, the condition under which test 1 holds the device half to the 2 % hand-back
    rate."""
    ctx, sp, hits, xd = searched("cover")
    db, doff, dna, off, _, _, td, tl = _data("cover")
    assert sorted(set((np.diff(off) % 3).tolist())) == [0, 1, 2] and len(set(np.diff(off).tolist())) > 40
    per_read = {}
    for r, t in ts.pairs_of(hits, tl):
        per_read[r] = per_read.get(r, 0) + 1
    assert len(per_read) > 60 and max(per_read.values()) <= 128
    _set_options(ctx, "min_score", "k25")
    ctx.set_filters()
    monkeypatch.setenv("DMND_EXTEND_DEVICE", "0")
    m, _ = ctx.extend(xd, td, hits, threads=4)
    qcov, scov = tfs.hsp_covers(m, off, tl)
    assert len(m) > 800 and len(np.unique(m["frame"])) == 6
    for t in (80.13, 70.13, 60.13):
        assert (qcov < t).sum() > 50 and (qcov >= t).sum() > 50, t
    for t in (70.29, 50.29):
        assert (scov < t).sum() > 20 and (scov >= t).sum() > 50, t


@pytest.mark.parametrize("with_tr", [False, True], ids=["records", "transcripts"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CTX_FILTERS))
@pytest.mark.parametrize("rset", ["constructed", "cover"])
def test_filtered_reads_are_extended_on_the_device_and_equal_the_host_path(searched, rset, name, mode, with_tr, monkeypatch):
    assert torch.cuda.is_available()
    ctx, sp, hits, xd = searched(rset)
    td = _data(rset)[6]
    _set_options(ctx, name, mode)
    a, tra, b, trb, plan, dev = _both_paths(ctx, xd, td, hits, with_tr, monkeypatch)
    print(rset, name, mode, "records", len(a), "plan", plan, "device", dev)
    assert plan["groups"] > 0, "the call was not planned on the device"
    assert dev["queries"] > 0, "no read was extended on the device"
    if name != "min_score":                     # (--min-score is a cutoff, not a filter: it is the one combination the parent takes too)
        assert dev["records_filtered"] > 0
    if rset == "cover":
        assert dev["queries_back_to_host"] <= max(1, dev["queries"] // 50)
    else:                                       # (its family of 320 is ranked over several chunks)
        assert dev["queries"] > dev["queries_back_to_host"]
    assert len(b) > 0
    _same_records(a, b, tra, trb)


def test_ranking_goes_on_past_targets_that_fail_the_identity_filter(monkeypatch):
    db, doff, dna, off, xd, xl, td, tl = _data("best_fail")
    n_long = tfs.best_fail_set()[4]
    assert len(off) - 1 == 12 and n_long > 2 * 128
    ctx, sp, hits, xd = _context("best_fail")
    try:
        per_read = {}
        for r, t in ts.pairs_of(hits, tl):
            per_read.setdefault(r, []).append(t)
        assert len(per_read) == 12 and all(sum(t % (n_long + 5) < n_long for t in v) > 2 * 128 for v in per_read.values())
        ctx.set_max_target_seqs(25)
        plain, _ = ctx.extend(xd, td, hits, threads=4)
        assert len(plain) == 12 * 25 and (plain["target"] % (n_long + 5) < n_long).all()      # unfiltered: the long targets only
        ctx.set_filters(min_id=90.0)
        a, tra, b, trb, plan, dev = _both_paths(ctx, xd, td, hits, True, monkeypatch)
        print("best_fail", "records", len(a), "plan", plan, "device", dev)
        assert plan["groups"] > 0 and dev["queries"] > dev["queries_back_to_host"] and dev["records"] > 0
        assert dev["records_filtered"] > 2 * 128 * (dev["queries"] - dev["queries_back_to_host"])      # per read finished here: more than two chunks
        assert sorted(set(b["query"].tolist())) == list(range(12)) and (b["target"] % (n_long + 5) >= n_long).all()      # filtered: pieces, for every read
        _same_records(a, b, tra, trb)
    finally:
        ctx.close()


def test_two_query_blocks_in_turn_and_other_lengths_for_the_same_block(monkeypatch):
    db, doff, dna, off, _, _, td, tl = _data("cover")
    ctx, sp, hits, xd = _context("cover", reads=slice(0, 45))
    try:
        _set_options(ctx, "all", "k25")
        for reads in (slice(0, 45), slice(45, 80)):
            if reads.start:
                hits, xd = _query_block(ctx, sp, "cover", reads=reads)          # upload_block(QUERY), then set_query_source_lengths
            a, _, b, _, plan, dev = _both_paths(ctx, xd, td, hits, False, monkeypatch)
            assert plan["groups"] > 0 and dev["queries"] > 0 and dev["records_filtered"] > 0, reads
            assert len(b) > 0
            _same_records(a, b)
        # the same block, other lengths: every read 90 bases longer than it is -- the query covers shrink, records go
        lens = np.diff(off)[45:80]
        ctx.set_filters(query_cover=60.13)
        ctx.set_approx_id(0)
        first, _, host_first, _, _, dev = _both_paths(ctx, xd, td, hits, False, monkeypatch)
        assert dev["queries"] > 0
        _same_records(first, host_first)
        ctx.set_query_source_lengths(lens + 90)
        second, _, host_second, _, _, dev = _both_paths(ctx, xd, td, hits, False, monkeypatch)
        assert dev["queries"] > 0 and dev["records_filtered"] > 0
        _same_records(second, host_second)
        assert 0 < len(second) < len(first)
        # ... and back
        ctx.set_query_source_lengths(lens)
        third, _ = ctx.extend(xd, td, hits, threads=4)
        assert ctx.extend_device_stats()["queries"] > 0
        _same_records(third, first)
    finally:
        ctx.close()


def test_the_gate_from_both_sides():
    db, doff, dna, off, _, _, td, tl = _data("constructed")
    ctx, sp, hits, xd = _context("constructed", lengths=False)
    try:
        ctx.set_filters(query_cover=70.13)
        with pytest.raises(hip.DiamondHipError, match="error -1: .*read lengths"):      # DMND_E_ARG
            ctx.extend(xd, td, hits, threads=4)
        ctx.set_filters(min_id=61.37)
        a, _ = ctx.extend(xd, td, hits, threads=4)
        assert ctx.extend_device_stats()["queries"] == 0 and ctx.extend_plan_stats()["groups"] == 0      # without read lengths: the host path
        ctx.set_query_source_lengths(np.diff(off))
        b, _ = ctx.extend(xd, td, hits, threads=4)
        dev = ctx.extend_device_stats()
        assert ctx.extend_plan_stats()["groups"] > 0 and dev["queries"] > dev["queries_back_to_host"] and dev["records_filtered"] > 0
        assert len(a) > 300
        _same_records(a, b)                                   # (--id reads no length: the same records either way)
        # a wrong number of lengths is none
        ctx.set_query_source_lengths(np.diff(off)[:-1])
        c, _ = ctx.extend(xd, td, hits, threads=4)
        assert ctx.extend_device_stats()["queries"] == 0 and ctx.extend_plan_stats()["groups"] == 0
        _same_records(a, c)
    finally:
        ctx.close()


def test_reads_at_the_chunk_cap_come_back_to_the_host_with_the_filters_on(monkeypatch):
    monkeypatch.setenv("DMND_EXTEND_MAX_CHUNKS", "1")
    td = _data("constructed")[6]
    out = []
    for device in (True, False):
        if not device:
            monkeypatch.setenv("DMND_EXTEND_DEVICE", "0")
        ctx, sp, hits, xd = _context("constructed")           # (a fresh context: no earlier call has left a host buffer behind)
        try:
            _set_options(ctx, "id", "k25")
            m, tr = ctx.extend(xd, td, hits, threads=4, with_transcripts=True)
            out.append((m.copy(), tr.copy()))
            plan, dev = ctx.extend_plan_stats(), ctx.extend_device_stats()
            if device:
                assert plan["groups"] > 0 and dev["queries_capped"] > 0 and dev["queries"] > dev["queries_back_to_host"] and dev["records_filtered"] > 0
            else:
                assert plan["groups"] == 0 and dev["queries"] == 0
        finally:
            ctx.close()
    assert len(out[0][0]) > 300
    _same_records(out[0][0], out[1][0], out[0][1], out[1][1])


CLI_CASES = {
    "query_cover": ["--query-cover", "70.13"],
    "id": ["--id", "61.37"],
    "subject_cover_k3": ["--subject-cover", "70.29", "-k", "3"],
    "approx_id": ["--approx-id", "45.77"],
    "all": COMBOS["all"],
    "id_top10": ["--id", "61.37", "--top", "10"],
    "query_cover_sensitive": ["--query-cover", "60.13", "--sensitive"],
    "btop": ["--query-cover", "70.13", "-f", "6", "qseqid", "sseqid", "qstart", "qend", "btop"],
}


@pytest.mark.parametrize("case", list(CLI_CASES))
@pytest.mark.parametrize("rset", ["constructed", "cover"])
def test_cli_equals_the_reference_binary(tmp_path, rset, case):
    if not os.path.exists(REF):
        pytest.fail("oracle/_ref/diamond is missing: under -m gpu the reference binary is the checker, its absence is a failure")
    db, doff, dna, off = _data(rset)[:4]
    synth.write_fasta(str(tmp_path / "db.faa"), "t", db, doff)
    synth.write_dna_fasta(str(tmp_path / "reads.fna"), "r", dna, off)
    common = ["blastx", "-q", str(tmp_path / "reads.fna"), "-d", str(tmp_path / "db.faa"), "-p", "4"] + CLI_CASES[case]
    r = subprocess.run([REF] + common + ["--algo", "0", "--masking", "0", "--motif-masking", "0", "-o", str(tmp_path / "ref.tsv")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1000:]
    h = subprocess.run([CLI] + common + ["--masking", "0", "-o", str(tmp_path / "hip.tsv")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, DMND_TRACE="1", DMND_EXTEND_GUARD="1"))
    assert h.returncode == 0, h.stderr[-1500:]
    assert "dmnd_extend (device half)" in h.stderr, "the call did not reach the device half"
    assert open(tmp_path / "hip.tsv", "rb").read() == open(tmp_path / "ref.tsv", "rb").read()
    assert os.path.getsize(tmp_path / "ref.tsv") > 5000
