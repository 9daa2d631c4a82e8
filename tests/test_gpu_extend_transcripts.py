"""-m gpu: transcripts from the device half of the extension stage (csrc/extend_kernels.hip ext_tr_* kernels, csrc/extend_device.hip).
A dmnd_extend call with a transcript arena takes the device half for every query it takes without one; the packed transcripts are
written into raw slots by the trace walk, kept in a dense store piece by piece and gathered into the caller's arena in record order.
 * both paths in one process on the golden taps: same records, same transcript bytes, offsets that tile the arena;
 * the CLI against the reference binary on every output format that needs transcripts, in each search mode of the device half
   (-k, the chunk-by-chunk filter path, --top, --top with filters, --sensitive), byte-identical;
 * several ranking chunks (kept traces and chunks swept again), several pieces per walk, both halves filling one arena, an arena one
   byte too small, and the same under DMND_EXTEND_GUARD."""
import ctypes
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
CLI = os.path.join(os.path.dirname(HERE), "diamond_amd", "diamond-hip")
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/diamond missing")

SUMMARY = re.compile(r"dmnd_extend \(device half\): (\d+) queries, (\d+) handed back to the host \((\d+) ambiguous, (\d+) saturated, (\d+) at the "
                     r"chunk cap of (\d+)\), (\d+) records; (\d+) groups, (\d+) bands, (\d+) bytes of work arrays")
FIELDS = "queries back ambiguous saturated capped cap records groups bands bytes".split()
TRANSCRIPTS = re.compile(r"dmnd_extend \(device half\) transcripts: (\d+) pieces of at most (\d+) raw bytes, (\d+) raw bytes, (\d+) kept bytes, (\d+) gathered bytes")


def _summaries(stderr):
    return [dict(zip(FIELDS, map(int, m.groups()))) for m in SUMMARY.finditer(stderr)]


def _transcript_lines(stderr):
    return [dict(zip("pieces limit raw kept gathered".split(), map(int, m.groups()))) for m in TRANSCRIPTS.finditer(stderr)]


# ---- 1. both paths in one process -------------------------------------------------------------------------------------------------

def _search_tap(cfg, monkeypatch, device):
    if device:
        monkeypatch.delenv("DMND_EXTEND_DEVICE", raising=False)
    else:
        monkeypatch.setenv("DMND_EXTEND_DEVICE", "0")
    ctx = hip.Context()
    try:
        qd, ql, td, tl = cfg["query"]["data"], cfg["query"]["limits"], cfg["target"]["data"], cfg["target"]["limits"]
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, td, tl)
        ctx.set_db_letters(float(tl[-1] - tl[0] - (len(tl) - 1)))
        ctx.set_gapped_filter(cfg["gapped_filter_evalue"])
        ctx.set_query_contexts(cfg["query_contexts"])
        hits = ctx.seed_search(to_hip_params(cfg))
        m, tr = ctx.extend(qd, td, hits, threads=4, with_transcripts=True)
        return m.copy(), tr.copy(), ctx.extend_device_stats()
    finally:
        ctx.close()


def _check_arena(m, tr):
    """every record's transcript_len + 1 bytes end in the terminator, and the offsets sorted tile [0, used) exactly"""
    off, ln = m["hsp"]["transcript_off"].astype(np.int64), m["hsp"]["transcript_len"].astype(np.int64)
    assert (off >= 0).all() and (ln >= 0).all()
    order = np.argsort(off, kind="stable")
    ends = off[order] + ln[order] + 1
    assert off[order][0] == 0 and np.array_equal(off[order][1:], ends[:-1]) and ends[-1] == len(tr)
    assert (tr[off + ln] == 0).all()


@pytest.mark.parametrize("tap", ["ext_fast_synth.tap", "ext_default_synth.tap", "ext_sensitive.tap"])
def test_host_and_device_paths_return_the_same_records_and_transcripts(tap, monkeypatch):
    assert torch.cuda.is_available()
    cfg, recs = read_ext_tap(os.path.join(GOLDEN, tap))
    mh, trh, dev_h = _search_tap(cfg, monkeypatch, device=False)
    md, trd, dev = _search_tap(cfg, monkeypatch, device=True)
    assert dev_h["queries"] == 0
    assert dev["queries"] > 0 and dev["records"] > 0, "a call with a transcript arena did not take the device half"
    assert dev["queries_back_to_host"] <= max(1, dev["queries"] // 50)
    assert len(md) == len(mh) > 0
    for name in md.dtype.names:
        if name != "hsp":
            assert np.array_equal(md[name], mh[name]), name
    for name in md["hsp"].dtype.names:
        if name != "transcript_off":
            assert np.array_equal(md["hsp"][name], mh["hsp"][name]), name
    _check_arena(mh, trh)
    _check_arena(md, trd)
    for a, b in zip(md, mh):
        n = int(a["hsp"]["transcript_len"]) + 1
        oa, ob = int(a["hsp"]["transcript_off"]), int(b["hsp"]["transcript_off"])
        assert np.array_equal(trd[oa: oa + n], trh[ob: ob + n]), (int(a["query"]), int(a["target"]))
    # ... and the reference's own transcripts where the tap holds them
    pos = 0
    for r in sorted(recs, key=lambda x: x["query_id"]):
        for ref in r["matches"]:
            got = md[pos]
            pos += 1
            assert (got["query"], got["target"]) == (r["query_id"], ref["target_block_id"])
            want = ref["hsps"][0]["transcript"]
            if len(want):
                o = int(got["hsp"]["transcript_off"])
                assert np.array_equal(trd[o: o + len(want)], want), (r["query_id"], ref["target_block_id"])
    assert pos == len(md)


# ---- 2 - 5, 7: the CLI against the reference binary ---------------------------------------------------------------------------------

BLOCK_2 = dict(n=40, members=60, queries=300, seed=23, sub=(0.1, 0.4), qsub=(0.1, 0.4))
BLOCK_3 = dict(n=3, members=400, queries=300, seed=11, sub=(0.1, 0.3), qsub=(0.1, 0.3))


def _block_dir(factory, name, spec):
    d = factory.mktemp(name)
    spec = dict(spec)
    db, doff, q, qoff = synth.generate(spec.pop("n"), **spec)
    synth.write_fasta(str(d / "db.faa"), "t", db, doff)
    synth.write_fasta(str(d / "q.faa"), "q", q, qoff)
    if os.path.exists(REF):
        assert subprocess.run([REF, "makedb", "--in", str(d / "db.faa"), "-d", str(d / "db")], capture_output=True).returncode == 0
    return d


@pytest.fixture(scope="module")
def block2(tmp_path_factory):
    return _block_dir(tmp_path_factory, "block2", BLOCK_2)


@pytest.fixture(scope="module")
def block3(tmp_path_factory):
    return _block_dir(tmp_path_factory, "block3", BLOCK_3)


_ref_cache = {}


def _normal(fmt, data):
    """what of an output names the program that wrote it: the version line of BLAST XML, the header lines of SAM"""
    if fmt == "xml":
        return b"\n".join(l for l in data.split(b"\n") if b"<BlastOutput_version>" not in l)
    if fmt == "sam":
        return b"\n".join(l for l in data.split(b"\n") if not l.startswith(b"@"))
    return data


FORMATS = {
    "pairwise": ["-f", "0"], "xml": ["-f", "5"], "sam": ["-f", "101"], "paf": ["-f", "paf"], "daa": ["-f", "100"],
    "tab": ["-f", "6", "qseqid", "sseqid", "btop", "cigar", "qseq_gapped", "sseq_gapped"], "btop": ["-f", "6", "qseqid", "sseqid", "btop"],
}
MODES = {
    "fast": ["--fast"], "filters": ["--fast", "--id", "40", "--query-cover", "50"], "top": ["--fast", "--top", "10"],
    "top_id": ["--fast", "--top", "10", "--id", "40"], "sensitive": ["--sensitive"], "id": ["--fast", "--id", "40"],
}


def _cli_equals_reference(block, tmp_path, mode, fmt, env_extra=None, min_bytes=1000):
    """The CLI (DMND_TRACE=1 and env_extra) and the reference binary on the block's files: the same output; returns the CLI's stderr.
    A DAA archive is compared as tests/test_gpu_cli.py compares them: one thread on either side, byte for byte."""
    common = ["blastp", "--algo", "0", "--masking", "0", "--motif-masking", "0", "-q", str(block / "q.faa"), "-d", str(block / "db.dmnd")] + MODES[mode] + FORMATS[fmt]
    ext = ".daa" if fmt == "daa" else ".out"
    key = (str(block), mode, fmt)
    if key not in _ref_cache:
        out = block / ("ref_%s_%s" % (mode, fmt))
        r = subprocess.run([REF] + common + ["-o", str(out) + ("" if fmt == "daa" else ext), "-p", "1" if fmt == "daa" else "4"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-1000:]
        _ref_cache[key] = open(str(out) + ext, "rb").read()
    want = _ref_cache[key]
    env = dict(os.environ, DMND_TRACE="1", **(env_extra or {}))
    out = tmp_path / "hip"
    h = subprocess.run([CLI] + common + ["-o", str(out) + ("" if fmt == "daa" else ext)] + (["-p", "1"] if fmt == "daa" else []), capture_output=True, text=True, timeout=600, env=env)
    assert h.returncode == 0, h.stderr[-1500:]
    assert len(want) > min_bytes
    assert _normal(fmt, open(str(out) + ext, "rb").read()) == _normal(fmt, want)
    return h.stderr


def _device_half_ran(err, arena=True):
    """arena: the CLI passed a transcript arena (every format here but PAF, which prints from the record's counts alone)"""
    sums, trs = _summaries(err), _transcript_lines(err)
    assert sums and sum(s["records"] for s in sums) > 0, "no record came from the device half:\n" + err[-1500:]
    if not arena:
        assert not trs, "a call without an arena made transcripts:\n" + err[-1500:]
        return sums, trs
    assert trs and sum(t["gathered"] for t in trs) > 0, "no transcript came from the device half:\n" + err[-1500:]
    assert all(t["gathered"] <= t["kept"] <= t["raw"] for t in trs)
    return sums, trs


@needs_ref
@pytest.mark.parametrize("fmt", ["pairwise", "xml", "sam", "paf", "tab", "daa"])
@pytest.mark.parametrize("mode", ["fast", "filters", "top", "top_id", "sensitive"])
def test_cli_formats_with_transcripts_equal_the_reference_binary(block2, tmp_path, mode, fmt):
    _device_half_ran(_cli_equals_reference(block2, tmp_path, mode, fmt), arena=fmt != "paf")


@needs_ref
@pytest.mark.parametrize("mode,arena_mb", [("fast", None), ("fast", "8"), ("id", None)], ids=["kept_traces", "swept_again", "filters_chunk_by_chunk"])
def test_transcripts_of_several_ranking_chunks_equal_the_reference_binary(block3, tmp_path, mode, arena_mb):
    """Four ranking chunks per query. arena_mb = 8: the chunks are swept for scores only and the survivors swept again with traceback
    before the walk; --id 40: every chunk is walked before the next is swept, and the kept transcripts of all chunks meet in one store."""
    err = _cli_equals_reference(block3, tmp_path, mode, "btop", {"DMND_TRACE_ARENA_MB": arena_mb} if arena_mb else None, min_bytes=10000)
    _device_half_ran(err)
    chunks = [l for l in err.splitlines() if "dmnd_extend (device half): chunk" in l]
    assert any("chunk 1:" in l for l in chunks), "no query was ranked in more than one chunk on the device:\n" + err[-1500:]
    if arena_mb:
        assert any("scores only" in l for l in chunks)


@needs_ref
@pytest.mark.parametrize("mode,guard", [("fast", False), ("fast", True), ("id", True)], ids=["pieces", "pieces_guard", "pieces_filters_guard"])
def test_a_walk_in_several_pieces_equals_the_reference_binary(block2, tmp_path, mode, guard):
    """DMND_EXTEND_PIECE_KB=512: about 7 000 walked targets of ~600 raw bytes each take several pieces per walk."""
    env = {"DMND_EXTEND_PIECE_KB": "512"}
    if guard:
        env["DMND_EXTEND_GUARD"] = "1"
    err = _cli_equals_reference(block2, tmp_path, mode, "tab", env)
    _, trs = _device_half_ran(err)
    assert sum(t["pieces"] for t in trs) >= 3, trs
    assert all(t["limit"] == 512 << 10 for t in trs)


@needs_ref
@pytest.mark.parametrize("mode", ["fast", "filters", "id"])
def test_transcripts_under_the_guard_equal_the_reference_binary(block2, tmp_path, mode):
    """DMND_EXTEND_GUARD=1: the bytes behind the transcript arrays, the raw slots, the store and the gathered output stay untouched."""
    _device_half_ran(_cli_equals_reference(block2, tmp_path, mode, "tab", {"DMND_EXTEND_GUARD": "1"}))


@needs_ref
def test_both_halves_fill_one_arena(block3, tmp_path):
    """DMND_EXTEND_MAX_CHUNKS=1: queries still ranking after their first chunk go back to the host path, which writes its transcripts
    behind the device half's in the same arena."""
    err = _cli_equals_reference(block3, tmp_path, "fast", "btop", {"DMND_EXTEND_MAX_CHUNKS": "1"}, min_bytes=10000)
    sums, _ = _device_half_ran(err)
    assert sum(s["back"] for s in sums) > 0, "no query was handed back to the host"


# ---- 6. an arena one byte too small ---------------------------------------------------------------------------------------------------

def test_an_arena_one_byte_too_small_is_refused_and_nothing_is_written_past_it():
    spec = dict(BLOCK_2)
    db, doff, q, qoff = synth.generate(spec.pop("n"), **spec)
    qd, ql = workload.sequence_set(q, qoff)
    td, tl = workload.sequence_set(db, doff)
    params = hip.default_params()
    params.db_letters = float(doff[-1])
    ctx = hip.Context(params=params)
    try:
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, td, tl)
        hits = np.ascontiguousarray(ctx.seed_search(hip.seed_params_fast(threads=4)), dtype=hip.SEED_HIT_DTYPE)
        first, tr_first = ctx.extend(qd, td, hits, threads=4, with_transcripts=True, transcript_cap=16 << 20)
        first, tr_first = first.copy(), tr_first.copy()
        dev = ctx.extend_device_stats()
        assert dev["records"] > 0 and len(tr_first) > 1000
        used_ok = len(tr_first)
        v = ctypes.c_void_p

        def call(cap):
            arena = np.full(used_ok + 4096, 0xC3, np.uint8)          # (the arena, then 4096 pattern bytes at the least)
            out = np.zeros(len(first) + 16, dtype=hip.MATCH_DTYPE)
            n, used = ctypes.c_int64(0), ctypes.c_int64(0)
            rc = ctx.lib.dmnd_extend(ctx.h, qd.ctypes.data_as(v), td.ctypes.data_as(v), hits.ctypes.data_as(v), ctypes.c_int64(hits.size), 4, ctypes.c_uint32(510),
                                     out.ctypes.data_as(v), ctypes.c_int64(out.size), ctypes.byref(n), arena.ctypes.data_as(v), ctypes.c_int64(cap), ctypes.byref(used))
            return rc, out[:max(0, n.value)], arena, used.value

        rc, _, arena, _ = call(used_ok - 1)
        assert rc == -5, (rc, ctx.lib.dmnd_last_error())                      # DMND_E_CAP
        assert b"transcript arena too small" in ctx.lib.dmnd_last_error()
        assert (arena[used_ok - 1:] == 0xC3).all(), "bytes past the arena's capacity were written"
        rc, again, arena, used = call(used_ok)
        assert rc == 0 and used == used_ok
        assert np.array_equal(again, first) and np.array_equal(arena[:used], tr_first)      # (field by field: the records' padding is nobody's)
        assert (arena[used_ok:] == 0xC3).all()
    finally:
        ctx.close()
