"""-m gpu: traceback_kernel (csrc/swipe_kernels.hip, the speculative wave form traceback_walk_wave of the serial walk in swipe_core.h)
on the constructed corpus of tests/traceback_cases.py (the CPU file test_traceback_cases.py asserts what that corpus contains): gaps
of 1 .. 200 letters in both directions around the multiples of 63 and 64, diagonal runs of 63 / 64 / 65 / 127 / ... columns ended
by the matrix origin, by the score, at a running score of exactly 0 and by a gap, two gaps back to back, target letters 20 - 24 and
bit 7, a random bias, matrices of the items' own (the 32-bit kernels' trace layouts at P <= 4), a saturating item, bands of the
classes 8 / 16 / 32 and of several wavefronts, with score-0 and 1 x 1 items in between -- in every band class, rows off and on.
Every number, every transcript byte and the terminator equal the oracle's; a failure names the case's tag. The same corpus rebuilt
for BLOSUM80 25/2, PAM30 5/2 and PAM250 11/3 (traceback_cases.corpus(scheme)) on a context of that system, in every mode, rows off
and on: the walk's own gap accounting under gap extend 2 and 3 and its stop rule over PAM30's cell scores."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import scoring_schemes as ss
import traceback_cases as tc
from diamond_amd import hip, synth, workload
from gpu_util import pack_records_m
from test_gpu_swipe import KEYS, STAT_KEYS, _rescore

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "diamond")
CLI = os.path.join(os.path.dirname(HERE), "diamond_amd", "diamond-hip")


@pytest.fixture(scope="module")
def c():
    return tc.corpus()


@pytest.fixture(scope="module")
def ref(c):
    return tc.oracle(c)


@pytest.fixture(scope="module")
def ctx(c):
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    x = hip.Context(params=c.params)
    yield x
    x.close()


def _upload(ctx, c, index):
    qb, tb, cbs, items, meta, mats = pack_records_m([c.recs[int(k)] for k in index])
    ctx.upload_block(hip.QUERY, qb)
    ctx.upload_block(hip.TARGET, tb)
    ctx.upload_cbs(cbs)
    ctx.upload_matrices(mats)
    return items


def _check_traceback(c, ref, index, out, tr, what):
    """out / tr: a SWIPE_TRACEBACK result for the records `index`, in that order"""
    for pos, k in enumerate(index):
        o, otr, _ = ref[int(k)]
        g, tag = out[pos], c.recs[int(k)]["tag"]
        assert g["score"] == o["score"], (what, tag, "score", int(g["score"]), o["score"])
        off, n = int(g["transcript_off"]), int(g["transcript_len"])
        if o["score"] > 0:
            for key in KEYS:
                assert g[key] == o[key], (what, tag, key, int(g[key]), o[key])
            assert n == len(otr) and np.array_equal(tr[off: off + n], otr), (what, tag, "transcript", tr[off: off + n].tolist(), otr.tolist())
        else:
            assert n == 0, (what, tag, "transcript_len", n)
        assert tr[off + n] == 0, (what, tag, "terminator")


def _check_tiling(out, tr, what):
    """in input order, the transcript_off / transcript_len + 1 ranges tile [0, used) exactly"""
    off, n = out["transcript_off"].astype(np.int64), out["transcript_len"].astype(np.int64)
    assert (n >= 0).all(), what
    ends = off + n + 1
    assert off[0] == 0 and np.array_equal(off[1:], ends[:-1]) and ends[-1] == len(tr), what


@pytest.mark.parametrize("rows", ["0", "1"])
def test_corpus_equals_the_oracle_in_every_mode(ctx, c, ref, rows, monkeypatch):
    monkeypatch.setenv("DMND_SWEEP_ROWS", rows)
    index = np.arange(len(c.recs))
    items = _upload(ctx, c, index)
    assert int((items["cbs_off"] <= -2).sum()) >= 100 and int((items["cbs_off"] >= 0).sum()) >= 100      # own matrices, biases
    what = "rows " + rows
    score, _ = ctx.banded_swipe(items, hip.SWIPE_SCORE)
    coords, _ = ctx.banded_swipe(items, hip.SWIPE_COORDS)
    out, tr = ctx.banded_swipe(items, hip.SWIPE_TRACEBACK)
    stats, _ = ctx.banded_swipe(items, hip.SWIPE_STATS, 510)
    for k, rec in enumerate(c.recs):
        o, _, st = ref[k]
        tag = rec["tag"]
        assert score[k]["score"] == o["score"], (what, tag, "score-only score", int(score[k]["score"]), o["score"])
        assert coords[k]["score"] == o["score"], (what, tag, "coordinate-mode score", int(coords[k]["score"]), o["score"])
        assert stats[k]["score"] == st["score"], (what, tag, "statistics score", int(stats[k]["score"]), st["score"])
        if o["score"] > 0:
            assert (coords[k]["q_end"], coords[k]["s_end"]) == (o["q_end"], o["s_end"]), (what, tag, "end cell", coords[k], o)
            for key in STAT_KEYS:
                assert stats[k][key] == st[key], (what, tag, "statistics " + key, int(stats[k][key]), st[key])
    _check_traceback(c, ref, index, out, tr, what)
    _check_tiling(out, tr, what)
    ctx.upload_matrices(np.zeros((0, 32, 32), np.int8))


@pytest.mark.parametrize("rows", ["0", "1"])
def test_shuffled_order_and_exact_arena(ctx, c, ref, rows, monkeypatch):
    """Other items share a wavefront and a launch; the arena holds exactly the sum of query_len + target_len + 2 bytes, without
    the binding's 16 spare ones"""
    monkeypatch.setenv("DMND_SWEEP_ROWS", rows)
    index = c.shuffled
    items = _upload(ctx, c, index)
    out, tr = ctx.banded_swipe(items, hip.SWIPE_TRACEBACK)
    _check_traceback(c, ref, index, out, tr, "shuffled, rows " + rows)
    _check_tiling(out, tr, "shuffled, rows " + rows)
    cap = int((items["query_len"].astype(np.int64) + items["target_len"] + 2).sum())
    exact, etr = ctx.banded_swipe(items, hip.SWIPE_TRACEBACK, transcript_cap=cap)
    assert np.array_equal(exact, out) and np.array_equal(etr, tr)
    ctx.upload_matrices(np.zeros((0, 32, 32), np.int8))


@pytest.fixture(scope="module", params=ss.TRACEBACK, ids=ss.scheme_id)
def scheme_ctx(request):
    """(corpus of the scheme, its oracle, a context on the scheme's params)"""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    sc = tc.corpus(request.param)
    x = hip.Context(params=sc.params)
    yield sc, tc.oracle(sc), x
    x.close()


@pytest.mark.parametrize("rows", ["0", "1"])
def test_scheme_corpus_equals_the_oracle_in_every_mode(scheme_ctx, rows, monkeypatch):
    """test_corpus_equals_the_oracle_in_every_mode on the corpus of another scoring system"""
    sc, sref, x = scheme_ctx
    assert sc.scheme is not None and (x.params.gap_open, x.params.gap_extend) == (sc.gap_open, sc.gap_extend) != (tc.GAP_OPEN, tc.GAP_EXTEND)
    test_corpus_equals_the_oracle_in_every_mode(x, sc, sref, rows, monkeypatch)


def test_host_call_shape(ctx, c, ref):
    """dmnd_banded_swipe_host, one query and its target: up to six cases of every family and variant, spread over the family (the
    short and the long gaps and runs, narrow and wide bands)"""
    groups = {}
    for k, rec in enumerate(c.recs):
        groups.setdefault((rec["info"]["family"], rec["info"]["variant"]), []).append(k)
    assert len(groups) == 12
    n = 0
    for key, idx in sorted(groups.items()):
        for k in idx[::max(1, len(idx) // 5)][:6]:
            rec = c.recs[k]
            t = rec["targets"][0]
            out, tr = ctx.banded_swipe_host(rec["query"], rec["cbs"], [(t["seq"], t["d_begin"], t["d_end"], t["matrix"])], hip.SWIPE_TRACEBACK)
            _check_traceback(c, ref, [k], out, tr, "host call shape")
            n += 1
    assert n >= 50


# ---- the extension stage --------------------------------------------------------------------------------------------------------

def _pairs(c):
    """(query, target) of the gap, between and adjacent cases, each once"""
    seen, out = set(), []
    for rec in c.recs:
        i = rec["info"]
        if i["family"] in ("gap", "between", "adjacent") and i["variant"] == "plain":
            key = rec["tag"].rsplit("/", 1)[0]
            if key not in seen:
                seen.add(key)
                out.append((key, rec["query"], rec["targets"][0]["seq"]))
    return out


def _block(seqs):
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return np.concatenate(seqs).astype(np.int8), off


def _search(c, qd, ql, td, tl, device, monkeypatch):
    if device:
        monkeypatch.delenv("DMND_EXTEND_DEVICE", raising=False)
    else:
        monkeypatch.setenv("DMND_EXTEND_DEVICE", "0")
    params = hip.default_params()
    params.db_letters = float(tl[-1] - tl[0] - (len(tl) - 1))
    x = hip.Context(params=params)
    try:
        x.upload_block(hip.QUERY, qd, ql)
        x.upload_block(hip.TARGET, td, tl)
        sp, gf = hip.seed_params_preset("default", params, threads=1)
        x.set_gapped_filter(gf)
        hits = x.seed_search(sp)
        m, tr = x.extend(qd, td, hits, threads=4, with_transcripts=True)
        return m.copy(), tr.copy(), x.extend_device_stats(), hits
    finally:
        x.close()


def _long_gaps(m, tr):
    """records with a gap run of 64 letters or more: (insertions, deletions)"""
    n = [0, 0]
    for r in m:
        h = r["hsp"]
        runs = tc.gap_runs(tr[int(h["transcript_off"]): int(h["transcript_off"]) + int(h["transcript_len"])])
        for op in (1, 2):
            n[op - 1] += any(o == op and length >= 64 for o, length, _ in runs)
    return tuple(n)


def _blocks(c):
    pairs = _pairs(c)
    assert len(pairs) == 2 * len(tc.GAPS) + 2 * len(tc.BETWEEN) + 2
    q, qoff = _block([p[1] for p in pairs])
    t, toff = _block([p[2] for p in pairs])
    return pairs, q, qoff, t, toff


def test_extension_stage_walks_the_same_long_gaps_on_both_halves(c, monkeypatch):
    """Query i against target i of the gap, between and adjacent pairs through seed_search (default preset) and extend with
    transcripts, on the device half and on the host path: the same records and bytes, transcripts that re-score to their records,
    and gap runs of 64 letters and more in both directions on either path"""
    pairs, q, qoff, t, toff = _blocks(c)
    qd, ql = workload.sequence_set(q, qoff)
    td, tl = workload.sequence_set(t, toff)
    mh, trh, dev_h, hits = _search(c, qd, ql, td, tl, False, monkeypatch)
    md, trd, dev, _ = _search(c, qd, ql, td, tl, True, monkeypatch)
    assert dev_h["queries"] == 0 and dev["queries"] > 0 and dev["records"] > 0, "the call did not take the device half"
    assert len(md) == len(mh) >= len(pairs)
    for name in md.dtype.names:
        if name != "hsp":
            assert np.array_equal(md[name], mh[name]), name
    for name in md["hsp"].dtype.names:
        if name != "transcript_off":
            assert np.array_equal(md["hsp"][name], mh["hsp"][name]), name
    cbs = hip.extend_plan(c.params, qd, ql, td, tl, np.zeros(0, hip.SEED_HIT_DTYPE))[0]
    for a, b in zip(md, mh):
        tag = pairs[int(a["query"])][0] if a["query"] == a["target"] else "%d x %d" % (a["query"], a["target"])
        n = int(a["hsp"]["transcript_len"]) + 1
        oa, ob = int(a["hsp"]["transcript_off"]), int(b["hsp"]["transcript_off"])
        assert np.array_equal(trd[oa: oa + n], trh[ob: ob + n]), tag
        qi, ti = int(a["query"]), int(a["target"])
        qs, ts = qd[ql[qi]: ql[qi + 1] - 1], td[tl[ti]: tl[ti + 1] - 1]
        got = _rescore(qs, cbs[ql[qi]: ql[qi + 1] - 1], ts, a["hsp"], trd, c.M)
        assert got == (a["hsp"]["score"], a["hsp"]["q_end"], a["hsp"]["s_end"]), (tag, got, a["hsp"])
    long_h, long_d = _long_gaps(mh, trh), _long_gaps(md, trd)
    print("records with a gap run of 64 letters or more (insertions, deletions): host form %s, device half %s" % (long_h, long_d))
    assert long_h[0] > 0 and long_h[1] > 0 and long_d == long_h


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/diamond missing")
def test_cli_prints_the_reference_binarys_transcripts_of_the_long_gaps(c, tmp_path):
    """the same sequences as FASTA files through the CLI and the reference binary: cigar, btop and the gapped sequences"""
    pairs, q, qoff, t, toff = _blocks(c)
    synth.write_fasta(str(tmp_path / "q.faa"), "q", q, qoff)
    synth.write_fasta(str(tmp_path / "db.faa"), "t", t, toff)
    assert subprocess.run([REF, "makedb", "--in", str(tmp_path / "db.faa"), "-d", str(tmp_path / "db")], capture_output=True).returncode == 0
    common = ["blastp", "--algo", "0", "--masking", "0", "--motif-masking", "0", "-q", str(tmp_path / "q.faa"), "-d", str(tmp_path / "db.dmnd"),
              "-f", "6", "qseqid", "sseqid", "btop", "cigar", "qseq_gapped", "sseq_gapped"]
    r = subprocess.run([REF] + common + ["-o", str(tmp_path / "ref.out"), "-p", "4"], capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-1000:]
    h = subprocess.run([CLI] + common + ["-o", str(tmp_path / "hip.out")], capture_output=True, text=True, timeout=200)
    assert h.returncode == 0, h.stderr[-1500:]
    want = open(str(tmp_path / "ref.out"), "rb").read()
    got = open(str(tmp_path / "hip.out"), "rb").read()
    assert len(want.splitlines()) >= len(pairs) and got == want
    cigars = [l.split(b"\t")[3] for l in got.splitlines()]
    assert sum(any(int(n) >= 64 for n in re.findall(rb"(\d+)I", x)) for x in cigars) >= 5 and sum(any(int(n) >= 64 for n in re.findall(rb"(\d+)D", x)) for x in cigars) >= 5
