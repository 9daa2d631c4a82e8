"""-m gpu: --ext full and the final pass of --global-ranking through the device half of the extension stage (csrc/plan_kernels.hip
plan_full_kernel, csrc/extend_kernels.hip ext_mark_kernel with the full-matrix DP size; the arithmetic in csrc/plan_core.h).
Every case runs the same call on the host path (DMND_EXTEND_DEVICE=0) and on the device in Extension::Mode::FULL and requires the same
record bytes, and that the device half extended queries at all (extend_device_stats()["queries"] > 0).
 * families (300 x 10, 300 queries) in three seed modes under -k 25, -k 1 and --top 10: at most 2 % of the queries handed back; no
   pair of the data outgrows 4096 diagonals or 10^6 cells, so the cap tests the code;
 * pairs at the band-class edges: query + target lengths = band + 1 for band 96 .. 4096, short query / long target and the reverse, row
   classes of the sweeps forced on and off: none handed back. Band 4097 and 1000 x 1001 letters go back to the host as whole queries
   (the device half does not count them among its queries at all: `queries` excludes what ext_mark_kernel refuses), 1000 x 1000 stays;
 * the shortest sequences the seed stage hits; several ranking chunks; the trace budget; transcripts; the HSP filters under -k and
   --top; six contexts with and without filters; the guard, fresh and after extend_reserve; the planner's own output;
 * the final pass of the global ranking: a table of N = 5 / 100 over two blocks (rank_targets_device + rank_update), the ranked
   targets as one block and one hit per entry as the CLI builds them; N = EXT_MAX_CHUNK + 1 stays on the host path."""
import numpy as np
import pytest
import torch

import translated_sets as ts
from diamond_amd import hip, synth, workload

pytestmark = pytest.mark.gpu
EXT_MAX_CHUNK = 1024                  # csrc/extend_core.h
MAX_SWIPE_DP = 1000000                # config.max_swipe_dp

FILTERS = {       # (min_id, query_cover, subject_cover, min_bit_score), approx_id
    "id": ((61.37, 0, 0, 0), 0),
    "covers": ((0, 80.13, 70.29, 0), 0),
    "approx_id": ((0, 0, 0, 0), 45.77),
    "min_score": ((0, 0, 0, 99.73), 0),
}
_cache = {}


def _pack(seqs):
    return np.concatenate(seqs).astype(np.int8), np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)


def _substituted(rng, s, n):
    t = s.copy()
    pos = rng.choice(len(s), n, replace=False)
    t[pos] = (t[pos] + rng.integers(1, 20, n)) % 20
    return t


def _families():
    if "families" not in _cache:
        _cache["families"] = synth.generate(300, members=10, queries=300, seed=5, sub=(0.05, 0.6), qsub=(0.05, 0.5))
    return _cache["families"]


def _chunks():
    """120 queries against 6 families of 200: two ranking chunks of 128 per query"""
    if "chunks" not in _cache:
        _cache["chunks"] = synth.generate(6, members=200, queries=120, seed=7, sub=(0.05, 0.6), qsub=(0.05, 0.5))
    return _cache["chunks"]


def _partial():
    """the block of partial targets of tests/test_gpu_filters_device.py, rebuilt"""
    if "partial" not in _cache:
        rng = np.random.default_rng(17)
        qs, tgts = [], []
        for qi in range(60):
            s = rng.integers(0, 20, 300).astype(np.int8)
            qs.append(s)
            for f in np.linspace(0.5, 1.0, 8):
                n = int(round(300 * f))
                a = int(rng.integers(0, 300 - n + 1))
                tgts.append(_substituted(rng, s[a:a + n], int(0.15 * n)))
            for f in np.linspace(0.5, 1.0, 8):
                flank = int(round(300 / f)) - 300
                t = _substituted(rng, s, 15 if f < 0.7 else 75)
                left = flank // 2
                tgts.append(np.concatenate([rng.integers(0, 20, left), t, rng.integers(0, 20, flank - left)]).astype(np.int8))
        _cache["partial"] = _pack(tgts) + _pack(qs)
    return _cache["partial"]


def _planted(rng, pairs, seg=40):
    """one (query, target) pair of random letters per (qlen, tlen), sharing `seg` identical letters at a random place of either"""
    qs, tgts = [], []
    for qlen, tlen in pairs:
        q, t = rng.integers(0, 20, qlen).astype(np.int8), rng.integers(0, 20, tlen).astype(np.int8)
        s = rng.integers(0, 20, seg).astype(np.int8)
        a, b = int(rng.integers(0, qlen - seg + 1)), int(rng.integers(0, tlen - seg + 1))
        q[a:a + seg] = s
        t[b:b + seg] = s
        qs.append(q)
        tgts.append(t)
    return _pack(tgts) + _pack(qs)


def _extend(data, device, monkeypatch, mode="fast", k=25, top=None, filters=None, env=None, reserve=False, with_tr=False):
    """(records, transcripts, device statistics, stage statistics) of one search of the block pair in Mode::FULL"""
    db, doff, q, qoff = data
    monkeypatch.setenv("DMND_EXTEND_DEVICE", "1" if device else "0")
    for name in ("DMND_EXTEND_GUARD", "DMND_EXTEND_MAX_CHUNKS", "DMND_SWEEP_ROWS", "DMND_TRACE_ARENA_MB"):
        monkeypatch.delenv(name, raising=False)
    for name, v in (env or {}).items():
        monkeypatch.setenv(name, v)
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
        ctx.set_extension_mode(hip.EXT_FULL)
        ctx.set_max_target_seqs(k)
        ctx.set_top_percent(top)
        if filters:
            f, approx = FILTERS[filters]
            ctx.set_filters(*f)
            ctx.set_approx_id(approx)
        hits = ctx.seed_search(sp)
        m, tr = ctx.extend(qd, td, hits, threads=4, with_transcripts=with_tr)
        return m.copy(), (tr.copy() if with_tr else None), ctx.extend_device_stats(), ctx.extend_stats(), hits.copy(), tl
    finally:
        ctx.close()


def _device_equals_host(data, monkeypatch, **kw):
    host = _extend(data, False, monkeypatch, **{n: v for n, v in kw.items() if n not in ("env", "reserve")})
    dev = _extend(data, True, monkeypatch, **kw)
    print("--ext full", kw, "host records", len(host[0]), "device stats", dev[2])
    assert host[2]["queries"] == 0 and len(host[0]) > 0
    assert dev[2]["queries"] > 0, "no query was extended on the device"
    assert dev[0].tobytes() == host[0].tobytes()
    return dev


def _pairs_of_hits(hits, tl, ql_lens, tl_lens):
    """(query length, target length) of every (query, target) pair with a seed hit"""
    t = np.searchsorted(tl, hits["subject"], "right") - 1
    return ql_lens[hits["query"]].astype(np.int64), tl_lens[t].astype(np.int64)


@pytest.mark.parametrize("mode", ["fast", "default", "sensitive"])
@pytest.mark.parametrize("k,top", [(25, None), (1, None), (25, 10.0)], ids=["k25", "k1", "top10"])
def test_families_are_extended_over_the_full_matrix_on_the_device(mode, k, top, monkeypatch):
    assert torch.cuda.is_available()
    data = _families()
    m, _, ds, st, hits, tl = _device_equals_host(data, monkeypatch, mode=mode, k=k, top=top)
    # the data: no pair with a seed hit outgrows what the device half takes, so every hand-back is the code's own doing
    qlen, tlen = _pairs_of_hits(hits, tl, np.diff(data[3]), np.diff(data[1]))
    assert (qlen + tlen - 1).max() <= 4096 and (qlen * tlen).max() <= MAX_SWIPE_DP
    assert ds["queries_back_to_host"] <= ds["queries"] // 50
    assert 0 < ds["records"] <= len(m)
    print("lane use of the sweeps:", ds["band_diagonal_steps"] / max(1.0, ds["wavefront_diagonal_steps"]))


BANDS = (96, 97, 128, 129, 160, 161, 256, 257, 4096)
SHORT = 45


def _edges(short_query):
    key = "edges%d" % short_query
    if key not in _cache:
        pairs = [(SHORT, b + 1 - SHORT) if short_query else (b + 1 - SHORT, SHORT) for b in BANDS]
        _cache[key] = _planted(np.random.default_rng(71 + short_query), pairs)
    return _cache[key]


@pytest.mark.parametrize("rows", ["0", "1"], ids=["wavefront_classes", "row_classes"])
@pytest.mark.parametrize("short_query", [1, 0], ids=["short_query", "short_target"])
def test_band_class_edges_stay_on_the_device(short_query, rows, monkeypatch):
    """d_begin far below zero (short query, long target) or d_end far above it; every band width on either side of a class edge"""
    data = _edges(short_query)
    m, _, ds, st, hits, tl = _device_equals_host(data, monkeypatch, env={"DMND_SWEEP_ROWS": rows})
    qlen, tlen = _pairs_of_hits(hits, tl, np.diff(data[3]), np.diff(data[1]))
    assert set(BANDS) <= set((qlen + tlen - 1).tolist())               # the seed stage found every planted pair
    assert (qlen + tlen - 1).max() <= 4096
    assert ds["queries"] == len(np.unique(hits["query"])) and ds["queries_back_to_host"] == 0
    for i in range(len(BANDS)):
        assert ((m["query"] == i) & (m["target"] == i)).sum() == 1, BANDS[i]


@pytest.mark.parametrize("pair,on_device", [((46, 4052), False), ((4052, 46), False), ((1000, 1001), False), ((1001, 1000), False), ((1000, 1000), True)],
                         ids=["band4097", "band4097_long_query", "1000x1001", "1001x1000", "1000x1000"])
def test_what_outgrows_the_device_half_goes_back_as_a_whole_query(pair, on_device, monkeypatch):
    """beside an ordinary pair (query 0), so that the call is taken: query 1 is refused by ext_mark_kernel -- more than 4096 diagonals,
    or more cells than max_swipe_dp counted over the whole matrix -- or, at exactly 10^6 cells, stays"""
    data = _planted(np.random.default_rng(73), [(100, 120), pair])
    m, _, ds, st, hits, tl = _device_equals_host(data, monkeypatch)
    qlen, tlen = _pairs_of_hits(hits, tl, np.diff(data[3]), np.diff(data[1]))
    assert sorted(set(zip(hits["query"].tolist(), qlen.tolist(), tlen.tolist()))) == [(0, 100, 120), (1,) + pair]      # the two planted pairs and no other
    assert ds["queries"] == (2 if on_device else 1) and ds["queries_back_to_host"] == 0
    assert ds["items"] == ds["queries"]
    assert ((m["query"] == 1) & (m["target"] == 1)).sum() == 1


def test_the_shortest_sequences_the_seed_stage_hits(monkeypatch):
    """identical query and target of falling length, until the seed stage finds nothing: the shortest pair it still hits is extended on
    the device, over a matrix of a dozen letters either way"""
    rng = np.random.default_rng(79)
    seqs = [rng.integers(0, 20, n).astype(np.int8) for n in range(30, 7, -1)]
    data = _pack(seqs) + _pack(seqs)
    m, _, ds, st, hits, tl = _device_equals_host(data, monkeypatch)
    qlen, tlen = _pairs_of_hits(hits, tl, np.diff(data[3]), np.diff(data[1]))
    print("shortest pair with a seed hit:", int(qlen.min()), "x", int(tlen.min()))
    assert qlen.min() < 30 and ds["queries_back_to_host"] == 0 and ds["queries"] == len(np.unique(hits["query"]))


@pytest.mark.parametrize("k,top", [(25, None), (25, 10.0)], ids=["k25", "top10"])
def test_several_ranking_chunks(k, top, monkeypatch):
    m, _, ds, st, hits, tl = _device_equals_host(_chunks(), monkeypatch, mode="default", k=k, top=top)
    assert ds["queries_back_to_host"] <= ds["queries"] // 50
    assert ds["items"] > 128 * ds["queries"] // 2              # the queries swept more than one chunk's worth of targets


@pytest.mark.parametrize("env", [{"DMND_TRACE_ARENA_MB": "1"}, {"DMND_EXTEND_KEEP_TRACE": "0"}], ids=["arena_1mb", "keep_trace_off"])
def test_the_trace_budget(env, monkeypatch):
    """a budget the first iteration's trace rows do not fit: scores first, the survivors swept again with traceback"""
    m, _, ds, st, hits, tl = _device_equals_host(_families(), monkeypatch, env=env)
    assert ds["queries_back_to_host"] <= ds["queries"] // 50
    if "DMND_TRACE_ARENA_MB" in env:
        assert ds["round2_cells_swept_again"] > 0, "the rows fitted the budget: the case tests nothing"


def test_transcripts_equal_the_host_path(monkeypatch):
    host = _extend(_families(), False, monkeypatch, with_tr=True)
    dev = _extend(_families(), True, monkeypatch, with_tr=True)
    assert host[2]["queries"] == 0 and dev[2]["queries"] > 0 and dev[2]["records"] > 0
    a, b, tra, trb = dev[0], host[0], dev[1], host[1]
    assert len(a) == len(b) > 0
    for name in a.dtype.names:
        if name != "hsp":
            assert np.array_equal(a[name], b[name]), name
    for name in a["hsp"].dtype.names:
        if name != "transcript_off":
            assert np.array_equal(a["hsp"][name], b["hsp"][name]), name
    for x, y in zip(a, b):
        n = int(x["hsp"]["transcript_len"]) + 1
        ox, oy = int(x["hsp"]["transcript_off"]), int(y["hsp"]["transcript_off"])
        assert ox >= 0 and oy >= 0 and np.array_equal(tra[ox:ox + n], trb[oy:oy + n]), (int(x["query"]), int(x["target"]))
    assert len(tra) == len(trb)


@pytest.mark.parametrize("top", [None, 33.3], ids=["k25", "top33"])
@pytest.mark.parametrize("name", ["id", "covers", "approx_id", "min_score"])
def test_hsp_filters(name, top, monkeypatch):
    m, _, ds, st, hits, tl = _device_equals_host(_partial(), monkeypatch, filters=name, top=top)
    assert ds["queries_back_to_host"] <= ds["queries"] // 50
    if name == "covers":
        assert ds["records_filtered"] > 0


def test_layout_under_the_guard_fresh_and_reserved(monkeypatch):
    fresh = _device_equals_host(_families(), monkeypatch, env={"DMND_EXTEND_GUARD": "1"})
    res = _extend(_families(), True, monkeypatch, env={"DMND_EXTEND_GUARD": "1"}, reserve=True)
    assert res[2]["queries"] == fresh[2]["queries"] > 0 and res[2]["records"] == fresh[2]["records"] > 0
    assert res[0].tobytes() == fresh[0].tobytes()


def test_the_planner_gives_every_group_its_whole_matrix(monkeypatch):
    monkeypatch.delenv("DMND_EXTEND_DEVICE", raising=False)
    db, doff, q, qoff = _families()
    qd, ql = workload.sequence_set(q, qoff)
    td, tl = workload.sequence_set(db, doff)
    params = hip.default_params()
    params.db_letters = float(doff[-1])
    ctx = hip.Context(device=0, params=params)
    try:
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, td, tl)
        sp, gf = hip.seed_params_preset("fast", params, threads=1)
        hits = ctx.seed_search(sp)
        ctx.set_extension_mode(hip.EXT_FULL)
        rows, groups, info = ctx.extend_plan_device(hits)
    finally:
        ctx.close()
    assert info["planned"] and not info["unsorted"] and info["n_on_host"] == 0 and info["n_chain"] == 0 and info["n_chain_big"] == 0
    t = np.searchsorted(tl, hits["subject"], "right") - 1
    want = sorted(set(zip(hits["query"].tolist(), t.tolist())))
    assert len(want) > 300 and info["n_groups"] == info["n_bands"] == len(want) == len(rows) == len(groups)
    assert list(zip(groups["query"].tolist(), groups["target"].tolist())) == want
    assert (groups["n_bands"] == 1).all() and (groups["on_host"] == 0).all() and (groups["pass"] == 1).all()
    qlen, tlen = np.diff(qoff)[rows["query"]], np.diff(doff)[rows["target"]]
    assert list(zip(rows["query"].tolist(), rows["target"].tolist())) == want
    assert np.array_equal(rows["d_begin"], -(tlen - 1)) and np.array_equal(rows["d_end"], qlen)
    best = {}
    for qq, tt, s in zip(hits["query"].tolist(), t.tolist(), hits["score"].tolist()):
        best[(qq, tt)] = max(best.get((qq, tt), 0), s)
    assert rows["ungapped_score"].tolist() == [best[x] for x in want]


# ---- six contexts -------------------------------------------------------------------------------------------------------------------

def _constructed():
    """The read set of tests/translated_sets.py, and behind it reads that hold the head of a database protein on both strands: the coding string
    followed by its reverse complement reads the same on either strand -- frames 0 and 3 hold the protein --, and three copies one base
    apart followed by their reverse complement put it into all six frames."""
    if "set" not in _cache:
        db, doff, dna, off, kinds = ts.constructed_set()
        reads = [dna[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        rc = lambda x: (3 - x[::-1]).astype(np.int8)
        for k, i in enumerate((0, 4, 8, 12)):            # (the first 100 letters of four proteins of different families)
            assert doff[i + 1] - doff[i] >= 100
            s = ts._coding(db[doff[i]:doff[i] + 100], 500 + k)
            assert s.max() <= 3
            reads.append(np.concatenate([s, rc(s)]).astype(np.int8))
            fwd = np.concatenate([s, [1], s, [2], s]).astype(np.int8)
            reads.append(np.concatenate([fwd, rc(fwd)]).astype(np.int8))
            kinds = kinds + ["strands", "six"]
        dna = np.concatenate(reads).astype(np.int8)
        off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
        xd, xl = hip.translated_block(dna, off)
        td, tl = workload.sequence_set(db, doff)
        _cache["set"] = (db, doff, dna, off, kinds, xd, xl, td, tl)
    return _cache["set"]


def _translated_ctx(monkeypatch):
    db, doff, dna, off, kinds, xd, xl, td, tl = _constructed()
    params = hip.default_params()
    params.db_letters = float(doff[-1])
    ctx = hip.Context(params=params)
    ctx.upload_block(hip.TARGET, td, tl)
    ctx.upload_block(hip.QUERY, xd, xl)
    ctx.set_query_contexts(6)
    ctx.set_query_source_lengths(np.diff(off))
    sp, gf = hip.seed_params_preset("default", params, threads=4)
    sp.query_translated = 1
    ctx.set_gapped_filter(gf)
    ctx.set_extension_mode(hip.EXT_FULL)
    return ctx, ctx.seed_search(sp)


def _frames_per_pair(hits, tl):
    return {p: sorted({f for f, _ in v}) for p, v in ts.pairs_of(hits, tl).items()}


def test_six_contexts_with_and_without_filters(monkeypatch):
    """reads with hits in one frame and in two frames of one strand (tests/translated_sets.py), in two frames of opposite strands and in
    all six frames (_constructed)"""
    monkeypatch.setenv("DMND_EXTEND_GUARD", "1")
    db, doff, dna, off, kinds, xd, xl, td, tl = _constructed()
    ctx, hits = _translated_ctx(monkeypatch)
    try:
        frames = _frames_per_pair(hits, tl)
        n_frames = [len(v) for v in frames.values()]
        print("pairs by number of frames with a hit:", np.bincount(n_frames).tolist())
        assert 1 in n_frames
        assert any(len(v) == 2 and v[0] < 3 <= v[1] for v in frames.values()), "no pair with hits in two frames of opposite strands"
        assert any(len(v) == 2 and (v[1] < 3 or v[0] >= 3) for v in frames.values()), "no pair with hits in two frames of one strand"
        assert 6 in n_frames, "no pair with hits in all six frames"
        for k, top, filt in ((25, None, None), (1, None, None), (25, 10.0, None), (25, None, "covers"), (25, 10.0, "id")):
            ctx.set_max_target_seqs(k)
            ctx.set_top_percent(top)
            f, approx = FILTERS[filt] if filt else ((0, 0, 0, 0), 0)
            ctx.set_filters(*f)
            ctx.set_approx_id(approx)
            monkeypatch.delenv("DMND_EXTEND_DEVICE", raising=False)
            a, _ = ctx.extend(xd, td, hits, threads=4)
            plan, dev = ctx.extend_plan_stats(), ctx.extend_device_stats()
            assert plan["groups"] > 0 and dev["queries"] > dev["queries_back_to_host"] and dev["records"] > 0, (k, top, filt)
            monkeypatch.setenv("DMND_EXTEND_DEVICE", "0")
            b, _ = ctx.extend(xd, td, hits, threads=4)
            assert ctx.extend_device_stats()["queries"] == 0
            print((k, top, filt), "records", len(a), len(b), "device", dev)
            assert len(a) == len(b) > 100, (k, top, filt)
            for name in a.dtype.names:
                assert np.array_equal(a[name], b[name]), (k, top, filt, name)
            assert a.tobytes() == b.tobytes(), (k, top, filt)
    finally:
        ctx.close()


def test_six_contexts_plan_one_band_per_frame_with_a_hit(monkeypatch):
    monkeypatch.delenv("DMND_EXTEND_DEVICE", raising=False)
    db, doff, dna, off, kinds, xd, xl, td, tl = _constructed()
    ctx, hits = _translated_ctx(monkeypatch)
    try:
        rows, groups, info = ctx.extend_plan_device(hits)
    finally:
        ctx.close()
    assert info["planned"] and info["n_on_host"] == 0
    frames = _frames_per_pair(hits, tl)
    want_pairs = sorted(frames)
    assert list(zip((groups["query"] // 6).tolist(), groups["target"].tolist())) == want_pairs
    assert groups["n_bands"].tolist() == [len(frames[p]) for p in want_pairs]
    want_rows = [(r * 6 + f, t) for (r, t) in want_pairs for f in frames[(r, t)]]
    assert list(zip(rows["query"].tolist(), rows["target"].tolist())) == want_rows
    qlen = (np.diff(xl) - 1)[rows["query"]]
    tlen = np.diff(doff)[rows["target"]]
    assert np.array_equal(rows["d_begin"], -(tlen - 1)) and np.array_equal(rows["d_end"], qlen)
    # the score that travels into the record: context 0's best stage-1 score, 0 without a hit there
    pairs = ts.pairs_of(hits, tl)
    u0 = {p: max([int(hits["score"][k]) for f, k in v if f == 0] or [0]) for p, v in pairs.items()}
    assert rows["ungapped_score"].tolist() == [u0[(q // 6, t)] for q, t in want_rows]


# ---- the final pass of the global ranking -------------------------------------------------------------------------------------------

def _ranked_call(n, monkeypatch):
    """The table of the n best targets per query over two blocks of the families data, then what the CLI hands to dmnd_extend: the ranked
    targets as one block in database order, one seed hit per table entry (its score and context, at the target's first letter), sorted
    by (query, location)."""
    key = "ranked%d" % n
    if key in _cache:
        return _cache[key]
    db, doff, q, qoff = _families()
    nq, nt = len(qoff) - 1, len(doff) - 1
    qd, ql = workload.sequence_set(q, qoff)
    params = hip.default_params()
    params.db_letters = float(doff[-1])
    table = np.zeros(nq * n, hip.RANKED_DTYPE)
    half = nt // 2
    ctx = hip.Context(device=0, params=params)
    try:
        ctx.upload_block(hip.QUERY, qd, ql)
        sp, gf = hip.seed_params_preset("fast", params, threads=1)
        for t0, t1 in ((0, half), (half, nt)):
            td, tl = workload.sequence_set(db[doff[t0]:doff[t1]], doff[t0:t1 + 1] - doff[t0])
            ctx.upload_block(hip.TARGET, td, tl)
            ctx.seed_search(sp)
            hip.rank_update(table, n, ctx.rank_targets_device(None, n_keep=n, target_offset=t0))
    finally:
        ctx.close()
    entries = table[table["score"] > 0]
    ordinals = np.unique(entries["target"])
    rd, rl = workload.sequence_set(np.concatenate([db[doff[o]:doff[o + 1]] for o in ordinals]),
                                   np.concatenate([[0], np.cumsum(np.diff(doff)[ordinals])]).astype(np.int64))
    hits = np.zeros(len(entries), hip.SEED_HIT_DTYPE)
    hits["query"] = entries["query"] + entries["context"]
    hits["subject"] = rl[np.searchsorted(ordinals, entries["target"])]
    hits["score"] = entries["score"]
    hits = hits[np.lexsort((hits["subject"], hits["query"]))]
    per_query = np.bincount(entries["query"], minlength=nq)
    _cache[key] = (qd, ql, rd, rl, hits, per_query, params)
    return _cache[key]


def _extend_ranked(call, n, device, monkeypatch):
    qd, ql, rd, rl, hits, per_query, params = call
    monkeypatch.setenv("DMND_EXTEND_DEVICE", "1" if device else "0")
    ctx = hip.Context(device=0, params=params)
    try:
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, rd, rl)
        ctx.set_extension_mode(hip.EXT_FULL)
        ctx.set_global_ranking(n)
        m, _ = ctx.extend(qd, rd, hits, threads=4)
        return m.copy(), ctx.extend_device_stats()
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [5, 100, EXT_MAX_CHUNK + 1])
def test_the_final_pass_of_the_global_ranking(n, monkeypatch):
    call = _ranked_call(n, monkeypatch)
    per_query = call[5]
    assert per_query.max() <= n and (per_query.max() == n or n > 10), "the table is not cut at n anywhere"
    host, hs = _extend_ranked(call, n, False, monkeypatch)
    dev, ds = _extend_ranked(call, n, True, monkeypatch)
    print("-g", n, "entries", len(call[4]), "records", len(host), "device stats", ds)
    assert hs["queries"] == 0 and len(host) > 250
    assert dev.tobytes() == host.tobytes()
    if n <= EXT_MAX_CHUNK:
        assert ds["queries"] > 0 and ds["queries_back_to_host"] <= ds["queries"] // 50
    else:
        assert ds["queries"] == 0                          # a chunk the device half does not take: the whole call on the host path
