"""The traceback corpus (tests/traceback_cases.py) without a GPU. From the oracle alone: every family has the property the device
test (test_gpu_traceback_edges.py) relies on -- gaps of exactly G letters, runs of exactly N columns ended at the origin, by score
and at a running score of exactly 0, two gaps with no column between, a saturating score, every band class -- so a generator that
stops producing an edge fails here and not silently there. Then the corpus through the CPU emulators (the sweeps' trace layouts of
every class they reach and the serial walk traceback_walk of swipe_core.h): the oracle's numbers and transcript bytes."""
import numpy as np
import pytest

import emu_py as emu
import oracle_py as orc
import scoring_schemes as ss
import traceback_cases as tc

KEYS = "score q_begin q_end s_begin s_end length identities mismatches positives gap_openings gaps transcript_len".split()
STAT_KEYS = "score q_begin q_end s_begin s_end length identities mismatches gap_openings gaps".split()
INS, DEL = 1, 2


@pytest.fixture(scope="module")
def c():
    return tc.corpus()


@pytest.fixture(scope="module")
def ref(c):
    return tc.oracle(c)


def _of(c, ref, **want):
    idx = c.select(**want)
    assert idx, want
    return [(c.recs[k], ref[k][0], ref[k][1]) for k in idx]


# the launch classes as swipe_core.h's band_class / band_class_rows class a band, restated
def _class(width):
    P = 1
    while 128 * P < width:
        P *= 2
    return P


def _class_rows(width):
    return 3 if width <= 96 else 1 if width <= 128 else 5 if width <= 160 else _class(width)


def test_corpus_size_and_bands(c):
    assert 300 <= len(c.recs) <= 900 and c.cells() < 10 ** 8, (len(c.recs), c.cells())
    assert sorted(c.shuffled.tolist()) == list(range(len(c.recs)))
    assert len({r["tag"] for r in c.recs}) == len(c.recs)
    for r in c.recs:
        t = r["targets"][0]
        assert -(len(t["seq"]) - 1) <= t["d_begin"] < t["d_end"] <= len(r["query"]), r["tag"]          # inside the matrix's diagonals
        if "lo" in r["info"]:
            assert t["d_begin"] <= r["info"]["lo"] and r["info"]["hi"] <= t["d_end"], r["tag"]
        assert r["cbs"] is None or (t["matrix"] is None and len(r["cbs"]) == len(r["query"]))
        for s in (r["query"], t["seq"]):
            assert set(np.unique(s.view(np.uint8) & 31).tolist()) <= set(range(25)), r["tag"]


def test_gaps_of_exactly_g_letters(c, ref):
    seen = set()
    for rec, o, tr in _of(c, ref, family="gap") + _of(c, ref, family="wide", kind="gap"):
        G, direction = rec["info"]["G"], rec["info"]["dir"]
        assert (o["gap_openings"], o["gaps"]) == (1, G), (rec["tag"], o)
        (op, n, _), = tc.gap_runs(tr)
        assert (op, n) == (INS if direction == "ins" else DEL, G), rec["tag"]
        gap_bytes = [int(b) for b in tr if int(b) >> 6 == op]
        if direction == "ins":
            assert len(gap_bytes) == -(-G // 63) and sum(b & 63 for b in gap_bytes) == G and all(0 < b & 63 <= 63 for b in gap_bytes), rec["tag"]
        else:
            assert len(gap_bytes) == G, rec["tag"]
        seen.add((G, direction, rec["info"]["variant"]))
    assert seen == {(G, d, v) for G in tc.GAPS for d in ("ins", "del") for v in ("plain", "bias", "own")}


def test_runs_of_exactly_n_columns_by_each_ender(c, ref):
    seen = set()
    for rec, o, tr in _of(c, ref, family="run"):
        N, form = rec["info"]["N"], rec["info"]["form"]
        begin = {"origin": 0, "score": 7, "zero": 5}[form]
        seen.add((N, form, rec["info"]["variant"]))
        if (N, form) == (1, "zero"):
            # no single column outscores the prefix's own W:W (+11, the matrix's largest entry): the optimum starts on that column and
            # not behind the prefix. The item stays in the corpus and is held to the oracle like every other; the shortest run behind
            # this prefix is N = 63
            assert o["score"] >= 11 and o["s_begin"] == 0, (rec["tag"], o)
            continue
        assert (o["length"], o["q_begin"], o["s_begin"], o["gaps"]) == (N, begin, begin, 0), (rec["tag"], o)
        assert (o["q_end"], o["s_end"]) == (begin + N, begin + N) and len(tr) == N, rec["tag"]
        if form == "zero":
            M, cbs, t = c.matrix_of(rec), rec["cbs"], rec["targets"][0]["seq"]
            sums = np.cumsum([int(M[t[k] & 31, rec["query"][k] & 31]) + (int(cbs[k]) if cbs is not None else 0) for k in range(5)])
            assert sums[-1] == 0 and sums[0] > 0, (rec["tag"], sums)          # back at exactly 0 after a positive start
        seen.add((N, form, rec["info"]["variant"]))
    assert seen == {(N, f, v) for N in tc.RUNS for f in ("origin", "score", "zero") for v in ("plain", "bias", "own")}


def test_runs_between_gaps_and_adjacent_gaps(c, ref):
    for rec, o, tr in _of(c, ref, family="between"):
        r, order = rec["info"]["r"], rec["info"]["order"]
        runs = tc.gap_runs(tr)
        want = [(INS, 5, r), (DEL, 5, r)] if order == "ID" else [(DEL, 5, r), (INS, 5, r)]
        assert runs == want and o["length"] == 3 * r + 10 and o["q_begin"] == 0, (rec["tag"], runs, o)
    orders = set()
    for rec, o, tr in _of(c, ref, family="adjacent") + _of(c, ref, family="wide", kind="adjacent"):
        runs = tc.gap_runs(tr)
        assert (o["gap_openings"], o["gaps"]) == (2, 2 * tc.ADJ_GAP), (rec["tag"], o)
        assert len(runs) == 2 and {runs[0][0], runs[1][0]} == {INS, DEL} and runs[0][1] == runs[1][1] == tc.ADJ_GAP, (rec["tag"], runs)
        assert runs[1][2] == 0, (rec["tag"], runs)                                # no match column between the two runs
        orders.add((rec["info"]["family"], runs[0][0]))
    # (the walk meets the insertion first from the end whichever sequence holds the W: deletion then insertion in both pairs)
    assert orders == {("adjacent", DEL), ("wide", DEL)}, orders


def test_letters_saturation_and_zero_scores(c, ref):
    for rec, o, tr in _of(c, ref, family="letters"):
        subs = {int(b) & 63 for b in tr if int(b) >> 6 == 3}
        assert {20, 21, 22, 23, 24} <= subs, (rec["tag"], sorted(subs))
        assert o["positives"] >= o["identities"] + 5 and o["mismatches"] >= 15, (rec["tag"], o)
        t = rec["targets"][0]["seq"]
        assert (rec["query"] < 0).sum() >= 5 and (t < 0).sum() >= 5
        if rec["info"]["kind"] == "deletion":
            dels = [int(b) & 63 for b in tr if int(b) >> 6 == DEL]
            assert dels == [20, 21, 22, 23, 24, 5, 20, 21], (rec["tag"], dels)
    sat = _of(c, ref, family="sat")
    assert len(sat) == 2
    for rec, o, tr in sat:
        assert o["score"] >= 32767 and (o["gap_openings"], o["gaps"]) == (1, tc.SAT_GAP), (rec["tag"], o)
    zeros = _of(c, ref, family="zero", kind="WxD")
    ones = _of(c, ref, family="zero", kind="1x1")
    assert len(zeros) >= 20 and len(ones) >= 20
    assert all(o["score"] == 0 for _, o, _ in zeros)
    assert all(o["score"] > 0 and o["length"] == 1 and len(r["query"]) == 1 for r, o, _ in ones)
    # ... and they lie between the long items
    fam = [r["info"]["family"] for r in c.recs]
    assert all(fam[k - 1] != "zero" and fam[k + 1] != "zero" for k in range(1, len(fam) - 1) if fam[k] == "zero")


def test_every_band_class_per_family(c):
    counts = {}
    for r in c.recs:
        w = c.width(r)
        key = (r["info"]["family"], r["info"]["variant"])
        for rows, P in ((0, _class(w)), (1, _class_rows(w))):
            counts.setdefault(key, {}).setdefault((rows, P), 0)
            counts[key][(rows, P)] += 1
        # the class the case was built for
        assert r["info"]["class"] == (tc.width_class(w) or w), r["tag"]
    print({"%s/%s" % k: {"rows %d: P %d" % rp: n for rp, n in sorted(v.items())} for k, v in sorted(counts.items())})
    packed = {(0, 1), (0, 2), (0, 4), (1, 3), (1, 1), (1, 5), (1, 2), (1, 4)}
    for key in (("gap", "plain"), ("gap", "bias"), ("gap", "own"), ("run", "plain"), ("run", "bias"), ("run", "own"), ("between", "plain"),
                ("adjacent", "plain"), ("letters", "plain")):
        assert set(counts[key]) == packed, (key, counts[key])
    assert {P for _, P in counts[("wide", "plain")]} == {8, 16, 32, 64}
    for band, P in zip(tc.WIDE_BANDS, (8, 16, 32, 64)):
        got = [r["info"]["kind"] for r in c.recs if r["info"]["family"] == "wide" and c.width(r) == band]
        assert sorted(got) == ["adjacent", "gap"] and _class(band) == P
    assert tc.WIDE_BANDS[-1] > 4096                                               # several wavefronts per item
    assert {_class_rows(c.width(r)) for r in c.recs if r["info"]["family"] == "sat"} == {3, 1}
    # a long gap in every class that is wide enough for one
    for direction in ("ins", "del"):
        for width in (96, 128, 160, 256, 512):
            G = max(r["info"]["G"] for r in c.recs if r["info"]["family"] == "gap" and r["info"]["dir"] == direction and r["info"]["class"] == width)
            assert G == {96: 65, 128: 65, 160: 129, 256: 200, 512: 200}[width]


# ---- the emulators ---------------------------------------------------------------------------------------------------------------

def _same(rec, e, etr, o, otr, what):
    assert e["status"] == 0 and e["score"] == o["score"], (rec["tag"], what, e, o)
    if o["score"] > 0:
        for k in KEYS:
            assert e[k] == o[k], (rec["tag"], what, k, e, o)
        assert np.array_equal(etr, otr), (rec["tag"], what)


def test_32_bit_lanes_and_statistics_equal_the_oracle(c, ref):
    """emu.banded_swipe: the 32-bit kernels' lane code, trace layout and the serial walk in the item's class and in every wider
    one the emulator has (P <= 8); emu.swipe_stats (P <= 4)"""
    n = {1: 0, 2: 0, 4: 0, 8: 0}
    for rec, (o, otr, st) in zip(c.recs, ref):
        t = rec["targets"][0]
        P0 = _class(c.width(rec))
        if o["score"] >= 32767 and c.width(rec) > 96:
            continue                                                              # (one of the two saturating items is enough here)
        long_item = len(rec["query"]) > 1000
        for P in (1, 2, 4, 8):
            if P < P0 or (long_item and P != P0):
                continue
            rc, e, etr = emu.banded_swipe(rec["query"], rec["cbs"], t["seq"], t["d_begin"], t["d_end"], c.matrix_of(rec), c.gap_open, c.gap_extend, 2, P)
            assert rc == 0, rec["tag"]
            _same(rec, e, etr, o, otr, "32-bit class %d" % P)
            n[P] += 1
        if P0 <= 4:
            rc, e = emu.swipe_stats(rec["query"], rec["cbs"], t["seq"], t["d_begin"], t["d_end"], c.matrix_of(rec), c.gap_open, c.gap_extend)
            assert rc == 0 and e["score"] == st["score"], rec["tag"]
            if st["score"] > 0:
                for k in STAT_KEYS:
                    assert e[k] == st[k], (rec["tag"], k, e, st)
    assert all(v >= 100 for v in n.values()), n


def test_packed_sweeps_equal_the_oracle_in_every_class(c, ref):
    """emu.banded_swipe16: the packed sweeps' trace layouts (classes 1, 2, 4 and the row classes 3, 5 with their 15-byte records) and
    the serial walk; items of neighbouring band widths share a wavefront, an item with a matrix of its own is paired with itself"""
    order = sorted(range(len(c.recs)), key=lambda k: (c.width(c.recs[k]), k))
    plain = [k for k in order if c.recs[k]["targets"][0]["matrix"] is None and c.width(c.recs[k]) <= 512 and ref[k][0]["score"] < 32767]
    own = [k for k in order if c.recs[k]["targets"][0]["matrix"] is not None]
    pairs = [(plain[k], plain[min(k + 1, len(plain) - 1)]) for k in range(0, len(plain), 2)] + [(k, k) for k in own]
    n = {1: 0, 2: 0, 3: 0, 4: 0, 5: 0}

    def item(k):
        r = c.recs[k]
        t = r["targets"][0]
        return {"query": r["query"], "cbs": r["cbs"], "target": t["seq"], "d_begin": t["d_begin"], "d_end": t["d_end"]}

    for ka, kb in pairs:
        w = max(c.width(c.recs[ka]), c.width(c.recs[kb]))
        classes = [P for P in (1, 2, 4) if 128 * P >= w] + ([3] if w <= 96 else []) + ([5] if w <= 160 else [])
        for P in classes:
            rc, (ea, tra), (eb, trb) = emu.banded_swipe16(item(ka), item(kb), c.matrix_of(c.recs[ka]), c.gap_open, c.gap_extend, True, P)
            assert rc == 0, (c.recs[ka]["tag"], P)
            _same(c.recs[ka], ea, tra, ref[ka][0], ref[ka][1], "packed class %d" % P)
            _same(c.recs[kb], eb, trb, ref[kb][0], ref[kb][1], "packed class %d" % P)
            n[P] += 1
    assert all(v >= 50 for v in n.values()), n
    # the saturating item reports 32767 and leaves its partner alone
    sat = c.select(family="sat")[0]
    rc, (ea, _), (eb, trb) = emu.banded_swipe16(item(sat), item(plain[0]), c.M, c.gap_open, c.gap_extend, True, 0)
    assert rc == 0 and ea["score"] == 32767
    _same(c.recs[plain[0]], eb, trb, ref[plain[0]][0], ref[plain[0]][1], "next to a saturating item")


# ---- the corpus under other scoring systems ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=ss.TRACEBACK, ids=ss.scheme_id)
def sc(request):
    return tc.corpus(request.param)


@pytest.fixture(scope="module")
def sref(sc):
    return tc.oracle(sc)


def test_scheme_corpus_bands_and_classes(sc):
    assert sc is not tc.corpus() and (sc.params.gap_open, sc.params.gap_extend) == sc.scheme[1:]
    assert np.array_equal(sc.M, ss.matrix(sc.scheme[0]))
    test_corpus_size_and_bands(sc)
    test_every_band_class_per_family(sc)
    x, y = sc.low_pair
    assert int(sc.M[x, y]) == int(sc.M[:20, :20].min()) and -int(sc.M[x, y]) > 2 * sc.gap_extend
    assert sc.adj_gap * (-int(sc.M[x, y])) >= 2 * (sc.gap_open + sc.adj_gap * sc.gap_extend) + sc.gap_open, sc.adj_gap       # two gaps win by a gap open and more


def test_scheme_gaps_of_exactly_g_letters(sc, sref):
    """one gap of exactly G letters although it costs up to go + 200 ge (611 under PAM250 11/3): both flanks outscore it"""
    test_gaps_of_exactly_g_letters(sc, sref)
    cost = sc.gap_open + 200 * sc.gap_extend
    for rec, o, _ in _of(sc, sref, family="gap", G=200, variant="plain"):
        flank = (len(rec["query"]) + len(rec["targets"][0]["seq"]) - 200) // 4
        assert o["score"] >= 0.6 * cost and o["identities"] == 2 * flank, (rec["tag"], o, cost)


def test_scheme_runs_of_exactly_n_columns_by_each_ender(sc, sref):
    assert sc.zero_prefix is not None and 2 <= len(sc.zero_prefix) <= 5
    first = int(sc.M[sc.zero_prefix[0][1], sc.zero_prefix[0][0]])
    assert first == int(sc.M[tc.W, tc.W]) == int(sc.M[:20, :20].max())
    seen = set()
    for rec, o, tr in _of(sc, sref, family="run"):
        N, form = rec["info"]["N"], rec["info"]["form"]
        begin = {"origin": 0, "score": 7, "zero": len(sc.zero_prefix)}[form]
        seen.add((N, form, rec["info"]["variant"]))
        if (N, form) == (1, "zero"):
            assert o["score"] >= first and o["s_begin"] == 0, (rec["tag"], o)          # (as under BLOSUM62: no column outscores W:W)
            continue
        assert (o["length"], o["q_begin"], o["s_begin"], o["gaps"]) == (N, begin, begin, 0), (rec["tag"], o)
        assert (o["q_end"], o["s_end"]) == (begin + N, begin + N) and len(tr) == N, rec["tag"]
        M, t = sc.matrix_of(rec), rec["targets"][0]["seq"]
        if form == "zero":
            assert rec["cbs"] is None or not rec["cbs"][:begin].any()
            sums = np.cumsum([int(M[t[k] & 31, rec["query"][k] & 31]) for k in range(begin)])
            assert sums[-1] == 0 and (sums[:-1] > 0).all(), (rec["tag"], sums)
        if form == "score":
            assert all(int(M[t[k], rec["query"][k]]) < 0 for k in range(7)), rec["tag"]
    assert seen == {(N, f, v) for N in tc.RUNS for f in ("origin", "score", "zero") for v in ("plain", "bias", "own")}


def test_scheme_runs_between_gaps_and_adjacent_gaps(sc, sref):
    for rec, o, tr in _of(sc, sref, family="between"):
        r, order = rec["info"]["r"], rec["info"]["order"]
        runs = tc.gap_runs(tr)
        want = [(INS, 5, r), (DEL, 5, r)] if order == "ID" else [(DEL, 5, r), (INS, 5, r)]
        assert runs == want and o["length"] == 3 * r + 10 and o["q_begin"] == 0, (rec["tag"], runs, o)
    n = 0
    for rec, o, tr in _of(sc, sref, family="adjacent") + _of(sc, sref, family="wide", kind="adjacent"):
        runs = tc.gap_runs(tr)
        assert (o["gap_openings"], o["gaps"]) == (2, 2 * sc.adj_gap), (rec["tag"], o)
        assert len(runs) == 2 and {runs[0][0], runs[1][0]} == {INS, DEL} and runs[0][1] == runs[1][1] == sc.adj_gap, (rec["tag"], runs)
        assert runs[1][2] == 0, (rec["tag"], runs)
        n += 1
    assert n >= 2 * 3 + 4


def test_scheme_letters_saturation_and_zero_scores(sc, sref):
    assert len(sc.letter_columns) >= 4 and (sc.scheme != ("pam30", 5, 2) or sc.letter_columns == (20, 21, 22, 23))
    for rec, o, tr in _of(sc, sref, family="letters"):
        subs = {int(b) & 63 for b in tr if int(b) >> 6 == 3}
        assert set(sc.letter_columns) <= subs, (rec["tag"], sorted(subs))
        assert o["positives"] >= o["identities"] + 5 and o["mismatches"] >= 12, (rec["tag"], o)
        t = rec["targets"][0]["seq"]
        assert (rec["query"] < 0).sum() >= 5 and (t < 0).sum() >= 5
        if rec["info"]["kind"] == "deletion":
            dels = [int(b) & 63 for b in tr if int(b) >> 6 == DEL]
            want = [20, 21, 22, 23, 24, 5, 20, 21]
            at = [k for k in range(len(dels) - 7) if dels[k: k + 8] == want]
            assert len(at) == 1, (rec["tag"], dels)
            # (a letter that cannot stand in a column is deleted against an inserted query letter)
            assert all(d not in sc.letter_columns and d >= 20 for d in dels[:at[0]] + dels[at[0] + 8:]), (rec["tag"], dels)
    sat = _of(sc, sref, family="sat")
    assert len(sat) == 2
    for rec, o, tr in sat:
        assert o["score"] >= 32767 and (o["gap_openings"], o["gaps"]) == (1, tc.SAT_GAP), (rec["tag"], o)
    zeros, ones = _of(sc, sref, family="zero", kind="WxD"), _of(sc, sref, family="zero", kind="1x1")
    assert len(zeros) >= 20 and len(ones) >= 20
    assert all(o["score"] == 0 for _, o, _ in zeros)
    assert all(o["score"] > 0 and o["length"] == 1 and len(r["query"]) == 1 for r, o, _ in ones)


def test_scheme_corpus_through_the_emulators(sc, sref):
    """the serial walk of swipe_core.h keeps its own gap accounting too: gaps of up to 200 letters under gap extend 2 and 3"""
    test_32_bit_lanes_and_statistics_equal_the_oracle(sc, sref)
    test_packed_sweeps_equal_the_oracle_in_every_class(sc, sref)
