"""The gapped filter's edge cases (tests/gapped_cases.py) without a GPU: the lane emulator over gapped_core.h
(tests/emu/gapped_emu.cpp) equals the C oracle on every blastp case, and the case list has the properties the device test
(test_gpu_gapped_edges.py) relies on. Of gapped_core.h the kernels use hit_window, scan_range, DiagAln and bit_length32, so for
these the emulator speaks for the kernels; the per-cell arithmetic it runs (scan_diag, profile_score: the 255 cap, the bias on rows
below 20, the int8 clamp) is written a second time in gapped_kernels.hip (diag_step, the profile builder, scan_diags_profile), and
only the device test judges those lines. The properties are asserted from the numpy restatement of the reference's scan and from the
oracle alone, so a generator that stops producing an edge fails here and not silently there."""
import numpy as np
import pytest

import emu_py as emu
import gapped_cases as gc
import oracle_py as orc

BLASTP = ("blastp", "pam30")


@pytest.fixture(scope="module", params=BLASTP)
def c(request):
    return gc.corpus(request.param)


@pytest.fixture(scope="module")
def full():
    return gc.corpus("blastp")


@pytest.fixture(scope="module")
def tx():
    return gc.corpus("blastx")


def _scans(c, family, band):
    return {int(k): c.scan(int(k), band) for k in c.family(*family)}


def test_emulated_kernel_equals_oracle_on_every_blastp_case(c):
    p = emu.GfParams(diag_score=c.diag_score, gap_open=c.params.gap_open, gap_extend=c.params.gap_extend, window2=gc.WINDOW2, use_cbs=1, contexts=1)
    flags, scores = gc.expected(c)
    for k in range(len(c.hits)):
        q, b, t, hi, hj, _ = c.inputs(k)
        b1, b2 = len(q).bit_length(), len(t).bit_length()
        got = emu.gapped_filter_hit(p, c.M, q, b, t, hi, hj, c.cut1[b1, b2], c.cut2[b1, b2])
        assert got == (int(flags[k]), int(scores[k, 0]), int(scores[k, 1])), c.tags[k]


def test_cutoffs_and_diag_score(c, full):
    assert (full.diag_score, full.params.gap_open, full.params.gap_extend) == (20, 11, 1)
    # BLOSUM62: the tables test_oracle_gapped.py proves equal to the reference's
    assert np.array_equal(full.cut1, orc.cutoff_table2d(gc.EVALUE1)) and np.array_equal(full.cut2, orc.cutoff_table2d(gc.EVALUE2))
    other = gc.corpus("pam30")
    assert (other.diag_score, other.params.gap_open, other.params.gap_extend) == (21, 9, 1)
    m, M62 = other.M[:20, :20].astype(int), full.M[:20, :20].astype(int)
    assert m.max() - m.min() > M62.max() - M62.min()                      # a wider score range: the clamp under bias binds sooner
    assert (c.cut1[1:, 1:] <= c.cut2[1:, 1:]).all() and c.cut1[7, 7] < c.cut1[12, 7]


def test_every_hit_lies_inside_its_sequences(c, tx):
    for x in (c, tx):
        h = x.hits
        qlen = x.ql[h["query"].astype(np.int64) + 1] - 1 - x.ql[h["query"]]
        assert (h["seed_offset"] >= 0).all() and (h["seed_offset"] < qlen).all()
        for k in range(len(h)):
            q, b, t, hi, hj, _ = x.inputs(k)
            assert 0 <= hj < len(t) and len(b) == len(q)
            assert int(np.searchsorted(x.tl, h["subject"][k], side="right") - 1) == x.target_of[k]
        assert max(len(s) for s in x.qs + x.ts) <= 2600 and len(h) <= 4000 and len(x.cbs) == len(x.qd)


# ---- saturation ----------------------------------------------------------------------------------------------------------
def test_saturation_cases_saturate(c):
    flags, scores = gc.expected(c)
    sat = _scans(c, ("sat",), 128)
    assert sum(1 for k, v in sat.items() if scores[k, 1] >= 0 and v.max() == 255) >= 20
    assert all(sat[int(k)].max() == 255 for k in c.family("sat", "identical") if scores[k, 1] >= 0)
    assert int((scores[:, 1] > 255).sum()) >= 10                          # above 255 only the combination can go
    # 255 within 60 columns of the start of the diagonal, and held from there on
    k = int(c.family("sat", "identical")[2])
    best, hist = c.scan(k, 128, history=True)
    lane = int(np.argmax(best))
    first = int(np.argmax(hist[:, lane] == 255))
    assert first < 60 and (hist[first:, lane] == 255).all() and len(hist) > first + 100


def test_both_profile_clamps_bind_inside_scanned_windows(c):
    hi = lo = 0
    for k in c.family("sat", "bias"):
        q, b, t, i, j, _ = c.inputs(int(k))
        a, z = gc.clamped_cells(c.M, q, b, t, i, j, 64, gc.WINDOW1)
        hi, lo = hi + (a > 0), lo + (z > 0)
    assert hi >= 5 and lo >= 5
    # and the clamp matters: an unclamped sum gives another profile
    q, b = c.inputs(int(c.family("sat", "bias")[0]))[:2]
    raw = c.M[:20, q & 31].astype(int) + b.astype(int)
    assert raw.max() > 127 and raw.min() < -128
    assert int(b.max()) == 127 and int(b.min()) == -128


def test_rows_of_letters_20_to_25_take_no_bias(c):
    flags, scores = gc.expected(c)
    n = 0
    for k in c.family("sat", "nonstd"):
        q, b, t, i, j, _ = c.inputs(int(k))
        assert t.min() >= 20 and t.max() <= 25 and (t == 23).any()
        if b.any():
            n += 1
            assert np.array_equal(gc.diag_scan(c.M, q, b, t, i, j, 64, gc.WINDOW1), gc.diag_scan(c.M, q, None, t, i, j, 64, gc.WINDOW1))
            # a bias on these rows would show: +127 per column on forty query letters
            biased = np.clip(c.M[:, q & 31].astype(int) + b.astype(int), -128, 127)
            assert (biased[20:26] != c.M[20:26, q & 31]).any()
    assert n >= 5
    mixed = c.family("sat", "mixed")
    assert len(mixed) >= 10 and all(((c.inputs(int(k))[2] >= 20).any() and (c.inputs(int(k))[2] < 20).any()) for k in mixed)


def test_fallback_case_returns_to_zero_and_rises_again(c):
    seen = 0
    for k in c.family("sat", "fallback"):
        best, hist = c.scan(int(k), 128, history=True)
        lane = int(np.argmax(best))
        col = hist[:, lane]
        top = np.nonzero(col == 255)[0]
        zero = np.nonzero(col == 0)[0]
        if len(top) and any(top[0] < z and (col[z:] >= 200).any() for z in zero):
            seen += 1
    assert seen >= 3


# ---- diagonal combination ------------------------------------------------------------------------------------------------
def test_combination_cases_put_the_two_diagonals_on_the_intended_lanes(c):
    flags, scores = gc.expected(c)
    seen = set()
    for k in np.concatenate([c.family("comb"), c.family("longcomb")]):
        k = int(k)
        _, kind, gap, name, lo, hi, helper = c.info[k]
        assert scores[k, 1] >= 0, c.tags[k]                                # a stage-2 hit
        v = c.scan(k, 128)
        rest = np.delete(v, [lo, hi])
        assert v[lo] == v[hi] == 255 and rest.max() < 255, c.tags[k]       # the two strongest, exactly there
        assert scores[k, 1] > 255, c.tags[k]
        if helper:                                                         # the third, weaker diagonal that carried stage 1
            assert c.diag_score <= v[64] < 255 and not (0 <= lo - 32 < 64 or 0 <= hi - 32 < 64), c.tags[k]
        if name == "band1":
            v1 = c.scan(k, 64)
            assert v1[0] == v1[63] == 255 and v1[1:63].max() < 255, c.tags[k]
        seen.add((kind, gap, name, lo, hi))
    for kind in ("del", "ins"):
        for gap in gc.KS:
            assert any(s[:2] == (kind, gap) and s[3] <= 63 < s[4] for s in seen) or gap > 127, (kind, gap)
            if gap <= 63:
                assert (kind, gap, "low", 0, gap) in seen and (kind, gap, "high", 64, 64 + gap) in seen
        assert (kind, 1, "seam", 63, 64) in seen and (kind, 127, "seam", 0, 127) in seen and (kind, 63, "band1", 32, 95) in seen


def test_exact_pair_sits_at_diag_score_and_one_below(c):
    flags, scores = gc.expected(c)
    at, below = int(c.family("exact", "at")[0]), int(c.family("exact", "below")[0])
    va, vb = c.scan(at, 128), c.scan(below, 128)
    assert (va[63], va[66]) == (gc.STRONG, c.diag_score) and (vb[63], vb[66]) == (gc.STRONG, c.diag_score - 1)
    assert np.delete(va, [63, 66]).max() < c.diag_score and np.delete(vb, [63, 66]).max() < c.diag_score
    # the twin counts at diag_score (one gap of three diagonals), and not below it
    assert scores[at, 1] == gc.STRONG + c.diag_score - c.params.gap_open - 3 * c.params.gap_extend and scores[below, 1] == gc.STRONG


# ---- geometry ------------------------------------------------------------------------------------------------------------
def test_geometry_cases_cover_the_listed_shapes(full):
    c = full
    flags, scores = gc.expected(c)
    corner = c.family("geo", "corner")
    pairs = {c.info[k][2:4] for k in corner}
    assert pairs == {(n, m) for n in gc.QUERY_LENS for m in gc.TARGET_LENS + gc.EXTRA_TARGET_LENS}
    for n, m in pairs:
        got = {c.info[k][4:6] for k in corner if c.info[k][2:4] == (n, m)}
        assert {(0, 0), (0, m - 1), (n - 1, 0), (n - 1, m - 1)} <= got
    geo = c.family("geo")
    ranges = {}
    for k in geo:
        d, j0, j1, _ = c.window(int(k), 64)
        ranges.setdefault(j1 - j0, []).append(int(k))
    assert set(gc.RANGE_LENS) <= set(ranges)
    # every short range shows in the result, and a scan that leaves out the tail columns or misreads the second quad shows too
    g = (c.diag_score, c.params.gap_open, c.params.gap_extend)
    for L in gc.RANGE_LENS:
        seen = [k for k in ranges[L] if scores[k, 0] > 0]
        assert seen, L
        assert all(c.combine(c.scan(k, 64)) == scores[k, 0] for k in seen)            # the numpy scan agrees with the oracle here
        if L % 4:
            assert any(c.combine(c.scan(k, 64, fault="tail")) != scores[k, 0] for k in seen), L
        if L > 4:
            assert any(c.combine(c.scan(k, 64, fault="quad2")) != scores[k, 0] for k in seen), L
        two = [k for k in ranges[L] if scores[k, 1] > 0 and c.window(k, 128)[2] - c.window(k, 128)[1] == L]
        assert two or L == 1, L                                                        # and in stage 2 (one column never gets there)
        if L % 4:
            assert L == 1 or any(c.combine(c.scan(k, 128, fault="tail")) != scores[k, 1] for k in two), L
    for m in (1, 2, 3, 4, 5):                                             # every short target, and the one-letter query
        assert any(scores[k, 0] > 0 for k in geo if len(c.inputs(int(k))[2]) == m), m
    assert sum(1 for k in geo if len(c.inputs(int(k))[0]) == 1 and scores[k, 0] > 0) >= 5
    assert {len(c.inputs(int(k))[2]) for k in c.family("geo", "short") if scores[k, 0] > 0} == set(range(1, 10))
    # the clamp on d_begin binds, per band; for band 128 on hits whose stage 2 runs
    assert sum(1 for k in geo if c.window(int(k), 64)[3]) >= 10
    assert sum(1 for k in c.family("geo", "clamp") if c.window(int(k), 64)[3] and scores[k, 0] >= 100) >= 4
    assert sum(1 for k in geo if scores[k, 1] >= 0 and c.window(int(k), 128)[3]) >= 10
    assert sum(1 for k in c.family("geo", "clamp") if scores[k, 1] >= 100 and c.window(int(k), 128)[3]) >= 4
    # a column range that the query clips on either side (j0 > j_begin, j1 < j_end)
    assert any(c.window(int(k), 64)[1] > max(c.inputs(int(k))[4] - gc.WINDOW1, 0) for k in geo)
    assert any(c.window(int(k), 64)[2] < min(c.inputs(int(k))[4] + gc.WINDOW1, len(c.inputs(int(k))[2])) for k in geo)


def test_first_and_last_sequences_of_both_blocks_carry_hits(full):
    c = full
    nq, nt = len(c.qs), len(c.ts)
    assert c.ql[0] == 256 and len(c.qd) == c.ql[-1] + 256 and c.tl[0] == 256 and len(c.td) == c.tl[-1] + 256
    h = c.hits
    for qid in (0, nq - 1):
        mine = np.nonzero(h["query"] == qid)[0]
        assert len(mine) >= 10
        # bands that reach before the first letter and past the last letter of the query: reads in the perimeter
        assert any(c.window(int(k), 64)[0] + c.window(int(k), 64)[1] < 0 for k in mine)
        assert any(c.window(int(k), 64)[0] + 63 + c.window(int(k), 64)[2] - 1 >= len(c.qs[qid]) for k in mine)
    for tid in (0, nt - 1):
        mine = [k for k in range(len(h)) if c.target_of[k] == tid]
        assert len(mine) >= 10
        assert any(c.inputs(k)[4] == 0 for k in mine) and any(c.inputs(k)[4] == len(c.ts[tid]) - 1 for k in mine)


# ---- units ---------------------------------------------------------------------------------------------------------------
def test_unit_runs(full):
    c = full
    unit = c.family("unit")
    assert (np.diff(unit) == 1).all()                                     # one stretch of the hit list
    q = c.hits["query"][unit]
    cuts = np.concatenate([[0], np.nonzero(np.diff(q))[0] + 1, [len(q)]])
    runs = {}
    for a, z in zip(cuts[:-1], cuts[1:]):
        runs.setdefault(len(c.qs[int(q[a])]), []).append(int(z - a))
    assert runs == {n: list(gc.RUNS) for n in gc.CLASS_QLENS}             # every query: nine non-adjacent runs
    flags, scores = gc.expected(c)
    for n in gc.CLASS_QLENS:
        mine = c.family("unit", n)
        assert len(mine) == sum(gc.RUNS)
        assert int((scores[mine, 1] >= 0).sum()) >= 100 and int((scores[mine, 1] < 0).sum()) >= 10
        assert int(flags[mine].sum()) >= 100 and int((flags[mine] == 0).sum()) >= 10


# ---- translated queries --------------------------------------------------------------------------------------------------
def test_translated_cases(tx):
    c = tx
    flags, scores = gc.expected(c)
    assert c.contexts == 6 and len(c.qs) == 6 * len(gc.READ_LENS)
    lens0 = [len(c.qs[6 * r]) for r in range(len(gc.READ_LENS))]
    assert lens0 == list(gc.FRAME0_LENS) + [128, 127, 128]
    assert [len(c.qs[6 * gc.READ_LENS.index(384) + f]) for f in range(6)] == [128, 127, 127, 128, 127, 127]
    assert [len(c.qs[6 * gc.READ_LENS.index(383) + f]) for f in range(6)] == [127] * 6
    off = [k for k in range(len(c.hits)) if c.inputs(k)[5] < gc.MIN_QLEN]
    one = [k for k in range(len(c.hits)) if gc.MIN_QLEN <= c.inputs(k)[5] < gc.MIN_STAGE2_QLEN]
    both = [k for k in range(len(c.hits)) if c.inputs(k)[5] >= gc.MIN_STAGE2_QLEN]
    assert len(off) >= 10 and len(one) >= 10 and len(both) >= 10
    assert all(flags[k] == 1 and tuple(scores[k]) == (-1, -1) for k in off)
    assert all(scores[k, 1] == -1 for k in one) and sum(int(flags[k]) for k in one) >= 10 and sum(1 for k in one if not flags[k]) >= 3
    assert sum(1 for k in both if scores[k, 1] >= 0) >= 10 and sum(1 for k in both if scores[k, 1] < 0) >= 3
    for regime in (off, one, both):
        assert {int(c.hits["query"][k]) % 6 for k in regime} == set(range(6))          # hits in every one of the six contexts
    # a context shorter than 85 letters whose read is filtered all the same: the rule reads context 0
    assert any(len(c.inputs(k)[0]) < gc.MIN_QLEN <= c.inputs(k)[5] for k in one)
    # the cutoff row: context 0's length, not the frame's own
    rows = c.family("tx", "row")
    assert len(rows) >= 2 and {c.info[k][2] for k in rows} >= {384, 385}
    for k in rows:
        k = int(k)
        q, _, _, _, _, qlen0 = c.inputs(k)
        assert (len(q), qlen0) == (127, 128) and flags[k] == 0
        assert c.judge(k, row_len=len(q))[0] == 1 and c.judge(k, row_len=qlen0)[0] == 0


def test_long_query_carries_the_edges_onto_the_unit_kernel_matrix_path(full):
    c = full
    flags, scores = gc.expected(c)
    mine = np.sort(np.concatenate([c.family("long"), c.family("longcomb")]))
    assert len(mine) >= 80 and len({int(q) for q in c.hits["query"][mine]}) == 1
    q, b = c.inputs(int(mine[0]))[:2]
    assert len(q) > gc.CLASS_QLENS[2] and (np.diff(mine) == 1).all()       # no LDS class holds it; one stretch: units of its own
    sat = c.family("long", "sat")
    assert sum(1 for k in sat if c.scan(int(k), 64).max() == 255) >= 10
    hi = lo = 0
    for k in sat:
        x = c.inputs(int(k))
        a, z = gc.clamped_cells(c.M, x[0], x[1], x[2], x[3], x[4], 64, gc.WINDOW1)
        hi, lo = hi + (a > 0), lo + (z > 0)
    assert hi >= 5 and lo >= 5
    assert any((c.inputs(int(k))[2] >= 20).any() for k in sat)
    assert {c.info[k][2] for k in c.family("longcomb")} == {1, 63, 64, 127} and (scores[c.family("longcomb"), 1] > 255).all()
    corner = c.family("long", "corner")
    short = [k for k in corner if len(c.inputs(int(k))[2]) <= 9]
    assert {c.window(int(k), 64)[2] - c.window(int(k), 64)[1] for k in short if scores[k, 0] > 0} >= set(gc.RANGE_LENS)
    assert any(c.inputs(int(k))[3] == 0 for k in corner) and any(c.inputs(int(k))[3] == len(q) - 1 for k in corner)
