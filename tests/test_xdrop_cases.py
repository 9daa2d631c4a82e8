"""The x-drop corpus (tests/xdrop_cases.py) without a GPU: the walk the kernel shares with the host (xdrop_core.h, its host
instantiation through tests/emu/xdrop_emu.cpp) equals the restated reference function on every case, and the corpus has the
properties the device test (test_gpu_xdrop_edges.py) relies on -- asserted from the reference's results alone, so a generator that
stops producing an edge fails here and not silently there."""
import numpy as np
import pytest

import emu_py as emu
import scoring_schemes as ss
import xdrop_cases as xc


@pytest.fixture(scope="module")
def c():
    return xc.corpus()


def _ends(c, xdrop, use_bias=False):
    Md, q, cbs, t = c._plain[use_bias]
    return [xc.walk_ends(Md, q, cbs, t, c.qa(k), int(c.hits["subject"][k]), xdrop) for k in range(len(c.hits))]


@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("xdrop", xc.XDROPS)
def test_shared_walk_equals_the_reference_function(c, xdrop, use_bias):
    qa = c.ql[c.hits["query"]] + c.hits["seed_offset"]
    got = emu.xdrop_segments(c.M, c.qd, c.cbs if use_bias else None, c.td, qa, c.hits["subject"], xdrop)
    want = xc.reference(c, xdrop, use_bias)
    for name, g, w in (("left", got[:, 0], want[:, 0]), ("len", got[:, 0] + got[:, 1], want[:, 1]), ("score", got[:, 2], want[:, 2])):
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (name, c.tags[bad[0]], int(g[bad[0]]), int(w[bad[0]]), len(bad))


def test_corpus_size_and_order(c):
    assert 20000 <= len(c.hits) <= 30000
    assert sorted(c.shuffled.tolist()) == list(range(len(c.hits)))
    assert set(xc.family_counts(c)) == {"grid", "long", "corner", "delim", "boundary", "tie", "homolog"}
    # what dmnd_xdrop_ungapped accepts: the seed on a query letter, the subject anywhere inside the target block
    h = c.hits
    assert (h["seed_offset"] >= 0).all() and (c.ql[h["query"]] + h["seed_offset"] < c.ql[h["query"] + 1] - 1).all()
    assert (h["subject"] >= c.tl[0]).all() and (h["subject"] < c.tl[-1]).all()


def test_every_cell_of_the_delimiter_grid_in_both_directions(c):
    ref = xc.reference(c, 10 ** 6, False)
    seen = set()
    for k, i in enumerate(c.info):
        if i[0] != "grid":
            continue
        _, direction, a, b, _ = i
        delta, length, _ = ref[k]
        # the walk of that direction ends on the delimiter that comes first: its reach is the whole identical run
        if direction == "left":
            assert delta == min(a, b), c.tags[k]
        else:
            assert length - delta == 1 + min(a, b), c.tags[k]
        seen.add((direction, a, b))
    assert seen == {(d, a, b) for d in ("left", "right") for a in range(19) for b in range(19)}
    longs = {i[1:] for i in c.info if i[0] == "long"}
    for n in xc.LONG_RUNS:
        assert ("left", n, 0) in longs and ("right", 0, n) in longs
    for a in xc.LONG_RUNS[:6]:
        for b in xc.LONG_RUNS[:6]:
            assert ("both", a, b) in longs
    for k, i in enumerate(c.info):
        if i[0] == "long":
            # the run is taken whole (the other side of a one-sided case is a few random letters)
            assert i[1] == "right" or ref[k][0] == i[2], c.tags[k]
            assert i[1] == "left" or ref[k][1] - ref[k][0] == i[3], c.tags[k]


def test_walks_cross_one_two_and_three_chunks(c):
    ref = xc.reference(c, c.default_xdrop, False)
    left, right = ref[:, 0], ref[:, 1] - ref[:, 0]
    for n in (16, 32, 48):
        assert int((left > n).sum()) >= 50 and int((right > n).sum()) >= 50, (n, int((left > n).sum()), int((right > n).sum()))


def test_corners_and_delimiter_subjects(c):
    ref = xc.reference(c, c.default_xdrop, False)
    h = c.hits
    last_q, last_t = c.n_queries - 1, c.n_targets - 1
    tid = np.searchsorted(c.tl, h["subject"], side="right") - 1
    tpos = h["subject"] - c.tl[tid]
    qlen = c.ql[h["query"] + 1] - c.ql[h["query"]] - 1
    tlen = c.tl[tid + 1] - c.tl[tid] - 1
    for q in (0, last_q):
        for t in (0, last_t):
            at = (h["query"] == q) & (tid == t)
            assert (at & (h["seed_offset"] == 0) & (tpos == 0)).any() and (at & (h["seed_offset"] == qlen - 1) & (tpos == tlen - 1)).any()
            # the whole diagonal of the 48 identical letters, from either end: three full chunks up to the perimeter
            for k in np.nonzero(at & (h["seed_offset"] == tpos) & (tpos < tlen))[0]:
                assert (ref[k][0], ref[k][1]) == (h["seed_offset"][k], xc.CORNER_LEN), c.tags[k]
    assert ((qlen == 1) & (tlen == 1)).any() and ((qlen == 1) & (tlen > 1)).any() and ((qlen > 1) & (tlen == 1)).any()
    on_delim = tpos == tlen
    assert {int(t) for t in tid[on_delim]} >= {0, last_t} and on_delim.sum() >= 10
    n = 0
    for k in np.nonzero(on_delim)[0]:
        if c.info[k][:2] == ("delim", "nothing"):
            assert tuple(ref[k]) == (0, 0, 0), c.tags[k]
            n += 1
    assert n >= 9
    assert any(c.info[k][:2] == ("delim", "walks") and ref[k][2] > 0 for k in np.nonzero(on_delim)[0])


def test_both_endings_for_every_xdrop_and_sharp_boundary_triples(c):
    for x in c.xdrops[:-1]:
        ends = _ends(c, x)
        by_x = sum(e[0][0] == "x" for e in ends) + sum(e[1][0] == "x" for e in ends)
        by_d = sum(e[0][0] == "d" for e in ends) + sum(e[1][0] == "d" for e in ends)
        assert by_x >= 50 and by_d >= 50, (x, by_x, by_d)
        ref = xc.reference(c, x, False)
        triples = {}
        for k, i in enumerate(c.info):
            if i[0] == "boundary" and i[2] == x:
                triples.setdefault((i[1], i[4], i[5]), {})[i[3]] = (k, ends[k][0 if i[1] == "left" else 1])
        assert len(triples) == 2 * len(xc.OFFSETS) * xc.BOUNDARY_VARIANTS
        offsets = set()
        for (direction, o, v), tr in triples.items():
            segs = {tuple(ref[tr[d][0]]) for d in (-1, 0, 1)}
            assert len(segs) >= 2, (x, direction, o, v)
            # one short of xdrop the walk goes on into the stronger run; at xdrop and one beyond, it ends by x-drop on the very letter
            (k0, e0), (k1, e1), (k2, e2) = tr[-1], tr[0], tr[1]
            assert e1[0] == "x" and e2[0] == "x" and e1[1] == e2[1] and e0[1] > e1[1], (x, direction, o, v, e0, e1, e2)
            assert e1[1] % 16 == o % 16, (x, direction, o, v, e1)      # letters taken before the decisive one = its index in the walk
            offsets.add(e1[1])
        assert {w % 16 for w in offsets} == {0, 1, 14, 15} and {16, 17} <= offsets, (x, sorted(offsets))
    ends = _ends(c, 10 ** 6)
    assert all(e[0][0] == "d" and e[1][0] == "d" for e in ends)      # only delimiters end a walk


def test_bias_and_xdrop_change_segments(c):
    plain, biased = xc.reference(c, c.default_xdrop, False), xc.reference(c, c.default_xdrop, True)
    assert int((plain != biased).any(axis=1).sum()) >= 100
    narrow = xc.reference(c, 7, False)
    assert int((plain != narrow).any(axis=1).sum()) >= 100
    # the low-complexity queries carry a strongly negative bias that shortens walks
    low = np.array([i[0] == "homolog" and i[1] == "lowcomplex" for i in c.info])
    assert int((biased[low, 1] < plain[low, 1]).sum()) >= 100
    assert c.cbs.min() <= -4


def test_letters_of_the_corpus(c):
    for data in (c.qd, c.td):
        assert int(((data.view(np.uint8) & 0x80) != 0).sum()) > 2000                  # soft-mask bits
        low = data.view(np.uint8) & 31
        for letter in (20, 21, 22, 23, 24):
            assert int((low == letter).sum()) >= 20
        assert set(np.unique(low).tolist()) <= set(range(25)) | {31}
    kinds = {i[1] for i in c.info if i[0] == "homolog"}
    assert kinds == {"plain", "softmask", "nonstd", "lowcomplex"}


def test_every_tie_has_a_later_equal_maximum_left_alone(c):
    ref = xc.reference(c, c.default_xdrop, False)
    Md, q, _, t = c._plain[False]
    n = 0
    for k, i in enumerate(c.info):
        if i[0] != "tie":
            continue
        delta, length, score = (int(x) for x in ref[k])
        qa, sa = c.qa(k), int(c.hits["subject"][k])
        if i[1] == "left":
            sums, reach = xc.diagonal_sums(Md, q, t, qa, sa, -1), delta
            assert length == delta, c.tags[k]                                         # the right walk adds nothing
        else:
            assert delta == 0, c.tags[k]
            sums, reach = xc.diagonal_sums(Md, q, t, qa, sa, +1), length
        assert reach == i[2], c.tags[k]                                               # the L strong letters and no more
        assert max(sums + [0]) == score and any(s == score for s in sums[reach:]), (c.tags[k], sums, reach, score)
        n += 1
    assert n == len([i for i in c.info if i[0] == "tie"]) >= 600


# ---- the corpus on other matrices --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=ss.XDROP, ids=ss.scheme_id)
def sc(request):
    return xc.corpus(ss.params(request.param))


def test_scheme_corpus_is_built_around_its_own_default(sc):
    want = int(np.ceil((12.3 * np.log(2.0) + np.log(sc.params.K)) / sc.params.lambda_))
    assert sc.default_xdrop == want != xc.DEFAULT_XDROP and want in sc.xdrops and set(xc.XDROPS) <= set(sc.xdrops)
    assert sc is not xc.corpus() and not np.array_equal(sc.M, xc.corpus().M) and sc is xc.corpus(sc.params)
    assert len(sc.tie_ks) == 4 and all(k in sc.M[:20, :20] and -k in sc.M[:20, :20] for k in sc.tie_ks)
    assert {i[3] for i in sc.info if i[0] == "tie"} == set(sc.tie_ks)
    assert {i[2] for i in sc.info if i[0] == "boundary"} == set(sc.xdrops[:-1])


@pytest.mark.parametrize("use_bias", [False, True])
def test_scheme_shared_walk_equals_the_reference_function(sc, use_bias):
    for xdrop in sc.xdrops:
        test_shared_walk_equals_the_reference_function(sc, xdrop, use_bias)


def test_scheme_corpus_properties(sc):
    """every property of the BLOSUM62 corpus, from the reference function on this matrix"""
    test_corpus_size_and_order(sc)
    test_every_cell_of_the_delimiter_grid_in_both_directions(sc)
    test_walks_cross_one_two_and_three_chunks(sc)
    test_corners_and_delimiter_subjects(sc)
    test_bias_and_xdrop_change_segments(sc)
    test_letters_of_the_corpus(sc)
    test_every_tie_has_a_later_equal_maximum_left_alone(sc)


def test_scheme_both_endings_and_sharp_boundary_triples(sc):
    test_both_endings_for_every_xdrop_and_sharp_boundary_triples(sc)
    # the default differs from its neighbours on the triples built around it: xdrop = 0 read as 20, or as one more or less, shows
    x = sc.default_xdrop
    at = np.array([i[0] == "boundary" and i[2] == x for i in sc.info])
    for other in (x - 1, x + 1, xc.DEFAULT_XDROP):
        assert int((xc.reference(sc, x, False)[at] != xc.reference(sc, other, False)[at]).any(axis=1).sum()) >= 100, other
