"""-m gpu: the gapped filter kernels (csrc/gapped_kernels.hip) through dmnd_gapped_filter on the constructed cases of
tests/gapped_cases.py (the CPU file test_gapped_cases.py asserts what they contain): diagonals held at 255 and fallen back to 0, both
int8 clamps of the biased profile, unbiased rows 20-25, two saturated diagonals k lanes apart on either side of the 63/64 seam of the
stage-2 band and at its ends, a diagonal at diag_score and at diag_score - 1, targets of 1 to 129 and queries of 1 to 65 letters with
hits in every corner, clamped bands, the first and last sequence of both blocks, runs of 1 to 129 hits per query in every LDS width
class and on the matrix path, six-frame queries around the 85- and 100-letter rules and the cutoff row of context 0, and PAM30 9/1.
Flag, f1 and f2 of every hit equal the C oracle under the reference's rules (gapped_cases.expected), once per launch form, each
compared with the oracle on its own:
  "units"   the default: gapped_filter_unit_kernel, one workgroup per unit -- on the LDS profile for queries up to 1792 letters, with
            the matrix in LDS (scan_diags_lds) for longer ones, which here are the 1793-letter unit query and the 1800-letter query
            of the families long / longcomb (saturation, clamps, letters 20-25, seam pairs, short ranges, corners);
  "perhit"  DMND_GF_PROFILE_TEST=0: gapped_filter_kernel, one wavefront per hit, scan_diags_lds for every query.
A failure names the hit's tag."""
import numpy as np
import pytest
import torch

import gapped_cases as gc
from diamond_amd import hip

pytestmark = pytest.mark.gpu
PATHS = ("units", "perhit")


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    x = hip.Context()
    yield x
    x.close()


def _load(ctx, c):
    ctx.upload_block(hip.QUERY, c.qd, c.ql)
    ctx.upload_block(hip.TARGET, c.td, c.tl)
    ctx.upload_cbs(c.cbs)
    ctx.set_query_contexts(c.contexts)
    ctx.set_gapped_filter(gc.EVALUE2)


def _path(monkeypatch, path):
    if path == "perhit":
        monkeypatch.setenv("DMND_GF_PROFILE_TEST", "0")                    # read per call: gapped_filter_kernel, one wavefront per hit
    else:
        monkeypatch.delenv("DMND_GF_PROFILE_TEST", raising=False)


def _run(ctx, c, index, what):
    """The hits `index` of the corpus in that order: every flag and both values against the expected ones"""
    index = np.asarray(index, np.int64)
    flags, scores = ctx.gapped_filter(c.hits[index], use_cbs=True, with_scores=True)
    want_flags, want_scores = gc.expected(c)
    for name, got, want in (("f1", scores[:, 0], want_scores[index, 0]), ("f2", scores[:, 1], want_scores[index, 1]), ("flag", flags, want_flags[index])):
        bad = np.nonzero(got != want)[0]
        if len(bad):
            k = int(index[bad[0]])
            fams = sorted({"/".join(c.tags[int(index[b])].split("/")[:2]) for b in bad})
            raise AssertionError("%s: %s of %d of %d hits differs (families %s); first: position %d, hit %d [%s] got %s, want %s"
                                 % (what, name, len(bad), len(index), fams, int(bad[0]), k, c.tags[k], got[bad[0]], want[bad[0]]))
    print("%s: %d hits, %d ran stage 2, %d passed, %d with a value of 255 or more"
          % (what, len(index), int((scores[:, 1] >= 0).sum()), int(flags.sum()), int((scores.max(axis=1) >= 255).sum())))
    return flags, scores


@pytest.mark.parametrize("path", PATHS)
def test_every_hit_of_every_blastp_case_equals_the_oracle(ctx, monkeypatch, path):
    c = gc.corpus("blastp")
    _load(ctx, c)
    _path(monkeypatch, path)
    _run(ctx, c, np.arange(len(c.hits)), "blastp, %s launch" % path)
    for family in ("sat", "comb", "exact", "geo", "long", "longcomb"):     # each family in a call of its own: other units, other waves
        _run(ctx, c, c.family(family), "%s, %s launch" % (family, path))


@pytest.mark.parametrize("path", PATHS)
def test_long_query_and_short_ranges_in_calls_of_their_own(ctx, monkeypatch, path):
    """The 1800-letter query alone ("units": every unit of the call takes the unit kernel's matrix path), in order, shuffled and
    reversed; the targets of 1 to 9 letters under the +16 bias, where every column of a range of 1 to 9 shows in f1."""
    c = gc.corpus("blastp")
    _load(ctx, c)
    _path(monkeypatch, path)
    mine = np.sort(np.concatenate([c.family("long"), c.family("longcomb")]))
    _run(ctx, c, mine, "1800-letter query, %s launch" % path)
    _run(ctx, c, mine[::-1], "1800-letter query reversed, %s launch" % path)
    _run(ctx, c, np.random.default_rng(14).permutation(mine), "1800-letter query shuffled, %s launch" % path)
    short = c.family("geo", "short")
    flags, scores = _run(ctx, c, short, "short ranges, %s launch" % path)
    assert (scores[:, 0] > 0).all() and int((scores[:, 1] > 0).sum()) >= 50
    _run(ctx, c, short[::-1], "short ranges reversed, %s launch" % path)


@pytest.mark.parametrize("path", PATHS)
def test_unit_cases_in_other_orders(ctx, monkeypatch, path):
    """The runs of 1 to 129 hits as they stand, shuffled (nearly every unit is one hit), with every query's hits reversed, every
    query's hits in one piece (462 consecutive hits: seven full units and one of 14), and calls that use one class only."""
    c = gc.corpus("blastp")
    _load(ctx, c)
    _path(monkeypatch, path)
    unit = c.family("unit")
    base_flags, base_scores = _run(ctx, c, unit, "units, %s launch" % path)
    perm = np.random.default_rng(11).permutation(len(unit))
    f, s = _run(ctx, c, unit[perm], "units shuffled, %s launch" % path)
    assert np.array_equal(f, base_flags[perm]) and np.array_equal(s, base_scores[perm])
    q = c.hits["query"][unit]
    rev = unit.copy()
    for qid in np.unique(q):
        at = np.nonzero(q == qid)[0]
        rev[at] = unit[at[::-1]]
    assert np.array_equal(c.hits["query"][rev], q) and not np.array_equal(rev, unit)
    _run(ctx, c, rev, "units, every query's hits reversed, %s launch" % path)
    order = np.argsort(q, kind="stable")
    _run(ctx, c, unit[order], "units, one piece per query, %s launch" % path)
    for n in (gc.CLASS_QLENS[-1], gc.CLASS_QLENS[0]):                      # only the matrix class; only the smallest class
        _run(ctx, c, c.family("unit", n), "units of the %d-letter query alone, %s launch" % (n, path))
    for r in gc.RUNS:                                                      # one run per class and nothing else in the call
        _run(ctx, c, [k for k in unit if c.info[k][2] == r], "runs of %d, %s launch" % (r, path))


@pytest.mark.parametrize("path", PATHS)
def test_translated_cases_equal_the_oracle_under_the_reference_rules(ctx, monkeypatch, path):
    c = gc.corpus("blastx")
    _load(ctx, c)
    _path(monkeypatch, path)
    try:
        flags, scores = _run(ctx, c, np.arange(len(c.hits)), "blastx, %s launch" % path)
        off = np.array([c.inputs(k)[5] < gc.MIN_QLEN for k in range(len(c.hits))])
        assert off.sum() >= 10 and (flags[off] == 1).all() and (scores[off] == -1).all()
        perm = np.random.default_rng(12).permutation(len(c.hits))
        _run(ctx, c, perm, "blastx shuffled, %s launch" % path)
        _run(ctx, c, c.family("tx", "row"), "blastx cutoff row, %s launch" % path)
    finally:
        ctx.set_query_contexts(1)


@pytest.mark.parametrize("path", PATHS)
def test_second_scoring_system(monkeypatch, path):
    """PAM30 9/1: another matrix, other gap costs in the combination, diag_score 21, other cutoff tables"""
    c = gc.corpus("pam30")
    assert torch.cuda.is_available()
    x = hip.Context(params=c.params)
    try:
        _load(x, c)
        _path(monkeypatch, path)
        _run(x, c, np.arange(len(c.hits)), "pam30, %s launch" % path)
        _run(x, c, np.random.default_rng(13).permutation(len(c.hits)), "pam30 shuffled, %s launch" % path)
    finally:
        x.close()


@pytest.mark.parametrize("path", PATHS)
def test_second_call_with_fewer_hits_returns_its_own_values(ctx, monkeypatch, path):
    """The context keeps its flag and score buffers between calls: a shorter call after a long one must overwrite every entry it
    returns. The second call's hits are chosen so that nearly every entry differs from what the first call left there."""
    c = gc.corpus("blastp")
    _load(ctx, c)
    _path(monkeypatch, path)
    n = len(c.hits)
    _run(ctx, c, np.arange(n), "first call, %s launch" % path)
    want_flags, want_scores = gc.expected(c)
    for index in (np.arange(n)[::-1][:700], np.arange(n)[::-1][:65], np.arange(n)[::-1][:1]):
        stale = (want_scores[index] == want_scores[:len(index)]).all(axis=1)
        assert stale.mean() < 0.2
        _run(ctx, c, index, "second call of %d hits, %s launch" % (len(index), path))
        _run(ctx, c, np.arange(n), "first call again, %s launch" % path)
