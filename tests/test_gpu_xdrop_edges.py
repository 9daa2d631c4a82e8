"""-m gpu: xdrop_seg_kernel (csrc/bias_kernels.hip) through dmnd_xdrop_ungapped on the constructed corpus of tests/xdrop_cases.py
(the CPU file test_xdrop_cases.py asserts what that corpus contains): the delimiter at every byte of a sixteen-letter chunk in both
directions, walks across one, two and three chunks and up to 2000 letters, the first and last sequence of both blocks (chunks that
reach into the 256-byte perimeter), one-letter sequences, a subject on a delimiter, losses of exactly xdrop - 1 / xdrop / xdrop + 1
completed in front of chunk offsets 0, 1, 14, 15, 16, 17, ties, soft-mask bits, B J Z X *, low-complexity queries. Every field of
every hit equals the restated reference function, for five x-drop values, without and with the Hauser bias (the host's restatement,
hip.extend_plan); a failure names the hit's family tag. The corpus rebuilt on PAM30 9/1 and BLOSUM45 14/2 (xdrop_cases.corpus(params),
with a boundary family around each system's own x-drop default) runs on a context of that system: every hit for every x-drop value,
and xdrop = 0 against the default worked out here from the system's lambda and K -- 22 and 27, not BLOSUM62's 20."""
import math

import numpy as np
import pytest
import torch

import scoring_schemes as ss
import xdrop_cases as xc
from diamond_amd import hip

pytestmark = pytest.mark.gpu
FIELDS = ("i", "j", "len", "score")


@pytest.fixture(scope="module")
def c():
    return xc.corpus()


@pytest.fixture(scope="module")
def ctx(c):
    assert torch.cuda.is_available()
    x = hip.Context(params=c.params)
    x.upload_block(hip.QUERY, c.qd, c.ql)
    x.upload_block(hip.TARGET, c.td, c.tl)
    yield x
    x.close()


def _same(c, got, want, index, what):
    assert len(got) == len(want)
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        if len(bad):
            k = int(bad[0])
            tags = sorted({c.tags[int(index[b])].split("/")[0] for b in bad})
            raise AssertionError("%s: field %s of %d hits differs (families %s); first: hit %d [%s] got %s, want %s"
                                 % (what, f, len(bad), tags, int(index[k]), c.tags[int(index[k])], got[k], want[k]))


@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("xdrop", xc.XDROPS)
def test_every_hit_of_the_corpus_equals_the_reference(c, ctx, xdrop, use_bias):
    everything = np.arange(len(c.hits))
    got = ctx.xdrop_ungapped(c.hits, use_bias=use_bias, xdrop=xdrop)
    _same(c, got, c.expected(xdrop, use_bias), everything, "xdrop %d, bias %s" % (xdrop, use_bias))
    # another order: other hits share a wavefront, the results are the same hits' results
    shuffled = ctx.xdrop_ungapped(c.hits[c.shuffled], use_bias=use_bias, xdrop=xdrop)
    _same(c, shuffled, c.expected(xdrop, use_bias, c.shuffled), c.shuffled, "shuffled, xdrop %d, bias %s" % (xdrop, use_bias))
    assert all(np.array_equal(shuffled[f], got[f][c.shuffled]) for f in FIELDS)


@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("n", xc.LAUNCH_SIZES)
def test_hit_arrays_around_one_workgroup(c, ctx, n, use_bias):
    """1, 255, 256 and 257 hits: the last wavefront of a launch is partly idle, the 257th hit is a workgroup's only one"""
    for index in (np.arange(n), c.shuffled[:n], np.arange(len(c.hits) - n, len(c.hits))):
        got = ctx.xdrop_ungapped(c.hits[index], use_bias=use_bias, xdrop=xc.DEFAULT_XDROP)
        _same(c, got, c.expected(xc.DEFAULT_XDROP, use_bias, index), index, "%d hits, bias %s" % (n, use_bias))


@pytest.mark.parametrize("use_bias", [False, True])
def test_xdrop_zero_means_the_matrix_default(c, ctx, use_bias):
    """BLOSUM62 11/1: raw_ungapped_xdrop = 20"""
    everything = np.arange(len(c.hits))
    got = ctx.xdrop_ungapped(c.hits, use_bias=use_bias, xdrop=0)
    _same(c, got, c.expected(20, use_bias), everything, "xdrop 0, bias %s" % use_bias)
    same = ctx.xdrop_ungapped(c.hits, use_bias=use_bias, xdrop=20)
    assert all(np.array_equal(got[f], same[f]) for f in FIELDS)
    narrow = c.expected(7, use_bias)
    assert int(((got["len"] != narrow["len"]) | (got["score"] != narrow["score"])).sum()) >= 100      # and 7 is another answer


# ---- other matrices: an x-drop default away from 20 ----------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=ss.XDROP, ids=ss.scheme_id)
def scheme_ctx(request):
    """(corpus on the scheme's matrix, a context on the scheme's params with the corpus's blocks)"""
    assert torch.cuda.is_available()
    sc = xc.corpus(ss.params(request.param))
    x = hip.Context(params=sc.params)
    x.upload_block(hip.QUERY, sc.qd, sc.ql)
    x.upload_block(hip.TARGET, sc.td, sc.tl)
    yield sc, x
    x.close()


@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("which", range(len(xc.XDROPS) + 1))
def test_scheme_every_hit_of_the_corpus_equals_the_reference(scheme_ctx, which, use_bias):
    """test_every_hit_of_the_corpus_equals_the_reference on the corpus of another matrix, for XDROPS and the system's own default"""
    sc, x = scheme_ctx
    assert len(sc.xdrops) == len(xc.XDROPS) + 1 and sc.default_xdrop in sc.xdrops and sc.default_xdrop not in xc.XDROPS
    test_every_hit_of_the_corpus_equals_the_reference(sc, x, sc.xdrops[which], use_bias)


@pytest.mark.parametrize("use_bias", [False, True])
def test_scheme_xdrop_zero_means_the_matrix_default(scheme_ctx, use_bias):
    """raw_ungapped_xdrop = ceil((12.3 ln 2 + ln K) / lambda) of the context's system, from its params"""
    sc, x = scheme_ctx
    p = x.params
    want = int(math.ceil((12.3 * math.log(2.0) + math.log(p.K)) / p.lambda_))
    assert want != 20
    everything = np.arange(len(sc.hits))
    got = x.xdrop_ungapped(sc.hits, use_bias=use_bias, xdrop=0)
    _same(sc, got, sc.expected(want, use_bias), everything, "xdrop 0 = %d, bias %s" % (want, use_bias))
    same = x.xdrop_ungapped(sc.hits, use_bias=use_bias, xdrop=want)
    assert all(np.array_equal(got[f], same[f]) for f in FIELDS)
    for other in (20, want - 1, want + 1):                                  # and BLOSUM62's default and the neighbours are other answers
        e = sc.expected(other, use_bias)
        assert int(((got["len"] != e["len"]) | (got["score"] != e["score"])).sum()) >= 100, other
