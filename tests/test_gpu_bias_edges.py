"""-m gpu: hauser_bias_kernel (csrc/bias_kernels.hip) itself, position by position. The device bias has no entry of its own; it is
read back through dmnd_xdrop_ungapped with a probe: the context's matrix scores every query letter against letter 30 (used by no
sequence) with 100, the target block is the one one-letter sequence [30], and every query position p is a seed hit on it with
xdrop 10**6. The left walk meets the target's delimiter at once, the right walk takes the one letter: score = 100 + bias[p], len 1
(and exactly 100 without the bias -- the control). The Hauser sums and the background scores read matrix columns below 20 only, so
neither the device bias nor the host restatement (hip.extend_plan with the same params, pinned on the reference's taps by
test_extend_plan.py) sees the probe column. |bias| stays far below 100 for BLOSUM62: no position goes unobserved.

Query blocks: every phase of the five window loops around W / 2 = 20 and W + 1 = 41, the thread stride of a workgroup (sequences
around 256 and 512 letters, 1000, 3000), each length with random letters, with B J Z X * and soft-mask bits, and of low complexity;
65536 + 300 sequences of one to three letters (more sequences than workgroups: the grid stride)."""
import numpy as np
import pytest
import torch

from diamond_amd import hip, workload

pytestmark = pytest.mark.gpu
PROBE = 30
LENGTHS = [1, 2, 3, 19, 20, 21, 22, 39, 40, 41, 42, 43, 60, 61, 80, 81, 82, 255, 256, 257, 511, 512, 513, 1000, 3000]


def _block(seqs):
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    return workload.sequence_set(np.concatenate(seqs).astype(np.int8), off)


def phase_block():
    rng = np.random.default_rng(41)
    seqs = []
    for n in LENGTHS:
        seqs.append(rng.integers(0, 20, n).astype(np.int8))                            # random letters
        s = rng.integers(0, 20, n).astype(np.int8)                                     # B J Z X * and soft-mask bits sprinkled in
        at = rng.random(n) < 0.12
        s[at] = rng.integers(20, 25, int(at.sum())).astype(np.int8)
        if n == 1:
            s[0] = 23
        soft = rng.random(n) < 0.3
        s[soft] = (s[soft].astype(np.uint8) | 0x80).astype(np.int8)
        seqs.append(s)
        s = rng.integers(0, 20, n).astype(np.int8)                                     # low complexity: the first half one residue
        s[: n // 2] = s[0]
        seqs.append(s)
    for letter in (0, 17, 4):                                                          # poly-A, poly-W, poly-C
        seqs.append(np.full(50, letter, np.int8))
    return seqs


def stride_block():
    rng = np.random.default_rng(42)
    lens = rng.integers(1, 4, 65536 + 300)
    return [rng.integers(0, 20, int(n)).astype(np.int8) for n in lens]


@pytest.fixture(scope="module")
def probe():
    assert torch.cuda.is_available()
    params = hip.default_params()
    for a in range(31):
        params.matrix8[a * 32 + PROBE] = 100
    ctx = hip.Context(params=params)
    td, tl = _block([np.array([PROBE], np.int8)])
    ctx.upload_block(hip.TARGET, td, tl)
    yield ctx, params, td, tl
    ctx.close()


def _probe_hits(ql, tl):
    lens = np.diff(ql) - 1
    hits = np.zeros(int(lens.sum()), dtype=hip.SEED_HIT_DTYPE)
    hits["query"] = np.repeat(np.arange(len(lens)), lens)
    hits["seed_offset"] = np.arange(len(hits)) - np.repeat(np.cumsum(lens) - lens, lens)
    hits["subject"] = tl[0]
    return hits, lens


@pytest.mark.parametrize("name,make", [("window phases and thread stride", phase_block), ("grid stride", stride_block)])
def test_device_bias_equals_the_host_restatement_at_every_position(probe, name, make):
    ctx, params, td, tl = probe
    seqs = make()
    qd, ql = _block(seqs)
    hits, lens = _probe_hits(ql, tl)
    pos = ql[hits["query"]] + hits["seed_offset"]
    want = hip.extend_plan(params, qd, ql, td, tl, np.zeros(0, hip.SEED_HIT_DTYPE))[0].astype(np.int32)[pos]
    plain = hip.extend_plan(hip.default_params(), qd, ql, td, tl, np.zeros(0, hip.SEED_HIT_DTYPE))[0].astype(np.int32)[pos]
    assert np.array_equal(want, plain)                     # the probe column is outside what the bias reads
    assert want.min() > -100 and want.max() < 100          # no position goes unobserved
    assert want.min() < -3 and want.max() > 1 and len(np.unique(want)) >= 8      # and there is something to observe
    ctx.upload_block(hip.QUERY, qd, ql)
    control = ctx.xdrop_ungapped(hits, use_bias=False, xdrop=10 ** 6)
    assert (control["score"] == 100).all() and (control["len"] == 1).all()
    assert np.array_equal(control["i"], hits["seed_offset"]) and (control["j"] == tl[0]).all()
    got = ctx.xdrop_ungapped(hits, use_bias=True, xdrop=10 ** 6)
    assert (got["len"] == 1).all() and np.array_equal(got["i"], hits["seed_offset"]) and (got["j"] == tl[0]).all()
    bias = got["score"].astype(np.int32) - 100
    bad = np.nonzero(bias != want)[0]
    assert len(bad) == 0, "%s: %d of %d positions differ; first: sequence %d (%d letters) position %d, device %d, host %d" % (
        name, len(bad), len(want), hits["query"][bad[0]], lens[hits["query"][bad[0]]], hits["seed_offset"][bad[0]], bias[bad[0]], want[bad[0]])
    # zeros the definition demands, asserted on the device's values
    letter = qd[pos].view(np.uint8) & 31
    assert (letter >= 20).sum() > (50 if "phases" in name else -1) and (bias[letter >= 20] == 0).all()
    one = lens[hits["query"]] == 1
    assert one.any() and (bias[one] == 0).all()
    if "phases" in name:
        assert len(want) == 3 * sum(LENGTHS) + 150
        assert (want[-150:] < -3).all()                    # poly-A, poly-W, poly-C: a strongly negative bias throughout
    else:
        assert len(seqs) > 65536
        tail = hits["query"] >= 65536                      # the sequences a workgroup reaches only in its second round
        assert tail.sum() >= 300 and (bias[tail] != 0).any()
