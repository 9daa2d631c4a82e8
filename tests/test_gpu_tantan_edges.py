"""-m gpu: tantan masking on the MI355X (dmnd_mask_block, dmnd_mask_sequences) at its structural edges, letter for letter and count
for count against the oracle (oracle/tantan.c) on the corpus of tests/tantan_corpus.py -- whose own conditions
tests/test_tantan_corpus.py asserts on the CPU: sequence lengths around every chunk, group and kernel boundary, repeat periods
around the window of 50, non-standard letters, every standard matrix, subsets in any order, the list of masked positions below,
at and above its capacity, the block as it stands in HBM afterwards. The default mode (sequences up to 1024 letters in the
lane-per-sequence kernel, longer ones in the wavefront-per-sequence kernel) runs in this process; DMND_TANTAN_WAVE and
DMND_TANTAN_LONG are read once per process, so each forced kernel choice runs in a child of its own, which also reports the split
of every call (DMND_TRACE)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as orc
import tantan_corpus as tc
from diamond_amd import hip
from test_matrices import NAMES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context()
    yield c
    c.close()


def _same(got, want, group, limits, what):
    """got == want, byte for byte; a difference is reported with the first sequence (or the delimiter / padding) it lies in"""
    if np.array_equal(got, want):
        return
    at = int(np.flatnonzero(got != want)[0])
    i = int(np.searchsorted(limits, at, "right")) - 1
    where = "padding" if i < 0 or i >= len(group) else ("delimiter after " if at == limits[i + 1] - 1 else "") + group[i][0]
    n_diff = int((got != want).sum())
    raise AssertionError("%s: %d bytes differ, the first at %d (%s, position %d): %d for %d"
                         % (what, n_diff, at, where, at - int(limits[max(i, 0)]), int(got[at]), int(want[at])))


def check_block(ctx, which, group, ids=None, host=True, matrix="blosum62"):
    """Uploads the block of `group` (a list of (name, letters)) and masks it -- all of it (dmnd_mask_block) or the sequences `ids`
    and then the rest (dmnd_mask_sequences twice). After each call: the masked sequences equal the oracle's, every other byte --
    the other sequences, delimiters, padding -- is as uploaded, the returned count is the oracle's total, and the block read back
    from HBM (dmnd_download_block) is the host copy byte for byte, so no byte but letters, 23 and 31 is left in it. host=False
    passes no host copy: the device writes the mask letter itself and only the block read back is compared.
    Returns the counts of the calls."""
    data, limits = tc.block(group)
    want = data.copy()
    counts = np.zeros(len(group), np.int64)
    for i, (_, s) in enumerate(group):
        m, counts[i] = tc.masked(s, matrix)
        want[limits[i]:limits[i] + len(s)] = m
    assert (want[:256] == 31).all() and (want[-256:] == 31).all() and (want[limits[1:] - 1] == 31).all()
    ctx.upload_block(which, data, limits)
    mine = data.copy() if host else None
    expect = data.copy()
    out = []
    calls = [None] if ids is None else [np.asarray(ids, np.int64), np.setdiff1d(np.arange(len(group)), ids)]
    for call in calls:
        if call is None:
            n = ctx.mask_block(which, mine)
            expect, total = want, int(counts.sum())
        else:
            n = ctx.mask_sequences(which, mine, call)
            for i in call:
                expect[limits[i]:limits[i + 1]] = want[limits[i]:limits[i + 1]]
            total = int(counts[call].sum())
        hbm = ctx.download_block(which, len(data))
        what = "%d of %d sequences" % (len(group) if call is None else len(call), len(group))
        if host:
            _same(mine, expect, group, limits, "host copy, " + what)
            _same(hbm, mine, group, limits, "block in HBM against the host copy, " + what)
        else:
            _same(hbm, expect, group, limits, "block in HBM, " + what)
        assert set(np.unique(hbm).tolist()) <= set(range(26)) | {31}
        assert n == total, (what, n, total)
        out.append(int(n))
    if ids is not None:
        assert np.array_equal(expect, want)                      # the two calls together: the whole block
    return out


# ---- default mode ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("host", [True, False], ids=["host_copy", "hbm_only"])
@pytest.mark.parametrize("which", [hip.TARGET, hip.QUERY], ids=["target", "query"])
def test_lengths_periods_and_letters(ctx, which, host):
    n, = check_block(ctx, which, tc.default_mode(), host=host)
    assert n > 100000


def test_dense_block_takes_the_full_copy(ctx):
    data, _ = tc.block(tc.dense())
    assert tc.total_masked(tc.dense()) > tc.capacity(data)
    check_block(ctx, hip.TARGET, tc.dense())
    check_block(ctx, hip.QUERY, tc.dense(), host=False)


@pytest.mark.parametrize("delta", [0, 1], ids=["list_exactly_full", "one_over"])
def test_position_list_at_its_capacity(ctx, delta):
    group = tc.cap_edge(delta)
    data, _ = tc.block(group)
    assert tc.total_masked(group) == tc.capacity(data) + delta
    check_block(ctx, hip.TARGET, group)


@pytest.mark.parametrize("name", sorted(tc.subsets()))
def test_subset_then_the_rest(ctx, name):
    check_block(ctx, hip.TARGET, tc.default_mode(), ids=tc.subsets()[name])


def test_subset_without_a_host_copy(ctx):
    check_block(ctx, hip.QUERY, tc.default_mode(), ids=tc.subsets()["listed_mix"], host=False)


@pytest.mark.parametrize("name", NAMES)
def test_every_matrix(name):
    p = hip.matrix_params(name)
    lib = hip.load()
    lib.dmnd_masking_lambda.restype = ctypes.c_double
    lam = lib.dmnd_masking_lambda(ctypes.byref(p))
    assert orc.tantan_lambda(hip.matrix_of(p)) == lam
    assert (lam == -1.0) == (name == "pam250")
    group = tc.periods() + tc.letters()
    c = hip.Context(params=p)
    try:
        n, = check_block(c, hip.TARGET, group, matrix=name)
    finally:
        c.close()
    assert n > 20000
    if name == "pam250":
        assert n > 0.5 * sum(len(s) for _, s in group)             # exp(-score): most letters count as repeats, as in the reference


# ---- forced kernel choice: one child process per mode ------------------------------------------------------------------------------

def forced_cases():
    """(name, group, ids) of the calls every child makes"""
    sub = tc.subsets()
    return [("corpus", tc.default_mode(), None), ("dense", tc.dense(), None), ("cap_edge0", tc.cap_edge(0), None), ("cap_edge1", tc.cap_edge(1), None),
            ("short65", tc.default_mode(), sub["short65"]), ("long3", tc.default_mode(), sub["long3"]), ("listed_mix", tc.default_mode(), sub["listed_mix"])]


def run_forced_cases():
    c = hip.Context()
    try:
        out = {name: check_block(c, hip.TARGET, group, ids=ids) for name, group, ids in forced_cases()}
        out["corpus_hbm_only"] = check_block(c, hip.QUERY, tc.default_mode(), host=False)
    finally:
        c.close()
    return out


CHILD = r"""
import sys
sys.path[:0] = {paths!r}
import json
import test_gpu_tantan_edges as t
print("ok", json.dumps(t.run_forced_cases()))
"""

TRACE_LINE = re.compile(r"^dmnd_mask_(?:block|sequences): (\d+) sequences \((\d+) long, > (\d+) letters\)", re.M)


@pytest.mark.parametrize("env", [{"DMND_TANTAN_WAVE": "1"}, {"DMND_TANTAN_LONG": "16"}, {"DMND_TANTAN_LONG": "128"}, {"DMND_TANTAN_LONG": "1000000"}],
                         ids=["wavefront_kernel_only", "split_at_16", "split_at_128", "lanes_kernel_only"])
def test_forced_kernel_choice(env):
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = CHILD.format(paths=[here, root, os.path.join(root, "oracle")])
    keep = {k: v for k, v in os.environ.items() if k not in ("DMND_TANTAN_WAVE", "DMND_TANTAN_LONG")}
    r = subprocess.run([sys.executable, "-c", code], env=dict(keep, DMND_TRACE="1", **env), cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads(r.stdout[3:])
    # the counts are the oracle's (the child asserted as much): so every mode masks what every other mode masks
    want, split = {}, []
    long_len = int(env.get("DMND_TANTAN_LONG", 0))
    for name, group, ids in forced_cases() + [("corpus_hbm_only", tc.default_mode(), None)]:
        counts = np.array([tc.masked(s)[1] for _, s in group])
        lens = np.array([len(s) for _, s in group])
        calls = [np.arange(len(group))] if ids is None else [ids, np.setdiff1d(np.arange(len(group)), ids)]
        want[name] = [int(counts[c].sum()) for c in calls]
        split += [(len(c), int((lens[c] > long_len).sum()) if long_len else 0, long_len) for c in calls]
    assert got == want
    # and the kernels were the forced ones: the library's own account of every call
    assert [tuple(int(x) for x in m) for m in TRACE_LINE.findall(r.stderr)] == split, r.stderr[-4000:]
    n, n_long, _ = split[0]
    if env == {"DMND_TANTAN_LONG": "128"}:
        assert n_long >= 200 and n - n_long >= 200                 # hundreds of sequences in each kernel in one call
    if env == {"DMND_TANTAN_LONG": "16"}:
        assert n_long >= 200 and n - n_long == 32                  # the sequences of 1 .. 16 letters alone in the lanes kernel
    if env == {"DMND_TANTAN_LONG": "1000000"}:
        assert n_long == 0 and lens.max() == 20000                 # the 5000- and 20000-letter sequences in the lanes kernel
