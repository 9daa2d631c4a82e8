"""The conditions that keep tests/test_gpu_tantan_edges.py from passing vacuously, asserted on tests/tantan_corpus.py with the oracle
alone (oracle/tantan.c, pinned on the reference's tap by tests/test_oracle_tantan.py): the repeats that must be masked are, the
periods beyond the window are not, the blocks built for the capacity of the position list stand exactly on it, both kernels get
sequences in the default mode -- and the lane emulator of the wavefront kernel agrees with the oracle on every sequence. CPU only."""
import ctypes

import numpy as np
import pytest

import emu_py as emu
import oracle_py as orc
import tantan_corpus as tc
from diamond_amd import hip
from test_matrices import NAMES
from test_oracle_seed import blosum62_matrix8


def test_the_corpus_is_small_and_named_once():
    group = tc.everything()
    names = [n for n, _ in group]
    assert len(set(names)) == len(names)
    assert len(group) <= 1500 and sum(len(s) for _, s in group) < 10 ** 6
    assert all(s.dtype == np.int8 and len(s) > 0 and 0 <= s.min() and s.max() < 26 for _, s in group)
    assert np.array_equal(hip.matrix_of(hip.matrix_params("blosum62")), blosum62_matrix8())
    got = {len(s) for _, s in tc.lengths()}
    assert got == set(tc.EDGE_LENGTHS) and len(tc.lengths()) == 2 * len(tc.EDGE_LENGTHS)


def test_periods_up_to_the_window_are_masked_and_longer_ones_are_not():
    for p in tc.PERIODS:
        for where in tc.PLACEMENTS:
            s, a = tc.placed(p, False, where)
            m, k = tc.masked(s)
            R = len(tc.repeat_of(p, False))
            inside = int((m[a:a + R] != s[a:a + R]).sum())
            if p <= 50:
                assert inside > 0, (p, where)
            else:
                assert k == 0 and np.array_equal(m, s), (p, where)         # neither the repeat nor, by the choice of seeds, the flanks
    # the repeats with substitutions are not all lost either
    assert sum(tc.masked(tc.placed(p, True, "mid")[0])[1] > 0 for p in range(1, 51)) >= 40
    # the placements are where their names say
    for p in (1, 7, 50, 64):
        R = len(tc.repeat_of(p, False))
        assert tc.placed(p, False, "start")[1] == 0 and tc.placed(p, False, "end")[1] + R == len(tc.placed(p, False, "end")[0])
        a = tc.placed(p, False, "at64")[1]
        assert a <= 63 and a + R > 64
        s, a = tc.placed(p, False, "at1024")
        assert len(s) == 1100 and a <= 1023 and a + R > 1024
        if p <= 50:
            m = tc.masked(s)[0]
            assert m[1023] == 23 and m[1024] == 23                           # the mask itself crosses the default split length


def test_non_standard_letters_in_runs():
    group = dict(tc.letters())
    run = slice(tc.FLANK, tc.FLANK + tc.LETTER_RUN)
    in_run = {}
    for l in range(20, 26):
        s = group["run_of_%d" % l]
        assert (s[run] == l).all()
        m, k = tc.masked(s)
        in_run[l] = int((m[run] == 23).sum()) if l != 23 else k
    print(in_run)
    for l in (20, 21, 22, 24):
        assert in_run[l] >= tc.LETTER_RUN // 2, in_run
    for l in (23, 25):
        assert tc.masked(group["run_of_%d" % l])[1] == 0, in_run
    m, k = tc.masked(group["repeat_with_x_run"])
    assert k > 40
    assert sum((s == 23).sum() > 0 for n, s in tc.letters() if n.startswith("random")) >= 10


def test_threshold_cases_change_their_mask_under_one_wrong_rounding():
    """What gives the mask comparisons on the device their hold on the ARITHMETIC: on these sequences the oracle with the 50
    offsets summed in another order (forward: 1, backward: 2) or with a fused multiply-add (3) masks other letters than the
    oracle proper -- and on no sequence of the other groups of the default-mode block, which is why they are here."""
    lr = tc.likelihood_ratios()
    cases = tc.threshold_cases()
    per_wrong = {v: 0 for v in (1, 2, 3)}
    for name, wrong, s in cases:
        right = tc.masked(s)[0]
        assert np.array_equal(orc.tantan_mask_wrong(s, lr, 0)[0], right), name
        assert len(s) <= tc.SPLIT and 0 < tc.masked(s)[1] < len(s), name
        for v in (1, 2, 3):
            assert (not np.array_equal(orc.tantan_mask_wrong(s, lr, v)[0], right)) == (v in wrong), (name, v)
            per_wrong[v] += v in wrong
    assert min(per_wrong.values()) >= 4, per_wrong
    others = tc.lengths() + tc.periods() + tc.letters()
    assert all(np.array_equal(orc.tantan_mask_wrong(s, lr, 1)[0], tc.masked(s)[0]) for _, s in others)


def test_dense_exceeds_the_capacity_of_the_position_list():
    data, _ = tc.block(tc.dense())
    m = tc.total_masked(tc.dense())
    print(m, len(data), tc.capacity(data))
    assert m > 4 * tc.capacity(data)
    assert len(tc.dense()) == 200 and all(len(s) == 300 for _, s in tc.dense())


@pytest.mark.parametrize("delta", [0, 1])
def test_cap_edge_hits_its_count_exactly(delta):
    group = tc.cap_edge(delta)
    data, limits = tc.block(group)
    m = tc.total_masked(group)
    print(m, len(data), tc.capacity(data))
    assert m == tc.capacity(data) + delta == len(data) // 16 + 1024 + delta
    assert m > 4000 and sum(".repeat" in n for n, _ in group) == 40
    assert all(tc.masked(s)[1] == 0 for n, s in group if ".pad" in n)
    assert len(data) < 1 << 32                                  # below that the list is used at all


def test_both_kernels_get_sequences_in_the_default_mode():
    group = tc.default_mode()
    assert len(group) == len(tc.lengths()) + len(tc.periods()) + len(tc.letters()) + len(tc.threshold())
    data, _ = tc.block(group)
    assert max(1024, len(data) // 45000) == tc.SPLIT            # mask_impl's long_len for this block
    lens = np.array([len(s) for _, s in group])
    long_masked = sum(tc.masked(s)[1] > 0 for _, s in group if len(s) > tc.SPLIT)
    short_masked = sum(tc.masked(s)[1] > 0 for _, s in group if len(s) <= tc.SPLIT)
    assert (lens > tc.SPLIT).sum() >= 15 and (lens <= tc.SPLIT).sum() >= 15
    assert long_masked >= 15 and short_masked >= 15
    # the whole block masks more letters than the position list holds: the list path with both kernels in one call is the
    # share of a subset
    cap = tc.capacity(data)
    assert tc.total_masked(group) > cap
    sub = tc.subsets()
    count = lambda ids: sum(tc.masked(group[i][1])[1] for i in ids)
    mix = sub["listed_mix"]
    assert (lens[mix] > tc.SPLIT).sum() >= 15 and (lens[mix] <= tc.SPLIT).sum() >= 15 and 5000 < count(mix) < cap
    assert count(sub["shuffled"]) > cap
    for k in (1, 63, 64, 65, 129):
        assert len(sub["short%d" % k]) == k and (lens[sub["short%d" % k]] <= tc.SPLIT).all()
    for k in (1, 2, 3, 5):
        assert len(sub["long%d" % k]) == k and (lens[sub["long%d" % k]] > tc.SPLIT).all() and count(sub["long%d" % k]) < cap
    assert count(sub["long5"]) > 0 and count(sub["short63"]) > 0
    assert all(len(np.unique(v)) == len(v) for v in sub.values())


@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_and_the_library_derive_the_same_lambda(name):
    """Two implementations of the matrix scale (oracle_tantan_lambda, dmnd_masking_lambda) and of exp(lambda * score)."""
    p = hip.matrix_params(name)
    lib = hip.load()
    lib.dmnd_masking_lambda.restype = ctypes.c_double
    want, got = orc.tantan_lambda(hip.matrix_of(p)), lib.dmnd_masking_lambda(ctypes.byref(p))
    print(name, repr(want), repr(got))
    assert want == got
    if name == "pam250":
        assert got == -1.0


def test_lane_emulator_equals_the_oracle_on_the_whole_corpus():
    p = emu.tantan_params()
    lr = tc.likelihood_ratios()
    for name, s in tc.everything():
        want, k = tc.masked(s)
        got, n = emu.tantan_mask(p, lr, s)
        assert n == k and np.array_equal(got, want), name
