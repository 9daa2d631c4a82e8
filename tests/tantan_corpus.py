"""Test data of the tantan edge tests (tests/test_tantan_corpus.py, tests/test_gpu_tantan_edges.py): named groups of sequences
built from fixed seeds, laid at the places where the two masking kernels of csrc/mask_kernels.hip and the call around them
(mask_impl, csrc/mask_api.hip) change their path.

 lengths    every length 1 .. 130, then the lengths around 192, 256, 1024 (the default split between the lane-per-sequence and the
            wavefront-per-sequence kernel), 1040, 2048, and 5000 and 20000 letters -- each once with random letters and once as a
            perfect period-3 repeat, whose mask reaches as close to both ends as tantan allows;
 periods    a random unit of p = 1 .. 50, 51, 52, 64 letters repeated to max(6 p, 60) letters, clean and with 8 % substitutions:
            between random flanks of 80 letters, at offset 0, at the sequence end, across positions 63 | 64, and across positions
            1023 | 1024 of a 1100-letter sequence. The window has 50 offsets: a clean period of 51 or more is left alone;
 letters    runs of 60 of each non-standard letter 20 .. 25, a sequence of X (23) only, random sequences with 2 % X, a repeat with a
            run of X in its middle;
 dense      200 perfect repeats of 300 letters, periods 1 .. 7: nearly every letter masked, far above the capacity of the list of
            masked positions, so the host copy is copied back whole;
 cap_edge   a block whose masked letters number exactly that capacity (delta 0: the list is full) or one more (delta 1);
 threshold  repeats with a repeat probability within an ulp of the mask threshold (tests/golden/tantan_threshold.txt, found by
            tests/golden/make_tantan_threshold.py): one wrong rounding in the recurrences -- the 50 offsets summed in another order,
            a fused multiply-add -- changes their masks, and those of no other group. Part of the default-mode block.

A group is a list of (name, int8 letters). masked() is the oracle's answer (oracle/tantan.c), kept per sequence and matrix."""
import functools
import os

import numpy as np

import oracle_py as orc
from diamond_amd import hip, workload

FLANK = 80
EDGE_LENGTHS = list(range(1, 131)) + [191, 192, 193, 255, 256, 257, 1023, 1024, 1025, 1039, 1040, 1041, 2047, 2048, 2049, 5000, 20000]
PERIODS = list(range(1, 51)) + [51, 52, 64]
PLACEMENTS = ("mid", "start", "end", "at64", "at1024")
SPLIT = 1024                       # mask_impl: long_len = max(1024, letters / 45000); longer sequences go to the wavefront kernel
X = 23


def _letters(rng, n):
    return rng.integers(0, 20, int(n)).astype(np.int8)


@functools.lru_cache(maxsize=None)
def lengths():
    rng = np.random.default_rng(101)
    out = []
    for n in EDGE_LENGTHS:
        out.append(("len%d.random" % n, _letters(rng, n)))
        out.append(("len%d.period3" % n, np.resize(rng.permutation(20)[:3].astype(np.int8), n)))
    return out


def repeat_of(p, subs):
    """The repeat of period p that all placements of periods() share: a random unit repeated to max(6 p, 60) letters."""
    rng = np.random.default_rng([202, p, int(subs)])
    r = np.resize(_letters(rng, p), max(6 * p, 60))
    if subs:
        flip = rng.random(len(r)) < 0.08
        r[flip] = _letters(rng, int(flip.sum()))
    return r


def placed(p, subs, where):
    """(sequence, first position of the repeat)"""
    r = repeat_of(p, subs)
    R = len(r)
    rng = np.random.default_rng([303, p, int(subs), PLACEMENTS.index(where)])
    if where == "mid":
        a, tail = FLANK, FLANK
    elif where == "start":
        a, tail = 0, FLANK
    elif where == "end":
        a, tail = FLANK, 0
    elif where == "at64":
        a, tail = max(1, 64 - R // 2), FLANK
        assert a <= 63 and a + R > 64
    else:
        right = min(R // 2, 70)                           # letters of the repeat from position 1024 on
        a = 1024 + right - R
        tail = 1100 - a - R
        assert 0 < a <= 1023 and a + R > 1024 and tail > 0
    return np.concatenate([_letters(rng, a), r, _letters(rng, tail)]), a


@functools.lru_cache(maxsize=None)
def periods():
    return [("period%d.%s.%s" % (p, "subs" if subs else "clean", where), placed(p, subs, where)[0])
            for p in PERIODS for subs in (False, True) for where in PLACEMENTS]


LETTER_RUN = 60


@functools.lru_cache(maxsize=None)
def letters():
    rng = np.random.default_rng(404)
    out = []
    for l in range(20, 26):                               # the run stands at [FLANK, FLANK + LETTER_RUN)
        out.append(("run_of_%d" % l, np.concatenate([_letters(rng, FLANK), np.full(LETTER_RUN, l, np.int8), _letters(rng, FLANK)])))
    out.append(("x_only", np.full(150, X, np.int8)))
    for k, n in enumerate([100, 130, 160, 190, 220, 250, 280, 310, 340, 370, 400, 64, 65, 1500, 1025, 1024]):
        s = _letters(rng, n)
        s[rng.random(n) < 0.02] = X
        out.append(("random%d_with_x.%d" % (n, k), s))
    r = np.resize(_letters(rng, 4), 120)
    r[50:70] = X
    out.append(("repeat_with_x_run", np.concatenate([_letters(rng, FLANK), r, _letters(rng, FLANK)])))
    return out


ALPHABET = "ARNDCQEGHILKMFPSTWYVBJZX*_"


@functools.lru_cache(maxsize=None)
def threshold_cases():
    """[(name, the wrong roundings of orc.tantan_mask_wrong that change the mask, letters)]"""
    out = []
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tantan_threshold.txt")) as f:
        for line in f:
            if not line.startswith("#"):
                name, wrong, text = line.rstrip("\n").split("\t")
                out.append((name, tuple(int(v) for v in wrong.split(",")), np.array([ALPHABET.index(c) for c in text], np.int8)))
    return out


def threshold():
    return [(name, s) for name, _, s in threshold_cases()]


def default_mode():
    """the groups of the default-mode block"""
    return lengths() + periods() + letters() + threshold()


@functools.lru_cache(maxsize=None)
def dense():
    rng = np.random.default_rng(505)
    return [("dense%d.period%d" % (k, 1 + k % 7), np.resize(_letters(rng, 1 + k % 7), 300)) for k in range(200)]


def capacity(data):
    """The capacity of the list of masked positions that patches the host copy, as mask_impl (csrc/mask_api.hip) sizes it:
        pos_cap = raw / 16 + 1024                    (raw = the bytes of the block, padding included)
        if (n_pos <= pos_cap) patch the host copy from the list; else copy the whole block back
    A change of that formula must break cap_edge() and its tests, not silently move them off the edge."""
    return len(data) // 16 + 1024


@functools.lru_cache(maxsize=None)
def cap_edge(delta):
    """40 repeats of 120 letters and random sequences that tantan leaves alone, M masked letters in all, in a block of
    16 (M - 1024 - delta) bytes: M = capacity + delta."""
    rng = np.random.default_rng(606)
    out = [("cap%d.repeat%d" % (delta, k), np.resize(_letters(rng, 1 + k % 7), 120)) for k in range(40)]
    m = sum(masked(s)[1] for _, s in out)
    target = 16 * (m - 1024 - delta)
    room = target - 512 - sum(len(s) + 1 for _, s in out)   # bytes left; every sequence takes its letters and one delimiter
    assert room > 2
    while room > 0:
        n = 400 if room >= 403 else room - 1              # never leaves room for a delimiter alone
        for _ in range(100):
            s = _letters(rng, n)
            if masked(s)[1] == 0:
                break
        else:
            raise AssertionError("no unmasked random sequence of %d letters" % n)
        out.append(("cap%d.pad%d" % (delta, len(out)), s))
        room -= n + 1
    assert room == 0
    return out


@functools.lru_cache(maxsize=None)
def subsets():
    """Named id lists into default_mode() for dmnd_mask_sequences: the group remainders of the lanes kernel (64 sequences to a
    wavefront) among sequences it takes, the grid remainders of the wavefront kernel (4 sequences to a workgroup) among sequences
    only it takes -- the lanes launch is then skipped --, one kernel's share alone, orders other than ascending, and a mix for both
    kernels that stays below the capacity of the position list."""
    group = default_mode()
    lens = np.array([len(s) for _, s in group])
    rng = np.random.default_rng(707)
    short, long_ = rng.permutation(np.flatnonzero(lens <= SPLIT)), rng.permutation(np.flatnonzero(lens > SPLIT))
    names = [n for n, _ in group]
    first = [names.index(n) for n in ("len5000.period3", "len20000.random", "len1025.period3", "period50.clean.at1024", "len2049.random")]
    long_ = np.concatenate([first, [i for i in long_ if i not in first]])
    out = {}
    for k in (1, 63, 64, 65, 129):
        out["short%d" % k] = short[:k]
    for k in (1, 2, 3, 5):
        out["long%d" % k] = long_[:k]
    out["all_short"] = np.flatnonzero(lens <= SPLIT)
    out["all_long"] = np.flatnonzero(lens > SPLIT)
    out["descending"] = np.arange(len(group))[::-1]
    out["shuffled"] = rng.permutation(len(group))[: len(group) // 2]
    out["listed_mix"] = np.array([i for i, (n, _) in enumerate(group) if "random" in n or n.endswith("clean.at1024") or n.endswith("clean.mid")])
    return {k: np.ascontiguousarray(v, dtype=np.int64) for k, v in out.items()}


def everything():
    return default_mode() + dense() + cap_edge(0) + cap_edge(1)


def block(group):
    """(data, limits) of a group in the SequenceSet layout"""
    seqs = [s for _, s in group]
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return workload.sequence_set(np.concatenate(seqs).astype(np.int8), off)


@functools.lru_cache(maxsize=None)
def likelihood_ratios(matrix="blosum62"):
    return orc.tantan_matrix(hip.matrix_of(hip.matrix_params(matrix)))


_masked = {}


def masked(seq, matrix="blosum62"):
    """(masked letters, number of masked letters) by the oracle; not to be written to"""
    key = (matrix, seq.tobytes())
    if key not in _masked:
        m, k = orc.tantan_mask(seq, likelihood_ratios(matrix))
        m.setflags(write=False)
        _masked[key] = (m, int(k))
    return _masked[key]


def total_masked(group, matrix="blosum62"):
    return sum(masked(s, matrix)[1] for _, s in group)
