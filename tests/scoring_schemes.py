"""The scoring systems the kernel-level tests sweep: (matrix name, gap open, gap extend). Params and matrices come from the
library (hip.matrix_params, hip.matrix_of); no matrix is typed into a test.

 DEFAULTS  the eight matrices of --matrix with their default gap costs.
 EDGES     the largest and the smallest gap open, gap extend 3 with its smallest opens, and two rows far from their matrix's default.
 GPU       DEFAULTS + EDGES: what the GPU tests run, one context per system.
 TRACEBACK the three systems under which the traceback corpus (traceback_cases.py) is rebuilt.
 XDROP     the two systems under which the x-drop corpus (xdrop_cases.py) is rebuilt: their x-drop default is not BLOSUM62's 20.
 rows(name) / all_rows(): every (gap open, gap extend) the library accepts for a matrix -- the table of score_matrices.h read
           through hip.matrix_params, gap open 5 .. 25, gap extend 1 .. 3; a pair that raises is not a row. 82 rows in all."""
import functools

import numpy as np

from diamond_amd import hip

NAMES = ("blosum45", "blosum50", "blosum62", "blosum80", "blosum90", "pam30", "pam70", "pam250")
DEFAULTS = (("blosum45", 14, 2), ("blosum50", 13, 2), ("blosum62", 11, 1), ("blosum80", 10, 1), ("blosum90", 10, 1),
            ("pam30", 9, 1), ("pam70", 10, 1), ("pam250", 14, 2))
EDGES = (("blosum80", 25, 2), ("pam30", 5, 2), ("pam250", 11, 3), ("blosum50", 9, 3), ("pam250", 21, 1), ("blosum62", 6, 2))
GPU = DEFAULTS + EDGES
TRACEBACK = (("blosum80", 25, 2), ("pam30", 5, 2), ("pam250", 11, 3))
XDROP = (("pam30", 9, 1), ("blosum45", 14, 2))
GAP_OPENS, GAP_EXTENDS = range(5, 26), range(1, 4)
N_ROWS = 82


def scheme_id(scheme):
    return "%s-%d-%d" % tuple(scheme)


@functools.lru_cache(maxsize=None)
def params(scheme):
    """hip.Params of a scheme (a fresh copy per scheme, shared by its users: do not write to it)"""
    name, go, ge = scheme
    p = hip.matrix_params(name, go, ge)
    assert (p.gap_open, p.gap_extend) == (go, ge), scheme
    return p


@functools.lru_cache(maxsize=None)
def matrix(name):
    """the int8 32 x 32 matrix of a name, read-only"""
    m = hip.matrix_of(hip.matrix_params(name))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def rows(name):
    out = []
    for go in GAP_OPENS:
        for ge in GAP_EXTENDS:
            try:
                p = hip.matrix_params(name, go, ge)
            except hip.DiamondHipError:
                continue
            assert (p.gap_open, p.gap_extend) == (go, ge)
            out.append((go, ge))
    return tuple(out)


def all_rows():
    return tuple((name, go, ge) for name in NAMES for go, ge in rows(name))


def other_matrix(name):
    """another standard matrix for an item's own matrix in the context of `name`: the one five places on in NAMES (pam30 items
    go into the blosum45 context, blosum62 items into the pam30 context)"""
    return NAMES[(NAMES.index(name) + 5) % len(NAMES)]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------

GAPPED_BAND = (-40, 41)


def gapped_pair(rng):
    """The related pair with gaps: a query of 150 - 400 letters (0 - 19) and a copy with 15 % substitutions and two indels of
    1 - 8 letters each (extra letters or a cut, either with probability 1/2), both at least 40 letters from the ends and from
    each other. The diagonals [-40, 41) hold the alignment. A CPU run over all 14 systems of GPU aligns every such pair with a
    positive score and at least 99.5 % of them with a gap; the tests that use the recipe assert their own share from the oracle."""
    n = int(rng.integers(150, 401))
    q = rng.integers(0, 20, n).astype(np.int8)
    t = q.copy()
    mut = rng.random(n) < 0.15
    t[mut] = rng.integers(0, 20, int(mut.sum()))
    a = int(rng.integers(40, n - 100))
    b = int(rng.integers(a + 50, n - 48))
    parts, at = [], 0
    for p in (a, b):
        g = int(rng.integers(1, 9))
        if rng.random() < 0.5:                               # extra letters in the target: a deletion (diagonals move down)
            parts += [t[at:p], rng.integers(0, 20, g).astype(np.int8)]
            at = p
        else:                                                # letters cut from the target: an insertion
            parts.append(t[at:p])
            at = p + g
    parts.append(t[at:])
    return q, np.concatenate(parts)


def unrelated_pair(rng, lo=150, hi=401):
    return rng.integers(0, 20, int(rng.integers(lo, hi))).astype(np.int8), rng.integers(0, 20, int(rng.integers(lo, hi))).astype(np.int8)


def odd_letters(rng, q, t):
    """letters 20 - 24 on 3 % of the positions of both sequences and bit 7 on a tenth of them"""
    for s in (q, t):
        at = rng.random(len(s)) < 0.03
        s[at] = rng.integers(20, 25, int(at.sum())).astype(np.int8)
        at = rng.random(len(s)) < 0.1
        s[at] = (s[at].astype(np.uint8) | 0x80).astype(np.int8)


def bias(rng, n):
    return rng.integers(-3, 2, int(n)).astype(np.int8)


def geometry_item(rng, it):
    """the mix of test_emulated_wavefront_random_geometry: short sequences of all 25 letters, every second pair related by
    substitutions and one indel, a band anywhere across the matrix (also leaving it), a bias on two of three, bit 7 on one of five"""
    qlen = int(rng.integers(1, 200))
    q = rng.integers(0, 25, qlen).astype(np.int8)
    if it % 2 == 0:
        t = q.copy()
        mut = rng.random(qlen) < 0.3
        t[mut] = rng.integers(0, 20, int(mut.sum()))
        cut = int(rng.integers(0, qlen))
        t = np.concatenate([t[:cut], rng.integers(0, 20, int(rng.integers(0, 6))).astype(np.int8), t[cut + int(rng.integers(0, 4)):]])
        if len(t) == 0:
            t = q[:1].copy()
    else:
        t = rng.integers(0, 25, int(rng.integers(1, 200))).astype(np.int8)
    if it % 5 == 0:
        q[rng.integers(0, qlen)] |= -128
    d0 = int(rng.integers(-(len(t) - 1) - 5, qlen + 3))
    d1 = d0 + int(rng.integers(1, 140 if it % 7 else 300))
    if d1 <= -(len(t) - 1) or d0 >= qlen:
        d0, d1 = -2, 3
    return {"query": q, "cbs": bias(rng, qlen) if it % 3 else None, "target": t, "d_begin": d0, "d_end": d1}


def gapped_item(rng, it):
    """gapped_pair on its band [-40, 41), widened at random up to 96 / 160 / 300 diagonals; a bias on one of three"""
    q, t = gapped_pair(rng)
    extra = int(rng.integers(0, (16, 80, 220)[it % 3]))
    left = int(rng.integers(0, extra + 1))
    return {"query": q, "cbs": bias(rng, len(q)) if it % 3 == 1 else None, "target": t,
            "d_begin": GAPPED_BAND[0] - left, "d_end": GAPPED_BAND[1] + extra - left}


def emulator_items(seed, n=40):
    """n seeded items for one gap row of the emulator sweeps: three of the geometry mix, then one gapped item"""
    rng = np.random.default_rng(seed)
    return [gapped_item(rng, it) if it % 4 == 3 else geometry_item(rng, it) for it in range(n)]


def row_seed(name, go, ge):
    return 1000003 * NAMES.index(name) + 1009 * go + ge
