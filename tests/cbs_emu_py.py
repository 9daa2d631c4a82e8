"""TEST INFRASTRUCTURE ONLY -- ctypes view of the lane emulator of the matrix-adjustment kernel (tests/emu/cbs_emu.cpp, built into
tests/emu/libswipe_emu.so): one (query, target) pair through the kernel's 64-lane schedule with glibc's libm, and through the
host arithmetic with its trace."""
import ctypes
import numpy as np

import emu_py

ST_DEVICE, ST_ROUNDING, ST_ITERATIONS, ST_RULE = 0, 1, 2, 3
RULE_NONE, RULE_SCALE_OLD, RULE_REL_ENTROPY = -1, 0, 4
UNTOUCHED = 0x55          # the pattern matrices are pre-filled with: the kernel writes a table only with status 0
_TRACE = 3 + 256 + 1


def guards():
    """(eps_round, eps_norm, eps_angle, device iteration cap) as compiled into cbs_core.h."""
    out = np.zeros(4)
    emu_py.lib().emu_cbs_guards(out.ctypes.data_as(ctypes.c_void_p))
    return float(out[0]), float(out[1]), float(out[2]), int(out[3])


def _args(query_comp, target):
    return np.ascontiguousarray(query_comp, dtype=np.float64), np.ascontiguousarray(target, dtype=np.int8)


def pair(params, mode, query_comp, query_true_aa, target, max_its=0):
    """-> dict(rule, status, matrix int8[32, 32] (UNTOUCHED where no table was written), scores float64[21, 21] (NaN where none),
    angle, its, rnorm float64[tests])."""
    v = ctypes.c_void_p
    qc, t = _args(query_comp, target)
    rule, status = ctypes.c_int32(99), ctypes.c_uint8(99)
    m = np.full((32, 32), UNTOUCHED, np.int8)
    sc = np.full((21, 21), np.nan)
    tr = np.zeros(_TRACE)
    rc = emu_py.lib().emu_cbs_pair(ctypes.byref(params), int(mode), int(max_its), qc.ctypes.data_as(v), int(query_true_aa), t.ctypes.data_as(v), len(t),
                                   ctypes.byref(rule), ctypes.byref(status), m.ctypes.data_as(v), sc.ctypes.data_as(v), tr.ctypes.data_as(v))
    assert rc == 0
    return dict(rule=rule.value, status=status.value, matrix=m, scores=sc, angle=tr[0], its=int(tr[1]), rnorm=tr[3:3 + int(tr[2])].copy())


def host_pair(params, mode, query_comp, query_true_aa, target):
    """The host arithmetic on the same pair -> dict(rule, matrix, scores (NaN where the optimisation did not converge or the rule is
    not REL_ENTROPY), angle, its, rnorm, converged)."""
    v = ctypes.c_void_p
    qc, t = _args(query_comp, target)
    rule = ctypes.c_int32(99)
    m = np.full((32, 32), UNTOUCHED, np.int8)
    sc = np.full((21, 21), np.nan)
    tr = np.zeros(_TRACE)
    rc = emu_py.lib().emu_cbs_host_pair(ctypes.byref(params), int(mode), qc.ctypes.data_as(v), int(query_true_aa), t.ctypes.data_as(v), len(t),
                                        ctypes.byref(rule), m.ctypes.data_as(v), sc.ctypes.data_as(v), tr.ctypes.data_as(v))
    assert rc == 0
    return dict(rule=rule.value, matrix=m, scores=sc, angle=tr[0], its=int(tr[1]), rnorm=tr[3:3 + int(tr[2])].copy(), converged=bool(tr[3 + 256]))


def edge_pairs(rng=None):
    """The structural edge cases of the device form's tests, as (name, query letters int8[], target letters int8[]): target lengths
    around the high_pair threshold and the composition count's lane boundaries, a long target, mask letters only, one residue
    repeated, letters 20 - 25 and letters with bit 7 set, a query of one residue."""
    rng = rng or np.random.default_rng(20)
    bg = np.array([7.4, 5.2, 4.5, 5.3, 2.5, 3.4, 5.4, 7.4, 2.6, 6.8, 9.9, 5.8, 2.5, 4.7, 3.9, 5.7, 5.1, 1.3, 3.2, 7.3])
    bg = bg / bg.sum()

    def seq(n, p=bg):
        return rng.choice(20, size=n, p=p).astype(np.int8)
    skew = bg.copy()
    skew[[3, 6]] *= 6
    skew /= skew.sum()
    q = seq(180)
    out = []
    for n in (1, 2, 49, 50, 51, 63, 64, 65, 127, 128, 129):
        out.append(("len%d" % n, q, seq(n)))
        out.append(("len%d_skew" % n, q, seq(n, skew)))
    out.append(("len5000", q, seq(5000)))
    out.append(("mask_only", q, np.full(30, 23, np.int8)))
    out.append(("one_residue", q, np.full(80, 9, np.int8)))
    t = seq(90)
    t[::7] = np.resize(np.arange(20, 26, dtype=np.int8), len(t[::7]))
    out.append(("letters_20_25", q, t))
    t = seq(90)
    t[::3] |= np.int8(-128)
    out.append(("bit7", q, t))
    out.append(("query_one_residue", np.array([11], np.int8), seq(70)))
    out.append(("skew_query", seq(300, skew), seq(60)))
    return out
