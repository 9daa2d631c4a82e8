"""CPU checks of the HSP filter values of a translated (blastx) HSP (diamond_amd/csrc/filter_core.h filter_values_contexts: the one
statement of the rule the host path and the filter kernel of the device half both call), via tests/emu/libswipe_emu.so.

The expected values are a restatement of the reference in Python floats (IEEE doubles), compared for exact equality:
  filter_hsp, src/align/culling.cpp:147-170: qcov = hsp.query_cover_percent(source_query_len), tcov = hsp.subject_cover_percent(subject_len),
    id_percent() < min_id, approx_id < approx_min_id
  Hsp::query_cover_percent (src/basic/match.h:213-216): (double)query_source_range.length() * 100 / query_source_len -- for a translated
    query the source range is in bases, 3 x the translated range, and the source length the DNA read's
  Hsp::subject_cover_percent: (double)subject_range.length() * 100 / subject_len; Hsp::id_percent: (double)identities * 100.0 / (double)length
  Stats::approx_id (src/stats/stats.cpp:113-118) with one fused multiply-add, 100 for identical ranges.
Cases: reads of 200, 201 and 202 bases (context lengths 66/66/66, 67/66/66, 67/67/66), an HSP in each of the six frames, ranges of one
letter and of the whole context, one context (what filter_values gives a protein call), HSPs whose verdict under --query-cover is
another with 'range over the read length' than with '3 x range over the read length', a value on a threshold and one 2e-9 away."""
import ctypes
from fractions import Fraction

import pytest

import emu_py as emu

READS = (200, 201, 202)
CONTEXT_LENS = {200: (66, 66, 66), 201: (67, 66, 66), 202: (67, 67, 66)}


def _lib():
    lib = emu.lib()
    out = ctypes.POINTER(ctypes.c_double)
    lib.emu_ftr_values.argtypes = [ctypes.c_int] * 11 + [out]
    lib.emu_ftr_values.restype = None
    lib.emu_ftr_values_protein.argtypes = [ctypes.c_int] * 9 + [out]
    lib.emu_ftr_values_protein.restype = None
    lib.emu_ftr_verdict.argtypes = [ctypes.c_double] * 4 + [ctypes.c_int] * 11
    return lib


def context_len(read_len, frame):
    """letters of reading frame `frame` (0-2 forward, 3-5 reverse) of a read"""
    return (read_len - frame % 3) // 3


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))      # exact product and sum, rounded once


def ref_values(score, identities, length, q_begin, q_end, s_begin, s_end, contexts, ctx_len, read_len, target_len):
    """(identity, approximate identity, query cover, subject cover) as the reference computes them"""
    q_range, s_range = q_end - q_begin, s_end - s_begin
    ident = float(identities) * 100.0 / float(length)
    if q_range == s_range and identities == length:
        approx = 100.0
    else:
        m = max(q_range, s_range)
        approx = 100.0 if m == 0 else min(max(_fma(float(score) / float(m), 16.56, 11.41), 0.0), 100.0)
    source_range, source_len = (q_range, ctx_len) if contexts == 1 else (3 * q_range, read_len)
    return ident, approx, float(source_range) * 100 / source_len, float(s_range) * 100 / target_len


def values(lib, *hsp):
    out = (ctypes.c_double * 4)()
    lib.emu_ftr_values(*hsp, out)
    return tuple(out)


def test_context_lengths_of_the_three_read_lengths():
    for r in READS:
        assert tuple(context_len(r, f) for f in range(3)) == CONTEXT_LENS[r] == tuple(context_len(r, f) for f in range(3, 6))


@pytest.mark.parametrize("read_len", READS)
@pytest.mark.parametrize("frame", range(6))
def test_translated_values_equal_the_reference_arithmetic(read_len, frame):
    lib = _lib()
    n = context_len(read_len, frame)
    tlen = 97
    ranges = [(0, 1), (n - 1, n), (0, n), (5, 48), (n // 2, n // 2 + 1), (3, n - 2)]      # one letter (first, last, middle), the whole context, inner ranges
    for qb, qe in ranges:
        for sb, se in ((0, qe - qb), (7, 7 + (qe - qb) + 3), (0, tlen)):
            if se > tlen:
                continue
            length = max(qe - qb, se - sb)
            for identities in sorted({length, max(length * 2 // 3, 1), 1}):
                for score in (1, 37, 5 * (qe - qb)):
                    hsp = (score, identities, length, qb, qe, sb, se, 6, n, read_len, tlen)
                    assert values(lib, *hsp) == ref_values(*hsp), hsp
    # the whole context of frame 0 of a read that is a multiple of 3 long covers it all; the cover never exceeds 100
    whole = values(lib, 300, n, n, 0, n, 0, n, 6, n, read_len, tlen)
    assert whole[2] == float(3 * n) * 100 / read_len <= 100.0 and (whole[2] == 100.0) == (3 * n == read_len)
    assert whole[1] == 100.0


def test_one_context_gives_what_filter_values_gives_a_protein_call():
    lib = _lib()
    out = (ctypes.c_double * 4)()
    for qlen in (66, 67, 300):
        for qb, qe in ((0, 1), (0, qlen), (10, 60)):
            for read_len in (0, 1, 200, 12345):                 # (ignored with one context)
                hsp = (123, 30, qe - qb + 2, qb, qe, 4, 4 + (qe - qb) + 2)
                lib.emu_ftr_values_protein(*hsp, qlen, 150, out)
                want = tuple(out)
                assert values(lib, *hsp, 1, qlen, read_len, 150) == want == ref_values(*hsp, 1, qlen, read_len, 150)
                assert want[2] == float(qe - qb) * 100 / qlen


def test_translated_cover_without_read_lengths_is_measured_against_one():
    lib = _lib()
    v = values(lib, 50, 20, 20, 3, 23, 0, 20, 6, 66, 0, 40)
    assert v[2] == float(60) * 100 / 1 and v[3] == 50.0


def test_query_cover_verdict_is_that_of_three_times_the_range_over_the_read_length():
    lib = _lib()
    verdict = lambda qcov, hsp: lib.emu_ftr_verdict(0, 0, qcov, 0, *hsp)
    wrong = lambda qcov, hsp: int(float(hsp[4] - hsp[3]) * 100 / hsp[9] < qcov)      # 'range over the read length'
    a = (150, 40, 50, 2, 52, 0, 50, 6, 67, 201, 60)             # 150 of 201 bases: 74.6 %; its 50 letters are 24.9 % of 201
    b = (60, 15, 21, 40, 61, 0, 21, 6, 66, 201, 60)             # 63 of 201 bases: 31.3 %; 10.4 %
    assert [verdict(30.13, a), verdict(30.13, b)] == [0, 0] and [wrong(30.13, a), wrong(30.13, b)] == [1, 1]
    assert [verdict(70.13, a), verdict(70.13, b)] == [0, 1] and [wrong(70.13, a), wrong(70.13, b)] == [1, 1]
    assert [verdict(20.13, a), verdict(20.13, b)] == [0, 0] and [wrong(20.13, a), wrong(20.13, b)] == [0, 1]
    # ... and not that of the range over the context's length either (21 of 66 letters = 31.8 %, 63 of 201 bases = 31.3 %)
    assert verdict(31.5, b) == 1 and float(21) * 100 / 66 > 31.5


def test_value_on_a_threshold_and_next_to_it():
    lib = _lib()
    hsp = (150, 60, 100, 0, 50, 0, 90, 6, 66, 200, 120)          # identity 60 %, query cover 150 / 200 = 75 %, subject cover 75 %
    v = values(lib, *hsp)
    assert v[0] == 60.0 and v[2] == 75.0 and v[3] == 75.0
    for slot, x in ((0, 60.0), (2, 75.0), (3, 75.0)):
        t = [0.0, 0.0, 0.0, 0.0]
        t[slot] = x
        assert lib.emu_ftr_verdict(*t, *hsp) == 2                # on the threshold: not decided on the device
        t[slot] = x * (1 - 1e-10)
        assert lib.emu_ftr_verdict(*t, *hsp) == 2                # within 1e-9 relative: still not decided
        t[slot] = x * (1 + 2e-9)
        assert lib.emu_ftr_verdict(*t, *hsp) == 1                # 2e-9 above: decided, removed
        t[slot] = x * (1 - 2e-9)
        assert lib.emu_ftr_verdict(*t, *hsp) == 0                # 2e-9 below: decided, kept
    approx = v[1]
    assert 0 < approx < 100
    assert lib.emu_ftr_verdict(0, approx, 0, 0, *hsp) == 2 and lib.emu_ftr_verdict(0, approx * (1 + 2e-9), 0, 0, *hsp) == 1
    assert lib.emu_ftr_verdict(0, approx * (1 - 2e-9), 0, 0, *hsp) == 0
