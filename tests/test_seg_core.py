"""CPU checks of the device form of SEG (diamond_amd/csrc/seg_core.h, via tests/emu/seg_emu.cpp in tests/emu/libswipe_emu.so) against the
host statement (seg_mask.h) and the reference's own SEG (the goldens minted from oracle/_ref/seg_ref): the class table, the candidate
form of the trim step, and the driver with its one saved frame."""
import ctypes
import functools
import gzip
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
AA = "ARNDCQEGHILKMFPSTWYVBJZX*_"
CODE = {c: i for i, c in enumerate(AA)}
NONE, TRIGGER, EXTEND, BREAK = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def emu():
    return ctypes.CDLL(os.path.join(HERE, "emu", "libswipe_emu.so"))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _fasta(text):
    for r in text.split(">")[1:]:
        h, *s = r.strip().split("\n")
        yield h.split()[0], np.array([CODE.get(c, 23) for c in "".join(s).upper()], np.int8)


def _tsv(path):
    for line in gzip.open(path, "rt"):
        f = line.rstrip("\n").split("\t")
        yield f[0], [tuple(int(x) for x in r.split("-")) for r in f[1:]]


@functools.lru_cache(maxsize=None)
def fixtures():
    """[(name, letters, golden ranges)] of the three SEG fixtures: the reference's ctest proteins, the synthetic cases, the device cases."""
    seqs = list(_fasta(open(os.path.join(GOLDEN, "ref_ctest", "data.faa")).read()))
    seqs += list(_fasta(gzip.open(os.path.join(GOLDEN, "seg_cases.faa.gz"), "rt").read()))
    gold = list(_tsv(os.path.join(GOLDEN, "seg_golden.tsv.gz")))
    seqs += list(_fasta(gzip.open(os.path.join(GOLDEN, "seg_device_cases.faa.gz"), "rt").read()))
    gold += list(_tsv(os.path.join(GOLDEN, "seg_device_golden.tsv.gz")))
    assert [n for n, _ in seqs] == [n for n, _ in gold]
    return [(n, s, g) for (n, s), (_, g) in zip(seqs, gold)]


@functools.lru_cache(maxsize=None)
def emulated():
    """Per fixture sequence: (ranges, raw segments [(left, len)], stats [trims, remainder searches, most segments in one, handed back])."""
    out = []
    for _, s, _ in fixtures():
        ranges, raw, st = np.zeros(2 * 4096, np.int32), np.zeros(2 * 8192, np.int32), np.zeros(4, np.int32)
        n, n_raw = ctypes.c_int32(0), ctypes.c_int32(0)
        rc = emu().emu_seg_ranges(_ptr(s), len(s), _ptr(ranges), 4096, ctypes.byref(n), _ptr(raw), 8192, ctypes.byref(n_raw), _ptr(st))
        assert rc == 0
        out.append(([(int(ranges[2 * i]), int(ranges[2 * i + 1])) for i in range(n.value)],
                    [(int(raw[2 * i]), int(raw[2 * i + 1])) for i in range(n_raw.value)], [int(x) for x in st]))
    return out


def test_the_device_fixture_holds_the_cases_it_was_made_for():
    names = {n for n, _ in _tsv(os.path.join(GOLDEN, "seg_device_golden.tsv.gz"))}
    fx = [(n, s, g) for n, s, g in fixtures() if n in names]
    stats = {n: e[2] for (n, _, _), e in zip(fixtures(), emulated())}
    assert 200 <= len(fx) <= 400
    assert sum(stats[n][1] > 0 for n, _, _ in fx) >= 50                    # the left remainder of a trim is searched again
    assert sum(stats[n][2] > 1 for n, _, _ in fx) >= 1                     # ... and holds more than one segment
    assert sum(any(g[i + 1][0] <= g[i][1] for i in range(len(g) - 1)) for _, _, g in fx) >= 20      # overlapping neighbours
    assert {9, 10, 11, 63, 64, 65, 127, 128, 129} <= {len(s) for _, s, _ in fx}
    by_name = {n: (s, g) for n, s, g in fx}
    bogus = lambda s, x: int(np.sum((s[x:x + 10] & 31) >= 20))
    s2, g2 = by_name["bogus2_only_180"]
    s3, g3 = by_name["bogus3_only_181"]
    assert bogus(s2, 0) == 2 and g2 == [(0, 9)] and bogus(s3, 0) == 3 and g3 == []
    assert any(np.all(s == 23) and len(s) >= 50 and g == [] for _, s, g in fx)
    assert any(len(s) == 10050 and g == [(0, 10049)] and stats[n][3] == 1 for n, s, g in fx)       # above the ln n! table: handed back
    assert sum(st[3] for st in stats.values()) == 1


def test_class_table_equals_the_entropy_of_every_state_vector():
    cap = 256
    states = np.zeros((cap, 11), np.int32)
    by_key, by_window, by_entropy = (np.zeros(cap, np.uint8) for _ in range(3))
    n = emu().emu_seg_class_states(_ptr(states), _ptr(by_key), _ptr(by_window), _ptr(by_entropy), cap)
    assert n == 22 + 30 + 42                                               # the partitions of 8, 9 and 10: no two share a key
    assert sorted(set(states[:n].sum(axis=1).tolist())) == [8, 9, 10]
    assert len({tuple(r) for r in states[:n].tolist()}) == n
    for k in range(n):
        sv = [int(x) for x in states[k] if x]
        total = sum(sv)
        h = abs(sum(c * np.log(c / total) / 0.69314718055994530941723212145818 for c in sv) / total)
        want = TRIGGER if h <= 1.8 else EXTEND if h <= 2.1 else BREAK
        if min(abs(h - 1.8), abs(h - 2.1)) > 1e-9:                         # (numpy's log is not the C library's: only away from the cuts)
            assert by_entropy[k] == want, sv
        assert by_key[k] == by_entropy[k] == by_window[k], sv
    assert {TRIGGER, EXTEND, BREAK} == set(by_entropy[:n].tolist())


def test_candidate_form_of_the_trim_equals_the_host_trim():
    n_trims = n_cut_left = 0
    out = np.zeros(4, np.int32)
    for (name, s, _), (_, raw, _) in zip(fixtures(), emulated()):
        for left, length in raw:
            seg = np.ascontiguousarray(s[left:left + length])
            emu().emu_seg_trim_both(_ptr(seg), length, _ptr(out))
            assert (out[0], out[1]) == (out[2], out[3]), (name, left, length)
            n_trims += 1
            n_cut_left += out[0] > 0
    assert n_trims > 1800 and n_cut_left > 300
    # short raw segments (fewer candidates than a round), segments of non-standard letters only (no value below 1.0)
    for seg in (np.zeros(10, np.int8), np.arange(11, dtype=np.int8), np.full(30, 23, np.int8), np.array([0] * 5 + [23] * 2 + [1] * 5, np.int8)):
        emu().emu_seg_trim_both(_ptr(seg), len(seg), _ptr(out))
        assert (out[0], out[1]) == (out[2], out[3])


def test_emulated_driver_gives_the_golden_ranges():
    n_ranges = 0
    for (name, s, gold), (ranges, _, st) in zip(fixtures(), emulated()):
        if st[3]:
            assert ranges == [] and max(e - b + 1 for b, e in gold) > 10000, name      # handed back: redone by the host code
            continue
        assert ranges == gold, name
        n_ranges += len(ranges)
    assert n_ranges > 1600
