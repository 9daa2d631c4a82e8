"""The three-frame banded sweep of frameshift alignment (blastx -F), CPU side:
  * the oracle restatement (oracle/frameshift_swipe.c) against known answers tapped from the genuine reference at its dispatch
    point banded_3frame_swipe (/root/reference/src/dp/dp.h:296; fixtures tests/golden/f3_*.tap, make_frameshift_golden.sh) --
    score-only calls with the reference's 16-channel vector batches (one band geometry per batch), traceback calls with
    coordinates in the read, statistics and transcripts incl. the frameshift operations;
  * the per-item code of the device kernels (diamond_amd/csrc/frameshift_core.h, run by tests/emu) against the oracle on the same
    items and on random ones."""
import ctypes
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle_py as orc  # noqa: E402
from tapfile import read_3frame_tap  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
KEYS = "score frame q_begin q_end s_begin s_end qs_begin qs_end length identities mismatches positives gap_openings gaps".split()


def _emu():
    lib = ctypes.CDLL(os.path.join(HERE, "emu", "libswipe_emu.so"))
    return lib


def _frames(frames):
    fr = [np.ascontiguousarray(f, dtype=np.int8) for f in frames]
    ptrs = (ctypes.c_void_p * 3)(*[f.ctypes.data for f in fr])
    lens = (ctypes.c_int32 * 3)(*[len(f) for f in fr])
    return fr, ptrs, lens


def emu_score(frames, target, band, i0, i1, pos0, M, go, ge, fs, stride=1):
    fr, ptrs, lens = _frames(frames)
    t = np.ascontiguousarray(target, dtype=np.int8)
    m = np.ascontiguousarray(M, dtype=np.int8)
    mc = ctypes.c_int(0)
    assert i1 - i0 + 1 == band
    s = _emu().emu_3frame_score(ptrs, lens, ctypes.c_void_p(t.ctypes.data), len(t), int(i0), int(i1), int(pos0), ctypes.c_void_p(m.ctypes.data),
                                int(go), int(ge), int(fs), int(stride), ctypes.byref(mc))
    return s, mc.value


def emu_traceback(frames, strand, dna_len, target, d_begin, d_end, M, go, ge, fs):
    fr, ptrs, lens = _frames(frames)
    t = np.ascontiguousarray(target, dtype=np.int8)
    m = np.ascontiguousarray(M, dtype=np.int8)
    out = np.zeros(16, np.int32)
    cap = 2 * len(t) + len(fr[0]) + 64
    tr = np.zeros(cap, np.uint8)
    rc = _emu().emu_3frame_traceback(ptrs, lens, int(strand), int(dna_len), ctypes.c_void_p(t.ctypes.data), len(t), int(d_begin), int(d_end),
                                     ctypes.c_void_p(m.ctypes.data), int(go), int(ge), int(fs), ctypes.c_void_p(out.ctypes.data),
                                     ctypes.c_void_p(tr.ctypes.data), cap)
    d = dict(zip(KEYS + ["transcript_len", "status"], out.tolist()))
    return rc, d, tr[:d["transcript_len"]].copy()


@pytest.mark.parametrize("tap", ["f3_k3.tap", "f3_k1.tap"])
def test_oracle_and_device_code_equal_the_reference(tap):
    hdr, recs = read_3frame_tap(os.path.join(GOLDEN, tap))
    M, go, ge, fs = hdr["matrix8"], hdr["gap_open"], hdr["gap_extend"], hdr["frame_shift"]
    assert fs == 15
    ev = orc.evaluer(hdr["db_letters"], go, ge)
    n_score = n_trace = n_shift = 0
    for r in recs:
        fr = r["frames"]
        by_target = {}
        for h in r["hsps"]:
            by_target.setdefault(h["swipe_target"], []).append(h)
        if r["score_only"]:
            for batch in orc.frameshift_batches(r["targets"]):
                for k, band, i0, i1, pos0 in batch:
                    t = r["targets"][k]
                    s, mc, ov = orc.frameshift_score(fr, t["seq"], band, i0, i1, pos0, M, go, ge, fs)
                    assert not ov
                    assert emu_score(fr, t["seq"], band, i0, i1, pos0, M, go, ge, fs, stride=1 + k % 3) == (s, mc)
                    if orc.evalue(ev, s, len(fr[0]), len(t["seq"])) > hdr["max_evalue"]:
                        continue
                    rg = orc.frameshift_score_range(r["strand"], r["dna_len"], len(fr[0]), band, i0, pos0, mc)
                    out = np.zeros(4, np.int32)
                    _emu().emu_3frame_score_range(r["strand"], r["dna_len"], len(fr[0]), band, i0, pos0, mc, ctypes.c_void_p(out.ctypes.data))
                    assert out.tolist() == [rg["q_begin"], rg["q_end"], rg["qs_begin"], rg["qs_end"]]
                    assert any(h["score"] == s and all(h[x] == rg[x] for x in ("frame", "q_begin", "q_end", "qs_begin", "qs_end")) for h in by_target.get(t["target_idx"], [])), (t["target_idx"], s, rg)
                    n_score += 1
        else:
            for t in r["targets"]:
                rc, o, tr = orc.frameshift_traceback(fr, r["strand"], r["dna_len"], t["seq"], t["d_begin"], t["d_end"], M, go, ge, fs)
                assert rc == 0
                rc2, e, etr = emu_traceback(fr, r["strand"], r["dna_len"], t["seq"], t["d_begin"], t["d_end"], M, go, ge, fs)
                assert rc2 == 0 and e["score"] == o["score"]
                if o["score"] > 0:
                    assert all(e[x] == o[x] for x in KEYS), (e, o)
                    assert np.array_equal(etr, tr)
                if o["score"] <= 0 or orc.evalue(ev, o["score"], len(fr[0]), len(t["seq"])) > hdr["max_evalue"]:
                    continue
                assert any(all(h[x] == o[x] for x in KEYS) and np.array_equal(h["transcript"][:-1], tr) for h in by_target.get(t["target_idx"], [])), (t["target_idx"], o)
                n_trace += 1
                n_shift += int(((tr == 218) | (tr == 219)).sum())
    assert n_trace > 50 and n_shift > 20 and (n_score > 20 or tap == "f3_k3.tap")


# letters 0-25 as a translated read and a database hold them: the 20 amino acids, B / J / Z (20 - 22), X = 23, stops (24) at about
# 1 in 20 and the hard-mask letter 25 (also the column the sweep scores before a channel's target begins)
WIDE_ALPHABET = np.full(26, 0.88 / 20)
WIDE_ALPHABET[20:23], WIDE_ALPHABET[23], WIDE_ALPHABET[24], WIDE_ALPHABET[25] = 0.01, 0.02, 0.05, 0.02
WIDE_ALPHABET /= WIDE_ALPHABET.sum()
# (matrix, gap open, gap extend): the default and three other pairs the matrices' tables hold
MATRICES = (("BLOSUM62", 11, 1), ("BLOSUM45", 14, 2), ("BLOSUM80", 10, 1), ("PAM30", 9, 1))


def _random_case(rng, M, alphabet=None, mutate=0.25):
    """A read of one strand (three frames cut from a random letter stream, as a translation gives them), a target related to one
    frame up to a frameshift in the middle, a random band. alphabet: None = letters 0-20 in the frames and 0-19 in the targets,
    or the probabilities of the letters 0 .. len - 1 for both; mutate: the share of target letters drawn again."""
    if alphabet is None:
        draw = lambda hi, k: rng.integers(0, hi, k).astype(np.int8)
    else:
        draw = lambda hi, k: rng.choice(len(alphabet), k, p=alphabet).astype(np.int8)
    n = int(rng.integers(4, 260))
    dna_len = 3 * n + int(rng.integers(0, 3))
    frames = [draw(21, max((dna_len - f) // 3, 0)) for f in range(3)]
    f0 = int(rng.integers(0, 3))
    cut = int(rng.integers(0, len(frames[f0]) + 1))
    f1 = (f0 + int(rng.integers(0, 3))) % 3
    t = np.concatenate([frames[f0][:cut], frames[f1][cut:cut + int(rng.integers(0, 120))], draw(20, int(rng.integers(0, 30)))])
    mut = rng.random(len(t)) < mutate
    t[mut] = draw(20, int(mut.sum()))
    if len(t) == 0:
        t = np.array([3], np.int8)
    if rng.random() < 0.3:
        t = np.concatenate([draw(20, int(rng.integers(1, 40))), t])
    qlen, tlen = len(frames[0]), len(t)
    d0 = int(rng.integers(-(tlen - 1) - 3, qlen + 2))
    d1 = d0 + int(rng.integers(1, 90))
    d0, d1 = max(d0, -(tlen - 1)), min(d1, qlen - 1)
    if d1 <= d0:
        d0, d1 = max(-(tlen - 1), -2), min(qlen - 1, 3)
    if d1 <= d0:
        d0, d1 = 0, 1
    return frames, dna_len, t, d0, d1


def test_device_code_equals_oracle_on_random_items():
    rng = np.random.default_rng(5)
    from diamond_amd import hip
    M = hip.matrix_of(hip.default_params())
    n_hit = n_gap = 0
    for it in range(700):
        frames, dna_len, t, d0, d1 = _random_case(rng, M)
        if len(frames[0]) == 0:
            continue
        strand = it % 2
        fs = int(rng.choice([15, 15, 5, 30]))
        rc, o, tr = orc.frameshift_traceback(frames, strand, dna_len, t, d0, d1, M, 11, 1, fs)
        rc2, e, etr = emu_traceback(frames, strand, dna_len, t, d0, d1, M, 11, 1, fs)
        assert rc == 0 and rc2 == 0 and e["score"] == o["score"], (it, rc, rc2)
        if o["score"] > 0:
            assert all(e[x] == o[x] for x in KEYS), (it, e, o)
            assert np.array_equal(etr, tr)
            n_hit += 1
            n_gap += o["gap_openings"] > 0
        # the same target as a channel of a wider batch: band widened downwards, a later start
        widen, late = int(rng.integers(0, 40)), int(rng.integers(0, 25))
        band = d1 - d0 + widen
        i1 = max(max(d1 - 1, 0) - late, 0)
        i0 = i1 + 1 - band
        pos0 = i1 - (d1 - 1)
        s, mc, ov = orc.frameshift_score(frames, t, band, i0, i1, pos0, M, 11, 1, fs)
        assert emu_score(frames, t, band, i0, i1, pos0, M, 11, 1, fs, stride=1 + it % 4) == (s, mc)
    assert n_hit > 300 and n_gap > 20


# ---- items of the edge tests (shared with tests/test_gpu_frameshift_edges.py: the device runs the lists the emulator runs) ----------

def own_geometry(d0, d1):
    """(band, i0, i1, pos0) of a target swept alone on its own band (f3_own_geometry restated)"""
    i1 = max(d1 - 1, 0)
    return d1 - d0, i1 + 1 - (d1 - d0), i1, i1 - (d1 - 1)


def group_runs(groups):
    """[(first, end)] of the runs of equal neighbours: the calls of a score-only pass"""
    runs, k = [], 0
    while k < len(groups):
        e = k
        while e < len(groups) and groups[e] == groups[k]:
            e += 1
        runs.append((k, e))
        k = e
    return runs


def oracle_score_only(meta, groups, cols, M, go, ge, fs, channels):
    """What a score-only pass reports per item, from the oracle alone: the item on the geometry of its vector batch, or -- where the
    oracle flags the int16 saturation there -- swept again alone on its own band (banded_3frame_swipe.cpp:520-528, 619).
    meta: [(frames, strand, dna_len, target, d_begin, d_end)]. -> ([(score, max_col, q_begin, q_end, read_begin, read_end, frame)],
    [saturated on the batch geometry], [score on the batch geometry])"""
    want, again, first = [None] * len(meta), [False] * len(meta), [0] * len(meta)
    for k0, k1 in group_runs(groups):
        targets = [dict(d_begin=meta[x][4], d_end=meta[x][5], cols=int(cols[x])) for x in range(k0, k1)]
        for batch in orc.frameshift_batches(targets, channels=channels):
            for j, band, i0, i1, pos0 in batch:
                frames, strand, dna_len, t, d0, d1 = meta[k0 + j]
                s, mc, ov = orc.frameshift_score(frames, t, band, i0, i1, pos0, M, go, ge, fs)
                first[k0 + j] = s
                if ov:
                    band, i0, i1, pos0 = own_geometry(d0, d1)
                    s, mc, _ = orc.frameshift_score(frames, t, band, i0, i1, pos0, M, go, ge, fs)
                    again[k0 + j] = True
                rg = orc.frameshift_score_range(strand, dna_len, len(frames[0]), band, i0, pos0, mc)
                want[k0 + j] = (s, mc, rg["q_begin"], rg["q_end"], rg["qs_begin"], rg["qs_end"], rg["frame"])
    return want, again, first


def wide_items(n, seed=41, mutate=0.25):
    """n random items with letters 0-25 (WIDE_ALPHABET): [(frames, strand, dna_len, target, d_begin, d_end)]"""
    rng = np.random.default_rng(seed)
    meta = []
    while len(meta) < n:
        frames, dna_len, t, d0, d1 = _random_case(rng, None, alphabet=WIDE_ALPHABET, mutate=mutate)
        meta.append((frames, len(meta) % 2, dna_len, t, d0, d1))
    return meta


def degenerate_items():
    """Every read of 3 - 14 nucleotides (frames of 1/0/0 .. 4/4/4 letters) x targets of 1 - 4 letters x both strands x every band
    [d_begin, d_end) inside -(tlen - 1) .. qlen, the one-diagonal bands and those touching either corner included; letters from
    three that match often (W, C, H), each with the target planted in frame 0, 1 and 2 in turn."""
    rng = np.random.default_rng(9)
    letters = np.array([17, 4, 8], np.int8)
    meta = []
    for dna_len in range(3, 15):
        for tlen in range(1, 5):
            for strand in (0, 1):
                qlen = dna_len // 3
                for d0 in range(-(tlen - 1), qlen):
                    for d1 in range(d0 + 1, qlen + 1):
                        for f in range(3):
                            frames = [letters[rng.integers(0, 3, (dna_len - x) // 3)] for x in range(3)]
                            t = letters[rng.integers(0, 3 if len(meta) % 4 else 2, tlen)]
                            if len(frames[f]):
                                at = int(rng.integers(0, max(len(frames[f]) - tlen, 0) + 1))
                                m = min(tlen, len(frames[f]) - at)
                                frames[f][at:at + m] = t[:m]
                            meta.append((frames, strand, dna_len, t, d0, d1))
    return meta


def end_frame(o, strand, dna_len):
    """frame of the last aligned query position of a walked alignment, from its range in the read (f3_read_range restated)"""
    return o["qs_end"] - 3 * o["q_end"] if strand == 0 else dna_len - o["qs_begin"] - 3 * o["q_end"]


def saturation_groups():
    """Score-only calls (groups) of four items each: one read whose frame 0 is a run of tryptophans (W-W = 11 in BLOSUM62) plus a
    few other letters against the same string as target -- the score is the sum of the self-scores, chosen around the int16
    vectors' 65535 -- and three short targets of the same read with wider bands and smaller d_end, so that the batch geometry is
    not the long item's own. -> [(strand, wanted score of the long item, [(frames, strand, dna_len, target, d_begin, d_end)])]"""
    rng = np.random.default_rng(3)
    W, P, H = 17, 14, 8                                      # self-scores 11, 7, 8
    plans = [(0, 5957, [P], 65534), (1, 5957, [H], 65535), (0, 5957, [H], 65535), (1, 5958, [], 65538), (0, 7000, [P, H], 77015), (1, 5957, [P], 65534)]
    out = []
    for strand, n_w, pad, score in plans:
        f0 = np.concatenate([np.full(n_w // 2, W), np.array(pad, np.int64), np.full(n_w - n_w // 2, W)]).astype(np.int8)
        dna_len = 3 * len(f0) + 2
        frames = [f0, rng.integers(0, 20, len(f0)).astype(np.int8), rng.integers(0, 20, len(f0)).astype(np.int8)]
        items = [(frames, strand, dna_len, f0.copy(), -3, 5)]
        for m in range(3):
            items.append((frames, strand, dna_len, frames[m][m:m + 30].copy(), m - 20 - 4 * m, m + 1))      # its match on diagonal m
        out.append((strand, score, items))
    return out


def _emu_equals_oracle(meta, M, go, ge, fs, groups, cols, channels):
    """traceback items and score-only batches of one list: emulator against oracle; -> (positive scores, [oracle Hsp])"""
    hsps = []
    for k, (frames, strand, dna_len, t, d0, d1) in enumerate(meta):
        rc, o, tr = orc.frameshift_traceback(frames, strand, dna_len, t, d0, d1, M, go, ge, fs)
        rc2, e, etr = emu_traceback(frames, strand, dna_len, t, d0, d1, M, go, ge, fs)
        assert rc == 0 and rc2 == 0 and e["score"] == o["score"], (k, rc, rc2, e, o)
        if o["score"] > 0:
            assert all(e[x] == o[x] for x in KEYS), (k, e, o)
            assert np.array_equal(etr, tr), k
        hsps.append(o)
    for k0, k1 in group_runs(groups):
        targets = [dict(d_begin=meta[x][4], d_end=meta[x][5], cols=int(cols[x])) for x in range(k0, k1)]
        for batch in orc.frameshift_batches(targets, channels=channels):
            for j, band, i0, i1, pos0 in batch:
                frames, strand, dna_len, t, d0, d1 = meta[k0 + j]
                s, mc, ov = orc.frameshift_score(frames, t, band, i0, i1, pos0, M, go, ge, fs)
                assert emu_score(frames, t, band, i0, i1, pos0, M, go, ge, fs, stride=1 + j % 3) == (s, mc), (k0 + j, band, i0, i1, pos0)
    return sum(o["score"] > 0 for o in hsps), hsps


def edge_cols(n):
    """DpTarget::cols of the edge lists' items: any value orders a call's batches, negative ones included"""
    return (np.arange(n) * 37) % 950 - 50


def test_device_code_equals_oracle_with_letters_above_20_and_other_matrices():
    """Letters 0-25 (X, stops, the hard-mask letter) under four matrices / gap penalties and frameshift penalties 1, 15, 50."""
    from diamond_amd import hip
    meta = wide_items(240)
    seen = np.bincount(np.concatenate([np.concatenate(m[0]) for m in meta] + [m[3] for m in meta]), minlength=26)
    assert seen[23] > 100 and seen[24] > 1000 and seen[25] > 100 and len(seen) == 26
    groups, cols = np.arange(len(meta)) // 5, edge_cols(len(meta))
    for x, (name, go, ge) in enumerate(MATRICES):
        M = hip.matrix_of(hip.matrix_params(name, go, ge))
        for fs in (1, 15, 50):
            sub = slice(x % 2, None, 2) if fs != 15 else slice(None)
            n_hit, _ = _emu_equals_oracle(meta[sub], M, go, ge, fs, groups[sub], cols[sub], 4)
            assert n_hit >= 0.4 * len(meta[sub]), (name, fs, n_hit)


def test_device_code_equals_oracle_on_degenerate_geometry():
    """Reads of 3 - 14 nucleotides, targets of 1 - 4 letters, every band: the early end of the shorter frames, one-letter frames,
    empty frames, bands of one diagonal."""
    from diamond_amd import hip
    M = hip.matrix_of(hip.default_params())
    meta = degenerate_items()
    assert 2000 < len(meta) < 6000
    assert {tuple(len(f) for f in m[0]) for m in meta} >= {(1, 0, 0), (1, 1, 0), (1, 1, 1)} and any(m[5] - m[4] == 1 for m in meta)
    n_hit, hsps = _emu_equals_oracle(meta, M, 11, 1, 15, np.arange(len(meta)) // 7, edge_cols(len(meta)), 16)
    assert n_hit >= len(meta) / 3
    n_short_end = 0
    for (frames, strand, dna_len, t, d0, d1), o in zip(meta, hsps):
        if o["score"] > 0:
            f = end_frame(o, strand, dna_len)
            assert 0 <= f <= 2
            n_short_end += f > 0 and len(frames[f]) < len(frames[0]) and o["q_end"] == len(frames[f])
    assert n_short_end >= 20, n_short_end


def test_device_code_equals_oracle_around_the_int16_saturation():
    """Reads of about 6 000 tryptophans against themselves: the oracle's scores are the planned ones (65534: below the saturation;
    65535 and above: flagged), the emulator equals it on the batch geometry and on the item's own."""
    from diamond_amd import hip
    M = hip.matrix_of(hip.default_params())
    for strand, score, items in saturation_groups():
        want, again, first = oracle_score_only(items, [0] * 4, [0] * 4, M, 11, 1, 15, 4)
        assert first[0] == score and want[0][0] == score and again == [score >= 65535, False, False, False]
        targets = [dict(d_begin=m[4], d_end=m[5], cols=0) for m in items]
        (batch,) = list(orc.frameshift_batches(targets, channels=4))
        for j, band, i0, i1, pos0 in batch:
            frames, _, _, t, d0, d1 = items[j]
            assert (band, i0, i1, pos0) != own_geometry(d0, d1) or j != 0
            for geo in ((band, i0, i1, pos0), own_geometry(d0, d1)):
                s, mc, ov = orc.frameshift_score(frames, t, *geo, M, 11, 1, 15)
                assert emu_score(frames, t, *geo, M, 11, 1, 15, stride=2) == (s, mc)
