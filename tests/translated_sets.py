"""Test data of the translated (blastx) tests: the constructed read set of tests/test_gpu_extend_translated.py and
tests/test_gpu_plan_translated.py, and the grouping of seed hits per (read, target) pair the tests assert its cases with.

The golden block (tests/golden/ext_blastx.tap) has no (read, target) pair with hits in two frames, so the rules that only show with
several frames are built here, from synth.generate proteins and synth.back_translate reads:
 (a) reads with one base inserted in the middle of the gene: the halves of the gene lie in two frames, one target is hit in both;
 (b) reads that hold the same coding string twice with one base between, the protein itself being in the database: contexts 0 and 1
     reach the same score on that target, and the lower context must be reported. Both copies stand between the same two flanks of 22
     codons, so the composition bias (a window of 40 letters) is the same over both copies and the two scores are equal by construction;
 (c) fragments of 60 bases: short enough to leave (read, target) pairs with one seed hit, which are not x-drop extended;
 (d) one family of 320 members: its reads have more targets than a ranking chunk (128 at -k 25);
 (e) reads of 300 bases whose gene lies in frame 1: context 0 has 100 letters, the frame of the hits 99 -- two classes of the band
     width (16 below 100 letters, 30 from there on), and the width is that of context 0.
About half of the plain reads are reverse-complemented (synth.back_translate)."""
import numpy as np

from diamond_amd import synth


def _concat(*sets):
    db = np.concatenate([s[0] for s in sets])
    q = np.concatenate([s[2] for s in sets])
    doff, qoff, d0, q0 = [np.zeros(1, np.int64)], [np.zeros(1, np.int64)], 0, 0
    for s in sets:
        doff.append(s[1][1:] + d0)
        qoff.append(s[3][1:] + q0)
        d0 += int(s[1][-1])
        q0 += int(s[3][-1])
    return db, np.concatenate(doff), q, np.concatenate(qoff)


def _coding(protein, seed):
    """the protein written in codons, forward, without flanks"""
    dna, off = synth.back_translate(np.asarray(protein, np.int8), np.array([0, len(protein)], np.int64), seed=seed, flank=(0, 0), reverse_frac=0.0)
    assert off[-1] == 3 * len(protein)
    return dna


def constructed_set():
    """Returns (db, doff, dna, off, kinds): database proteins, DNA reads (ACGTN = 0..4) and per read its kind ('plain', 'a' .. 'e')."""
    small = synth.generate(30, members=4, queries=150, seed=61, sub=(0.05, 0.3), qsub=(0.05, 0.3))
    big = synth.generate(1, members=320, queries=12, seed=62, sub=(0.05, 0.25), qsub=(0.05, 0.25), decoy_frac=0.0)
    db, doff, q, qoff = _concat(small, big)
    rng = np.random.default_rng(63)
    base, boff = synth.back_translate(q, qoff, seed=7)
    reads = [base[boff[i]:boff[i + 1]] for i in range(len(boff) - 1)]
    kinds = ["plain"] * len(reads)
    for i in range(40):                                    # (a)
        r = reads[i]
        reads.append(np.insert(r, len(r) // 2, rng.integers(0, 4)).astype(np.int8))
        kinds.append("a")
    proteins = [db[doff[i]:doff[i + 1]] for i in range(len(doff) - 1)]
    short = [p for p in proteins[:120] if 60 <= len(p) <= 260][:8]
    assert len(short) == 8
    for k, p in enumerate(short):                          # (b)
        f1, f2 = _coding(rng.integers(0, 20, 22), 100 + k), _coding(rng.integers(0, 20, 22), 200 + k)
        half = np.concatenate([f1, _coding(p, 300 + k), f2])
        reads.append(np.concatenate([half, rng.integers(0, 4, 1), half]).astype(np.int8))
        kinds.append("b")
    for i in range(40, 80):                                # (c)
        r = reads[i]
        m = len(r) // 2
        reads.append(r[m - 30:m + 30].copy())
        kinds.append("c")
    longer = [p for p in proteins[:120] if len(p) >= 99][8:14]
    assert len(longer) == 6
    for k, p in enumerate(longer):                         # (e)
        reads.append(np.concatenate([rng.integers(0, 4, 1), _coding(p[:99], 400 + k), rng.integers(0, 4, 2)]).astype(np.int8))
        assert len(reads[-1]) == 300
        kinds.append("e")
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    return db, doff, np.concatenate(reads).astype(np.int8), off, kinds


def doubled_targets(doff):
    """the database protein each read of kind 'b' holds twice, in the order of those reads"""
    lens = np.diff(doff)[:120]
    return [int(i) for i in np.flatnonzero((lens >= 60) & (lens <= 260))[:8]]


def pairs_of(hits, tl):
    """The seed hits per (read, target) pair: dict (read, target) -> list of (frame, index into hits), in hit order."""
    tgt = np.searchsorted(tl, hits["subject"], "right") - 1
    out = {}
    for k in range(len(hits)):
        q = int(hits["query"][k])
        out.setdefault((q // 6, int(tgt[k])), []).append((q % 6, k))
    return out


def assert_cases_present(hits, tl, kinds):
    """Cases (a), (c) and (d) from the seed hits, grouped per read; returns the pairs"""
    pairs = pairs_of(hits, tl)
    per_read = {}
    two_frames, single = set(), set()
    for (r, t), v in pairs.items():
        per_read[r] = per_read.get(r, 0) + 1
        if len({f for f, _ in v}) > 1:
            two_frames.add(r)
        if len(v) == 1:
            single.add(r)
    assert any(kinds[r] == "a" for r in two_frames), "no read with an inserted base hits a target in two frames"
    assert any(kinds[r] == "b" for r in two_frames), "no doubled read hits its protein in two frames"
    assert any(kinds[r] == "c" for r in single), "no fragment leaves a single-hit pair"
    assert max(per_read.values()) > 128, "no read has more targets than a ranking chunk"
    assert any(kinds[r] == "e" for r in per_read), "no 300-base read has hits"
    return pairs
