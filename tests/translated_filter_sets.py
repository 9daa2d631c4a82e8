"""Read sets of tests/test_gpu_filters_translated.py: translated (blastx) reads on which the HSP filters decide something.

cover_set(): 80 reads and 16 targets per read. A read holds the coding string of a protein of 100 random letters (synth.back_translate)
between random DNA flanks, so that the gene is 50 .. 100 % of the read -- the query cover of a full-length alignment, measured in bases
on the read, spans that range. The reads come in many lengths, the residues 0, 1 and 2 modulo 3 taken in turn (context lengths differ
inside a read), and every other read is reverse-complemented. The targets are those of the `partial` fixture of
tests/test_gpu_filters_device.py: 8 pieces of the protein that span 50 .. 100 % of it, 15 % of their letters substituted (subject
cover about 100 %, query cover = the span x the gene's share of the read), and 8 whole copies between random protein flanks that make
up 0 .. 50 % of the target -- 5 % substituted where the subject cover is below 70 %, 25 % above, so that a read's best-scoring targets
fail the subject cover. Every fourth read has distant targets only (50 .. 58 % of the letters substituted): its best target, where the
seed stage finds it, fails --id and --approx-id, so that those filters remove records at -k 1 and among the --top survivors too.

best_fail_set(): the blastx counterpart of that file's `best_fail` fixture: 12 reads whose gene has 300 random letters; per read 280
targets that are the protein with 30 % of its letters substituted (no indels: high seed-hit and alignment scores, about 70 % identity)
and 5 targets that are 50-letter pieces of it, unchanged. With --id 90 every target of the first two ranking chunks (128 each) fails."""
import numpy as np

from diamond_amd import synth

GENE = 100


def _pack(seqs):
    return np.concatenate(seqs).astype(np.int8), np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)


def _coding(protein, seed):
    dna, off = synth.back_translate(np.asarray(protein, np.int8), np.array([0, len(protein)], np.int64), seed=seed, flank=(0, 0), reverse_frac=0.0)
    assert off[-1] == 3 * len(protein)
    return dna


def _read(rng, protein, seed, total, reverse):
    """the protein's coding string at a random place of a read of `total` bases (ACGTN = 0..4), reverse-complemented on request"""
    gene = _coding(protein, seed)
    left = int(rng.integers(0, total - len(gene) + 1))
    r = np.concatenate([rng.integers(0, 4, left), gene, rng.integers(0, 4, total - len(gene) - left)]).astype(np.int8)
    return (3 - r[::-1]).astype(np.int8) if reverse else r


def _substituted(rng, s, n):
    t = s.copy()
    pos = rng.choice(len(s), n, replace=False)
    t[pos] = (t[pos] + rng.integers(1, 20, n)) % 20
    return t


def cover_set(n_reads=80):
    """Returns (db, doff, dna, off): database proteins and DNA reads."""
    rng = np.random.default_rng(29)
    reads, ts = [], []
    for i, f in enumerate(np.linspace(0.5, 1.0, n_reads)):
        s = rng.integers(0, 20, GENE).astype(np.int8)
        total = int(round(3 * GENE / f))
        total += (i % 3 - total % 3) % 3                       # read lengths = 0, 1, 2 modulo 3 in turn
        reads.append(_read(rng, s, 1000 + i, total, i % 2 == 1))
        weak = i % 4 == 3                                      # every fourth read: all its targets are distant, the best one included
        for g in np.linspace(0.5, 1.0, 8):
            n = int(round(GENE * g))
            a = int(rng.integers(0, GENE - n + 1))
            ts.append(_substituted(rng, s[a:a + n], int((0.5 if weak else 0.15) * n)))
        for g in np.linspace(0.5, 1.0, 8):
            flank = int(round(GENE / g)) - GENE
            t = _substituted(rng, s, (50 if g < 0.7 else 58) if weak else (5 if g < 0.7 else 25))      # (the copies that will fail the subject cover score best)
            left = flank // 2
            ts.append(np.concatenate([rng.integers(0, 20, left), t, rng.integers(0, 20, flank - left)]).astype(np.int8))
    (db, doff), (dna, off) = _pack(ts), _pack(reads)
    return db, doff, dna, off


def best_fail_set():
    """Returns (db, doff, dna, off, n_long): per read n_long substituted copies first, then 5 unchanged pieces."""
    rng = np.random.default_rng(31)
    reads, ts = [], []
    n_long = 280
    for i in range(12):
        s = rng.integers(0, 20, 300).astype(np.int8)
        reads.append(_read(rng, s, 2000 + i, 900 + 20 + i, i % 2 == 1))
        for _ in range(n_long):
            ts.append(_substituted(rng, s, 90))
        for m in range(5):
            ts.append(s[40 * m + 10: 40 * m + 60].copy())
    (db, doff), (dna, off) = _pack(ts), _pack(reads)
    return db, doff, dna, off, n_long


def hsp_covers(records, off, tl):
    """(query cover, subject cover) in per cent of every record of a translated call, as filter_hsp measures them: 3 x the translated
    range over the read's length in bases, the subject range over the target's length"""
    read_len = np.diff(off)[records["query"]].astype(np.float64)
    tlen = (tl[records["target"] + 1] - tl[records["target"]] - 1).astype(np.float64)
    h = records["hsp"]
    return 3.0 * (h["q_end"] - h["q_begin"]) * 100 / read_len, (h["s_end"] - h["s_begin"]).astype(np.float64) * 100 / tlen
