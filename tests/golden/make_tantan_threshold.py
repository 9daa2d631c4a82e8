"""Finds the sequences of tests/golden/tantan_threshold.txt: repeats on which a single wrong rounding in tantan's recurrences
changes a masked letter. A test that compares masks sees an arithmetic mistake of the last bit only where a repeat probability
lies within an ulp or two of the mask threshold 0.9 -- fewer than one letter in 10^8 of random repeats (none in 8 * 10^7 tried):
the other groups of tests/tantan_corpus.py do not notice the sum of the 50 offsets taken in another order. The oracle restates
three such mistakes (oracle/tantan.c, oracle_tantan_mask_wrong) and gives the repeat probabilities out. This script draws a repeat
with substitutions, then changes one letter at a time, keeping a change when it brings the probability closest to the threshold
closer still, until the wrong arithmetic gives another mask than the right one; CASES sequences for each mistake are written down.

    python tests/golden/make_tantan_threshold.py [seconds]       (all cores, stops at the time limit)"""
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(HERE)]

ALPHABET = "ARNDCQEGHILKMFPSTWYVBJZX*_"
VARIANTS = (1, 2, 3)
CASES = 4


def draw(rng):
    p = int(rng.integers(30, 51)) if rng.random() < 0.7 else int(rng.integers(1, 30))
    n = int(rng.integers(max(60, 3 * p), 360))
    r = np.resize(rng.integers(0, 20, p), n).astype(np.int8)
    flip = rng.random(n) < rng.choice([0.05, 0.1, 0.15, 0.2])
    r[flip] = rng.integers(0, 20, int(flip.sum()))
    return np.concatenate([rng.integers(0, 20, 20), r, rng.integers(0, 20, 20)]).astype(np.int8), p


def search(args):
    seed, seconds = args
    import oracle_py as orc
    import tantan_corpus as tc
    lr = tc.likelihood_ratios()
    rng = np.random.default_rng([808, seed])
    found, t0, tried = [], time.time(), 0
    threshold = np.float32(0.9)

    def distance(s, pf):
        orc.tantan_mask_wrong(s, lr, 0, probabilities=pf)
        return float(np.abs(pf.astype(np.float64) - float(threshold)).min())

    while time.time() - t0 < seconds:
        s, p = draw(rng)
        pf = np.zeros(len(s), np.float32)
        d = distance(s, pf)
        for _ in range(4000):
            if d < 1e-7 or time.time() - t0 > seconds:
                break
            j = int(rng.integers(0, len(s)))
            old = s[j]
            s[j] = rng.integers(0, 20)
            d2 = distance(s, pf)
            if d2 < d:
                d = d2
            else:
                s[j] = old
        tried += 1
        if d >= 1e-7:
            continue
        right = orc.tantan_mask(s, lr)[0]
        hit = [v for v in VARIANTS if not np.array_equal(orc.tantan_mask_wrong(s, lr, v)[0], right)]
        if hit:
            found.append((hit, p, s))
    return found, tried


if __name__ == "__main__":
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    n = os.cpu_count() or 1
    with multiprocessing.Pool(n) as pool:
        results = pool.map(search, [(k, seconds) for k in range(n)])
    found = [f for r in results for f in r[0]]
    print("%d sequences brought to the threshold, %d found" % (sum(r[1] for r in results), len(found)))
    keep, have = [], {v: 0 for v in VARIANTS}
    for hit, p, s in sorted(found, key=lambda f: len(f[2])):
        if any(have[v] < CASES for v in hit):
            keep.append((hit, p, s))
            for v in hit:
                have[v] += 1
    print("cases per wrong rounding:", have)
    with open(os.path.join(HERE, "tantan_threshold.txt"), "w") as f:
        f.write("# written by make_tantan_threshold.py: name, the wrong roundings of oracle_tantan_mask_wrong that change its mask, letters\n")
        for k, (hit, p, s) in enumerate(keep):
            f.write("threshold%d.period%d\t%s\t%s\n" % (k, p, ",".join(str(v) for v in hit), "".join(ALPHABET[x] for x in s)))
