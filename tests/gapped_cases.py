"""Test data of the gapped filter's edge tests (tests/test_gapped_cases.py, tests/test_gpu_gapped_edges.py): seeded block pairs and
seed hits laid at the places where the two filter kernels (csrc/gapped_kernels.hip: the LDS-profile path and the matrix path) can
leave the reference's scan -- the 0 / 255 saturation of a diagonal, the int8 clamp of the biased profile, the diagonal combination
across the 63/64 seam of the two stage-2 half bands, the clipped windows of short sequences and corner hits, the units the host
side cuts the hit list into, and the translated-query rules.

corpus(name) returns a Corpus; a hit's family is the first word of its tag, Corpus.info holds the same as a tuple.

 "blastp" (BLOSUM62 11/1)
   sat     identical: a 300-letter query against itself (a diagonal is at 255 after about 50 columns and stays there);
           bias: the same with a bias of +127 on query letters 40-79 and -128 on 120-159 (both int8 clamps of the profile bind);
           nonstd / mixed: targets of letters 20-25 alone, and the identical target with such letters sprinkled in, under that bias
           (profile rows >= 20 take no bias); fallback: 70 identical letters, 80 of the worst mismatches, 80 identical letters.
   comb    targets equal to the query but for k deleted ("del") or k inserted ("ins") letters: two diagonals k apart that both
           saturate. The hit's own diagonal puts them on chosen lanes of the 128-lane stage-2 band: "seam" (either side of 63/64;
           k = 127 gives lanes 0 and 127), "low" (both in lanes 0-63), "high" (both in 64-127), "band1" (k = 63: lanes 0 and 63 of
           the 64-lane stage-1 band). Where neither of the two lies inside the stage-1 band a 20-letter helper run on the hit's own
           diagonal carries the hit into stage 2.
   exact   a diagonal of 120 and a twin three lanes away that scores exactly diag_score ("at": the combination counts it) or
           diag_score - 1 ("below": it does not); every other column mismatches on both.
   geo     corner: queries of 1, 10, 63, 64, 65 letters against targets of 1-5, 7-9, 63-65, 127-129 letters, a hit in every corner;
           clamp: hits whose band would begin left of diagonal -(slen - 1), with the homology inside the clamped band;
           anchor: the first and the last sequence of both blocks (the out-of-query reads of the matrix path land in the blocks'
           perimeter on either side).
           short: targets of 1 to 9 letters under a bias of +16 on every query letter, so that one column already reaches
           diag_score and every letter of a range of 1 to 9 columns shows in f1.
   long /  a query of 1800 letters, which a unit launch scans with the matrix in LDS (gapped_filter_unit_kernel<false>, what
   longcomb  queries above 1792 letters get in production): saturation under both clamps, letters 20-25, pairs of saturated
           diagonals 1, 63, 64 and 127 lanes apart, short ranges, its corners.
   unit    queries of 512, 1024, 1792 and 1793 letters (one per LDS width class; the last takes the matrix path), runs of 1, 3,
           4, 5, 63, 64, 65, 128, 129 consecutive hits each, the four queries taking turns: every query's hits come in nine
           non-adjacent runs.
 "pam30" (PAM30 9/1: scores -17 .. 13, diag_score 21)    sat, comb and exact once more.
 "blastx" (BLOSUM62, six contexts per read, built with hip.translated_block)
   tx      reads whose context 0 has 84 letters (filter off), 85 and 99 (stage 1 only), 100, 101, 127, 128 (both stages); a
           mutated copy of every frame as a target, hits in all six contexts;
           row: in the reads of 384 and 385 nucleotides context 0 has 128 letters and some other context 127. The hit of such a
           context against a target made for it passes with the cutoffs of row bit_length(127) and fails with those of row
           bit_length(128), which is the row the reference takes (the length of context 0). 383 nucleotides: all frames 127.

Expected values: expected(corpus) -- f1 and f2 from the C oracle (oracle_py.gapped_filter_hit), the flag and the translated rules
restated from the reference (gapped_filter.cpp:43-54, extend.cpp:195-206), the cutoffs from the oracle's CutoffTable2D. diag_scan is
a plain numpy statement of the reference's scan_diags over make_profile8; it proves that a case is what its name says and never
judges the kernel."""
import ctypes
import functools
import math

import numpy as np

import oracle_py as orc
from diamond_amd import hip, workload

KS = (1, 2, 31, 32, 33, 62, 63, 64, 65, 100)
TARGET_LENS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129)
EXTRA_TARGET_LENS = (7, 8, 9)                      # column ranges of 7, 8 and 9: one quad + tail, two quads, two quads + tail
QUERY_LENS = (1, 10, 63, 64, 65)
RANGE_LENS = (1, 2, 3, 4, 5, 7, 8, 9)
RUNS = (1, 3, 4, 5, 63, 64, 65, 128, 129)
CLASS_QLENS = (512, 1024, 1792, 1793)
FRAME0_LENS = (84, 85, 99, 100, 101)
READ_LENS = tuple(3 * n for n in FRAME0_LENS) + (384, 383, 385)
WINDOW1, WINDOW2 = 100, 200                        # gapped_filter.cpp:44, config.gapped_filter_window
EVALUE1, EVALUE2 = 2000.0, 1.0                     # config.gapped_filter_evalue1; Search::Config::gapped_filter_evalue of --sensitive
MIN_QLEN, MIN_STAGE2_QLEN = 85, 100                # extend.cpp:197, gapped_filter.cpp:44
PAD = 128                                          # LongScoreProfile::DEFAULT_PADDING
HELPER, STRONG, SHORT_BIAS = 20, 120, 16


# ---- the reference's scan, restated in numpy -----------------------------------------------------------------------------
def profile8(M, q, bias):
    """DP::make_profile8 (score_profile.cpp:33-64): row l = scores of target letter l along the query, the bias joined to rows
    l < 20 by a saturating int8 add, 128 cells of -1 on either side."""
    p = M[:, np.asarray(q, np.int64) & 31].astype(np.int32)
    if bias is not None:
        p[:20] = np.clip(p[:20] + np.asarray(bias, np.int32), -128, 127)
    return np.pad(p, ((0, 0), (PAD, PAD)), constant_values=-1)


def window(qlen, slen, hit_i, hit_j, band, win):
    """(d_begin, j0, j1, clamped): gapped_filter.cpp:34-37, then the column clipping of scan_diags (scan_diags.cpp:36-38)"""
    raw = hit_i - hit_j - band // 2
    d = max(raw, -(slen - 1))
    jb, je = max(hit_j - win, 0), min(hit_j + win, slen)
    return d, max(jb, -(d + band - 1)), min(qlen - d, je), raw < -(slen - 1)


def diag_scan(M, q, bias, t, hit_i, hit_j, band, win, history=False, fault=None):
    """The band's per-diagonal values of one hit: a biased int8 accumulator per diagonal, floor 0, ceiling 255, and its maximum.
    history: also the accumulators after every column, [columns, band]. fault: a wrong scan, to show that a case would notice
    it -- "tail": the last (range length mod 4) columns are left out; "quad2": columns 4-7 of the range read letter 0."""
    d, j0, j1, _ = window(len(q), len(t), hit_i, hit_j, band, win)
    if fault == "tail":
        j1 -= max(j1 - j0, 0) % 4
    elif fault == "quad2":
        t = np.array(t, np.int8)
        t[j0 + 4:min(j0 + 8, j1)] = 0
    P = profile8(M, q, bias)
    v = np.zeros(band, np.int32)
    best, hist = v.copy(), []
    for j in range(j0, j1):
        v = np.clip(v + P[int(t[j]), PAD + d + j: PAD + d + j + band], 0, 255)
        best = np.maximum(best, v)
        if history:
            hist.append(v)
    return (best, np.array(hist).reshape(-1, band)) if history else best


def clamped_cells(M, q, bias, t, hit_i, hit_j, band, win):
    """(cells above +127, cells below -128) before the clamp, among the profile cells the scan of this hit reads"""
    d, j0, j1, _ = window(len(q), len(t), hit_i, hit_j, band, win)
    hi = lo = 0
    for j in range(j0, j1):
        if t[j] >= 20:
            continue
        i = np.arange(max(d + j, 0), min(d + j + band, len(q)))
        raw = M[int(t[j]), np.asarray(q, np.int64)[i] & 31].astype(np.int32) + np.asarray(bias, np.int32)[i]
        hi += int((raw > 127).sum())
        lo += int((raw < -128).sum())
    return hi, lo


def combine(values, diag_score, gap_open, gap_extend):
    """DP::diag_alignment of per-diagonal values, by the oracle"""
    v = np.ascontiguousarray(values, np.int32)
    return int(orc.lib().oracle_diag_alignment(v.ctypes.data_as(ctypes.c_void_p), len(v), int(diag_score), int(gap_open), int(gap_extend)))


def diag_score_of(p):
    """rawscore(12 bits) as gapped_api.hip takes it"""
    return int(math.ceil((12.0 * math.log(2.0) + math.log(p.K)) / p.lambda_))


def cutoff_tables(p):
    """CutoffTable2D(2000) and CutoffTable2D(1) by the oracle, for the Gumbel constants of these parameters"""
    consts = dict(lambda_=p.lambda_, K=p.K, alpha=p.alpha, alpha_v=p.alpha_v, sigma=p.sigma, u_alpha=p.u_alpha, u_alpha_v=p.u_alpha_v)
    e = orc.evaluer(1e9, p.gap_open, p.gap_extend, consts)
    out = []
    for ev in (EVALUE1, EVALUE2):
        t = np.zeros(32 * 32, np.int32)
        orc.lib().oracle_cutoff_table2d(ctypes.byref(e), ctypes.c_double(ev), t.ctypes.data_as(ctypes.c_void_p))
        out.append(t.reshape(32, 32))
    return out


def judge_hit(c, q, b, t, hi, hj, qlen0, row_len=None):
    """(flag, f1, f2) by the reference's rules; c: M, diag_score, params, contexts, cut1, cut2"""
    if c.contexts > 1 and qlen0 < MIN_QLEN:                                  # extend.cpp:206: the filter is not applied
        return 1, -1, -1
    g = (c.diag_score, c.params.gap_open, c.params.gap_extend)
    b1, b2 = int(qlen0 if row_len is None else row_len).bit_length(), len(t).bit_length()
    f1 = orc.gapped_filter_hit(c.M, q, b, t, hi, hj, 64, WINDOW1, *g)
    if f1 <= c.cut1[b1, b2]:
        return 0, f1, -1
    if c.contexts > 1 and qlen0 < MIN_STAGE2_QLEN:                           # gapped_filter.cpp:54
        return 1, f1, -1
    f2 = orc.gapped_filter_hit(c.M, q, b, t, hi, hj, 128, WINDOW2, *g)
    return int(f2 > c.cut2[b1, b2]), f1, f2


# ---- corpus --------------------------------------------------------------------------------------------------------------
class Corpus:
    """qd, ql, td, tl: the two blocks (workload.sequence_set); cbs: the bias, indexed like qd; hits: SEED_HIT_DTYPE; tags / info:
    one per hit; qs, ts: the sequences; M, params, diag_score, contexts, cut1, cut2."""

    def inputs(self, k):
        """query, bias slice, target, hit_i, hit_j, length of context 0: what the oracle needs for hit k"""
        qi = int(self.hits["query"][k])
        ti = self.target_of[k]
        q0 = int(self.ql[qi])
        c0 = qi // self.contexts * self.contexts
        return (self.qs[qi], self.cbs[q0:q0 + len(self.qs[qi])], self.ts[ti], int(self.hits["seed_offset"][k]),
                int(self.hits["subject"][k] - self.tl[ti]), len(self.qs[c0]))

    def family(self, *prefix):
        return np.array([k for k, i in enumerate(self.info) if i[:len(prefix)] == prefix], np.int64)

    def judge(self, k, row_len=None):
        """(flag, f1, f2) of hit k; row_len: the query length the cutoff row is taken from (default: context 0's)"""
        return judge_hit(self, *self.inputs(k), row_len=row_len)

    def scan(self, k, band, history=False, fault=None):
        q, b, t, hi, hj, _ = self.inputs(k)
        return diag_scan(self.M, q, b, t, hi, hj, band, WINDOW1 if band == 64 else WINDOW2, history, fault)

    def combine(self, values):
        return combine(values, self.diag_score, self.params.gap_open, self.params.gap_extend)

    def window(self, k, band):
        q, _, t, hi, hj, _ = self.inputs(k)
        return window(len(q), len(t), hi, hj, band, WINDOW1 if band == 64 else WINDOW2)


class _Builder:
    def __init__(self, M, diag_score, seed):
        self.M, self.diag_score = M, diag_score
        self.rng = np.random.default_rng(seed)
        self.qs, self.bias, self.ts, self.rows, self.info = [], [], [], [], []
        self.worst = np.argmin(M[:20, :20], axis=0).astype(np.int8)         # the letter that scores lowest against each letter
        self.reachable = {0}                                               # sums of self scores
        for s in range(1, 400):
            if any(s - int(M[a, a]) in self.reachable for a in range(20)):
                self.reachable.add(s)

    def letters(self, n, lo=0, hi=20):
        return self.rng.integers(lo, hi, int(n)).astype(np.int8)

    def exact_run(self, s):
        """random letters whose self scores add up to s"""
        out = []
        while s > 0:
            a = int(self.rng.choice([a for a in range(20) if s - int(self.M[a, a]) in self.reachable]))
            out.append(a)
            s -= int(self.M[a, a])
        return np.array(out, np.int8)

    def add_q(self, q, bias=None):
        self.qs.append(np.asarray(q, np.int8))
        self.bias.append(np.zeros(len(q), np.int8) if bias is None else np.asarray(bias, np.int8))
        return len(self.qs) - 1

    def add_t(self, t):
        self.ts.append(np.asarray(t, np.int8))
        return len(self.ts) - 1

    def hit(self, qid, i, tid, j, info):
        assert 0 <= i < len(self.qs[qid]) and 0 <= j < len(self.ts[tid]), info       # every hit lies inside its sequences
        self.rows.append((qid, int(i), tid, int(j)))
        self.info.append(tuple(info))

    # ---- saturation ------------------------------------------------------------------------------------------------------
    def saturation(self):
        q = self.letters(300)
        bias = np.zeros(300, np.int8)
        bias[40:80], bias[120:160] = 127, -128
        plain, biased = self.add_q(q), self.add_q(q, bias)
        same = self.add_t(q)
        places = ((0, 0), (30, 30), (150, 150), (299, 299), (100, 90), (90, 100), (200, 231), (231, 200), (60, 0), (0, 60),
                  (299, 250), (250, 299), (150, 120), (120, 150), (45, 45), (125, 125))
        for i, j in places:
            self.hit(plain, i, same, j, ("sat", "identical"))
            self.hit(biased, i, same, j, ("sat", "bias"))
        odd = self.letters(150, 20, 26)
        odd[::7] = 23
        t_odd = self.add_t(odd)
        mixed = q.copy()
        mixed[2::5] = self.letters(len(mixed[2::5]), 20, 26)
        t_mixed = self.add_t(mixed)
        for i, j in ((60, 60), (140, 100), (20, 0), (100, 149), (59, 20), (139, 19), (0, 0), (299, 149)):
            self.hit(biased, i, t_odd, j, ("sat", "nonstd"))
            self.hit(plain, i, t_odd, j, ("sat", "nonstd"))
        for i, j in places:
            self.hit(biased, i, t_mixed, j, ("sat", "mixed"))
        t_fall = self.add_t(np.concatenate([q[:70], self.worst[q[70:150]], q[150:230]]))
        for i, j in ((75, 75), (110, 110), (149, 149), (160, 160), (20, 20), (229, 229)):
            self.hit(plain, i, t_fall, j, ("sat", "fallback"))

    # ---- diagonal combination --------------------------------------------------------------------------------------------
    def piecewise(self, q, segments):
        """Target letters column by column: a segment (D, n) copies n query letters along diagonal D (t[j] = q[j + D]),
        (None, n) is n random letters."""
        out, j = [], 0
        for D, n in segments:
            if D is None:
                out.append(self.letters(n))
            else:
                assert 0 <= j + D and j + D + n <= len(q), (D, n, j)
                out.append(q[j + D: j + D + n])
            j += n
        return np.concatenate(out)

    def combination(self):
        for k in KS + (127,):
            q = self.letters(520)
            self.gap_pair(q, self.add_q(q), k, 0, "comb")

    def gap_pair(self, q, qid, k, base, family):
        """Targets that follow the query from letter `base` on but for k deleted / k inserted letters, and the hits that put the two
        diagonals on the chosen stage-2 lanes"""
        a = 160
        placements = [("seam", max(0, 63 - k // 2))]
        if k <= 63:
            placements += [("low", 0), ("high", 64)]
        if k == 63:
            placements.append(("band1", 32))
        for kind in ("del", "ins"):
            for name, low in placements:
                # the two diagonals are base and base + k ("del") or base and base - k ("ins"); `low` is the stage-2 lane of the lower
                lower = 0 if kind == "del" else -k
                hd = 64 - low + lower                                      # the hit's diagonal (less base): lane = D - (hd - 64)
                lanes1 = [lower - (hd - 32), lower + k - (hd - 32)]
                helper = not any(0 <= x < 64 for x in lanes1)
                first = [(base, a)] if kind == "del" else [(base, a), (None, k)]
                j_mid = sum(n for _, n in first)
                mid = [(base + hd, HELPER)] if helper else []
                last = [(base + (k if kind == "del" else -k), 200)]
                tid = self.add_t(self.piecewise(q, first + mid + last))
                # the hit's column: inside the helper run, else at the seam ("ins": in the middle of the inserted letters)
                jh = j_mid + HELPER // 2 if helper else j_mid - (k // 2 if kind == "ins" else 0)
                for dj in (0, 3):
                    self.hit(qid, jh + dj + base + hd, tid, jh + dj, (family, kind, k, name, low, low + k, int(helper)))

    def exact(self):
        """Two diagonals with exact values: STRONG on D = -1 and `twin` on D = 2 (stage-2 lanes 63 and 66 for a hit on diagonal 0)"""
        for name, twin in (("at", self.diag_score), ("below", self.diag_score - 1)):
            for attempt in range(200):
                specs = ((-1, STRONG), (2, twin))
                q = self.letters(100)
                cols, j = [], 8
                for D, s in specs:
                    run = self.exact_run(s)
                    q[j + D: j + D + len(run)] = run
                    cols.append((j, len(run), D))
                    j += len(run) + 8
                j = max(j, 72)                                             # slen >= 65: the band is not clamped
                t = np.zeros(j, np.int8)
                for x in range(j):
                    inside = [D for (c, n, D) in cols if c <= x < c + n]
                    if inside:
                        t[x] = q[x + inside[0]]
                    else:                                                  # a letter that scores below zero on both diagonals
                        t[x] = int(np.argmin(np.max(self.M[:20, q[[x - 1, x + 2]]], axis=1)))
                hi = hj = cols[0][0] + 4
                best = diag_scan(self.M, q, None, t, hi, hj, 128, WINDOW2)
                rest = np.delete(best, [63, 66])
                if best[63] == STRONG and best[66] == twin and rest.max() < self.diag_score:
                    break
            else:
                raise AssertionError("no exact pair for %s" % name)
            self.hit(self.add_q(q), hi, self.add_t(t), hj, ("exact", name, twin))

    # ---- geometry --------------------------------------------------------------------------------------------------------
    def corners(self, qid, tid, info):
        n, m = len(self.qs[qid]), len(self.ts[tid])
        for c in sorted({(0, 0), (0, m - 1), (n - 1, 0), (n - 1, m - 1)}):
            self.hit(qid, c[0], tid, c[1], info + c)

    def geometry(self):
        master = self.letters(400)
        qids = [self.add_q(master[20:20 + n], self.letters(n, 0, 7) - 3) for n in QUERY_LENS]
        tids = [self.add_t(master[15:15 + m]) for m in TARGET_LENS + EXTRA_TARGET_LENS]
        for qid in qids:
            for tid in tids:
                self.corners(qid, tid, ("geo", "corner", len(self.qs[qid]), len(self.ts[tid])))
        self.hit(qids[-1], 32, tids[TARGET_LENS.index(129)], 64, ("geo", "corner", 65, 129, 32, 64))
        for slen in (65, 129):
            P = self.letters(31)
            qid = self.add_q(np.concatenate([P, self.letters(34)]))
            tid = self.add_t(np.concatenate([self.letters(slen - 31), P]))
            for i, j in ((0, slen - 31), (0, slen - 1), (3, slen - 10), (15, slen - 16), (30, slen - 1)):
                self.hit(qid, i, tid, j, ("geo", "clamp", slen, i, j))

    def anchor(self, S):
        return self.add_q(S, self.letters(len(S), 0, 7) - 3), self.add_t(S)

    def anchor_hits(self, first, last, others):
        for qn, qid in (("first", first[0]), ("last", last[0])):
            for tn, tid in (("first", first[1]), ("last", last[1])):
                self.corners(qid, tid, ("geo", "anchor", qn, tn))
                self.hit(qid, 24, tid, 24, ("geo", "anchor", qn, tn, 24, 24))
            for tid in others:                                             # a long target: the band reaches far past the query
                m = len(self.ts[tid])
                for i, j in ((0, m - 1), (len(self.qs[qid]) - 1, 0), (10, m // 2)):
                    self.hit(qid, i, tid, j, ("geo", "anchor", qn, "long", i, j))

    # ---- units -----------------------------------------------------------------------------------------------------------
    def units(self):
        per_query = []
        for n in CLASS_QLENS:
            q = self.letters(n)
            qid = self.add_q(q, self.letters(n, 0, 7) - 3)
            homologs = []
            for _ in range(3):
                a = int(self.rng.integers(0, n - 80))
                piece = q[a:a + int(self.rng.integers(60, 400))].copy()
                mut = self.rng.random(len(piece)) < 0.35
                piece[mut] = self.letters(int(mut.sum()))
                left = int(self.rng.integers(0, 150))
                t = np.concatenate([self.letters(left), piece, self.letters(self.rng.integers(0, 150))])
                t[self.rng.random(len(t)) < 0.02] = 23
                homologs.append((self.add_t(t), a, left, len(piece)))
            per_query.append((qid, n, homologs))
        for r in RUNS:
            for qid, n, homologs in per_query:
                for x in range(r):
                    tid, a, left, m = homologs[int(self.rng.integers(0, 3))]
                    if self.rng.random() < 0.6:                            # near the homology's diagonal
                        p = int(self.rng.integers(0, m))
                        i = min(max(a + p + int(self.rng.integers(-10, 11)), 0), n - 1)
                        j = left + p
                    else:
                        i, j = int(self.rng.integers(0, n)), int(self.rng.integers(0, len(self.ts[tid])))
                    self.hit(qid, i, tid, j, ("unit", n, r, x))

    # ---- short ranges that show --------------------------------------------------------------------------------------------
    def short(self):
        """Targets of 1 to 9 letters that begin like the queries, under a bias of +16 on every query letter: a cell is worth 12 to
        27, one on the common diagonal 20 to 27, so one column reaches diag_score and nine stay below 255 -- every letter of
        a range of 1 to 9 columns shows in f1."""
        master = self.letters(80)
        qids = [self.add_q(master[:n], np.full(n, SHORT_BIAS, np.int8)) for n in QUERY_LENS]
        tids = [self.add_t(master[:m]) for m in range(1, 10)]
        for qid in qids:
            for tid in tids:
                self.corners(qid, tid, ("geo", "short", len(self.qs[qid]), len(self.ts[tid])))
        return tids

    # ---- a query on the unit kernel's matrix path --------------------------------------------------------------------------
    def long_query(self, short_tids):
        """1800 letters: longer than the widest LDS class, so in a unit launch its hits scan with the matrix in LDS. Saturation with
        both clamps, letters 20-25, two saturated diagonals around the seam and at the band's ends, short ranges, its corners."""
        base = 700
        q = self.letters(1800)
        bias = np.zeros(len(q), np.int8)
        bias[base + 40:base + 80], bias[base + 120:base + 160] = 127, -128
        bias[:10], bias[-10:] = SHORT_BIAS, SHORT_BIAS
        qid = self.add_q(q, bias)
        same = self.add_t(q[base:base + 300])
        mixed = q[base:base + 300].copy()
        mixed[2::5] = self.letters(len(mixed[2::5]), 20, 26)
        t_mixed = self.add_t(mixed)
        for i, j in ((0, 0), (30, 30), (150, 150), (299, 299), (100, 90), (90, 100), (60, 0), (0, 60), (45, 45), (125, 125)):
            self.hit(qid, base + i, same, j, ("long", "sat"))
            self.hit(qid, base + i, t_mixed, j, ("long", "sat"))
        for k in (1, 63, 64, 127):                                         # on letters 1100 and up: clear of the biased stretches
            self.gap_pair(q, qid, k, base + 400, "longcomb")
        head, tail = self.add_t(q[:9]), self.add_t(q[-9:])
        for tid in (head, tail, same) + tuple(short_tids):
            self.corners(qid, tid, ("long", "corner", len(self.ts[tid])))


def _finish(b, params, contexts=1, qblock=None):
    c = Corpus()
    c.params, c.M, c.diag_score, c.contexts = params, b.M, b.diag_score, contexts

    def block(seqs):
        off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
        return workload.sequence_set(np.concatenate(seqs).astype(np.int8), off)

    c.qd, c.ql = block(b.qs) if qblock is None else qblock
    c.td, c.tl = block(b.ts)
    c.qs, c.ts = b.qs, b.ts
    c.cbs = np.zeros(len(c.qd), np.int8)
    for qid, bias in enumerate(b.bias):
        c.cbs[c.ql[qid]:c.ql[qid] + len(bias)] = bias
    for qid, q in enumerate(b.qs):
        assert np.array_equal(c.qd[c.ql[qid]:c.ql[qid + 1] - 1], q)
    hits = np.zeros(len(b.rows), dtype=hip.SEED_HIT_DTYPE)
    for k, (qid, i, tid, j) in enumerate(b.rows):
        hits[k]["query"], hits[k]["seed_offset"], hits[k]["subject"] = qid, i, int(c.tl[tid]) + j
    c.hits, c.info = hits, b.info
    c.tags = ["/".join(str(x) for x in i) for i in b.info]
    c.target_of = [tid for _, _, tid, _ in b.rows]
    c.cut1, c.cut2 = cutoff_tables(params)
    return c


def _blastx(params, M, diag_score):
    b = _Builder(M, diag_score, 4711)
    dna = [b.letters(n, 0, 4) for n in READ_LENS]
    off = np.concatenate([[0], np.cumsum([len(x) for x in dna])]).astype(np.int64)
    qd, ql = hip.translated_block(np.concatenate(dna), off)
    for qid in range(len(ql) - 1):
        q = qd[ql[qid]:ql[qid + 1] - 1]
        b.add_q(q, b.letters(len(q), 0, 7) - 3)
    for qid, q in enumerate(b.qs):
        read = READ_LENS[qid // 6]
        copy = q.copy()
        mut = b.rng.random(len(q)) < 0.2
        copy[mut] = b.letters(int(mut.sum()))
        left = int(b.rng.integers(10, 30))
        tid = b.add_t(np.concatenate([b.letters(left), copy, b.letters(b.rng.integers(10, 30))]))
        for p in (len(q) // 4, len(q) // 2, 3 * len(q) // 4):
            b.hit(qid, p, tid, left + p, ("tx", "homolog", read, qid % 6))
        b.hit(qid, int(b.rng.integers(0, len(q))), tid, int(b.rng.integers(0, len(b.ts[tid]))), ("tx", "random", read, qid % 6))
    c = _finish(b, params, 6, (qd, ql))
    # the cutoff row: a context of 127 letters in a read whose context 0 has 128. An identical run is grown and moved until the hit
    # passes with row bit_length(127) and fails with row bit_length(128)
    found = 0
    for read, ctx in ((384, 1), (384, 2), (384, 4), (385, 2), (385, 5)):
        qid = 6 * READ_LENS.index(read) + ctx
        q = b.qs[qid]
        assert len(q) == 127 and len(b.qs[qid - ctx]) == 128
        for L, s in ((L, s) for L in range(6, 60) for s in range(0, 60, 3)):
            t = np.concatenate([b.letters(s), q[s:s + L], b.letters(40)])
            at = s + L // 2
            if judge_hit(c, q, b.bias[qid], t, at, at, 128, 127)[0] == 1 and judge_hit(c, q, b.bias[qid], t, at, at, 128, 128)[0] == 0:
                b.hit(qid, at, b.add_t(t), at, ("tx", "row", read, ctx))
                found += 1
                break
    assert found >= 2
    return _finish(b, params, 6, (qd, ql))


@functools.lru_cache(maxsize=None)
def corpus(name):
    c = _corpus(name)
    c.name = name
    return c


def _corpus(name):
    params = hip.default_params() if name != "pam30" else hip.matrix_params("pam30")
    M = hip.matrix_of(params)
    ds = diag_score_of(params)
    if name == "blastx":
        return _blastx(params, M, ds)
    b = _Builder(M, ds, {"blastp": 20250, "pam30": 30}[name])
    if name == "pam30":
        b.saturation()
        b.combination()
        b.exact()
        return _finish(b, params)
    S = b.letters(48)
    first = b.anchor(S)
    b.saturation()
    long_q, long_t = len(b.qs) - 2, len(b.ts) - 4                          # the 300-letter query and its identical target
    b.combination()
    b.exact()
    b.geometry()
    b.units()
    b.long_query(b.short())
    last = b.anchor(S)
    b.anchor_hits(first, last, (long_t,))
    for tn, tid in (("first", first[1]), ("last", last[1])):
        b.corners(long_q, tid, ("geo", "anchor", "long", tn))
    return _finish(b, params)


@functools.lru_cache(maxsize=None)
def _expected_cached(name):
    c = corpus(name)
    flags, scores = np.zeros(len(c.hits), np.uint8), np.zeros((len(c.hits), 2), np.int32)
    for k in range(len(c.hits)):
        flags[k], scores[k, 0], scores[k, 1] = c.judge(k)
    flags.setflags(write=False)
    scores.setflags(write=False)
    return flags, scores


def expected(c):
    """(flags, scores[n, 2]) every hit of the corpus has to get, computed once"""
    assert c is corpus(c.name)
    return _expected_cached(c.name)
