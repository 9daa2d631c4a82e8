"""Test data of the traceback edge tests (tests/test_traceback_cases.py, tests/test_gpu_traceback_edges.py): a seeded list of work
items laid at the places where traceback_walk_wave (csrc/swipe_kernels.hip) can leave the serial walk traceback_walk (swipe_core.h)
-- it scores 64 diagonal steps per round trip, ends a run by a ballot, applies the stop rule `sc < best` by a wave prefix sum, cuts
insertion counts at 63, writes deletions in a lane-strided loop and moves the transcript 64 bytes per pass. Letters 0 - 19 unless
said otherwise, the context's matrix (hip.matrix_of) and gap costs, records in the shape pack_records / pack_records_m take.
corpus() is built for BLOSUM62 with gap open 11 / extend 1; corpus(scheme), scheme = (matrix name, gap open, gap extend), rebuilds
the families for another scoring system (see "Other scoring systems" below). Diagonals are query position - target position: extra
letters in the query are an insertion (towards +G).

Every record carries rec["tag"] = family/.../variant/band class and rec["info"], a dict with "family", "variant" and the property
the case is meant to have (test_traceback_cases.py asserts it from the oracle):

 gap      two random flanks of 120 letters, identical in query and target, G random letters between them in one sequence only,
          G = 1 .. 200 around the multiples of 63 and 64, "ins" (query) and "del" (target); band [-8, G + 9) and its mirror.
 run      identical pairs of N letters, N around 64 / 128 / 192: "origin" alone (the walk ends at the matrix origin), "score" behind
          seven columns of W against D (it ends by score), "zero" behind W:W W:D W:D A:R G:W = +11 -4 -4 -1 -2 (it ends where the
          running score is back at exactly 0).
 between  M r . I5 . M r . D5 . M r, r = 63 / 64 / 65 / 127 / 128 / 129, and the two gaps swapped: a gap at lane 0 right after one or
          two (nearly) full round trips.
 adjacent 80-letter identical flanks around 30 W in one sequence against 30 D in the other: two gaps with no column between.
 letters  mismatch columns with target letters 20 - 24, mismatches with a positive score, bit 7 set in query and target letters; the
          same letters inside a deletion.
 sat      6 400 identical letters with a 70-letter insertion in the middle, band [-10, 81): a score above 32 767.
 wide     one gap item (G = 200) and one adjacent item per band of about 1 000 / 2 000 / 4 000 / above 4 096 (the 32-bit classes 8, 16,
          32 and the several-wavefront sweep), flanks as short as the band allows.
 zero     all W against all D (score 0), and 1 x 1 items; laid between the others.

Variants: "plain"; "bias" (gap and run again with a random bias of -3 .. +1 per query letter); "own" (again with a perturbed
matrix of the item's own and no bias: such items are swept by the 32-bit kernels). Every case is present once per band class
(widths of up to 96 / 128 / 160 / 256 / 512) that can hold its diagonals, the band widened around the case inside the matrix.

Other scoring systems. What the families above take from BLOSUM62 11/1 comes from the scheme's own numbers instead (_Costs):
 * flanks are as long as it takes for a flank of identical pairs to score twice the case's largest gap cost, go + G ge, with a
   bias of -1 per letter allowed for (and never shorter than for BLOSUM62); the builder asserts 1.3 times the cost per flank;
 * W and D become the letter pair with the matrix's lowest score (x : y), "adjacent" takes 3 go / (|x : y| - 2 ge) letters of each
   (30 at least), so that two gaps beat the mismatch columns by a margin that grows with the run;
 * run letters have a diagonal entry of 4 or more, so a column stays positive under a bias of -3 and a perturbation of -2;
 * the four flank letters on either side of a gap are the four letters with the largest diagonal entries, and the letters inside
   a gap are taken from the other sixteen. A gap then cannot slide along a repeated letter, and under a cheap gap open with a
   bias (PAM30 5/2: a bias difference of 4 on two letters outweighs an open of 5) it cannot split in two around letters that
   pair with the flank's end as well as the flank's own;
 * the "zero" prefix is found by search: the matrix's W:W, then up to four pairs with negative scores whose running sum stays
   positive and ends at exactly 0. A matrix without such a prefix of five pairs or fewer gets no run/zero cases (all eight
   standard matrices have one);
 * "letters" faces each target letter 20 - 24 with the query letter it scores best against; a letter whose best score is still
   below two one-letter gaps, -2 (go + ge), cannot stand in a column (PAM30 5/2: the stop, -17 against -14) and is then only
   present inside the deletion. Corpus.letter_columns lists the letters that can.
A scheme whose lowest score does not exceed two gap extensions has no "adjacent" case and is refused (BLOSUM50 9/3)."""
import functools

import numpy as np

from diamond_amd import hip

GAPS = (1, 62, 63, 64, 65, 126, 127, 128, 129, 189, 190, 200)
RUNS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193)
BETWEEN = (63, 64, 65, 127, 128, 129)
FLANK, ADJ_FLANK, ADJ_GAP = 120, 80, 30
CLASS_WIDTHS = (96, 128, 160, 256, 512)                    # the packed sweeps' classes, by the widest band each takes
WIDE_BANDS = (1000, 2000, 4000, 4100)                      # 32-bit classes 8 / 16 / 32, several wavefronts
SAT_LEN, SAT_GAP = 6400, 70
W, D, A, R, G_ = 17, 3, 0, 1, 7
ZERO_PREFIX = ((W, W), (W, D), (W, D), (A, R), (G_, W))    # (query, target): +11 -4 -4 -1 -2
GAP_OPEN, GAP_EXTEND = 11, 1


class _Costs:
    """What the families take from the scoring system. scheme None: BLOSUM62 11/1 with the constants above."""

    def __init__(self, M, scheme):
        self.scheme, self.M = scheme, M
        if scheme is None:
            self.go, self.ge = GAP_OPEN, GAP_EXTEND
            self.x, self.y, self.zero_prefix, self.adj_gap = W, D, ZERO_PREFIX, ADJ_GAP
            self.solid, self.letter_columns = np.arange(20, dtype=np.int8), (20, 21, 22, 23, 24)
            return
        _, self.go, self.ge = scheme
        m = M[:20, :20].astype(int)
        self.x, self.y = (int(v) for v in np.unravel_index(m.argmin(), m.shape))
        low = -int(m[self.x, self.y])
        assert low > 2 * self.ge, scheme
        self.adj_gap = max(ADJ_GAP, -(-3 * self.go // (low - 2 * self.ge)))
        self.solid = np.array([a for a in range(20) if m[a, a] >= 4], np.int8)
        order = np.argsort(-np.diag(m), kind="stable")
        self.junction, self.filler = order[:4].astype(np.int8), np.sort(order[4:]).astype(np.int8)
        self.mean_diag = float(np.diag(m).mean())
        self.zero_prefix = self._find_zero_prefix(m)
        self.best_against = {L: int(M[L, :20].astype(int).argmax()) for L in range(20, 25)}                 # query letter per target letter
        self.letter_columns = tuple(L for L in range(20, 25) if int(M[L, self.best_against[L]]) > -2 * (self.go + self.ge))

    def gap_cost(self, G):
        return self.go + G * self.ge

    def flank(self, cost, least):
        """letters per flank around gaps that cost `cost` together"""
        if self.scheme is None:
            return least
        return max(least, int(-(-2 * cost // (self.mean_diag - 1))))

    def check_flank(self, letters, cost):
        if self.scheme is not None:
            score = int(sum(int(self.M[a, a]) for a in letters)) - len(letters)
            assert score >= 1.3 * cost, (self.scheme, score, cost)

    @staticmethod
    def _find_zero_prefix(m):
        """((query, target), ...): W:W, then pairs of negative scores, the running sum positive until it ends at 0; five pairs at most"""
        by_score = {}
        for a in range(20):
            for b in range(20):
                if m[a, b] < 0 and W not in (a, b):             # (a second W could pair with the first column's)
                    by_score.setdefault(int(m[a, b]), (a, b))

        def search(left, room):
            if left == 0:
                return []
            if room == 0:
                return None
            for sc in sorted(by_score):                    # the large losses first: short prefixes
                if -sc <= left:
                    rest = search(left + sc, room - 1)
                    if rest is not None:
                        return [by_score[sc]] + rest
            return None

        rest = search(int(m[W, W]), 4)
        return None if rest is None else ((W, W),) + tuple(rest)


def width_class(width):
    """The narrowest of CLASS_WIDTHS that takes a band of `width` diagonals (None: wider than all of them)"""
    for w in CLASS_WIDTHS:
        if width <= w:
            return w
    return None


class _Builder:
    def __init__(self, M, seed, costs):
        self.M = M
        self.c = costs
        self.rng = np.random.default_rng(seed)
        self.recs = []

    def gap_letters(self, n):
        """the letters inside a gap"""
        if self.c.scheme is None:
            return self.letters(n)
        return self.c.filler[self.rng.integers(0, len(self.c.filler), int(n))]

    def flank_letters(self, n, left=False, right=False):
        """a flank; left / right: a gap lies on that side"""
        a = self.letters(n)
        if self.c.scheme is not None:
            if left:
                a[:4] = self.c.junction[self.rng.integers(0, 4, min(4, len(a)))][:len(a[:4])]
            if right:
                a[-4:] = self.c.junction[self.rng.integers(0, 4, min(4, len(a)))][:len(a[-4:])]
        return a

    def run_letters(self, n):
        """letters whose identical pair stays positive under any bias and perturbation the variants apply"""
        return self.c.solid[self.rng.integers(0, len(self.c.solid), int(n))]

    def letters(self, n):
        return self.rng.integers(0, 20, int(n)).astype(np.int8)

    def own_matrix(self):
        """the context's matrix perturbed as test_random_matrices_against_oracle perturbs it; the pairs of the constructed prefixes
        keep their scores"""
        m = self.M.copy()
        m[:24, :24] = np.clip(m[:24, :24].astype(int) + self.rng.integers(-2, 3, (24, 24)), -128, 127).astype(np.int8)
        for a, b in self.c.zero_prefix or ():
            m[a, b], m[b, a] = self.M[a, b], self.M[b, a]
        return m

    def put(self, q, t, lo, hi, info, cbs=None, matrix=None, d_begin=None, d_end=None, klass=None):
        info = dict(info)
        info["class"], info["lo"], info["hi"] = klass, int(lo), int(hi)       # lo, hi: the diagonals the case was built on
        tag = "/".join(str(info[k]) for k in info if k not in ("lo", "hi"))
        self.recs.append({"query": np.asarray(q, np.int8), "cbs": cbs, "tag": tag, "info": info,
                          "targets": [{"seq": np.asarray(t, np.int8), "d_begin": int(lo if d_begin is None else d_begin),
                                       "d_end": int(hi if d_end is None else d_end), "matrix": matrix}]})

    def per_class(self, q, t, lo, hi, info, variants=("plain",), bias_free=0):
        """The case with its diagonals [lo, hi) once per variant and band class: the band is widened on both sides to the class's
        width, or to as much of it as the matrix has diagonals. bias_free: leading query letters that get no bias."""
        first, last = -(len(t) - 1), len(q) - 1                      # the matrix's diagonals
        assert first <= lo < hi <= last + 1
        for variant in variants:
            cbs = matrix = None
            if variant == "bias":
                cbs = self.rng.integers(-3, 2, len(q)).astype(np.int8)
                cbs[:bias_free] = 0
            elif variant == "own":
                matrix = self.own_matrix()
            prev = 0
            for width in CLASS_WIDTHS:
                w = min(width, last + 1 - first)
                if w > prev and w >= hi - lo:
                    extra = w - (hi - lo)
                    d0 = max(first, lo - extra // 2)
                    d0 = min(d0, last + 1 - w)
                    self.put(q, t, lo, hi, dict(info, variant=variant), cbs, matrix, d0, d0 + w, width)
                prev = width

    # ---- families ----------------------------------------------------------------------------------------------------------
    def gap_pair(self, G, direction, flank):
        a, b, x = self.flank_letters(flank, right=True), self.flank_letters(flank, left=True), self.gap_letters(G)
        self.c.check_flank(a, self.c.gap_cost(G))
        self.c.check_flank(b, self.c.gap_cost(G))
        longer, shorter = np.concatenate([a, x, b]), np.concatenate([a, b])
        return (longer, shorter, -8, G + 9) if direction == "ins" else (shorter, longer, -G - 8, 9)

    def gaps(self):
        for G in GAPS:
            for direction in ("ins", "del"):
                q, t, lo, hi = self.gap_pair(G, direction, self.c.flank(self.c.gap_cost(G), FLANK))
                self.per_class(q, t, lo, hi, {"family": "gap", "dir": direction, "G": G}, ("plain", "bias", "own"))

    def runs(self):
        for N in RUNS:
            x = self.run_letters(N)
            for form in ("origin", "score", "zero"):
                if form == "origin":
                    pq, pt = [], []
                elif form == "score":
                    pq, pt = [self.c.x] * 7, [self.c.y] * 7
                elif self.c.zero_prefix is None:
                    continue
                else:
                    pq, pt = [p[0] for p in self.c.zero_prefix], [p[1] for p in self.c.zero_prefix]
                q, t = np.concatenate([np.array(pq, np.int8), x]), np.concatenate([np.array(pt, np.int8), x])
                self.per_class(q, t, 0, 1, {"family": "run", "form": form, "N": N}, ("plain", "bias", "own"), bias_free=len(pq))

    def between(self):
        for r in BETWEEN:
            for order in ("ID", "DI"):
                a, b, c = self.flank_letters(r, right=True), self.flank_letters(r, True, True), self.flank_letters(r, left=True)
                x, y = self.gap_letters(5), self.gap_letters(5)
                if order == "ID":                                    # M r . I5 . M r . D5 . M r
                    q, t, lo, hi = np.concatenate([a, x, b, c]), np.concatenate([a, b, y, c]), -8, 14
                else:
                    q, t, lo, hi = np.concatenate([a, b, x, c]), np.concatenate([a, y, b, c]), -13, 9
                self.per_class(q, t, lo, hi, {"family": "between", "order": order, "r": r})

    def adjacent_pair(self, flank):
        a, b = self.letters(flank), self.letters(flank)
        n, x, y = self.c.adj_gap, self.c.x, self.c.y
        a[-1] = b[0] = [k for k in (A, R, G_) if k not in (x, y)][0]      # (a W or D next to the run could pair with the run's first or last letter between the gaps)
        self.c.check_flank(a, 2 * self.c.gap_cost(n))
        self.c.check_flank(b, 2 * self.c.gap_cost(n))
        return np.concatenate([a, np.full(n, x, np.int8), b]), np.concatenate([a, np.full(n, y, np.int8), b])

    def adjacent(self):
        for order in ("WD", "DW"):
            q, t = self.adjacent_pair(self.c.flank(2 * self.c.gap_cost(self.c.adj_gap), ADJ_FLANK))
            if order == "DW":
                q, t = t, q
            self.per_class(q, t, -self.c.adj_gap - 8, self.c.adj_gap + 9, {"family": "adjacent", "order": order})

    def letter_cases(self):
        positive = [(a, b) for a in range(20) for b in range(20) if a != b and self.M[a, b] > 0]
        for kind in ("columns", "deletion"):
            q = self.letters(150)
            t = q.copy()
            for k, p in enumerate(range(6, 144, 6)):
                if k % 2 == 0:
                    t[p] = 20 + (k // 2) % 5                             # B J Z X * in the target: the substitution byte carries it
                    if self.c.scheme is not None:
                        q[p] = self.c.best_against[int(t[p])]
                else:
                    q[p], t[p] = positive[int(self.rng.integers(0, len(positive)))]
            lo, hi = -8, 9
            if kind == "deletion":
                x = np.array([20, 21, 22, 23, 24, 5, 20, 21], np.int8)
                x[5] |= -128
                t = np.concatenate([t[:75], x, t[75:]])
                lo, hi = -16, 9
            for s in (q, t):
                at = np.arange(3, len(s), 11)
                s[at] = (s[at].astype(np.uint8) | 0x80).astype(np.int8)
            self.per_class(q, t, lo, hi, {"family": "letters", "kind": kind})

    def saturation(self):
        a, b, x = self.letters(SAT_LEN // 2), self.letters(SAT_LEN // 2), self.letters(SAT_GAP)
        q, t = np.concatenate([a, x, b]), np.concatenate([a, b])
        for width, (lo, hi) in ((96, (-10, SAT_GAP + 11)), (128, (-28, SAT_GAP + 30))):
            self.put(q, t, lo, hi, {"family": "sat", "G": SAT_GAP, "variant": "plain"}, klass=width)

    def wide(self):
        for k, band in enumerate(WIDE_BANDS):
            direction = ("ins", "del")[k % 2]
            flank = -(-(band - 199) // 4) + 8                        # 4 flank + 199 diagonals >= band
            q, t, lo, hi = self.gap_pair(200, direction, self.c.flank(self.c.gap_cost(200), flank))
            d0 = -(len(t) - 1) + (len(q) + len(t) - 1 - band) // 2
            assert d0 <= lo and hi <= d0 + band
            self.put(q, t, lo, hi, {"family": "wide", "kind": "gap", "dir": direction, "G": 200, "variant": "plain"}, None, None, d0, d0 + band, band)
            flank = -(-(band - 2 * ADJ_GAP + 1) // 4) + 8
            q, t = self.adjacent_pair(self.c.flank(2 * self.c.gap_cost(self.c.adj_gap), flank))
            if k % 2:
                q, t = t, q
            d0 = -(len(t) - 1) + (len(q) + len(t) - 1 - band) // 2
            self.put(q, t, -self.c.adj_gap - 8, self.c.adj_gap + 9, {"family": "wide", "kind": "adjacent", "order": ("WD", "DW")[k % 2], "variant": "plain"}, None, None, d0, d0 + band, band)

    def neighbours(self, every=9):
        """items of score 0 and 1 x 1 items between the others"""
        out, k = [], 0
        keep, self.recs = self.recs, []
        for n, rec in enumerate(keep):
            out.append(rec)
            if n % every == every - 1:
                if k % 2 == 0:
                    n_q, n_t = int(self.rng.integers(1, 90)), int(self.rng.integers(1, 90))
                    self.put(np.full(n_q, self.c.x, np.int8), np.full(n_t, self.c.y, np.int8), -(n_t - 1), n_q, {"family": "zero", "kind": "WxD", "n": k, "variant": "plain"},
                             cbs=None if k % 4 else np.zeros(n_q, np.int8), klass=width_class(n_q + n_t - 1))
                else:
                    x = self.letters(1)
                    self.put(x, x.copy(), 0, 1, {"family": "zero", "kind": "1x1", "n": k, "variant": "plain"}, klass=96)
                out.append(self.recs.pop())
                k += 1
        self.recs = out


class Corpus:
    """recs: the records in construction order (a long case next to short neighbours); shuffled: a permutation of them; M: the
    context's matrix; params; scheme (None: BLOSUM62 11/1), gap_open, gap_extend; what the families took from the scheme: adj_gap,
    zero_prefix (None: no run/zero cases), low_pair (the letters that stand for W and D), letter_columns."""

    def matrix_of(self, rec):
        m = rec["targets"][0]["matrix"]
        return self.M if m is None else m

    def width(self, rec):
        t = rec["targets"][0]
        return t["d_end"] - t["d_begin"]

    def cells(self):
        return sum(min(len(r["query"]), len(r["targets"][0]["seq"])) * self.width(r) for r in self.recs)

    def select(self, **want):
        return [k for k, r in enumerate(self.recs) if all(r["info"].get(a) == b for a, b in want.items())]


def corpus(scheme=None):
    """The corpus under BLOSUM62 11/1, or rebuilt for scheme = (matrix name, gap open, gap extend); one object per scheme"""
    return _corpus_cached(None if scheme is None else tuple(scheme))


@functools.lru_cache(maxsize=None)
def _corpus_cached(scheme):
    params = hip.default_params() if scheme is None else hip.matrix_params(*scheme)
    M = hip.matrix_of(params)
    costs = _Costs(M, scheme)
    assert (params.gap_open, params.gap_extend) == (costs.go, costs.ge)
    b = _Builder(M, 6364, costs)
    b.gaps()
    b.runs()
    b.between()
    b.adjacent()
    b.letter_cases()
    b.saturation()
    b.wide()
    b.neighbours()
    c = Corpus()
    c.params, c.M, c.recs = params, M, b.recs
    c.scheme, c.gap_open, c.gap_extend = scheme, costs.go, costs.ge
    c.adj_gap, c.zero_prefix, c.low_pair, c.letter_columns = costs.adj_gap, costs.zero_prefix, (costs.x, costs.y), costs.letter_columns
    c.shuffled = np.random.default_rng(99).permutation(len(c.recs))
    return c


@functools.lru_cache(maxsize=None)
def _oracle_cached(scheme):
    import oracle_py as orc
    c = corpus(scheme)
    out = []
    for rec in c.recs:
        t = rec["targets"][0]
        m = c.matrix_of(rec)
        rc, o, tr = orc.banded_swipe(rec["query"], rec["cbs"], t["seq"], t["d_begin"], t["d_end"], m, c.gap_open, c.gap_extend, orc.TRACEBACK)
        assert rc == 0, rec["tag"]
        rc, st = orc.swipe_stats(rec["query"], rec["cbs"], t["seq"], t["d_begin"], t["d_end"], m, c.gap_open, c.gap_extend, 510)
        assert rc == 0, rec["tag"]
        tr.setflags(write=False)
        out.append((o, tr, st))
    return tuple(out)


def oracle(c):
    """(hsp dict, transcript bytes, statistics dict) of oracle/banded_swipe.c for every record, computed once"""
    assert c is corpus(c.scheme)
    return _oracle_cached(c.scheme)


def gap_runs(tr):
    """[(operation, letters)] of the gap runs of a packed transcript, in order, and for each the number of match / substitution
    columns since the run before (or the start)"""
    runs, k, cols = [], 0, 0
    tr = [int(x) for x in tr]
    while k < len(tr):
        op = tr[k] >> 6
        if op == 0:
            cols += tr[k] & 63
            k += 1
        elif op == 3:
            cols += 1
            k += 1
        else:
            n = 0
            while k < len(tr) and tr[k] >> 6 == op:
                n += (tr[k] & 63) if op == 1 else 1
                k += 1
            runs.append((op, n, cols))
            cols = 0
    return runs
