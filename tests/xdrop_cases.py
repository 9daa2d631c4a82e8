"""Test data of the x-drop edge tests (tests/test_xdrop_cases.py, tests/test_gpu_xdrop_edges.py): one seeded block pair and a list
of seed hits laid at the places where xdrop_seg_kernel (csrc/bias_kernels.hip) can leave the per-letter walk of xdrop_core.h -- it
fetches sixteen letters at a time in either direction and leans on the blocks' 256-byte perimeter. Letter pairs are chosen from a
wanted score series with the context's matrix, so every family is exact by construction and not by luck. corpus() is built on
BLOSUM62 11/1; corpus(params) builds the same families on another system's matrix (hip.matrix_params): where that matrix has no
letter pair of a wanted score the nearest score it has stands in (the larger of two equally near ones: PAM30 has no 3, 4, 5, its
strong matches score 6), the ties use the four smallest k for which it has both -k and +k (PAM30: 1, 2, 6, 7), and the boundary
family is built once more around the system's own x-drop default, Corpus.default_xdrop = ceil((12.3 ln 2 + ln K) / lambda).

A hit's family is the first word of its tag; Corpus.info holds the same as a tuple.

 grid      the delimiter's place inside a chunk. "left": a letters before the seed in the query, b in the target, identical as far as
           both reach, a, b = 0 .. 18 -- the left walk ends on whichever delimiter comes first. "right": the seed's own letter, then
           a more letters in the query and b in the target (the entry refuses a seed on a query delimiter, so the seed letter leads
           the run): the right walk takes 1 + min(a, b) letters.
 long      identical runs of 15 .. 2000 letters on one side, and every left x right pair of the six shortest.
 corner    the first and the last sequence of both blocks are one 48-letter sequence: seeds at offset 0, len - 1 and on the chunk
           boundaries, subjects on the first and last letter of a target; a one-letter query, a one-letter target.
 delim     the subject on a delimiter with seed_offset 0 (nothing to walk: score 0, len 0), and with a left side to walk.
 boundary  per direction, x-drop value x, d = -1 / 0 / +1 and chunk offset o: strong matches, then mismatches that lose exactly
           x + d, then a stronger run; the letter before which the loss is complete (the first of the stronger run) is letter
           o of the walk, or letter o + 32 where the loss does not fit in front of o. Three hits of one variant form a triple.
 tie       L strong letters, then -k, +k: the sum returns to its best, which must stay where it was first reached.
 homolog   mutated copies at 50 / 70 / 90 % identity with twelve seeds on the diagonal: plain, with the soft-mask bit on a third
           of the letters, with B J Z X * in both sequences, and with a low-complexity query (first half one residue).
"""
import functools
import math

import numpy as np

from diamond_amd import hip, workload

XDROPS = (1, 2, 7, 20, 10 ** 6)
DEFAULT_XDROP = 20                          # raw_ungapped_xdrop of BLOSUM62 11/1: what xdrop=0 means
GRID = 19                                   # a, b = 0 .. 18
LONG_RUNS = (15, 16, 17, 31, 32, 33, 47, 48, 49, 100, 300, 2000)
OFFSETS = (0, 1, 14, 15, 16, 17)
LAUNCH_SIZES = (1, 255, 256, 257)
CORNER_LEN = 48
GRID_VARIANTS, BOUNDARY_VARIANTS, TIE_VARIANTS, HOMOLOG_PAIRS, SEEDS_PER_PAIR = 6, 80, 2, 400, 12


def default_xdrop(params):
    """config.raw_ungapped_xdrop: the raw score of 12.3 bits, what xdrop = 0 means"""
    return int(math.ceil((12.3 * math.log(2.0) + math.log(params.K)) / params.lambda_))


def _reference_xdrop(M, q, cbs, t, qa, sa, xdrop):
    score = st = 0
    n, delta, length = 1, 0, 0
    i, j = qa - 1, sa - 1
    while score - st < xdrop and (q[i] & 31) != 31 and (t[j] & 31) != 31:
        st += int(M[q[i] & 31, t[j] & 31]) + (int(cbs[i]) if cbs is not None else 0)
        if st > score:
            score, delta = st, n
        i -= 1; j -= 1; n += 1
    i, j, st, n = qa, sa, score, 1
    while score - st < xdrop and (q[i] & 31) != 31 and (t[j] & 31) != 31:
        st += int(M[q[i] & 31, t[j] & 31]) + (int(cbs[i]) if cbs is not None else 0)
        if st > score:
            score, length = st, n
        i += 1; j += 1; n += 1
    return delta, length + delta, score


def plain_inputs(M, q, cbs, t):
    """The same values as Python objects, which _reference_xdrop indexes several times faster than numpy arrays: the matrix as
    a dict keyed by (query letter, target letter), the blocks as bytes (only their low five bits are read), the bias as a list."""
    Md = {(a, b): int(M[a, b]) for a in range(32) for b in range(32)}
    return Md, np.ascontiguousarray(q, np.int8).tobytes(), (None if cbs is None else [int(x) for x in cbs]), np.ascontiguousarray(t, np.int8).tobytes()


def walk_ends(M, q, cbs, t, qa, sa, xdrop):
    """How the two walks of _reference_xdrop end and how many letters each adds: ("x" | "d", letters) for the left, then the right
    walk. "x": the sum fell xdrop below the best; "d": a delimiter."""
    out = []
    score = 0
    for i, j, d in ((qa - 1, sa - 1, -1), (qa, sa, 1)):
        st, n = score, 0
        while score - st < xdrop and (q[i] & 31) != 31 and (t[j] & 31) != 31:
            st += int(M[q[i] & 31, t[j] & 31]) + (int(cbs[i]) if cbs is not None else 0)
            score = max(score, st)
            i += d; j += d; n += 1
        out.append(("x" if score - st >= xdrop else "d", n))
    return out


def diagonal_sums(M, q, t, qa, sa, direction, start=0):
    """Running sums of the letter scores from the seed on in one direction, up to the next delimiter (no x-drop, no bias)."""
    i, j = (qa - 1, sa - 1) if direction < 0 else (qa, sa)
    out, st = [], start
    while (q[i] & 31) != 31 and (t[j] & 31) != 31:
        st += int(M[q[i] & 31, t[j] & 31])
        out.append(st)
        i += direction; j += direction
    return out


class Corpus:
    """qd, ql, td, tl: the two blocks (workload.sequence_set); hits: SEED_HIT_DTYPE; tags / info: one per hit; cbs: the host's
    Hauser bias of the query block (hip.extend_plan); M: the matrix; params; default_xdrop: what xdrop = 0 means under params;
    xdrops: XDROPS and default_xdrop, the values the boundary family is built around and the tests run; tie_ks."""

    def qa(self, k):
        return int(self.ql[self.hits["query"][k]]) + int(self.hits["seed_offset"][k])

    def expected(self, xdrop, use_bias, index=None):
        """What dmnd_xdrop_ungapped has to return: fields i, j, len, score per hit (all hits, or those of `index`)."""
        ref = reference(self, xdrop, use_bias)
        h = self.hits
        out = np.zeros(len(h), dtype=np.dtype([("i", "<i4"), ("j", "<i8"), ("len", "<i4"), ("score", "<i4")], align=True))
        out["i"], out["j"], out["len"], out["score"] = h["seed_offset"] - ref[:, 0], h["subject"] - ref[:, 0], ref[:, 1], ref[:, 2]
        return out if index is None else out[index]


class _Builder:
    def __init__(self, M, seed, boundary_xdrops):
        self.M = M
        self.rng = np.random.default_rng(seed)
        self.qs, self.ts, self.rows, self.tags, self.info = [], [], [], [], []
        self.boundary_xdrops = boundary_xdrops
        self.by_score = {}
        for a in range(20):
            for b in range(20):
                self.by_score.setdefault(int(M[a, b]), []).append((a, b))
        have = sorted(self.by_score)
        # a wanted score the matrix does not have: the nearest it has, of two equally near ones the larger in magnitude
        self.nearest = {s: s if s in self.by_score else min(have, key=lambda c: (abs(c - s), -abs(c))) for s in range(-8, 9)}
        self.tie_ks = tuple(k for k in range(1, 20) if k in self.by_score and -k in self.by_score)[:4]
        assert len(self.tie_ks) == 4 and all(self.nearest[s] * s > 0 for s in (-4, -3, 4, 5, 6)) and all(-y in self.by_score for y in range(5))

    def letters(self, n):
        return self.rng.integers(0, 20, int(n)).astype(np.int8)

    def series(self, scores):
        """Query and target letters whose pairwise scores are `scores`."""
        q, t = np.zeros(len(scores), np.int8), np.zeros(len(scores), np.int8)
        for k, s in enumerate(scores):
            c = self.by_score[self.nearest.get(int(s), int(s))]
            q[k], t[k] = c[int(self.rng.integers(0, len(c)))]
        return q, t

    def strong(self, n):
        return [int(x) for x in self.rng.integers(4, 7, int(n))]

    def add(self, q, t):
        self.qs.append(np.asarray(q, np.int8)); self.ts.append(np.asarray(t, np.int8))
        return len(self.qs) - 1, len(self.ts) - 1

    def hit(self, qid, off, tid, tpos, info):
        self.rows.append((qid, int(off), tid, int(tpos)))
        self.info.append(info)
        self.tags.append("/".join(str(x) for x in info))

    def case(self, Lq, Lt, Rq, Rt, info):
        """A pair of sequences around one seed. L*: the letters the left walk meets, in walking order (the first one lies just
        before the seed); R*: the letters from the seed on to the right. Rt may be empty: the subject is then the delimiter."""
        q = np.concatenate([np.asarray(Lq, np.int8)[::-1], np.asarray(Rq, np.int8)])
        t = np.concatenate([np.asarray(Lt, np.int8)[::-1], np.asarray(Rt, np.int8)])
        assert len(Rq) >= 1 and len(t) >= 1
        qid, tid = self.add(q, t)
        self.hit(qid, len(Lq), tid, len(Lt), info)

    # ---- families ------------------------------------------------------------------------------------------------------
    def run_pair(self, a, b):
        """a letters and b letters, identical as far as both reach"""
        x = self.letters(max(a, b))
        y = self.letters(max(a, b))
        n = min(a, b)
        y[:n] = x[:n]
        return x[:a], y[:b]

    def grid(self):
        for v in range(GRID_VARIANTS):
            for a in range(GRID):
                for b in range(GRID):
                    Lq, Lt = self.run_pair(a, b)
                    self.case(Lq, Lt, self.letters(self.rng.integers(1, 5)), self.letters(self.rng.integers(1, 5)), ("grid", "left", a, b, v))
                    Rq, Rt = self.run_pair(a + 1, b + 1)
                    self.case(self.letters(self.rng.integers(0, 4)), self.letters(self.rng.integers(0, 4)), Rq, Rt, ("grid", "right", a, b, v))

    def long(self):
        for n in LONG_RUNS:
            Lq, Lt = self.run_pair(n, n)
            self.case(Lq, Lt, self.letters(2), self.letters(3), ("long", "left", n, 0))
            Rq, Rt = self.run_pair(n, n)
            self.case(self.letters(3), self.letters(2), Rq, Rt, ("long", "right", 0, n))
        for a in LONG_RUNS[:6]:
            for b in LONG_RUNS[:6]:
                Lq, Lt = self.run_pair(a, a)
                Rq, Rt = self.run_pair(b, b)
                self.case(Lq, Lt, Rq, Rt, ("long", "both", a, b))

    def boundary_series(self, x, d, o):
        """(scores in walking order, index of the decisive letter)"""
        D = x + d
        m = max(1, -(-D // 4))
        w = o if o >= m else o + 32
        if D == 0:
            drops = [0]
        else:
            drops = [D // m + (1 if k < D % m else 0) for k in range(m)]
            self.rng.shuffle(drops)
        assert len(drops) == m and sum(drops) == D and all(0 <= y <= 4 for y in drops)
        tail = self.strong(D // 4 + 3)                    # regains more than it lost: a new best if the walk goes on
        return self.strong(w - m) + [-y for y in drops] + tail + [int(y) for y in self.rng.integers(-2, 3, 2)], w

    def boundary(self):
        for v in range(BOUNDARY_VARIANTS):
            for direction in ("left", "right"):
                for x in self.boundary_xdrops:
                    for o in OFFSETS:
                        for d in (-1, 0, 1):
                            s, w = self.boundary_series(x, d, o)
                            wq, wt = self.series(s)
                            info = ("boundary", direction, x, d, o, v)
                            if direction == "left":
                                n = int(self.rng.integers(1, 4))
                                self.case(wq, wt, self.letters(n), self.letters(n), info)
                            else:
                                n = int(self.rng.integers(0, 3))
                                self.case(self.letters(n), self.letters(n), wq, wt, info)

    def tie(self):
        for v in range(TIE_VARIANTS):
            for direction in ("left", "right"):
                for L in range(0, 21):
                    for k in self.tie_ks:
                        for end in ("delimiter", "loss"):
                            s = self.strong(L) + [-k, k] + ([] if end == "delimiter" else [-4, -4, -3, -4, -4, -4])
                            wq, wt = self.series(s)
                            info = ("tie", direction, L, k, end, v)
                            if direction == "left":
                                rq, rt = self.series([-4])                                # a right walk that adds nothing
                                self.case(wq, wt, rq, rt, info)
                            else:
                                self.case(np.zeros(0, np.int8), np.zeros(0, np.int8), wq, wt, info)

    def homolog(self):
        kinds = ("plain", "softmask", "nonstd", "lowcomplex")
        for v in range(HOMOLOG_PAIRS):
            kind, ident = kinds[v % 4], (0.5, 0.7, 0.9)[(v // 4) % 3]
            n = int(self.rng.integers(100, 220))
            q = self.letters(n)
            if kind == "lowcomplex":
                q[: n // 2] = q[0]
            core = q.copy()
            mut = self.rng.random(n) > ident
            core[mut] = self.letters(int(mut.sum()))
            a = int(self.rng.integers(0, 40))
            t = np.concatenate([self.letters(a), core, self.letters(self.rng.integers(0, 40))])
            if kind == "nonstd":
                for s in (q, t):
                    at = self.rng.random(len(s)) < 0.05
                    s[at] = self.rng.integers(20, 25, int(at.sum())).astype(np.int8)
            if kind == "softmask":
                for s in (q, t):
                    at = self.rng.random(len(s)) < 1.0 / 3
                    s[at] = (s[at].astype(np.uint8) | 0x80).astype(np.int8)
            qid, tid = self.add(q, t)
            for p in self.rng.integers(0, n, SEEDS_PER_PAIR):
                self.hit(qid, p, tid, a + int(p), ("homolog", kind, int(ident * 100), v))

    def corners(self, first, last):
        """first / last: (query id, target id) of the 48-letter sequence at the head / tail of both blocks"""
        n = CORNER_LEN
        for qn, qid in (("first", first[0]), ("last", last[0])):
            for tn, tid in (("first", first[1]), ("last", last[1])):
                for off, tpos in ((0, 0), (n - 1, n - 1), (15, 15), (16, 16), (31, 31), (32, 32), (0, n - 1), (n - 1, 0)):
                    self.hit(qid, off, tid, tpos, ("corner", qn, tn, off, tpos))
        x = np.array([7], np.int8)
        q1, t1 = self.add(x, x)
        self.hit(q1, 0, t1, 0, ("corner", "one-letter", "one-letter", 0, 0))
        for tpos in (0, 20, n - 1):
            self.hit(q1, 0, first[1], tpos, ("corner", "one-letter", "first", 0, tpos))
            self.hit(q1, 0, last[1], tpos, ("corner", "one-letter", "last", 0, tpos))
        for off in (0, 20, n - 1):
            self.hit(first[0], off, t1, 0, ("corner", "first", "one-letter", off, 0))
            self.hit(last[0], off, t1, 0, ("corner", "last", "one-letter", off, 0))
        # the subject on a delimiter: the one behind the first, a middle and the last target
        for tn, tid in (("first", first[1]), ("middle", t1), ("last", last[1])):
            for qn, qid in (("first", first[0]), ("one-letter", q1), ("last", last[0])):
                self.hit(qid, 0, tid, len(self.ts[tid]), ("delim", "nothing", qn, tn))
        for tn, tid in (("first", first[1]), ("last", last[1])):
            for qn, qid in (("first", first[0]), ("last", last[0])):
                self.hit(qid, n - 1, tid, n, ("delim", "walks", qn, tn))
        X = self.letters(20)                              # twenty identical letters before the seed and before the delimiter
        qx, tx = self.add(np.concatenate([X, self.letters(1)]), X)
        self.hit(qx, 20, tx, 20, ("delim", "walks", "run", "run"))


def corpus(params=None):
    """The corpus on BLOSUM62 11/1, or on the matrix of `params` (hip.matrix_params); one object per system"""
    return _corpus_cached(None if params is None else bytes(params))


@functools.lru_cache(maxsize=None)
def _corpus_cached(key):
    params = hip.default_params() if key is None else hip.Params.from_buffer_copy(key)
    M = hip.matrix_of(params)
    x0 = default_xdrop(params)
    assert key is not None or x0 == DEFAULT_XDROP
    xdrops = XDROPS if x0 in XDROPS else tuple(sorted(XDROPS + (x0,)))
    b = _Builder(M, 20240, xdrops[:-1])
    S = b.letters(CORNER_LEN)
    first = b.add(S, S)
    b.grid()
    b.long()
    b.boundary()
    b.tie()
    b.homolog()
    last = b.add(S, S)
    b.corners(first, last)
    # the corner sequences must be the blocks' first and last: move `last` behind the sequences corners() added
    order_q = [i for i in range(len(b.qs)) if i != last[0]] + [last[0]]
    order_t = [i for i in range(len(b.ts)) if i != last[1]] + [last[1]]
    new_q = {old: new for new, old in enumerate(order_q)}
    new_t = {old: new for new, old in enumerate(order_t)}
    qs, ts = [b.qs[i] for i in order_q], [b.ts[i] for i in order_t]

    def block(seqs):
        off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
        return workload.sequence_set(np.concatenate(seqs).astype(np.int8), off)

    c = Corpus()
    c.params, c.M, c.key = params, M, key
    c.default_xdrop, c.xdrops, c.tie_ks = x0, xdrops, b.tie_ks
    c.qd, c.ql = block(qs)
    c.td, c.tl = block(ts)
    hits = np.zeros(len(b.rows), dtype=hip.SEED_HIT_DTYPE)
    for k, (qid, off, tid, tpos) in enumerate(b.rows):
        hits[k]["query"], hits[k]["seed_offset"], hits[k]["subject"] = new_q[qid], off, int(c.tl[new_t[tid]]) + tpos
    c.hits, c.tags, c.info = hits, b.tags, b.info
    c.n_queries, c.n_targets = len(qs), len(ts)
    c.cbs = hip.extend_plan(params, c.qd, c.ql, c.td, c.tl, np.zeros(0, hip.SEED_HIT_DTYPE))[0]
    c.shuffled = np.random.default_rng(77).permutation(len(hits))
    c._plain = {False: plain_inputs(M, c.qd, None, c.td), True: plain_inputs(M, c.qd, c.cbs, c.td)}
    return c


@functools.lru_cache(maxsize=None)
def _reference_cached(key, xdrop, use_bias):
    c = _corpus_cached(key)
    Md, q, cbs, t = c._plain[bool(use_bias)]
    out = np.zeros((len(c.hits), 3), np.int64)
    qa = c.ql[c.hits["query"]] + c.hits["seed_offset"]
    for k in range(len(c.hits)):
        out[k] = _reference_xdrop(Md, q, cbs, t, int(qa[k]), int(c.hits["subject"][k]), xdrop)
    out.setflags(write=False)
    return out


def reference(c, xdrop, use_bias):
    """(delta, len, score) of _reference_xdrop for every hit of the corpus, computed once per setting"""
    assert c is _corpus_cached(c.key)
    return _reference_cached(c.key, int(xdrop), bool(use_bias))


def family_counts(c):
    out = {}
    for i in c.info:
        out[i[0]] = out.get(i[0], 0) + 1
    return out
