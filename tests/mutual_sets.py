"""TEST INFRASTRUCTURE ONLY -- inputs for the tests of the mutual-coverage search (--min-len-ratio; equal --query-cover /
--subject-cover). The length test can only be checked where it removes something, and the families of diamond_amd.synth have
near-equal lengths; here every member of a family is a random slice of 45-100 % of a mutated copy of the family's base, so that
members of one family differ in length by up to a factor of 2.2 and share seeds all the same.

generate() returns (db, db_off, q, q_off) like synth.generate: letters without delimiters and n + 1 offsets, in an order that is
NOT length-sorted and holds equal lengths (the reference's sort breaks ties by descending index: a stable sort is wrong).
`near` families are near-identical (1 % substitutions) and only truncated at their ends: their window scores pass 255, which is what
the deferred pass of the seed stage needs, and their truncations give it batch mates that fail the length test."""
import numpy as np

from diamond_amd import workload


def generate(families=80, members=6, queries=2, seed=1, lo=120, hi=520, near=0, near_members=12, near_queries=3, exact_34=True):
    rng = np.random.default_rng(seed)

    def member(base, rate, ends_only):
        m = base.copy()
        flip = rng.random(len(m)) < rate
        m[flip] = rng.integers(0, 20, int(flip.sum()))
        n = len(m)
        keep = int(round(n * rng.uniform(0.45, 1.0)))
        a = int(rng.integers(0, n - keep + 1))
        if ends_only and rng.random() < 0.5:
            a = 0 if rng.random() < 0.5 else n - keep
        return m[a:a + keep]

    db, q = [], []
    for f in range(families + near):
        is_near = f >= families
        base = rng.integers(0, 20, int(rng.integers(lo, hi + 1))).astype(np.int8)
        rate = 0.01 if is_near else float(rng.uniform(0.05, 0.25))
        for _ in range(near_members if is_near else members):
            db.append(member(base, rate, is_near))
        for _ in range(near_queries if is_near else queries):
            q.append(member(base, rate, is_near))
        if f < 4:                                      # equal lengths on both sides (ties of the length sort) ...
            twin = base.copy()
            twin[::7] = rng.integers(0, 20, len(twin[::7]))
            db.append(twin[:len(db[-1])])
            q.append(base[:len(q[-1])].copy())
        if exact_34 and f == 4:                        # ... and lengths in the exact ratio 3 : 4 (0.75 passes, the next ratio up does not)
            db.append(base[:120].copy()); q.append(base[:90].copy())
            db.append(base[10:100].copy()); q.append(base[:120].copy())
    perm_t, perm_q = rng.permutation(len(db)), rng.permutation(len(q))
    db, q = [db[i] for i in perm_t], [q[i] for i in perm_q]
    off = lambda seqs: np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return np.concatenate(db).astype(np.int8), off(db), np.concatenate(q).astype(np.int8), off(q)


def length_sorted(data, off):
    """(data, off) with the sequences in the reference's length-sorted order: (length, index) descending."""
    lens = np.diff(off)
    order = sorted(range(len(lens)), key=lambda i: (int(lens[i]), i), reverse=True)
    parts = [data[off[i]:off[i + 1]] for i in order]
    return np.concatenate(parts).astype(np.int8), np.concatenate([[0], np.cumsum(lens[order])]).astype(np.int64), np.array(order)


def sorted_blocks(db, doff, q, qoff):
    """Both sides length-sorted and laid out as SequenceSets: (qdata, qlimits, tdata, tlimits)."""
    sq, sqo, _ = length_sorted(q, qoff)
    st, sto, _ = length_sorted(db, doff)
    qd, ql = workload.sequence_set(sq, sqo)
    td, tl = workload.sequence_set(st, sto)
    return qd, ql, td, tl


def passes(qlen, tlen, mlr):
    """length_ratio_passes, in Python's doubles (IEEE division, as the reference's)."""
    return float(qlen) / float(tlen) >= mlr and float(tlen) / float(qlen) >= mlr
