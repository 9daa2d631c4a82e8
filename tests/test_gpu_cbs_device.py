"""-m gpu: the composition-based matrix adjustment of --comp-based-stats 2 - 5 on the device (diamond_amd/csrc/cbs_kernels.hip;
arithmetic, lane schedule and guards in cbs_core.h). The kernel's own results through dmnd_cbs_target_matrices_device -- no host
fallback there -- against the reference's answers (tests/golden/cbs_*.tap) and against the host form at the structural edges; the
hand-back path; and dmnd_extend with the kernel against dmnd_extend with the host form (DMND_CBS_DEVICE=0), records and transcripts."""
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import tapfile  # noqa: E402
import cbs_emu_py as ce  # noqa: E402
from diamond_amd import hip, workload  # noqa: E402
from test_cbs_device_emu import CASES, MAX_HANDED_BACK, check_table  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0x55


class Env:
    """environment switches the library reads per call, for the duration of a block"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _device(ctx, mode, pairs, with_scores=False):
    """pairs: (query_comp, query_true_aa, target) -> rule, status, matrices (pre-filled with FILL) [, scores]"""
    pre = np.full((len(pairs), 32, 32), FILL, np.int8)
    return ctx.cbs_target_matrices_device(mode, [p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs], matrices=pre, with_scores=with_scores)


@pytest.mark.parametrize("name,matrix,mode", CASES)
def test_goldens_through_the_kernel(name, matrix, mode):
    hdr, adj, tmx = tapfile.read_cbs_tap(os.path.join(HERE, "golden", name))
    p = hip.matrix_params(matrix)
    eps_round = ce.guards()[0]
    ctx = hip.Context(params=p)
    try:
        recs = tmx + adj
        rule, status, mats, scores = _device(ctx, mode, [(r["query_comp"], r["query_len"], r["target"]) for r in recs], with_scores=True)
    finally:
        ctx.close()
    n = handed = 0
    seen = set()
    worst = 0.0
    for k, r in enumerate(recs):
        if r["rule"] != ce.RULE_SCALE_OLD:
            n += 1
            handed += status[k] != 0
        else:
            assert status[k] == ce.ST_RULE
        if status[k] != ce.ST_RULE:
            assert rule[k] == r["rule"], k
        if status[k] == 0:
            seen.add(int(rule[k]))
        if status[k] == 0 and rule[k] == ce.RULE_REL_ENTROPY:
            if k < len(tmx):
                check_table(mats[k], r, p)
            want = ce.host_pair(p, mode, r["query_comp"], r["query_len"], r["target"])
            assert np.array_equal(mats[k], want["matrix"]), k
            worst = max(worst, float(np.abs(scores[k] - want["scores"]).max()))
        else:
            assert (mats[k] == FILL).all(), k
            if k < len(tmx):          # the host form computes it: the reference's table
                check_table(hip.cbs_target_matrix(p, r["rule"], r["query_comp"], r["query_len"], r["target"]), r, p)
    print("%s: %d pairs without SCALE_OLD, %d handed back, largest score deviation from the host %.3g" % (name, n, handed, worst))
    assert seen == ({-1, 4} if mode in (2, 3) else {4})
    assert handed <= MAX_HANDED_BACK * n, (handed, n)
    assert worst < eps_round / 10


def _edge_list():
    out = []
    for name, q, t in ce.edge_pairs():
        comp, n = hip.cbs_composition(q)
        out.append((comp, n, t))
    return out


@pytest.mark.parametrize("mode", [3, 4, 5])
def test_structural_edges_against_the_host_form(mode):
    p = hip.default_params()
    base = _edge_list()
    ctx = hip.Context(params=p)
    try:
        want = [hip.cbs_rule(p, mode, c, n, t) for c, n, t in base]
        by_n = {}
        for n_pairs in (1, 63, 64, 65, 3000):
            pairs = [base[(k * 7) % len(base)] for k in range(n_pairs)]
            by_n[n_pairs] = (pairs, _device(ctx, mode, pairs))
    finally:
        ctx.close()
    tables = {}
    decided = 0
    r0, s0, m0 = by_n[3000][1]
    first = {}
    for k in range(3000):
        first.setdefault((k * 7) % len(base), k)
    for n_pairs, (pairs, (rule, status, mats)) in by_n.items():
        for k in range(n_pairs):
            b = (k * 7) % len(base)
            comp, n, t = base[b]
            if status[k] == 0:
                decided += 1
                assert rule[k] == want[b], (n_pairs, k)
                if rule[k] == ce.RULE_REL_ENTROPY:
                    if b not in tables:
                        tables[b] = hip.cbs_target_matrix(p, 4, comp, n, t)
                    assert np.array_equal(mats[k], tables[b]), (n_pairs, k, b)
                else:
                    assert (mats[k] == FILL).all()
            else:
                assert (mats[k] == FILL).all()
                assert status[k] in (1, 2, 3) and (mode != 4 or status[k] != ce.ST_RULE)
            # a pair's result does not depend on its place in the list or on the list's length
            f = first[b]
            assert (rule[k], status[k]) == (r0[f], s0[f]) and np.array_equal(mats[k], m0[f]), (n_pairs, k, b)
    assert decided > (600 if mode == 5 else 2000)          # (mode 5: the lambda-rescaling pairs all go back)


def test_one_residue_target_and_degenerate_pairs():
    p = hip.default_params()
    comp, n = hip.cbs_composition(np.arange(20, dtype=np.int8))
    t = np.arange(20, dtype=np.int8)
    ctx = hip.Context(params=p)
    try:
        # mode 1: nothing to adjust
        rule, status, mats = _device(ctx, 1, [(comp, n, t)])
        assert (rule[0], status[0]) == (-1, 0) and (mats == FILL).all()
        # an empty target among others, a query without residues
        rule, status, mats = _device(ctx, 4, [(comp, n, t), (comp, n, np.zeros(0, np.int8)), (comp, 0, t), (comp, 1, t)])
        assert list(rule) == [4, -1, -1, 4] and list(status[1:3]) == [0, 0] and (mats[1:3] == FILL).all()
        for k in (0, 3):
            if status[k] == 0:
                assert np.array_equal(mats[k], hip.cbs_target_matrix(p, 4, comp, (n, 0, 0, 1)[k], t))
        assert status[0] == 0
        # one residue repeated: a long, ill-conditioned iteration; if the device gives it up, then by the iteration guard
        t1 = np.full(80, 9, np.int8)
        rule, status, mats = _device(ctx, 4, [(comp, n, t1)])
        assert rule[0] == 4 and status[0] in (0, ce.ST_ITERATIONS)
        if status[0] == 0:
            assert np.array_equal(mats[0], hip.cbs_target_matrix(p, 4, comp, n, t1))
        else:
            assert (mats == FILL).all()
    finally:
        ctx.close()


def test_iteration_cap_of_one_hands_every_adjusted_pair_back():
    p = hip.default_params()
    base = _edge_list()
    ctx = hip.Context(params=p)
    try:
        with Env(DMND_CBS_DEVICE_MAX_ITS=1):
            rule, status, mats = _device(ctx, 4, base)
            rule3, status3, mats3 = _device(ctx, 3, base)
        rule0, status0, _ = _device(ctx, 3, base)
    finally:
        ctx.close()
    # mode 4: every pair is a relative-entropy pair
    assert (mats == FILL).all() and (rule == 4).all() and (status == ce.ST_ITERATIONS).all() and len(base) > 20
    # mode 3: those the conditional test selects; the others are decided as without the hook
    assert (mats3 == FILL).all() and (rule3 == 4).sum() > 3
    for k in range(len(base)):
        if rule3[k] == ce.RULE_REL_ENTROPY and status3[k] != ce.ST_RULE:
            assert status3[k] == ce.ST_ITERATIONS
        else:
            assert (rule3[k], status3[k]) == (rule0[k], status0[k])
    assert (status0 == 0).sum() > (status3 == 0).sum()


# ---- through dmnd_extend ---------------------------------------------------------------------------------------------------------------

def _families(n_families, members, seed):
    """Queries and targets in families whose compositions lie far from the matrix background (so that the conditional test of modes
    2 / 3 / 5 takes both branches), beside ordinary ones."""
    rng = np.random.default_rng(seed)
    full = np.arange(20, dtype=np.int8)
    pools = [full, np.array([0, 10, 19, 9, 12, 13], np.int8), np.array([3, 6, 11, 1, 15, 5], np.int8), np.array([7, 14, 15, 16, 2], np.int8)]

    def mutate(s, rate, alphabet):
        m = s.copy()
        mut = rng.random(len(m)) < rate
        m[mut] = rng.choice(alphabet, int(mut.sum()))
        return m
    qs, ts = [], []
    for k in range(n_families):
        n = int(rng.integers(60, 300))
        pool = pools[k % 4]
        w = rng.dirichlet(np.ones(len(pool)) * (0.5 if k % 2 else 3.0))
        anc = np.where(rng.random(n) < (0.7 if k % 4 else 0.0), rng.choice(pool, n, p=w), rng.choice(full, n)).astype(np.int8)
        qs.append(mutate(anc, 0.15, full))
        for j in range(members):
            t = mutate(anc, float(rng.uniform(0.08, 0.4)), pool if rng.random() < 0.5 else full)
            if j % 3 == 2:          # a long flank of another composition: the pair's deviations from the background point apart
                other = pools[1 + (k + 1 + j // 3) % 3]
                t = np.concatenate([rng.choice(other, int(rng.integers(100, 400))).astype(np.int8), t])
            ts.append(t)

    def block(seqs):
        off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
        return workload.sequence_set(np.concatenate(seqs), off)
    return block(qs) + block(ts)


_blocks = {}


def _block(n_families, members, seed):
    """the block pair and its seed hits (computed once per shape)"""
    key = (n_families, members, seed)
    if key not in _blocks:
        qd, ql, td, tl = _families(n_families, members, seed)
        params = hip.default_params()
        params.db_letters = float(tl[-1] - tl[0] - (len(tl) - 1))
        ctx = hip.Context(params=params)
        try:
            ctx.upload_block(hip.QUERY, qd, ql)
            ctx.upload_block(hip.TARGET, td, tl)
            sp, gf = hip.seed_params_preset("default", params, threads=1)
            ctx.set_gapped_filter(gf)
            hits = ctx.seed_search(sp)
        finally:
            ctx.close()
        assert len(hits) > 500
        _blocks[key] = (qd, ql, td, tl, params, gf, hits)
    return _blocks[key]


def _extend(blk, mode, k, env):
    qd, ql, td, tl, params, gf, hits = blk
    ctx = hip.Context(params=params)
    try:
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, td, tl)
        ctx.set_gapped_filter(gf)
        ctx.set_comp_based_stats(mode)
        ctx.set_max_target_seqs(k)
        with Env(**env):
            m, tr = ctx.extend(qd, td, hits, threads=4, with_transcripts=True)
        return m, tr, ctx.cbs_device_stats()
    finally:
        ctx.close()


def _fields(a, b, dtype, path=""):
    for name in dtype.names:
        if dtype[name].names:
            yield from _fields(a[name], b[name], dtype[name], path + name + ".")
        else:
            yield path + name, a[name], b[name]


def _same(got, want, what, at_least=51):
    (m, tr, _), (m0, tr0, _) = got, want
    assert len(m) == len(m0) and len(m) >= at_least, (what, len(m), len(m0))
    for name, g, w in _fields(m, m0, m.dtype):
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: field %s of %d records differs from the host form's; first: record %d (query %d, target %d): %s, host form %s" % (
            what, name, len(bad), bad[0], m["query"][bad[0]], m["target"][bad[0]], g[bad[0]], w[bad[0]])
    end = int((m["hsp"]["transcript_off"] + m["hsp"]["transcript_len"] + 1).max())
    assert end > 0 and np.array_equal(tr[:end], tr0[:end]), what


def _stats_ok(st, mode, what):
    assert st["pairs"] > 100 and st["device"] > 0, (what, st)
    assert st["pairs"] == st["device"] + st["rounding"] + st["iterations"] + st["rule"] and st["kernel_ms"] > 0
    if mode == 5:          # `rule` holds every lambda-rescaling pair: not part of the share
        assert st["rule"] > 0 and st["rounding"] + st["iterations"] <= MAX_HANDED_BACK * (st["pairs"] - st["rule"]), (what, st)
    else:
        assert st["rounding"] + st["iterations"] + st["rule"] <= MAX_HANDED_BACK * st["pairs"], (what, st)


@pytest.mark.parametrize("mode", [3, 4, 5])
def test_extend_equals_the_host_form(mode):
    blk = _block(40, 10, 5)
    host = _extend(blk, mode, 25, dict(DMND_CBS_DEVICE=0))
    assert host[2]["pairs"] == 0
    dev = _extend(blk, mode, 25, {})
    _same(dev, host, "mode %d" % mode)
    _stats_ok(dev[2], mode, "mode %d" % mode)
    print("mode %d: %s" % (mode, dev[2]))
    # three passes: the store is reset between them
    n_hits = len(blk[6])
    passes = _extend(blk, mode, 25, dict(DMND_CBS_PASS_HITS=n_hits // 3 + 1))
    _same(passes, host, "mode %d, three passes" % mode)
    _stats_ok(passes[2], mode, "mode %d, three passes" % mode)
    assert passes[2]["pairs"] == dev[2]["pairs"]
    # every slot filled by the host threads
    back = _extend(blk, mode, 25, dict(DMND_CBS_DEVICE_MAX_ITS=1))
    _same(back, host, "mode %d, iteration cap 1" % mode)
    assert back[2]["iterations"] > 100 and back[2]["pairs"] == dev[2]["pairs"]


@pytest.mark.parametrize("mode", [3, 4, 5])
def test_extend_with_several_ranking_chunks_appends_to_the_store(mode):
    """-k 1 over 300 targets per query: the ranking loop takes several chunks of 128 targets, and every chunk after the first finds
    the earlier chunks' matrices in the store. Mode 5 hands every lambda-rescaling pair back, so the host's tables are copied into
    slots behind those; with an iteration cap of 1 so is every relative-entropy pair, in every mode."""
    blk = _block(4, 300, 6)
    what = "mode %d, -k 1" % mode
    host = _extend(blk, mode, 1, dict(DMND_CBS_DEVICE=0))
    dev = _extend(blk, mode, 1, {})
    _same(dev, host, what, at_least=3)
    print("%s: %s" % (what, dev[2]))
    _stats_ok(dev[2], mode, what)
    # a ranking chunk holds 128 targets: more pairs than four first chunks means that later chunks appended theirs to the store
    assert dev[2]["pairs"] > 4 * 128, dev[2]
    back = _extend(blk, mode, 1, dict(DMND_CBS_DEVICE_MAX_ITS=1))
    _same(back, host, what + ", iteration cap 1", at_least=3)
    assert back[2]["pairs"] == dev[2]["pairs"] and back[2]["iterations"] > 4 * 128 // 2 and back[2]["rule"] == dev[2]["rule"], back[2]


def test_cli_modes_equal_the_reference(tmp_path):
    from test_gpu_cli import CLI, REF, _run, _write_biased_files
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/diamond is not built here")
    _write_biased_files(tmp_path)
    base = ["-q", str(tmp_path / "q.faa"), "-d", str(tmp_path / "db.faa"), "-p", "4"]
    for extra in (["2"], ["3"], ["4"], ["5"], ["4", "-f", "0"]):
        args = ["--comp-based-stats"] + extra
        _run([REF, "blastp"] + base + args + ["-o", str(tmp_path / "ref.out")])
        _run([CLI, "blastp"] + base + args + ["-o", str(tmp_path / "hip.out")])
        ref, got = open(tmp_path / "ref.out").read(), open(tmp_path / "hip.out").read()
        assert len(ref) > 5000 and got == ref, extra
