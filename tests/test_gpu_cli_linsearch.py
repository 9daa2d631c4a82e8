"""-m gpu tests of the linearised search on the command line: `diamond-hip blastp --linsearch` against the unmodified reference binary
on the same files, byte for byte. The files are those of tests/test_gpu_cli_mutual_cover.py (the same generator call): NOT
length-sorted, with equal lengths among the targets (the reference sorts every reference block by (length, index) descending, the
query blocks stay as they are), families whose members share seeds at several reference positions -- the reference's own
--linsearch output has 10 % to 50 % fewer lines than its plain output, asserted below."""
import os
import re

import numpy as np
import pytest

import mutual_sets
from test_gpu_cli_mutual_cover import BASE, CLI, FIELDS, REF, _run, write_fasta

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    if not os.path.exists(REF):
        pytest.fail("oracle/_ref/diamond is missing: under -m gpu the reference binary is the checker, its absence is a failure")
    assert os.path.exists(CLI), "diamond-hip not built (make product)"
    d = tmp_path_factory.mktemp("linsearch")
    db, doff, q, qoff = mutual_sets.generate(families=40, members=6, queries=2, near=2, near_members=8, near_queries=3, seed=51)
    write_fasta(str(d / "db.faa"), ["t%d" % i for i in range(len(doff) - 1)], db, doff)
    write_fasta(str(d / "q.faa"), ["q%d some title" % i for i in range(len(qoff) - 1)], q, qoff)
    # the same queries with five unrelated ones among them (every query of q.faa aligns: --un would stay empty)
    rng = np.random.default_rng(8)
    parts, names = [], []
    for i in range(len(qoff) - 1):
        if i % 20 == 7:
            parts.append(rng.integers(0, 20, 150 + i).astype(np.int8)); names.append("stranger%d" % i)
        parts.append(q[qoff[i]:qoff[i + 1]]); names.append("q%d some title" % i)
    write_fasta(str(d / "q_un.faa"), names, np.concatenate(parts), np.concatenate([[0], np.cumsum([len(x) for x in parts])]))
    tlen = np.diff(doff)
    assert len(set(tlen.tolist())) < len(tlen) and (np.diff(tlen) > 0).any()                       # equal lengths, not sorted
    return d


def both(files, tag, args, q="q.faa", db="db.faa", base=BASE):
    """The reference and diamond-hip with the same arguments; returns (reference output, ours, our stderr)."""
    common = ["blastp", "-q", str(files / q), "-d", str(files / db)] + list(base) + list(args)
    _run([REF] + common + ["-o", str(files / ("ref_%s.out" % tag))])
    r = _run([CLI] + common + ["-o", str(files / ("hip_%s.out" % tag))])
    return open(files / ("ref_%s.out" % tag), "rb").read(), open(files / ("hip_%s.out" % tag), "rb").read(), r.stderr


CASES = {
    "fast": ["--linsearch", "--fast", "-k", "0"],
    "default": ["--linsearch", "-k", "0"],
    "k3": ["--linsearch", "-k", "3"],
    "top10": ["--linsearch", "--top", "10"],
    "max_hsps0": ["--linsearch", "--max-hsps", "0"],
    "fields": ["--linsearch", "-k", "0", "-f", "6"] + FIELDS,
    "pairwise": ["--linsearch", "-f", "0"],
    "xml": ["--linsearch", "-f", "5"],
    "banded_fast": ["--linsearch", "--ext", "banded-fast", "-k", "0"],
}


@pytest.mark.parametrize("tag", sorted(CASES))
def test_output_equals_reference(files, tag):
    ref, hip, _ = both(files, tag, CASES[tag])
    assert len(ref.splitlines()) > 50
    if tag == "xml":                                           # the header names the programs and their versions
        cut = lambda b: b[b.index(b"<BlastOutput_iterations>"):]
        ref, hip = cut(ref), cut(hip)
    assert hip == ref


@pytest.mark.parametrize("mode", [["--fast"], []], ids=["fast", "default"])
def test_the_rule_removes_a_tenth_to_a_half_of_the_reference_s_lines(files, mode):
    tag = "share_" + (mode[0][2:] if mode else "default")
    lin, hip, _ = both(files, tag, mode + ["--linsearch", "-k", "0"])
    plain, hip_plain, _ = both(files, tag + "_plain", mode + ["-k", "0"])
    fewer = 1.0 - len(lin.splitlines()) / len(plain.splitlines())
    print("%s: plain %d lines, --linsearch %d, %.1f %% fewer" % (tag, len(plain.splitlines()), len(lin.splitlines()), 100 * fewer))
    assert 0.10 <= fewer <= 0.50
    assert hip == lin and hip_plain == plain


def test_query_indexed_algorithm_equals_reference(files):
    base = ["--masking", "0", "--motif-masking", "0", "--algo", "1", "-p", "4"]
    ref, hip, _ = both(files, "algo1", ["--linsearch", "-k", "0"], base=base)
    assert len(ref.splitlines()) > 50 and hip == ref


def test_default_masking_equals_reference(files):
    ref, hip, _ = both(files, "masked", ["--linsearch", "-k", "0"], base=["--algo", "0", "-p", "4"])
    assert len(ref.splitlines()) > 50 and hip == ref


def test_self_hits_are_dropped_as_in_the_reference(files):
    """All against all: the database file as the query file, --no-self-hits (titles and letters agree) over sorted reference blocks."""
    ref, hip, _ = both(files, "self", ["--linsearch", "--no-self-hits"], q="db.faa")
    plain, _, _ = both(files, "self_kept", ["--linsearch"], q="db.faa")
    assert len(ref.splitlines()) > 50 and len(plain.splitlines()) > len(ref.splitlines())
    assert hip == ref


def test_several_reference_blocks_with_un_and_al(files):
    """-b small enough for at least three reference blocks: per-block sorting and first positions, database ordinals through the
    join, --un / --al in the file's query order."""
    common = ["blastp", "-q", str(files / "q_un.faa"), "-d", str(files / "db.faa")] + BASE + ["--linsearch", "-b", "0.000012"]
    _run([REF] + common + ["-o", str(files / "ref_b.out"), "--un", str(files / "ref_un.faa"), "--al", str(files / "ref_al.faa")])
    r = _run([CLI] + common + ["-o", str(files / "hip_b.out"), "--un", str(files / "hip_un.faa"), "--al", str(files / "hip_al.faa")])
    m = re.search(r"query blocks=(\d+) reference blocks=(\d+)", r.stderr)
    assert m and int(m.group(2)) >= 3, r.stderr[-500:]
    ref = open(files / "ref_b.out", "rb").read()
    assert len(ref.splitlines()) > 50
    assert open(files / "hip_b.out", "rb").read() == ref
    for name in ("un", "al"):
        want = open(files / ("ref_%s.faa" % name), "rb").read()
        assert want.count(b">") > 3
        assert open(files / ("hip_%s.faa" % name), "rb").read() == want, name
    # first positions are per reference block: another answer than one block's
    one, _, _ = both(files, "b_one", ["--linsearch"], q="q_un.faa")
    assert one != ref


def test_short_shapes_are_refused_with_the_reference_s_sentence(files):
    args = ["blastp", "-q", str(files / "q.faa"), "-d", str(files / "db.faa"), "--sensitive", "--linsearch", "-o", str(files / "s.out")]
    ref, hip = _run([REF] + args, ok=False), _run([CLI] + args, ok=False)
    msg = "Linearization is only supported for seed shapes of weight >= 10."
    assert ref.returncode != 0 and msg in ref.stderr
    assert hip.returncode != 0 and msg in hip.stderr


def test_refused_combinations_name_their_option(files):
    common = ["-q", str(files / "q.faa"), "-d", str(files / "db.faa"), "--linsearch", "-o", str(files / "n.out")]
    for extra, word in ((["--min-len-ratio", "0.75"], "--min-len-ratio"), (["--query-cover", "80", "--subject-cover", "80"], "--query-cover"),
                        (["--global-ranking", "5"], "--global-ranking"), (["--gpus", "2"], "--gpus")):
        r = _run([CLI, "blastp"] + common + extra, ok=False)
        assert r.returncode != 0 and word in r.stderr and "--linsearch" in r.stderr and "not part of this build" in r.stderr, extra
    with open(files / "reads.fna", "w") as f:
        f.write(">r0\nATGGCTGCTAAAGGTGAACTGCGTCATATTCTGAAAGAAGTTGGTAACCCGTGGTTC\n")
    r = _run([CLI, "blastx", "-q", str(files / "reads.fna"), "-d", str(files / "db.faa"), "--linsearch", "-o", str(files / "x.out")], ok=False)
    assert r.returncode != 0 and "--linsearch" in r.stderr and "blastp" in r.stderr
