"""-m gpu tests of the mutual-coverage search on the command line: `diamond-hip blastp` with --min-len-ratio, or with equal
--query-cover / --subject-cover of 50 and more (which stand for a ratio of their own: run/config.cpp:156-165), against the
unmodified reference binary on the same files, byte for byte. The files are NOT length-sorted and hold equal lengths on both
sides (the reference sorts every block by (length, index) descending and prints in that order) and lengths in the exact ratio
3 : 4; their families hold slices of 45-100 % of a base (tests/mutual_sets.py), so that the length test removes a good third of
what the plain search reports -- asserted below to lie between 20 % and 80 %."""
import os
import subprocess

import numpy as np
import pytest

import mutual_sets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "diamond")
CLI = os.path.join(ROOT, "diamond_amd", "diamond-hip")
ALPHABET = "ARNDCQEGHILKMFPSTWYV"
FIELDS = ["qseqid", "sseqid", "pident", "length", "mismatch", "gapopen", "qstart", "qend", "sstart", "send", "evalue", "bitscore", "qlen", "slen"]
BASE = ["--masking", "0", "--motif-masking", "0", "--algo", "0", "-p", "4"]


def _run(cmd, ok=True):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stderr[-2000:]
    return r


def write_fasta(path, names, data, off):
    with open(path, "w") as f:
        for i, name in enumerate(names):
            f.write(">%s\n%s\n" % (name, "".join(ALPHABET[x] for x in data[off[i]:off[i + 1]])))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    if not os.path.exists(REF):
        pytest.fail("oracle/_ref/diamond is missing: under -m gpu the reference binary is the checker, its absence is a failure")
    assert os.path.exists(CLI), "diamond-hip not built (make product)"
    d = tmp_path_factory.mktemp("mutual")
    db, doff, q, qoff = mutual_sets.generate(families=40, members=6, queries=2, near=2, near_members=8, near_queries=3, seed=51)
    tn, qn = ["t%d" % i for i in range(len(doff) - 1)], ["q%d some title" % i for i in range(len(qoff) - 1)]
    write_fasta(str(d / "db.faa"), tn, db, doff)
    write_fasta(str(d / "q.faa"), qn, q, qoff)
    tlen, qlen = np.diff(doff), np.diff(qoff)
    assert len(set(tlen.tolist())) < len(tlen) and len(set(qlen.tolist())) < len(qlen)             # equal lengths on both sides
    assert (np.diff(tlen) > 0).any() and (np.diff(qlen) > 0).any()                                  # not sorted
    assert 90 in qlen and 120 in tlen and 120 in qlen and 90 in tlen                                # the exact ratio 3 : 4
    # the same sequences pre-sorted as the reference sorts a block, titles carried along
    sdb, sdoff, to = mutual_sets.length_sorted(db, doff)
    sq, sqoff, qo = mutual_sets.length_sorted(q, qoff)
    write_fasta(str(d / "db_sorted.faa"), [tn[i] for i in to], sdb, sdoff)
    write_fasta(str(d / "q_sorted.faa"), [qn[i] for i in qo], sq, sqoff)
    return d


def both(files, tag, args, q="q.faa", db="db.faa", extra_cli=()):
    """The reference and diamond-hip with the same arguments; returns (reference output, ours, our stderr)."""
    common = ["blastp", "-q", str(files / q), "-d", str(files / db)] + BASE + list(args)
    _run([REF] + common + ["-o", str(files / ("ref_%s.out" % tag))])
    r = _run([CLI] + common + list(extra_cli) + ["-o", str(files / ("hip_%s.out" % tag))])
    return open(files / ("ref_%s.out" % tag), "rb").read(), open(files / ("hip_%s.out" % tag), "rb").read(), r.stderr


CASES = {
    "cover80_fast": ["--fast", "--query-cover", "80", "--subject-cover", "80"],
    "cover80_default": ["--query-cover", "80", "--subject-cover", "80"],
    "cover80_sensitive": ["--sensitive", "--query-cover", "80", "--subject-cover", "80"],
    "cover60": ["--query-cover", "60", "--subject-cover", "60"],
    "cover95": ["--query-cover", "95", "--subject-cover", "95"],
    "ratio_k0": ["--min-len-ratio", "0.75", "-k", "0"],
    "ratio_k3": ["--min-len-ratio", "0.75", "-k", "3"],
    "ratio_fields": ["--min-len-ratio", "0.75", "-k", "0", "-f", "6"] + FIELDS,
    "cover80_given_ratio": ["--min-len-ratio", "0.5", "--query-cover", "80", "--subject-cover", "80"],
    "pairwise": ["--min-len-ratio", "0.75", "-f", "0"],
    "xml": ["--min-len-ratio", "0.75", "-f", "5"],
    "cbs3": ["--min-len-ratio", "0.75", "--comp-based-stats", "3"],
}


@pytest.mark.parametrize("tag", sorted(CASES))
def test_output_equals_reference(files, tag):
    ref, hip, _ = both(files, tag, CASES[tag])
    assert len(ref.splitlines()) > 10                          # (covers of 95 leave a few dozen lines of the several hundred)
    if tag == "xml":                                           # the header names the programs and their versions
        cut = lambda b: b[b.index(b"<BlastOutput_iterations>"):]
        ref, hip = cut(ref), cut(hip)
    assert hip == ref


def test_query_indexed_algorithm_equals_reference(files):
    common = ["blastp", "-q", str(files / "q.faa"), "-d", str(files / "db.faa"), "--masking", "0", "--motif-masking", "0", "--algo", "1", "-p", "4", "--min-len-ratio", "0.75", "-k", "0"]
    _run([REF] + common + ["-o", str(files / "ref_algo1.out")])
    _run([CLI] + common + ["-o", str(files / "hip_algo1.out")])
    ref = open(files / "ref_algo1.out", "rb").read()
    assert len(ref.splitlines()) > 50 and open(files / "hip_algo1.out", "rb").read() == ref


def test_self_hits_are_dropped_as_in_the_reference(files):
    """All against all: the database file as the query file, --no-self-hits (titles and letters agree)."""
    ref, hip, _ = both(files, "self", ["--min-len-ratio", "0.75", "--no-self-hits"], q="db.faa")
    plain, _, _ = both(files, "self_kept", ["--min-len-ratio", "0.75"], q="db.faa")
    assert len(ref.splitlines()) > 50 and len(plain.splitlines()) > len(ref.splitlines())
    assert hip == ref


def test_several_blocks_with_un_and_al(files):
    """-b small enough for at least three reference blocks and two query blocks: per-block sorting, database ordinals through the
    join, --un / --al in the sorted order of every query block."""
    args = ["--min-len-ratio", "0.75", "-b", "0.000012"]
    common = ["blastp", "-q", str(files / "q.faa"), "-d", str(files / "db.faa")] + BASE + args
    _run([REF] + common + ["-o", str(files / "ref_b.out"), "--un", str(files / "ref_un.faa"), "--al", str(files / "ref_al.faa")])
    r = _run([CLI] + common + ["-o", str(files / "hip_b.out"), "--un", str(files / "hip_un.faa"), "--al", str(files / "hip_al.faa")])
    import re
    m = re.search(r"query blocks=(\d+) reference blocks=(\d+)", r.stderr)
    assert m and int(m.group(1)) >= 2 and int(m.group(2)) >= 3, r.stderr[-500:]
    ref = open(files / "ref_b.out", "rb").read()
    assert len(ref.splitlines()) > 50
    assert open(files / "hip_b.out", "rb").read() == ref
    for name in ("un", "al"):
        want = open(files / ("ref_%s.faa" % name), "rb").read()
        assert want.count(b">") > 3
        assert open(files / ("hip_%s.faa" % name), "rb").read() == want, name
    # the same search with the query index kept over the reference blocks of ONE query block
    ref1, hip1, _ = both(files, "b_t", ["--min-len-ratio", "0.75", "-b", "0.00005"])
    assert hip1 == ref1


def test_ratio_run_equals_filtered_plain_run_on_sorted_files(files):
    """diamond-hip --min-len-ratio 0.75 -k 0 on the files as they are equals diamond-hip without it on the pre-sorted files with every
    line removed whose lengths fail the two inequalities; the length test removes between 20 % and 80 % of the lines."""
    fields = ["-f", "6"] + FIELDS
    common = ["blastp"] + BASE + ["-k", "0"] + fields
    _run([CLI] + common + ["-q", str(files / "q.faa"), "-d", str(files / "db.faa"), "--min-len-ratio", "0.75", "-o", str(files / "hip_ratio.tsv")])
    _run([CLI] + common + ["-q", str(files / "q_sorted.faa"), "-d", str(files / "db_sorted.faa"), "-o", str(files / "hip_plain.tsv")])
    plain = open(files / "hip_plain.tsv").read().splitlines()
    kept = [l for l in plain if mutual_sets.passes(int(l.split("\t")[12]), int(l.split("\t")[13]), 0.75)]
    removed = 1.0 - len(kept) / len(plain)
    print("plain %d lines, kept %d, removed %.1f %%" % (len(plain), len(kept), 100 * removed))
    assert 0.2 <= removed <= 0.8
    assert open(files / "hip_ratio.tsv").read().splitlines() == kept
    # ... and so does the reference's own plain run
    _run([REF] + common + ["-q", str(files / "q_sorted.faa"), "-d", str(files / "db_sorted.faa"), "-o", str(files / "ref_plain.tsv")])
    ref_plain = open(files / "ref_plain.tsv").read().splitlines()
    assert [l for l in ref_plain if mutual_sets.passes(int(l.split("\t")[12]), int(l.split("\t")[13]), 0.75)] == kept


def test_translated_search_refuses_the_ratio_with_the_reference_message(files):
    with open(files / "reads.fna", "w") as f:
        f.write(">r0\nATGGCTGCTAAAGGTGAACTGCGTCATATTCTGAAAGAAGTTGGTAACCCGTGGTTC\n")
    args = ["blastx", "-q", str(files / "reads.fna"), "-d", str(files / "db.faa"), "--min-len-ratio", "0.75", "-o", str(files / "x.out")]
    ref, hip = _run([REF] + args, ok=False), _run([CLI] + args, ok=False)
    msg = "--min-len-ratio is not supported for translated searches"
    assert ref.returncode != 0 and msg in ref.stderr
    assert hip.returncode != 0 and msg in hip.stderr
    # equal covers switch nothing for translated searches
    args = ["blastx", "-q", str(files / "reads.fna"), "-d", str(files / "db.faa"), "--query-cover", "80", "--subject-cover", "80", "--masking", "0", "-o", str(files / "x.out")]
    assert _run([CLI] + args, ok=False).returncode == 0


def test_unsupported_combinations_say_so(files):
    for extra, word in ((["--global-ranking", "5"], "--global-ranking"), (["--gpus", "2"], "--gpus")):
        r = _run([CLI, "blastp", "-q", str(files / "q.faa"), "-d", str(files / "db.faa"), "--min-len-ratio", "0.75", "-o", str(files / "n.out")] + extra, ok=False)
        assert r.returncode != 0 and word in r.stderr and "not part of this build" in r.stderr
