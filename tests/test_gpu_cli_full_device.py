"""-m gpu: the CLI in --ext full and --global-ranking against the reference binary, with the device half of the extension stage doing
the work: the output is byte-identical to the reference's, and under DMND_TRACE=1 the device half's summary line reports queries
(without that the runs would pass through the host path, as they did before the device half took these modes)."""
import os
import re
import subprocess

import pytest

from diamond_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "diamond")
CLI = os.path.join(os.path.dirname(HERE), "diamond_amd", "diamond-hip")
SUMMARY = re.compile(r"dmnd_extend \(device half\): (\d+) queries, (\d+) handed back to the host")
BTOP = ["-f", "6", "qseqid", "sseqid", "length", "gapopen", "gaps", "btop"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    if not os.path.exists(REF):
        pytest.fail("oracle/_ref/diamond is missing: under -m gpu the reference binary is the checker, its absence is a failure")
    d = tmp_path_factory.mktemp("full")
    db, doff, q, qoff = synth.generate(150, members=12, queries=200, seed=31, decoy_frac=0.3, indel=0.05)
    dna, off = synth.back_translate(q[: qoff[60]], qoff[:61], seed=32)
    synth.write_fasta(str(d / "db.faa"), "t", db, doff)
    synth.write_fasta(str(d / "q.faa"), "q", q, qoff)
    synth.write_dna_fasta(str(d / "reads.fna"), "r", dna, off)
    return d


def _run(cmd, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-1500:]
    return r.stderr


def _equals_reference(d, tmp_path, mode, query, extra):
    args = [mode, "-q", str(d / query), "-d", str(d / "db.faa"), "-p", "4"] + extra
    _run([REF] + args + ["-o", str(tmp_path / "ref.out")])
    err = _run([CLI] + args + ["-o", str(tmp_path / "hip.out")], env=dict(os.environ, DMND_TRACE="1"))
    ref = open(tmp_path / "ref.out", "rb").read()
    assert len(ref.splitlines()) > 50, extra
    assert open(tmp_path / "hip.out", "rb").read() == ref, (mode, extra)
    laps = [(int(a), int(b)) for a, b in SUMMARY.findall(err)]
    assert laps and sum(a for a, _ in laps) > 0, "the device half extended no query of this run"
    return laps


@pytest.mark.parametrize("mode,query,extra", [
    ("blastp", "q.faa", ["--ext", "full"]),
    ("blastp", "q.faa", ["--ext", "full", "--sensitive"] + BTOP),
    ("blastp", "q.faa", ["--ext", "full", "--top", "10"]),
    ("blastp", "q.faa", ["--ext", "full", "--id", "30", "--query-cover", "40"]),
    ("blastx", "reads.fna", ["--ext", "full"]),
], ids=["full", "full_sensitive_btop", "full_top10", "full_filters", "blastx_full"])
def test_ext_full_runs_in_the_device_half_and_equals_the_reference(files, tmp_path, mode, query, extra):
    _equals_reference(files, tmp_path, mode, query, extra)


@pytest.mark.parametrize("mode,query,extra", [
    ("blastp", "q.faa", ["-g", "2"]),
    ("blastp", "q.faa", ["-g", "100", "-b0.00003"]),
    ("blastp", "q.faa", ["-g", "6", "--top", "20", "-b0.00003"]),
    ("blastp", "q.faa", ["-g", "5"] + BTOP),
    ("blastx", "reads.fna", ["-g", "5"]),
], ids=["g2", "g100_blocks", "g6_top20_blocks", "g5_btop", "blastx_g5"])
def test_global_ranking_final_pass_runs_in_the_device_half_and_equals_the_reference(files, tmp_path, mode, query, extra):
    _equals_reference(files, tmp_path, mode, query, extra)
