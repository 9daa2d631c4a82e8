"""-m gpu test of `diamond-hip blastp --masking seg` with SEG on the device (the default) against the same command line with the host
form (DMND_SEG_HOST=1) and against the reference binary: masked up front, lazily over two query blocks, and on the gathered block
of --global-ranking. Sizes as in test_gpu_cli.test_cli_seg_masking_matches_reference."""
import os
import subprocess

import numpy as np
import pytest

from diamond_amd import synth
import test_gpu_cli as base

pytestmark = pytest.mark.gpu


def _cli(args, env_extra):
    env = {k: v for k, v in os.environ.items() if k != "DMND_SEG_HOST"}
    env.update(env_extra, DMND_CLI_TIMELINE="1")
    r = subprocess.run([base.CLI] + args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def test_cli_seg_on_the_device_equals_the_host_form_and_the_reference(tmp_path):
    rng = np.random.default_rng(71)
    db, doff, q, qoff = synth.generate(300, members=10, queries=300, seed=71)
    db, q = base._plant_repeats(db, doff, rng, frac=0.5), base._plant_repeats(q, qoff, rng)
    synth.write_fasta(str(tmp_path / "db.faa"), "t", db, doff)
    synth.write_fasta(str(tmp_path / "q.faa"), "q", q, qoff)
    two_query_blocks = "-b%.9f" % (0.6 * float(qoff[-1]) / 1e9)
    seen = set()
    for extra, where, n_query_blocks in ((["--algo", "0"], "masked (seg, on the %s)", 1),
                                         (["--algo", "1", two_query_blocks], "masked lazily (seg, on the %s)", 2),
                                         (["--global-ranking", "8"], "ranked targets masked (seg, on the %s)", 1)):
        args = ["blastp", "-q", str(tmp_path / "q.faa"), "-d", str(tmp_path / "db.faa"), "-p", "4", "--masking", "seg"] + extra
        dev = _cli(args + ["-o", str(tmp_path / "dev.tsv")], {})
        host = _cli(args + ["-o", str(tmp_path / "host.tsv")], {"DMND_SEG_HOST": "1"})
        out = open(tmp_path / "dev.tsv").read()
        assert len(out.splitlines()) > 100, extra
        assert open(tmp_path / "host.tsv").read() == out, extra
        # the default run masks on the device, the other on the host; both print the summary line with the same count
        assert where % "device" in dev.stderr and where % "host" not in dev.stderr, extra
        assert where % "host" in host.stderr and where % "device" not in host.stderr, extra
        assert dev.stderr.count("query block uploaded and masked") == n_query_blocks, extra
        line = [l for l in dev.stderr.splitlines() if l.startswith("Masking reference (seg)")]
        assert len(line) == 1 and int(line[0].rsplit(":", 1)[1]) > 1000
        assert [l.rsplit(":", 1)[1] for l in host.stderr.splitlines() if l.startswith("Masking reference (seg)")] == [line[0].rsplit(":", 1)[1]]
        if os.path.exists(base.REF):
            base._run([base.REF] + args + ["-o", str(tmp_path / "ref.tsv")])
            assert open(tmp_path / "ref.tsv").read() == out, extra
        seen.add(out)
    # SEG changes this workload: the unmasked run gives other lines
    plain = _cli(["blastp", "-q", str(tmp_path / "q.faa"), "-d", str(tmp_path / "db.faa"), "-p", "4", "--masking", "0", "--algo", "0", "-o", str(tmp_path / "plain.tsv")], {})
    assert plain.returncode == 0 and open(tmp_path / "plain.tsv").read() not in seen
