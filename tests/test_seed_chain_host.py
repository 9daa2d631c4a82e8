"""CPU test of the host arithmetic of the seed search's chain mode (csrc/seed_chain.h: counter-block and readback layout,
decoding of the status word): tests/host/seed_chain_check.cpp as a stand-alone program under the address and
undefined-behaviour sanitizers."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_seed_chain_host_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "seed_chain_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-format-truncation", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "host", "seed_chain_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and "seed_chain_check ok" in out.stdout, out.stderr
