"""CPU: bench.py --dump-outputs -- the match records of the last timed step written as one float64 array per field, exactly, and a
fixed sample of them when the arrays would exceed the size cap. No device: the records are made up here."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from diamond_amd import hip


def _records(n, seed=0):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=hip.MATCH_DTYPE)
    r["query"] = np.sort(rng.integers(0, 1 << 31, n)).astype(np.uint32)
    r["target"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    r["d_begin"] = rng.integers(-1 << 31, 1 << 31, n)
    r["evalue"] = rng.random(n) * 1e-5
    r["bit_score"] = rng.random(n) * 500
    r["hsp"]["score"] = rng.integers(0, 1 << 20, n)
    r["hsp"]["transcript_off"] = rng.integers(0, 1 << 40, n)
    return r


def test_dump_writes_every_field_exactly(tmp_path):
    r = _records(1000)
    names = bench.dump_outputs(r, str(tmp_path))
    assert "records_count" in names and "records_sample_index" not in names
    assert "records_hsp_transcript_off" not in names                 # a position in the trace buffer, not a result
    assert np.load(tmp_path / "records_count.npy").tolist() == [1000]
    for f in r.dtype.names:
        if f == "hsp":
            continue
        a = np.load(tmp_path / ("records_%s.npy" % f))
        assert a.dtype == np.float64 and np.array_equal(a, r[f].astype(np.float64)), f
    for f in r.dtype["hsp"].names:
        if f != "transcript_off":
            a = np.load(tmp_path / ("records_hsp_%s.npy" % f))
            assert a.dtype == np.float64 and np.array_equal(a, r["hsp"][f].astype(np.float64)), f
    assert sorted(p[:-4] for p in os.listdir(tmp_path)) == names


def test_dump_samples_within_the_cap_and_repeats(tmp_path):
    r = _records(5000, seed=1)
    cap = 200_000
    names = bench.dump_outputs(r, str(tmp_path / "a"), cap=cap)
    bench.dump_outputs(r, str(tmp_path / "b"), cap=cap)
    assert "records_sample_index" in names
    total = sum(np.load(tmp_path / "a" / (n + ".npy")).nbytes for n in names)
    assert total <= cap
    idx = np.load(tmp_path / "a" / "records_sample_index.npy").astype(np.int64)
    assert len(idx) > 100 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "records_target.npy"), r["target"][idx].astype(np.float64))
    for n in names:                                                 # the sample is fixed: the same records give the same files
        assert np.array_equal(np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))), n


def test_default_cap_is_below_64_mb():
    assert bench.DUMP_CAP_BYTES <= 64 * 10 ** 6
