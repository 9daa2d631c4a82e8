"""The sliced long-seed stream under level-1 filters of several sizes: C2's block pair, per size a fresh context,
one forced sliced search that builds the reference cache and --searches more that keep it, the filter's word count set with
DMND_SEED_SLICES_FILTER_WORDS (0: the library's own rule). Stream kernel time per search, the geometry of the DMND_TRACE line,
the hits compared with the plain stream's.
  python tools/seed_filter_sweep.py --words 786432,1048576,2097152
  python tools/seed_filter_sweep.py --words 0 --lib PATH/libdiamond_hip.so      another build of the library
Under `rocprofv3 --pmc ...` (counters in a run of their own, one size per run) the stream kernel's launches are these searches'.
Prints one JSON object."""
import argparse
import json
import os
import re
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diamond_amd import hip, synth, workload


def traced_search(ctx, sp):
    """one search with DMND_TRACE; returns (hits, the trace's stream line). The library writes to the C stderr: redirected to a file"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        os.environ["DMND_TRACE"] = "1"
        try:
            hits = ctx.seed_search(sp)
        finally:
            del os.environ["DMND_TRACE"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        m = re.search(r"stream: ([^,]*),", tmp.read().decode(errors="replace"))
    return hits, m.group(1) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", default="0", help="comma-separated word counts of the level-1 filter (0: the library's rule)")
    ap.add_argument("--searches", type=int, default=6)
    ap.add_argument("--lib", default=None, help="another libdiamond_hip.so than this tree's")
    args = ap.parse_args()
    if args.lib:
        hip._lib, hip.LIB_PATH = None, args.lib
    sp = hip.seed_params_fast(threads=8)
    db, doff, q, qoff = synth.generate(100_000, members=10, queries=10_000, seed=20260923)
    qd, ql = workload.sequence_set(q, qoff)
    td, tl = workload.sequence_set(db, doff)
    out = dict(query_positions=int(ql[-1] - ql[0]), reference_letters=int(tl[-1] - tl[0]), sizes=[])
    plain = None
    for words in [int(w) for w in args.words.split(",")]:
        ctx = hip.Context()
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, td, tl)
        if plain is None:
            os.environ["DMND_SEED_SLICES"] = "0"
            plain = ctx.seed_search(sp)
        os.environ["DMND_SEED_SLICES"] = "1"
        if words:
            os.environ["DMND_SEED_SLICES_FILTER_WORDS"] = str(words)
        hits, stream = traced_search(ctx, sp)             # builds the cache
        equal = bool(np.array_equal(hits, plain))
        ms = []
        for _ in range(args.searches):
            hits = ctx.seed_search(sp)
            k = ctx.seed_kernel_ms()
            ms.append(dict(index=round(k[0], 4), stream=round(k[1], 4)))
            equal = equal and bool(np.array_equal(hits, plain))
        os.environ.pop("DMND_SEED_SLICES_FILTER_WORDS", None)
        del os.environ["DMND_SEED_SLICES"]
        ctx.close()
        s = [r["stream"] for r in ms]
        out["sizes"].append(dict(filter_words=words, stream=stream, searches=ms, stream_ms_median=float(np.median(s)), stream_ms_min=min(s), stream_ms_max=max(s),
                                 hits=int(len(hits)), hits_equal_plain=equal))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
