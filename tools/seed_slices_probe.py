"""The sliced long-seed stream against the plain one in one process: stream kernel time of repeated --fast
searches with DMND_SEED_SLICES=0 and =1 on the same context, the hits compared.
  python tools/seed_slices_probe.py              C2's block pair (10 000 queries, 100 000 families of 10): the stage gate
  python tools/seed_slices_probe.py --sizes      C2's query block against reference blocks of 100 ... 30 000 families: the threshold
  python tools/seed_slices_probe.py --libs parent=PATH/libdiamond_hip.so,this=   the stage gate once per library, all loaded into this
                                                 process one after the other (empty path: this tree's): one object per label
Prints one JSON object."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diamond_amd import hip, synth, workload


def timed(ctx, sp, n, slices):
    os.environ["DMND_SEED_SLICES"] = str(slices)
    rows, hits = [], None
    for _ in range(n):
        t0 = time.perf_counter()
        hits = ctx.seed_search(sp)
        wall = (time.perf_counter() - t0) * 1e3
        ms = ctx.seed_kernel_ms()
        rows.append(dict(index=round(ms[0], 4), stream=round(ms[1], 4), call_wall=round(wall, 3)))
    del os.environ["DMND_SEED_SLICES"]
    return rows, hits


def main():
    if "--libs" in sys.argv:
        out, own = {}, hip.LIB_PATH
        for item in sys.argv[sys.argv.index("--libs") + 1].split(","):
            label, _, path = item.partition("=")
            hip._lib, hip.LIB_PATH = None, path or own
            out[label] = measure(False)
        print(json.dumps(out))
    else:
        print(json.dumps(measure("--sizes" in sys.argv)))


def measure(sizes):
    sp = hip.seed_params_fast(threads=8)
    out = {}
    if sizes:
        _, _, q, qoff = synth.generate(1000, members=10, queries=10_000, seed=20260923)
        qd, ql = workload.sequence_set(q, qoff)
        out["sizes"] = []
        for fam in (100, 300, 1000, 3000, 10000, 30000):
            db, doff, _, _ = synth.generate(fam, members=10, queries=10, seed=7)
            td, tl = workload.sequence_set(db, doff)
            ctx = hip.Context()
            ctx.upload_block(hip.QUERY, qd, ql)
            ctx.upload_block(hip.TARGET, td, tl)
            res = dict(letters=int(tl[-1] - tl[0]))
            for tag, v in (("plain", 0), ("slices", 1)):
                rows, _ = timed(ctx, sp, 8, v)
                res[tag + "_stream_ms_median"] = float(np.median([r["stream"] for r in rows[2:]]))
            ctx.close()
            out["sizes"].append(res)
    else:
        db, doff, q, qoff = synth.generate(100_000, members=10, queries=10_000, seed=20260923)
        qd, ql = workload.sequence_set(q, qoff)
        td, tl = workload.sequence_set(db, doff)
        ctx = hip.Context()
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, td, tl)
        out["letters"] = int(tl[-1] - tl[0])
        out["plain"], h0 = timed(ctx, sp, 6, 0)
        out["slices_first_search_builds"], h1 = timed(ctx, sp, 1, 1)
        out["slices"], h2 = timed(ctx, sp, 6, 1)
        out["plain_again"], h3 = timed(ctx, sp, 3, 0)
        out["hits"] = int(len(h0))
        out["hits_equal"] = bool(np.array_equal(h0, h1) and np.array_equal(h0, h2) and np.array_equal(h0, h3))
        ctx.close()
    return out


if __name__ == "__main__":
    main()
