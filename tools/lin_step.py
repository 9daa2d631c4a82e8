#!/usr/bin/env python3
"""Times the seed stage of a linearised search (--linsearch, Context.set_linsearch) on the C2 workload (bench.py's: 10 000 queries x
1M sequences, --fast, blocks resident) through hip.Context, the reference block length-sorted the way the reference sorts it
(hip.length_sort_order), the query block as generated: wall time of dmnd_seed_search per step with the switch on and with it off,
the two interleaved step by step in ONE process, `--steps` steps after `--warmup` warm-up steps, `--repeats` times; beside them the
hit counts of both and the stage's own kernel times per phase (index, stream, mask, pairs, all -- the reduction to first positions
runs inside `pairs`, in front of the pair filter). One JSON line.
  python tools/lin_step.py [--sensitivity fast|default] [--members N]
--members: sequences per synthetic family (C2: 10); a seed joins about that many reference positions, of which the rule keeps one."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diamond_amd import hip, synth, workload      # noqa: E402
from mutual_step import length_sorted             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=100_000)
    ap.add_argument("--members", type=int, default=10)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--sensitivity", choices=["fast", "default"], default="fast")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    db, doff, q, qoff = synth.generate(args.families, members=args.members, queries=args.queries, seed=20260923)
    db, doff = length_sorted(db, doff)
    qd, ql = workload.sequence_set(q, qoff)
    td, tl = workload.sequence_set(db, doff)
    params = hip.default_params()
    params.db_letters = float(doff[-1])
    ctx = hip.Context(device=0, params=params)
    try:
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, td, tl)
        sp, gf = hip.seed_params_preset(args.sensitivity, params, threads=1)
        ctx.set_gapped_filter(gf)
        modes = (("lin", True), ("off", False))
        hits, reps = {}, {name: [] for name, _ in modes}
        kernel_ms = {}
        for r in range(args.repeats):
            wall = {name: [] for name, _ in modes}
            for s in range(args.warmup + args.steps):
                for name, on in modes:
                    ctx.set_linsearch(on)
                    t0 = time.perf_counter()
                    n = ctx.seed_search(sp, fetch=False)
                    dt = (time.perf_counter() - t0) * 1e3
                    if s >= args.warmup:
                        wall[name].append(dt)
                    hits[name] = int(n)
                    kernel_ms[name] = [round(x, 3) for x in ctx.seed_kernel_ms()]
            for name, _ in modes:
                reps[name].append(round(float(np.median(wall[name])), 3))
        out = dict(workload="C2, reference block length-sorted", sensitivity=args.sensitivity, queries=int(len(qoff) - 1), targets=int(len(doff) - 1),
                   members=args.members, steps=args.steps, repeats=args.repeats, seed_ms_lin=reps["lin"], seed_ms_off=reps["off"],
                   hits_lin=hits["lin"], hits_off=hits["off"], kernel_ms_lin=kernel_ms["lin"], kernel_ms_off=kernel_ms["off"])
        print(json.dumps(out))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
