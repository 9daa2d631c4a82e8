#!/usr/bin/env python3
"""Times the seed stage of a mutual-coverage search on the C2 workload (bench.py's: 10 000 queries x 1M sequences, --fast, blocks
resident) through hip.Context, both blocks length-sorted the way the reference sorts them (hip.length_sort_order): wall time of
dmnd_seed_search per step with the minimum length ratio set and with it off, the two interleaved step by step in ONE process,
`--steps` steps after `--warmup` warm-up steps, `--repeats` times; beside them the hit counts of both and the stage's own kernel
times. One JSON line.
  python tools/mutual_step.py [--ratio 0.75] [--sensitivity fast|default|sensitive] [--slices]
--slices: the length lists of the synthetic families are narrow (members within a few per cent of their base), so the ratio removes
little there; with --slices every sequence is cut to a random 45-100 % of itself first, as in tests/mutual_sets.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diamond_amd import hip, synth, workload      # noqa: E402


def sliced(data, off, rng):
    lens = np.diff(off)
    keep = np.maximum(1, np.round(lens * rng.uniform(0.45, 1.0, len(lens))).astype(np.int64))
    start = (rng.random(len(lens)) * (lens - keep + 1)).astype(np.int64)
    parts = [data[off[i] + start[i]: off[i] + start[i] + keep[i]] for i in range(len(lens))]
    return np.concatenate(parts), np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)


def length_sorted(data, off):
    order = hip.length_sort_order(np.concatenate([[0], np.cumsum(np.diff(off) + 1)]))
    lens = np.diff(off)[order]
    new_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.repeat(off[:-1][order] - new_off[:-1], lens) + np.arange(new_off[-1])
    return data[idx], new_off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratio", type=float, default=0.75)
    ap.add_argument("--families", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--sensitivity", choices=["fast", "default", "sensitive"], default="fast")
    ap.add_argument("--slices", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    db, doff, q, qoff = synth.generate(args.families, members=10, queries=args.queries, seed=20260923)
    if args.slices:
        rng = np.random.default_rng(7)
        db, doff = sliced(db, doff, rng)
        q, qoff = sliced(q, qoff, rng)
    q, qoff = length_sorted(q, qoff)
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
        modes = (("ratio", args.ratio), ("off", 0.0))
        hits, reps = {}, {name: [] for name, _ in modes}
        kernel_ms = {}
        for r in range(args.repeats):
            wall = {name: [] for name, _ in modes}
            for s in range(args.warmup + args.steps):
                for name, ratio in modes:
                    ctx.set_min_length_ratio(ratio)
                    t0 = time.perf_counter()
                    n = ctx.seed_search(sp, fetch=False)
                    dt = (time.perf_counter() - t0) * 1e3
                    if s >= args.warmup:
                        wall[name].append(dt)
                    hits[name] = int(n)
                    kernel_ms[name] = [round(x, 3) for x in ctx.seed_kernel_ms()]
            for name, _ in modes:
                reps[name].append(round(float(np.median(wall[name])), 3))
        out = dict(workload="C2, length-sorted" + (", sliced 45-100 %" if args.slices else ""), sensitivity=args.sensitivity, ratio=args.ratio,
                   queries=int(len(qoff) - 1), targets=int(len(doff) - 1), steps=args.steps, repeats=args.repeats,
                   seed_ms_ratio=reps["ratio"], seed_ms_off=reps["off"], hits_ratio=hits["ratio"], hits_off=hits["off"],
                   kernel_ms_ratio=kernel_ms["ratio"], kernel_ms_off=kernel_ms["off"])
        print(json.dumps(out))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
