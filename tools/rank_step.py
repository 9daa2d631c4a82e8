#!/usr/bin/env python3
"""Times the ranking step of a --global-ranking search on one C2 block pair (bench.py's: 10 000 queries x 1M sequences, --fast, blocks
resident) through hip.Context, in its two forms:
  host    dmnd_seed_hits + dmnd_rank_targets on `--threads` host threads. The hit list has to reach the host: where the seed search ran
          as one device chain it came with the search's own readback and dmnd_seed_hits copies host memory, otherwise dmnd_seed_hits
          downloads it
  device  dmnd_rank_targets_device on the hits where the seed stage left them, n_keep = `--keep`, after a search made under
          dmnd_set_seed_hits_resident (the chain's readback then carries no hits)
Wall time per step, `--steps` steps after `--warmup` warm-up steps, `--repeats` times, and the md5 of the records (device: of the kept
records; the host's records cut the same way give the same md5). `bus_bytes_per_block_pair` is COMPUTED, not observed: what a block
pair's hits and records put on the bus towards the host in that form -- host: 24 bytes per seed hit (inside the seed search or inside
dmnd_seed_hits); device: 24 bytes of counters + 12 bytes per record. One JSON line.
  python tools/rank_step.py [--lib PATH] [--form host|device|both]
                          --lib: another build's libdiamond_hip.so (an earlier commit's, for DESIGN.md 5.0-rank); a build without the
                          device entry times the host form only
The seed stage runs outside the timed region: every step ranks the same seed hits."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diamond_amd import hip, synth, workload      # noqa: E402


def cut(recs, n_keep):
    order = np.lexsort((recs["target"], 65535 - recs["score"].astype(np.int64), recs["query"]))
    s = recs[order]
    first = np.searchsorted(s["query"], s["query"], "left")
    return s[np.arange(len(s)) - first < n_keep]


def timed(step, warmup, steps, repeats):
    reps, last = [], None
    for _ in range(repeats):
        wall = []
        for s in range(warmup + steps):
            t0 = time.perf_counter()
            last = step()
            t1 = time.perf_counter()
            if s >= warmup:
                wall.append((t1 - t0) * 1e3)
        reps.append(float(np.median(wall)))
    return dict(wall_ms_median_of_repeats=float(np.median(reps)), wall_ms_spread=float(max(reps) - min(reps)), repeats=reps), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--keep", type=int, default=25)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--form", choices=["host", "device", "both"], default="both")
    args = ap.parse_args()
    if args.lib:
        hip.LIB_PATH = os.path.abspath(args.lib)
    db, doff, q, qoff = synth.generate(args.families, members=10, queries=args.queries, seed=20260923)
    qd, ql = workload.sequence_set(q, qoff)
    td, tl = workload.sequence_set(db, doff)
    params = hip.default_params()
    params.db_letters = float(doff[-1])
    ctx = hip.Context(device=0, params=params)
    try:
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, td, tl)
        sp, _ = hip.seed_params_preset("fast", params, threads=1)
        hits = ctx.seed_search(sp)
        out = dict(lib=args.lib or "this build", seed_hits=int(len(hits)), threads=args.threads, keep=args.keep)
        if args.form != "device":
            host, recs = timed(lambda: ctx.rank_targets(qd, td, ctx.seed_hits(len(hits)), threads=args.threads), args.warmup, args.steps, args.repeats)
            kept = cut(recs, args.keep)
            host.update(records=int(len(recs)), bus_bytes_per_block_pair=int(len(hits)) * hip.SEED_HIT_DTYPE.itemsize, kept_md5=hashlib.md5(kept.tobytes()).hexdigest())
            out["host"] = host
        if args.form != "host" and hasattr(ctx.lib, "dmnd_rank_targets_device"):
            ctx.set_seed_hits_resident(True)
            assert ctx.seed_search(sp, fetch=False) == len(hits)
            dev, got = timed(lambda: ctx.rank_targets_device(None, n_keep=args.keep), args.warmup, args.steps, args.repeats)
            st = ctx.rank_device_stats()
            dev.update(records=int(len(got)), bus_bytes_per_block_pair=24 + int(len(got)) * hip.RANKED_DTYPE.itemsize, kept_md5=hashlib.md5(got.tobytes()).hexdigest(),
                       groups=int(st[0]), hits_walked=int(st[1]))
            out["device"] = dev
        print(json.dumps(out))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
