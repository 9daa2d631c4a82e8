#!/usr/bin/env python3
"""Times the extension stage of a --top search on the C2 workload (bench.py's: 10 000 queries x 1M sequences, --fast, blocks
resident) through hip.Context: wall time of dmnd_extend per step and process CPU time per step, `--steps` steps after `--warmup`
warm-up steps, `--repeats` times; beside them the device half's counters and the md5 of the records. One JSON line.
  python tools/top_step.py [--top 10] [--lib PATH]      --top -1: the default -k 25 step; --lib: another build's libdiamond_hip.so
                                                         (the parent commit's, for DESIGN.md 5.0)
  python tools/top_step.py --blastx --top -1 [--id 50 --query-cover 50]
                                                         the C4 workload instead (bench.py's: the first 5 000 queries back-translated into
                                                         DNA reads, six contexts, default sensitivity, read lengths set), with HSP filters
  python tools/top_step.py --ext full -k 25          the same step over the whole matrix of every target with a seed hit (--ext full;
  python tools/top_step.py --ext full --top 10        -k N implies --top -1), for DESIGN.md 5.0-full
The seed stage runs once, outside the timed region: every step extends the same seed hits."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diamond_amd import hip, synth, workload      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--top", type=float, default=10.0)
    ap.add_argument("--families", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=12)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--blastx", action="store_true")
    ap.add_argument("--id", type=float, default=0.0)
    ap.add_argument("--query-cover", type=float, default=0.0)
    ap.add_argument("--ext", choices=["banded-fast", "banded-slow", "full"], default=None)
    ap.add_argument("-k", "--max-target-seqs", type=int, default=None)
    args = ap.parse_args()
    if args.max_target_seqs is not None:
        args.top = -1.0
    if args.lib:
        hip.LIB_PATH = os.path.abspath(args.lib)
    db, doff, q, qoff = synth.generate(args.families, members=10, queries=args.queries, seed=20260923)
    source_lens = None
    if args.blastx:
        n_reads = min(args.queries, 5000)
        dna, dna_off = synth.back_translate(q[:qoff[n_reads]], qoff[:n_reads + 1], seed=5)
        qd, ql = hip.translated_block(dna, dna_off)
        source_lens = np.diff(dna_off)
    else:
        qd, ql = workload.sequence_set(q, qoff)
    td, tl = workload.sequence_set(db, doff)
    params = hip.default_params()
    params.db_letters = float(doff[-1])
    ctx = hip.Context(device=0, params=params)
    try:
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, td, tl)
        sp, gf = hip.seed_params_preset("default" if args.blastx else "fast", params, threads=8 if args.blastx else 1)
        if args.blastx:
            sp.query_translated = 1
            ctx.set_query_contexts(6)
            ctx.set_query_source_lengths(source_lens)
        ctx.set_gapped_filter(gf)
        ctx.set_filters(min_id=args.id, query_cover=args.query_cover)
        ctx.set_top_percent(args.top if args.top >= 0 else None)
        if args.max_target_seqs is not None:
            ctx.set_max_target_seqs(args.max_target_seqs)
        if args.ext:
            ctx.set_extension_mode({"banded-fast": hip.EXT_BANDED_FAST, "banded-slow": hip.EXT_BANDED_SLOW, "full": hip.EXT_FULL}[args.ext])
        hits = ctx.seed_search(sp)
        reps, md5, n_records = [], None, 0
        for r in range(args.repeats):
            wall, cpu = [], []
            for s in range(args.warmup + args.steps):
                c0, t0 = time.process_time(), time.perf_counter()
                m, _ = ctx.extend(qd, td, hits, threads=args.threads)
                t1, c1 = time.perf_counter(), time.process_time()
                if s >= args.warmup:
                    wall.append((t1 - t0) * 1e3)
                    cpu.append((c1 - c0) * 1e3)
            reps.append(dict(wall_ms_median=float(np.median(wall)), wall_ms_mean=float(np.mean(wall)), cpu_ms_mean=float(np.mean(cpu))))
            md5, n_records = hashlib.md5(m.tobytes()).hexdigest(), len(m)
        dv, st = ctx.extend_device_stats(), ctx.extend_stats()
        w = [x["wall_ms_median"] for x in reps]
        print(json.dumps(dict(top=args.top, ext=args.ext or "default", k=args.max_target_seqs, blastx=args.blastx, id=args.id, query_cover=args.query_cover, lib=args.lib or "this build", seed_hits=int(len(hits)), records=n_records, records_md5=md5,
                              wall_ms_median_of_repeats=float(np.median(w)), wall_ms_spread=float(max(w) - min(w)),
                              cpu_ms_median_of_repeats=float(np.median([x["cpu_ms_mean"] for x in reps])), repeats=reps,
                              device=dict(queries=dv["queries"], back_to_host=dv["queries_back_to_host"], capped=dv["queries_capped"],
                                          records=dv["records"], items=dv["items"],
                                          lane_use=dv["band_diagonal_steps"] / dv["wavefront_diagonal_steps"] if dv["wavefront_diagonal_steps"] else None,
                                          round1_sweep_ms=st["round1_swipe_kernel_ms"], round2_sweep_ms=st["round2_swipe_kernel_ms"], walk_ms=st["traceback_kernel_ms"],
                                          records_filtered=dv["records_filtered"], on_filter_threshold=dv["queries_on_filter_threshold"]))))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
