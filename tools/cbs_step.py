#!/usr/bin/env python3
"""Times the extension stage with --comp-based-stats 3 and 4 on the C2 workload (bench.py's: 10 000 queries x 1M sequences, --fast,
blocks resident) through hip.Context, the host form of the matrix adjustment (DMND_CBS_DEVICE=0) and the device form (default)
INTERLEAVED in one process: A B A B ..., `--warmup` steps of each first, then `--steps` of each. Per mode and form: wall time of
dmnd_extend per step (median, and the range over the steps), process CPU time per step, and from the device form's counters the
kernel's time, the pairs per step and the shares handed back. The records of the two forms must be the same bytes.
  python tools/cbs_step.py [--modes 3 4] [--lib PATH]      --lib: another build's libdiamond_hip.so (the parent commit's: it has the
                                                            host form only, so both columns then time the same code)
  python tools/cbs_step.py --host-only                     both columns run the host form: what the host form takes when no
                                                            device-form step runs between its steps
  python tools/cbs_step.py --extend-device                 the matrix adjustment is the device form in both columns; the "host" column runs
                                                            the host path's ranking loop around it (DMND_EXTEND_DEVICE=0), the "device" column
                                                            the default: the device half of the extension stage with the adjustment inside.
                                                            With --lib of a build without that route both columns time its default form
The seed stage runs once, outside the timed region: every step extends the same seed hits."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diamond_amd import hip, synth, workload      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", type=int, nargs="+", default=[3, 4])
    ap.add_argument("--families", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=12)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--extend-device", action="store_true")
    args = ap.parse_args()
    if args.lib:
        hip.LIB_PATH = os.path.abspath(args.lib)
    db, doff, q, qoff = synth.generate(args.families, members=10, queries=args.queries, seed=20260923)
    qd, ql = workload.sequence_set(q, qoff)
    td, tl = workload.sequence_set(db, doff)
    params = hip.default_params()
    params.db_letters = float(doff[-1])
    ctx = hip.Context(device=0, params=params)
    have_stats = hasattr(ctx.lib, "dmnd_cbs_device_stats")
    try:
        ctx.upload_block(hip.QUERY, qd, ql)
        ctx.upload_block(hip.TARGET, td, tl)
        sp, gf = hip.seed_params_preset("fast", params, threads=1)
        ctx.set_gapped_filter(gf)
        hits = ctx.seed_search(sp)
        for mode in args.modes:
            ctx.set_comp_based_stats(mode)
            forms = {"host": dict(wall=[], cpu=[]), "device": dict(wall=[], cpu=[])}
            stats = ext = None
            switch = "DMND_EXTEND_DEVICE" if args.extend_device else "DMND_CBS_DEVICE"
            for s in range(args.warmup + args.steps):
                for form in ("host", "device"):
                    if form == "host" or args.host_only:
                        os.environ[switch] = "0"
                    else:
                        os.environ.pop(switch, None)
                    c0, t0 = time.process_time(), time.perf_counter()
                    m, _ = ctx.extend(qd, td, hits, threads=args.threads)
                    t1, c1 = time.perf_counter(), time.process_time()
                    f = forms[form]
                    if s >= args.warmup:
                        f["wall"].append((t1 - t0) * 1e3)
                        f["cpu"].append((c1 - c0) * 1e3)
                    f["m"] = m
                    if form == "device" and have_stats:
                        stats = ctx.cbs_device_stats()
                        ext = ctx.extend_device_stats()
            os.environ.pop(switch, None)
            out = dict(mode=mode, lib=args.lib or "this build", host_only=args.host_only, extend_device=args.extend_device, seed_hits=int(len(hits)), steps=args.steps, threads=args.threads,
                       same_records=bool(np.array_equal(forms["host"]["m"], forms["device"]["m"])), records=len(forms["host"]["m"]))
            for form, f in forms.items():
                out[form] = dict(wall_ms_median=float(np.median(f["wall"])), wall_ms_min=float(min(f["wall"])), wall_ms_max=float(max(f["wall"])),
                                 cpu_ms_mean=float(np.mean(f["cpu"])))
            if stats and stats["pairs"]:
                n = stats["pairs"]
                out["device"].update(kernel_ms=stats["kernel_ms"], pairs=n, decided_on_device=stats["device"] / n, back_by_rounding=stats["rounding"] / n,
                                     back_by_iterations=stats["iterations"] / n, back_by_rule=stats["rule"] / n)
            if ext and args.extend_device:
                out["device"].update(queries_on_device=ext["queries"], queries_back_to_host=ext["queries_back_to_host"])
            print(json.dumps(out), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
