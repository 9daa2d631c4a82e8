#!/usr/bin/env python3
"""Where the masking of one C2 database block spends its time (round 5): tantan (dmnd_mask_block) and motif soft masking
(dmnd_soft_mask_block) timed apart on the 3.0e8-letter block, host wall clock per call; with DMND_TRACE=1 the laps of
dmnd_mask_block go to stderr; under `rocprofv3 --kernel-trace --stats` the kernels' own times. usage: tools/mask_probe.py [runs]
--seg [runs] [threads]: SEG on the same block instead -- the host form (dmnd_seg_mask_block, `threads` host threads, default 16) against
the device form (dmnd_seg_mask_block_device), one warm-up and then `runs` (default 5) timed repeats of each, the kernels' time apart
from the call's; one JSON line (SEG_PROBE_JSON) at the end."""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diamond_amd import hip, synth, workload

seg_mode = len(sys.argv) > 1 and sys.argv[1] == "--seg"
if seg_mode:
    del sys.argv[1]
runs = int(sys.argv[1]) if len(sys.argv) > 1 else (5 if seg_mode else 4)
db, doff, q, qoff = synth.generate(100_000, members=10, queries=10_000, seed=20260923)
td, tl = workload.sequence_set(db, doff)
qd, ql = workload.sequence_set(q, qoff)
hip.load_motif_table()
params = hip.default_params()
raw, mc = hip.Context(params=params), hip.Context(params=params)
for c in (raw, mc):
    c.upload_block(hip.QUERY, qd, ql)
    c.upload_block(hip.TARGET, td, tl)
td_m = td.copy()
if seg_mode:
    import json
    import numpy as np
    threads = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    host_ms, call_ms, kernel_ms, stats, n_host, n_dev = [], [], [], None, None, None
    for r in range(-1, runs):                                              # run -1 = warm-up
        td_m[:] = td
        t0 = time.perf_counter()
        n_host = hip.seg_mask_block(td_m, tl, threads=threads)
        t1 = time.perf_counter()
        want = td_m.copy() if r < 0 else None
        td_m[:] = td
        mc.copy_block(hip.TARGET, raw)
        t2 = time.perf_counter()
        n_dev = mc.seg_mask_block(hip.TARGET, td_m)
        t3 = time.perf_counter()
        stats = mc.seg_stats()
        if r < 0:
            assert n_dev == n_host and np.array_equal(td_m, want), "device SEG differs from the host form"
        else:
            host_ms.append((t1 - t0) * 1e3); call_ms.append((t3 - t2) * 1e3); kernel_ms.append(stats["kernel_ms"])
        print("SEG_PROBE run %d: host (%d threads) %.2f ms, device call %.2f ms (kernels %.2f), masked letters %d / %d, work list %d, handed back %d, ranges %d"
              % (r, threads, (t1 - t0) * 1e3, (t3 - t2) * 1e3, stats["kernel_ms"], n_host, n_dev, stats["work"], stats["handed_back"], stats["ranges"]), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    print("SEG_PROBE_JSON " + json.dumps(dict(letters=int(td.size), sequences=int(len(tl) - 1), threads=threads, runs=runs, host_ms=host_ms, device_call_ms=call_ms,
                                              device_kernel_ms=kernel_ms, host_ms_median=med(host_ms), device_call_ms_median=med(call_ms), device_kernel_ms_median=med(kernel_ms),
                                              masked_letters=int(n_dev), **stats)), flush=True)
    raw.close(); mc.close()
    sys.exit(0)
for r in range(runs):
    mc.copy_block(hip.TARGET, raw)
    t0 = time.perf_counter()
    n = mc.mask_block(hip.TARGET, td_m)
    t1 = time.perf_counter()
    mc.soft_mask_block(hip.TARGET)
    t2 = time.perf_counter()
    print("MASK_PROBE run %d: tantan call %.2f ms (kernel %.2f), motif soft masking call %.2f ms, masked letters %d" % (r, (t1 - t0) * 1e3, mc.mask_kernel_ms(), (t2 - t1) * 1e3, n), flush=True)
raw.close(); mc.close()
