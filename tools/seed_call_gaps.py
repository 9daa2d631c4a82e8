#!/usr/bin/env python3
"""Timeline of ONE seed-stage call from a rocprofv3 --kernel-trace CSV: every kernel on the seed stage's queue from the call's
first clear to its hit gather, with the idle gap in front of it (what the host's waits between the launches cost the device).
usage: seed_call_gaps.py KERNEL_TRACE.csv [which call, counted from the end: default 3]"""
import csv
import sys


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    back = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    stream = [r for r in rows if "seed_stream_fast" in r["Kernel_Name"]]
    queue = stream[-back]["Queue_Id"]
    sel = sorted((r for r in rows if r["Queue_Id"] == queue), key=lambda r: int(r["Start_Timestamp"]))
    k = [i for i, r in enumerate(sel) if "seed_stream_fast" in r["Kernel_Name"]][-back]
    while k > 0 and "seed_clear" not in sel[k]["Kernel_Name"]:
        k -= 1
    t0 = prev_end = None
    busy = gaps = 0.0
    for r in sel[k:]:
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        t0 = s if t0 is None else t0
        gap = (s - prev_end) / 1e3 if prev_end is not None else 0.0
        busy += (e - s) / 1e3
        gaps += max(gap, 0.0)
        print("%8.1f us  gap %6.1f  kernel %7.1f  %s" % ((s - t0) / 1e3, gap, (e - s) / 1e3, r["Kernel_Name"][:90]))
        prev_end = e
        if "hit_gather" in r["Kernel_Name"]:
            break
    print("first clear to the end of the gather: %.1f us = kernels %.1f us + gaps %.1f us" % ((prev_end - t0) / 1e3, busy, gaps))


if __name__ == "__main__":
    main()
