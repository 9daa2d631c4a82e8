#!/usr/bin/env python3
"""Measures what the guards of the device form of the matrix adjustment (diamond_amd/csrc/cbs_core.h) have to cover: the lane
emulator (the kernel's schedule and reduction trees, glibc's libm) against the host arithmetic (cbs_adjust.cpp) over the five
goldens tests/golden/cbs_*.tap and the structural edge cases of the tests -- largest deviation of the unrounded scores, of rnorm
at the convergence tests (relative to max(rnorm, tolerance)) and of the rule's angle; the host's iteration counts; the share of pairs each guard hands back.
No GPU. Writes profiles/cbs_device_guards.json (or the path given)."""
import json
import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import tapfile  # noqa: E402
import cbs_emu_py as ce  # noqa: E402
from diamond_amd import hip  # noqa: E402

CASES = [("cbs_mode3.tap", "blosum62", 3), ("cbs_mode4.tap", "blosum62", 4), ("cbs_mode5.tap", "blosum62", 5),
         ("cbs_blosum45.tap", "blosum45", 5), ("cbs_pam70.tap", "pam70", 4)]
TOL = 1e-8          # cbs_err_tolerance


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cbs_device_guards.json")
    eps_round, eps_norm, eps_angle, cap = ce.guards()
    dev = dict(score=0.0, rnorm_relative=0.0, rnorm_abs=0.0, angle=0.0)
    its = Counter()
    not_converged = 0
    sets = {}

    def one(p, mode, comp, n, target, tally):
        nonlocal not_converged
        e = ce.pair(p, mode, comp, n, target)
        h = ce.host_pair(p, mode, comp, n, target)
        if mode in (2, 3, 5) and len(target) and n and np.isfinite(e["angle"]) and np.isfinite(h["angle"]):
            dev["angle"] = max(dev["angle"], abs(e["angle"] - h["angle"]))
        if h["rule"] == ce.RULE_REL_ENTROPY:
            if h["converged"]:
                its[h["its"]] += 1
            else:
                not_converged += 1
            k = min(len(e["rnorm"]), len(h["rnorm"]))
            if k:
                # a deviation d flips `rnorm > tol` only if |rnorm - tol| <= d. With d <= delta * max(rnorm, tol) that needs rnorm within the
                # relative band delta around tol on either side: delta is the quantity eps_norm has to cover
                d = np.abs(e["rnorm"][:k] - h["rnorm"][:k])
                dev["rnorm_abs"] = max(dev["rnorm_abs"], float(d.max()))
                dev["rnorm_relative"] = max(dev["rnorm_relative"], float((d / np.maximum(h["rnorm"][:k], TOL)).max()))
            both = np.isfinite(e["scores"]) & np.isfinite(h["scores"])
            if both.any():
                dev["score"] = max(dev["score"], float(np.abs(e["scores"][both] - h["scores"][both]).max()))
        if h["rule"] != ce.RULE_SCALE_OLD:
            tally["pairs"] += 1
            tally[("device", "rounding", "iterations", "rule")[e["status"]]] += 1
        else:
            tally["scale_old"] += 1
        if e["status"] == ce.ST_DEVICE:
            assert e["rule"] == h["rule"], (e["rule"], h["rule"])
            if e["rule"] == ce.RULE_REL_ENTROPY:
                assert np.array_equal(e["matrix"], h["matrix"])

    for name, matrix, mode in CASES:
        hdr, adj, tmx = tapfile.read_cbs_tap(os.path.join(ROOT, "tests", "golden", name))
        p = hip.matrix_params(matrix)
        tally = Counter()
        for r in adj + tmx:
            one(p, mode, r["query_comp"], r["query_len"], r["target"], tally)
        sets[name] = dict(tally)
    tally = Counter()
    for matrix in ("blosum62", "blosum45", "pam70"):
        p = hip.matrix_params(matrix)
        for mode in (3, 4, 5):
            for _name, q, t in ce.edge_pairs():
                comp, n = hip.cbs_composition(q)
                one(p, mode, comp, n, t, tally)
    sets["edge cases"] = dict(tally)
    top = max(its) if its else 0
    pow2 = 1
    while pow2 < 2 * top:
        pow2 *= 2
    res = dict(
        what="lane emulator (kernel schedule, glibc libm) against the host arithmetic; no GPU",
        largest_deviation=dev,
        guard_width=dict(eps_round=eps_round, eps_norm_relative_to_err_tolerance=eps_norm, eps_angle_degrees=eps_angle),
        width_over_deviation=dict(eps_round=eps_round / dev["score"] if dev["score"] else None,
                                  eps_norm=eps_norm / dev["rnorm_relative"] if dev["rnorm_relative"] else None,
                                  eps_angle=eps_angle / dev["angle"] if dev["angle"] else None),
        host_iterations_histogram={str(k): its[k] for k in sorted(its)},
        host_pairs_not_converged=not_converged,
        largest_converging_iteration_count=top,
        smallest_power_of_two_with_factor_2_to_spare=pow2,
        device_iteration_cap=cap,
        pairs_by_status_without_scale_old=sets)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
