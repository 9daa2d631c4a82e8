"""The device form of the composition-based matrix adjustment (diamond_amd/csrc/cbs_core.h, the code of cbs_adjust_kernel) on the
CPU: the lane emulator (tests/emu/cbs_emu.cpp) runs the kernel's 64-lane schedule, reduction trees and guards with glibc's libm
over the reference's own answers (tests/golden/cbs_*.tap). What the device decides (status 0) has to equal the reference entry for
entry; what it hands back is computed by the host form, whose answers are pinned here as well; and it may hand back only a small
share, or the kernel would be a detour."""
import json
import os
import shutil
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import tapfile  # noqa: E402
import cbs_emu_py as ce  # noqa: E402
from diamond_amd import hip  # noqa: E402

CASES = [("cbs_mode3.tap", "blosum62", 3), ("cbs_mode4.tap", "blosum62", 4), ("cbs_mode5.tap", "blosum62", 5),
         ("cbs_blosum45.tap", "blosum45", 5), ("cbs_pam70.tap", "pam70", 4)]
MAX_HANDED_BACK = 0.05          # of a golden's records that are not CBS_RULE_SCALE_OLD


def check_table(got, x, p):
    """The assertions of tests/test_cbs_adjust.py on one 32 x 32 table against a golden `tmx` record."""
    assert np.array_equal(got[:26, :26], x["scores"][:, :26]), (x["rule"], x["query_len"], len(x["target"]))
    assert (got[26:, :] == -128).all() and (got[:, 26:] == -128).all()
    std = hip.matrix_of(p)
    keep = np.ones((26, 26), bool)
    idx = list(range(20)) + [23]
    keep[np.ix_(idx, idx)] = False
    assert np.array_equal(got[:26, :26][keep], std[:26, :26][keep])
    assert x["score_min"] == max(int(x["scores"][np.ix_(idx, idx)].min()), -128)


@pytest.mark.parametrize("name,matrix,mode", CASES)
def test_goldens_through_the_lane_emulator(name, matrix, mode):
    hdr, adj, tmx = tapfile.read_cbs_tap(os.path.join(HERE, "golden", name))
    p = hip.matrix_params(matrix)
    assert hdr["cbs"] == mode and len(adj) > 100 and len(tmx) > 100
    n, handed = 0, 0
    for x in tmx:
        e = ce.pair(p, mode, x["query_comp"], x["query_len"], x["target"])
        if x["rule"] != ce.RULE_SCALE_OLD:
            n += 1
            handed += e["status"] != ce.ST_DEVICE
        if e["status"] == ce.ST_DEVICE:
            assert e["rule"] == x["rule"] == ce.RULE_REL_ENTROPY
            check_table(e["matrix"], x, p)
        else:
            # nothing written; the host form, which then computes the pair, gives the reference's table
            assert (e["matrix"] == ce.UNTOUCHED).all()
            if x["rule"] == ce.RULE_SCALE_OLD:
                assert e["status"] == ce.ST_RULE and mode == 5
            check_table(hip.cbs_target_matrix(p, x["rule"], x["query_comp"], x["query_len"], x["target"]), x, p)
    seen = set()
    for a in adj:
        e = ce.pair(p, mode, a["query_comp"], a["query_len"], a["target"])
        if a["rule"] != ce.RULE_SCALE_OLD:
            n += 1
            handed += e["status"] != ce.ST_DEVICE
        if e["status"] != ce.ST_RULE:
            assert e["rule"] == a["rule"]
        if e["status"] == ce.ST_DEVICE:
            seen.add(e["rule"])
        if e["rule"] == ce.RULE_NONE:
            assert (e["matrix"] == ce.UNTOUCHED).all()
    assert seen == ({-1, 4} if mode in (2, 3) else {4})
    assert n > 100 and handed <= MAX_HANDED_BACK * n, (handed, n)


def test_edge_cases_equal_the_host_form_where_the_device_decides():
    eps_round = ce.guards()[0]
    decided = 0
    for matrix in ("blosum62", "pam70"):
        p = hip.matrix_params(matrix)
        for mode in (3, 4, 5):
            for name, q, t in ce.edge_pairs():
                comp, n = hip.cbs_composition(q)
                e, h = ce.pair(p, mode, comp, n, t), ce.host_pair(p, mode, comp, n, t)
                if e["status"] == ce.ST_DEVICE:
                    decided += 1
                    assert e["rule"] == h["rule"] == hip.cbs_rule(p, mode, comp, n, t), (matrix, mode, name)
                    if e["rule"] == ce.RULE_REL_ENTROPY:
                        assert np.array_equal(e["matrix"], hip.cbs_target_matrix(p, 4, comp, n, t)), (matrix, mode, name)
                        assert np.abs(e["scores"] - h["scores"]).max() < eps_round / 1000
                    else:
                        assert (e["matrix"] == ce.UNTOUCHED).all()
                else:
                    assert (e["matrix"] == ce.UNTOUCHED).all()
                    assert e["status"] != ce.ST_RULE or mode != 4
    assert decided > 100


def test_degenerate_pairs_and_the_iteration_hook():
    p = hip.default_params()
    comp, n = hip.cbs_composition(np.arange(20, dtype=np.int8))
    t = np.arange(20, dtype=np.int8)
    # mode 1, an empty target, a query without residues: no adjustment, decided on the device, nothing written
    for mode, aa, tt in ((1, n, t), (4, n, np.zeros(0, np.int8)), (4, 0, t)):
        e = ce.pair(p, mode, comp, aa, tt)
        assert (e["rule"], e["status"]) == (-1, 0) and (e["matrix"] == ce.UNTOUCHED).all()
    # a cap of one Newton step: every relative-entropy pair goes back by the iteration guard
    e = ce.pair(p, 4, comp, n, t, max_its=1)
    assert (e["rule"], e["status"]) == (4, ce.ST_ITERATIONS) and (e["matrix"] == ce.UNTOUCHED).all() and e["its"] == 1
    e = ce.pair(p, 4, comp, n, t)
    assert (e["rule"], e["status"]) == (4, 0) and np.array_equal(e["matrix"], hip.cbs_target_matrix(p, 4, comp, n, t))
    # a target of mask letters only: its composition is all zero, the pseudocounts make it the background
    t = np.full(30, 23, np.int8)
    e = ce.pair(p, 4, comp, n, t)
    assert e["status"] == 0 and np.array_equal(e["matrix"], hip.cbs_target_matrix(p, 4, comp, n, t)) and e["matrix"][23, 23] == -1


def test_guard_profile_is_what_the_header_holds():
    """profiles/cbs_device_guards.json (tools/cbs_guards.py) records the measurement the widths in cbs_core.h come from: every width
    at least 1000 x the largest deviation of the schedule from the host arithmetic, the cap the smallest power of two with a factor
    of 2 over the longest converging pair."""
    prof = json.load(open(os.path.join(ROOT, "profiles", "cbs_device_guards.json")))
    eps_round, eps_norm, eps_angle, cap = ce.guards()
    w, d = prof["guard_width"], prof["largest_deviation"]
    assert (w["eps_round"], w["eps_norm_relative_to_err_tolerance"], w["eps_angle_degrees"], prof["device_iteration_cap"]) == (eps_round, eps_norm, eps_angle, cap)
    assert eps_round >= 1000 * d["score"] and eps_norm >= 1000 * d["rnorm_relative"] and eps_angle >= 1000 * d["angle"]
    assert cap == prof["smallest_power_of_two_with_factor_2_to_spare"] >= 2 * prof["largest_converging_iteration_count"]


def test_slot_bookkeeping_under_address_sanitizer(tmp_path):
    """Slot numbering and the patch-in of handed-back pairs (cbs_slots_assign, cbs_patch_runs): a stand-alone program over the header
    the library uses, compiled with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the host compiler that built tests/emu"
    exe = str(tmp_path / "cbs_slots_main")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, os.path.join(HERE, "asan", "cbs_slots_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
