#!/usr/bin/env python3
"""Fixed-lag smoothing: what one slide of a window costs (gpslam_hip_marginalize_head).

SE(3) GP chain with odometry (synthetic.pose3_chain), windows of 1e4 and 1e5 states slid by 100.  Per window, medians over --slides slides, wall clock in ms
(every call ends with a stream synchronisation):
  marginalize_head(100), append_states(100) + the new factors, compile(), two Gauss-Newton iterations;
  the alternative the library offered before: clear_factors + every factor of the window again + compile() + the same iterations;
  marginalize_head(k) at k = 1, 100, 10 000 on a fresh window, and k_head_schur alone in those calls: the kernel's own time from a
  rocprofv3 --kernel-trace run of a child process (--schur-child) that makes nothing but those calls;
  two Gauss-Newton iterations of a fresh window as it is, and of the same window with a state Gaussian whose A is zero on state 0 --
  the same solution, but compile() turns Plan::fold_retract and Plan::lines off: what carrying a head prior costs an iteration.
With --landmarks: a Plaza-like SE(2) window (synthetic.pose2_range_chain: odometry, interpolated ranges at Plaza's rate, 4 beacons seen
from everywhere) slid by 100 with the head marginalised onto the landmarks (gpslam_hip_marginalize_head_onto_landmarks): the cost of
marginalize_head, of k_head_schur_border alone (the kernel trace of a child process) and of two iterations with the border Gaussian.
Prints one JSON line per window; profiles/fixed_lag.txt keeps a run."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpslam_amd as gp                      # noqa: E402
from gpslam_amd import synthetic as S        # noqa: E402


def window_of(p, lo, hi, new_from=None):
    """states lo .. hi - 1 of the chain and the factors among them (new_from: only those that touch a state >= new_from)"""
    out = dict(kind=p["kind"], qc=p["qc"], N=hi - lo, pose=p["pose"][lo:hi], vel=p["vel"][lo:hi])
    for key, others, two in (("gp_left", ["gp_dt"], 1), ("between_left", ["between_meas", "between_sig"], 1), ("prior_idx", ["prior_pose", "prior_sig"], 0)):
        idx = p[key]
        m = (idx >= lo) & (idx + two < hi)
        if new_from is not None:
            m &= idx + two >= new_from
        out[key] = (idx[m] - lo).astype(np.int32)
        for o in others:
            out[o] = p[o][m]
    return out


def add_factors(dev, w):
    dev.add_gp_priors(w["gp_left"], w["gp_dt"])
    if len(w["prior_idx"]):
        dev.add_pose_priors(w["prior_idx"], w["prior_pose"], w["prior_sig"])
    dev.add_between(w["between_left"], w["between_meas"], w["between_sig"])


def ms(f):
    t = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t)


SCHUR_KS, SCHUR_REPS = (1, 100, 10000), 3


def schur_calls(W, timed=None):
    """marginalize_head(k) on fresh windows of W states, SCHUR_REPS times per k of SCHUR_KS below W, in that order"""
    p = S.pose3_chain(W)
    for k in SCHUR_KS:
        if k >= W:
            continue
        for _ in range(SCHUR_REPS):
            d2 = S.apply(p, gp.ChainSolver(p["kind"]))
            d2.iterate_gn()
            t = ms(lambda: d2.marginalize_head(k))
            if timed is not None:
                timed.setdefault(k, []).append(t)
            d2.close()


def schur_kernel_us(W):
    """k_head_schur's own time per k: the kernel trace of a child process that runs schur_calls(W); best of SCHUR_REPS, in us"""
    tmp = tempfile.mkdtemp(prefix="fixed_lag_trace_")
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                        "--schur-child", str(W)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            rows += [r for r in csv.DictReader(open(path)) if "k_head_schur" in r["Kernel_Name"]]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ks = [k for k in SCHUR_KS if k < W]
    if len(rows) != len(ks) * SCHUR_REPS:
        raise RuntimeError("the kernel trace holds %d launches of k_head_schur, expected %d" % (len(rows), len(ks) * SCHUR_REPS))
    dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    return {k: round(min(dur[i * SCHUR_REPS:(i + 1) * SCHUR_REPS]), 2) for i, k in enumerate(ks)}


def bench(W, step, slides):
    p = S.pose3_chain(W + step * (slides + 1))
    dev = S.apply(window_of(p, 0, W), gp.ChainSolver(p["kind"]))
    dev.run_gn(2)
    rows = {k: [] for k in ("marginalize", "append_add", "compile", "two_gn", "alt_readd", "alt_compile", "alt_two_gn")}
    lo, hi = 0, W
    for _ in range(slides):
        rows["marginalize"].append(ms(lambda: dev.marginalize_head(step)))
        new = window_of(p, lo + step, hi + step, new_from=hi)

        def grow():
            dev.append_states(p["pose"][hi:hi + step], p["vel"][hi:hi + step])
            add_factors(dev, new)
        rows["append_add"].append(ms(grow))
        rows["compile"].append(ms(dev.compile))
        rows["two_gn"].append(ms(lambda: (dev.iterate_gn(), dev.iterate_gn())))
        lo, hi = lo + step, hi + step
        # the alternative: the same handle, every factor of the window again (the head's information is lost)
        w = window_of(p, lo, hi)
        idx, pl, vl, A, c = dev.get_state_gaussians()

        def readd():
            dev.clear_factors()
            add_factors(dev, w)
            dev.add_state_gaussians(idx, pl, vl, A, c)      # (kept, so that the next slide starts from the same graph)
        rows["alt_readd"].append(ms(readd))
        rows["alt_compile"].append(ms(dev.compile))
        rows["alt_two_gn"].append(ms(lambda: (dev.iterate_gn(), dev.iterate_gn())))
    out = dict(window=W, step=step, slides=slides, **{k: round(statistics.median(v), 3) for k, v in rows.items()})
    dev.close()
    timed = {}
    schur_calls(W, timed)
    for k, t in timed.items():
        out["marginalize_head_k%d" % k] = round(min(t), 3)
    # what a state Gaussian costs an iteration: the same window without one, and with one that says nothing (A = 0)
    w = window_of(p, 0, W)
    b = 2 * w["vel"].shape[1]
    for name in ("two_gn_plain", "two_gn_zero_gaussian"):
        d3 = S.apply(w, gp.ChainSolver(p["kind"]))
        if name == "two_gn_zero_gaussian":
            d3.add_state_gaussians([0], w["pose"][:1], w["vel"][:1], np.zeros((1, b, b)), np.zeros((1, b)))
            d3.compile()
        d3.run_gn(2)
        out[name] = round(statistics.median(ms(lambda: (d3.iterate_gn(), d3.iterate_gn())) for _ in range(7)), 3)
        d3.close()
    return out


# ---------------------------------------------------------------- the landmark case
RANGE_KEYS = ("range_lm", "range_z", "range_sigma", "range_dt", "range_tau")


def lm_window_of(p, lo, hi, new_from=None):
    out = window_of(p, lo, hi, new_from)
    idx = p["range_left"]
    m = (idx >= lo) & (idx + 1 < hi)
    if new_from is not None:
        m &= idx + 1 >= new_from
    out["range_left"] = (idx[m] - lo).astype(np.int32)
    for o in RANGE_KEYS:
        out[o] = p[o][m]
    for key in ("landmarks", "lprior_idx", "lprior", "lprior_sig"):
        out[key] = p[key]
    return out


def lm_solver(w):
    dev = S.apply(w, gp.ChainSolver(w["kind"], landmark_dim=2))
    dev.marginalize_head_onto_landmarks()
    return dev


def border_calls(W, step, timed=None):
    """marginalize_head(step) onto the landmarks on fresh windows of W states, SCHUR_REPS times"""
    p = S.pose2_range_chain(W, L=4)
    for _ in range(SCHUR_REPS):
        d2 = lm_solver(lm_window_of(p, 0, W))
        d2.iterate_gn()
        t = ms(lambda: d2.marginalize_head(step))
        if timed is not None:
            timed.append(t)
        d2.close()


def border_kernel_us(W, step):
    tmp = tempfile.mkdtemp(prefix="fixed_lag_trace_")
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                        "--border-child", str(W), "--step", str(step)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            rows += [r for r in csv.DictReader(open(path)) if "k_head_schur_border" in r["Kernel_Name"]]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if len(rows) != SCHUR_REPS:
        raise RuntimeError("the kernel trace holds %d launches of k_head_schur_border, expected %d" % (len(rows), SCHUR_REPS))
    return round(min((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows), 2)


def bench_landmarks(W, step, slides):
    p = S.pose2_range_chain(W + step * (slides + 1), L=4)
    dev = lm_solver(lm_window_of(p, 0, W))
    for _ in range(2):
        dev.iterate_gn()
    rows = {k: [] for k in ("marginalize", "append_add", "compile", "two_gn")}
    lo, hi = 0, W
    for _ in range(slides):
        rows["marginalize"].append(ms(lambda: dev.marginalize_head(step)))
        new = lm_window_of(p, lo + step, hi + step, new_from=hi)

        def grow():
            dev.append_states(p["pose"][hi:hi + step], p["vel"][hi:hi + step])
            add_factors(dev, new)
            dev.add_interp_range(new["range_left"], new["range_lm"], new["range_z"], new["range_sigma"], new["range_dt"], new["range_tau"])
        rows["append_add"].append(ms(grow))
        rows["compile"].append(ms(dev.compile))
        rows["two_gn"].append(ms(lambda: (dev.iterate_gn(), dev.iterate_gn())))
        lo, hi = lo + step, hi + step
    out = dict(case="landmarks", window=W, step=step, slides=slides, beacons=4, **{k: round(statistics.median(v), 3) for k, v in rows.items()})
    dev.close()
    timed = []
    border_calls(W, step, timed)
    out["marginalize_head_fresh"] = round(min(timed), 3)
    d3 = lm_solver(lm_window_of(p, 0, W))
    d3.iterate_gn()
    out["two_gn_plain"] = round(statistics.median(ms(lambda: (d3.iterate_gn(), d3.iterate_gn())) for _ in range(7)), 3)
    d3.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--step", type=int, default=100)
    ap.add_argument("--slides", type=int, default=5)
    ap.add_argument("--schur-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--landmarks", action="store_true", help="the Plaza-like SE(2) window with 4 beacons instead (default window 4000)")
    ap.add_argument("--border-child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.schur_child:
        schur_calls(a.schur_child)
        sys.exit(0)
    if a.border_child:
        border_calls(a.border_child, a.step)
        sys.exit(0)
    if a.landmarks:
        for W in ([4000] if a.windows == [10000, 100000] else a.windows):
            kernel = border_kernel_us(W, a.step)          # (a child process of its own, before this one opens the device)
            res = bench_landmarks(W, a.step, a.slides)
            res["k_head_schur_border_us"] = kernel
            print(json.dumps(res), flush=True)
        sys.exit(0)
    for W in a.windows:
        kernel = schur_kernel_us(W)          # (a child process of its own, before this one opens the device)
        res = bench(W, a.step, a.slides)
        res.update({"k_head_schur_us_k%d" % k: v for k, v in kernel.items()})
        print(json.dumps(res), flush=True)
