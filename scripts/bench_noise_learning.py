#!/usr/bin/env python3
"""What the measurement-noise statistic costs (gpslam_hip_meas_noise_statistic) next to gpslam_hip_marginals,
whose S / S_next / S_x_lm / S_lm it reads, and what Plaza2's range sigma is when it is learned by EM.

Graphs: Plaza2 (4091 SE(2) states, 1816 interpolated ranges, 4 landmarks; tests/golden/plaza2.npz) and config 5 as
tests/test_gpu_configs.py builds it (SE(3) GP chain with odometry and 4 interpolated GPS factors per interval) at 1e5 and 1e6 states.
Per graph, one JSON line:

  statistic_ms, marginals_ms   wall clock of ChainSolver.meas_noise_statistic() / .marginals() on WARMED handles (either ran once
                               before), every call ending in its own synchronisation; medians over --reps handles, three statistics
                               behind each marginals -- the same process, the same handle
  kernels_us                   from a rocprofv3 --kernel-trace run of a child process (--trace-child), per call of the statistic: the
                               summed time of k_mn_stat and of k_mn_reduce over the chunks of a call, of every k_meas launch of a
                               marginals + statistic pair (the inspection launches and the marginals' own linearisation), and the level-0 k_mg_forward / k_mg_backward of the same handle ([median, minimum] per launch)
  must_read_bytes, stat_gbs    the bytes the contraction has to read -- e and J of every factor, S_i and Sn_i once per distinct
                               interval (S_{i+1} is S_i of the next one), the landmark columns and block per factor -- over the
                               time of k_mn_stat per call

--learn (Plaza2 only): evidence.learn_meas_noise(mode="scale") of the range sigma from the recipe's 0.5, alone and with
with_qc=(Qc, scale_only), Levenberg-Marquardt with 30 iterations at most: wall time, steps, sigma and Qc scale per step, log Z.

Run every graph as a step of its own under a limit sized to it, the steps chained so that none starts behind one that failed:
  timeout -k 10 240 python scripts/bench_noise_learning.py --graphs plaza2 && timeout -k 10 300 python scripts/bench_noise_learning.py --graphs 100000 &&
  timeout -k 10 540 python scripts/bench_noise_learning.py --graphs 1000000 --reps 3 && timeout -k 10 400 python scripts/bench_noise_learning.py --learn"""
import argparse
import csv
import glob
import json
import os
import shutil
import signal
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpslam_amd as gp                      # noqa: E402
from gpslam_amd import evidence as EV        # noqa: E402
from gpslam_amd import synthetic as S        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plaza_problem():
    from gpslam_amd import plaza
    return plaza, plaza.build_problem(plaza.load(os.path.join(ROOT, "tests", "golden", "plaza2.npz")))


def make(which):
    """(a function that returns a fresh compiled handle of the graph, the MEAS_* kind, the factors' left states, landmark doubles per factor)"""
    if which == "plaza2":
        plaza, p = plaza_problem()
        return (lambda: plaza.apply(p, gp.ChainSolver(gp.POSE2, chart=gp.CHART_FIRST_ORDER, landmark_dim=2))), gp.chain.MEAS_INTERP_RANGE, p["range_left"], 2 * 6 * 2 + 4
    p = S.pose3_gps_chain(int(which), keep_odometry=True)
    return (lambda: S.apply(p, gp.ChainSolver(gp.POSE3))), gp.chain.MEAS_INTERP_GPS, p["gps_left"], 0


def timed_pair(fresh, kind, reps):
    a, b, out = [], [], None
    for _ in range(reps):
        dev = fresh()
        dev.marginals()
        dev.meas_noise_statistic(kind)
        dev.error()
        for _ in range(3):
            t = time.perf_counter()
            dev.marginals()
            b.append(1e3 * (time.perf_counter() - t))
            for _ in range(3):
                t = time.perf_counter()
                out = dev.meas_noise_statistic(kind)
                a.append(1e3 * (time.perf_counter() - t))
        dev.close()
    return statistics.median(a), statistics.median(b), out


def trace_child(which, reps):
    fresh, kind, _, _ = make(which)
    dev = fresh()
    for _ in range(reps + 1):
        dev.marginals()
        dev.meas_noise_statistic(kind)
    dev.close()


def kernel_us(which, reps):
    tmp = tempfile.mkdtemp(prefix="noise_trace_")
    try:
        child = subprocess.Popen(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                                  "--trace-child", which, "--reps", str(reps)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
        try:
            if child.wait(timeout=600) != 0:
                raise RuntimeError("the trace child ended with status %d" % child.returncode)
        except subprocess.TimeoutExpired:
            os.killpg(child.pid, signal.SIGKILL)      # rocprofv3 AND the python under it
            child.wait()
            raise
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(path)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    def dur(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    out = {}
    calls = reps + 1
    for name in ("k_mn_stat", "k_mn_reduce"):       # summed over the chunks of a call (the first call loads the code object: it is in the mean)
        d = [dur(r) for r in rows if name in r["Kernel_Name"]]
        if d:
            out[name + "_per_call"] = round(sum(d) / calls, 2)
            out[name + "_launches_per_call"] = len(d) // calls
    # every k_meas launch of a marginals + statistic pair: the statistic's inspection launches AND the linearisation of the marginals
    d = [dur(r) for r in rows if "k_meas" in r["Kernel_Name"]]
    if d:
        out["k_meas_per_pair"] = round(sum(d) / calls, 2)
        out["k_meas_launches_per_pair"] = len(d) // calls
    for name in ("k_mg_forward", "k_mg_backward"):      # per call the longest launch is level 0's
        d = sorted(dur(r) for r in rows if name in r["Kernel_Name"])[-calls:]
        if d:
            out[name + "_level0"] = [round(statistics.median(d), 2), round(min(d), 2)]
    return out


def measure(which, reps, trace):
    fresh, kind, left, lm_doubles = make(which)
    res = {"graph": which}
    res["statistic_ms"], res["marginals_ms"], (B, Bw, n) = timed_pair(fresh, kind, reps)
    probe = fresh()
    b, rows = probe.b, probe.MEAS_ROWS[kind]
    res.update(states=probe.N, block=b, factors=n, rows=rows, Bw_trace_over_n_r=float(np.trace(Bw)) / (n * rows), ratio=res["statistic_ms"] / res["marginals_ms"])
    probe.close()
    res["must_read_bytes"] = int(n * rows * (2 * b + 4) * 8 + len(np.unique(left)) * 2 * b * b * 8 + n * lm_doubles * 8)
    if trace:
        k = kernel_us(which, max(3, reps))
        res["kernels_us"] = k
        if "k_mn_stat_per_call" in k:
            res["stat_gbs"] = round(res["must_read_bytes"] / (k["k_mn_stat_per_call"] * 1e-6) / 1e9, 1)
    for key, v in list(res.items()):
        if isinstance(v, float):
            res[key] = round(v, 4)
    return res


def learn():
    plaza, p = plaza_problem()
    dev = plaza.apply(p, gp.ChainSolver(gp.POSE2, chart=gp.CHART_FIRST_ORDER, landmark_dim=2))
    par = dev.default_params(use_lm=1, max_iterations=30)
    kind = gp.chain.MEAS_INTERP_RANGE
    args = (dev, kind, p["pose"], p["vel"], p["landmarks"])
    EV.learn_meas_noise(*args, params=par, steps=1, cov0=np.array([[0.25]]))      # (warm: buffers, code objects)
    for name, with_qc in (("alone", None), ("with_qc", (np.asarray(p["qc"]), True))):
        dev.set_qc(p["qc"])
        t = time.perf_counter()
        out = EV.learn_meas_noise(*args, params=par, steps=40, rtol=1e-3, mode="scale", with_qc=with_qc, cov0=np.array([[0.25]]))
        secs = time.perf_counter() - t
        theta = [o[0][0] if with_qc else o[0] for o in out]
        res = {"graph": "plaza2", "learn": name, "seconds": round(secs, 3), "steps": len(out), "iterations": int(sum(o[2] for o in out)),
               "range_sigma": [round(float(np.sqrt(0.25 * th)), 5) for th in theta], "logZ": [o[1] for o in out]}
        if with_qc:
            res["qc_scale"] = [round(float(o[0][1][0, 0] / p["qc"][0, 0]), 5) for o in out]
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graphs", default="100000,1000000,plaza2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child (kernel times)")
    ap.add_argument("--learn", action="store_true", help="Plaza2: the range sigma by learn_meas_noise, alone and with_qc")
    ap.add_argument("--trace-child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        trace_child(a.trace_child, a.reps)
        return
    if a.learn:
        learn()
        return
    for which in a.graphs.split(","):
        print(json.dumps(measure(which, a.reps, not a.no_trace)), flush=True)


if __name__ == "__main__":
    main()
