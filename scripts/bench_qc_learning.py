#!/usr/bin/env python3
"""What the Qc statistic costs (gpslam_hip_qc_statistic) next to gpslam_hip_marginals, whose S / S_next it reads,
and what learning Qc's scale by EM costs next to the grid of evidence.qc_scale_sweep.

Graphs: BASELINE config 3 (SE(3) GP chain with odometry) at 1e5 and 1e6 states, and Plaza2 (4091 SE(2) states, interpolated ranges, 4
landmarks; tests/golden/plaza2.npz).  Per graph, one JSON line:

  qc_statistic_ms, marginals_ms   wall clock of ChainSolver.qc_statistic() / .marginals() on WARMED handles (either ran once before), every
                                  call ending in its own synchronisation; medians over --reps handles, three statistics behind each marginals
  kernels_us                      from a rocprofv3 --kernel-trace run of a child process (--trace-child): [median, minimum] of k_qc_stat,
                                  k_qc_reduce and, for scale, the level-0 k_mg_forward / k_mg_backward of the same handle
  s_bytes, stat_gbs               the bytes of S and S_next the pass must read, n_f 2 b^2 8 (S_{i+1} is S_i of the next prior), over the
                                  median time of k_qc_stat; the kernel itself asks for three blocks per prior (fetched_bytes), the third
                                  of which the next prior's read finds in the cache when the two share a workgroup

--learn (Plaza2 only): evidence.learn_qc(scale_only=True) from theta = 10 against evidence.qc_scale_sweep over 10^-2 .. 10^2 in steps of
10^0.5 (the grid of tests/test_gpu_evidence.py::test_qc_scale_sweep_follows_the_textbook_curve), both with Levenberg-Marquardt, 30
iterations at most: wall time, optimiser iterations, the scale found and its log-evidence.

k_mg_forward is the parent commit's, byte for byte (scripts/compare_device_code.py).  Run every graph as a step of its own under a limit
sized to it, the steps chained so that none starts behind one that failed:
  timeout -k 10 240 python scripts/bench_qc_learning.py --graphs plaza2 && timeout -k 10 300 python scripts/bench_qc_learning.py --graphs 100000 &&
  timeout -k 10 540 python scripts/bench_qc_learning.py --graphs 1000000 --reps 3 && timeout -k 10 400 python scripts/bench_qc_learning.py --learn"""
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
    """a function that returns a fresh compiled handle of the graph"""
    if which == "plaza2":
        plaza, p = plaza_problem()
        return lambda: plaza.apply(p, gp.ChainSolver(gp.POSE2, chart=gp.CHART_FIRST_ORDER, landmark_dim=2))
    p = S.pose3_chain(int(which))
    return lambda: S.apply(p, gp.ChainSolver(gp.POSE3))


def timed_pair(fresh, reps):
    a, b, out = [], [], None
    for _ in range(reps):
        dev = fresh()
        dev.marginals()
        dev.qc_statistic()
        dev.error()
        for _ in range(3):
            t = time.perf_counter()
            dev.marginals()
            b.append(1e3 * (time.perf_counter() - t))
            for _ in range(3):
                t = time.perf_counter()
                out = dev.qc_statistic()
                a.append(1e3 * (time.perf_counter() - t))
        dev.close()
    return statistics.median(a), statistics.median(b), out


def trace_child(which, reps):
    dev = make(which)()
    for _ in range(reps + 1):
        dev.marginals()
        dev.qc_statistic()
    dev.close()


def kernel_us(which, reps):
    tmp = tempfile.mkdtemp(prefix="qc_trace_")
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
    for name in ("k_qc_stat", "k_qc_reduce"):
        d = [dur(r) for r in rows if name in r["Kernel_Name"]]
        d = d[1:] if len(d) > 1 else d              # (the first launch loads the code object)
        if d:
            out[name] = [round(statistics.median(d), 2), round(min(d), 2)]
    for name in ("k_mg_forward", "k_mg_backward"):      # per call the longest launch is level 0's
        d = sorted(dur(r) for r in rows if name in r["Kernel_Name"])[-(reps + 1):]
        if d:
            out[name + "_level0"] = [round(statistics.median(d), 2), round(min(d), 2)]
    return out


def measure(which, reps, trace):
    fresh = make(which)
    res = {"graph": which}
    res["qc_statistic_ms"], res["marginals_ms"], (A, n_f) = timed_pair(fresh, reps)
    probe = fresh()
    res.update(states=probe.N, block=probe.b, priors=n_f, A_trace=float(np.trace(A)))
    b = probe.b
    probe.close()
    if trace:
        k = kernel_us(which, max(3, reps))
        res["kernels_us"] = k
        if "k_qc_stat" in k:
            res["s_bytes"] = n_f * 2 * b * b * 8
            res["fetched_bytes"] = n_f * 3 * b * b * 8
            res["stat_gbs"] = round(res["s_bytes"] / (k["k_qc_stat"][0] * 1e-6) / 1e9, 1)
    for key, v in list(res.items()):
        if isinstance(v, float):
            res[key] = round(v, 4)
    return res


def learn():
    plaza, p = plaza_problem()
    dev = plaza.apply(p, gp.ChainSolver(gp.POSE2, chart=gp.CHART_FIRST_ORDER, landmark_dim=2))
    par = dev.default_params(use_lm=1, max_iterations=30)
    thetas = 10.0 ** np.arange(-2.0, 2.01, 0.5)
    EV.qc_scale_sweep(dev, p["qc"], [1.0], p["pose"], p["vel"], p["landmarks"], params=par)      # (warm: buffers, code objects)
    t = time.perf_counter()
    out5, iters = EV.qc_scale_sweep(dev, p["qc"], thetas, p["pose"], p["vel"], p["landmarks"], params=par)
    sweep_s = time.perf_counter() - t
    k = int(np.argmax(out5[:, 0]))
    t = time.perf_counter()
    out = EV.learn_qc(dev, 10.0 * p["qc"], p["pose"], p["vel"], p["landmarks"], params=par, steps=50, rtol=1e-3, scale_only=True)
    learn_s = time.perf_counter() - t
    res = {"graph": "plaza2", "sweep_s": round(sweep_s, 3), "sweep_points": len(thetas), "sweep_iterations": int(iters.sum()),
           "sweep_theta": float(thetas[k]), "sweep_logZ": float(out5[k, 0]),
           "learn_s": round(learn_s, 3), "learn_steps": len(out), "learn_iterations": int(sum(o[2] for o in out)),
           "learn_theta": [round(float(o[0][0, 0] / p["qc"][0, 0]), 5) for o in out], "learn_logZ": [o[1] for o in out]}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graphs", default="100000,1000000,plaza2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child (kernel times)")
    ap.add_argument("--learn", action="store_true", help="Plaza2: learn_qc(scale_only=True) against qc_scale_sweep")
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
