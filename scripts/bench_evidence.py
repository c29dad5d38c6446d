#!/usr/bin/env python3
"""What log det H costs (gpslam_hip_log_determinant) next to gpslam_hip_marginals, which computes the same pivots,
keeps 5 b^2 doubles per state and sweeps back down.

Graphs: BASELINE config 3 (SE(3) GP chain with odometry) at 1e5 and 1e6 states, and Plaza2 (4091 SE(2) states, interpolated ranges, 4
landmarks; tests/golden/plaza2.npz).  Per graph, one JSON line:

  logdet_ms, marginals_ms     wall clock of ChainSolver.log_determinant() / .marginals() on WARMED handles (the call ran once before: its
                              buffers exist, the code objects are loaded), every call ending in its own synchronisation; medians over
                              --reps handles, the two calls alternating on the same handle
  logdet_bytes, marginals_bytes   device memory the first call of either reserves on a fresh handle (hipMemGetInfo before and after)
  kernels_us                  from a rocprofv3 --kernel-trace run of a child process (--trace-child) that makes --reps calls of each:
                              [median, minimum] over the level-0 launches of k_ev_forward and of k_mg_forward (the launches whose grid
                              is ceil(N / 16) workgroups: both read the same records), and of the whole log_determinant's kernels
  l0_record_bytes, ev_l0_gbs  the bytes of D and O the level-0 launch reads (N 2 b^2 8) over its median time

k_mg_forward is the parent commit's, byte for byte (scripts/compare_device_code.py), so the comparison is against the parent's kernel.
Run every graph as a step of its own under a limit sized to it, the steps chained so that none starts behind one that failed:
  timeout -k 10 240 python scripts/bench_evidence.py --graphs plaza2 && timeout -k 10 300 python scripts/bench_evidence.py --graphs 100000 &&
  timeout -k 10 540 python scripts/bench_evidence.py --graphs 1000000 --reps 5"""
import argparse
import csv
import ctypes as C
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpslam_amd as gp                      # noqa: E402
from gpslam_amd import synthetic as S        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(which):
    """a function that returns a fresh compiled handle of the graph"""
    if which == "plaza2":
        from gpslam_amd import plaza
        p = plaza.build_problem(plaza.load(os.path.join(ROOT, "tests", "golden", "plaza2.npz")))
        return lambda: plaza.apply(p, gp.ChainSolver(gp.POSE2, chart=gp.CHART_FIRST_ORDER, landmark_dim=2))
    p = S.pose3_chain(int(which))
    return lambda: S.apply(p, gp.ChainSolver(gp.POSE3))


def free_bytes():
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert gp.load_library().hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def reserved(fresh, call):
    dev = fresh()
    dev.error()
    before = free_bytes()
    call(dev)
    after = free_bytes()
    dev.close()
    return before - after


def timed_pair(fresh, reps):
    """medians of log_determinant and marginals, alternating on warmed handles"""
    a, b, out = [], [], None
    for _ in range(reps):
        dev = fresh()
        dev.log_determinant()
        dev.marginals()
        dev.error()
        for _ in range(3):
            t = time.perf_counter()
            out = dev.log_determinant()
            a.append(1e3 * (time.perf_counter() - t))
            t = time.perf_counter()
            dev.marginals()
            b.append(1e3 * (time.perf_counter() - t))
        dev.close()
    return statistics.median(a), statistics.median(b), out


def trace_child(which, reps):
    fresh = make(which)
    dev = fresh()
    for _ in range(reps + 1):
        dev.log_determinant()
        dev.marginals()
    dev.close()


def kernel_us(which, reps, l0_grid):
    tmp = tempfile.mkdtemp(prefix="evidence_trace_")
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

    def grid(r):
        for key in ("Grid_Size", "Grid_Size_X"):
            if key in r:
                return int(r[key])
        return -1

    out = {}
    for name in ("k_ev_forward", "k_mg_forward"):
        mine = [r for r in rows if name in r["Kernel_Name"]]
        l0 = [dur(r) for r in mine if grid(r) == l0_grid * 64]
        if not l0 and mine:          # (no grid column: per call the longest launch is level 0's)
            l0 = sorted(dur(r) for r in mine)[-(reps + 1):]
        l0 = l0[1:] if len(l0) > 1 else l0       # (the first launch loads the code object)
        if l0:
            out[name + "_level0"] = [round(statistics.median(l0), 2), round(min(l0), 2)]
    for name in ("k_ev_top", "k_ev_core", "k_ev_reduce"):
        d = [dur(r) for r in rows if name in r["Kernel_Name"]]
        if d:
            out[name] = [round(statistics.median(d), 2), round(min(d), 2)]
    return out


def measure(which, reps, trace):
    fresh = make(which)
    probe = fresh()
    N, b, R = probe.N, probe.b, probe.plan_info()["R"]
    probe.close()
    res = {"graph": which, "states": N, "block": b, "rhs_columns": R}
    res["logdet_bytes"] = reserved(fresh, lambda d: d.log_determinant())
    res["marginals_bytes"] = reserved(fresh, lambda d: d.marginals())
    res["logdet_ms"], res["marginals_ms"], res["logdet"] = timed_pair(fresh, reps)
    if trace:
        k = kernel_us(which, max(3, reps), (N + 15) // 16)
        res["kernels_us"] = k
        if "k_ev_forward_level0" in k:
            nbytes = N * 2 * b * b * 8
            res["l0_record_bytes"] = nbytes
            res["ev_l0_gbs"] = round(nbytes / (k["k_ev_forward_level0"][0] * 1e-6) / 1e9, 1)
    for key, v in list(res.items()):
        if isinstance(v, float):
            res[key] = round(v, 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graphs", default="100000,1000000,plaza2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child (kernel times)")
    ap.add_argument("--trace-child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        trace_child(a.trace_child, a.reps)
        return
    for which in a.graphs.split(","):
        print(json.dumps(measure(which, a.reps, not a.no_trace)), flush=True)


if __name__ == "__main__":
    main()
