#!/usr/bin/env python3
"""What a dense posterior draw costs (gpslam_hip_sample_posterior_at) next to a draw of the support states
alone (gpslam_hip_sample_posterior: existing code, the yardstick) in the same process.

Graphs: Plaza2 (4091 SE(2) states, interpolated ranges, 4 landmarks; tests/golden/plaza2.npz) and BASELINE config 3 (SE(3) GP chain
with odometry) at 1e5 and 1e6 states; 1, 4 and 16 queries in every interval, evenly spaced.  Per graph and query density one JSON
line:

  draw_ms         wall clock per draw, the slope between a call of 1 draw and a call of 1 + draws_between draws on a warmed handle
                  (the fastest of --reps each; draws_between is sized so that the extra draws take four times a call of one, and a
                  slope whose extra draws took less than a call of one is null): "support" (sample_posterior, only the landmarks asked for: nothing of
                  the states is written or copied), "dense" (sample_posterior_at, only the landmarks asked for: the bridge runs,
                  nothing of the queries is copied), "dense_to_host" (query_poses, query_poses_mb per draw, copied to the host)
  call_ms         a call of one draw less one draw: for the dense call the queries checked, the coefficient table made on the host
                  and uploaded, on top of the linearisation
  bridge_bytes    what k_ps_bridge moves per draw: two support states read per run, pose_dim doubles written per query, 2 d staged
                  normals and eleven coefficients read per query

--child GRAPH:PER runs five dense draws and nothing else: the command scripts/kernel_times.sh wraps for k_ps_bridge's own time;
--trace-table DIR prints every kernel of the trace that script left (its own table cuts the names of sampling.hip's kernels short):
  timeout -k 10 200 bash scripts/kernel_times.sh dense timeout -k 10 180 python scripts/bench_sampling_dense.py --child 1000000:4 &&
  python scripts/bench_sampling_dense.py --trace-table /tmp/kt_dense
Run every graph as a step of its own under a limit sized to it, the steps chained with &&."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpslam_amd as gp                      # noqa: E402
from gpslam_amd import chain                 # noqa: E402
from gpslam_amd import synthetic as S        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
EXTRA = {"plaza2": 32, "100000": 8, "1000000": 6}      # K: the draws between the two calls of a slope, at least (slope sizes them)


def problem(which):
    """(the graph's description, a function that puts it on a fresh compiled handle)"""
    if which == "plaza2":
        from gpslam_amd import plaza
        p = plaza.build_problem(plaza.load(os.path.join(ROOT, "tests", "golden", "plaza2.npz")))
        return p, lambda: plaza.apply(p, gp.ChainSolver(gp.POSE2, chart=gp.CHART_FIRST_ORDER, landmark_dim=2))
    p = S.pose3_chain(int(which))
    return p, lambda: S.apply(p, gp.ChainSolver(gp.POSE3))


def interval_dt(p):
    """the interval lengths the graph's GP priors carry, in chain order"""
    dt = np.zeros(len(p["gp_left"]))
    dt[np.asarray(p["gp_left"])] = p["gp_dt"]
    return dt


def queries(dts, per):
    n = len(dts)
    left = np.repeat(np.arange(n, dtype=np.int32), per)
    tau = (dts[:, None] * (np.arange(1, per + 1) / (per + 1.0))[None, :]).reshape(-1)
    return left, np.ascontiguousarray(dts[left]), np.ascontiguousarray(tau)


class Dense:
    """sample_posterior_at through the C entry point, into buffers allocated once"""
    def __init__(self, dev, q, to_host, most):
        self.dev, self.lib, self.q = dev, chain._sampling_at_lib(), q
        self.lm = np.zeros(max(dev.L * dev.ld, 1) * most)
        self.qp = np.zeros(most * len(q[0]) * dev.pd) if to_host else None

    def __call__(self, count, seed=1):
        left, dt, tau = self.q
        rc = self.lib.gpslam_hip_sample_posterior_at(self.dev._h, count, seed, 0, None, len(left), left.ctypes.data_as(IP), dt.ctypes.data_as(DP),
                                                     tau.ctypes.data_as(DP), None if self.qp is None else self.qp.ctypes.data_as(DP), None,
                                                     None, None, None, self.lm.ctypes.data_as(DP))
        self.dev._chk(rc, "sample_posterior_at")


class Support:
    def __init__(self, dev, most):
        self.dev, self.lib = dev, chain._sampling_lib()
        self.lm = np.zeros(max(dev.L * dev.ld, 1) * most)

    def __call__(self, count, seed=1):
        self.dev._chk(self.lib.gpslam_hip_sample_posterior(self.dev._h, count, seed, 0, None, None, None, None, self.lm.ctypes.data_as(DP)), "sample_posterior")


def slope(draw, K, reps, most=1024):
    """(ms per draw or None, ms of a call of one draw, the draws between the two calls).  A dense call spends tens to hundreds of ms
    on the host before its first draw (the coefficient table of millions of queries made and uploaded), and that share varies from
    call to call: the second call gets as many more draws as take four times a call of one (at least K, at most `most`), and a
    slope whose extra draws took less than a call of one is not reported."""
    draw(1)
    t = time.perf_counter()
    draw(1)
    t1 = 1e3 * (time.perf_counter() - t)
    t = time.perf_counter()
    draw(1 + K)       # warmed: the buffers exist, the code objects are loaded
    per = max((1e3 * (time.perf_counter() - t) - t1) / K, 1e-3)
    K = int(min(max(K, 4.0 * t1 / per), max(most, 1)))
    one, many = [], []
    for _ in range(reps):
        t = time.perf_counter()
        draw(1)
        one.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter()
        draw(1 + K)
        many.append(1e3 * (time.perf_counter() - t))
    extra = min(many) - min(one)
    return (extra / K if extra >= min(one) else None), min(one), K


def measure(which, pers, reps, to_host):
    K = EXTRA.get(which, 4)
    p, build = problem(which)
    dev = build()
    dts = interval_dt(p)
    support, support_one, _ = slope(Support(dev, 1 + 1024), K, reps)
    for per in pers:
        q = queries(dts, per)
        nq, d, pd = len(q[0]), dev.d, dev.pd
        res = {"graph": which, "states": dev.N, "per_interval": per, "queries": nq, "n_noise": dev.posterior_noise_dim(),
               "n_noise_at": dev.posterior_noise_dim_at(nq), "draw_ms": {"support": round(support, 4)}}
        dense, dense_one, Kd = slope(Dense(dev, q, False, 1 + 1024), K, reps)
        res["draws_between"] = Kd
        res["draw_ms"]["dense"] = None if dense is None else round(dense, 4)
        res["dense_over_support"] = None if dense is None else round(dense / support, 3)
        # a call besides its draws: the queries checked, the coefficient table made on the host and uploaded, the linearisation
        res["call_ms"] = {"support": round(support_one - support, 4), "dense": None if dense is None else round(dense_one - dense, 4)}
        if to_host:
            most = int(4e9 / (8.0 * nq * pd)) - 1      # (the host buffer holds the query poses of every draw of a call: 4 GB at most)
            if most >= 1:
                host, _, Kh = slope(Dense(dev, q, True, 1 + most), min(K, most), reps, most)
                res["draw_ms"]["dense_to_host"] = None if host is None else round(host, 4)
                res["draws_between_to_host"] = Kh
            res["query_poses_mb"] = round(8e-6 * nq * pd, 1)
        res["bridge_bytes"] = 8 * ((dev.N - 1) * 2 * (pd + d) + nq * (pd + 2 * d + 11))
        print(json.dumps(res), flush=True)
    dev.close()


def trace_table(path):
    """per kernel of a rocprofv3 kernel trace under `path` (scripts/kernel_times.sh leaves it in /tmp/kt_<tag>): calls and mean time"""
    import csv
    import glob
    import re
    agg = {}
    for f in glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"k_[a-z][a-z0-9_]*", r["Kernel_Name"])
            agg.setdefault(m.group(0) if m else r["Kernel_Name"][:40], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    print(json.dumps({"trace": path, "kernel_us": {k: [len(v), round(sum(v) / len(v) / 1e3, 1)] for k, v in sorted(agg.items(), key=lambda kv: -sum(kv[1]))}}))


def child(spec):
    which, per = spec.split(":")
    p, build = problem(which)
    dev = build()
    draw = Dense(dev, queries(interval_dt(p), int(per)), False, 4)
    draw(1)
    draw(4)
    dev.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graphs", default="plaza2,100000,1000000")
    ap.add_argument("--per", default="1,4,16", help="queries per interval")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the draws whose query poses are copied to the host")
    ap.add_argument("--child", default="", help="GRAPH:PER -- a few dense draws and nothing else, for a kernel trace")
    ap.add_argument("--trace-table", default="", help="DIR -- print the per-kernel table of the kernel trace found under DIR")
    a = ap.parse_args()
    if a.trace_table:
        trace_table(a.trace_table)
        return
    if a.child:
        child(a.child)
        return
    for which in a.graphs.split(","):
        measure(which, [int(v) for v in a.per.split(",")], a.reps, not a.no_host)


if __name__ == "__main__":
    main()
