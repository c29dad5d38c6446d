#!/usr/bin/env python3
"""What the statistics of dense posterior draws cost when they are reduced on the device (gpslam_hip_sample_posterior_stats; DESIGN.md
section 4o) next to today's route -- gpslam_hip_sample_posterior_at with query_poses copied to the host -- in the same process.

Graphs, query densities and the slope are scripts/bench_sampling_dense.py's: Plaza2 and the SE(3) chain at 1e5 and 1e6 states; 1, 4 and
16 queries in every interval; wall clock per draw as the slope between a call of 1 draw and a call of 1 + K draws on a warmed
handle, the fastest of --reps each.  The four variants of a combination share one handle and alternate inside every repetition:

  stats_all     the stats call with s1 / s2, hits, clearance and length asked for
  stats_hits    the stats call with hits and clearance only
  dense         sample_posterior_at with nothing of the queries copied (the draws themselves)
  to_host       sample_posterior_at with query_poses copied to pageable host memory (the yardstick; null where 4 GB of host buffer
                hold fewer than two draws)

Obstacles: eight spheres of radius 0.5 beside the estimate's path (a centre one radius off every N / 8-th state).
moments_bytes / paths_bytes: what k_ps_moments and k_ps_paths move in a launch over ONE draw, from the shapes -- per query the pose
read, the sums read and written (2 (d + d (d + 1) / 2) doubles; 2 (that + 1) with the count), q^ read, two slab entries written;
then the two slab entries read again and two numbers per draw written.  (The next query's position is a neighbour's pose: counted
once.)  With `hits` and `clearance` only: pose, count, one slab entry.

--child GRAPH:PER[:hits] runs five stats draws in calls of one draw and nothing else: the command scripts/kernel_times.sh wraps;
--trace-table DIR is bench_sampling_dense.py's table of the trace it left.
  timeout -k 10 200 bash scripts/kernel_times.sh stats timeout -k 10 180 python scripts/bench_sampling_stats.py --child 1000000:4 &&
  python scripts/bench_sampling_stats.py --trace-table /tmp/kt_stats
Run every graph as a step of its own under a limit sized to it, the steps chained with &&."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_sampling_dense import DP, IP, Dense, interval_dt, problem, queries, trace_table      # noqa: E402
from gpslam_amd import chain                 # noqa: E402

LP = C.POINTER(C.c_int64)
EXTRA = {"plaza2": 32, "100000": 8, "1000000": 6}


def obstacles(p, dev):
    pose = np.asarray(p["pose"], dtype=np.float64)
    pos = pose[:, 9:12] if dev.pd == 12 else pose[:, :2]
    at = pos[np.linspace(0, len(pos) - 1, 8).astype(int)].copy()
    at[:, 0] += 0.5
    return np.ascontiguousarray(np.concatenate([at, np.full((8, 1), 0.5)], axis=1))


class Stats:
    """sample_posterior_stats through the C entry point, into buffers allocated once"""
    def __init__(self, dev, q, ob, everything, most):
        self.dev, self.lib, self.q, self.ob, self.all = dev, chain._sampling_stats_lib(), q, ob, everything
        nq, d = len(q[0]), dev.d
        self.s1, self.s2, self.hits = np.zeros(nq * d), np.zeros(nq * d * (d + 1) // 2), np.zeros(nq, dtype=np.int64)
        self.clear, self.len, self.n = np.zeros(most), np.zeros(most), C.c_int64(0)

    def __call__(self, count, seed=1):
        left, dt, tau = self.q
        on = lambda a: a.ctypes.data_as(DP) if self.all else None
        rc = self.lib.gpslam_hip_sample_posterior_stats(self.dev._h, count, seed, 0, None, len(left), left.ctypes.data_as(IP), dt.ctypes.data_as(DP),
                                                        tau.ctypes.data_as(DP), len(self.ob), self.ob.ctypes.data_as(DP), 0.05, 0, C.byref(self.n),
                                                        on(self.s1), on(self.s2), self.hits.ctypes.data_as(LP), self.clear.ctypes.data_as(DP), on(self.len))
        self.dev._chk(rc, "sample_posterior_stats")


def clock(draw, count):
    t = time.perf_counter()
    draw(count)
    return 1e3 * (time.perf_counter() - t)


def measure(which, pers, reps):
    p, build = problem(which)
    dev = build()
    dts = interval_dt(p)
    ob = obstacles(p, dev)
    for per in pers:
        q = queries(dts, per)
        nq, d, pd = len(q[0]), dev.d, dev.pd
        tri = d * (d + 1) // 2
        most_host = int(4e9 / (8.0 * nq * pd))                      # draws whose query poses 4 GB of host buffer hold
        variants = {"stats_all": (Stats(dev, q, ob, True, 1025), 1024), "stats_hits": (Stats(dev, q, ob, False, 1025), 1024),
                    "dense": (Dense(dev, q, False, 1025), 1024)}
        if most_host >= 2:
            variants["to_host"] = (Dense(dev, q, True, min(most_host, 1025)), min(most_host, 1025) - 1)
        K = {}
        for name, (draw, most) in variants.items():                 # warmed, and K sized as bench_sampling_dense.slope sizes it
            draw(1)
            t1 = clock(draw, 1)
            k0 = min(EXTRA.get(which, 4), most)
            per_draw = max((clock(draw, 1 + k0) - t1) / k0, 1e-3)
            K[name] = int(min(max(k0, 4.0 * t1 / per_draw), most))
        one, many = {n: [] for n in variants}, {n: [] for n in variants}
        for _ in range(reps):
            for name, (draw, _) in variants.items():                # alternating
                one[name].append(clock(draw, 1))
                many[name].append(clock(draw, 1 + K[name]))
        res = {"graph": which, "states": dev.N, "per_interval": per, "queries": nq, "obstacles": len(ob), "draw_ms": {}, "call_ms": {}, "draws_between": K}
        for name in ("stats_all", "stats_hits", "dense", "to_host"):
            if name not in variants:
                res["draw_ms"][name] = None
                continue
            extra = min(many[name]) - min(one[name])
            res["draw_ms"][name] = round(extra / K[name], 4) if extra >= min(one[name]) else None      # (bench_sampling_dense.slope's rule)
            res["call_ms"][name] = round(min(one[name]) - extra / K[name], 4)
        res["query_poses_mb"] = round(8e-6 * nq * pd, 1)
        res["moments_bytes"] = {"all": 8 * nq * (2 * pd + 2 * (d + tri + 1) + 2), "hits": 8 * nq * (pd + 2 + 1)}
        res["paths_bytes"] = {"all": 8 * (2 * nq + 2), "hits": 8 * (nq + 1)}
        print(json.dumps(res), flush=True)
    dev.close()


def child(spec):
    parts = spec.split(":")
    p, build = problem(parts[0])
    dev = build()
    draw = Stats(dev, queries(interval_dt(p), int(parts[1])), obstacles(p, dev), len(parts) < 3, 4)
    for _ in range(5):
        draw(1)
    dev.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graphs", default="plaza2,100000,1000000")
    ap.add_argument("--per", default="1,4,16", help="queries per interval")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default="", help="GRAPH:PER[:hits] -- five stats draws in calls of one and nothing else, for a kernel trace")
    ap.add_argument("--trace-table", default="", help="DIR -- print the per-kernel table of the kernel trace found under DIR")
    a = ap.parse_args()
    if a.trace_table:
        trace_table(a.trace_table)
        return
    if a.child:
        child(a.child)
        return
    for which in a.graphs.split(","):
        measure(which, [int(v) for v in a.per.split(",")], a.reps)


if __name__ == "__main__":
    main()
