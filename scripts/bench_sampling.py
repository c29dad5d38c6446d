#!/usr/bin/env python3
"""What one posterior draw costs (gpslam_hip_sample_posterior) next to one Gauss-Newton iteration of a
GPSLAM_PLAN_UNFUSED_LEVEL0 twin -- existing code, the yardstick: a draw is that iteration's assembly and solve without its
linearisation, plus k_ps_place in front and k_ps_emit behind.

Graphs: Plaza2 (4091 SE(2) states, interpolated ranges, 4 landmarks; tests/golden/plaza2.npz) and BASELINE config 3 (SE(3) GP chain
with odometry) at 1e5 and 1e6 states.  Per graph, one JSON line:

  draw_ms           wall clock per draw, the slope between a call of 1 draw and a call of 1 + K draws on a warmed handle (medians over
                    --reps pairs), for three sets of outputs: "solve" (only the landmarks are asked for: no slab but theirs is written
                    or copied), "delta" (the tangent draw: N b + nl doubles to the host per draw), "all" (delta, poses, velocities,
                    landmarks: what ChainSolver.sample_posterior returns)
  call_ms           what a call costs besides its draws ("solve" outputs): the linearisation, saving and restoring the tables' errors,
                    the synchronisations
  gn_ms             wall clock of one iterate_gn() of the unfused twin, in the same process (median)
  trace             from a rocprofv3 --kernel-trace run of a child process: per draw (k_ps_place .. k_ps_emit) and per twin iteration the
                    number of launches, the sum of the kernels' times and the span from the first kernel's start to the last one's end
                    (medians, microseconds), and the draw's time by kernel

Run every graph as a step of its own under a limit sized to it, the steps chained so that none starts behind one that failed.
--budget says what that limit is: the rocprofv3 child runs in a session of its own, so it gets what is left of the budget less a
margin and is killed by this process, which an outer limit that fired first could not do.
  timeout -k 10 240 python scripts/bench_sampling.py --graphs plaza2 --budget 220 &&
  timeout -k 10 300 python scripts/bench_sampling.py --graphs 100000 --budget 280 &&
  timeout -k 10 540 python scripts/bench_sampling.py --graphs 1000000 --reps 3 --budget 520"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
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
from gpslam_amd import chain                 # noqa: E402
from gpslam_amd import synthetic as S        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = {"plaza2": 64, "100000": 16, "1000000": 4}      # K: the draws between the two calls of a slope
DP = C.POINTER(C.c_double)


def make(which, **kw):
    """a function that returns a fresh compiled handle of the graph"""
    if which == "plaza2":
        from gpslam_amd import plaza
        p = plaza.build_problem(plaza.load(os.path.join(ROOT, "tests", "golden", "plaza2.npz")))
        return lambda: plaza.apply(p, gp.ChainSolver(gp.POSE2, chart=gp.CHART_FIRST_ORDER, landmark_dim=2, **kw))
    p = S.pose3_chain(int(which))
    return lambda: S.apply(p, gp.ChainSolver(gp.POSE3, **kw))


class Draws:
    """sample_posterior through the C entry point with a chosen set of outputs, into buffers allocated once"""
    def __init__(self, dev, outputs, most):
        self.dev, self.lib = dev, chain._sampling_lib()
        nl = dev.L * dev.ld
        width = {"delta": dev.N * dev.b + nl, "poses": dev.N * dev.pd, "vels": dev.N * dev.d, "landmarks": max(nl, 1)}
        self.buf = {k: (np.zeros(most * width[k]) if k in outputs else None) for k in width}

    def __call__(self, count, seed=1):
        p = [None if self.buf[k] is None else self.buf[k].ctypes.data_as(DP) for k in ("delta", "poses", "vels", "landmarks")]
        rc = self.lib.gpslam_hip_sample_posterior(self.dev._h, count, seed, 0, None, *p)
        self.dev._chk(rc, "sample_posterior")


OUTPUTS = {"solve": ("landmarks",), "delta": ("delta",), "all": ("delta", "poses", "vels", "landmarks")}


def slope(draw, K, reps):
    """(ms per draw, ms of a call besides its draws)"""
    draw(1 + K)       # warmed: the buffers exist, the code objects are loaded
    one, many = [], []
    for _ in range(reps):
        t = time.perf_counter()
        draw(1)
        one.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter()
        draw(1 + K)
        many.append(1e3 * (time.perf_counter() - t))
    per = (statistics.median(many) - statistics.median(one)) / K
    return per, statistics.median(one) - per


def trace_child(which, reps):
    """draws, then twin iterations with a k_ps_noise launch in front of, between and behind them as the marker"""
    dev = make(which)()
    draw = Draws(dev, OUTPUTS["delta"], 1 + reps)
    draw(1)
    draw(1 + reps)
    twin = make(which, plan=gp.PLAN_UNFUSED_LEVEL0)()
    twin.iterate_gn()
    for _ in range(reps):
        dev.posterior_noise(0, 0, 1)
        twin.iterate_gn()
    dev.posterior_noise(0, 0, 1)
    dev.close()
    twin.close()


def kernel_trace(which, reps, limit):
    tmp = tempfile.mkdtemp(prefix="sampling_trace_")
    try:
        child = subprocess.Popen(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                                  "--trace-child", which, "--reps", str(reps)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
        try:
            if child.wait(timeout=limit) != 0:
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

    def short(name):      # k_assemble_ghost of "void gps::k_assemble_ghost<double, 12, 4, double>(...)", demangled or not
        m = re.search(r"k_[a-z][a-z0-9_]*", name)
        return m.group(0) if m else name
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in rows)
    draws, cur = [], None
    for e in ev:
        if e[2] == "k_ps_place":
            cur = []
        if cur is not None:
            cur.append(e)
            if e[2] == "k_ps_emit":
                draws.append(cur)
                cur = None
    marks = [i for i, e in enumerate(ev) if e[2] == "k_ps_noise"]
    iters = [ev[a + 1:b] for a, b in zip(marks, marks[1:]) if b - a > 1 and not any(e[2].startswith("k_ps_") for e in ev[a + 1:b])]
    draws = draws[2:] if len(draws) > 2 else draws      # (the first call's draw and the second's first: code objects, buffers)

    def summary(groups):
        if not groups:
            return None
        return {"launches": statistics.median(len(g) for g in groups),
                "kernels_us": round(statistics.median(sum(e[1] - e[0] for e in g) for g in groups) / 1e3, 2),
                "span_us": round(statistics.median(g[-1][1] - g[0][0] for g in groups) / 1e3, 2)}
    out = {"draw": summary(draws), "gn_iteration": summary(iters)}
    if draws:
        names = sorted({e[2] for g in draws for e in g})
        by = {n: round(statistics.median(sum(e[1] - e[0] for e in g if e[2] == n) for g in draws) / 1e3, 2) for n in names}
        out["draw_by_kernel_us"] = dict(sorted(by.items(), key=lambda kv: -kv[1]))
    if iters:
        names = sorted({e[2] for g in iters for e in g})
        by = {n: round(statistics.median(sum(e[1] - e[0] for e in g if e[2] == n) for g in iters) / 1e3, 2) for n in names}
        out["gn_by_kernel_us"] = dict(sorted(by.items(), key=lambda kv: -kv[1]))
    return out


def measure(which, reps, trace, deadline):
    K = EXTRA.get(which, 8)
    dev = make(which)()
    res = {"graph": which, "states": dev.N, "block": dev.b, "n_noise": dev.posterior_noise_dim(), "draws_between": K, "draw_ms": {}}
    for mode, outs in OUTPUTS.items():
        per, fixed = slope(Draws(dev, outs, 1 + K), K, reps)
        print("%s %s: %.4f ms per draw" % (which, mode, per), file=sys.stderr, flush=True)
        res["draw_ms"][mode] = round(per, 4)
        if mode == "solve":
            res["call_ms"] = round(fixed, 4)
    dev.close()
    twin = make(which, plan=gp.PLAN_UNFUSED_LEVEL0)()
    twin.iterate_gn()
    t_gn = []
    for _ in range(max(reps, 5)):
        t = time.perf_counter()
        twin.iterate_gn()
        t_gn.append(1e3 * (time.perf_counter() - t))
    twin.close()
    res["gn_ms"] = round(statistics.median(t_gn), 4)
    res["draw_over_gn"] = round(res["draw_ms"]["solve"] / res["gn_ms"], 3)
    if trace:
        left = deadline - time.monotonic() - 15.0      # (the margin: killing the child's session and reading what it wrote)
        if left < 20.0:
            raise RuntimeError("%.0f s of the budget are left: no kernel trace is started" % max(left, 0.0))
        res["trace"] = kernel_trace(which, max(3, reps), left)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graphs", default="plaza2,100000,1000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget", type=float, default=220.0, help="seconds this command may take in all: the limit it runs under, less a little")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child (launch counts, kernel times)")
    ap.add_argument("--trace-child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        trace_child(a.trace_child, a.reps)
        return
    deadline = time.monotonic() + a.budget
    for which in a.graphs.split(","):
        print(json.dumps(measure(which, a.reps, not a.no_trace, deadline)), flush=True)


if __name__ == "__main__":
    main()
