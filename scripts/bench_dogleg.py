#!/usr/bin/env python3
"""Powell's dogleg against Levenberg-Marquardt: what an iteration and what a FURTHER trial costs.

Graphs: BASELINE config 3 (SE(3) GP chain with odometry, 1e5 states), the same chain at 1e6 states, and Plaza2 (4091 SE(2) states,
interpolated ranges, 4 landmarks; tests/golden/plaza2.npz).  Wall clock in ms, every call ends with a synchronisation; medians over
--reps handles.  Every handle is WARMED first: the call that is to be measured runs once untimed (the handle's buffers -- the state
backup, the dogleg's partial sums -- are allocated by a first call), the graph's initial states and landmarks are put back
(set_states / set_landmarks: no new compile), and the second call is the one that is timed, so every sample sees the same problem.

  dogleg_1        iterate_dogleg, ONE_STEP_PER_ITERATION, one trial
  dogleg_k        iterate_dogleg, SEARCH_EACH_ITERATION from a trust radius of 1e-3: k trials (the radius grows threefold per trial)
  dogleg_extra    (dogleg_k - dogleg_1) / (k - 1): a further trial = blend, retraction, error pass, one read of three scalars
  lm_1            iterate_lm at lambda = 1e-5, one trial, accepted
  lm_k            iterate_lm with min_model_fidelity = 2 (no trial can pass): k trials, up to lambda's bound, every one restored
  lm_extra        (lm_k - lm_1) / (k - 1): a further trial = assembly (unless fused), elimination, back-substitution, retraction, error pass
  gn_1            iterate_gn (the handle's own level-0 form), for scale
  kernels_us, quad_hbm_fraction   the dogleg's kernels' own times from a rocprofv3 --kernel-trace run of a child process (--trace-child)
                  that makes --reps iterate_dogleg calls: the MEDIAN over its launches (and the minimum beside it); the fraction of
                  --hbm-peak-gbs that k_dl_quad's record bytes (N (2 b^2 + b R) 8) come to at its median
Prints one JSON line per graph; profiles/dogleg.txt keeps a run.

The script sets no time limit on its own measurements (the trace child has one, and is killed with its whole process group).  Run
every graph as a step of its own under a limit sized to it, the steps chained so that none starts behind one that failed:
  timeout -k 10 240 python scripts/bench_dogleg.py --graphs plaza2 && timeout -k 10 300 python scripts/bench_dogleg.py --graphs 100000 &&
  timeout -k 10 540 python scripts/bench_dogleg.py --graphs 1000000 --reps 5"""
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


def sync(dev):
    dev.error()


def timed(fresh, call, reps):
    """median wall clock of call(handle) over warmed handles (module docstring), and what the last call returned"""
    ts, out = [], None
    for _ in range(reps):
        dev = fresh()
        pose, vel = dev.get_states()
        lm = dev.get_landmarks() if dev.L else None
        call(dev)
        dev.set_states(pose, vel)
        if lm is not None:
            dev.set_landmarks(lm)
        sync(dev)
        t = time.perf_counter()
        out = call(dev)
        ts.append(1e3 * (time.perf_counter() - t))
        dev.close()
    return statistics.median(ts), out


def trace_child(which, reps):
    fresh = make(which)
    for _ in range(reps):
        dev = fresh()
        dev.iterate_dogleg(1.0)
        dev.close()


def kernel_us(which, reps):
    """{kernel: [median, minimum] in us over the launches} of the dogleg's kernels from the kernel trace of a child process"""
    tmp = tempfile.mkdtemp(prefix="dogleg_trace_")
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
    out = {}
    for name in ("k_dl_quad", "k_dl_lm", "k_dl_blend"):
        dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if dur:
            out[name] = [round(statistics.median(dur), 2), round(min(dur), 2)]
    return out


def measure(which, reps, hbm_peak_gbs, trace):
    fresh = make(which)
    probe = fresh()
    N, b, R = probe.N, probe.b, probe.plan_info()["R"]
    fused = probe.plan_info()["fused"]
    probe.close()
    res = {"graph": which, "states": N, "block": b, "rhs_columns": R, "fused_level0": fused}
    res["gn_1"], _ = timed(fresh, lambda d: d.iterate_gn(), reps)
    t1, (st, _) = timed(fresh, lambda d: d.iterate_dogleg(1.0, gp.DOGLEG_ONE_STEP_PER_ITERATION), reps)
    res["dogleg_1"], res["dogleg_1_trials"], res["dogleg_1_accepted"] = t1, st.trials, st.accepted
    tk, (st, _) = timed(fresh, lambda d: d.iterate_dogleg(1e-3, gp.DOGLEG_SEARCH_EACH_ITERATION), reps)
    res["dogleg_k"], res["dogleg_k_trials"] = tk, st.trials
    res["dogleg_extra"] = (tk - t1) / (st.trials - 1) if st.trials > 1 else None

    def lm(d, fidelity):
        return d.iterate_lm(1e-5, d.default_params(use_lm=1, min_model_fidelity=fidelity))
    l1, (_, st, _) = timed(fresh, lambda d: lm(d, 1e-3), reps)
    res["lm_1"], res["lm_1_trials"], res["lm_1_accepted"] = l1, st.trials, st.accepted
    lk, (_, st, _) = timed(fresh, lambda d: lm(d, 2.0), reps)
    res["lm_k"], res["lm_k_trials"] = lk, st.trials
    res["lm_extra"] = (lk - l1) / (st.trials - 1) if st.trials > 1 else None
    if trace:
        k = kernel_us(which, max(3, reps // 2))
        res["kernels_us"] = k
        if "k_dl_quad" in k:
            nbytes = N * (2 * b * b + b * R) * 8
            res["quad_record_bytes"] = nbytes
            res["quad_gbs"] = round(nbytes / (k["k_dl_quad"][0] * 1e-6) / 1e9, 1)
            res["quad_hbm_fraction"] = round(res["quad_gbs"] / hbm_peak_gbs, 3)
    for key, v in list(res.items()):
        if isinstance(v, float):
            res[key] = round(v, 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graphs", default="100000,1000000,plaza2")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--hbm-peak-gbs", type=float, default=8000.0, help="the HBM roof the fraction is taken of (MI355X: 8 TB/s)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child (kernel times)")
    ap.add_argument("--trace-child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        trace_child(a.trace_child, a.reps)
        return
    for which in a.graphs.split(","):
        print(json.dumps(measure(which, a.reps, a.hbm_peak_gbs, not a.no_trace)), flush=True)


if __name__ == "__main__":
    main()
