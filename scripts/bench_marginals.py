"""gtsam::Marginals on the device: gpslam_hip_marginals time (median of 10 after a warm-up) beside the same handle's Gauss-Newton
iteration, interpolate_covariances for a batch of queries (median of 10), and the selected inversion's algorithmic HBM bytes with
the fraction of the HBM peak they reach in the time of the whole call.  Prints one JSON line.
  --only pose3_1e6   one case (e.g. under rocprofv3 --kernel-trace --stats)
  --closures         the loop-closure cases instead: 1e5-state chains, SE(3) with 4 (one pass: the control) / 8 / 20 closures, SE(2)
                     with 9 (control) / 18 / 40; beyond one pass the handle keeps the closures' columns at every state
                     (marginals_keep_closure_columns) and the closure term runs on the matrix cores (k_mg_clo_finish).  The yardsticks
                     are the control rows and the same handle's Gauss-Newton iteration, which is already P + 1 chain solves.
                     clo_finish_madds: multiply-adds of k_mg_clo_finish as it runs them (padded tiles, band and off-band), to set
                     against its time in a kernel trace and the 78.6 TFLOP/s fp64 matrix peak."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpslam_amd as gp                      # noqa: E402
from gpslam_amd import plaza                 # noqa: E402
from gpslam_amd import synthetic as S        # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak, as bench.py


def algorithmic_bytes(N, b):
    """HBM bytes of the selected inversion at level 0 (the levels above add 1 / 15 of it): read D and O of the records (2 b^2),
    write and read back [P^-1 | U | V] (3 b^2 each way), write Sigma_{i,i} and Sigma_{i,i+1} (2 b^2); fp64"""
    return int(N * 10 * b * b * 8 * 16 / 15)


def median_ms(f, reps=10):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def case(name, p, queries=0, dev=None):
    dev = dev or S.apply(p, gp.ChainSolver(p["kind"]))
    dev.iterate_gn()
    out = dict(case=name, N=int(dev.N), marginals_ms=median_ms(dev.marginals))
    out["algorithmic_bytes"] = algorithmic_bytes(dev.N, dev.b)
    out["hbm_frac"] = out["algorithmic_bytes"] / (out["marginals_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS
    st, t = dev.run_gn(10, timed=True)
    out["gn_iter_ms"] = float(t[4]) / 10
    if queries:
        dev.marginals()
        rng = np.random.default_rng(0)
        left = rng.integers(0, dev.N - 1, queries).astype(np.int32)
        dt = np.full(queries, 0.1)
        tau = rng.uniform(0.0, 0.1, queries)
        out["interp_cov_ms"] = median_ms(lambda: dev.interpolate_covariances(left, dt, tau))
        out["queries"] = queries
    dev.close()
    return out


def closure_pairs(N, K, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < K:
        i, j = (int(v) for v in rng.integers(0, N, 2))
        if abs(i - j) > 1:
            out.append([i, j])
    return out


def pose2_chain(N):
    p = S.pose2_range_chain(N, seed=9)
    p = {k: v for k, v in p.items() if not (k.startswith("range_") or k.startswith("lprior") or k.startswith("landmark"))}
    p["prior_sig"] = np.full_like(p["prior_sig"], 1e-3)
    return p


def clo_finish_madds(N, b, nc):
    """k_mg_clo_finish: groups of 48 rows, three row tiles each; per row tile nt^2 * 4 MFMAs for T (nt = ceil(nc / 16)) and nt * 4
    per column tile of the band (three of four, SE(2)'s first row tile two); 1024 multiply-adds per v_mfma_f64_16x16x4_f64"""
    nt = -(-nc // 16)
    groups = -(-N * b // 48)
    band = 9 if b == 12 else 8
    return groups * (3 * nt * nt * 4 + band * nt * 4) * 1024


def closure_case(kind, K, N=100000):
    base = S.pose3_chain(N, seed=2) if kind == "pose3" else pose2_chain(N)
    p = S.add_loop_closures(base, closure_pairs(N, K, 100 + K), seed=3)
    dev = gp.ChainSolver(p["kind"])
    dev.set_closure_passes(32)
    S.apply(p, dev)
    dev.marginals_keep_closure_columns()
    info = dev.closure_info()
    dev.iterate_gn()
    out = dict(case="%s_1e5_clo%d" % (kind, K), N=int(dev.N), closures=K, passes=info["passes"], solves=info["solves"],
               marginals_ms=median_ms(dev.marginals))
    t = []
    for it in range(12):
        dev.set_states(p["pose"], p["vel"])
        rc, st = dev.iterate_gn()
        assert rc == 0
        if it >= 2:
            t.append(dev.last_timing()[4])
    out["gn_iter_ms"] = float(np.median(t))
    out["ratio"] = out["marginals_ms"] / out["gn_iter_ms"]
    if info["passes"] > 1:
        out["clo_finish_madds"] = clo_finish_madds(dev.N, dev.b, K * dev.d)
    dev.close()
    return out


def plaza2():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = plaza.build_problem(plaza.load(os.path.join(root, "tests", "golden", "plaza2.npz")))
    return case("plaza2", None, dev=plaza.apply(p, gp.ChainSolver(gp.POSE2, chart=gp.CHART_FIRST_ORDER, landmark_dim=2)))


CASES = {
    "pose3_1e5": lambda: case("pose3_1e5", S.pose3_chain(100000), queries=100000),
    "pose3_1e6": lambda: case("pose3_1e6", S.pose3_chain(1000000), queries=1000000),
    "linear3_1e6": lambda: case("linear3_1e6", S.linear_chain(1000000, D=3)),
    "plaza2": plaza2,
}
CLOSURE_CASES = [("pose3", 4), ("pose3", 8), ("pose3", 20), ("pose2", 9), ("pose2", 18), ("pose2", 40)]
for _kind, _K in CLOSURE_CASES:
    CASES["%s_1e5_clo%d" % (_kind, _K)] = (lambda kind=_kind, K=_K: closure_case(kind, K))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(CASES), default=None)
    ap.add_argument("--closures", action="store_true")
    a = ap.parse_args()
    names = ["%s_1e5_clo%d" % c for c in CLOSURE_CASES] if a.closures else ["pose3_1e5", "pose3_1e6", "linear3_1e6", "plaza2"]
    if a.only:
        names = [a.only]
    print(json.dumps(dict(bench="marginals", hbm_peak_gbs=HBM_PEAK_GBS, results=[CASES[n]() for n in names])))


if __name__ == "__main__":
    main()
