"""gtsam::Marginals on the device: gpslam_hip_marginals time (median of 10 after a warm-up) beside the same handle's Gauss-Newton
iteration, interpolate_covariances for a batch of queries (median of 10), and the selected inversion's algorithmic HBM bytes with
the fraction of the HBM peak they reach in the time of the whole call.  Prints one JSON line.
  --only pose3_1e6   one case (e.g. under rocprofv3 --kernel-trace --stats)"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(CASES), default=None)
    a = ap.parse_args()
    names = [a.only] if a.only else ["pose3_1e5", "pose3_1e6", "linear3_1e6", "plaza2"]
    print(json.dumps(dict(bench="marginals", hbm_peak_gbs=HBM_PEAK_GBS, results=[CASES[n]() for n in names])))


if __name__ == "__main__":
    main()
