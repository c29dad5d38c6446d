"""Pair marginals and the closure gate on the device: first measurements (they set no target).

  (1) 1e5 SE(3) states (no landmarks, no closures: no opt-in needed).  After one gpslam_hip_marginals(): get_state_pair_marginals
      for 1, 256 and 4096 random pairs and gate_between_pairs for as many candidates -- wall clock of the whole call (uploads, kernels,
      the copy back, the stream drained), median of --reps after a warm-up.
  (2) 1e5 SE(2) states with 8 planar landmarks (16 border columns): gpslam_hip_marginals() with and without
      marginals_keep_pair_terms (the copy of Y, N * b * m doubles), median of --reps, and the pair getter there (it adds Y_a K Y_b^T).
Prints one JSON line.

The kernels' own durations come from a run of their own under the profiler, which slows the host:
    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python scripts/bench_pair_marginals.py --reps 3
    python scripts/bench_pair_marginals.py --kernel-times DIR
prints, per kernel of marginals_pairs.hip and grid size (k_mg_pair: one workgroup per pair), calls and the mean / min duration."""
import argparse
import collections
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COUNTS = (1, 256, 4096)
KERNELS = ("k_mg_pair_finish", "k_mg_pair", "k_mg_gate", "k_mg_keep_y")


def median_ms(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def relative_pose3(x1, x2):
    """x1^-1 x2 for poses stored (R row-major, t), batched"""
    R1, R2 = x1[:, :9].reshape(-1, 3, 3), x2[:, :9].reshape(-1, 3, 3)
    R = np.einsum("nji,njk->nik", R1, R2)
    t = np.einsum("nji,nj->ni", R1, x2[:, 9:] - x1[:, 9:])
    return np.concatenate([R.reshape(-1, 9), t], axis=1)


def random_pairs(N, count, rng):
    a = rng.integers(0, N, count).astype(np.int32)
    b = rng.integers(0, N, count).astype(np.int32)
    b[a == b] = (a[a == b] + N // 2) % N
    return a, b


def measure(reps):
    import gpslam_amd as gp
    from gpslam_amd import synthetic as S
    N = 100000
    out = dict(bench="pair_marginals", N=N, reps=reps)
    p = S.pose3_chain(N)
    dev = S.apply(p, gp.ChainSolver(p["kind"]))
    dev.iterate_gn()
    out["pose3_marginals_ms"] = median_ms(dev.marginals, reps)
    pose, _ = dev.get_states()
    rng = np.random.default_rng(0)
    rows = []
    for count in COUNTS:
        a, b = random_pairs(N, count, rng)
        meas = relative_pose3(pose[a], pose[b])
        sig = np.full((count, 6), 0.05)
        rows.append(dict(count=count, mean_distance=float(np.mean(np.abs(a.astype(np.int64) - b))),
                         pairs_ms=median_ms(lambda: dev.get_state_pair_marginals(a, b), reps),
                         gate_ms=median_ms(lambda: dev.gate_between_pairs(a, b, meas, sig), reps)))
    out["pose3_1e5"] = rows
    dev.close()

    q = dict(S.pose2_range_chain(N, L=8, seed=1))
    q["prior_sig"] = np.full_like(q["prior_sig"], 1e-3)
    lm = S.apply(q, gp.ChainSolver(q["kind"], landmark_dim=2))
    lm.iterate_gn()
    m = lm.plan_info()["R"] - 1
    res = dict(N=N, border_columns=m, segmented=bool(lm.segment_plan()["active"]), kept_bytes=N * lm.b * m * 8)
    res["marginals_ms"] = median_ms(lm.marginals, reps)
    lm.marginals_keep_pair_terms()
    res["marginals_keep_ms"] = median_ms(lm.marginals, reps)
    a, b = random_pairs(N, 4096, rng)
    res["pairs_4096_ms"] = median_ms(lambda: lm.get_state_pair_marginals(a, b), reps)
    lm.marginals_keep_pair_terms(False)
    res["marginals_again_ms"] = median_ms(lm.marginals, reps)
    out["pose2_landmarks_1e5"] = res
    lm.close()
    print(json.dumps(out))


def kernel_times(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        sys.exit("no kernel trace under " + d)
    agg = collections.defaultdict(list)
    with open(f[0]) as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"]
            k = next((k for k in KERNELS if k in name), None)
            if k is None:
                continue
            tmpl = name[name.find(k) + len(k):].split("(")[0]
            agg[(k + tmpl, int(r.get("Grid_Size_X", r.get("Grid_Size", 0))))].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for (k, grid), v in sorted(agg.items()):
        print("  %-28s grid %8d  calls %4d  mean %9.1f us  min %9.1f us" % (k, grid, len(v), sum(v) / len(v) / 1e3, min(v) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-times", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.kernel_times:
        kernel_times(a.kernel_times)
    else:
        measure(a.reps)


if __name__ == "__main__":
    main()
