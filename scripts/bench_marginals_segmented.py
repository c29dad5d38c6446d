"""gtsam::Marginals on the segmented landmark path (gpslam_hip_marginals_on_segments): BASELINE config 4 -- 1e6 SE(2) states, N / 20
locally visible range landmarks -- and twice its landmark density where the fat blocks stay within 64 columns.  Per case: the
marginals() wall clock (median of 10 behind two untimed calls), the Gauss-Newton iteration of the same handle
(gpslam_hip_last_timing) and their ratio; the multiply-adds k_mg_fs_finish issues (padded tiles, band and off-band) and the bytes
k_mg_fs_walk moves (|fac| + 2 |Y|), to set against their times in a kernel trace, the 78.6 TFLOP/s fp64 matrix peak and the HBM
peak.  Prints one JSON line.
  --n 1000000       states
  --only c4|c4x2    one case (e.g. under rocprofv3 --kernel-trace --stats, in a run of its own)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpslam_amd as gp                      # noqa: E402
from gpslam_amd import synthetic as S        # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E peak, as bench.py
FP64_MATRIX_PEAK_TFLOPS = 78.6
MAX_NB = 64                    # kMgFsMaxNB


def finish_madds(cuts, b, NB):
    """k_mg_fs_finish: per segment groups of 48 rows, three row tiles each; per row tile nt^2 * 4 MFMAs for T (nt = ceil(2 NB / 16))
    and nt * 4 per column tile of the band (8 of 12 per group at block size 4 and 6, 9 at 12); 1024 multiply-adds per MFMA"""
    nt = -(-2 * NB // 16)
    band = 9 if b == 12 else 8
    groups = sum(-(-(c1 - c0 - 1) * b // 48) for c0, c1 in zip(cuts[:-1], cuts[1:]) if c1 - c0 > 1)
    return groups * (3 * nt * nt * 4 + band * nt * 4) * 1024


def make_cuts(N, C):
    c = list(range(0, N - 1, C))
    if c[-1] != N - 1:
        c.append(N - 1)
    if len(c) >= 3 and c[-1] - c[-2] < 2:
        del c[-2]
    return c


def case(name, N, density):
    p = S.pose2_local_landmarks_chain(N, L=max(int(density * N / 20), 1))
    dev = S.apply(p, gp.ChainSolver(p["kind"], chart=gp.CHART_FIRST_ORDER, landmark_dim=2))
    plan = dev.segment_plan()
    out = dict(case=name, N=int(dev.N), L=int(dev.L), plan=plan)
    if not plan["active"] or plan["NB"] > MAX_NB:
        out["skipped"] = "NB %d beyond %d" % (plan["NB"], MAX_NB)
        dev.close()
        return out
    dev.run_gn(3)
    dev.marginals_on_segments()
    dev.marginals()
    dev.marginals()
    t = []
    for _ in range(10):
        t0 = time.perf_counter()
        dev.marginals()
        t.append((time.perf_counter() - t0) * 1e3)
    out["marginals_ms"] = float(np.median(t))
    out["marginals_ms_min_max"] = [float(min(t)), float(max(t))]
    ti = []
    for it in range(12):
        dev.set_states(p["pose"], p["vel"])
        dev.set_landmarks(p["landmarks"])
        rc, st = dev.iterate_gn()
        assert rc == 0
        if it >= 2:
            ti.append(dev.last_timing()[4])
    out["gn_iter_ms"] = float(np.median(ti))
    out["ratio"] = out["marginals_ms"] / out["gn_iter_ms"]
    b = dev.b
    out["finish_madds"] = finish_madds(make_cuts(N, plan["C"]), b, plan["NB"])
    out["walk_bytes"] = int(N) * (2 * b * b + 2 * b * plan["NCP"]) * 8
    out["G_bytes"] = (int(N) * b + 64) * plan["NCP"] * 8
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--only", choices=["c4", "c4x2"], default=None)
    a = ap.parse_args()
    cases = [("c4", 1.0), ("c4x2", 2.0)]
    res = [case(n, a.n, d) for n, d in cases if a.only in (None, n)]
    print(json.dumps(dict(bench="marginals_segmented", hbm_peak_gbs=HBM_PEAK_GBS, fp64_matrix_peak_tflops=FP64_MATRIX_PEAK_TFLOPS, results=res)))


if __name__ == "__main__":
    main()
