"""ms per Gauss-Newton iteration against the number of loop closures, at 1e5 states: SE(3) with 0 / 4 / 8 / 20 closures, SE(2) (no
landmarks) with 0 / 9 / 18 / 40.  Beyond one border (SE(3): 4 closures, SE(2): 9) the closures go through the chain solver in column
passes (gpslam_hip_set_closure_passes): P passes over the slices and a final one, each a full forward /
backward sweep at the width of one border.  Per case: two untimed iterations, then the median over 10 of gpslam_hip_last_timing
(linearize, assemble, solve, retract + error, total; hipEvents on the handle's stream).  The states are reset in front of every
iteration, so each one is the same first step.  Prints a markdown table and one JSON line.
   python scripts/bench_closures.py [states]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401
import gpslam_amd
from gpslam_amd import synthetic as S

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100000


def pairs(K, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < K:
        i, j = (int(v) for v in rng.integers(0, N, 2))
        if abs(i - j) > 1:
            out.append([i, j])
    return out


def pose2():
    p = S.pose2_range_chain(N, seed=9)
    p = {k: v for k, v in p.items() if not (k.startswith("range_") or k.startswith("lprior") or k.startswith("landmark"))}
    p["prior_sig"] = np.full_like(p["prior_sig"], 1e-3)
    return p


rows = []
for name, base, counts in (("SE(3)", S.pose3_chain(N, seed=2), (0, 4, 8, 20)), ("SE(2)", pose2(), (0, 9, 18, 40))):
    for K in counts:
        p = S.add_loop_closures(base, pairs(K, 100 + K), seed=3) if K else base
        s = gpslam_amd.ChainSolver(p["kind"])
        multi = hasattr(s.lib, "gpslam_hip_set_closure_passes")     # (GPSLAM_LIB may name a build older than the column passes)
        if not multi and 1 + K * s.d > 28:
            continue
        if multi:
            s.set_closure_passes(32)
        S.apply(p, s)
        info = s.closure_info() if multi else dict(per_pass=K, passes=1 if K else 0, solves=1)
        t = []
        for it in range(12):
            s.set_states(p["pose"], p["vel"])
            rc, st = s.iterate_gn()
            assert rc == 0
            if it >= 2:
                t.append(s.last_timing())
        med = np.median(np.array(t), axis=0)
        rows.append(dict(chain=name, states=N, closures=K, per_pass=info["per_pass"], passes=info["passes"], solves=info["solves"],
                         R=s.plan_info()["R"], linearize_ms=med[0], assemble_ms=med[1], solve_ms=med[2], retract_ms=med[3], total_ms=med[4]))
        s.close()

print("| chain | closures | w | P | solves | R | linearize | assemble | solve | retract + error | total (ms) |")
print("|---|---|---|---|---|---|---|---|---|---|---|")
for r in rows:
    print("| %s | %d | %d | %d | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f |" % (r["chain"], r["closures"], r["per_pass"], r["passes"], r["solves"], r["R"],
          r["linearize_ms"], r["assemble_ms"], r["solve_ms"], r["retract_ms"], r["total_ms"]))
print(json.dumps(dict(bench="closures", rows=rows)))
