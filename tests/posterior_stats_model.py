"""Statistics of posterior draws at query times (include/gpslam_hip_sampling_stats.h) in plain numpy: the
reference side of tests/test_posterior_stats_model.py and tests/test_gpu_sampling_stats.py.

  position      where a pose row keeps its position: the first two coordinates, the translation (9 .. 11) on SE(3)
  eta           local coordinates of query poses around the reference poses, by oracle.local under a chart
  pack          the lower triangle of a d x d matrix in rows: entry (r, c) at r (r + 1) / 2 + c
  stats         s1, s2, hits (summed in draw order k = 0, 1, ...), g, clearance, length of a block of draws
  moments       mean and unbiased covariance from the sums, by numpy.mean / numpy.cov's formulas on the sums
  model_draws   draws to try the model on without a device: dense_sampling_model.walk_call from the description's own states
                over posterior_model's normals
  CASES, case   the graphs and query sets both test files run, by the names of tests/test_gpu_sampling_at.py's graph() and queries()
  dense_queries 64 evenly spaced queries in every interval: the query set that makes a call span two chunks
  obstacles     the obstacle set of a graph and query set, fixed here for the CPU and the GPU tests alike
"""
import numpy as np

from oracle import oracle as O
import dense_sampling_model as DS
import posterior_model as PM

MODEL_SEED, MODEL_COUNT = (5 << 40) + 23, 3
# (graph, with landmarks, states, query set) of tests/test_gpu_sampling_at.py's graph() and queries(); "dense" is dense_queries():
# every manifold, both SE(2) charts, one query, 300 queries on 301 states (one in every interval), 64 in each of 299 intervals
CASES = [("r2", False, None, "runs"), ("r3", True, None, "runs"), ("se2", True, None, "runs"), ("se2_expmap", False, None, "runs"),
         ("so3", False, None, "runs"), ("se3", True, None, "runs"), ("se3", False, None, "runs"), ("se3", False, 2, "one"), ("se2", True, 2, "one"),
         ("se2", True, 301, "every"), ("se3", False, 300, "dense")]
CASE_IDS = ["%s%s%s_%s" % (n, "_lm" if lm else "", "" if N is None else "_%d" % N, w) for n, lm, N, w in CASES]


def case(name, lm, N, which):
    """(description, (left, dt, tau)) of one of CASES"""
    import test_gpu_sampling_at as AT
    p = dict(AT.graph("se2", lm, N), chart=O.CHART_EXPMAP) if name == "se2_expmap" else AT.graph(name, lm, N)
    return p, (dense_queries(p) if which == "dense" else AT.queries(p, which))


def position(kind, poses):
    poses = np.asarray(poses, dtype=np.float64)
    return poses[..., 9:12] if kind == O.POSE3 else poses[..., :2]


def eta(kind, qhat, qp, chart):
    """(K, n, d): oracle.local(kind, qhat[q], qp[k, q], chart)"""
    qp = np.asarray(qp, dtype=np.float64)
    K, n = qp.shape[:2]
    return np.array([[O.local(kind, qhat[q], qp[k, q], chart) for q in range(n)] for k in range(K)]).reshape(K, n, O.TANGENT_DIM[kind])


def tri(d):
    return [(r, c) for r in range(d) for c in range(r + 1)]


def pack(M):
    return np.array([M[r, c] for r, c in tri(M.shape[0])])


def unpack(s2, d):
    M = np.zeros((d, d))
    for v, (r, c) in zip(s2, tri(d)):
        M[r, c] = M[c, r] = v
    return M


def stats(kind, chart, qhat, qp, obstacles=None, margin=0.0, start=None):
    """a block of draws qp (K, n, pose_dim) around qhat (n, pose_dim): dict of n, s1 (n, d), s2 (n, d (d + 1) / 2), eta (K, n, d), and
    -- where the manifold has a position -- length (K,) and, with obstacles (m, w + 1), g (K, n), hits (n,), clearance (K,).
    start: an earlier result to continue (n, s1, s2, hits)."""
    qp = np.asarray(qp, dtype=np.float64)
    K, n = qp.shape[:2]
    d = O.TANGENT_DIM[kind]
    e = eta(kind, qhat, qp, chart)
    out = dict(eta=e, n=K + (start["n"] if start else 0))
    s1 = np.array(start["s1"], dtype=np.float64) if start else np.zeros((n, d))
    s2 = np.array(start["s2"], dtype=np.float64) if start else np.zeros((n, d * (d + 1) // 2))
    for k in range(K):      # in draw order
        s1 = s1 + e[k]
        s2 = s2 + np.stack([e[k, :, r] * e[k, :, c] for r, c in tri(d)], axis=1)
    out.update(s1=s1, s2=s2)
    if kind == O.ROT3:
        return out
    p = position(kind, qp)
    out["length"] = np.array([sum(np.sqrt(((p[k, q + 1] - p[k, q]) ** 2).sum()) for q in range(n - 1)) if n > 1 else 0.0 for k in range(K)])
    if obstacles is not None and len(obstacles):
        ob = np.asarray(obstacles, dtype=np.float64)
        w = ob.shape[1] - 1
        dist = np.sqrt(((p[:, :, None, :] - ob[None, None, :, :w]) ** 2).sum(axis=3)) - ob[None, None, :, w]
        g = dist.min(axis=2) - margin
        hits = (g < 0.0).sum(axis=0).astype(np.int64)
        if start and start.get("hits") is not None:
            hits = hits + np.asarray(start["hits"], dtype=np.int64)
        out.update(g=g, hits=hits, clearance=g.min(axis=1))
    return out


def moments(n, s1, s2):
    """(mean (nq, d), cov (nq, d, d)): mean = s1 / n, cov = (S2 - n mean mean^T) / (n - 1)"""
    nq, d = s1.shape
    mean = s1 / n
    cov = np.array([(unpack(s2[q], d) - n * np.outer(mean[q], mean[q])) / (n - 1.0) for q in range(nq)])
    return mean, cov


def reference_poses(p, left, dt, tau):
    """the interpolated estimate at the queries, from the model's walk without noise (test_dense_sampling_model.py holds that to the
    oracle's interpolators)"""
    d = O.TANGENT_DIM[p["kind"]]
    return DS.walk_call(p["kind"], p["pose"], p["vel"], left, dt, tau, np.eye(d), np.zeros((len(left), 2 * d)))[0]


def model_draws(p, left, dt, tau, count=MODEL_COUNT, seed=MODEL_SEED):
    """(count, n, pose_dim): the bridge's walk from the description's own states over the generator's normals"""
    d = O.TANGENT_DIM[p["kind"]]
    Lq = np.linalg.cholesky(np.asarray(p["qc"], dtype=np.float64))
    eps = PM.noise(seed, 0, count, 2 * d * len(left))
    return np.stack([DS.walk_call(p["kind"], p["pose"], p["vel"], left, dt, tau, Lq, eps[k])[0] for k in range(count)])


def dense_queries(p, per=64):
    """(left, dt, tau): `per` evenly spaced queries in every interval of the chain (tests/test_gpu_sampling_at.py's two-chunk call)"""
    N = p["pose"].shape[0]
    dts = np.zeros(N - 1)
    dts[p["gp_left"]] = p["gp_dt"]
    left = np.repeat(np.arange(N - 1, dtype=np.int32), per)
    tau = (dts[:, None] * (np.arange(1, per + 1) / (per + 1.0))[None, :]).reshape(-1)
    return left, dts[left], tau


def obstacles(p, left, dt, tau):
    """(m, w + 1), from the path's own geometry so that it serves any graph: a sphere of radius 0.5 whose surface passes through the
    estimate's position at the middle query (n // 2: in the "runs" set a query in mid-interval, where the bridge's noise is not
    small) -- a draw falls inside or outside by its own noise there -- and, with more than one query, a second around the estimate's
    position at the last query, which every draw of it hits"""
    kind = p["kind"]
    pos = position(kind, reference_poses(p, left, dt, tau))
    w = pos.shape[1]
    e = np.zeros(w)
    e[0] = 1.0
    out = [np.concatenate([pos[len(left) // 2] + 0.5 * e, [0.5]])]
    if len(left) > 1:
        out.append(np.concatenate([pos[-1], [0.25]]))
    return np.array(out)
