"""Posterior sampling at query times on the device (include/gpslam_hip_sampling_at.h, gpslam_amd/csrc/sampling.hip: k_ps_bridge;
DESIGN.md section 4n) against numpy: tests/dense_sampling_model.py's walk and its conditioning route, dogleg_model.system's dense H,
and the generator's model of tests/posterior_model.py.

Graphs: dogleg_model.FAMILY (12 to 16 states) and SIZES (two states; 300 states) as tests/test_gpu_posterior.py uses them -- se2 and so3
without their per-interval Qc, which the bridge refuses -- the r3 graph with a non-diagonal Qc, and 12-state LINEAR2 / LINEAR3 chains of GP priors, priors
and between factors (LINEAR2 with landmarks: landmark priors only, no LINEAR2 factor names a landmark; the family's r3 graph exists
with landmarks only).
Query sets: one query on a two-state chain; on the 12 to 16-state chains runs of 2, 7 and 1 queries on intervals 0, 3 and N - 2 with
empty intervals between, gaps of 1e-3 dt among them; a query in every interval of the 300-state graphs (299 runs: three workgroups,
the last one partial), with landmarks too (the bridge's normals sit behind the landmark priors' entries).

Bounds.
  Covariance identity, noise = I (vector spaces): sum_k (q_k - mean)(q_k - mean)^T against G inv(H) G^T + the bridge's blocks from the
    conditioning route, entry by entry, at tests/test_gpu_posterior.py's rule: 2 * 1e-9 * sum_k |q_k - mean|_inf^2 plus ten times the
    twin distance of the model's matrix (float64 against np.longdouble), capped at 1e-7.
  The walk and the conditional mean: 1e-11 * max(1, |want|), the bar tests/test_gpu_parity.py holds interpolated poses to.
  Marginals: the identity's bound plus 1e-9 |P|.  Generator: 1e-12 absolute.  Statistics at a fixed seed, 2048 draws: second moments
    within 6 sqrt((1 + [i = j]) / K) of I, mean within 6 / sqrt(K).
Everything else is to the bit."""
import numpy as np
import pytest

import gpslam_amd as gp
from oracle import oracle as O
import dogleg_model as DM
import posterior_model as PM
import dense_sampling_model as DS
from test_gpu_dogleg import device, ahrs_pair, STEP_TOL
from test_gpu_posterior import inv_long, same_bits, SEED, FIRST, REFUSALS
from test_posterior_model import STAT_SEED, STAT_K

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-11
KSLAB = 1 << 22           # doubles per slab of a chunk of draws (sampling.hip: kPsSlab)
QC3 = np.array([[0.9, 0.3, -0.2], [0.3, 0.6, 0.1], [-0.2, 0.1, 0.8]])
QC2 = np.array([[0.8, 0.25], [0.25, 0.6]])


# ---------------------------------------------------------------------------------------------------------------- graphs and queries
def shared_qc(p):
    """the description with every GP prior on the handle's Qc"""
    return {k: v for k, v in p.items() if k != "gp_qc"}


def linear(kind, landmarks):
    """a 12-state chain on a vector space: GP priors, position priors at both ends, a velocity prior, between factors; with landmarks:
    two landmarks under priors"""
    from test_gpu_parity import random_chain
    N, d = 12, O.TANGENT_DIM[kind]
    c = random_chain(kind, N, 5)
    rng = np.random.default_rng(41)
    idx = np.arange(N - 1, dtype=np.int32)
    p = dict(kind=kind, chart=O.CHART_EXPMAP, velocity_world=False, N=N, qc=QC2 if d == 2 else QC3, pose=c["pose"], vel=c["vel"],
             gp_left=idx[::-1].copy(), gp_dt=c["dt"][::-1].copy(),
             prior_idx=np.array([0, N - 1], dtype=np.int32), prior_pose=c["truth_pose"][[0, N - 1]], prior_sig=0.05 + 0.05 * rng.random((2, d)),
             vprior_idx=np.array([0], dtype=np.int32), vprior=c["truth_vel"][:1], vprior_sig=0.1 + 0.1 * rng.random((1, d)),
             between_left=idx, between_meas=np.diff(c["truth_pose"], axis=0) + 0.02 * rng.standard_normal((N - 1, d)),
             between_sig=0.05 + 0.05 * rng.random((N - 1, d)))
    if landmarks:
        lands = np.array([[1.0, 2.0], [3.0, -1.0]])
        p.update(ld=2, landmarks=lands + 0.1, lprior_idx=np.arange(2, dtype=np.int32), lprior=lands, lprior_sig=0.5 + 0.2 * rng.random((2, 2)))
    return p


def graph(name, lm, N=None):
    if name in ("r2", "r3_plain"):
        return linear(O.LINEAR2 if name == "r2" else O.LINEAR3, lm)
    p = shared_qc(DM.graph(name, lm, N))
    if name == "r3":
        p["qc"] = QC3
    return p


def interval_dt(p):
    dt = np.zeros(p["pose"].shape[0] - 1)
    dt[p["gp_left"]] = p["gp_dt"]
    return dt


def queries(p, which):
    """(left, dt, tau) of a query set (module docstring)"""
    N, dts = p["pose"].shape[0], interval_dt(p)
    if which == "one":
        runs = [(0, [0.37])]
    elif which == "runs":
        runs = [(0, [1e-3, 0.6]), (3, [0.1, 0.101, 0.3, 0.5, 0.7, 0.9, 1.0 - 1e-3]), (N - 2, [0.45])]
    else:
        rng = np.random.default_rng(9)
        runs = [(i, [0.05 + 0.9 * rng.random()]) for i in range(N - 1)]
    left = np.array([i for i, fr in runs for _ in fr], dtype=np.int32)
    tau = np.array([f * dts[i] for i, fr in runs for f in fr])
    return left, dts[left], tau


def lq_of(p):
    return np.linalg.cholesky(np.asarray(p["qc"], dtype=np.float64))


@pytest.fixture(scope="module")
def reference():
    """per vector-space graph: the description, its query set and the model's matrices (computed once, never written to)"""
    cache = {}

    def get(name, lm):
        if (name, lm) not in cache:
            p = graph(name, lm)
            H, _, _ = DM.system(p)
            N, d = p["pose"].shape[0], O.TANGENT_DIM[p["kind"]]
            left, dt, tau = queries(p, "runs")
            G, C = DS.linear_maps(N, d, left, dt, tau, p["qc"])
            Gf = np.zeros((G.shape[0], H.shape[0]))
            Gf[:, :G.shape[1]] = G
            model = Gf @ np.linalg.inv(H) @ Gf.T + C
            long = Gf.astype(np.longdouble) @ inv_long(H) @ Gf.T.astype(np.longdouble) + C.astype(np.longdouble)
            twin = float(np.abs(model.astype(np.longdouble) - long).max())
            mean = G @ np.concatenate([p["pose"], p["vel"]], axis=1).reshape(-1)
            cache[(name, lm)] = dict(p=p, q=(left, dt, tau), model=model, twin=twin, mean=mean, d=d)
        return cache[(name, lm)]
    return get


VECTOR = [("r2", False), ("r2", True), ("r3_plain", False), ("r3", True)]      # (the family's r3 graph exists with landmarks only)
VECTOR_IDS = ["linear2", "linear2_lm", "linear3", "linear3_lm"]


def unit_noise_sum(ref):
    """(S, tol): sum over the n_noise_at unit-noise draws of (q - mean)(q - mean)^T, q = per query [position; velocity], and its bound"""
    dev = device(ref["p"])
    left, dt, tau = ref["q"]
    n_at = dev.posterior_noise_dim_at(len(left))
    assert n_at == dev.posterior_noise_dim() + 2 * ref["d"] * len(left)
    qp, qv = dev.sample_posterior_at(left, dt, tau, n_at, noise=np.eye(n_at), want=("query_poses", "query_vels"))[:2]
    Z = np.concatenate([qp, qv], axis=2).reshape(n_at, -1) - ref["mean"]
    tol = 2.0 * STEP_TOL * float((np.abs(Z).max(axis=1) ** 2).sum()) + min(10.0 * ref["twin"], 1e-7)
    return Z.T @ Z, tol, n_at


# ---------------------------------------------------------------- 1. the covariance identity
@pytest.mark.parametrize("name,lm", VECTOR, ids=VECTOR_IDS)
def test_unit_noise_gives_the_covariance(reference, name, lm):
    ref = reference(name, lm)
    S, tol, n_at = unit_noise_sum(ref)
    err = np.abs(S - ref["model"]).max()
    print("%s%s: n_noise_at %d, %d queries: |sum (q - mean)(q - mean)^T - (G inv(H) G^T + bridge)| %.3g of %.3g (twin %.3g, largest entry %.3g)"
          % (name, "_lm" if lm else "", n_at, len(ref["q"][0]), err, tol, ref["twin"], np.abs(ref["model"]).max()))
    assert err <= tol


# ---------------------------------------------------------------- 2. the walk on every accepted manifold
def check_walk(p, which, what, draws=2):
    dev = device(p)
    kind, d = p["kind"], O.TANGENT_DIM[p["kind"]]
    left, dt, tau = queries(p, which)
    n_noise, n_at = dev.posterior_noise_dim(), dev.posterior_noise_dim_at(len(left))
    noise = PM.noise(SEED, FIRST, draws, n_at)
    vector = kind in DS.VECTOR
    want = ("query_poses", "delta", "poses", "vels", "landmarks") + (("query_vels",) if vector else ())
    qp, qv, delta, poses, vels, lms = dev.sample_posterior_at(left, dt, tau, draws, noise=noise, want=want)
    assert qp.shape == (draws, len(left), O.POSE_DIM[kind]) and delta is not None and (lms is None) == ("landmarks" not in p)
    worst = 0.0
    for k in range(draws):
        mp, mg = DS.walk_call(kind, poses[k], vels[k], left, dt, tau, lq_of(p), noise[k, n_noise:])
        worst = max(worst, (np.abs(qp[k] - mp) / np.maximum(1.0, np.abs(mp))).max())
        if vector:
            worst = max(worst, (np.abs(qv[k] - mg[:, d:]) / np.maximum(1.0, np.abs(mg[:, d:]))).max())
    # the draw moved the queries off the conditional mean of its own support states
    moved = np.abs(qp[0] - dev.sample_posterior_at(left, dt, tau, 1, noise=np.concatenate([noise[:1, :n_noise], np.zeros((1, n_at - n_noise))], axis=1))[0][0]).max()
    print("%s, %d queries in %d runs: query poses against the model's walk %.3g of %.3g; bridge noise moved them by up to %.3g"
          % (what, len(left), len(DS.runs(left)), worst, POSE_TOL, moved))
    assert worst <= POSE_TOL
    assert moved > 1e-6


WALKS = [("r2", False, None, "runs"), ("r2", True, None, "runs"), ("r3", True, None, "runs"), ("se2", True, None, "runs"), ("se2_expmap", False, None, "runs"),
         ("so3", False, None, "runs"), ("se3", True, None, "runs"), ("se3", False, None, "runs"),
         ("se3", False, 2, "one"), ("se2", True, 2, "one"), ("se3", False, 300, "every"), ("se2", True, 300, "every")]


@pytest.mark.parametrize("name,lm,N,which", WALKS, ids=["%s%s%s_%s" % (n, "_lm" if lm else "", "" if N is None else "_%d" % N, w) for n, lm, N, w in WALKS])
def test_the_walk_from_the_draws_own_support_states(name, lm, N, which):
    if name == "se2_expmap":
        p = dict(graph("se2", lm, N), chart=O.CHART_EXPMAP)
    else:
        p = graph(name, lm, N)
    check_walk(p, which, "%s N %s" % (name, p["pose"].shape[0]))


# ---------------------------------------------------------------- 3. zero bridge noise is the conditional mean
@pytest.mark.parametrize("name,lm,N,which", [("se3", True, None, "runs"), ("se2", True, 300, "every"), ("r3", True, None, "runs")], ids=["se3_lm", "se2_lm_300", "linear3_lm"])
def test_zero_bridge_noise_is_the_conditional_mean(name, lm, N, which):
    p = graph(name, lm, N)
    dev, twin = device(p), device(p)
    left, dt, tau = queries(p, which)
    n_noise, n_at = dev.posterior_noise_dim(), dev.posterior_noise_dim_at(len(left))
    noise = dev.posterior_noise_at(SEED, FIRST, 1, len(left))
    noise[:, n_noise:] = 0.0
    qp, _, _, poses, vels, _ = dev.sample_posterior_at(left, dt, tau, 1, noise=noise, want=("query_poses", "poses", "vels"))
    twin.set_states(poses[0], vels[0])
    want = twin.interpolate_poses(left, dt, tau)
    err = (np.abs(qp[0] - want) / np.maximum(1.0, np.abs(want))).max()
    print("%s: zero bridge noise against interpolate_poses of the drawn support states %.3g of %.3g" % (name, err, POSE_TOL))
    assert n_at > n_noise and err <= POSE_TOL


# ---------------------------------------------------------------- 4. consistency with the marginals
def test_diagonal_blocks_are_the_interpolated_covariances(reference):
    ref = reference("r3", True)
    S, tol, _ = unit_noise_sum(ref)
    left, dt, tau = ref["q"]
    d = ref["d"]
    twin = device(ref["p"])
    twin.marginals()
    P = twin.interpolate_covariances(left, dt, tau, gp_term=True)
    worst = 0.0
    for q in range(len(left)):
        blk = S[2 * d * q:2 * d * q + d, 2 * d * q:2 * d * q + d]
        bound = tol + 1e-9 * np.abs(P[q]).max()
        worst = max(worst, np.abs(blk - P[q]).max() / bound)
        assert np.abs(blk - P[q]).max() <= bound, (q, np.abs(blk - P[q]).max(), bound)
    print("position blocks against interpolate_covariances(gp_term=True): worst %.3g of the bound" % worst)


# ---------------------------------------------------------------- 5. to the bit
SE2_LM = ("se2", True, None)


def test_support_outputs_are_sample_posteriors():
    for name, lm, N in (SE2_LM, ("se3", False, None)):
        p = graph(name, lm, N)
        dev = device(p)
        left, dt, tau = queries(p, "runs")
        plain = dev.sample_posterior(3, seed=SEED, first=FIRST)
        dense = dev.sample_posterior_at(left, dt, tau, 3, seed=SEED, first=FIRST, want=("query_poses", "delta", "poses", "vels", "landmarks"))
        same_bits(plain, dense[2:])
        # the same leading columns from the caller: the same support states
        noise = dev.posterior_noise_at(SEED, FIRST, 3, len(left))
        noise[:, dev.posterior_noise_dim():] = 1.0
        same_bits(plain, dev.sample_posterior_at(left, dt, tau, 3, noise=noise, want=("delta", "poses", "vels", "landmarks"))[2:])
        same_bits(plain, dev.sample_posterior(3, seed=SEED, first=FIRST))


@pytest.mark.parametrize("name,lm,N", [SE2_LM, ("se3", False, None)], ids=["se2_lm", "se3"])
def test_a_draw_does_not_depend_on_the_batch(name, lm, N):
    p = graph(name, lm, N)
    dev = device(p)
    left, dt, tau = queries(p, "runs")
    want = ("query_poses", "delta", "poses", "vels", "landmarks")
    five = dev.sample_posterior_at(left, dt, tau, 5, seed=SEED, first=FIRST, want=want)
    for k in range(5):
        one = dev.sample_posterior_at(left, dt, tau, 1, seed=SEED, first=FIRST + k, want=want)
        same_bits([None if a is None else a[k] for a in five], [None if a is None else a[0] for a in one])
    assert not np.array_equal(five[0][0], five[0][1])


def test_a_call_that_spans_two_chunks():
    """ps_chunk's rule: a chunk is KSLAB // (the widest slab row) draws; 64 queries in every interval of the 300-state SE(3) graph make
    the noise row the widest and the chunk a dozen and a half draws"""
    name, lm, N = DM.SIZES[2]
    p = graph(name, lm, N)
    dev = device(p)
    dts = interval_dt(p)
    per = 64
    left = np.repeat(np.arange(N - 1, dtype=np.int32), per)
    tau = (dts[:, None] * (np.arange(1, per + 1) / (per + 1.0))[None, :]).reshape(-1)
    nq = len(left)
    n_at = dev.posterior_noise_dim_at(nq)
    widest = max(n_at, N * dev.b + dev.L * dev.ld, N * dev.pd, nq * dev.pd)
    chunk = KSLAB // widest
    assert 2 <= chunk <= 40, chunk
    count = chunk + 2
    want = ("query_poses", "poses")
    all_ = dev.sample_posterior_at(left, dts[left], tau, count, seed=SEED, first=FIRST, want=want)
    for k in (chunk - 1, chunk, chunk + 1):      # the last draw of the first chunk, the two of the second
        one = dev.sample_posterior_at(left, dts[left], tau, 1, seed=SEED, first=FIRST + k, want=want)
        same_bits([None if a is None else a[k] for a in all_], [None if a is None else a[0] for a in one])
    print("chunk of %d draws (widest row %d doubles), %d draws of %d queries" % (chunk, widest, count, nq))


def test_generated_equals_the_call_on_the_generators_numbers_and_reruns():
    p = graph(*SE2_LM)
    left, dt, tau = queries(p, "runs")
    want = ("query_poses", "delta", "poses", "vels", "landmarks")
    out = []
    for _ in range(2):
        dev = device(p)
        out.append(dev.sample_posterior_at(left, dt, tau, 3, seed=SEED, first=FIRST, want=want))
    same_bits(out[0], out[1])
    noise = dev.posterior_noise_at(SEED, FIRST, 3, len(left))
    same_bits(out[0], dev.sample_posterior_at(left, dt, tau, 3, noise=noise, want=want))


def test_only_the_outputs_asked_for_come_back():
    p = graph("r3", True)
    dev = device(p)
    left, dt, tau = queries(p, "runs")
    names = ("query_poses", "query_vels", "delta", "poses", "vels", "landmarks")
    full = dev.sample_posterior_at(left, dt, tau, 3, seed=SEED, first=FIRST, want=names)
    assert all(a is not None for a in full)
    for want in (("query_poses",), ("query_vels",), ("delta",), ("poses", "vels"), ("landmarks", "query_poses")):
        part = dev.sample_posterior_at(left, dt, tau, 3, seed=SEED, first=FIRST, want=want)
        for name, a, b in zip(names, full, part):
            assert (b is None) == (name not in want)
            assert b is None or np.array_equal(a, b)
    assert dev.sample_posterior_at(left, dt, tau, 1)[0].shape == (1, len(left), 3)      # (the default: the query poses)
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\)"):
        dev.sample_posterior_at(left, dt, tau, 1, want=())
    with pytest.raises(gp.GpslamHipError, match="want"):
        dev.sample_posterior_at(left, dt, tau, 1, want=("states",))


def test_the_handle_is_left_alone_and_the_marginals_are_stale():
    p = graph(*SE2_LM)
    dev, twin = device(p), device(p)
    left, dt, tau = queries(p, "runs")
    before = dev.get_states() + (dev.get_landmarks(),)
    rows = dev.get_rows()
    dev.marginals()
    marg = dev.get_marginals(cross=True)
    dev.sample_posterior_at(left, dt, tau, 4, seed=3)
    same_bits(before, dev.get_states() + (dev.get_landmarks(),))
    same_bits(rows, dev.get_rows())
    with pytest.raises(gp.GpslamHipError, match="stale"):
        dev.get_marginals()
    dev.marginals()
    same_bits(marg, dev.get_marginals(cross=True))
    for _ in range(2):
        dev.iterate_gn()
        twin.iterate_gn()
        same_bits(dev.get_states() + (dev.get_landmarks(),), twin.get_states() + (twin.get_landmarks(),))


# ---------------------------------------------------------------- 6. the generator
@pytest.mark.parametrize("name,lm,N,which", [("se3", False, 2, "one"), ("se2", True, None, "runs"), ("se2", True, 300, "every")], ids=["se3_2", "se2_lm", "se2_lm_300"])
def test_generator_equals_the_model(name, lm, N, which):
    p = graph(name, lm, N)
    dev = device(p)
    nq = len(queries(p, which)[0])
    n_noise, n_at, count = dev.posterior_noise_dim(), dev.posterior_noise_dim_at(nq), 3
    got = dev.posterior_noise_at(SEED, FIRST, count, nq)
    want = PM.noise(SEED, FIRST, count, n_at)
    err = np.abs(got - want).max()
    print("%s N %s: n_noise %d, n_noise_at %d, generator against the model %.3g" % (name, N, n_noise, n_at, err))
    assert got.shape == want.shape and n_at == n_noise + 2 * dev.d * nq and err <= 1e-12
    assert np.array_equal(got[:, :n_noise], dev.posterior_noise(SEED, FIRST, count))


# ---------------------------------------------------------------- 7. statistics at a fixed seed
def test_statistics_of_generated_draws(reference):
    ref = reference("r3", True)
    K, d = STAT_K, ref["d"]
    left, dt, tau = ref["q"]
    dev = device(ref["p"])
    qp = dev.sample_posterior_at(left, dt, tau, K, seed=STAT_SEED)[0]
    pos = (np.arange(2 * d * len(left)) % (2 * d)) < d                 # the position rows of the model's [position; velocity] stacking
    C = ref["model"][np.ix_(pos, pos)]
    n = C.shape[0]
    w = np.linalg.solve(np.linalg.cholesky(C), (qp.reshape(K, -1) - ref["mean"][pos]).T).T
    bm, bs = PM.moment_bounds(n, K)
    mean, S = w.mean(axis=0), w.T @ w / K
    print("seed %d, %d draws of %d query coordinates: mean at most %.2f sigma, second moments at most %.2f sigma"
          % (STAT_SEED, K, n, np.abs(mean).max() * np.sqrt(K), (np.abs(S - np.eye(n)) / (bs / 6.0)).max()))
    assert np.abs(mean).max() <= bm
    assert (np.abs(S - np.eye(n)) <= bs).all()


# ---------------------------------------------------------------- 8. refusals and argument errors
def check_untouched(a, b, p, call, pattern):
    lm = "landmarks" in p
    before = a.get_states() + ((a.get_landmarks(),) if lm else ())
    a.launch_census()
    nothing = a.launch_census()
    with pytest.raises(gp.GpslamHipError, match=pattern):
        call(a)
    assert a.launch_census() == nothing
    same_bits(before, a.get_states() + ((a.get_landmarks(),) if lm else ()))
    a.iterate_gn()
    b.iterate_gn()
    same_bits(a.get_states(), b.get_states())


def _edit(q, **kw):
    left, dt, tau = (np.array(a) for a in q)
    for name, (at, val) in kw.items():
        dict(left=left, dt=dt, tau=tau)[name][at] = val
    return left, dt, tau


def test_query_errors_name_the_query():
    p = graph("se3", False)
    N = p["pose"].shape[0]
    q = queries(p, "runs")           # queries 0, 1 on interval 0; 2 .. 8 on interval 3; 9 on interval N - 2
    cases = [
        ("unsorted left", _edit(q, left=(9, 1)), r"query 9: left must be non-decreasing"),
        ("tau does not increase", _edit(q, tau=(4, q[2][3])), r"query 4: tau must increase"),
        ("tau decreases", _edit(q, tau=(5, 0.5 * q[2][4])), r"query 5: tau must increase"),
        ("tau = 0", _edit(q, tau=(0, 0.0)), r"query 0: tau must lie inside"),
        ("tau < 0", _edit(q, tau=(2, -0.01)), r"query 2: tau must lie inside"),
        ("tau = dt", _edit(q, tau=(9, q[1][9])), r"query 9: tau must lie inside"),
        ("tau > dt", _edit(q, tau=(8, 1.5 * q[1][8])), r"query 8: tau must lie inside"),
        ("unequal dt", _edit(q, dt=(6, 1.01 * q[1][6])), r"query 6: delta_t differs"),
        ("left = N - 1", _edit(q, left=(9, N - 1)), r"query 9: interval out of range"),
        ("left < 0", _edit(q, left=(0, -1)), r"query 0: interval out of range"),
    ]
    for what, (left, dt, tau), message in cases:
        check_untouched(device(p), device(p), p, lambda s: s.sample_posterior_at(left, dt, tau, 2), r"\(-1\).*" + message)
    dev = device(p)
    for count in (0, -1):
        with pytest.raises(gp.GpslamHipError, match=r"\(-1\)"):
            dev.sample_posterior_at(*q, count)
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\)"):
        dev.sample_posterior_at([], [], [], 1)
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\)"):
        dev.posterior_noise_dim_at(0)
    with pytest.raises(gp.GpslamHipError, match="noise must be"):
        dev.sample_posterior_at(*q, 1, noise=np.zeros((1, dev.posterior_noise_dim())))


def test_what_the_bridge_refuses():
    # query velocities on a Lie group
    p = graph("se2", True)
    q = queries(p, "runs")
    check_untouched(device(p), device(p), p, lambda s: s.sample_posterior_at(*q, 2, want=("query_vels",)), r"\(-5\).*query_vels")
    # GP priors with a Qc of their own: the family's se2 graph as it is
    p = DM.graph("se2", True)
    assert "gp_qc" in p
    check_untouched(device(p), device(p), p, lambda s: s.sample_posterior_at(*q, 2), r"\(-5\).*Qc of their own")
    # world-frame velocities
    p = DM.graph("se3_vw", False)
    q = queries(p, "runs")
    check_untouched(device(p), device(p), p, lambda s: s.sample_posterior_at(*q, 2), r"\(-5\).*world-frame")
    # GPSLAM_ROT3_BIAS
    _, dev = ahrs_pair()
    before = dev.get_states()
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*ROT3_BIAS"):
        dev.sample_posterior_at([0], [0.1], [0.05], 1)
    same_bits(before, dev.get_states())


@pytest.mark.parametrize("what,kw,extra,message,lm", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_what_sample_posterior_refuses_is_refused(what, kw, extra, message, lm):
    p = DM.graph("se2", lm, 60 if what == "segmented" else None)      # (segments need a chain to cut)
    q = queries(p, "runs")
    check_untouched(device(p, extra, **kw), device(p, extra, **kw), p, lambda s: s.sample_posterior_at(*q, 2), r"\(-5\).*sample_posterior_at.*" + message)


def test_uncompiled_handle():
    import fixed_lag_mix_model as FM
    p = graph(*SE2_LM)
    raw = FM.chain(p, gp.ChainSolver)
    raw.set_qc(p["qc"])
    raw.set_states(p["pose"], p["vel"])
    with pytest.raises(gp.GpslamHipError, match=r"\(-4\)"):
        raw.sample_posterior_at(*queries(p, "runs"), 1)
