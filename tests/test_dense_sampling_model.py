"""The bridge of include/gpslam_hip_sampling_at.h as tests/dense_sampling_model.py restates it, on the CPU: the walk against direct
Gaussian conditioning of the prior kernel, the closed-form Cholesky factor of K, the walk without noise against the oracle's
interpolators on every manifold, where the bridge's normals sit in the generator's stream, and the whitened moments of model draws at
the seed the GPU statistics test uses."""
import numpy as np
import pytest

from oracle import oracle as O
import dense_sampling_model as DS
import posterior_model as PM
from test_posterior_model import STAT_SEED, STAT_K

DT = 0.37
# runs of 1, 2, 3 and 7 queries as fractions of dt: gaps of 1e-3 dt to either end and between neighbours among them
GRID = {
    "one": [0.4], "one_at_the_left": [1e-3], "one_at_the_right": [1.0 - 1e-3],
    "two": [0.3, 0.8], "two_close": [0.5, 0.501],
    "three": [0.2, 0.5, 0.9], "three_at_the_ends": [1e-3, 0.5, 1.0 - 1e-3],
    "seven": [0.05, 0.2, 0.35, 0.5, 0.65, 0.8, 0.95], "seven_tight": [1e-3, 2e-3, 0.3, 0.5, 0.501, 0.998, 0.999],
}
QC = {2: np.array([[0.9, 0.3], [0.3, 0.6]]), 3: np.array([[0.9, 0.3, -0.2], [0.3, 0.6, 0.1], [-0.2, 0.1, 0.8]])}
MANIFOLDS = {"linear2": O.LINEAR2, "linear3": O.LINEAR3, "se2": O.POSE2, "so3": O.ROT3, "se3": O.POSE3}


@pytest.mark.parametrize("d", [2, 3])
def test_the_walk_is_the_conditional(d):
    Qc = QC[d]
    Lq = np.linalg.cholesky(Qc)
    worst_c = worst_w = 0.0
    for name, fr in GRID.items():
        taus = [f * DT for f in fr]
        A, B, N = DS.walk_weights(DT, taus)
        Wa, Wb, C = DS.conditioning(DT, taus, Qc)
        Nf = np.kron(N, Lq)
        ec = np.abs(Nf @ Nf.T - C).max() / np.abs(C).max()
        ew = max(np.abs(DS.full(A, np.eye(d)) - Wa).max() / np.abs(Wa).max(), np.abs(DS.full(B, np.eye(d)) - Wb).max() / np.abs(Wb).max())
        print("d %d, %s: covariance %.3g, mean weights %.3g (of 1e-12)" % (d, name, ec, ew))
        worst_c, worst_w = max(worst_c, ec), max(worst_w, ew)
    print("d %d: worst covariance %.3g, worst mean weights %.3g, of 1e-12" % (d, worst_c, worst_w))
    assert worst_c <= 1e-12 and worst_w <= 1e-12


def test_the_closed_form_cholesky_factor():
    worst = 0.0
    for name, fr in GRID.items():
        a = 0.0
        for f in fr:
            tau = f * DT
            _, _, K, l = DS.bridge(a, tau, DT)
            want = np.linalg.cholesky(K)
            err = max(abs(l[i, j] - want[i, j]) / abs(want[i, j]) for i, j in ((0, 0), (1, 0), (1, 1)) if want[i, j] != 0.0)
            assert l[0, 1] == 0.0
            worst = max(worst, err)
            a = tau
    print("closed-form l against numpy's Cholesky factor of K: worst %.3g of 1e-12 relative per entry" % worst)
    assert worst <= 1e-12


def _pair(kind, rng):
    """two neighbouring states a realistic step apart"""
    d = O.TANGENT_DIM[kind]
    if kind == O.POSE3:
        p1 = O.pose3((0.4, -0.2, 0.3), (1.0, -2.0, 0.5))
    elif kind == O.ROT3:
        p1 = O.rot3_ypr(0.4, -0.2, 0.3)
    else:
        p1 = rng.standard_normal(O.POSE_DIM[kind])
    v1 = rng.standard_normal(d)
    p2 = O.retract(kind, p1, DT * v1 + 0.05 * rng.standard_normal(d))
    return p1, v1, p2, v1 + 0.2 * rng.standard_normal(d)


@pytest.mark.parametrize("name", list(MANIFOLDS))
def test_without_noise_the_walk_is_the_interpolator(name):
    kind = MANIFOLDS[name]
    d = O.TANGENT_DIM[kind]
    p1, v1, p2, v2 = _pair(kind, np.random.default_rng(11))
    Qc = np.eye(d)
    worst = 0.0
    for fr in GRID.values():
        taus = [f * DT for f in fr]
        got, _ = DS.walk(kind, p1, v1, p2, v2, DT, taus, np.eye(d), np.zeros((len(taus), 2 * d)))
        for k, tau in enumerate(taus):
            Lam, Psi = O.lambda_psi(d, Qc, DT, tau)
            want, _ = O.interpolate(kind, Lam, Psi, p1, v1, p2, v2, jac=False)
            worst = max(worst, (np.abs(got[k] - want) / np.maximum(1.0, np.abs(want))).max())
    print("%s: walked poses against oracle.interpolate, worst %.3g of 1e-12" % (name, worst))
    assert worst <= 1e-12


def test_where_the_bridge_normals_sit():
    seed, first, n_noise, d, nq = (7 << 40) + 11, 2 ** 32 + 3, 37, 3, 5
    a = PM.noise(seed, first, 4, n_noise + 2 * d * nq)
    assert np.array_equal(a[:, :n_noise], PM.noise(seed, first, 4, n_noise))
    for s in range(4):
        for q in range(nq):
            j = DS.noise_index(n_noise, d, q)
            assert np.array_equal(j, n_noise + 2 * d * q + np.arange(2 * d))
            for c in range(2 * d):
                assert a[s, j[c]] == PM.normals(seed, np.uint64(first + s), np.uint64(n_noise + 2 * d * q + c))


def test_the_statistics_seed_on_the_cpu():
    """model bridge draws on one interval with three queries, whitened by the Cholesky factor of the conditioning covariance"""
    K, d = STAT_K, 3
    Qc = QC[d]
    Lq = np.linalg.cholesky(Qc)
    taus = [0.2 * DT, 0.5 * DT, 0.9 * DT]
    n = 2 * d * len(taus)
    eps = PM.noise(STAT_SEED, 0, K, n)
    rng = np.random.default_rng(3)
    p1, v1 = rng.standard_normal(d), rng.standard_normal(d)
    p2, v2 = p1 + DT * v1 + 0.05 * rng.standard_normal(d), v1 + 0.2 * rng.standard_normal(d)
    _, mean = DS.walk(O.LINEAR3, p1, v1, p2, v2, DT, taus, Lq, np.zeros((len(taus), 2 * d)))
    draws = np.stack([DS.walk(O.LINEAR3, p1, v1, p2, v2, DT, taus, Lq, e)[1].reshape(-1) for e in eps])
    _, _, C = DS.conditioning(DT, taus, Qc)
    w = np.linalg.solve(np.linalg.cholesky(C), (draws - mean.reshape(-1)).T).T
    bm, bs = PM.moment_bounds(n, K)
    m, S = w.mean(axis=0), w.T @ w / K
    print("seed %d, %d draws of %d coordinates: mean at most %.2f sigma, second moments at most %.2f sigma"
          % (STAT_SEED, K, n, np.abs(m).max() * np.sqrt(K), (np.abs(S - np.eye(n)) / (bs / 6.0)).max()))
    assert np.abs(m).max() <= bm
    assert (np.abs(S - np.eye(n)) <= bs).all()
