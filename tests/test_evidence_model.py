"""The numpy model of gpslam_hip_log_determinant and of the Laplace log-evidence (tests/evidence_model.py) against numpy's dense
slogdet and against the textbook GP marginal likelihood: the algebra evidence.hip implements, checked on the CPU."""
import numpy as np
import pytest

import evidence_model as EM
import marginals_model as MM


@pytest.mark.parametrize("N,b", [(N, b) for N in (1, 2, 15, 16, 17, 32, 33, 256, 257, 4097) for b in (4, 6, 12) if (N, b) != (4097, 12)])
def test_chunked_forward_recursion_against_slogdet(N, b):
    D, O = MM.random_chain(N, b, seed=N + b)
    got, levels = EM.chain_logdet(D, O)
    assert levels == {1: 0, 2: 1, 15: 1, 16: 1, 17: 2, 32: 2, 33: 2, 256: 2, 257: 3, 4097: 4}[N]
    if N * b <= 3100:
        ref, tol = EM.reference_logdet(MM.dense(D, O))
    else:           # (a dense reference of this size is minutes of LAPACK and gigabytes: the plain block recursion, kappa <= 1e9 asserted)
        ref, tol = EM.banded_reference_logdet(D, O)
    assert abs(got - ref) <= tol, (got, ref, tol)


@pytest.mark.parametrize("nl,nclo", [(0, 3), (4, 0), (6, 5), (16, 10)])
def test_lowrank_parts_sum_to_the_dense_logdet(nl, nclo):
    rng = np.random.default_rng(nl * 31 + nclo)
    N, b, d = 40, 6, 3
    D, O = MM.random_chain(N, b, seed=5)
    A = MM.dense(D, O)
    n = N * b
    Jc = None
    if nclo:
        Jc = np.zeros((nclo * d, n))
        for k in range(nclo):
            i, j = sorted(rng.choice(N, 2, replace=False))
            Jc[k * d:(k + 1) * d, i * b:i * b + d] = rng.standard_normal((d, d))
            Jc[k * d:(k + 1) * d, j * b:j * b + d] = rng.standard_normal((d, d))
    B = HLL = None
    if nl:
        B = 0.2 * rng.standard_normal((n, nl))
        G = rng.standard_normal((nl, nl))
        HLL = G @ G.T / nl + (1.0 + 0.04 * n) * np.eye(nl)
    ld_a, _ = EM.chain_logdet(D, O)
    ld_m, ld_s = EM.lowrank_parts(np.linalg.inv(A), B, Jc, HLL)
    Hxx = A + (Jc.T @ Jc if nclo else 0.0)
    H = np.block([[Hxx, B], [B.T, HLL]]) if nl else Hxx
    ref, tol = EM.reference_logdet(H)
    assert abs(ld_a + ld_m + ld_s - ref) <= tol, (ld_a, ld_m, ld_s, ref, tol)
    if not nl:
        assert ld_s == 0.0
    if not nclo:
        assert ld_m == 0.0


@pytest.mark.parametrize("d", [2, 3, 6])
@pytest.mark.parametrize("dt", [1e-3, 0.1, 7.0])
def test_gp_normaliser_formula(d, dt):
    rng = np.random.default_rng(d)
    G = rng.standard_normal((d, d))
    Qc = G @ G.T + 0.5 * np.eye(d)
    ref = -0.5 * np.linalg.slogdet(EM.gp_Q(dt, Qc))[1]
    assert abs(EM.gp_log_normaliser(Qc, dt) - ref) <= 1e-11 * max(1.0, abs(ref))


@pytest.mark.parametrize("theta", [0.01, 1.0, 30.0])
def test_laplace_evidence_of_a_linear_graph_is_the_gp_marginal_likelihood(theta):
    """The formula of include/gpslam_hip_evidence.h on the dense least-squares problem against log N(y; C m, C K C^T + R), which
    forms no Jacobian and no H"""
    pr = EM.linear_gp_problem(N=40, d=3, theta=1.0, seed=2)
    logZ, cost, logdet, lognorm, mn = EM.linear_gp_graph_logZ(pr, theta)
    ref = EM.gp_marginal_loglik(pr["m0"], pr["P0"], pr["dts"], theta * pr["Qc0"], pr["meas_idx"], pr["y"], pr["sig"])
    assert mn == pr["y"].size
    assert abs(logZ - ref) <= 1e-8 * max(1.0, abs(ref)), (logZ, ref)


def test_evidence_curve_peaks_near_the_truth():
    pr = EM.linear_gp_problem(N=40, d=3, theta=1.0, seed=2)
    thetas = 10.0 ** np.arange(-2.0, 2.01, 0.5)
    curve = [EM.gp_marginal_loglik(pr["m0"], pr["P0"], pr["dts"], t * pr["Qc0"], pr["meas_idx"], pr["y"], pr["sig"]) for t in thetas]
    k = int(np.argmax(curve))
    assert 0 < k < len(thetas) - 1 and 0.1 <= thetas[k] <= 10.0, (thetas[k], curve)


def test_banded_reference_with_its_power_iteration_kappa():
    """evidence_model.banded_reference_logdet (the reference of the one chain too long for a dense matrix) against the dense one: the
    same log det, and a bound that is no wider than the dense kappa gives"""
    D, O = MM.random_chain(257, 4, seed=9)
    ref, tol = EM.reference_logdet(MM.dense(D, O))
    got, btol = EM.banded_reference_logdet(D, O)
    assert abs(got - ref) <= tol
    assert btol <= tol * (1.0 + 1e-6)
