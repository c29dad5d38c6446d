"""Marginals on handles whose loop closures go through the solver in column passes (gpslam_hip_marginals_keep_closure_columns;
marginals_clo.hip: k_mg_clo_inverse, k_mg_clo_finish; api_impl.inc launch_solve_passes with keep_z) against dense inverses of the oracle's H.

Sigma_xx = A^-1 + W S^-1 W^T - Z M^-1 Z^T with Z = A^-1 U^T kept at every state, a slice per pass (the algebra:
tests/marginals_passes_model.py).  Tolerance: the project's, tol_of(H) = max(1e-10, 100 eps kappa_s) in correlation units, kappa_s
the condition number of the Jacobi-scaled dense H; tol_of caps it at 1e-7, and the graphs are small enough that the oracle alone
stays under the cap (kappa_s of every case is in its docstring, computed on the CPU oracle after the stated Gauss-Newton steps).
Every test looks at closure_info() before it looks at a number, and every test calls the opt-in."""
import numpy as np
import pytest

from oracle import oracle as O
from gpslam_amd import synthetic as S
import marginals_model as MM
from test_gpu_parity import gpu
from test_gpu_marginals import oracle_H, tol_of, check_blocks, gn
from test_gpu_closure_passes import _pairs, _device, _info
from test_gpu_closure import _anchored, _strip_landmarks

pytestmark = pytest.mark.gpu


def _oracle(p):
    return S.apply(p, O.Chain(p["kind"], landmark_dim=2 if "landmarks" in p else 0))


def _keep(p, *a, **kw):
    dev = _device(p, *a, **kw)
    dev.marginals_keep_closure_columns()
    return dev


def _check(p, dev, steps, cross=False):
    """steps of Gauss-Newton, then every Sigma_{i,i} and Sigma_{i,i+1} (and the landmark blocks) against inv(oracle_H)"""
    gn(dev, steps)
    H = oracle_H(_oracle(p), dev, p)
    tol = tol_of(H)
    dev.marginals()
    if not cross:
        Sd, Sn = dev.get_marginals()
        return check_blocks(H, Sd, Sn, dev.b, tol), tol
    Sd, Sn, Slm, Sxl = dev.get_marginals(cross=True)
    Sig = check_blocks(H, Sd, Sn, dev.b, tol)
    n = dev.N * dev.b
    dg = np.sqrt(np.diag(Sig))
    assert np.max(np.abs(Slm - Sig[n:, n:]) / np.outer(dg[n:], dg[n:])) <= tol
    ref = Sig[:n, n:].reshape(dev.N, dev.b, -1)
    assert np.max(np.abs(Sxl - ref) / np.outer(dg[:n], dg[n:]).reshape(Sxl.shape)) <= tol
    return Sig, tol


def _pose2_graph(K):
    return S.add_loop_closures(_anchored(_strip_landmarks(S.pose2_range_chain(60, seed=9))), _pairs(60, K, 21), seed=5)


def _pose3_graph(K):
    return S.add_loop_closures(S.pose3_chain(100, seed=2), _pairs(100, K, 31), seed=8)


@pytest.mark.parametrize("K,P", [(12, 2), (40, 5)])
def test_pose2_chain(K, P):
    """SE(2), 60 states.  12 closures: slices 9 + 3, nc = 36, kappa_s 5.6e5; 40: nc = 120, the cap, kappa_s 2.3e5.  (120 states and
    more: kappa_s 8.2e6, beyond tol_of's cap.)"""
    p = _pose2_graph(K)
    dev = _keep(p)
    _info(dev, K, 9, P)
    _check(p, dev, 3)


@pytest.mark.parametrize("K,P", [(6, 2), (20, 5)])
def test_pose3_chain(K, P):
    """SE(3), 100 states: 25 groups of four states, four workgroups.  6 closures: nc = 36, kappa_s 4.5e5; 20: nc = 120, kappa_s 1.3e5"""
    p = _pose3_graph(K)
    dev = _keep(p)
    _info(dev, K, 4, P)
    _check(p, dev, 3)


def test_pose3_closures_at_the_ends_and_in_both_orders():
    """The first state and the last one (whose Sigma_{i,i+1} is zero: check_blocks asserts it), both key orders, and states shared by
    closures of different slices (0, 50 and 99: closures 0 .. 3 are slice 0, 4 and 5 slice 1 -- 99 is in both).  kappa_s 1.6e5"""
    pairs = [[0, 99], [99, 50], [50, 0], [10, 60], [61, 11], [30, 98]]
    p = S.add_loop_closures(S.pose3_chain(100, seed=2), pairs, seed=8)
    dev = _keep(p)
    _info(dev, 6, 4, 2)
    _check(p, dev, 3)


@pytest.mark.parametrize("N", [33, 47, 48, 49, 64, 65])
def test_tile_remainders(N):
    """LINEAR3 (block size 6: a wave's group is eight states, a workgroup's eight groups 64), 10 closures in slices 9 + 1: nc = 30,
    neither a multiple of 4 nor of 16.  Chain lengths around one and two groups of tiles and around one workgroup; none is a multiple
    of eight but 48 and 64.  kappa_s 1.1e5 .. 2.9e5"""
    p = S.add_loop_closures(S.linear_chain(N, seed=4), _pairs(N, 10, 41), seed=9)
    dev = _keep(p)
    _info(dev, 10, 9, 2)
    _check(p, dev, 1)


def test_linear3_with_40_closures():
    """150 states, P = 5, kappa_s 4.7e5"""
    p = S.add_loop_closures(S.linear_chain(150, seed=4), _pairs(150, 40, 41), seed=9)
    dev = _keep(p)
    _info(dev, 40, 9, 5)
    _check(p, dev, 1)


def test_landmarks_and_closures_all_four_outputs():
    """8 landmark columns leave room for 6 closures per pass: 10 closures in two, every border column in use.  The landmark term
    W S^-1 W^T comes from the closure-corrected landmark columns of the final pass, the closure term from the kept Z.  kappa_s 3.8e5"""
    p = S.add_loop_closures(_anchored(S.pose2_range_chain(60, L=4, seed=3)), _pairs(60, 10, 51), seed=7)
    dev = _keep(p)
    _info(dev, 10, 6, 2)
    assert dev.plan_info()["R"] == 27
    _check(p, dev, 4, cross=True)


def test_one_closure_per_pass_against_the_single_pass_path():
    """Three closures, one per pass (the new kernels), beside a default handle that takes all three in one (k_mg_core / k_mg_finish as
    before), at the same states: both within tol_of(H) of the oracle.  Prints how far the two are from each other.  kappa_s 3.5e5"""
    p = S.add_loop_closures(_anchored(_strip_landmarks(S.pose2_range_chain(60, seed=2))), [[3, 40], [59, 20], [21, 50]], seed=4)
    dev = _keep(p, 8, 1)
    _info(dev, 3, 1, 3)
    one = _device(p, None)
    _info(one, 3, 3, 1)
    gn(dev, 3)
    one.set_states(*dev.get_states())
    H = oracle_H(_oracle(p), dev, p)
    tol = tol_of(H)
    out = []
    for s in (dev, one):
        s.marginals()
        Sd, Sn = s.get_marginals()
        check_blocks(H, Sd, Sn, s.b, tol)
        out.append((Sd, Sn))
    dg = np.sqrt(np.einsum("nii->ni", out[1][0]))
    worst = float(np.max(np.abs(out[0][0] - out[1][0]) / (dg[:, :, None] * dg[:, None, :])))
    print("three passes vs one pass: largest difference of a Sigma_{i,i} entry in correlation units %.3e (tolerance %.3e)" % (worst, tol))


def test_interpolated_covariance_against_the_oracle():
    """24 random queries on the SE(3) handle with 6 closures, drawn and checked as test_lie_interpolated_covariance_against_the_oracle
    does; Sigma from the oracle's H with the closures' coupling blocks"""
    p = _pose3_graph(6)
    dev = _keep(p)
    _info(dev, 6, 4, 2)
    Sig, tol = _check(p, dev, 3)
    Qc, dts = p["qc"], np.asarray(p["gp_dt"], dtype=np.float64)
    pose, vel = dev.get_states()
    rng = np.random.default_rng(9)
    left = rng.integers(0, dev.N - 1, 24).astype(np.int32)
    dt = dts[left]
    tau = dt * rng.uniform(0.05, 0.95, 24)
    P = dev.interpolate_covariances(left, dt, tau, gp_term=True)
    d, b = dev.d, dev.b
    for q in range(24):
        i = left[q]
        Lam, Psi = O.lambda_psi(d, Qc, dt[q], tau[q])
        _, Hq = O.interpolate(dev.kind, Lam, Psi, pose[i], vel[i], pose[i + 1], vel[i + 1])
        HJ = np.hstack(Hq)
        ref = HJ @ Sig[i * b:(i + 2) * b, i * b:(i + 2) * b] @ HJ.T + MM.gp_conditional(dt[q], tau[q], Qc)[:d, :d]
        s = np.sqrt(np.diag(ref))
        assert np.max(np.abs(P[q] - ref) / np.outer(s, s)) <= tol, q


def test_contract_refusal_staleness_and_no_side_effects():
    gp = gpu()
    p = _pose2_graph(12)
    dev = _device(p)
    _info(dev, 12, 9, 2)
    with pytest.raises(gp.GpslamHipError, match="column pass"):      # without the opt-in: as before
        dev.marginals()
    dev.marginals_keep_closure_columns()
    with pytest.raises(gp.GpslamHipError, match="stale"):
        dev.get_marginals()
    twin = _device(p)
    _info(twin, 12, 9, 2)
    gn(dev, 2)
    gn(twin, 2)
    D0, O0, g0, _ = dev.normal_equations()
    x0, v0 = dev.get_states()
    dev.marginals()
    S1, N1 = dev.get_marginals()
    dev.marginals()
    S2, N2 = dev.get_marginals()
    assert np.array_equal(S1, S2) and np.array_equal(N1, N2)
    D1, O1, g1, _ = dev.normal_equations()
    x1, v1 = dev.get_states()
    assert np.array_equal(D0, D1) and np.array_equal(O0, O1) and np.array_equal(g0, g1)
    assert np.array_equal(x0, x1) and np.array_equal(v0, v1)
    dev.marginals()
    gn(dev, 2)
    with pytest.raises(gp.GpslamHipError, match="stale"):
        dev.get_marginals()
    gn(twin, 2)       # ... and the two steps behind marginals() are those of a handle that never called it
    (xa, va), (xb, vb) = dev.get_states(), twin.get_states()
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    dev.marginals()
    dev.marginals_keep_closure_columns(False)      # enable = 0: the handle refuses again, what it held included
    with pytest.raises(gp.GpslamHipError, match="column pass"):
        dev.marginals()
    with pytest.raises(gp.GpslamHipError, match="column pass"):
        dev.get_marginals()
    dev.marginals_keep_closure_columns()           # ... and the call itself leaves nothing valid behind
    with pytest.raises(gp.GpslamHipError, match="stale"):
        dev.get_marginals()


def test_contract_single_pass_handles_and_fp32():
    gp = gpu()
    p = S.add_loop_closures(_anchored(_strip_landmarks(S.pose2_range_chain(60, seed=9))), [[4, 50], [55, 9]], seed=1)
    a, b = _device(p, 8), _device(p, None)
    _info(a, 2, 2, 1)
    _info(b, 2, 2, 1)
    a.marginals_keep_closure_columns()
    gn(a, 2)
    gn(b, 2)
    a.marginals()
    b.marginals()
    for u, v in zip(a.get_marginals(), b.get_marginals()):
        assert np.array_equal(u, v)
    q = S.linear_chain(50, seed=4)
    f32 = S.apply(q, gp.ChainSolver(q["kind"], precision=gp.FP32))
    f32.marginals_keep_closure_columns()
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*fp32"):
        f32.marginals()
