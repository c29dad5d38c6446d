"""gtsam::Marginals on the device (gpslam_hip_marginals, gpslam_amd/csrc/marginals.hip) against dense inverses of H.

Tolerance: correlation units |S_hat - S| / sqrt(S_kk S_ll) <= max(1e-10, 100 eps kappa_s), kappa_s the condition number of the
Jacobi-scaled dense H (each test computes it).  References: H from the oracle at the device's states (D / O / B / HLL of
O.Chain.normal_equations, which already hold the closures' diagonal blocks; the closures' coupling blocks J_lo^T J_hi are added from
the oracle's own BetweenFactor Jacobians, orc_between_factor).  The chain-length sweep and the closure test on LINEAR3 take H0 from
the device's normal_equations -- the same assembly marginals() runs, pinned to the oracle by tests/test_gpu_parity.py -- and add
J_c^T J_c, whose whitened rows are -I / sigma, I / sigma."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import synthetic as S
from oracle import oracle as O
import marginals_model as MM
from test_gpu_vw import build_vw_pair

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


def dense_H(D, O_, B=None, HLL=None):
    A = MM.dense(D, O_)
    if B is None:
        return A
    N, b, nl = B.shape
    Bf = B.reshape(N * b, nl)
    return np.block([[A, Bf], [Bf.T, HLL]])


def tol_of(H):
    s = np.sqrt(np.diag(H))
    kappa = np.linalg.cond(H / np.outer(s, s))
    tol = max(1e-10, 100 * EPS * kappa)
    assert tol <= 1e-7, kappa
    return tol


def check_blocks(H, Sd, Sn, b, tol, pad=None, states=None):
    Sig = np.linalg.inv(H)
    if pad is not None:
        Sig[pad, :] = 0.0
        Sig[:, pad] = 0.0
    N = Sd.shape[0]
    dg = np.sqrt(np.maximum(np.diag(Sig), 1e-300))
    dg[dg == 0] = 1.0
    for i in (range(N) if states is None else states):
        r = slice(i * b, (i + 1) * b)
        e = np.abs(Sd[i] - Sig[r, r]) / np.outer(dg[r], dg[r])
        assert e.max() <= tol, (i, e.max())
        if i + 1 < N:
            r2 = slice((i + 1) * b, (i + 2) * b)
            e = np.abs(Sn[i] - Sig[r, r2]) / np.outer(dg[r], dg[r2])
            assert e.max() <= tol, (i, e.max())
        else:
            assert np.all(Sn[i] == 0.0)
    return Sig


def solver(p, **kw):
    return S.apply(p, gp.ChainSolver(p["kind"], **kw))


def gn(dev, k):
    for _ in range(k):
        dev.iterate_gn()


def oracle_H(orc, dev, p=None):
    """Dense H of the oracle at the device's current states (and landmarks), the closures' coupling blocks included."""
    pose, vel = dev.get_states()
    orc.set_states(pose, vel)
    if dev.L:
        orc.set_landmarks(dev.get_landmarks())
    D, O_, _, B, HLL, _ = orc.normal_equations()
    H = dense_H(D, O_, B, HLL)
    if p is not None and "closure_first" in p:
        b, d, pd = dev.b, dev.d, dev.pd
        for f, s_, m, sg in zip(p["closure_first"], p["closure_second"], p["closure_meas"], p["closure_sig"]):
            e, H1, H2 = np.zeros(d), np.zeros((d, d)), np.zeros((d, d))
            O.call("orc_between_factor", int(p["kind"]), int(orc.chart), np.ascontiguousarray(m, dtype=np.float64),
                   np.ascontiguousarray(pose[f]), np.ascontiguousarray(pose[s_]), e, H1, H2)
            J1, J2 = H1 / sg[:, None], H2 / sg[:, None]
            cpl = J1.T @ J2
            H[f * b:f * b + d, s_ * b:s_ * b + d] += cpl
            H[s_ * b:s_ * b + d, f * b:f * b + d] += cpl.T
    return H


def _pose2_chain(N):
    p = _anchored_range_chain(N)
    return {k: v for k, v in p.items() if not (k.startswith("range_") or k.startswith("lprior") or k.startswith("landmark"))}


CHAINS = {
    "linear2": lambda: S.linear_chain(200, D=2),
    "linear3": lambda: S.linear_chain(300, D=3),
    "pose2": lambda: _pose2_chain(60),
    "pose3": lambda: S.pose3_chain(200),
    "rot3": lambda: S.rot3_attitude_chain(240),
    "rot3_bias": lambda: S.rot3_bias_ahrs_chain(160),
}


@pytest.mark.parametrize("name", sorted(CHAINS) + ["pose3_vw"])
def test_chain_marginals_every_manifold(name):
    if name == "pose3_vw":      # the *Pose3VW family: velocity slot [v; w] as stored
        orc, dev, _, _ = build_vw_pair(130, 3)
        p = dict(kind=gp.POSE3)
    else:
        p = CHAINS[name]()
        dev = solver(p)
        orc = S.apply(p, O.Chain(p["kind"]))
    gn(dev, 3)
    H = oracle_H(orc, dev)
    dev.marginals()
    Sd, Sn = dev.get_marginals()
    b = dev.b
    pad = None
    if p["kind"] == gp.ROT3_BIAS:    # the three pad coordinates of the velocity slot: zero rows and columns
        pad = np.concatenate([np.arange(i * b + 9, i * b + 12) for i in range(dev.N)])
        assert np.all(Sd[:, 9:, :] == 0) and np.all(Sd[:, :, 9:] == 0) and np.all(Sn[:, 9:, :] == 0) and np.all(Sn[:, :, 9:] == 0)
    check_blocks(H, Sd, Sn, b, tol_of(H), pad=pad)


@pytest.mark.parametrize("N", [2, 3, MM.CHUNK - 1, MM.CHUNK, MM.CHUNK + 1, MM.CHUNK * MM.CHUNK + 1])
def test_chain_lengths_across_the_partition(N):
    p = S.linear_chain(N, D=3, every=3)
    dev = solver(p)
    gn(dev, 1)
    D, O_, _, _ = dev.normal_equations()
    dev.marginals()
    Sd, Sn = dev.get_marginals()
    H = dense_H(D, O_)
    check_blocks(H, Sd, Sn, dev.b, tol_of(H))


def test_long_linear3_chain_against_the_model():
    """4e4 states (four levels of chunks): the device against the numpy model of the same recursion, at every state next to a
    chunk or level boundary and a strided sample"""
    N = 40000
    dev = solver(S.linear_chain(N, D=3))
    gn(dev, 1)
    D, O_, _, _ = dev.normal_equations()
    dev.marginals()
    Sd, Sn = dev.get_marginals()
    md, mn = MM.selinv(D, O_)
    C = MM.CHUNK
    idx = set(range(0, N, 97)) | {N - 2, N - 1}
    for step in (C, C * C, C * C * C):
        for k in range(0, N, step):
            idx |= {max(k - 1, 0), k, min(k + 1, N - 1)}
    for i in sorted(idx):
        s = np.sqrt(np.diag(md[i]))
        assert np.max(np.abs(Sd[i] - md[i]) / np.outer(s, s)) <= 1e-10, i
        if i + 1 < N:
            s2 = np.sqrt(np.diag(md[i + 1]))
            assert np.max(np.abs(Sn[i] - mn[i]) / np.outer(s, s2)) <= 1e-10, i


def _anchored_range_chain(N, L=8):
    p = dict(S.pose2_range_chain(N, L=L, seed=1))
    p["prior_sig"] = np.full_like(p["prior_sig"], 1e-3)
    return p


def test_landmarks_all_four_outputs():
    """pose2_range_chain, 60 states, 8 landmarks: kappa_s = 1.2e6 (200 states: 1.1e8, beyond the 1e-7 parity bound)"""
    p = _anchored_range_chain(60)
    dev = solver(p, landmark_dim=2)
    gn(dev, 3)
    orc = S.apply(p, O.Chain(O.POSE2, landmark_dim=2))
    pose, vel = dev.get_states()
    orc.set_states(pose, vel)
    orc.set_landmarks(dev.get_landmarks())
    D, O_, _, B, HLL, _ = orc.normal_equations()
    dev.marginals()
    Sd, Sn, Slm, Sxl = dev.get_marginals(cross=True)
    H = dense_H(D, O_, B, HLL)
    tol = tol_of(H)
    Sig = check_blocks(H, Sd, Sn, dev.b, tol)
    n = dev.N * dev.b
    dg = np.sqrt(np.diag(Sig))
    assert np.max(np.abs(Slm - Sig[n:, n:]) / np.outer(dg[n:], dg[n:])) <= tol
    Sxl_ref = Sig[:n, n:].reshape(dev.N, dev.b, -1)
    assert np.max(np.abs(Sxl - Sxl_ref) / np.outer(dg[:n], dg[n:]).reshape(Sxl.shape)) <= tol


@pytest.mark.parametrize("sigma,pairs", [(None, [[3 + 30 * k, 40 + 30 * k] for k in range(9)]), (1e-4, [[20, 250]])])
def test_linear3_closures(sigma, pairs):
    p = S.add_loop_closures(S.linear_chain(300, D=3), pairs, sigma=None if sigma is None else np.full(3, sigma))
    dev = solver(p)
    gn(dev, 1)
    D, O_, _, _ = dev.normal_equations()       # H0: the chain without the closures
    H = dense_H(D, O_)
    b, d = dev.b, dev.d
    for a, c, sg in zip(p["closure_first"], p["closure_second"], p["closure_sig"]):
        J = np.zeros((d, H.shape[0]))
        J[:, a * b:a * b + d] = -np.diag(1.0 / sg)
        J[:, c * b:c * b + d] = np.diag(1.0 / sg)
        H += J.T @ J
    dev.marginals()
    Sd, Sn = dev.get_marginals()
    check_blocks(H, Sd, Sn, b, tol_of(H))


def test_interpolated_covariance_linear3():
    p = S.linear_chain(120, D=3)
    dev = solver(p)
    gn(dev, 1)
    D, O_, _, _ = dev.normal_equations()
    Sig = np.linalg.inv(dense_H(D, O_))
    dev.marginals()
    rng = np.random.default_rng(5)
    left = rng.integers(0, dev.N - 1, 64).astype(np.int32)
    dt = np.full(64, 0.1)
    tau = rng.uniform(0.0, 0.1, 64)
    P = dev.interpolate_covariances(left, dt, tau)
    P0 = dev.interpolate_covariances(left, dt, tau, gp_term=False)
    _, Hj = dev.interpolate_poses_jac(left, dt, tau)
    b = dev.b
    for q in range(64):
        i = left[q]
        HJ = np.hstack(list(Hj[q]))
        SJ = Sig[i * b:(i + 2) * b, i * b:(i + 2) * b]
        ref0 = HJ @ SJ @ HJ.T
        ref = ref0 + MM.gp_c(dt[q], tau[q]) * p["qc"]
        s = np.sqrt(np.diag(ref))
        assert np.max(np.abs(P[q] - ref) / np.outer(s, s)) <= 1e-9
        s0 = np.sqrt(np.diag(ref0))
        assert np.max(np.abs(P0[q] - ref0) / np.outer(s0, s0)) <= 1e-9


def test_refusals_and_staleness():
    p = S.linear_chain(50, D=3)
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*fp32"):
        solver(p, precision=1).marginals()
    q = dict(p)
    for k in ("prior_idx", "prior_pose", "prior_sig", "vprior_idx", "vprior", "vprior_sig"):
        q.pop(k)
    with pytest.raises(gp.GpslamHipError, match=r"\(-3\)"):
        solver(q).marginals()
    dev = solver(p)
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\).*stale"):
        dev.get_marginals()
    dev.marginals()
    dev.get_marginals()
    dev.iterate_gn()
    with pytest.raises(gp.GpslamHipError, match="stale"):
        dev.get_marginals()
    dev.marginals()
    dev.set_qc(p["qc"])
    with pytest.raises(gp.GpslamHipError, match="stale"):
        dev.interpolate_covariances([0], [0.1], [0.05])
    dev.marginals()
    pose, vel = dev.get_states()
    dev.set_states(pose, vel)
    with pytest.raises(gp.GpslamHipError, match="stale"):
        dev.get_marginals()
    lp = _anchored_range_chain(60)
    seg = solver(lp, landmark_dim=2, force_segmented=True)
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*segmented"):
        seg.marginals()


def test_no_side_effects_and_determinism():
    p = S.pose3_chain(300)
    a, b = solver(p), solver(p)
    gn(a, 2)
    gn(b, 2)
    D0, O0, g0, _ = a.normal_equations()
    a.marginals()
    S1, N1 = a.get_marginals()
    a.marginals()
    S2, N2 = a.get_marginals()
    assert np.array_equal(S1, S2) and np.array_equal(N1, N2)
    D1, O1, g1, _ = a.normal_equations()
    assert np.array_equal(D0, D1) and np.array_equal(O0, O1) and np.array_equal(g0, g1)
    gn(a, 2)
    gn(b, 2)
    a.run_gn(3)
    b.run_gn(3)
    pa, va = a.get_states()
    pb, vb = b.get_states()
    assert np.array_equal(pa, pb) and np.array_equal(va, vb)


def test_pose3_1e5_against_the_model():
    """Scale: config 3's chain at 1e5 states, with a pose prior (sigma 0.1) on every 64th state so that its marginals stay bounded,
    against the model's recursion (numpy inverses in place of the kernels' Gauss-Jordan).  config 3 itself is anchored at one
    end only: its kappa_s grows with the length (oracle H after one GN step: 7.3e5 at 100 states, 4.1e6 at 200, 1.2e7 at 400, so
    100 eps kappa_s = 2.8e-7 already at 400 states and about 2e-2 at 1e5 by the same growth), and there the two roundings part by
    1e-7 at state 1.4e4 and 2e-5 at 6e4 in correlation units -- inside 100 eps kappa_s, but beyond the 1e-7 parity bound."""
    N = 100000
    p = dict(S.pose3_chain(N))
    idx = np.arange(0, N, 64, dtype=np.int32)
    p["prior_idx"] = idx
    p["prior_pose"] = np.ascontiguousarray(p["pose"][idx])
    p["prior_sig"] = np.full((len(idx), 6), 0.1)
    p["prior_sig"][0] = 1e-3
    dev = solver(p)
    gn(dev, 1)
    D, O_, _, _ = dev.normal_equations()
    dev.marginals()
    Sd, Sn = dev.get_marginals()
    md, mn = MM.selinv(D, O_)
    for i in list(range(0, N, 997)) + [N - 1]:
        s = np.sqrt(np.diag(md[i]))
        assert np.max(np.abs(Sd[i] - md[i]) / np.outer(s, s)) <= 1e-9, i
        if i + 1 < N:
            s2 = np.sqrt(np.diag(md[i + 1]))
            assert np.max(np.abs(Sn[i] - mn[i]) / np.outer(s, s2)) <= 1e-9, i


@pytest.mark.parametrize("case", ["pose3_4", "pose2_landmarks_R28"])
def test_closures_against_the_oracle(case):
    """4 closures on SE(3); SE(2) with 5 closures AND 6 landmarks: R = 1 + 6 * 2 + 5 * 3 = 28, every border column in use --
    K holds both S^-1 and -(I + J_c Z)^-1, and S is formed from the closure-corrected landmark columns"""
    if case == "pose3_4":
        p = S.add_loop_closures(S.pose3_chain(300), [[10, 150], [40, 220], [60, 290], [100, 250]], seed=4)
        dev, orc = solver(p), S.apply(p, O.Chain(O.POSE3))
    else:
        p = dict(S.pose2_range_chain(60, L=6, seed=1))
        p["prior_sig"] = np.full_like(p["prior_sig"], 1e-3)
        p = S.add_loop_closures(p, [[2, 40], [5, 50], [10, 58], [20, 45], [0, 30]], seed=5)
        dev, orc = solver(p, landmark_dim=2), S.apply(p, O.Chain(O.POSE2, landmark_dim=2))
        assert dev.plan_info()["R"] == 28
    gn(dev, 3)
    H = oracle_H(orc, dev, p)
    tol = tol_of(H)
    dev.marginals()
    Sd, Sn, Slm, Sxl = dev.get_marginals(cross=True)
    Sig = check_blocks(H, Sd, Sn, dev.b, tol)
    if dev.L:
        n = dev.N * dev.b
        dg = np.sqrt(np.diag(Sig))
        assert np.max(np.abs(Slm - Sig[n:, n:]) / np.outer(dg[n:], dg[n:])) <= tol
        ref = Sig[:n, n:].reshape(dev.N, dev.b, -1)
        assert np.max(np.abs(Sxl - ref) / np.outer(dg[:n], dg[n:]).reshape(Sxl.shape)) <= tol


def test_gp_interpolated_covariance_is_the_inserted_knots_marginal():
    """LINEAR3, gp_term = 1: P(tau) must equal the marginal of a knot inserted at t_i + tau -- the interval split into two GP
    priors (tau, dt - tau), no other factor on it.  Independent of the closed form c(dt, tau)."""
    N, i, dt = 40, 17, 0.1
    p = S.linear_chain(N, D=3, every=5)
    dev = solver(p)
    dev.marginals()
    for tau in (0.037, 0.011, 0.089):
        q = dict(p)
        q["N"] = N + 1
        q["pose"] = np.insert(p["pose"], i + 1, p["pose"][i], axis=0)
        q["vel"] = np.insert(p["vel"], i + 1, p["vel"][i], axis=0)
        q["gp_left"] = np.arange(N, dtype=np.int32)
        q["gp_dt"] = np.concatenate([p["gp_dt"][:i], [tau, dt - tau], p["gp_dt"][i + 1:]])
        q["prior_idx"] = np.where(p["prior_idx"] > i, p["prior_idx"] + 1, p["prior_idx"]).astype(np.int32)
        knot = solver(q)
        knot.marginals()
        ref = knot.get_marginals(first=i + 1, count=1)[0][0][:3, :3]
        P = dev.interpolate_covariances([i], [dt], [tau])[0]
        s = np.sqrt(np.diag(ref))
        assert np.max(np.abs(P - ref) / np.outer(s, s)) <= 1e-9, tau


@pytest.mark.parametrize("kind", ["pose3", "rot3", "pose3_vw"])
def test_lie_interpolated_covariance_against_the_oracle(kind):
    """P(tau) = H_J Sigma_J H_J^T + (Q(tau) - Psi Phi(dt - tau) Q(tau))_pose with H_J from the oracle's interpolatePose Jacobians
    (VW: through the world-velocity chain rule; there the GP term is not checked, gp_term = 0) and Sigma from the oracle's H"""
    if kind == "pose3_vw":
        orc, dev, c, Qc = build_vw_pair(130, 3)
        dts = np.asarray(c["dt"], dtype=np.float64)
    else:
        p = S.pose3_chain(120) if kind == "pose3" else S.rot3_attitude_chain(120)
        dev, orc = solver(p), S.apply(p, O.Chain(p["kind"]))
        Qc, dts = p["qc"], np.asarray(p["gp_dt"], dtype=np.float64)
    gn(dev, 3)
    H = oracle_H(orc, dev)
    tol = tol_of(H)
    Sig = np.linalg.inv(H)
    dev.marginals()
    pose, vel = dev.get_states()
    rng = np.random.default_rng(9)
    left = rng.integers(0, dev.N - 1, 24).astype(np.int32)
    dt = dts[left]
    tau = dt * rng.uniform(0.05, 0.95, 24)
    gpt = kind != "pose3_vw"
    P = dev.interpolate_covariances(left, dt, tau, gp_term=gpt)
    d, b = dev.d, dev.b
    for q in range(24):
        i = left[q]
        Lam, Psi = O.lambda_psi(d, Qc, dt[q], tau[q])
        if kind == "pose3_vw":
            _, H = O.interpolate_vw(Lam, Psi, pose[i], vel[i, :3], vel[i, 3:], pose[i + 1], vel[i + 1, :3], vel[i + 1, 3:])
        else:
            _, H = O.interpolate(dev.kind, Lam, Psi, pose[i], vel[i], pose[i + 1], vel[i + 1])
        HJ = np.hstack(H)
        ref = HJ @ Sig[i * b:(i + 2) * b, i * b:(i + 2) * b] @ HJ.T
        if gpt:
            ref = ref + MM.gp_conditional(dt[q], tau[q], Qc)[:d, :d]
        s = np.sqrt(np.diag(ref))
        assert np.max(np.abs(P[q] - ref) / np.outer(s, s)) <= tol, q


def test_sharded_handle_is_refused():
    p = S.linear_chain(50, D=3)
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*sharded"):
        solver(p, force_sharded=True).marginals()


# ---------------------------------------------------------------- staleness is total

def _entry_points():
    """every function include/gpslam_hip.h declares, without the gpslam_hip_ prefix"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gpslam_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return sorted(set(re.findall(r"\bgpslam_hip_([a-z0-9_]+)\s*\(", text)))


def _small_graph():
    """SE(2), 5 states, one landmark seen from the intervals behind states 1, 2, 3, one closure (1, 4): state 0 alone can be a head"""
    p = _anchored_range_chain(5, L=1)
    left = np.array([1, 2, 3], dtype=np.int32)
    z = np.linalg.norm(p["landmark_truth"][0] - p["truth"][left, :2], axis=1)
    p.update(range_left=left, range_lm=np.zeros(3, dtype=np.int32), range_z=z, range_sigma=np.full(3, 0.5), range_dt=np.full(3, 0.1),
             range_tau=np.full(3, 0.05))
    return S.add_loop_closures(p, [[1, 4]])


def _small_handle(p):
    dev = solver(p, landmark_dim=2)
    dev.marginals_keep_pair_terms()
    dev.marginals()
    return dev


def _raw(name, *args):
    """the entry point itself, its status ignored: a local handle is refused by the calls of a caller-owned loop"""
    return lambda d, p: getattr(d.lib, "gpslam_hip_" + name)(d._h, *args)


# Column one: the entry points that change what Sigma depends on (states, landmarks, factors, noise models, Qc, the kept terms) -- after
# any of them the getters answer "stale".  The value is the call on the small graph, or None where that graph cannot make it: factors
# of other manifolds, and the phases of the sharded handle, of a split piece and of the segmented path's caller-owned loop
# (iterate_phase1, fs_set_split, fs_phase1, fs_lm_trial_phase1).
_EYE = lambda n: np.eye(n)[None]
_CHANGES_SIGMA = {
    "set_states": lambda d, p: d.set_states(*d.get_states()),
    "set_halo_state": lambda d, p: d.set_halo_state(p["pose"][0], p["vel"][0]),
    "set_landmarks": lambda d, p: d.set_landmarks(d.get_landmarks()),
    "set_qc": lambda d, p: d.set_qc(p["qc"]),
    "add_gp_priors": lambda d, p: d.add_gp_priors([0], [0.1]),
    "add_gp_priors_qc": lambda d, p: d.add_gp_priors_qc([0], [0.1], p["qc"][None]),
    "add_pose_priors": lambda d, p: d.add_pose_priors([2], p["pose"][2:3], np.ones((1, 3))),
    "add_vel_priors": lambda d, p: d.add_vel_priors([2], p["vel"][2:3], np.ones((1, 3))),
    "add_between": lambda d, p: d.add_between([0], p["between_meas"][:1], p["between_sig"][:1]),
    "add_between_pairs": lambda d, p: d.add_between_pairs([2], [4], p["closure_meas"], p["closure_sig"]),
    "add_landmark_priors": lambda d, p: d.add_landmark_priors([0], p["lprior"], p["lprior_sig"]),
    "add_interp_range": lambda d, p: d.add_interp_range([2], [0], p["range_z"][1:2], [0.5], [0.1], [0.02]),
    "add_range": lambda d, p: d.add_range([2], [0], p["range_z"][1:2], [0.5]),
    "set_meas_covariance": lambda d, p: d.set_meas_covariance(gp.chain.MEAS_INTERP_RANGE, np.array([0.3])),
    "set_meas_robust": lambda d, p: d.set_meas_robust(gp.chain.MEAS_INTERP_RANGE, [gp.chain.ROBUST_HUBER], 1.0),
    "set_between_pairs_robust": lambda d, p: d.set_between_pairs_robust([gp.chain.ROBUST_HUBER], 1.0),
    "set_closure_passes": lambda d, p: d.set_closure_passes(4, 1),
    "add_state_gaussians": lambda d, p: d.add_state_gaussians([2], p["pose"][2], p["vel"][2], _EYE(6), np.zeros(6)),
    "add_border_gaussians": lambda d, p: d.add_border_gaussians([2], p["pose"][2], p["vel"][2], p["landmarks"], _EYE(8), np.zeros(8)),
    "marginalize_head": lambda d, p: d.marginalize_head(1),
    "append_states": lambda d, p: d.append_states(p["pose"][-1:], p["vel"][-1:]),
    "clear_factors": lambda d, p: d.clear_factors(),
    "compile": lambda d, p: d.compile(),
    "iterate_gn": lambda d, p: d.iterate_gn(),
    "run_gn": lambda d, p: d.run_gn(1),
    "iterate_lm": lambda d, p: d.iterate_lm(1e-3),
    "optimize": lambda d, p: d.optimize(),
    "lm_trial_phase1": _raw("lm_trial_phase1", C.c_double(1e-3)),
    "lm_reject": _raw("lm_reject"),
    "marginals_keep_closure_columns": lambda d, p: d.marginals_keep_closure_columns(),
    "marginals_on_segments": lambda d, p: d.marginals_on_segments(),
    "marginals_keep_pair_terms": lambda d, p: d.marginals_keep_pair_terms(),
    "add_interp_attitude": None, "add_ahrs": None, "add_interp_gps": None, "add_interp_projection": None, "add_interp_projection_ds2": None,
    "add_odometry2d": None, "add_bearing_range": None,
    "iterate_phase1": None, "fs_set_split": None, "fs_phase1": None, "fs_lm_trial_phase1": None,
}
# Column two: everything else -- the blocks of the last marginals() stay what they were, to the bit.  (error and lm_begin read the
# estimate and move nothing.)  None: not a call on this handle, or one the small graph cannot make
_LEAVES_SIGMA = {
    "get_states": lambda d, p: d.get_states(),
    "get_landmarks": lambda d, p: d.get_landmarks(),
    "closure_info": lambda d, p: d.closure_info(),
    "get_meas_weights": lambda d, p: d.meas_weights(gp.chain.MEAS_INTERP_RANGE, 3),
    "get_between_pairs_weights": lambda d, p: d.between_pairs_weights(1),
    "get_state_gaussians": lambda d, p: d.get_state_gaussians(),
    "get_border_gaussians": lambda d, p: d.get_border_gaussians(),
    "marginalize_head_onto_landmarks": lambda d, p: d.marginalize_head_onto_landmarks(),
    "linearize_gp": lambda d, p: d.linearize_gp(),
    "linearize_meas": lambda d, p: d.linearize_meas(gp.chain.MEAS_INTERP_RANGE, 3),
    "error": lambda d, p: d.error(),
    "normal_equations": lambda d, p: d.normal_equations(),
    "get_rows": lambda d, p: d.get_rows(),
    "interpolate_poses": lambda d, p: d.interpolate_poses([1], [0.1], [0.05]),
    "interpolate_poses_jac": lambda d, p: d.interpolate_poses_jac([1], [0.1], [0.05]),
    "marginals": lambda d, p: d.marginals(),
    "get_marginals": lambda d, p: d.get_marginals(cross=True),
    "get_landmark_marginals": lambda d, p: d.get_landmark_marginals(),
    "get_state_landmark_marginals": lambda d, p: d.get_state_landmark_marginals([2], [0]),
    "get_landmark_pair_marginals": lambda d, p: d.get_landmark_pair_marginals([0], [0]),
    "get_state_pair_marginals": lambda d, p: d.get_state_pair_marginals([0], [3]),
    "gate_between_pairs": lambda d, p: d.gate_between_pairs([0], [3], p["closure_meas"], p["closure_sig"]),
    "interpolate_covariances": lambda d, p: d.interpolate_covariances([1], [0.1], [0.05]),
    "plan_info": lambda d, p: d.plan_info(),
    "launch_census": lambda d, p: d.launch_census(),
    "segment_plan": lambda d, p: d.segment_plan(),
    "last_timing": lambda d, p: d.last_timing(),
    "last_level0_ms": lambda d, p: d.last_level0_ms(),
    "set_level0_stamps": lambda d, p: d.set_level0_stamps(False),
    "last_error": lambda d, p: d.lib.gpslam_hip_last_error(d._h),
    "stream": lambda d, p: d.stream(),
    "lm_begin": _raw("lm_begin"),
    "lm_trial_phase2": _raw("lm_trial_phase2", None),
    "abi_version": None, "struct_size": None, "create": None, "create_v2": None, "destroy": None, "default_params": None, "lm_decide": None,
    "robust_eval": None, "set_stream": None, "set_collectives": None, "get_head_prior": None, "get_head_prior_border": None,
    "block_tridiag_solve": None, "interpolate_velocities": None, "body_centric_velocity": None, "time_kernel": None,
    "interface_send": None, "interface_recv": None, "iterate_phase2": None, "iterate_phase2a": None, "iterate_phase2b": None,
    "landmark_reduce_buffer": None, "fs_split_info": None, "fs_set_top": None, "fs_interface": None, "fs_phase2": None, "fs_lm_trial_phase2": None,
}


def test_every_entry_point_is_classified():
    """The header's entry points, each in exactly one column: a new one fails here until it is classified."""
    names = _entry_points()
    assert len(names) > 90 and "marginals" in names and "abi_version" in names
    assert not set(_CHANGES_SIGMA) & set(_LEAVES_SIGMA)
    assert sorted(set(_CHANGES_SIGMA) | set(_LEAVES_SIGMA)) == names


@pytest.mark.parametrize("name", sorted(k for k, v in _CHANGES_SIGMA.items() if v is not None))
def test_staleness_is_total(name):
    p = _small_graph()
    dev = _small_handle(p)
    dev.get_marginals(cross=True)
    _CHANGES_SIGMA[name](dev, p)
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\).*stale"):
        dev.get_marginals()


def test_other_entry_points_leave_the_marginals_alone():
    p = _small_graph()
    dev = _small_handle(p)
    ref = dev.get_marginals(cross=True)
    for name in sorted(k for k, v in _LEAVES_SIGMA.items() if v is not None):
        _LEAVES_SIGMA[name](dev, p)
        now = dev.get_marginals(cross=True)
        assert all(np.array_equal(a, b) for a, b in zip(ref, now)), name


# ---------------------------------------------------------------- destroy frees

def _free_bytes():
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert gp.chain.load_library().hipMemGetInfo(C.byref(free), C.byref(total)) == 0     # (the HIP runtime the library itself is linked to)
    return free.value


def test_destroy_frees_the_device_memory():
    """A handle's whole life, again and again: the device's free memory after ten cycles is lower than after the first by less than half
    of what one handle holds (Z alone: mg_zrows(N, b) rows of 16 doubles, 15 MB).  A condition on gross leaks, not a tolerance."""
    N = 20000
    p = S.add_loop_closures(_pose2_chain(N), [[100, 5000], [2000, 12000], [7000, 19000], [300, 15000], [9000, 9500]])

    def cycle():
        dev = gp.ChainSolver(p["kind"])
        dev.set_closure_passes(8, 2)
        S.apply(p, dev)
        assert dev.closure_info()["passes"] == 3
        dev.marginals_keep_closure_columns()
        dev.marginals_keep_pair_terms()
        dev.marginals()
        dev.get_state_pair_marginals([3], [15000])
        inside = _free_bytes()
        dev.close()
        return inside

    cycle()
    free_warm = _free_bytes()
    footprint = free_warm - cycle()
    for _ in range(9):
        cycle()
    lost = free_warm - _free_bytes()
    print("footprint %d bytes, lost after ten cycles %d bytes" % (footprint, lost))
    assert footprint >= (N * 6 + 16) * 16 * 8
    assert lost < footprint / 2
