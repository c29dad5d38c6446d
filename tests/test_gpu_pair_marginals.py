"""Sigma_{a,b} of any two states (gpslam_hip_get_state_pair_marginals) and the chi-square gate of loop-closure candidates
(gpslam_hip_gate_between_pairs; gpslam_amd/csrc/marginals_pairs.hip) against dense inverses of the oracle's H.

Reference and tolerance are those of tests/test_gpu_marginals.py: np.linalg.inv(oracle_H(...)) and tol_of(H) = max(1e-10, 100 eps
kappa_s) in correlation units, |dSigma_rc| <= tol sigma_r sigma_c.  The gate is checked stage by stage, each against its own
reference (test_gate_stage_by_stage)."""
import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import synthetic as S
from gpslam_amd.chain import _p
from oracle import oracle as O
from test_gpu_marginals import oracle_H, tol_of, solver, gn, CHAINS, _pose2_chain, _anchored_range_chain
from test_gpu_vw import build_vw_pair
from test_gpu_closure_passes import _pairs, _device, _info
from test_gpu_closure import _anchored, _strip_landmarks

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps

SMALL = {
    "linear2": lambda N: S.linear_chain(N, D=2),
    "linear3": lambda N: S.linear_chain(N, D=3),
    "pose2": lambda N: _pose2_chain(N),
    "pose3": lambda N: S.pose3_chain(N),
    "rot3": lambda N: S.rot3_attitude_chain(N),
    "rot3_bias": lambda N: S.rot3_bias_ahrs_chain(N),
}


def pad_of(dev):
    if dev.kind != gp.ROT3_BIAS:
        return None
    return np.concatenate([np.arange(i * dev.b + 9, i * dev.b + 12) for i in range(dev.N)])


def reference(H, dev):
    Sig = np.linalg.inv(H)
    pad = pad_of(dev)
    if pad is not None:
        Sig[pad, :] = 0.0
        Sig[:, pad] = 0.0
    dg = np.sqrt(np.maximum(np.diag(Sig), 1e-300))
    dg[dg == 0] = 1.0
    return Sig, dg


def check_pairs(dev, H, pairs, tol):
    """every pair's block against inv(H) in correlation units; returns (the blocks, the worst error)"""
    a = np.array([p[0] for p in pairs], dtype=np.int32)
    c = np.array([p[1] for p in pairs], dtype=np.int32)
    Sig, dg = reference(H, dev)
    got = dev.get_state_pair_marginals(a, c)
    b = dev.b
    n = dev.N * b
    ref = Sig[:n, :n].reshape(dev.N, b, dev.N, b).transpose(0, 2, 1, 3)[a, c]
    den = dg[:n].reshape(dev.N, b)
    err = np.abs(got - ref) / (den[a][:, :, None] * den[c][:, None, :])
    worst = float(err.max())
    print("worst pair error %.2e correlation units (tol %.2e, %d pairs)" % (worst, tol, len(pairs)))
    assert worst <= tol, (pairs[int(np.argmax(err.reshape(len(pairs), -1).max(axis=1)))], worst)
    return got, worst


def all_pairs(N):
    return [(i, j) for i in range(N) for j in range(N)]


def fixed_pairs(N):
    """same chunk, neighbouring chunks, separator-interior, separator-separator, first-last, both orders, a == b"""
    ps = [(3, 9), (2, 14), (14, 17), (15, 18), (16, 5), (16, 20), (0, 16), (16, 32 if N > 32 else N - 1), (0, N - 1), (1, N - 2),
          (7, 7), (0, 0), (N - 1, N - 1), (16, 16), (4, 5), (15, 16), (16, 17), (0, 2)]
    if N > 256:
        ps += [(0, 256), (16, 256), (255, 257 if N > 257 else 256), (17, 256), (100, 240), (240, 256), (31, N - 1), (256, N - 1), (250, 256)]
    ps = [(min(a, N - 1), min(b, N - 1)) for a, b in ps]
    return ps + [(b, a) for a, b in ps]


@pytest.mark.parametrize("name", sorted(SMALL) + ["pose3_vw"])
def test_every_manifold_all_pairs(name):
    N = 40
    if name == "pose3_vw":
        orc, dev, _, _ = build_vw_pair(N, 3)
    else:
        p = SMALL[name](N)
        dev, orc = solver(p), S.apply(p, O.Chain(p["kind"]))
    gn(dev, 3)
    H = oracle_H(orc, dev)
    dev.marginals()
    got, _ = check_pairs(dev, H, all_pairs(N), tol_of(H))
    if name == "rot3_bias":        # the three pad coordinates of the velocity slot: zero rows and columns
        assert np.all(got[:, 9:, :] == 0) and np.all(got[:, :, 9:] == 0)
        assert np.any(got[:, :9, :9] != 0)


@pytest.mark.parametrize("N", [17, 33, 257, 300])
@pytest.mark.parametrize("name", ["linear3", "pose3"])
def test_lengths_across_the_partition(name, N):
    """SE(3): pose3_chain is anchored at one end only and its kappa_s grows with the length (5.8e6 at 257 states: 100 eps kappa_s is
    beyond tol_of's 1e-7 cap), so it takes a pose prior (sigma 0.1) on every 32nd state, as test_pose3_1e5_against_the_model does
    on every 64th"""
    p = dict(SMALL[name](N))
    if name == "pose3":
        idx = np.arange(0, N, 32, dtype=np.int32)
        p["prior_idx"] = idx
        p["prior_pose"] = np.ascontiguousarray(p["pose"][idx])
        p["prior_sig"] = np.full((len(idx), 6), 0.1)
        p["prior_sig"][0] = 1e-3
    dev, orc = solver(p), S.apply(p, O.Chain(p["kind"]))
    gn(dev, 2)
    H = oracle_H(orc, dev)
    dev.marginals()
    check_pairs(dev, H, fixed_pairs(N), tol_of(H))


def test_pose2_with_landmark_columns():
    """SE(2), 60 states, 4 planar landmarks: 8 border columns, + W_a S^-1 W_b^T from the kept copy"""
    p = _anchored(S.pose2_range_chain(60, L=4, seed=3))
    dev = solver(p, landmark_dim=2)
    dev.marginals_keep_pair_terms()
    orc = S.apply(p, O.Chain(O.POSE2, landmark_dim=2))
    gn(dev, 3)
    H = oracle_H(orc, dev)
    dev.marginals()
    check_pairs(dev, H, all_pairs(60)[::7] + fixed_pairs(60), tol_of(H))


@pytest.mark.parametrize("case", ["pose2", "pose3"])
def test_single_pass_closures(case):
    if case == "pose3":
        p = S.add_loop_closures(S.pose3_chain(100), [[10, 50], [40, 90], [60, 5], [99, 30]], seed=4)
    else:
        p = S.add_loop_closures(_anchored(_strip_landmarks(S.pose2_range_chain(60, seed=9))), [[2, 40], [50, 5], [10, 58], [20, 45], [0, 30]], seed=5)
    dev, orc = solver(p), S.apply(p, O.Chain(p["kind"]))
    assert dev.closure_info()["passes"] == 1
    dev.marginals_keep_pair_terms()
    gn(dev, 3)
    H = oracle_H(orc, dev, p)
    dev.marginals()
    check_pairs(dev, H, all_pairs(dev.N)[::5] + fixed_pairs(dev.N), tol_of(H))


@pytest.mark.parametrize("landmarks", [False, True])
def test_pose2_closures_in_column_passes(landmarks):
    """12 closures in two column passes (without landmarks 9 + 3; with 8 landmark columns 6 + 6), after keep_closure_columns:
    + W_a S^-1 W_b^T - Z_a M^-1 Z_b^T from mg_Y (W alone), mg_Z, mg_Minv"""
    base = S.pose2_range_chain(60, L=4, seed=3) if landmarks else _strip_landmarks(S.pose2_range_chain(60, seed=9))
    p = S.add_loop_closures(_anchored(base), _pairs(60, 12, 21), seed=5)
    dev = _device(p)
    _info(dev, 12, 6 if landmarks else 9, 2)
    dev.marginals_keep_closure_columns()
    dev.marginals_keep_pair_terms()
    orc = S.apply(p, O.Chain(p["kind"], landmark_dim=2 if landmarks else 0))
    gn(dev, 3)
    H = oracle_H(orc, dev, p)
    dev.marginals()
    check_pairs(dev, H, all_pairs(60)[::5] + fixed_pairs(60), tol_of(H))


def test_bit_rules():
    """a == b and adjacent pairs are get_marginals' blocks, Sigma_{b,a} is the transpose, reruns are identical"""
    p = S.add_loop_closures(S.pose3_chain(300), [[10, 150], [40, 220]], seed=4)
    dev = solver(p)
    dev.marginals_keep_pair_terms()
    gn(dev, 2)
    dev.marginals()
    Sd, Sn = dev.get_marginals()
    N = dev.N
    idx = np.arange(N, dtype=np.int32)
    assert np.array_equal(dev.get_state_pair_marginals(idx, idx), Sd)
    assert np.array_equal(dev.get_state_pair_marginals(idx[:-1], idx[1:]), Sn[:-1])
    assert np.array_equal(dev.get_state_pair_marginals(idx[1:], idx[:-1]), Sn[:-1].transpose(0, 2, 1))
    ps = fixed_pairs(N)
    a = np.array([q[0] for q in ps], dtype=np.int32)
    c = np.array([q[1] for q in ps], dtype=np.int32)
    X, Xt = dev.get_state_pair_marginals(a, c), dev.get_state_pair_marginals(c, a)
    ne = a != c                        # (Sigma_{a,a} is get_marginals' block as it is, which nothing symmetrises)
    assert ne.sum() >= 40 and np.array_equal(X[ne], Xt[ne].transpose(0, 2, 1))
    assert np.array_equal(X, dev.get_state_pair_marginals(a, c))
    dev.marginals()
    assert np.array_equal(X, dev.get_state_pair_marginals(a, c))


def test_contract_refusals():
    p = S.linear_chain(50, D=3)
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*fp32"):
        solver(p, precision=1).get_state_pair_marginals([0], [9])
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*sharded"):
        solver(p, force_sharded=True).get_state_pair_marginals([0], [9])
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*sharded"):
        solver(p, force_sharded=True).gate_between_pairs([0], [9], np.zeros((1, 3)), np.ones((1, 3)))
    seg = solver(_anchored_range_chain(60), landmark_dim=2, force_segmented=True)
    seg.marginals_on_segments()
    seg.marginals_keep_pair_terms()
    seg.marginals()
    seg.get_marginals()
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*get_state_pair_marginals.*segmented"):
        seg.get_state_pair_marginals([0], [9])
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*gate_between_pairs.*segmented"):
        seg.gate_between_pairs([0], [9], np.zeros((1, 3)), np.ones((1, 3)))
    dev = solver(p)                    # m = 0: works without the opt-in; stale before marginals() and after an iteration
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\).*stale"):
        dev.get_state_pair_marginals([0], [9])
    dev.marginals()
    dev.get_state_pair_marginals([0], [9])
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\).*item 1.*out of range"):
        dev.get_state_pair_marginals([0, 3], [9, 50])
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\).*item 0.*two different states"):
        dev.gate_between_pairs([4], [4], np.zeros((1, 3)), np.ones((1, 3)))
    dev.gate_between_pairs([4], [5], np.zeros((1, 3)), np.ones((1, 3)))       # adjacent states are allowed
    dev.iterate_gn()
    with pytest.raises(gp.GpslamHipError, match="stale"):
        dev.get_state_pair_marginals([0], [9])
    with pytest.raises(gp.GpslamHipError, match="stale"):
        dev.gate_between_pairs([0], [9], np.zeros((1, 3)), np.ones((1, 3)))
    # m > 0 without the opt-in: INVALID, the message names the call; the opt-in itself leaves nothing valid behind
    q = S.add_loop_closures(S.linear_chain(50, D=3), [[3, 40]], seed=1)
    clo = solver(q)
    clo.marginals()
    clo.get_marginals()
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\).*gpslam_hip_marginals_keep_pair_terms"):
        clo.get_state_pair_marginals([0], [9])
    clo.marginals_keep_pair_terms()
    with pytest.raises(gp.GpslamHipError, match="stale"):
        clo.get_state_pair_marginals([0], [9])
    clo.marginals()
    clo.get_state_pair_marginals([0], [9])
    clo.marginals_keep_pair_terms(False)
    clo.marginals()
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\).*gpslam_hip_marginals_keep_pair_terms"):
        clo.get_state_pair_marginals([0], [9])


def test_kept_copy_survives_later_calls_and_changes_nothing_else():
    """normal_equations, get_rows and error rewrite the solver's buffers between marginals() and the getter: the blocks stay, to the
    bit.  Iterations and get_marginals' outputs are bit-identical to a twin that never opted in."""
    p = dict(S.pose2_range_chain(60, L=4, seed=3))
    p = S.add_loop_closures(_anchored(p), [[2, 40], [50, 5]], seed=5)
    a, twin = solver(p, landmark_dim=2), solver(p, landmark_dim=2)
    a.marginals_keep_pair_terms()
    gn(a, 2)
    gn(twin, 2)
    a.marginals()
    twin.marginals()
    for x, y in zip(a.get_marginals(cross=True), twin.get_marginals(cross=True)):
        assert np.array_equal(x, y)
    ps = fixed_pairs(60)
    aa = np.array([q[0] for q in ps], dtype=np.int32)
    cc = np.array([q[1] for q in ps], dtype=np.int32)
    X = a.get_state_pair_marginals(aa, cc)
    a.normal_equations()
    a.get_rows()
    a.error()
    assert np.array_equal(X, a.get_state_pair_marginals(aa, cc))
    gn(a, 2)
    gn(twin, 2)
    a.run_gn(2)
    twin.run_gn(2)
    for x, y in zip(a.get_states(), twin.get_states()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.get_landmarks(), twin.get_landmarks())


# ---------------------------------------------------------------- the gate

def relative_pose(kind, x1, x2):
    """measured of a BetweenFactor whose error is zero at (x1, x2), in the library's pose layout"""
    if kind in (gp.LINEAR2, gp.LINEAR3):
        return x2 - x1
    if kind == gp.POSE2:
        c, s = np.cos(x1[2]), np.sin(x1[2])
        dx, dy = x2[0] - x1[0], x2[1] - x1[1]
        return np.array([c * dx + s * dy, -s * dx + c * dy, x2[2] - x1[2]])
    R1, R2 = x1[:9].reshape(3, 3), x2[:9].reshape(3, 3)
    return np.concatenate([(R1.T @ R2).ravel(), R1.T @ (x2[9:] - x1[9:])])


def gate_problem(case):
    if case == "linear3":
        p = S.add_loop_closures(S.linear_chain(120, D=3), [[5, 90]], seed=2)
    elif case == "pose2":
        p = S.add_loop_closures(_anchored(_strip_landmarks(S.pose2_range_chain(60, seed=9))), [[2, 40], [50, 5]], seed=5)
    else:
        p = S.add_loop_closures(S.pose3_chain(100), [[10, 50], [60, 5]], seed=4)
    dev, orc = solver(p), S.apply(p, O.Chain(p["kind"]))
    dev.marginals_keep_pair_terms()
    gn(dev, 3)
    H = oracle_H(orc, dev, p)
    dev.marginals()
    return p, dev, orc, H


@pytest.mark.parametrize("case", ["linear3", "pose2", "pose3"])
def test_gate_stage_by_stage(case):
    p, dev, orc, H = gate_problem(case)
    tol = tol_of(H)
    Sig, dg = reference(H, dev)
    pose, _ = dev.get_states()
    N, b, d, pd = dev.N, dev.b, dev.d, dev.pd
    rng = np.random.default_rng(11)
    first = np.array([3, N - 1, 17, 16, 0, 20, 31, 8], dtype=np.int32)
    second = np.array([N - 5, 2, 18, 48, N - 1, 19, 33, 40], dtype=np.int32)      # far, both orders, adjacent, separators
    n = len(first)
    # candidates: the closures' own noise level, measured = the current relative pose moved by the noise of another pair
    sig = np.tile(p["closure_sig"][0], (n, 1)) * rng.uniform(0.5, 2.0, (n, d))
    meas = np.array([relative_pose(dev.kind, pose[f], pose[s + 1 if s + 1 < N else s - 1]) for f, s in zip(first, second)])
    chi2, err, P = dev.gate_between_pairs(first, second, meas, sig)
    Spair = dev.get_state_pair_marginals(np.concatenate([first, first, second]), np.concatenate([first, second, second]))
    worst = dict(err=0.0, jac=0.0, cov=0.0, chol=0.0, end=0.0)
    for t in range(n):
        f, s = int(first[t]), int(second[t])
        e, H1, H2 = np.zeros(d), np.zeros((d, d)), np.zeros((d, d))
        O.call("orc_between_factor", int(p["kind"]), int(orc.chart), np.ascontiguousarray(meas[t], dtype=np.float64),
               np.ascontiguousarray(pose[f]), np.ascontiguousarray(pose[s]), e, H1, H2)
        # (1) err against the oracle's, 1e-11 (the project's row tolerance, relative to the row's scale)
        scale = max(1.0, np.max(np.abs(e)))
        worst["err"] = max(worst["err"], np.max(np.abs(err[t] - e)) / scale)
        assert np.max(np.abs(err[t] - e)) <= 1e-11 * scale, t
        # (2) the Jacobians behind P: P against R + [H1 H2] Sigma_dev [H1 H2]^T with the oracle's Jacobians and the device's own blocks
        HJ = np.hstack([H1, H2])
        Sdev = np.block([[Spair[t][:d, :d], Spair[n + t][:d, :d]], [Spair[n + t][:d, :d].T, Spair[2 * n + t][:d, :d]]])
        Rn = np.diag(sig[t] ** 2)
        mag = np.abs(HJ) @ np.abs(Sdev) @ np.abs(HJ).T + Rn
        djac = np.abs(P[t] - (Rn + HJ @ Sdev @ HJ.T))
        worst["jac"] = max(worst["jac"], np.max(djac / np.sqrt(np.outer(np.diag(mag), np.diag(mag)))))
        assert np.all(djac <= 1e-11 * mag), t
        # (3) innov_cov against the dense inverse, entrywise tol (|H| sigma)(|H| sigma)^T: plain correlation units of P would ignore
        # the cancellation between two strongly correlated states
        ix = np.concatenate([np.arange(f * b, f * b + d), np.arange(s * b, s * b + d)])
        Pref = Rn + HJ @ Sig[np.ix_(ix, ix)] @ HJ.T
        hs = np.abs(HJ) @ dg[ix]
        dP = tol * np.outer(hs, hs)
        worst["cov"] = max(worst["cov"], np.max(np.abs(P[t] - Pref) / np.outer(hs, hs)) / tol)
        assert np.all(np.abs(P[t] - Pref) <= dP), t
        # (4) chi2 against numpy on the device's own err and innov_cov, 100 eps cond(P) relative
        c_np = float(err[t] @ np.linalg.solve(P[t], err[t]))
        chol = abs(chi2[t] - c_np) / max(c_np, 1e-300)
        worst["chol"] = max(worst["chol"], chol / (EPS * np.linalg.cond(P[t])))
        assert chol <= 100 * EPS * np.linalg.cond(P[t]), t
        # (5) end to end against the reference's chi2 within y^T |dP| y, y = P^-1 e
        y = np.linalg.solve(Pref, e)
        c_ref = float(e @ y)
        bound = float(np.abs(y) @ dP @ np.abs(y))
        worst["end"] = max(worst["end"], abs(chi2[t] - c_ref) / max(bound, 1e-300))
        print("candidate %d (%d, %d): chi2 %.6e reference %.6e |diff| %.2e bound %.2e" % (t, f, s, chi2[t], c_ref, abs(chi2[t] - c_ref), bound))
        assert abs(chi2[t] - c_ref) <= bound, t
    print(case, "tol %.2e" % tol, "worst: err %(err).2e rel, jac %(jac).2e, cov %(cov).2e of its bound, chol %(chol).1f eps cond, end %(end).2e of the bound" % worst)
    # NULL err / innov_cov
    chi = np.zeros(n)
    meas, sig = np.ascontiguousarray(meas, dtype=np.float64), np.ascontiguousarray(sig, dtype=np.float64)
    rc = dev.lib.gpslam_hip_gate_between_pairs(dev._h, n, _p(first), _p(second), _p(meas), _p(sig), _p(chi), None, None)
    assert rc == 0 and np.array_equal(chi, chi2)


@pytest.mark.parametrize("case", ["linear3", "pose2", "pose3"])
def test_gate_consistent_candidate_passes(case):
    """measured = the current relative pose: chi2 <= |err|^2 / min sigma^2 (P >= diag(sigma^2))"""
    p, dev, orc, H = gate_problem(case)
    pose, _ = dev.get_states()
    first, second = np.array([3, dev.N - 2, 10], dtype=np.int32), np.array([dev.N - 5, 1, 11], dtype=np.int32)
    meas = np.array([relative_pose(dev.kind, pose[f], pose[s]) for f, s in zip(first, second)])
    sig = np.tile(p["closure_sig"][0], (3, 1))
    chi2, err, P = dev.gate_between_pairs(first, second, meas, sig)
    print("chi2", chi2, "|err|", np.linalg.norm(err, axis=1))
    assert np.all(np.abs(err) <= 1e-11)
    assert np.all(chi2 <= np.sum(err ** 2, axis=1) / np.min(sig ** 2, axis=1))


def test_gate_displaced_candidate_fails():
    """SE(2): measured = (current relative pose) o Exp(delta e_r), delta = k sqrt(P_rr), so that the error is -delta e_r along one
    tangent axis (a pure translation or a pure rotation: Logmap is exact there): chi2 = delta^2 (P^-1)_rr >= k^2, since
    (P^-1)_rr >= 1 / P_rr.  (On the LINEAR chains the axes decouple, P is diagonal and the inequality is an equality up to rounding.)"""
    p, dev, orc, H = gate_problem("pose2")
    pose, _ = dev.get_states()
    first, second = np.array([3, 50, 40], dtype=np.int32), np.array([55, 7, 41], dtype=np.int32)
    rel = np.array([relative_pose(dev.kind, pose[f], pose[s]) for f, s in zip(first, second)])
    sig = np.tile(p["closure_sig"][0], (3, 1))
    _, _, P = dev.gate_between_pairs(first, second, rel, sig)
    for k in (1.0, 3.0, 5.0):
        for r in range(3):
            delta = k * np.sqrt(P[:, r, r])
            meas = rel.copy()
            c, s_ = np.cos(rel[:, 2]), np.sin(rel[:, 2])
            if r == 0:
                meas[:, 0] += c * delta
                meas[:, 1] += s_ * delta
            elif r == 1:
                meas[:, 0] -= s_ * delta
                meas[:, 1] += c * delta
            else:
                meas[:, 2] += delta
            chi2, err, P2 = dev.gate_between_pairs(first, second, meas, sig)
            # the Jacobians, and with them P, move with measured on a Lie group: k is what the displacement is in units of
            # sqrt(P_rr) of the candidate as gated (delta was sized with P at the undisplaced measured)
            keff = np.abs(err[:, r]) / np.sqrt(P2[:, r, r])
            off = np.delete(err, r, axis=1)
            print("k = %g axis %d: k as gated" % (k, r), keff, "chi2", chi2, "err off the axis", np.max(np.abs(off)))
            assert np.max(np.abs(off)) <= 1e-11 * np.max(np.abs(err))
            assert np.all(np.abs(keff - k) <= 0.05 * k)
            assert np.all(chi2 >= keff * keff), (k, r, chi2, keff)
