"""gtsam::Marginals on the device (gpslam_hip_marginals) on every factor and noise model the shared assembly can hold, against dense
inverses of the oracle's H (tests/marginals_mix_model.py; DESIGN.md section 4f, "pinned on every factor and noise model").

Graphs: the five of tests/fixed_lag_mix_model.py (se2 in the first-order chart, se3, se3_vw, so3, r3; 12 to 16 states, k = 5) -- every
sigma, tau, dt, covariance, Qc, sensor offset and calibration differs from factor to factor and every kind arrives in two or three
calls --, their robust twins (Huber, Cauchy and Tukey factors on both sides of their k, Tukey factors at w = 0; one se2 case with
Geman-McClure, Welsh and Fair), SE(2) / SE(3) graphs of 60 states with robust loop closures in one pass and in column passes, handles
that carry state or border Gaussians (marginalize_head, add_state_gaussians, a slid window), and one segmented handle with losses.

Reference: np.linalg.inv of the oracle's H at the device's current states and landmarks; a robust graph as reweighted(p, w) with
w = np_loss at the whitened norms of a plain device twin's linearize_meas errors (the device's own weights are first held to those
at 1e-11, the bound of tests/test_gpu_robust.py's rows).  Every Sigma_{i,i}, Sigma_{i,i+1}, and with landmarks Sigma_LL and
Sigma_{i,L}, in correlation units at tol_of(H) = max(1e-10, 100 eps kappa_s); the last Sigma_{i,i+1} must be exactly zero.  Robust
cases add ten times the distance the reference itself moves when every acting weight is scaled by 1 + 1e-11 (both are printed).

Seen on one MI355X (worst error in correlation units; the table is in DESIGN.md section 4f): se2, so3, r3 1e-13 .. 3e-13 plain and
robust; se3 2.0e-11 plain, se3_vw 1.3e-11; robust se3 after two steps 1.07e-10 of 1.12e-10, the closest case; robust closures
2e-11 .. 1.4e-10 of 2e-9 .. 1.3e-8; the segmented handle 2.1e-11 of 2.7e-8."""
import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import synthetic as S
from oracle import oracle as O
import fixed_lag_mix_model as FM
import marginals_model as MM
import marginals_mix_model as MX
from test_gpu_marginals import tol_of, check_blocks, gn
from test_gpu_closure_passes import _info
from test_gpu_marginals_segmented import check_against_inverse, _corr

pytestmark = pytest.mark.gpu
WEIGHT_TOL = 1e-11      # the device's weights against np_loss
PROBE = 1.0 + 1e-11     # the scale of the acting weights that measures how far the reference moves with them


def device(p, onto=False, **kw):
    dev = FM.apply(p, FM.chain(p, gp.ChainSolver, **kw))
    if onto:
        dev.marginalize_head_onto_landmarks()
    return dev


def here(p, dev):
    """the description at the device's states and landmarks"""
    return MX.at(p, *MX.states_of(dev, p))


def outputs(dev, **kw):
    return dev.get_marginals(cross=True, **kw) if dev.L else dev.get_marginals(**kw)


def compare(what, dev, H, tol, first=0):
    """the outputs of the last marginals() against inv(H); the handle holds the states first .. of H"""
    out = outputs(dev)
    if first == 0:
        check_blocks(H, out[0], out[1], dev.b, tol)
    Sig = np.linalg.inv(H)
    e = MX.worst(Sig, out, first)
    print("%s: worst %.3g of tolerance %.3g (correlation units)" % (what, e, tol))
    assert e <= tol, (what, e, tol)
    return Sig


def robust_reference(what, p, dev, k_head=5, losses=FM.GRAPH_LOSSES):
    """(description at the device's states, H of the reweighted oracle there, tolerance): the device's weights against np_loss,
    check_populations, and the allowance for the weights"""
    ph = here(p, dev)
    h = device(FM.plain(ph))
    errors = FM.plain_errors(ph, h)
    h.close()
    rw = FM.robust_weights(ph, errors)
    for pre, (r, w) in rw.items():
        got = dev.meas_weights(FM.MEAS[pre][0], len(w))
        assert np.abs(got - w).max() <= WEIGHT_TOL, (pre, np.abs(got - w).max())
    FM.check_populations(ph, rw, k_head, losses)
    H = MX.H_of(FM.reweighted(ph, {pre: w for pre, (r, w) in rw.items()}))
    Hs = MX.H_of(FM.reweighted(ph, {pre: w for pre, (r, w) in FM.robust_weights(ph, errors, PROBE).items()}))
    move = MX.moved(np.linalg.inv(H), np.linalg.inv(Hs), ph["pose"].shape[0], dev.b)
    base = tol_of(H)
    print("%s: tol_of %.3g, the reference moves by %.3g when the weights move by 1e-11; %d factors at w = 0"
          % (what, base, move, sum(int((w == 0.0).sum()) for r, w in rw.values())))
    return ph, H, base + 10.0 * move


# ---------------------------------------------------------------- 1. every factor and option, plain
@pytest.mark.parametrize("name", list(FM.NS))
def test_every_factor_and_option(name):
    p = MX.graph(name)
    dev = device(p)
    done = 0
    for steps in MX.STEPS:
        gn(dev, steps - done)
        done = steps
        H = MX.H_of(here(p, dev))
        dev.marginals()
        compare("%s after %d steps" % (name, steps), dev, H, tol_of(H))


def test_marginals_leave_the_handle_as_it_was():
    """normal_equations() behind marginals(), and the next iteration, are those of a twin that never called it, to the bit"""
    p = MX.graph("se3")
    a, b = device(p), device(p)
    gn(a, 1)
    gn(b, 1)
    a.marginals()
    first = outputs(a)
    for x, y in zip(a.normal_equations(), b.normal_equations()):
        assert np.array_equal(x, y)
    a.marginals()
    for x, y in zip(first, outputs(a)):
        assert np.array_equal(x, y)
    gn(a, 1)
    gn(b, 1)
    for x, y in zip(MX.states_of(a, p), MX.states_of(b, p)):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------- 2. robust measurement factors
@pytest.mark.parametrize("name", MX.ROBUST_GRAPHS)
def test_robust_measurement_factors(name):
    p = MX.graph(name, robust=True)
    dev = device(p)
    done = 0
    for steps in MX.STEPS:
        gn(dev, steps - done)
        done = steps
        what = "robust %s after %d steps" % (name, steps)
        _, H, tol = robust_reference(what, p, dev)
        dev.marginals()
        compare(what, dev, H, tol)


def test_the_other_three_losses():
    """Geman-McClure, Welsh and Fair in the places of Huber, Cauchy and Tukey on se2: all six tabulated losses reach the marginals"""
    p = MX.swap_losses(MX.graph("se2", robust=True))
    dev = device(p)
    done = 0
    for steps in MX.STEPS:
        gn(dev, steps - done)
        done = steps
        what = "se2 with Geman-McClure, Welsh and Fair after %d steps" % steps
        _, H, tol = robust_reference(what, p, dev, losses=tuple(MX.OTHER.values()))
        dev.marginals()
        compare(what, dev, H, tol)


def test_the_form_of_the_marginals_assembly_on_robust_gps():
    """marginals() asks launch_factors for LaunchMode{}: GP priors as Jacobian rows, so no SE(3) record exists for an interpolated
    GPS factor to read and no 16-double lines are formed -- plain or robust, every GPS factor forms its own interpolation blocks
    (census meas_self), weighted by its loss.  (An iteration of a large plain graph takes the lines, of a robust one the rows that
    read the records: tests/test_gpu_robust.py.)"""
    for robust in (False, True):
        p = MX.graph("se3", robust=robust)
        dev = device(p)
        info = dev.plan_info()
        print("robust %d: plan %s" % (robust, info))
        assert info["fused"] == 0 and info["structured_gp"] == 0, info      # (13 states: an iteration takes the rows as well)
        dev.launch_census()
        dev.marginals()
        c = dev.launch_census()
        print("robust %d: census of marginals() %s" % (robust, c))
        assert c["gps_lines"] == 0 and c["meas_rec"] == 0 and c["meas_self"] == 1 and c["l0_fused"] == 0, c
        assert c["lin_rows"] + c["lin_rows_vp"] == 1 and c["lin_rec"] + c["lin_rec_vp"] == 0, c


# ---------------------------------------------------------------- 3. robust loop closures
def closure_device(p, chart, passes):
    K = len(p["closure_first"])
    dev = gp.ChainSolver(p["kind"], chart, 2 if "landmarks" in p else 0)
    if passes is not None:
        dev.set_closure_passes(32)
    S.apply(p, dev)
    dev.set_between_pairs_robust(p["closure_loss"], p["closure_k"])
    dev.compile()
    if passes is not None:
        dev.marginals_keep_closure_columns()
        _info(dev, *passes)
    else:
        _info(dev, K, K, 1)
    return dev


@pytest.mark.parametrize("name", ["pose2_5", "pose2_5_lm", "pose2_12", "pose3_6"])
def test_robust_loop_closures(name):
    """k_mg_core's -(I + J_c Z)^-1 (one pass) and k_mg_clo_inverse's M^-1 (column passes) with weighted J_c, one of them zero"""
    p, chart, passes = MX.closure_graph(name)
    dev = closure_device(p, chart, passes)
    if name == "pose2_5_lm":
        assert dev.plan_info()["R"] == 28
    gn(dev, MX.CLOSURE_STEPS)
    pose, vel = dev.get_states()
    lm = dev.get_landmarks() if dev.L else None
    r, w = MX.closure_weights(p, pose, chart)
    got = dev.between_pairs_weights(len(w))
    assert np.abs(got - w).max() <= WEIGHT_TOL, np.abs(got - w).max()
    H = MX.closure_H(MX.closure_reweighted(p, w), chart, pose, vel, lm)
    Hs = MX.closure_H(MX.closure_reweighted(p, w * PROBE), chart, pose, vel, lm)
    move = MX.moved(np.linalg.inv(H), np.linalg.inv(Hs), dev.N, dev.b)
    base = tol_of(H)
    print("%s: weights %s; tol_of %.3g, the reference moves by %.3g when the weights move by 1e-11" % (name, np.round(w, 4), base, move))
    dev.marginals()
    compare(name, dev, H, base + 10.0 * move)
    MX.check_closure_populations(p, r, w)      # (behind the comparison: a handle whose steps went elsewhere fails on its Sigma first)


# ---------------------------------------------------------------- 4. state Gaussians and a slid window
@pytest.mark.parametrize("name,k,onto,robust", MX.SCHUR)
def test_a_marginalised_head_leaves_the_covariance_of_the_rest(name, k, onto, robust):
    """the full handle, and a twin after marginalize_head(k) and compile() without a step: both against the dense inverse of the
    oracle's full H, and the twin's blocks against the full handle's at twice the tolerance"""
    p = MX.schur_case(name, k, onto, robust)
    what = "%s k = %d onto %d" % (name, k, onto)
    full, twin = device(p), device(p, onto)
    if robust:
        _, H, tol = robust_reference(what, p, full, k_head=k)
    else:
        H = MX.H_of(p)
        tol = tol_of(H)
    twin.marginalize_head(k)
    twin.compile()
    assert twin.N == full.N - k
    assert (twin.get_border_gaussians()[0].size if twin.L else 0, twin.get_state_gaussians()[0].size) == ((1, 0) if onto else (0, 1))
    full.marginals()
    Sig = compare(what + ", the full handle", full, H, tol)
    twin.marginals()
    compare(what + ", the twin", twin, H, tol, first=k)
    a, b = outputs(full, first=k), outputs(twin)
    dg = np.sqrt(np.diag(Sig))
    sx = dg[k * full.b:full.N * full.b].reshape(twin.N, full.b)
    e = max(float(np.max(np.abs(a[0] - b[0]) / (sx[:, :, None] * sx[:, None, :]))),
            float(np.max(np.abs(a[1][:-1] - b[1][:-1]) / (sx[:-1, :, None] * sx[1:, None, :]))) if twin.N > 1 else 0.0)
    if twin.L:
        sl = dg[full.N * full.b:]
        e = max(e, float(np.max(np.abs(a[2] - b[2]) / np.outer(sl, sl))), float(np.max(np.abs(a[3] - b[3]) / (sx[:, :, None] * sl[None, None, :]))))
    print("%s: the twin against the full handle %.3g" % (what, e))
    assert e <= 2 * tol


@pytest.mark.parametrize("name,onto", [("se2", True), ("se3_vw", False)])
def test_a_slid_window(name, onto):
    """marginalize_head(5) on the graph without its last two states, append_states of those two, the factors the window gains,
    compile, one step, marginals(); the reference: the oracle's H of the window plus the Lambda read back from the device"""
    p = MX.graph(name)
    N, k = FM.NS[name], 5
    dev = device(FM.window(p, 0, N - 2), onto)
    dev.marginalize_head(k)
    dev.append_states(p["pose"][N - 2:], p["vel"][N - 2:])
    new = FM.window(p, k, N, new_from=N - 2)
    assert all(len(new[key]) for key in FM.FACTOR_KEYS if key in new and key not in ("prior_idx", "vprior_idx"))
    FM.add_factors(new, dev)
    dev.compile()
    dev.iterate_gn()
    assert dev.N == N - k
    Lam = dev.get_head_prior_border()[1] if onto else dev.get_head_prior()[2]
    assert Lam.shape[0] == dev.b + (dev.L * dev.ld if onto else 0)
    H = MX.H_of(here(FM.window(p, k, N), dev), lambdas=[(0, Lam)])
    dev.marginals()
    compare("%s slid by %d" % (name, k), dev, H, tol_of(H))


def test_direct_state_gaussians():
    """add_state_gaussians on state 3 and on the last state of so3, random full-rank A"""
    p = MX.graph("so3")
    gs = MX.direct_gaussians(p)
    cols = list(zip(*gs))
    dev = device(p)
    dev.add_state_gaussians(cols[0], cols[1], cols[2], np.stack(cols[3]), np.stack(cols[4]))
    dev.compile()
    done = 0
    for steps in MX.STEPS:
        gn(dev, steps - done)
        done = steps
        H = MX.H_of(here(p, dev), gaussians=gs)
        dev.marginals()
        compare("so3 with two state Gaussians after %d steps" % steps, dev, H, tol_of(H))


# ---------------------------------------------------------------- 5. interpolated covariances
@pytest.mark.parametrize("name,robust", [("se3", False), ("so3", False), ("se3", True)])
def test_interpolated_covariances(name, robust):
    """16 queries in intervals whose GP prior carries the handle's Qc, tau / dt in [0.05, 0.95]: H_J Sigma_J H_J^T plus the GP term, as
    tests/test_gpu_marginals.py::test_lie_interpolated_covariance_against_the_oracle forms it"""
    p = MX.graph(name, robust=robust)
    dev = device(p)
    gn(dev, 2)
    what = "%s%s interpolated" % ("robust " if robust else "", name)
    if robust:
        _, H, tol = robust_reference(what, p, dev)
    else:
        H = MX.H_of(here(p, dev))
        tol = tol_of(H)
    dev.marginals()
    Sig = compare(what, dev, H, tol)
    own = np.ones(len(p["gp_left"]), dtype=bool) if "gp_qc" not in p else np.isnan(p["gp_qc"]).all(axis=(1, 2))
    assert own.sum() >= 4
    rng = np.random.default_rng(9)
    pick = rng.choice(np.nonzero(own)[0], 16)
    left, dt = p["gp_left"][pick].astype(np.int32), np.asarray(p["gp_dt"], dtype=np.float64)[pick]
    tau = dt * rng.uniform(0.05, 0.95, 16)
    P = dev.interpolate_covariances(left, dt, tau, gp_term=True)
    pose, vel = dev.get_states()
    d, b, Qc = dev.d, dev.b, p["qc"]
    worst = 0.0
    for q in range(16):
        i = left[q]
        Lam, Psi = O.lambda_psi(d, Qc, dt[q], tau[q])
        _, Hq = O.interpolate(dev.kind, Lam, Psi, pose[i], vel[i], pose[i + 1], vel[i + 1])
        HJ = np.hstack(Hq)
        ref = HJ @ Sig[i * b:(i + 2) * b, i * b:(i + 2) * b] @ HJ.T + MM.gp_conditional(dt[q], tau[q], Qc)[:d, :d]
        s = np.sqrt(np.diag(ref))
        worst = max(worst, float(np.max(np.abs(P[q] - ref) / np.outer(s, s))))
    print("%s: worst query %.3g of tolerance %.3g" % (what, worst, tol))
    assert worst <= tol


# ---------------------------------------------------------------- 6. the segmented path
def test_segmented_path_with_losses():
    """_anchored_range_chain(60) with segment_length 30 (cuts at 0, 30, 59), Huber and Cauchy in turn on its ranges: the segmented
    handle against the dense-border handle of the same graph at twice tol_of, both against the reweighted oracle"""
    p = MX.segmented_graph()
    dense = device(p)
    gn(dense, MX.SEGMENTED_STEPS)
    seg = device(p, force_segmented=True, segment_length=30)
    plan = seg.segment_plan()
    assert plan["active"] == 1 and plan["K"] == 3 and plan["C"] == 30, plan
    assert dense.segment_plan()["active"] == 0
    seg.set_states(*dense.get_states())
    seg.set_landmarks(dense.get_landmarks())
    ph, H, tol = robust_reference("segmented", p, seg, losses=(gp.chain.ROBUST_HUBER, gp.chain.ROBUST_CAUCHY))
    w = dense.meas_weights(0, len(p["range_left"]))
    assert np.array_equal(w, seg.meas_weights(0, len(w))) and (w < 1.0).sum() >= 6
    base = tol_of(H)
    dense.marginals()
    compare("the dense-border handle", dense, H, tol)
    seg.marginals_on_segments()
    seg.marginals()
    nsl, npair = check_against_inverse(seg, H, tol, p)
    assert nsl >= 60 and npair >= 8
    Sd, Sn, Slm, Sxl = dense.get_marginals(cross=True)
    Td, Tn = seg.get_marginals()
    N, ld, L = seg.N, seg.ld, seg.L
    sd = np.sqrt(np.einsum("ikk->ik", Sd))
    sl = np.sqrt(np.diag(Slm)).reshape(L, ld)
    worst = 0.0
    for i in range(N):
        worst = max(worst, _corr(Td[i], Sd[i], sd[i], sd[i]))
        if i + 1 < N:
            worst = max(worst, _corr(Tn[i], Sn[i], sd[i], sd[i + 1]))
    Tl = seg.get_landmark_marginals()
    for l in range(L):
        worst = max(worst, _corr(Tl[l], Slm[l * ld:(l + 1) * ld, l * ld:(l + 1) * ld], sl[l], sl[l]))
    print("segmented against dense border: %.3g of %.3g" % (worst, 2 * base))
    assert worst <= 2 * base
