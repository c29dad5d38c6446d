"""References and graph recipes of tests/test_gpu_fp32_rows.py, everything that needs no GPU (tests/test_fp32_rows_refs.py checks
them on the CPU): reference rows from the 50-digit pins, the translated twin of a recorded graph, the graphs of the per-kind
comparison with their side conditions, and the update a Gauss-Newton step made, recovered from the states."""
import json
import os

import numpy as np

import rows_model as RM
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
T32 = 5e-6                # tests/cpp/fp32_math_tests.cpp: the exact derivative of Jr^-1(xi) x in float against fp64, on O(1) entries
T32_NEAR_PI = 2e-5        # ... that file's allowance for theta > 2 rad (the coefficients divide by sin theta)
QUOTIENT = 1e-6           # |h = 1e-6 quotient - derivative| for 0.2 < theta < 1.5 (tests/test_highprec_pins.py)
E32 = 2.0 * 2.0 ** -24    # rowE: an fp64 error rounded to float once
PIN_SHIFT = np.array([1e5, -2e5, 5e4])
GPS_OFFSET = np.array([0.01, -0.02, 0.03])
GPS_SIGMA = np.array([0.05, 0.08, 0.11])       # a distinct sigma per axis
MOTION3, SEED3 = 4.0, 4                        # random_chain of the POSE3 graphs: consecutive relative rotations in (0.2, 1.5) rad


def load_pins():
    """the pins, each case with its `H_exact` from the companion file"""
    with open(os.path.join(HERE, "golden", "se3_jac_pins.json")) as f:
        pins = json.load(f)
    with open(os.path.join(HERE, "golden", "se3_jac_pins_exact.json")) as f:
        exact = json.load(f)
    for fam in ("gp_prior_pose3", "interpolate_pose3"):
        assert len(exact[fam]) == len(pins[fam])
        for c, h in zip(pins[fam], exact[fam]):
            c["H_exact"] = [c["H_ref"][m] if b is None else b for m, b in enumerate(h)]      # null: H_ref's block, bit for bit
    return pins


def t32_of(theta):
    return T32_NEAR_PI if theta > 2.0 else T32


def exact_derivative(c):
    """H1..H4 of a pin as derivatives.  `H_exact` is the central difference of the reference's e at h = 1e-20, and for th^2 <= eps
    that e sits inside the reference's flat branches (rightJacobianRot3inv returns I for th^2 <= eps, Pose3utils.cpp:215-224;
    Pose3::Logmap returns the translation below 1e-10): a step of 1e-20 differentiates the branch, not the function, and misses the
    rotation coupling by O(1) (tests/test_se3_jac_pins.py:test_record_reference_minus_exact).  There -- the pins at th = 0 and 1e-9 --
    the derivative is the rounding-free h = 1e-6 quotient `H_ref`, which steps far outside the branch and whose truncation, h^2 / 6
    times a third derivative, is 1e-12 (|H_ref - H_exact| at the th = 1e-6 pins, where both are derivatives: 5e-13 .. 3e-12)."""
    return c["H_ref"] if c["theta"] ** 2 <= RM.EPS else c["H_exact"]


# ---------------------------------------------------------------- reference rows from the pins

def pin_graph(pins, cases):
    """2K states, case k on (2k, 2k + 1), as tests/test_gpu_se3_jac_pins.py:solver"""
    fl = RM.FactorLists(6)
    fl.set_qc(np.asarray(pins["Qc"]))
    fl.set_states(np.array([p for c in cases for p in (c["p1"], c["p2"])]), np.array([v for c in cases for v in (c["v1"], c["v2"])]))
    return fl


def gp_prior_graph(pins):
    cases = pins["gp_prior_pose3"]
    fl = pin_graph(pins, cases)
    fl.add_gp_priors(np.arange(0, 2 * len(cases), 2), [c["dt"] for c in cases])
    return fl


def gp_prior_rows(pins):
    """per case: (R_w [H1 H2 H3 H4]_exact (12 x 24), R_w e (12)), R_w the oracle's whitening of the pins' Qc and dt"""
    Qc = O.A(pins["Qc"])
    out = []
    for c in pins["gp_prior_pose3"]:
        R = np.zeros((12, 12))
        assert O.call("orc_gp_whitening", 6, Qc, float(c["dt"]), R) == 0
        H = np.hstack([np.asarray(h) for h in exact_derivative(c)])
        out.append((R @ H, R @ np.asarray(c["e"])))
    return out


def gps_graph(pins, sigma=GPS_SIGMA, offset=GPS_OFFSET):
    """one GPInterpolatedGPSFactorPose3 per interpolation pin, at its tau: measured = the pin's interpolated translation + offset"""
    cases = pins["interpolate_pose3"]
    fl = pin_graph(pins, cases)
    meas = np.array([np.asarray(c["e"])[9:12] + offset for c in cases])
    fl.add_interp_gps(np.arange(0, 2 * len(cases), 2), meas, np.tile(sigma, (len(cases), 1)), [c["dt"] for c in cases],
                      [c["tau"] for c in cases], None)
    return fl


def gps_rows(pins, sigma=GPS_SIGMA, offset=GPS_OFFSET, whiten=True):
    """per case: (J (3 x 24), e (3)) of the GPS factor from the pins alone.  oracle/orc_factors.c, orc_interp_gps_pose3: e = t - measured
    and de/d(pose tangent [w, v]) = [0 | R] (orc_pose3_translation), so H_m = R (rows 3..5 of interpolatePose's H_m), R the pin's
    interpolated rotation; whitened by 1 / sigma per axis."""
    w = 1.0 / np.asarray(sigma) if whiten else np.ones(3)
    out = []
    for c in pins["interpolate_pose3"]:
        R = np.asarray(c["e"])[:9].reshape(3, 3)
        J = np.hstack([R @ np.asarray(h)[3:6, :] for h in exact_derivative(c)])
        out.append((w[:, None] * J, w * (-np.asarray(offset))))
    return out


# ---------------------------------------------------------------- a recorded graph moved by a common world translation

def trans_slice(kind):
    return {O.POSE3: slice(9, 12), O.POSE2: slice(0, 2), O.LINEAR3: slice(0, 2), O.LINEAR2: slice(0, 2)}.get(kind)


def translate(kind, T):
    """edit function for FactorLists.replay: states, pose priors, landmarks, landmark priors and GPS measurements moved by T.  LINEAR3
    here is (x, y, theta) of the 2D-linear factors: x and y move, theta does not."""
    sl = trans_slice(kind)
    T = np.asarray(T, dtype=float)
    n = sl.stop - sl.start

    def edit(name, a):
        a = list(a)
        if name == "set_states":
            a[0][:, sl] += T[:n]
        elif name == "add_pose_priors":
            a[1] = a[1].reshape(len(a[0]), -1)
            a[1][:, sl] += T[:n]
        elif name == "set_landmarks":
            a[0] = a[0] + T[:a[0].shape[-1]]
        elif name == "add_landmark_priors":
            a[1] = a[1] + T[:a[1].shape[-1]]
        elif name == "add_interp_gps":
            a[1] = a[1] + T[:3]
        return tuple(a)
    return edit


def world_shift(kind):
    """1e5 m per axis"""
    sl = trans_slice(kind)
    return None if sl is None else np.array([1e5, -1e5, 1e5])[:sl.stop - sl.start]


# ---------------------------------------------------------------- the graphs of the per-kind comparison

def linear2_feed(N=40, seed=7):
    from test_gpu_forms import chain
    return chain(O.LINEAR2, N, seed=seed, vpriors=2)[2]


def meas_cases():
    from test_gpu_measurements import CASES, IDS
    return list(zip(IDS, CASES))


def meas_kwargs(kind):
    """build_meas_pair's arguments: N = 40; the POSE3 chains move fast enough that the h = 1e-6 quotient is a derivative to 1e-6"""
    return dict(N=40, seed=SEED3, motion=MOTION3) if kind == O.POSE3 else dict(N=40, seed=5)


def relative_rotations(pose):
    """|Log(R_i^T R_i+1)| of consecutive SE(3) states"""
    out = []
    for a, b in zip(pose[:-1], pose[1:]):
        R = a[:9].reshape(3, 3).T @ b[:9].reshape(3, 3)
        out.append(float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))))
    return np.array(out)


def ranged_distances(kind, fl):
    """distance of every ranged landmark from the pose it is ranged from (interpolated range: the interpolated pose, through the
    sensor; range and bearing-range: the state), at the recorded states and landmarks"""
    from test_gpu_measurements import true_range
    pose, vel = fl.args_of("set_states")[0]
    lands = fl.args_of("set_landmarks")[0][0]
    Qc = fl.args_of("set_qc")[0][0]
    d = fl.d
    out = []
    for left, lm, z, sig, dt, tau, sensor in fl.args_of("add_interp_range"):
        for i, l, h, t in zip(left, lm, dt, tau):
            Lam, Psi = O.lambda_psi(d, Qc, h, t)
            p = O.interpolate(kind, Lam, Psi, pose[i], vel[i], pose[i + 1], vel[i + 1], jac=False)[0]
            out.append(true_range(kind, p, lands[l], sensor))
    for idx, lm, z, sig in fl.args_of("add_range"):
        out += [true_range(kind, pose[i], lands[l]) for i, l in zip(idx, lm)]
    for idx, lm, bear, rng, sig in fl.args_of("add_bearing_range"):
        out += [float(np.hypot(*(lands[l] - pose[i][:2]))) for i, l in zip(idx, lm)]
    return np.array(out)


def quotient_rows(kind, m):
    """rows of a POSE3 graph whose fp64 value passes through the reference's h = 1e-6 quotient: GP priors and the interpolated factors"""
    if kind != O.POSE3:
        return np.zeros(0, dtype=int)
    keys = ["gp"] + [k for k in (0, 3, 6) if k in m.row0]
    return np.concatenate([m.rows_of(k) for k in keys])


# ---------------------------------------------------------------- comparing row tables

def row_ratio(got, ref, tol):
    """per row: max_k |got - ref|_k / (tol max_k |ref|_k); a reference row of zeros admits zeros only"""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    err, scale = np.abs(got - ref).max(axis=1), np.abs(ref).max(axis=1)
    tol = np.broadcast_to(np.asarray(tol, dtype=float), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, err / (tol * scale), np.where(err > 0, np.inf, 0.0))
    return r


def by_kind(m, ratios):
    """worst ratio per factor kind of a row map"""
    out = {}
    for key in m.row0:
        rows = m.rows_of(key)
        if len(rows):
            out[RM.MEAS_NAMES.get(key, key)] = float(ratios[rows].max())
    return out


# ---------------------------------------------------------------- the fp32 step against the handle's own rows

def step_forms():
    """(id, recipe, device kwargs, census or None) of every form of the step comparison; recipe() -> (kind, chart, feed)"""
    import test_gpu_forms as F
    out = []
    for row in F.FP32_ROWS:
        out.append((row.id, row.recipe, dict(row.dev), row.expect))
        for plan, l0 in (("unfused", "l0_rows"), ("column", "l0_column")):
            census = dict(l0_fused=0, l0_rows=0, l0_column=0)
            census[l0] = 1
            out.append(("%s-plan-%s" % (row.id, plan), row.recipe, dict(row.dev, plan=F.PLAN[plan]), census))
    out += [
        ("fp32-4-landmarks-dense-border", lambda: F.landmarks(F.N0, 4), dict(chunk=4, landmark_dim=2, precision=1), None),
        ("fp32-11-landmarks-dense-border", lambda: F.landmarks(F.N0, 11), dict(chunk=4, landmark_dim=2, precision=1), None),
        ("fp32-4-landmarks-segmented", lambda: F.landmarks(F.N0, 4), dict(chunk=4, landmark_dim=2, precision=1, force_segmented=True), None),
        ("fp32-se3-interpolated-gps", lambda: F.gps(41, 4), dict(chunk=4, precision=1), None),
    ]
    return out


def update_of(kind, chart, before, after, lm_before=None, lm_after=None):
    """the update a step applied, in the columns of the normal equations: per state [local(pose) | velocity difference], then the
    landmarks.  Linear kinds give it exactly; the others through the handle's chart."""
    (x0, v0), (x1, v1) = before, after
    if kind in (O.LINEAR2, O.LINEAR3):
        dp = x1 - x0
    else:
        dp = np.stack([O.local(kind, a, b, chart) for a, b in zip(x0, x1)])
    dx = np.hstack([dp, v1 - v0]).ravel()
    if lm_before is not None:
        dx = np.concatenate([dx, (lm_after - lm_before).ravel()])
    return dx


def scaled_step_difference(H, dx_ref, dx):
    """Jacobi-scaled 2-norm of the update difference over the scaled update"""
    s = RM.jacobi_scale(H)
    return float(np.linalg.norm(s * (dx - dx_ref)) / np.linalg.norm(s * dx_ref))
