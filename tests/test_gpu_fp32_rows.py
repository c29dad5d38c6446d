"""The fp32 mode (GPSLAM_FP32: float Jacobian rows, fp64 residual, fp64 normal equations and solver) judged where it can be wrong:
row by row against references, and step by step against the handle's own rows.  gpslam_hip_get_rows returns an fp32 handle's rows as
k_lin<float>, k_simple<float> and k_meas<float> wrote them.

  1. get_rows() of fp64 handles, assembled by tests/rows_model.py in the row order include/gpslam_hip.h documents, equals the oracle's
     normal equations at 1e-9 max(1, |.|max): the baseline, and the pin of the row order.
  2. SE(3) GP-prior rows of an fp32 handle against R_w [H1 H2 H3 H4]_exact of the 50-digit pins (tests/golden/se3_jac_pins.json, `H_exact` in se3_jac_pins_exact.json),
     every case, small rotations and the 1e-5 branch included; again with the world translation (1e5, -2e5, 5e4) added.
  3. Interpolated-GPS rows of an fp32 handle against the interpolation pins (tau = dt, -0.1 dt, 1.1 dt included), likewise.
  4. Every factor kind of an fp32 handle against the fp64 handle's rows; the same graph moved by 1e5 m per axis against the unmoved
     fp64 rows (kernels.hpp: "a Jacobian computed 1e5 m from the origin is as accurate as one computed at the origin").
  5. One iterate_gn of an fp32 handle against the dense solve of its own rows, per level-0 form and landmark path.

Bounds.  T32 = 5e-6 of a row's largest reference entry (2e-5 for pins beyond 2 rad): what tests/cpp/fp32_math_tests.cpp holds the
deepest float computation of any row to.  Rows of the fp64 reference that pass through the reference's h = 1e-6 quotient get
T32 + 1e-6, on graphs whose relative rotations lie in (0.2, 1.5) rad (asserted).  rowE, an fp64 error rounded once: 2 * 2^-24 of the
entry; on a moved graph plus the fp64 rounding of the moved coordinates, 16 * 2^-36 m (a factor touches at most 9 of them, each rounded
when it is set and again in the difference) times the row's largest Jacobian entry.  rowLR and rowM are each held to their own largest
entry.  The step: tests/test_gpu_marginals.py's max(1e-10, 100 eps kappa_s) on the Jacobi-scaled update.  Side conditions and
references are checked without a GPU in tests/test_fp32_rows_refs.py.

Pins inside the reference's flat branch (th^2 <= eps: th = 0 and 1e-9) take the rounding-free h = 1e-6 quotient `H_ref` as the
derivative, not `H_exact`: fp32_rows_refs.exact_derivative says why, tests/test_fp32_rows_refs.py checks it.

Measured (MI355X), worst ratio to the bound:
  1. 0.027 (pose3; the other graphs below 5e-6).
  2. GP prior rows by theta: 0.024 (0), 0.036 (1e-9), 0.049 (1e-6), 0.90 (9.5e-6, the |rho| = 10 pin), 0.036 (1.05e-5), 0.038 (3e-5), 0.061 (1e-4), 0.055 (1e-3), 0.084 (0.01), 0.056 (0.3), 0.085 (1.5), 0.044 (3),
     0.058 (pi - 1e-3); the moved handle: the same ratios to three digits.
  3. GPS rows by theta: 0.013 (0), 0.012 (1e-9), 0.023 (1e-6), 0.016 (9.5e-6), 0.031 (1.05e-5), 0.0075 (3e-5), 0.011 (1e-4),
     0.027 (1e-3), 0.034 (0.01), 0.28 (0.3, |rho| = 10), 0.012 (1.5), 0.014 (3), 0.0091 (pi - 1e-3); moved: the same ratios.
  4. rowLR by kind: GP prior 0.25, velocity prior 0, pose prior 0.011, between 0.012, interpolated range 0.096, range 0.066,
     attitude 0.10, GPS 0.089, odometry2d 0.017, bearing-range 0.027, projection 0.060, AHRS 0.043; rowM 0.059; rowE 0.49 (0.47 moved);
     moved rowLR / rowM: the same ratios as unmoved; error of the moved graph within 6.2e-11 relative (linear2) of the unmoved.
  5. 0.15 (SE(3) + interpolated GPS); every other form below 1.1e-3.
Every test runs in under 0.3 s.
Before the fp32 overloads of so3_log / so3_jr / so3_exp / se3_exp and of the Pose2 maps (lie.hpp) these tests measured: GP prior and
GPS rows at pi - 1e-3 7000 and 1300 times the bound (acos, then sin of that angle), GPS rows at 3e-5 and 9.5e-6 rad with tau = dt 2.1
and 1.08 (Jr = I and t = v below th = 3.4e-4), interpolated range on SE(2) 112 (1 - sin(a) / a and 1 / a - cot(a / 2) / 2 in float)."""
import numpy as np
import pytest

import fp32_rows_refs as R
import rows_model as RM
from oracle import oracle as O

pytestmark = pytest.mark.gpu
POS_ULP = 2.0 ** -36          # spacing of float64 between 2^16 and 2^17 m


def gp():
    import gpslam_amd
    return gpslam_amd


@pytest.fixture(scope="module")
def pins():
    return R.load_pins()


def chart_of(kind):
    return O.CHART_FIRST_ORDER if kind == O.POSE2 else O.CHART_EXPMAP


def fp32_handle(kind, ld=0, **kw):
    g = gp()
    return g.ChainSolver(kind, chart_of(kind), ld, precision=g.FP32, **kw)


# ---------------------------------------------------------------- the graphs of sections 1 and 4

def meas_graph_handles(kind, sensor, fp32):
    """(FactorLists, oracle, fp64 handle, fp32 handle or None) of one case of tests/test_gpu_measurements.py"""
    from test_gpu_measurements import build_meas_pair, LD
    ld = LD[kind]
    makers = (lambda: RM.FactorLists(O.TANGENT_DIM[kind], ld),) + ((lambda: fp32_handle(kind, ld),) if fp32 else ())
    orc, dev, c, extra = build_meas_pair(kind, sensor=sensor, extra_makers=makers, **R.meas_kwargs(kind))
    return extra[0], orc, dev, (extra[1] if fp32 else None)


def linear2_handles(fp32):
    g = gp()
    feed = R.linear2_feed()
    return (feed(RM.FactorLists(2)), feed(O.Chain(O.LINEAR2)), feed(g.ChainSolver(O.LINEAR2)),
            feed(fp32_handle(O.LINEAR2)) if fp32 else None)


GRAPHS = [(name, kind, sensor) for name, (kind, sensor) in R.meas_cases()] + [("linear2", O.LINEAR2, False)]


def handles(name, kind, sensor, fp32):
    return linear2_handles(fp32) if name == "linear2" else meas_graph_handles(kind, sensor, fp32)


# ---------------------------------------------------------------- 1. fp64 rows against the oracle

@pytest.mark.parametrize("name,kind,sensor", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_fp64_rows_in_the_documented_order_assemble_to_the_oracles_normal_equations(name, kind, sensor):
    fl, orc, dev, _ = handles(name, kind, sensor, False)
    rows = dev.get_rows()
    assert len(rows[1]) == fl.n_rows() == len(fl.row_map().left)
    D1, O1, g1, B1, _, _ = fl.assemble(rows)
    D0, O0, g0, B0, _, _ = orc.normal_equations()
    worst = 0.0
    for a, b in ((D0, D1), (O0, O1), (g0, g1)) + (((B0, B1),) if B0 is not None else ()):
        r = np.abs(a - b).max() / (1e-9 * max(1.0, np.abs(a).max()))
        worst = max(worst, r)
        assert r <= 1.0, (name, r)
    print("%s: %d rows, assembled fp64 rows against the oracle / bound: %.3g" % (name, len(rows[1]), worst))
    dev.close()


# ---------------------------------------------------------------- 2. and 3. fp32 rows against the pins

def pin_rows_check(dev, cases, refs, per, what):
    """per case: its `per` rows of rowLR and, as one vector, of rowE, normwise against the reference; worst ratio by theta"""
    LR, E, _, _ = dev.get_rows()
    assert LR.shape == (per * len(cases), 24)
    worst, bad = {}, []
    for k, c in enumerate(cases):
        J, e = refs[k]
        rows = slice(per * k, per * k + per)
        tol = R.t32_of(c["theta"])
        r = max(float(R.row_ratio(LR[rows], J, tol).max()), float(R.row_ratio(E[rows][None, :], e[None, :], tol).max()))
        key = "%.3g" % c["theta"]
        worst[key] = max(worst.get(key, 0.0), r)
        if not r <= 1.0:
            bad.append((k, c["theta"], c.get("tau"), c["note"], r))
    print("%s, fp32 rows / bound by theta: %s" % (what, {k: float("%.3g" % v) for k, v in worst.items()}))
    assert not bad, (what, bad)


@pytest.mark.parametrize("shifted", [False, True], ids=["at-the-origin", "1e5-m-away"])
def test_fp32_gp_prior_rows_against_the_exact_derivative_pins(pins, shifted):
    fl = R.gp_prior_graph(pins)
    dev = fl.replay(fp32_handle(O.POSE3), edit=R.translate(O.POSE3, R.PIN_SHIFT) if shifted else None)
    pin_rows_check(dev, pins["gp_prior_pose3"], R.gp_prior_rows(pins), 12, "GP prior" + (" moved" if shifted else ""))
    dev.close()


@pytest.mark.parametrize("shifted", [False, True], ids=["at-the-origin", "1e5-m-away"])
def test_fp32_interpolated_gps_rows_against_the_interpolation_pins(pins, shifted):
    fl = R.gps_graph(pins)
    dev = fl.replay(fp32_handle(O.POSE3), edit=R.translate(O.POSE3, R.PIN_SHIFT) if shifted else None)
    pin_rows_check(dev, pins["interpolate_pose3"], R.gps_rows(pins), 3, "interpolated GPS" + (" moved" if shifted else ""))
    dev.close()


# ---------------------------------------------------------------- 4. every factor kind against the fp64 rows

def check_against_fp64_rows(name, kind, fl, rows64, dev32, moved):
    m = fl.row_map()
    LR0, E0, M0, Lm0 = rows64
    LR1, E1, M1, Lm1 = dev32.get_rows()
    assert LR1.shape == LR0.shape and len(E1) == fl.n_rows()
    tol = np.full(len(E0), R.T32)
    tol[R.quotient_rows(kind, m)] += R.QUOTIENT
    ratios = {"rowLR": R.row_ratio(LR1, LR0, tol)}
    scale = np.abs(LR0).max(axis=1)
    if M0 is not None:
        assert np.array_equal(Lm0, Lm1)
        ratios["rowM"] = R.row_ratio(M1, M0, tol)
        scale = np.maximum(scale, np.abs(M0).max(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        lim = R.E32 * np.abs(E0) + (16 * POS_ULP * scale if moved else 0.0)
        ratios["rowE"] = np.where(lim > 0, np.abs(E1 - E0) / lim, np.where(E1 != E0, np.inf, 0.0))
    for what, r in ratios.items():
        print("%s%s, fp32 %s / bound by factor kind: %s" % (name, " moved" if moved else "", what,
                                                             {k: float("%.3g" % v) for k, v in R.by_kind(m, r).items()}))
    for what, r in ratios.items():
        assert r.max() <= 1.0, (name, moved, what, R.by_kind(m, r))


def moved_twin(kind, ld, fl, dev32):
    """the graph moved by 1e5 m per axis on a second fp32 handle; its fp64 error equals the unmoved one"""
    twin = fl.replay(fp32_handle(kind, ld), edit=R.translate(kind, R.world_shift(kind)))
    e0, e1 = dev32.error(), twin.error()
    print("error %.15g, moved %.15g (relative difference %.3g)" % (e0, e1, abs(e0 - e1) / e0))
    assert abs(e0 - e1) <= 1e-10 * e0
    return twin


@pytest.mark.parametrize("name,kind,sensor", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_fp32_rows_of_every_factor_kind_against_the_fp64_rows(name, kind, sensor):
    """GP prior, pose and velocity priors, interpolated range (with and without sensor), range, attitude, GPS, odometry2d,
    bearing-range (the between factor: linear2 here, every manifold in the AHRS graph and the step comparison's chains)"""
    fl, orc, dev64, dev32 = handles(name, kind, sensor, True)
    if kind == O.POSE3:
        th = R.relative_rotations(dev64.get_states()[0])
        assert 0.2 < th.min() and th.max() < 1.5, (th.min(), th.max())
    if fl.args_of("add_interp_range") or fl.args_of("add_bearing_range"):
        assert R.ranged_distances(kind, fl).min() >= 0.5
    rows64 = dev64.get_rows()
    check_against_fp64_rows(name, kind, fl, rows64, dev32, False)
    if R.trans_slice(kind) is not None:
        twin = moved_twin(kind, fl.ld, fl, dev32)
        check_against_fp64_rows(name, kind, fl, rows64, twin, True)
        twin.close()
    dev64.close(); dev32.close()


def test_fp32_rows_of_the_ahrs_graph_against_the_fp64_rows():
    """GPSLAM_ROT3_BIAS: AHRS factors, bias between factors, GP priors, pose prior, interpolated attitude (tests/test_gpu_ahrs.py)"""
    from test_gpu_ahrs import random_pair, hip_chain
    g = gp()
    orc, dev64, N, M, (fl, dev32) = random_pair(extra_makers=(lambda: RM.FactorLists(6), lambda: hip_chain(precision=g.FP32)))
    assert set(fl.meas()) == {2, 7} and len(fl.first_args("add_between")) == N - 1
    check_against_fp64_rows("ahrs", g.ROT3_BIAS, fl, dev64.get_rows(), dev32, False)
    dev64.close(); dev32.close()


def test_fp32_rows_of_the_projection_graph_against_the_fp64_rows():
    """GPInterpolatedProjectionFactorPose3 with body_P_sensor (tests/test_gpu_projection.py), and the same graph 1e5 m away"""
    from test_gpu_projection import build_pair
    g = gp()
    (fl, dev64, dev32), n = build_pair(motion=R.MOTION3, makers=(lambda: RM.FactorLists(6, 3), lambda: g.ChainSolver(O.POSE3, landmark_dim=3),
                                                                lambda: fp32_handle(O.POSE3, 3)))
    assert n > 20 and list(fl.meas()) == [6]
    th = R.relative_rotations(dev64.get_states()[0])
    assert 0.2 < th.min() and th.max() < 1.5, (th.min(), th.max())
    rows64 = dev64.get_rows()
    check_against_fp64_rows("projection", O.POSE3, fl, rows64, dev32, False)
    twin = moved_twin(O.POSE3, 3, fl, dev32)
    check_against_fp64_rows("projection", O.POSE3, fl, rows64, twin, True)
    for s in (dev64, dev32, twin):
        s.close()


# ---------------------------------------------------------------- 5. the fp32 step against the handle's own rows

@pytest.mark.parametrize("form", R.step_forms(), ids=[f[0] for f in R.step_forms()])
def test_fp32_step_is_the_dense_solve_of_the_handles_own_rows(form):
    """launch_factors runs the same k_lin / k_simple / k_meas <float> for get_rows() and for an iteration: the rows are identical, the
    float rows' consumers (k_fused_level0<0, float, 12 | 6>, k_assemble_ghost, the column plan, the dense landmark border, the
    segmented elimination) differ from numpy's float64 assembly of them in summation order only."""
    import test_gpu_forms as F
    g = gp()
    id, recipe, kw, census = form
    kind, chart, feed = recipe()
    kw = dict(kw)
    ld = kw.pop("landmark_dim", 0)
    fl = feed(RM.FactorLists(O.TANGENT_DIM[kind], ld))
    dev = feed(g.ChainSolver(kind, chart, ld, **kw))
    if kw.get("force_segmented"):
        assert dev.segment_plan()["active"]
    rows = dev.get_rows()
    before, lm0 = dev.get_states(), (dev.get_landmarks() if ld else None)
    D, Om, gr, B, HLL, gL = fl.assemble(rows, lm0)
    H = RM.dense(D, Om, B, HLL)
    rhs = gr.ravel() if B is None else np.concatenate([gr.ravel(), gL])
    tol = RM.step_tol(H)
    dev.launch_census()
    rc, st = dev.iterate_gn()
    c = dev.launch_census()
    if census is not None:
        F.check_census(c, census, id)                          # the form first, then the numbers
    assert rc == 0
    dx = R.update_of(kind, chart, before, dev.get_states(), lm0, dev.get_landmarks() if ld else None)
    r = R.scaled_step_difference(H, np.linalg.solve(H, rhs), dx)
    print("%s: level 0 fused/rows/column %d/%d/%d; scaled step difference %.3g, bound %.3g, ratio %.3g"
          % (id, c["l0_fused"], c["l0_rows"], c["l0_column"], r, tol, r / tol))
    assert r <= tol
    dev.close()
