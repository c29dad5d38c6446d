"""Loop closures past one border: column passes (gpslam_hip_set_closure_passes; closures.hpp CloPass).  More closures than the 28
right-hand sides of one pass hold go through the chain solver a slice at a time; W = U [X | Z] is kept, one workgroup solves
(I + U Z) Y = [r | 0] - U X, and a final pass adds H0^-1 U^T Y to the X of pass 0 (the algebra: tests/closure_passes_model.py).
The oracle solves the same graphs by an envelope Cholesky of the whole system, so agreement at the project's 1e-9 per step checks the
slicing, the gather, the wide solve and the final pass together.  Every test looks at closure_info() before it looks at a number."""
import numpy as np
import pytest

from oracle import oracle as O
from gpslam_amd import synthetic as S
from test_gpu_parity import gpu, states_close
from test_gpu_closure import _anchored, _lockstep_gn, _strip_landmarks

pytestmark = pytest.mark.gpu


def _pairs(N, K, seed):
    """K closures (first, second) of an N-state chain: |first - second| > 1, either order, every fourth one starting at the state
    the one before ended at"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < K:
        i, j = (int(v) for v in rng.integers(0, N, 2))
        if len(out) % 4 == 3:
            i = out[-1][1]
        if abs(i - j) > 1:
            out.append([i, j])
    assert any(a > b for a, b in out) and any(a < b for a, b in out)
    return out


def _device(p, max_passes=32, per_pass=0, chart=None, **kw):
    ld = 2 if "landmarks" in p else 0
    if chart is not None:
        kw["chart"] = chart
    dev = gpu().ChainSolver(p["kind"], landmark_dim=ld, **kw)
    if max_passes is not None:
        dev.set_closure_passes(max_passes, per_pass)
    return S.apply(p, dev)


def _pair_passes(p, max_passes=32, per_pass=0, chart=None):
    ld = 2 if "landmarks" in p else 0
    kw = {} if chart is None else dict(chart=chart)
    return S.apply(p, O.Chain(p["kind"], landmark_dim=ld, **kw)), _device(p, max_passes, per_pass, chart)


def _info(dev, closures, per_pass, passes):
    assert dev.closure_info() == dict(closures=closures, per_pass=per_pass, passes=passes, solves=passes + 1 if passes > 1 else 1)


def _pose2_base():
    return _anchored(_strip_landmarks(S.pose2_range_chain(300, seed=9)))


def _pose2_graph(K, seed=21):
    return S.add_loop_closures(_pose2_base(), _pairs(300, K, seed), seed=5)


@pytest.mark.parametrize("K,P", [(12, 2), (40, 5)])
def test_pose2_chain_beyond_one_border(K, P):
    """12 closures: two passes (9 + 3); 40: closures * d = 120, the cap, in five"""
    orc, dev = _pair_passes(_pose2_graph(K))
    _info(dev, K, 9, P)
    assert dev.plan_info()["R"] == 28
    _lockstep_gn(orc, dev, O.POSE2, 3)


@pytest.mark.parametrize("K,P", [(6, 2), (20, 5)])
def test_pose3_chain_beyond_one_border(K, P):
    p = S.add_loop_closures(S.pose3_chain(200, seed=2), _pairs(200, K, 31), seed=8)
    orc, dev = _pair_passes(p)
    _info(dev, K, 4, P)
    assert dev.plan_info()["R"] == 25 and dev.plan_info()["fused"] == 0
    _lockstep_gn(orc, dev, O.POSE3, 3)


def test_linear_chain_with_40_closures_converges_in_one_step():
    p = S.add_loop_closures(S.linear_chain(300, seed=4), _pairs(300, 40, 41), seed=9)
    orc, dev = _pair_passes(p)
    _info(dev, 40, 9, 5)
    _lockstep_gn(orc, dev, O.LINEAR3, 1)
    rc, st = dev.iterate_gn()
    assert rc == 0 and st.delta_inf_norm < 1e-9


def test_one_closure_per_pass_against_the_single_pass_path():
    """The three closures of test_gpu_closure's "mixed" case, one per pass, beside a default handle that takes all three in one:
    both within 1e-9 of the oracle over three steps.  Prints how far the two handles are from each other."""
    p = S.add_loop_closures(_anchored(_strip_landmarks(S.pose2_range_chain(200, seed=2))), [[3, 140], [199, 60], [61, 150]], seed=4)
    orc, dev = _pair_passes(p, 8, 1)
    _info(dev, 3, 1, 3)
    assert dev.plan_info()["R"] == 1 + 3
    one = _device(p, None)
    _info(one, 3, 3, 1)
    assert one.plan_info()["R"] == 1 + 9
    worst = 0.0
    for it in range(3):
        rc0, s0 = orc.iterate_gn()
        rc1, s1 = dev.iterate_gn()
        rc2, s2 = one.iterate_gn()
        assert rc0 == 0 and rc1 == 0 and rc2 == 0
        (x0, v0), (x1, v1), (x2, v2) = orc.get_states(), dev.get_states(), one.get_states()
        worst = max(worst, float(np.abs(x1 - x2).max()), float(np.abs(v1 - v2).max()))
        print("step %d: three passes vs one pass, largest state difference %.3e (oracle: %.3e / %.3e)" %
              (it, max(np.abs(x1 - x2).max(), np.abs(v1 - v2).max()), max(np.abs(x1 - x0).max(), np.abs(v1 - v0).max()),
               max(np.abs(x2 - x0).max(), np.abs(v2 - v0).max())))
        for s in (s1, s2):
            assert abs(s0.error_after - s.error_after) <= 1e-9 * max(1.0, s0.error_after), it
        states_close(O.POSE2, x0, v0, x1, v1, 1e-9)
        states_close(O.POSE2, x0, v0, x2, v2, 1e-9)
    print("three passes vs one pass over 3 steps: largest state difference %.3e" % worst)


def test_landmarks_and_closures_in_two_passes():
    """8 landmark columns leave room for 6 closures per pass: 10 closures in two.  The final pass corrects the landmark columns too,
    before their Schur complement is formed (tolerance: the existing landmarks + closures test's)."""
    p = S.add_loop_closures(_anchored(S.pose2_range_chain(400, L=4, seed=3)), _pairs(400, 10, 51), seed=7)
    orc, dev = _pair_passes(p, chart=O.CHART_FIRST_ORDER)
    _info(dev, 10, 6, 2)
    assert dev.plan_info()["R"] == 1 + 8 + 18
    _lockstep_gn(orc, dev, O.POSE2, 4, tol=1e-8, landmarks=True)


def _lm_graph():
    return S.add_loop_closures(_anchored(_strip_landmarks(S.pose2_range_chain(300, seed=6))), _pairs(300, 12, 61), seed=10)


def test_levenberg_marquardt_and_optimize():
    import lm_lockstep
    p = _lm_graph()
    orc, dev = _pair_passes(p)
    _info(dev, 12, 9, 2)
    _, _, slack = lm_lockstep.run(orc, dev, 1e-5, 6, err_tol=1e-9)
    (x0, v0), (x1, v1) = orc.get_states(), dev.get_states()
    states_close(O.POSE2, x0, v0, x1, v1, 1e-8 + 2 * slack)
    for use_lm in (0, 1):
        orc, dev = _pair_passes(p)
        _info(dev, 12, 9, 2)
        rc0, s0 = orc.optimize(O.default_params(use_lm=use_lm))
        rc1, s1 = dev.optimize(dev.default_params(use_lm=use_lm))
        assert rc0 == 0 and rc1 == 0
        print("optimize use_lm=%d: iterations %d / %d" % (use_lm, s0.iterations, s1.iterations))
        assert s0.iterations == s1.iterations, (use_lm, s0.iterations, s1.iterations)
        assert abs(s0.error_after - s1.error_after) <= 1e-9 * max(1.0, s0.error_after)


def test_run_gn_equals_single_iterations():
    p = _pose2_graph(12)
    a, b = _device(p), _device(p)
    _info(a, 12, 9, 2)
    _info(b, 12, 9, 2)
    for it in range(3):
        a.iterate_gn()
    b.run_gn(3)
    (xa, va), (xb, vb) = a.get_states(), b.get_states()
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)


def test_reruns_are_bit_identical():
    p = _pose2_graph(40)
    out = []
    for rep in range(2):
        s = _device(p)
        _info(s, 40, 9, 5)
        for it in range(2):
            rc, _ = s.iterate_gn()
            assert rc == 0
        out.append(s.get_states())
        s.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_robust_closures_reweighting_identity():
    """Huber(1.345) on all 12 closures, two of them gross outliers: one Gauss-Newton step is the step of a plain handle whose
    closure sigmas are sigma / sqrt(w), w from the library's host-side robust_eval at the oracle's closure errors (the construction
    of tests/test_gpu_robust.py), both handles in two passes."""
    from test_gpu_robust import _closure_norms
    gp = gpu()
    p = _pose2_graph(12)
    m = p["closure_meas"].copy()
    m[2, 0] += 2.0
    m[10, 1] -= 3.0
    p["closure_meas"] = m
    K, k = 12, 1.345
    r = _closure_norms(p, p["pose"], O.CHART_EXPMAP)
    w = np.array([gp.chain.robust_eval(gp.chain.ROBUST_HUBER, k, float(v))[0] for v in r])
    assert (w < 1.0).sum() >= 2 and (w == 1.0).any(), w
    q = dict(p)
    q["closure_sig"] = p["closure_sig"] / np.sqrt(w)[:, None]
    ld = 0
    rob = gp.ChainSolver(p["kind"], landmark_dim=ld)
    rob.set_closure_passes(32)
    S.apply(p, rob)
    rob.set_between_pairs_robust(np.full(K, gp.chain.ROBUST_HUBER, dtype=np.int32), np.full(K, k))
    rob.compile()
    ref = _device(q)
    _info(rob, 12, 9, 2)
    _info(ref, 12, 9, 2)
    wd = rob.between_pairs_weights(K)
    assert np.abs(wd - w).max() <= 1e-13
    rc0, s0 = rob.iterate_gn()
    rc1, s1 = ref.iterate_gn()
    assert rc0 == 0 and rc1 == 0
    states_close(p["kind"], *ref.get_states(), *rob.get_states(), 1e-9)


def test_refusals_and_the_single_pass_control():
    gp = gpu()
    base = _pose2_base()
    with pytest.raises(gp.GpslamHipError, match="closures \\* d must not exceed 120"):
        _device(S.add_loop_closures(base, _pairs(300, 41, 71), seed=1))
    p40 = S.add_loop_closures(base, _pairs(300, 40, 71), seed=1)
    with pytest.raises(gp.GpslamHipError, match="max_passes"):
        _device(p40, 2)
    with pytest.raises(gp.GpslamHipError, match="too many loop closures"):      # the default handle: as before
        _device(p40, None)
    with pytest.raises(gp.GpslamHipError, match="closures_per_pass is larger than fits"):
        _device(p40, 32, 10)
    with pytest.raises(gp.GpslamHipError, match="fp32"):
        _device(p40, 32, 0, precision=gp.FP32)
    many = _device(S.add_loop_closures(base, _pairs(300, 12, 71), seed=1))
    _info(many, 12, 9, 2)
    with pytest.raises(gp.GpslamHipError, match="column pass"):
        many.marginals()
    # positive control: a graph within one pass keeps the single-pass path whatever the setter allows
    p2 = S.add_loop_closures(base, [[4, 250], [280, 90]], seed=1)
    a, b = _device(p2, 8), _device(p2, None)
    _info(a, 2, 2, 1)
    _info(b, 2, 2, 1)
    assert a.plan_info()["R"] == 7 and b.plan_info()["R"] == 7
    for it in range(2):
        a.iterate_gn(); b.iterate_gn()
    (xa, va), (xb, vb) = a.get_states(), b.get_states()
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    a.marginals()
    Sd, Sn = a.get_marginals(0, 4)
    assert np.isfinite(Sd).all() and (np.einsum("nii->n", Sd) > 0).all()
