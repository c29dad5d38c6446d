"""gtsam::Marginals on the segmented landmark path (gpslam_hip_marginals_on_segments, gpslam_amd/csrc/marginals_fs.hip) against dense
inverses of the oracle's H at the device's states, and against the dense-border handle of the same graph where one exists.

Tolerance: tol_of(H) of tests/test_gpu_marginals.py, max(1e-10, 100 eps kappa_s) in correlation units with its cap of 1e-7.
S.pose2_local_landmarks_chain as generated has kappa_s = 1-7e8, beyond the cap, so the local-landmark cases soften a copy of its
parameters (qc x 100, between sigma 0.05, range sigma 0.05, pose prior sigma 1e-2: kappa_s = 5e5 .. 1.4e6) and call marginals() at the
initial estimate, without iterations: Gauss-Newton does not settle on the softened graph, and the marginals do not need it to.

State-landmark and landmark-landmark blocks are served for neighbouring fat blocks only, and the plan does not say which landmark
sits where: the tests ask for every pair of their lists one by one, compare what is served and require that every pair of a state
and a landmark it observes IS served (the attachment rule)."""
import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import synthetic as S
from oracle import oracle as O
from test_gpu_marginals import tol_of, oracle_H, solver, gn, _anchored_range_chain

pytestmark = pytest.mark.gpu


def _soft(N, L, window):
    p = dict(S.pose2_local_landmarks_chain(N, L=L, window=window))
    p["qc"] = p["qc"] * 100.0
    p["between_sig"] = np.full_like(p["between_sig"], 0.05)
    p["range_sigma"] = np.full_like(p["range_sigma"], 0.05)
    p["prior_sig"] = np.full_like(p["prior_sig"], 1e-2)
    return p


def _cuts(N, C):
    """FatSepPlan::make_cuts"""
    c = list(range(0, N - 1, C))
    if c[-1] != N - 1:
        c.append(N - 1)
    if len(c) >= 3 and c[-1] - c[-2] < 2:
        del c[-2]
    return c


def _corr(a, ref, dr, dc):
    return float(np.max(np.abs(a - ref) / np.outer(dr, dc)))


def _served(call, *args):
    try:
        return call(*args)[0]
    except gp.GpslamHipError as ex:
        assert "(-1)" in str(ex) and "fat block" in str(ex), str(ex)
        return None


def check_against_inverse(dev, H, tol, p, states=None, lm_reach=12):
    """S, S_next at every state; every landmark block; the state-landmark blocks of `states` (default: all) with every landmark;
    landmark pairs up to lm_reach apart in index.  Returns the number of state-landmark and landmark-pair blocks served."""
    N, b, ld, L = dev.N, dev.b, dev.ld, dev.L
    n = N * b
    Sig = np.linalg.inv(H)
    dg = np.sqrt(np.diag(Sig))
    Sd, Sn = dev.get_marginals()
    worst = 0.0
    for i in range(N):
        r = slice(i * b, (i + 1) * b)
        worst = max(worst, _corr(Sd[i], Sig[r, r], dg[r], dg[r]))
        if i + 1 < N:
            r2 = slice((i + 1) * b, (i + 2) * b)
            worst = max(worst, _corr(Sn[i], Sig[r, r2], dg[r], dg[r2]))
    assert np.all(Sn[N - 1] == 0.0)
    lms = lambda l: slice(n + l * ld, n + (l + 1) * ld)
    Sl = dev.get_landmark_marginals()
    for l in range(L):
        worst = max(worst, _corr(Sl[l], Sig[lms(l), lms(l)], dg[lms(l)], dg[lms(l)]))
    observed = set()
    if "range_left" in p:
        for s_, l in zip(p["range_left"], p["range_lm"]):
            observed |= {(int(s_), int(l)), (int(s_) + 1, int(l))}
    nsl = npair = 0
    for i in (range(N) if states is None else states):
        r = slice(i * b, (i + 1) * b)
        for l in range(L):
            blk = _served(dev.get_state_landmark_marginals, [i], [l])
            assert blk is not None or (i, l) not in observed, (i, l)
            if blk is not None:
                nsl += 1
                worst = max(worst, _corr(blk, Sig[r, lms(l)], dg[r], dg[lms(l)]))
    for a in range(L):
        for c in range(max(a - lm_reach, 0), min(a + lm_reach + 1, L)):
            blk = _served(dev.get_landmark_pair_marginals, [a], [c])
            if blk is not None:
                npair += 1
                worst = max(worst, _corr(blk, Sig[lms(a), lms(c)], dg[lms(a)], dg[lms(c)]))
    print("N %d L %d plan %s: worst %.2e of tol %.2e; %d state-landmark and %d landmark-pair blocks served" % (N, L, dev.segment_plan(), worst, tol, nsl, npair))
    assert worst <= tol, (worst, tol)
    return nsl, npair


def _range60_pair(**kw):
    """_anchored_range_chain(60) on the dense border and on the segmented path (8 landmarks seen from everywhere: all in fat blocks),
    both at the dense handle's states after three Gauss-Newton iterations; and the oracle"""
    p = _anchored_range_chain(60)
    dense = solver(p, landmark_dim=2)
    gn(dense, 3)
    seg = solver(p, landmark_dim=2, force_segmented=True, **kw)
    assert seg.segment_plan()["active"] == 1
    seg.set_states(*dense.get_states())
    seg.set_landmarks(dense.get_landmarks())
    orc = S.apply(p, O.Chain(O.POSE2, landmark_dim=2))
    return p, dense, seg, orc


def test_contract():
    p, dense, seg, _ = _range60_pair()
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*segmented"):
        seg.marginals()
    seg.marginals_on_segments()
    seg.marginals()
    Sd, Sn = seg.get_marginals()
    assert np.isfinite(Sd).all() and np.isfinite(Sn).all()
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*get_landmark_marginals"):
        seg.get_marginals(cross=True)
    # two calls are bit-identical
    Sl, Sx = seg.get_landmark_marginals(), seg.get_state_landmark_marginals([0, 7, 59], [0, 3, 7])
    seg.marginals()
    Sd2, Sn2 = seg.get_marginals()
    assert np.array_equal(Sd, Sd2) and np.array_equal(Sn, Sn2)
    assert np.array_equal(Sl, seg.get_landmark_marginals()) and np.array_equal(Sx, seg.get_state_landmark_marginals([0, 7, 59], [0, 3, 7]))
    # enable = 0 refuses again, with the default's text
    seg.marginals_on_segments(False)
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*segmented"):
        seg.marginals()
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*segmented"):
        seg.get_marginals()
    # stale after iterate_gn
    seg.marginals_on_segments()
    seg.marginals()
    seg.iterate_gn()
    for call in (seg.get_marginals, seg.get_landmark_marginals, lambda: seg.get_state_landmark_marginals([0], [0]),
                 lambda: seg.get_landmark_pair_marginals([0], [1]), lambda: seg.interpolate_covariances([0], [0.1], [0.05])):
        with pytest.raises(gp.GpslamHipError, match="stale"):
            call()
    # out of range / NULL
    seg.marginals()
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\).*out of range"):
        seg.get_state_landmark_marginals([60], [0])
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\).*out of range"):
        seg.get_landmark_pair_marginals([0], [8])
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\)"):
        seg.get_landmark_marginals(4, 5)
    # the opt-in on a dense-border handle leaves its marginals bit-identical
    dense.marginals()
    before = dense.get_marginals(cross=True)
    dense.marginals_on_segments()
    dense.marginals()
    after = dense.get_marginals(cross=True)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


def test_iterations_after_marginals_are_bit_identical():
    p = _soft(333, 16, 100)
    a = solver(p, landmark_dim=2, chart=gp.CHART_FIRST_ORDER, segment_length=128)
    b = solver(p, landmark_dim=2, chart=gp.CHART_FIRST_ORDER, segment_length=128)
    a.marginals_on_segments()
    a.marginals()
    gn(a, 2)
    gn(b, 2)
    a.marginals()
    a.run_gn(2)
    b.run_gn(2)
    for x, y in zip(a.get_states() + (a.get_landmarks(),), b.get_states() + (b.get_landmarks(),)):
        assert np.array_equal(x, y)


def test_against_the_oracle_and_the_dense_border():
    p, dense, seg, orc = _range60_pair()
    H = oracle_H(orc, dense)
    tol = tol_of(H)
    seg.marginals_on_segments()
    seg.marginals()
    nsl, npair = check_against_inverse(seg, H, tol, p)
    assert nsl >= 60 and npair >= 8
    dense.marginals()
    Sd, Sn, Slm, Sxl = dense.get_marginals(cross=True)
    Td, Tn = seg.get_marginals()
    b, ld, L, N = seg.b, seg.ld, seg.L, seg.N
    sd = np.sqrt(np.einsum("ikk->ik", Sd))
    sl = np.sqrt(np.diag(Slm)).reshape(L, ld)
    for i in range(N):
        assert _corr(Td[i], Sd[i], sd[i], sd[i]) <= 2 * tol
        if i + 1 < N:
            assert _corr(Tn[i], Sn[i], sd[i], sd[i + 1]) <= 2 * tol
    # the dense-border handle serves every pair through the same getters, bit for bit what get_marginals(cross=True) holds
    ii, ll = np.repeat(np.arange(N), L), np.tile(np.arange(L), N)
    Dx = dense.get_state_landmark_marginals(ii, ll)
    assert np.array_equal(Dx.reshape(N, L, b, ld).transpose(0, 2, 1, 3).reshape(N, b, L * ld), Sxl)
    aa, bb = np.repeat(np.arange(L), L), np.tile(np.arange(L), L)
    Dp = dense.get_landmark_pair_marginals(aa, bb)
    for t in range(L * L):
        assert np.array_equal(Dp[t], Slm[aa[t] * ld:(aa[t] + 1) * ld, bb[t] * ld:(bb[t] + 1) * ld])
    assert np.array_equal(dense.get_landmark_marginals(2, 3), Dp.reshape(L, L, ld, ld)[[2, 3, 4], [2, 3, 4]])
    # the segmented handle: the pairs it serves, in one batch each
    sx = [t for t in range(N * L) if _served(seg.get_state_landmark_marginals, [ii[t]], [ll[t]]) is not None]
    Tx = seg.get_state_landmark_marginals(ii[sx], ll[sx])
    for k, t in enumerate(sx):
        assert _corr(Tx[k], Dx[t], sd[ii[t]], sl[ll[t]]) <= 2 * tol
    sp = [t for t in range(L * L) if _served(seg.get_landmark_pair_marginals, [aa[t]], [bb[t]]) is not None]
    Tp = seg.get_landmark_pair_marginals(aa[sp], bb[sp])
    for k, t in enumerate(sp):
        assert _corr(Tp[k], Dp[t], sl[aa[t]], sl[bb[t]]) <= 2 * tol
    assert len(sx) == nsl and len(sp) == npair


# (N, segment_length, window, L, forced) -> the class of the plan the case is about.  NB seen on the device: see the docstring.
# forced: 13 landmarks and fewer fit the dense border, which compile() then prefers
LOCAL = {
    "333-seg128": (333, 128, 100, 16, False),
    "333-auto": (333, 0, 100, 40, False),
    "260-seg48-six-cuts": (260, 48, 60, 11, True),      # (13 landmarks: one of them is seen from three 48-state segments)
    "520-seg256-lds-class": (520, 256, 100, 80, False),
    "333-seg128-narrow": (333, 128, 100, 8, True),
}


@pytest.mark.parametrize("name", sorted(LOCAL))
def test_local_landmarks_widths_and_levels(name):
    """Seen on the device: 333-seg128 NB 16 (K 4, 2 levels, tol 2.6e-8), 333-auto NB 24 (C 80, K 6, 3 levels, 1.2e-8),
    260-seg48-six-cuts NB 12 (K 7: six segments, 3 levels, 4.8e-8), 520-seg256-lds-class NB 64 (K 4, 1.5e-8), 333-seg128-narrow
    NB 12 (K 4, 5.0e-8); the worst block of any case is 1.3e-11 in correlation units."""
    N, seglen, window, L, forced = LOCAL[name]
    p = _soft(N, L, window)
    dev = solver(p, landmark_dim=2, chart=gp.CHART_FIRST_ORDER, segment_length=seglen, force_segmented=forced)
    orc = S.apply(p, O.Chain(O.POSE2, chart=O.CHART_FIRST_ORDER, landmark_dim=2))
    plan = dev.segment_plan()
    assert plan["active"] == 1, plan
    if name == "260-seg48-six-cuts":
        assert plan["K"] >= 6 and plan["levels"] >= 3, plan
    if name == "520-seg256-lds-class":
        assert 48 < plan["NB"] <= 64, plan
    if name == "333-seg128-narrow":
        assert plan["NB"] <= 16, plan
    H = oracle_H(orc, dev)
    tol = tol_of(H)
    dev.marginals_on_segments()
    dev.marginals()
    cuts = _cuts(N, plan["C"])
    assert len(cuts) == plan["K"]
    ends = sorted({min(max(c + o, 0), N - 1) for c in cuts for o in (-2, -1, 0, 1, 2)})
    nsl, npair = check_against_inverse(dev, H, tol, p, states=ends)
    assert nsl >= len(ends) and npair >= L


@pytest.mark.parametrize("kind,sensor,N,seg", [(O.POSE3, True, 61, 32), (O.POSE3, False, 130, 64), (O.LINEAR3, False, 61, 32), (O.POSE2, True, 97, 48)],
                         ids=["pose3+sensor", "pose3", "linear3", "pose2+sensor"])
def test_every_block_size_against_the_dense_border(kind, sensor, N, seg):
    """The four graphs of test_gpu_segmented.py::test_segmented_path_on_every_block_size_and_measurement_mix, replayed the same way:
    block sizes 12, 12, 4 (fat blocks and borders of every tile count) and 6, at the initial estimate on both handles."""
    from gpslam_amd import sharded
    from test_gpu_measurements import build_meas_pair, LD
    orc, ref, c, (rec,) = build_meas_pair(kind, N=N, seed=11, sensor=sensor, extra_makers=(sharded.GraphRecorder,))
    chart = O.CHART_FIRST_ORDER if kind == O.POSE2 else O.CHART_EXPMAP
    s = gp.ChainSolver(kind, chart, LD[kind], force_segmented=True, segment_length=seg)
    rec.replay(s)
    assert s.segment_plan()["active"] == 1
    H = oracle_H(orc, ref)
    tol = tol_of(H)
    print("kappa-derived tol %.2e, plan %s" % (tol, s.segment_plan()))
    ref.marginals()
    s.marginals_on_segments()
    s.marginals()
    Sd, Sn, Slm, Sxl = ref.get_marginals(cross=True)
    Td, Tn = s.get_marginals()
    b, ld, L = s.b, s.ld, s.L
    sd = np.sqrt(np.einsum("ikk->ik", Sd))
    sl = np.sqrt(np.diag(Slm)).reshape(L, ld)
    worst = 0.0
    for i in range(N):
        worst = max(worst, _corr(Td[i], Sd[i], sd[i], sd[i]))
        if i + 1 < N:
            worst = max(worst, _corr(Tn[i], Sn[i], sd[i], sd[i + 1]))
    Tl = s.get_landmark_marginals()
    served = 0
    for l in range(L):
        worst = max(worst, _corr(Tl[l], Slm[l * ld:(l + 1) * ld, l * ld:(l + 1) * ld], sl[l], sl[l]))
        for i in range(N):
            blk = _served(s.get_state_landmark_marginals, [i], [l])
            if blk is not None:
                served += 1
                worst = max(worst, _corr(blk, Sxl[i][:, l * ld:(l + 1) * ld], sd[i], sl[l]))
        for l2 in range(L):
            blk = _served(s.get_landmark_pair_marginals, [l], [l2])
            if blk is not None:
                worst = max(worst, _corr(blk, Slm[l * ld:(l + 1) * ld, l2 * ld:(l2 + 1) * ld], sl[l], sl[l2]))
    print("worst %.2e of 2 tol %.2e, %d state-landmark blocks served" % (worst, 2 * tol, served))
    assert served >= N and worst <= 2 * tol
    s.close()


def test_interpolated_covariances_on_a_segmented_handle():
    """queries in the first and the last interval of a segment, into and out of a cut state, and at both ends of the chain"""
    p, dense, seg, _ = _range60_pair(segment_length=30)
    plan = seg.segment_plan()
    assert plan["K"] == 3 and plan["C"] == 30, plan
    H = oracle_H(S.apply(p, O.Chain(O.POSE2, landmark_dim=2)), dense)
    tol = tol_of(H)
    seg.marginals_on_segments()
    seg.marginals()
    dense.marginals()
    left = np.array([0, 1, 28, 29, 30, 31, 57, 58], dtype=np.int32)
    dt, tau = np.full(len(left), 0.1), np.linspace(0.02, 0.08, len(left))
    for gp_term in (True, False):
        A = seg.interpolate_covariances(left, dt, tau, gp_term=gp_term)
        B = dense.interpolate_covariances(left, dt, tau, gp_term=gp_term)
        for q in range(len(left)):
            s_ = np.sqrt(np.diag(B[q]))
            assert _corr(A[q], B[q], s_, s_) <= 2 * tol, (q, gp_term)


def test_fat_blocks_beyond_64_columns_are_refused_with_a_message():
    p = S.pose2_local_landmarks_chain(1300, L=180, window=200)
    dev = solver(p, landmark_dim=2, chart=gp.CHART_FIRST_ORDER, segment_length=256)
    assert dev.segment_plan()["NB"] == 72
    dev.marginals_on_segments()
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*72.*64"):
        dev.marginals()
    dev.iterate_gn()          # (the handle is as usable as before)


def test_a_graph_that_nothing_anchors_is_not_spd():
    """pose2_local_landmarks_chain without its pose prior and without landmark priors: H has the three gauge directions of the plane
    in its null space and a pivot of the fat chain comes out non-positive, as in iterate_gn on the same handle.  (A rank-deficient
    H is detected where rounding leaves a pivot at or below zero, here as everywhere in the library.  Measured: the SOFTENED copy
    of this graph without priors, and _anchored_range_chain(60) without priors in the exponential chart, round their last pivots to
    small positive numbers -- variances of 8e10 and no error; this graph's sums are in a fixed order, so its outcome is the same on
    every run.)"""
    p = S.pose2_local_landmarks_chain(333, L=16, window=100)
    p = {k: v for k, v in p.items() if not (k.startswith("prior_") or k.startswith("lprior"))}
    dev = solver(p, landmark_dim=2, chart=gp.CHART_FIRST_ORDER, segment_length=128)
    assert dev.segment_plan()["active"] == 1
    dev.marginals_on_segments()
    with pytest.raises(gp.GpslamHipError, match=r"\(-3\).*non-positive pivot"):
        dev.marginals()
