"""Posterior sampling on the device (include/gpslam_hip_sampling.h, gpslam_amd/csrc/sampling.hip) against numpy:
dogleg_model.system's dense H and Gauss-Newton step on the oracle's arrays, and the generator's model of tests/posterior_model.py.

Graphs: dogleg_model.FAMILY (12 to 16 states, with and without landmarks), SIZES (two states; 300 and 1025 states: several workgroups
of every kernel), the robust graph, the GPSLAM_ROT3_BIAS chain of the AHRS recipe.

Bounds.
  Covariance identity, noise = I: sum_k delta_k delta_k^T against numpy's inv(H), entry by entry, at 2 * 1e-9 * sum_k |delta_k|_inf^2
    -- the project's 1e-9 per-step bound on each delta_k, carried through the outer product (2 |delta| |error|) -- plus ten times the
    twin distance of inv(H) (float64 against np.longdouble, DESIGN.md section 2's rule), capped at 1e-7.
  Own residuals: delta against the model's Gauss-Newton step at 1e-9 of its largest entry (test_gpu_dogleg.STEP_TOL), the emitted
    states and landmarks by test_gpu_dogleg.states_close's rule; the robust graph (sampled at its current weights, the model its
    reweighted twin) and the AHRS chain by the same two bounds.
  Generator: 1e-12 absolute against the model (values below 10; a few ulps of the device's log and cos are all the difference).
  Statistics at a fixed seed, K = 2048 draws: w = L^T delta (H = L L^T) has second moments within 6 sqrt((1 + [i = j]) / K) of I and
    a mean within 6 / sqrt(K) -- the entries' own standard deviations times six.  tests/test_posterior_model.py asks the same of the
    model's normals at this seed on the CPU.
Everything else is to the bit."""
import numpy as np
import pytest

import gpslam_amd as gp
from oracle import oracle as O
import dogleg_model as DM
import posterior_model as PM
from test_gpu_dogleg import device, ahrs_pair, STEP_TOL, ALL, IDS, _closure, _border
from test_posterior_model import STAT_SEED, STAT_K, STAT_N

pytestmark = pytest.mark.gpu
SMALL = DM.FAMILY + DM.SIZES[:2]
SEED = (0x5EED << 32) | 0x01234567      # bits above 32
FIRST = 2 ** 32 + 3
SE2_LM = ("se2", True, None)


def inv_long(H):
    """H^-1 by Gauss-Jordan in np.longdouble (H symmetric positive definite: no pivoting)"""
    n = H.shape[0]
    M = np.concatenate([H.astype(np.longdouble), np.eye(n, dtype=np.longdouble)], axis=1)
    for k in range(n):
        M[k] /= M[k, k]
        col = M[:, k].copy()
        col[k] = 0
        M -= np.outer(col, M[k])
    return M[:, n:]


@pytest.fixture(scope="module")
def reference():
    """per graph: the description and the model's numbers at its own states (computed once, never written to)"""
    cache = {}

    def get(name, lm, N, robust=False):
        key = (name, lm, N, robust)
        if key not in cache:
            p = DM.graph(name, lm, N, robust=robust)
            H, gv, arr = DM.system(p)
            cache[key] = dict(p=p, H=H, dn=DM.gn_step(H, gv, arr))
        return cache[key]
    return get


def unpack(dev, out, k=0):
    """sample k of a sample_posterior result as the description entries (pose, vel, landmarks)"""
    delta, poses, vels, lms = out
    return poses[k], vels[k], None if lms is None else lms[k]


def close_to(q, pose, vel, lm, tol=STEP_TOL):
    """test_gpu_dogleg.states_close's rule on arrays: relative to the largest entry of each array"""
    worst = max(np.abs(pose - q["pose"]).max() / max(1.0, np.abs(q["pose"]).max()), np.abs(vel - q["vel"]).max() / max(1.0, np.abs(q["vel"]).max()))
    if "landmarks" in q:
        worst = max(worst, np.abs(lm - q["landmarks"]).max() / max(1.0, np.abs(q["landmarks"]).max()))
    assert worst <= tol, worst
    return worst


def same_bits(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert np.array_equal(x, y)


# ---------------------------------------------------------------- 1. the covariance identity
@pytest.mark.parametrize("name,lm,N", SMALL, ids=IDS[:len(DM.FAMILY)] + IDS[len(DM.FAMILY):len(DM.FAMILY) + 2])
def test_unit_noise_gives_the_covariance(reference, name, lm, N):
    ref = reference(name, lm, N)
    H = ref["H"]
    dev = device(ref["p"])
    n_noise = dev.posterior_noise_dim()
    assert n_noise >= H.shape[0]
    delta = dev.sample_posterior(n_noise, noise=np.eye(n_noise))[0]
    assert delta.shape == (n_noise, H.shape[0])
    S = delta.T @ delta
    Hi = np.linalg.inv(H)
    twin = float(np.abs(Hi.astype(np.longdouble) - inv_long(H)).max())
    tol = 2.0 * STEP_TOL * float((np.abs(delta).max(axis=1) ** 2).sum()) + min(10.0 * twin, 1e-7)
    err = np.abs(S - Hi).max()
    print("%s N %s: n_noise %d, n %d: |sum delta delta^T - inv(H)| %.3g of %.3g (twin of inv(H) %.3g, largest entry %.3g)"
          % (name, N, n_noise, H.shape[0], err, tol, twin, np.abs(Hi).max()))
    assert err <= tol


# ---------------------------------------------------------------- 2. own residuals give the Gauss-Newton step
def check_own(dev, p, dn, q, what=""):
    e = PM.own_noise(dev, p)
    assert e.shape == (dev.posterior_noise_dim(),)
    out = dev.sample_posterior(1, noise=e[None, :])
    delta = out[0][0]
    err = np.abs(delta - dn).max() / np.abs(dn).max()
    worst = close_to(q, *unpack(dev, out))
    print("%s: delta %.3g of %.3g relative (|dn|_inf %.3g), states %.3g" % (what, err, STEP_TOL, np.abs(dn).max(), worst))
    assert err <= STEP_TOL
    return delta


@pytest.mark.parametrize("name,lm,N", ALL, ids=IDS)
def test_own_residuals_give_the_gauss_newton_step(reference, name, lm, N):
    ref = reference(name, lm, N)
    p, dn = ref["p"], ref["dn"]
    check_own(device(p), p, dn, DM.retracted(p, dn), what="%s N %s" % (name, N))


def test_own_residuals_on_the_robust_graph(reference):
    ref = reference(DM.ROBUST, True, None, robust=True)
    p, dn = ref["p"], ref["dn"]
    check_own(device(p), p, dn, DM.retracted(p, dn), what="robust %s" % DM.ROBUST)


def test_own_residuals_on_the_ahrs_chain():
    orc, dev = ahrs_pair()
    arr = orc.normal_equations()
    dn = DM.gn_step(None, arr[2].reshape(-1), arr)
    rc, _ = orc.iterate_gn()        # the oracle's own x (+) dn
    assert rc == 0
    pose, vel = orc.get_states()
    delta = check_own(dev, {}, dn, dict(pose=pose, vel=vel), what="rot3_bias")
    assert np.abs(delta.reshape(-1, 12)[:, 9:]).max() == 0.0      # the pad coordinates of a draw are exact zeros
    _, _, vels, _ = dev.sample_posterior(3, seed=5)
    assert np.abs(vels[:, :, 3:]).max() == 0.0                    # ... of a generated one too


# ---------------------------------------------------------------- 3. the generator is the model's
@pytest.mark.parametrize("name,lm,N", [DM.SIZES[0], SE2_LM, DM.SIZES[4]], ids=["se3_2", "se2_lm", "se3_1025"])
def test_generator_equals_the_model(reference, name, lm, N):
    dev = device(reference(name, lm, N)["p"])
    n_noise, count = dev.posterior_noise_dim(), 3
    got = dev.posterior_noise(SEED, FIRST, count)
    want = PM.noise(SEED, FIRST, count, n_noise)
    err = np.abs(got - want).max()
    print("%s N %s: n_noise %d, generator against the model %.3g, largest |eps| %.3f" % (name, N, n_noise, err, np.abs(want).max()))
    assert got.shape == want.shape and err <= 1e-12
    same_bits(dev.sample_posterior(count, seed=SEED, first=FIRST), dev.sample_posterior(count, noise=got))


# ---------------------------------------------------------------- 4. a draw does not depend on the batch
@pytest.mark.parametrize("name,lm,N", [SE2_LM, ("se3", False, None)], ids=["se2_lm", "se3"])
def test_a_draw_does_not_depend_on_the_batch(reference, name, lm, N):
    dev = device(reference(name, lm, N)["p"])
    five = dev.sample_posterior(5, seed=SEED, first=FIRST)
    for k in range(5):
        one = dev.sample_posterior(1, seed=SEED, first=FIRST + k)
        same_bits([None if a is None else a[k] for a in five], [None if a is None else a[0] for a in one])
    assert not np.array_equal(five[0][0], five[0][1])


def test_only_the_outputs_asked_for_come_back(reference):
    dev = device(reference(*SE2_LM)["p"])
    names = ("delta", "poses", "vels", "landmarks")
    full = dev.sample_posterior(3, seed=SEED, first=FIRST)
    for want in (("delta",), ("poses", "vels"), ("landmarks",)):
        part = dev.sample_posterior(3, seed=SEED, first=FIRST, want=want)
        for name, a, b in zip(names, full, part):
            assert (b is None) == (name not in want)
            assert b is None or np.array_equal(a, b)
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\)"):
        dev.sample_posterior(1, want=())
    with pytest.raises(gp.GpslamHipError, match="want"):
        dev.sample_posterior(1, want=("states",))


# ---------------------------------------------------------------- 5. the handle is left alone
def test_the_handle_is_left_alone(reference):
    p = reference(*SE2_LM)["p"]
    dev, twin = device(p), device(p)
    before = dev.get_states() + (dev.get_landmarks(),)
    rows = dev.get_rows()
    dev.sample_posterior(4, seed=3)
    same_bits(before, dev.get_states() + (dev.get_landmarks(),))
    e = PM.own_noise(dev, p)
    dev.sample_posterior(1, noise=e[None, :])
    same_bits(before, dev.get_states() + (dev.get_landmarks(),))
    same_bits(rows, dev.get_rows())
    for _ in range(2):
        dev.iterate_gn()
        twin.iterate_gn()
        same_bits(dev.get_states() + (dev.get_landmarks(),), twin.get_states() + (twin.get_landmarks(),))


def test_marginals_are_stale_after_sampling(reference):
    dev = device(reference(*SE2_LM)["p"])
    dev.marginals()
    want = dev.get_marginals(cross=True)
    dev.sample_posterior(2, seed=1)
    with pytest.raises(gp.GpslamHipError, match="stale"):
        dev.get_marginals()
    dev.marginals()
    same_bits(want, dev.get_marginals(cross=True))


# ---------------------------------------------------------------- 6. statistics at a fixed seed
def test_statistics_of_generated_draws(reference):
    ref = reference(*SE2_LM)
    H, K = ref["H"], STAT_K
    n = H.shape[0]
    assert n == STAT_N        # (the size tests/test_posterior_model.py checked the seed at)
    dev = device(ref["p"])
    delta = dev.sample_posterior(K, seed=STAT_SEED)[0]
    w = delta @ np.linalg.cholesky(H)       # rows L^T delta_k
    bm, bs = PM.moment_bounds(n, K)
    mean, S = w.mean(axis=0), w.T @ w / K
    print("seed %d, %d draws of %d unknowns: mean at most %.2f sigma, second moments at most %.2f sigma"
          % (STAT_SEED, K, n, np.abs(mean).max() * np.sqrt(K), (np.abs(S - np.eye(n)) / (bs / 6.0)).max()))
    assert np.abs(mean).max() <= bm
    assert (np.abs(S - np.eye(n)) <= bs).all()


# ---------------------------------------------------------------- 7. refusals
def _gaussian(s, p):
    b = s.b
    s.add_state_gaussians([3], p["pose"][3], p["vel"][3], np.eye(b), np.zeros(b))


REFUSALS = [
    ("fp32", dict(precision=gp.FP32), None, "fp32", False),
    ("sharded", dict(force_sharded=True), None, "sharded", False),
    ("segmented", dict(force_segmented=True), None, "segmented", True),
    ("closures", {}, _closure, "loop closures", True),
    ("state_gaussian", {}, _gaussian, "state Gaussians", True),
    ("border", {}, _border, "border Gaussians", True),
]


@pytest.mark.parametrize("what,kw,extra,message,lm", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_handle_as_it_was(what, kw, extra, message, lm):
    p = DM.graph("se2", lm, 60 if what == "segmented" else None)      # (segments need a chain to cut)
    a, b = device(p, extra, **kw), device(p, extra, **kw)
    before = a.get_states() + ((a.get_landmarks(),) if lm else ())
    a.launch_census()
    nothing = a.launch_census()
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*" + message):
        a.sample_posterior(2)
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*" + message):
        a.sample_posterior(1, noise=np.zeros((1, a.posterior_noise_dim())))
    assert a.launch_census() == nothing
    same_bits(before, a.get_states() + ((a.get_landmarks(),) if lm else ()))
    a.iterate_gn()
    b.iterate_gn()
    same_bits(a.get_states(), b.get_states())


def test_argument_errors(reference):
    p = reference(*SE2_LM)["p"]
    dev = device(p)
    before = dev.get_states()
    for count in (0, -1):
        with pytest.raises(gp.GpslamHipError, match=r"\(-1\)"):
            dev.sample_posterior(count)
        with pytest.raises(gp.GpslamHipError, match=r"\(-1\)"):
            dev.posterior_noise(1, 0, count)
    from gpslam_amd import chain
    assert chain._sampling_lib().gpslam_hip_sample_posterior(dev._h, 1, 0, 0, None, None, None, None, None) == -1
    same_bits(before, dev.get_states())
    import fixed_lag_mix_model as FM
    raw = FM.chain(p, gp.ChainSolver)
    raw.set_qc(p["qc"])
    raw.set_states(p["pose"], p["vel"])
    with pytest.raises(gp.GpslamHipError, match=r"\(-4\)"):
        raw.sample_posterior(1)


def test_reruns_are_bit_identical(reference):
    out = []
    for _ in range(2):
        dev = device(reference("se3", False, 1025)["p"])
        out.append(dev.sample_posterior(2, seed=SEED, first=FIRST))
    same_bits(out[0], out[1])
