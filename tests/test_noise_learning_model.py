"""The numpy model of the measurement-noise statistic (tests/noise_learning_model.py) against the textbook likelihood of a
linear-Gaussian problem y = C x + nu, log N(y; C m, C K C^T + R), which forms no J, no H and no posterior: the derivative
G = (n C - B) / 2 in the entries of W = C^-1 and dF / d log theta = (tr Bw - n r) / 2 against central differences, and the EM
updates' monotonicity -- the algebra meas_noise.hip implements, checked on the CPU.  Then, on the graphs of
tests/fixed_lag_mix_model.py, the model with Sigma = inv(H) against the model with Sigma from a Cholesky factor of H, inside the
bound the device is held to (tests/test_gpu_noise_learning.py).

The bound of every comparison with a finite difference is test_qc_learning_model's: the quotient is taken at h and h / 2, its
truncation error is taken as |FD(h) - FD(h / 2)|, and the rounding of the two likelihoods it subtracts as noise / h with
noise = 1e-11 (|quadratic form| / 2 + sum |log pivot|), the magnitudes the likelihood is the sum of:
    bound = 2 |FD(h) - FD(h / 2)| + noise / h.
The model is compared with FD(h / 2)."""
import numpy as np
import pytest

import noise_learning_model as NM
from test_qc_learning_model import H_STEP, REL, directions


def _tile(pr, C):
    return np.tile(C, (len(pr["idx"]), 1, 1))


def _fd(f, h):
    """(FD(h), FD(h / 2), noise) of f: t -> (value, magnitude) at t = 0"""
    def q(hh):
        (a, ma), (b, mb) = f(hh), f(-hh)
        return (a - b) / (2.0 * hh), REL * (ma + mb)
    (f1, n1), (f2, n2) = q(h), q(0.5 * h)
    return f1, f2, max(n1, n2)


@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_gradient_in_W_against_finite_differences_of_the_textbook_likelihood(scale):
    pr = NM.linear_problem(seed=1)
    C = scale * pr["C0"][0]
    B, Bw, n, _, _ = NM.linear_statistic(pr, _tile(pr, C))
    assert n == len(pr["idx"])
    G = NM.gradient(C, B, n)
    W = np.linalg.inv(C)
    for dW in directions(pr["r"]):
        f1, f2, noise = _fd(lambda t: NM.textbook(pr, _tile(pr, np.linalg.inv(W + t * dW))), H_STEP)
        bound = 2.0 * abs(f1 - f2) + noise / H_STEP
        got = float(np.sum(G * dW))
        print("scale %g dW %s: model %.10g, FD(h/2) %.10g, gap %.3g of %.3g" % (scale, np.flatnonzero(dW.reshape(-1)), got, f2, abs(got - f2), bound))
        assert abs(got - f2) <= bound
    # at the current whitening tr Bw = tr(W B): the two statistics say the same about a shared covariance
    assert abs(np.trace(Bw) - np.sum(W * B)) <= 1e-11 * np.sum(np.abs(W) * np.abs(B))


@pytest.mark.parametrize("theta", [0.5, 2.0])
def test_derivative_in_log_theta_of_the_scale_family(theta):
    """every factor keeps its own shape C0_f; dF / d log theta = (tr Bw - n r) / 2, per row (Bw[q, q] - n) / 2 for diagonal models"""
    pr = NM.linear_problem(seed=2, shapes=True)
    _, Bw, n, _, _ = NM.linear_statistic(pr, theta * pr["C0"])
    got = 0.5 * (np.trace(Bw) - n * pr["r"])
    f1, f2, noise = _fd(lambda t: NM.textbook(pr, theta * np.exp(t) * pr["C0"]), H_STEP)
    bound = 2.0 * abs(f1 - f2) + noise / H_STEP
    print("theta %g: model %.10g, FD(h/2) %.10g, gap %.3g of %.3g" % (theta, got, f2, abs(got - f2), bound))
    assert abs(got - f2) <= bound
    ratio, rows = NM.em_scale(Bw, n)
    assert abs(ratio - (1.0 + 2.0 * got / (n * pr["r"]))) <= 1e-13 * abs(ratio)
    # one scale per row of diagonal models
    D0 = np.stack([np.diag(np.diag(c)) for c in pr["C0"]])
    th = np.array([0.8, 1.7]) * theta
    _, Bw, n, _, _ = NM.linear_statistic(pr, D0 * th[None, :, None])
    for q in range(pr["r"]):
        def f(t, q=q):
            s = th.copy()
            s[q] *= np.exp(t)
            return NM.textbook(pr, D0 * s[None, :, None])
        f1, f2, noise = _fd(f, H_STEP)
        assert abs(0.5 * (Bw[q, q] - n) - f2) <= 2.0 * abs(f1 - f2) + noise / H_STEP


@pytest.mark.parametrize("mode", ["shared", "scale"])
def test_em_steps_never_lower_the_textbook_likelihood(mode):
    pr = NM.linear_problem(seed=3, shapes=(mode == "scale"))
    cov = 3.0 * pr["C0"]
    zs = []
    for _ in range(8):
        z, mag = NM.textbook(pr, cov)
        zs.append((z, REL * mag))
        B, Bw, n, _, _ = NM.linear_statistic(pr, cov)
        cov = _tile(pr, NM.em_update(B, n)) if mode == "shared" else NM.em_scale(Bw, n)[0] * cov
    for k in range(1, len(zs)):
        print("%s step %d: %.10g -> %.10g" % (mode, k, zs[k - 1][0], zs[k][0]))
        assert zs[k][0] >= zs[k - 1][0] - (zs[k][1] + zs[k - 1][1])
    assert zs[-1][0] > zs[0][0] + 1.0
    if mode == "scale":     # 3 theta_true C0 was the start: the scale has come most of the way down to theta_true
        assert abs(cov[0][0, 0] / pr["C0"][0][0, 0] - pr["theta_true"]) < 0.5 * pr["theta_true"]


def test_use_masks_and_the_host_arithmetic():
    pr = NM.linear_problem(seed=4)
    cov = _tile(pr, pr["C0"][0])
    M = len(pr["idx"])
    full = NM.linear_statistic(pr, cov)
    use = np.arange(M) % 2 == 0
    half, rest = NM.linear_statistic(pr, cov, use), NM.linear_statistic(pr, cov, ~use)
    assert half[2] + rest[2] == full[2] == M
    assert np.abs(half[0] + rest[0] - full[0]).max() <= 1e-13 * np.abs(full[0]).max()
    assert np.array_equal(half[3], full[3])                     # P of every factor, used or not
    none = NM.linear_statistic(pr, cov, np.zeros(M, bool))
    assert none[2] == 0 and np.all(none[0] == 0.0) and np.all(none[1] == 0.0)
    B, n = full[0], full[2]
    C1 = NM.em_update(B, n)
    assert np.array_equal(C1, C1.T) and np.abs(NM.gradient(C1, B, n)).max() <= 1e-13 * np.abs(B).max()


@pytest.mark.parametrize("name", ["se2", "se3", "se3_vw", "so3", "r3"])
def test_two_ways_to_sigma_agree_inside_the_devices_bound(name):
    """the reference of tests/test_gpu_noise_learning.py computed a second way sits inside the bound it sets"""
    import marginals_mix_model as MX
    from test_gpu_marginals import tol_of
    p = MX.graph(name)
    orc = MX.oracle(p)
    H = MX.H_of(p)
    tol = tol_of(H)
    Linv = np.linalg.inv(np.linalg.cholesky(H))
    N = p["pose"].shape[0]
    assert NM.kinds(p)
    for pre in NM.kinds(p):
        mk, idx, lm, two, rows, ld, R = NM.kind_of(p, pre)
        e, J = orc.linearize_meas(mk, len(idx))
        a = NM.statistic(np.linalg.inv(H), e, J, idx, lm, R, N=N, ld=ld, two=two)
        b = NM.statistic(Linv.T @ Linv, e, J, idx, lm, R, N=N, ld=ld, two=two)
        assert a[2] == b[2] == len(idx)
        for what, x, y, bound in zip(("B", "Bw", "P"), (a[0], a[1], a[3]), (b[0], b[1], b[3]), NM.bounds(tol, a, a[4])):
            worst = (np.abs(x - y) / np.maximum(bound, 1e-300)).max()
            print("%s %s %s: worst |inv - cholesky| / bound %.3g" % (name, pre, what, worst))
            assert np.all(np.abs(x - y) <= bound)


@pytest.mark.parametrize("mode", ["scale", "rows", "shared"])
def test_the_learning_problems_fixed_point_is_near_the_truth(mode):
    """the condition on the seed of tests/test_gpu_noise_learning.py's learning problem: from 3 x the truth the numpy model run on the
    oracle settles within 6 standard errors sqrt(2 / (n r)) of the covariance the noise was drawn at"""
    from oracle import oracle as O
    p = NM.learn_problem()
    M = len(p["gps_left"])
    start = 3.0 * (np.diag(np.diag(NM.C_TRUE)) if mode == "rows" else NM.C_TRUE)
    seq = NM.model_learn(p, mode, start, 40, NM.tight(O.default_params()))
    far, before = seq[-1][0], seq[-2][0]
    assert np.abs(far - before).max() <= 1e-6 * np.abs(far).max()      # (settled)
    se = np.sqrt(2.0 / (M * 3))
    if mode == "shared":
        Li = np.linalg.inv(np.linalg.cholesky(NM.C_TRUE))
        off = np.linalg.eigvalsh(Li @ far @ Li.T) - 1.0
    elif mode == "rows":
        off = 3.0 * far - 1.0
    else:
        off = np.array([3.0 * float(far) - 1.0])
    print("%s: fixed point off the truth by %s, 6 standard errors are %.3g" % (mode, off, 6.0 * se))
    assert np.all(np.abs(off) <= 6.0 * se)
