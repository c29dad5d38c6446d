"""The numpy model of the Qc statistic (tests/qc_learning_model.py) against the textbook GP marginal likelihood, which forms no J and
no H: the derivative G = n_f Qc - A / 2 against finite differences, the EM update's monotonicity and fixed point, the stationary
scale against a fine curve -- the algebra qc_learn.hip implements, checked on the CPU.

The bound of every comparison with a finite difference: the difference quotient is taken at two steps, h and h / 2; its truncation
error is taken as |FD(h) - FD(h / 2)| and the rounding of the two evidences it subtracts as evidence_noise / h, evidence_noise by the
rule of test_gpu_evidence._evidence_tol (half the log-det bound of the graph's H plus 1e-11 of the cost):
    bound = 2 |FD(h) - FD(h / 2)| + evidence_noise / h.
The model is compared with FD(h / 2)."""
import numpy as np
import pytest

import evidence_model as EM
import qc_learning_model as QM

H_STEP = 1e-3       # in the entries of W = Qc^-1, which are of order one here
REL = 1e-11


def evidence_noise(pr, Qc, H):
    return 0.5 * EM.logdet_tol(H) + REL * abs(QM.linear_chain(pr, Qc).error())


def directions(d):
    """the symmetric perturbations of W: E_rr, and E_rs + E_sr"""
    out = []
    for r in range(d):
        for s in range(r, d):
            dW = np.zeros((d, d))
            dW[r, s] = dW[s, r] = 1.0
            out.append(dW)
    return out


def fd_pair(pr, W, dW, h=H_STEP):
    def fd(hh):
        return (QM.textbook(pr, np.linalg.inv(W + hh * dW)) - QM.textbook(pr, np.linalg.inv(W - hh * dW))) / (2.0 * hh)
    return fd(h), fd(0.5 * h)


def check_gradient(pr, Qc, what):
    """tr(G dW) of the model against the textbook curve's difference quotient in every symmetric direction; returns the largest
    bound (what "zero" means for a gradient of this problem)"""
    A, n_f, H = QM.linear_statistic(pr, Qc)
    G = QM.gradient(Qc, A, n_f)
    assert np.abs(G - G.T).max() <= 1e-12 * np.abs(A).max()      # (relative to what G is the difference of: it vanishes at the fixed point)
    noise = evidence_noise(pr, Qc, H)
    W = np.linalg.inv(Qc)
    worst = 0.0
    for dW in directions(Qc.shape[0]):
        f1, f2 = fd_pair(pr, W, dW)
        bound = 2.0 * abs(f1 - f2) + noise / H_STEP
        got = float(np.sum(G * dW))
        print("%s dW %s: model %.10g, FD(h/2) %.10g, gap %.3g of %.3g (|FD(h) - FD(h/2)| %.3g)" % (what, np.flatnonzero(dW.reshape(-1)), got, f2, abs(got - f2), bound, abs(f1 - f2)))
        assert abs(got - f2) <= bound
        worst = max(worst, bound)
    return worst


@pytest.fixture(scope="module")
def problem():
    # position measurements of every state: the EM iteration of a sparser problem needs thousands of steps to settle
    return EM.linear_gp_problem(N=40, d=3, dt=0.1, theta=1.0, every=1, seed=0)


@pytest.mark.parametrize("scale", [1.0, 10.0])
def test_gradient_against_finite_differences_of_the_textbook_likelihood(problem, scale):
    """h = 1e-3, observed: at Qc0 gaps of 5e-7 .. 5e-6 under bounds of 4e-6 .. 3e-5, at 10 Qc0 gaps of 7e-4 .. 1e-2 under bounds of
    4e-3 .. 6e-2 -- a sixth of the bound throughout, as a truncation error that falls with h^2 gives (the gap is about a third of
    |FD(h) - FD(h / 2)|); evidence_noise / h is 1e-6.  On the sparser problem below the same holds at h = 1e-2 and h = 3e-4 (gaps
    5e-5 .. 4e-3 and 4e-8 .. 3e-6); at 3e-4 the noise term is already the larger part of the bound, so h stays at 1e-3."""
    check_gradient(problem, scale * problem["Qc0"], "scale %g" % scale)


def test_sparser_measurements_too():
    pr = EM.linear_gp_problem(N=40, d=3, dt=0.1, theta=1.0, every=4, seed=2)
    check_gradient(pr, pr["Qc0"], "every 4")


def test_em_steps_never_lower_the_textbook_evidence(problem):
    pr = problem
    seq = QM.em_fixed_point(pr, 10.0 * pr["Qc0"], 10)
    z = [QM.textbook(pr, Q) for Q in seq]
    for k in range(1, len(seq)):
        tol = sum(evidence_noise(pr, Q, QM.linear_statistic(pr, Q)[2]) for Q in (seq[k - 1], seq[k]))
        print("step %d: log Z %.10g -> %.10g (tol %.3g)" % (k, z[k - 1], z[k], tol))
        assert z[k] >= z[k - 1] - tol
    assert z[-1] > z[0] + 1.0      # ... and they do go up: from 10 Qc0 there is a lot to gain


def test_the_em_fixed_point_is_a_stationary_point_of_the_textbook_evidence(problem):
    pr = problem
    seq = QM.em_fixed_point(pr, 10.0 * pr["Qc0"], 2000, rtol=1e-12)
    assert len(seq) < 2000
    star = seq[-1]
    assert np.all(np.linalg.eigvalsh(star) > 0)
    bound = check_gradient(pr, star, "fixed point")
    # the model's G is zero there by construction (G = n_f (Qc - Qc+)); the content is the textbook side: its own difference
    # quotient is within the bound of zero
    A, n_f, H = QM.linear_statistic(pr, star)
    assert np.abs(QM.gradient(star, A, n_f)).max() <= bound
    noise = evidence_noise(pr, star, H)
    for dW in directions(3):
        f1, f2 = fd_pair(pr, np.linalg.inv(star), dW)
        assert abs(f2) <= 2.0 * abs(f1 - f2) + noise / H_STEP, (dW, f2)


def test_em_scale_lands_on_the_argmax_of_a_fine_textbook_curve(problem):
    pr = problem
    seq = QM.em_fixed_point(pr, 10.0 * pr["Qc0"], 2000, rtol=1e-12, scale_of=pr["Qc0"])
    assert len(seq) < 2000
    theta = seq[-1][0, 0] / pr["Qc0"][0, 0]
    assert np.abs(seq[-1] - theta * pr["Qc0"]).max() <= 1e-14 * theta * np.abs(pr["Qc0"]).max()
    # steps of 1e-3 theta: the curve falls by about n_f d / 2 * 1e-6 = 6e-5 per step next to its top, the noise of a point is 1e-9
    grid = theta * (1.0 + 1e-3 * np.arange(-10, 11))
    curve = [QM.textbook(pr, t * pr["Qc0"]) for t in grid]
    print("theta %.8g, curve around it %s" % (theta, np.array(curve) - curve[10]))
    assert int(np.argmax(curve)) == 10
    assert 0.2 <= theta <= 5.0      # (the data were drawn at theta = 1)
