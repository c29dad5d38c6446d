"""The numpy model of fixed-lag smoothing (tests/fixed_lag_model.py) against dense algebra on the oracle's arrays: CPU only.

The Schur recursion against a dense inverse of the assembled head at 1e-11 (relative to max |D_k|, max |g|); the factorisation of
Lambda; and, on linear_chain(64), a window of 16 states slid by 4 -- marginalise, append, two Gauss-Newton iterations, twelve times --
against the batch solution's last 16 states at 1e-9 (the problem is linear: the marginal is exact whatever the linearisation point)."""
import numpy as np
import pytest

from gpslam_amd import synthetic as S
from oracle import oracle as O
import fixed_lag_model as FL


def perturbed(p, seed=0, amp=0.02):
    rng = np.random.default_rng(77 + seed)
    kind, d = p["kind"], O.TANGENT_DIM[p["kind"]]
    q = dict(p)
    q["pose"] = np.stack([O.retract(kind, x, amp * rng.standard_normal(d)) for x in p["pose"]])
    q["vel"] = p["vel"] + amp * rng.standard_normal(p["vel"].shape)
    return q


def head_arrays(p, k):
    head, _ = FL.head_tail(p, k)
    orc = S.apply(head, O.Chain(p["kind"]))
    return orc.normal_equations()[:3]


@pytest.mark.parametrize("name", ["linear3", "pose3", "rot3"])
@pytest.mark.parametrize("k", [1, 2, 5, 11])
def test_schur_recursion_against_dense_inverse(name, k):
    p = perturbed({"linear3": lambda: S.linear_chain(12), "pose3": lambda: S.pose3_chain(12),
                   "rot3": lambda: S.rot3_attitude_chain(12, refs=2)}[name]())
    D, Om, g = head_arrays(p, k)
    Lam, gam, scale = FL.schur(D, Om, g, k)
    Lam_d, gam_d = FL.schur_dense(D, Om, g, k)
    assert np.abs(Lam - Lam_d).max() <= 1e-11 * scale
    assert np.abs(gam - gam_d).max() <= 1e-11 * np.abs(g).max()
    assert np.linalg.eigvalsh(0.5 * (Lam + Lam.T)).min() > 0.0      # (the other orientation of O gives an indefinite Lambda)
    # the factorisation the handle keeps: A^T A = Lambda (symmetrised), A^T c = -gamma
    A, c = FL.factor(Lam, gam, scale)
    assert np.abs(A.T @ A - 0.5 * (Lam + Lam.T)).max() <= 1e-13 * scale
    assert np.abs(A.T @ c + gam).max() <= 1e-11 * np.abs(g).max()


def test_factor_of_a_rank_deficient_lambda():
    rng = np.random.default_rng(5)
    J = rng.standard_normal((3, 6))
    Lam = J.T @ J
    gam = -J.T @ rng.standard_normal(3)
    A, c = FL.factor(Lam, gam, 10.0)
    assert np.all(A[3:] == 0.0) and np.all(c[3:] == 0.0)
    assert np.abs(A.T @ A - Lam).max() <= 1e-13
    assert np.abs(A.T @ c + gam).max() <= 1e-12
    A0, c0 = FL.factor(1e-18 * Lam, 1e-18 * gam, 10.0)              # Lambda ~ 0: no rows at all
    assert np.all(A0 == 0.0) and np.all(c0 == 0.0)


def slide_reference(p, window, step, slides, iters=2):
    """The model's fixed-lag smoother over problem p: returns (pose, vel) of the last window."""
    kind, chart = p["kind"], O.CHART_EXPMAP
    lo, hi = 0, window
    cur = FL.sub_problem(p, lo, hi)
    gaussians = []
    for _ in range(slides):
        head, tail = FL.head_tail(cur, step)
        orc = S.apply(head, O.Chain(kind))
        D, Om, g = orc.normal_equations()[:3]
        for idx, pl, vl, A, c in gaussians:
            assert idx < step
            xi = FL.xi_of(kind, chart, pl, vl, cur["pose"][idx], cur["vel"][idx])
            D[idx] += A.T @ A
            g[idx] += A.T @ (c - A @ xi)
        Lam, gam, scale = FL.schur(D, Om, g, step)
        A, c = FL.factor(Lam, gam, scale)
        gaussians = [(0, cur["pose"][step].copy(), cur["vel"][step].copy(), A, c)]
        new = FL.sub_problem(p, lo + step, hi + step, new_from=hi)
        cur = dict(tail)
        cur["pose"] = np.concatenate([tail["pose"], p["pose"][hi:hi + step]])
        cur["vel"] = np.concatenate([tail["vel"], p["vel"][hi:hi + step]])
        cur["N"] = window
        for key, (others, _two) in FL.FACTOR_KEYS.items():
            if key in new:
                for k2 in [key] + others:
                    cur[k2] = np.concatenate([cur[k2], new[k2]]) if k2 in cur else new[k2]
        lo, hi = lo + step, hi + step
        orc = S.apply(cur, O.Chain(kind))
        for _ in range(iters):
            cur["pose"], cur["vel"] = FL.gn_step(orc, kind, chart, gaussians)
    return cur["pose"], cur["vel"]


def test_sliding_window_equals_batch_on_a_linear_chain():
    p = S.linear_chain(64)
    orc = S.apply(p, O.Chain(p["kind"]))
    for _ in range(2):
        orc.iterate_gn()
    bp, bv = orc.get_states()
    wp, wv = slide_reference(p, 16, 4, 12)
    assert np.abs(wp - bp[48:]).max() <= 1e-9
    assert np.abs(wv - bv[48:]).max() <= 1e-9
