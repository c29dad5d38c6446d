"""Powell's dogleg (include/gpslam_hip_dogleg.h) in plain numpy on the oracle's arrays: the reference side of
tests/test_dogleg_*.py and tests/test_gpu_dogleg.py.

A problem is a description of tests/fixed_lag_mix_model.py at its own states; a robust one is linearised as its reweighted twin
(marginals_mix_model.reweighted_at) and costs sum rho.  Unknowns are the states, then the landmarks.

  system       dense H and g = -gradient (H dn = g), and the oracle's block arrays
  block_quad   g^T H g as the sum over the blocks, in any dtype (the device's order of terms, up to the order inside a block)
  scalars      (gg, gHg, gn, nn) and the Gauss-Newton step
  point        the dogleg point of a trust radius: (alpha, beta, |dd|, predicted decrease, branch)
  decide       one trust-region decision, written from the rule table of the header, not from the library's code
  retracted    the description at x (+) delta
  cost         the cost the optimiser compares
  iterate      one DoglegOptimizer::iterate()
  optimize     NonlinearOptimizer::defaultOptimize over iterate
  perturbed    a start away from the description's own
"""
import numpy as np

from gpslam_amd import chain as GC
from oracle import oracle as O
import fixed_lag_mix_model as FM
import marginals_mix_model as MX

EPS = np.finfo(np.float64).eps
FLOOR = 1e-5
ONE_STEP, SEARCH_EACH, SEARCH_REDUCE = 0, 1, 2
NONE, INCREASED, DECREASED = 0, 1, 2


DENSE_MAX = 5000      # unknowns up to which the dense H is formed (a chain without landmarks needs none: the block solve)


def system(p, gaussians=()):
    """(H, g, arrays): H is None beyond DENSE_MAX unknowns.  gaussians: state Gaussians (idx, pose_lin, vel_lin, A, c) on top"""
    q, _ = MX.reweighted_at(p)
    arr = MX.oracle(q).normal_equations()
    if gaussians:
        Dg, gg_ = FM.with_state_gaussians(arr[0], arr[2], p["kind"], p.get("chart", FM.E), p["pose"], p["vel"], gaussians)
        arr = (Dg, arr[1], gg_) + tuple(arr[3:])
    D, Om, g, B, HLL, gL = arr
    gv = g.reshape(-1) if B is None else np.concatenate([g.reshape(-1), gL])
    H = MX.dense_H(D, Om, B, HLL) if gv.size <= DENSE_MAX else None
    return H, gv, arr


def gn_step(H, gv, arr):
    """dn of H dn = g: the oracle's block-tridiagonal solve on a chain without landmarks, else dense"""
    if arr[3] is None:
        return O.block_tridiag_solve(arr[0], arr[1], arr[2]).reshape(-1)
    return np.linalg.solve(H, gv)


def block_quad(arr, dtype=np.float64):
    D, Om, g, B, HLL, gL = [None if a is None else np.asarray(a, dtype=dtype) for a in arr]
    N = D.shape[0]
    acc = dtype(0)
    for i in range(N):
        acc += g[i] @ (D[i] @ g[i])
        if i + 1 < N:
            acc += 2 * (g[i + 1] @ (Om[i] @ g[i]))
        if B is not None:
            acc += 2 * (g[i] @ (B[i] @ gL))
    if B is not None:
        acc += gL @ (HLL @ gL)
    return acc


def scalars(H, gv, arr, dtype=np.float64):
    """((gg, gHg, gn, nn), dn); dn is always the float64 solve, the sums run in dtype"""
    dn = gn_step(H, gv, arr)
    g_, d_ = gv.astype(dtype), dn.astype(dtype)
    return (g_ @ g_, block_quad(arr, dtype), g_ @ d_, d_ @ d_), dn


def predicted(s4, alpha, beta):
    gg, gHg, gn, nn = s4
    return (alpha * gg + beta * gn) - (alpha * alpha * gHg + 2 * alpha * beta * gg + beta * beta * gn) / 2


def point(s4, delta):
    gg, gHg, gn, nn = [float(v) for v in s4]
    norm_n = np.sqrt(nn) if nn > 0 else 0.0
    if not (gg > 0 and gHg > 0):
        alpha, beta, branch = 0.0, (min(1.0, delta / norm_n) if norm_n > 0 else 0.0), 2
    else:
        s = gg / gHg
        norm_u = np.sqrt(s * s * gg)      # |du|^2 = s^2 gg
        if delta < norm_u:
            alpha, beta, branch = delta / norm_u * s, 0.0, 0
        elif delta < norm_n:
            # |du + tau (dn - du)|^2 = delta^2 in longdouble, the root in [0, 1]
            L = np.longdouble
            uu, un = L(s) * L(s) * L(gg), L(s) * L(gn)
            a, b, c = uu - 2 * un + L(nn), 2 * (un - uu), uu - L(delta) * L(delta)
            if a > 0:
                disc = np.sqrt(max(b * b - 4 * a * c, L(0)))
                tau = float(min(L(1), max(L(0), (-2 * c) / (b + disc) if b >= 0 else (-b + disc) / (2 * a))))
            else:
                tau = 1.0
            alpha, beta, branch = (1.0 - tau) * s, tau, 1
        else:
            alpha, beta, branch = 0.0, 1.0, 2
    norm = float(np.sqrt(max(alpha * alpha * gg + 2 * alpha * beta * gn + beta * beta * nn, 0.0)))
    return alpha, beta, norm, float(predicted((gg, gHg, gn, nn), alpha, beta)), branch


def gain(f, f_new, pred):
    if abs(f - f_new) < 1e-15 or abs(pred) < 1e-15:
        return 0.5
    with np.errstate(all="ignore"):
        return float(np.float64(f - f_new) / np.float64(pred))


def decide(f, f_new, pred, norm, mode, delta, last_action):
    """(keep, stay, delta, last_action) by the rule table of include/gpslam_hip_dogleg.h"""
    rho = gain(f, f_new, pred)
    if np.isfinite(rho) and rho >= 0.75:
        nd = max(delta, 3.0 * norm)
        if mode != SEARCH_EACH or abs(nd - delta) < 1e-15 or last_action == DECREASED:
            return True, False, nd, last_action
        return True, True, nd, INCREASED
    if np.isfinite(rho) and rho >= 0.25:
        return True, False, delta, last_action
    if np.isfinite(rho) and rho >= 0.0:
        floor = not delta > FLOOR
        nd = delta if floor else delta / 2
        if mode == ONE_STEP or last_action == INCREASED or floor:
            return True, False, nd, last_action
        return True, True, nd, DECREASED
    if delta > FLOOR:
        return False, True, delta / 2, DECREASED
    return False, False, delta, last_action


def retracted(p, dd):
    kind, chart = p["kind"], p.get("chart", FM.E)
    d = O.TANGENT_DIM[kind]
    N = p["pose"].shape[0]
    x = dd[:N * 2 * d].reshape(N, 2 * d)
    pose = np.stack([O.retract(kind, p["pose"][i], x[i, :d], chart) for i in range(N)])
    lm = p["landmarks"] + dd[N * 2 * d:].reshape(p["landmarks"].shape) if "landmarks" in p else None
    return MX.at(p, pose, p["vel"] + x[:, d:], lm)


def cost(p):
    orc = MX.oracle(FM.plain(p))
    err = orc.error()
    if not FM.robust_kinds(p):
        return err
    for pre, (r, w) in FM.robust_weights(p, FM.plain_errors(p, orc)).items():
        for f, (loss, k) in enumerate(zip(p[pre + "_loss"], p[pre + "_k"])):
            if loss:
                err += GC.robust_eval(int(loss), float(k), float(r[f]))[1] - 0.5 * r[f] * r[f]
    return err


def margin(f, f_new, s4, s4_long, alpha, beta):
    """how close to 0, 0.25 or 0.75 the gain ratio may lie before rounding decides the branch: 100 eps f / |f - f_new| plus 100 times
    the distance of the predicted decrease from its np.longdouble twin, relative"""
    p64 = predicted([float(v) for v in s4], alpha, beta)
    pl = predicted(s4_long, np.longdouble(alpha), np.longdouble(beta))
    twin = float(abs(np.longdouble(p64) - pl) / abs(pl)) if pl != 0 else 0.0
    return (100.0 * EPS * abs(f) / abs(f - f_new) if f != f_new else np.inf) + 100.0 * twin


def iterate(p, delta, mode=ONE_STEP):
    """One iteration from the description's states.  Returns a dict: p (the description after), delta, trials, accepted, branch, s4,
    coef, pred, f, f_new, rejected (trials whose values were not kept), kept (the tangent step that was kept, or None), decidable (every trial's gain ratio is further than
    `margin` from 0, 0.25 and 0.75)."""
    H, gv, arr = system(p)
    s4, dn = scalars(H, gv, arr)
    s4l, _ = scalars(H, gv, arr, np.longdouble)
    f = cost(p)
    last, trials, stay, decidable, rejected = NONE, 0, True, True, 0
    while stay:
        alpha, beta, norm, pred, branch = point(s4, delta)
        dd = alpha * gv + beta * dn
        q = retracted(p, dd)
        f_new = cost(q)
        trials += 1
        rho = gain(f, f_new, pred)
        if np.isfinite(rho):
            m = margin(f, f_new, s4, s4l, alpha, beta)
            decidable = decidable and min(abs(rho - t) for t in (0.0, 0.25, 0.75)) > m
        keep, stay, delta, last = decide(f, f_new, pred, norm, mode, delta, last)
        rejected += not keep
    accepted = bool(keep and not f_new > f and f_new == f_new)
    return dict(p=q if accepted else p, delta=delta, trials=trials, accepted=accepted, branch=branch, s4=s4, coef=(alpha, beta), pred=pred,
                f=f, f_new=f_new, rejected=rejected, kept=dd if accepted else None, decidable=decidable, error_after=f_new if accepted else f,
                dinf=float(np.abs(dd).max()) if accepted else 0.0)


def optimize(p, delta_initial=1.0, mode=ONE_STEP, max_iterations=100, relative_error_tol=1e-5, absolute_error_tol=1e-5, error_tol=0.0,
             delta_tol=0.0):
    """(description at the end, iterations, error, delta)"""
    new_err = cost(p)
    delta, iters = delta_initial, 0
    if not new_err <= error_tol:
        while True:
            cur = new_err
            it = iterate(p, delta, mode)
            p, delta, new_err = it["p"], it["delta"], it["error_after"]
            iters += 1
            if iters >= max_iterations or new_err <= error_tol:
                break
            if (cur - new_err) / cur <= relative_error_tol or cur - new_err <= absolute_error_tol:
                break
            if delta_tol > 0.0 and it["dinf"] < delta_tol:
                break
    return p, iters, new_err, delta


def perturbed(p, scale, seed=3):
    """p at x (+) scale * (a seeded standard normal tangent vector)"""
    rng = np.random.default_rng(seed)
    N, d = p["pose"].shape[0], O.TANGENT_DIM[p["kind"]]
    nl = p["landmarks"].size if "landmarks" in p else 0
    return retracted(p, scale * rng.standard_normal(N * 2 * d + nl))


def twin_distance(arr):
    """the distance between the block-form g^T H g in float64 and in np.longdouble, relative"""
    a, b = block_quad(arr, np.float64), block_quad(arr, np.longdouble)
    return float(abs(np.longdouble(a) - b) / abs(b))


# ---------------------------------------------------------------------------------------------------------------- the test graphs
# (family, with landmarks, states): the families of tests/fixed_lag_mix_model.py at their NS sizes, with and without landmarks where
# the graph exists both ways (r3's bearing-range factors need them), and the sizes the device's kernels change their course at
FAMILY = [("se2", True, None), ("se2", False, None), ("se3", True, None), ("se3", False, None), ("se3_vw", False, None),
          ("so3", False, None), ("r3", True, None)]
SIZES = [("se3", False, 2), ("se2", True, 2), ("se3", False, 300), ("se2", True, 300), ("se3", False, 1025)]
ROBUST = "se3"      # the robust graph of the GPU tests: Huber, Cauchy and Tukey factors on GPS, range and projection factors
# (family, with landmarks, perturbation scale, its seed, first trust radius): from these starts the model rejects trials (rho < 0) in
# every mode within the first four iterations, all of them decidable (tests/test_dogleg_model.py holds both)
LOCKSTEP = [("se2", True, 3.0, 4, 1000.0), ("r3", True, 3.0, 4, 1000.0)]
LOCKSTEP_ITERATIONS = 6
# mode 1 takes three trials in its first iteration from here (the one-solve-per-iteration census)
THREE_TRIALS = ("se2", True, 3.0, 4, 30.0)


def graph(name, landmarks=True, N=None, robust=False):
    n = FM.NS[name] if N is None else N
    return FM.graph(name, n, min(5, n - 1), robust=robust, chart=O.CHART_FIRST_ORDER if name == "se2" else O.CHART_EXPMAP,
                    seed=MX.ROBUST_SEED[name] if robust else 7, landmarks=landmarks)


def lockstep(name, landmarks, scale, seed, delta, mode, iterations=LOCKSTEP_ITERATIONS):
    """the model's run: a list of iterate()'s dicts"""
    p = perturbed(graph(name, landmarks), scale, seed)
    out = []
    for _ in range(iterations):
        r = iterate(p, delta, mode)
        p, delta = r["p"], r["delta"]
        out.append(r)
    return out
