"""Problem descriptions for fixed-lag smoothing on every factor and noise model: plain numpy plus the oracle.

The description format of fixed_lag_model.FACTOR_KEYS / fixed_lag_border_model.FACTOR_KEYS (a dict of per-factor arrays, one index
key per kind of factor) gains
  brange_*   bearing-range (idx, lm, meas = [bearing, range], sigma)
  odo_*      odometry2d (left, meas, sigma)
  proj_*     interpolated projection (left, lm, meas, sigma, dt, tau, K: one calibration per factor)
  prange_*   plain range, also on a handle that does not marginalise onto the landmarks (its head factors are dropped then)
  gp_qc      one Qc per GP prior (count x d x d); rows of NaN: the handle's Qc
  gps_cov    a full covariance per interpolated GPS factor (count x 3 x 3); rows of NaN: the diagonal sigmas
  *_sensor   body_P_sensor per factor; rows of NaN: none
  *_loss, *_k   the robust loss (gpslam_amd.chain.ROBUST_*, 0: none) and its parameter per factor
  *_call     the add_* call a factor arrives in.  apply() issues one call per run of equal call numbers, and the options that an ABI
             call takes once (sensor, calibration) or that are set "on the most recently added" (covariance, loss) must be uniform in it.
  apply       a description onto oracle.Chain or gpslam_amd.ChainSolver (the oracle has no robust model: it takes `reweighted` ones)
  chain       the solver a description asks for (chart, landmark dimension, velocity_world)
  head_tail, window   the cuts of fixed_lag_border_model.head_tail and of the sliding tests, over every key above
  drop_head_landmark_factors   the description a handle without marginalize_head_onto_landmarks can marginalise
  reweighted  the plain description whose sigmas are sigma / sqrt(w) (covariance cov / w): what a robust handle linearises like
              (tests/test_gpu_robust.py); w = 0 on diagonal sigmas is sigma = inf
  whitened_norms   |whitened error| per factor from unwhitened errors
  graph       the test graphs: every per-factor quantity differs from factor to factor, every kind arrives in two or three calls
              (without the option, then with it), each call in a seeded shuffled order of its states
"""
import numpy as np

from gpslam_amd import chain as GC
from oracle import oracle as O
import fixed_lag_model as FL
import fixed_lag_border_model as FB

E = O.CHART_EXPMAP
LD = FB.LD
# prefix -> (MEAS_* kind, index key, the factor touches idx + 1 too, rows, names a landmark, required per-factor arrays)
MEAS = {
    "range": (0, "range_left", True, 1, True, ("lm", "z", "sigma", "dt", "tau")),
    "prange": (1, "prange_idx", False, 1, True, ("lm", "z", "sigma")),
    "att": (2, "att_left", True, 2, False, ("nz", "bref", "sigma", "dt", "tau")),
    "gps": (3, "gps_left", True, 3, False, ("meas", "sigma", "dt", "tau")),
    "odo": (4, "odo_left", True, 3, False, ("meas", "sigma")),
    "brange": (5, "brange_idx", False, 2, True, ("lm", "meas", "sigma")),
    "proj": (6, "proj_left", True, 2, True, ("lm", "meas", "sigma", "dt", "tau", "K")),
}
OPTIONAL = ("call", "sensor", "cov", "loss", "k")
FACTOR_KEYS = {
    "gp_left": (["gp_dt", "gp_qc", "gp_call"], True),
    "prior_idx": (["prior_pose", "prior_sig"], False),
    "vprior_idx": (["vprior", "vprior_sig"], False),
    "between_left": (["between_meas", "between_sig"], True),
}
for _pre, (_mk, _key, _two, _rows, _haslm, _req) in MEAS.items():
    FACTOR_KEYS[_key] = (["%s_%s" % (_pre, n) for n in _req + OPTIONAL], _two)
PASS_KEYS = ("kind", "qc", "chart", "velocity_world", "ld", "landmarks", "lprior_idx", "lprior", "lprior_sig")
K_CAL = np.array([500.0, 480.0, 0.5, 320.0, 240.0])


def chain(p, cls=O.Chain, **kw):
    return cls(p["kind"], chart=p.get("chart", E), landmark_dim=p.get("ld", 0), velocity_world=bool(p.get("velocity_world", False)), **kw)


def _runs(call, n):
    """[(a, b)]: the runs of equal call numbers among n factors (one run without call numbers)"""
    if n == 0:
        return []
    if call is None:
        return [(0, n)]
    cut = [0] + [f for f in range(1, n) if call[f] != call[f - 1]] + [n]
    return list(zip(cut[:-1], cut[1:]))


def _uniform(a, what):
    """the one value of an option within a call (None: rows of NaN), or an error"""
    a = np.asarray(a)
    nan = np.isnan(a.reshape(a.shape[0], -1)).all(axis=1)
    if nan.all():
        return None
    if nan.any() or not all(np.array_equal(a[0], x) for x in a[1:]):
        raise ValueError("%s differs within one call" % what)
    return a[0]


def _add(solver, pre, q):
    """one add_* call of the factors q (the description's arrays of one run, by their short names)"""
    i = q["idx"]
    sensor = _uniform(q["sensor"], pre + "_sensor") if "sensor" in q else None
    if pre == "range":
        solver.add_interp_range(i, q["lm"], q["z"], q["sigma"], q["dt"], q["tau"], sensor)
    elif pre == "prange":
        solver.add_range(i, q["lm"], q["z"], q["sigma"])
    elif pre == "att":
        solver.add_interp_attitude(i, q["nz"], q["bref"], q["sigma"], q["dt"], q["tau"])
    elif pre == "gps":
        solver.add_interp_gps(i, q["meas"], q["sigma"], q["dt"], q["tau"], sensor)
    elif pre == "odo":
        solver.add_odometry2d(i, q["meas"], q["sigma"])
    elif pre == "brange":
        solver.add_bearing_range(i, q["lm"], q["meas"][:, 0], q["meas"][:, 1], q["sigma"])
    elif pre == "proj":
        solver.add_interp_projection(i, q["lm"], q["meas"], q["sigma"], q["dt"], q["tau"], _uniform(q["K"], "proj_K"), sensor)
    mk = MEAS[pre][0]
    if "cov" in q:
        fin = np.isfinite(np.asarray(q["cov"]).reshape(len(i), -1)).all(axis=1)
        if fin.any():
            if not fin.all():
                raise ValueError("%s_cov: full and diagonal models within one call" % pre)
            solver.set_meas_covariance(mk, q["cov"])
    if "loss" in q and np.any(np.asarray(q["loss"]) != 0):
        if not np.all(np.asarray(q["loss"]) != 0):
            raise ValueError("%s_loss: factors with and without a loss within one call" % pre)
        if not hasattr(solver, "set_meas_robust"):
            raise ValueError("the oracle has no robust model: give it reweighted(p, w)")
        solver.set_meas_robust(mk, q["loss"], q["k"])


def add_factors(p, solver):
    """every factor of the description, one call per run of call numbers, in the description's order"""
    n = len(p["gp_left"])
    for a, b in _runs(p.get("gp_call"), n):
        qc = _uniform_qc(p["gp_qc"][a:b]) if "gp_qc" in p else None
        if qc is None:
            solver.add_gp_priors(p["gp_left"][a:b], p["gp_dt"][a:b])
        else:
            solver.add_gp_priors_qc(p["gp_left"][a:b], p["gp_dt"][a:b], qc)
    if "prior_idx" in p and len(p["prior_idx"]):
        solver.add_pose_priors(p["prior_idx"], p["prior_pose"], p["prior_sig"])
    if "vprior_idx" in p and len(p["vprior_idx"]):
        solver.add_vel_priors(p["vprior_idx"], p["vprior"], p["vprior_sig"])
    if "between_left" in p and len(p["between_left"]):
        solver.add_between(p["between_left"], p["between_meas"], p["between_sig"])
    for pre, (mk, key, two, rows, haslm, req) in MEAS.items():
        if key not in p:
            continue
        for a, b in _runs(p.get(pre + "_call"), len(p[key])):
            q = {n: np.asarray(p["%s_%s" % (pre, n)])[a:b] for n in req + OPTIONAL if "%s_%s" % (pre, n) in p}
            q["idx"] = np.asarray(p[key])[a:b]
            _add(solver, pre, q)


def _uniform_qc(qc):
    nan = np.isnan(qc.reshape(qc.shape[0], -1)).all(axis=1)
    if nan.all():
        return None
    if nan.any():
        raise ValueError("gp_qc: the handle's Qc and per-factor ones within one call")
    return qc


def apply(p, solver):
    solver.set_qc(p["qc"])
    solver.set_states(p["pose"], p["vel"])
    if "landmarks" in p:
        solver.set_landmarks(p["landmarks"])
        if "lprior_idx" in p:
            solver.add_landmark_priors(p["lprior_idx"], p["lprior"], p["lprior_sig"])
    add_factors(p, solver)
    solver.compile()
    return solver


def _cut(p, out, mask_of, shift):
    for key, (others, two) in FACTOR_KEYS.items():
        if key not in p:
            continue
        idx = np.asarray(p[key])
        m = mask_of(idx, idx + (1 if two else 0))
        out[key] = (idx[m] - shift).astype(np.int32)
        for o in others:
            if o in p:
                out[o] = np.asarray(p[o])[m]
    return out


def head_tail(p, k):
    """(head, tail): states 0 .. k with every factor whose (left) state is < k, the landmarks' positions, no landmark priors; states
    k .. with the other factors, indices lowered by k, and the landmark priors.  Factors keep their order and their call numbers."""
    N = p["pose"].shape[0]
    head = {key: p[key] for key in PASS_KEYS if key in p and not key.startswith("lprior")}
    head.update(N=k + 1, pose=p["pose"][:k + 1].copy(), vel=p["vel"][:k + 1].copy())
    tail = {key: p[key] for key in PASS_KEYS if key in p}
    tail.update(N=N - k, pose=p["pose"][k:].copy(), vel=p["vel"][k:].copy())
    _cut(p, head, lambda idx, last: idx < k, 0)
    _cut(p, tail, lambda idx, last: idx >= k, k)
    return head, tail


def window(p, lo, hi, new_from=None):
    """The states lo .. hi - 1 and the factors that touch only them -- with new_from, only those that also touch a state >= new_from
    (what a window gains when states new_from .. hi - 1 are appended).  Landmarks and their priors stay."""
    out = {key: p[key] for key in PASS_KEYS if key in p}
    out.update(N=hi - lo, pose=p["pose"][lo:hi].copy(), vel=p["vel"][lo:hi].copy())
    return _cut(p, out, lambda idx, last: (idx >= lo) & (last < hi) & ((last >= new_from) if new_from is not None else True), lo)


def drop_head_landmark_factors(p, k):
    """p without the factors of states < k that name a landmark: what marginalize_head accepts without the landmark option"""
    out = dict(p)
    for pre, (mk, key, two, rows, haslm, req) in MEAS.items():
        if not haslm or key not in p:
            continue
        m = np.asarray(p[key]) >= k
        for name in [key] + FACTOR_KEYS[key][0]:
            if name in p:
                out[name] = np.asarray(p[name])[m]
    return out


def without_factor(p, pre, f):
    """p without factor f of one measurement kind"""
    out = dict(p)
    key = MEAS[pre][1]
    m = np.arange(len(p[key])) != f
    for name in [key] + FACTOR_KEYS[key][0]:
        if name in p:
            out[name] = np.asarray(p[name])[m]
    return out


def robust_kinds(p):
    return [pre for pre in MEAS if pre + "_loss" in p]


def plain(p):
    """p without its losses"""
    return {key: v for key, v in p.items() if not key.endswith(("_loss", "_k"))}


def reweighted(p, w):
    """The plain description that a robust handle with weights w (prefix -> one weight per factor of that kind) linearises like:
    sigma / sqrt(w), covariance / w.  w = 1 leaves every number as it is; w = 0 on diagonal sigmas gives sigma = inf."""
    out = plain(p)
    for pre, wf in w.items():
        wf = np.asarray(wf, dtype=np.float64)
        sig = np.asarray(p[pre + "_sigma"], dtype=np.float64)
        assert wf.shape == (sig.shape[0],)
        with np.errstate(divide="ignore"):
            out[pre + "_sigma"] = sig / np.sqrt(wf).reshape((-1,) + (1,) * (sig.ndim - 1))
            if pre + "_cov" in p:
                out[pre + "_cov"] = np.asarray(p[pre + "_cov"]) / wf[:, None, None]
    return out


def whitened_norms(p, pre, e):
    """|whitened error|_2 per factor from the unwhitened errors e (count x rows) of one kind"""
    e = np.asarray(e).reshape(len(p[MEAS[pre][1]]), MEAS[pre][3])
    sig = np.asarray(p[pre + "_sigma"]).reshape(e.shape)
    r = np.sqrt(np.sum((e / sig) ** 2, axis=1))
    if pre + "_cov" in p:
        cov = np.asarray(p[pre + "_cov"])
        for f in np.nonzero(np.isfinite(cov).all(axis=(1, 2)))[0]:
            r[f] = np.sqrt(e[f] @ np.linalg.solve(cov[f], e[f]))
    return r


LOSS_NAMES = {GC.ROBUST_HUBER: "HUBER", GC.ROBUST_CAUCHY: "CAUCHY", GC.ROBUST_TUKEY: "TUKEY",
              GC.ROBUST_GEMAN_MCCLURE: "GEMAN_MCCLURE", GC.ROBUST_WELSH: "WELSH", GC.ROBUST_FAIR: "FAIR"}
GRAPH_LOSSES = (GC.ROBUST_HUBER, GC.ROBUST_CAUCHY, GC.ROBUST_TUKEY)      # the losses graph() deals out


def robust_weights(p, errors, scale=1.0):
    """prefix -> (r, w) of a robust description from the unwhitened errors of its plain twin (prefix -> count x rows): r the whitened
    norms, w = np_loss of each factor's own (loss, k) at r, 1 without a loss; `scale` multiplies w where a loss acts (the probe of
    how far the reference moves with the weights)"""
    from test_gpu_robust import np_loss
    out = {}
    for pre in robust_kinds(p):
        r = whitened_norms(p, pre, errors[pre])
        w = np.ones(len(r))
        for f, (loss, k) in enumerate(zip(p[pre + "_loss"], p[pre + "_k"])):
            if loss:
                w[f] = float(np_loss(LOSS_NAMES[int(loss)], float(k), r[f])[0]) * scale
        out[pre] = (r, w)
    return out


def check_populations(p, rw, k_head, losses=GRAPH_LOSSES):
    """every loss sees residuals on both sides of its k, none within 1e-6 relative of a kink, a Tukey factor of the head has w = 0
    (`losses`: the ones the description carries, where they are not graph()'s; without Tukey among them no factor need be dead)"""
    below, above, dead = set(), set(), False
    for pre, (r, w) in rw.items():
        idx = np.asarray(p[MEAS[pre][1]])
        for f, (loss, k) in enumerate(zip(p[pre + "_loss"], p[pre + "_k"])):
            if not loss:
                continue
            (below if r[f] < k else above).add(int(loss))
            if loss in (GC.ROBUST_HUBER, GC.ROBUST_TUKEY):
                assert abs(r[f] - k) > 1e-6 * k, (pre, f, r[f], k)
            dead |= bool(loss == GC.ROBUST_TUKEY and idx[f] < k_head and w[f] == 0.0)
    assert below == above == set(losses), (below, above)
    assert dead or GC.ROBUST_TUKEY not in losses


def plain_errors(p, solver):
    """prefix -> unwhitened errors of every kind that carries a loss, from a solver that holds plain(p)"""
    return {pre: solver.linearize_meas(MEAS[pre][0], len(p[MEAS[pre][1]]))[0] if len(p[MEAS[pre][1]]) else np.zeros((0, MEAS[pre][3]))
            for pre in robust_kinds(p)}


def head_reference(p, k, onto, dtype=np.float64, gaussians=()):
    """(Lambda, gamma, scale of Lambda, scale of gamma) of the head of a plain description on the oracle's arrays: the border
    recursion with `onto`, else the state recursion (scales as tests/test_gpu_fixed_lag_border.py / test_gpu_fixed_lag.py take them).
    gaussians: state Gaussians (idx, pose_lin, vel_lin, A, c) -- with onto border Gaussians (idx, pose_lin, vel_lin, lm_lin, A, c) --
    inside the head, added to the arrays before the recursion."""
    head, _ = head_tail(p, k)
    arrays = apply(head, chain(head)).normal_equations()
    if onto:
        if gaussians:
            arrays = with_border_gaussians(arrays, p["kind"], p.get("chart", E), head["pose"], head["vel"], head["landmarks"], gaussians)
        return FB.schur_border(*arrays, k, dtype)
    D, Om, g = arrays[:3]
    if gaussians:
        D, g = with_state_gaussians(D, g, p["kind"], p.get("chart", E), head["pose"], head["vel"], gaussians)
    Lam, gam, _ = FL.schur(D, Om, g, k, dtype)
    return Lam, gam, float(np.abs(D[k]).max()), float(np.abs(g).max())


# ---------------------------------------------------------------------------------------------------------------- the graphs
NS = {"se2": 14, "se3": 13, "se3_vw": 12, "so3": 15, "r3": 16}      # states of a graph of the family
HAS_LANDMARKS = ("se2", "se3", "r3")
LONG = [("se3", 300, 257), ("se3", 300, 100), ("se3", 300, 299), ("se2", 300, 257), ("se2", 300, 100), ("se2", 300, 299)]


def family():
    """[(name, k, onto)]: every graph at k = 1, 5, N - 1, with and without the landmark option where it has landmarks"""
    return [(name, k, onto) for name, N in NS.items() for k in (1, 5, N - 1) for onto in ((True, False) if name in HAS_LANDMARKS else (False,))]


def case(name, k, onto, robust=False, chart=E, N=None):
    """the description of one case: without `onto`, without the head's landmark factors"""
    p = graph(name, NS[name] if N is None else N, k, robust=robust, chart=chart, landmarks=not (N is not None and name == "se3"))
    return p if onto else drop_head_landmark_factors(p, k)


GRAPHS = {"se2": ("pose2", False), "se3": ("pose3", False), "se3_vw": ("pose3", True), "so3": ("rot3", False), "r3": ("linear3", False)}
KINDS = {"linear3": O.LINEAR3, "pose2": O.POSE2, "rot3": O.ROT3, "pose3": O.POSE3}


def _identity(kind):
    if kind == O.POSE3:
        return O.pose3((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    if kind == O.ROT3:
        return O.rot3_ypr(0.0, 0.0, 0.0)
    return np.zeros(O.POSE_DIM[kind])


def _spread(rng, n, base, rel=0.5):
    """n different values in base * [1, 1 + rel)"""
    return base * (1.0 + rel * (np.arange(n) + rng.random(n)) / max(n, 1))[rng.permutation(n)]


def _calls(rng, two, N, k, ncalls):
    """(idx, call): call 0 every state / interval, the later calls a random half plus k - 1 and k; each call in a shuffled order"""
    top = N - 1 if two else N
    idx, call = [], []
    for c in range(ncalls):
        pick = np.arange(top) if c == 0 else np.union1d(np.nonzero(rng.random(top) < 0.5)[0], [j for j in (k - 1, k, 0) if j < top])
        pick = rng.permutation(pick)
        idx.append(pick)
        call.append(np.full(len(pick), c))
    return np.concatenate(idx).astype(np.int32), np.concatenate(call).astype(np.int32)


def _pick_landmarks(rng, idx, k, roles):
    """roles = (head only, tail only, [both ...]): a landmark per factor; the first head factor names the head-only one, the first tail
    factor the tail-only one"""
    H, T, both = roles[0], roles[1], list(roles[2:])
    lm = np.zeros(len(idx), dtype=np.int32)
    seen = set()
    for f, i in enumerate(idx):
        own = H if i < k else T
        if (i < k) not in seen:
            seen.add(i < k)
            lm[f] = own
        else:
            lm[f] = rng.choice([own] + both + both)
    return lm


def graph(name, N=14, k=5, robust=False, chart=E, seed=7, landmarks=True):
    """One seeded test graph (module docstring; the table of tests/test_gpu_fixed_lag_mix.py).  Landmark roles: one landmark is named
    only by factors of states < k, one only by the others (k = N - 1 may leave it to its prior), the rest by both; on se3 the two are
    landmarks no camera looks at.  landmarks=False: the graph without its landmarks and the factors that name one."""
    from test_gpu_parity import random_chain
    base, vw = GRAPHS[name]
    kind = KINDS[base]
    d = O.TANGENT_DIM[kind]
    rng = np.random.default_rng(1000 * seed + 17 * N + k)
    c = random_chain(kind, N, 3)
    dt = c["dt"]
    between = np.stack([O.retract(kind, _identity(kind), dt[j] * c["truth_vel"][j]) for j in range(N - 1)])
    if vw:
        from test_gpu_vw import world_velocities
        c.update(world_velocities(c))
    p = dict(kind=kind, chart=chart, velocity_world=vw, N=N, qc=np.diag(0.5 + rng.random(d)), pose=c["pose"], vel=c["vel"])
    # GP priors in two calls; on se2 and so3 the second call carries one Qc per interval
    order = rng.permutation(N - 1)
    half = (N - 1) // 2
    gl = np.concatenate([order[:half], order[half:]]).astype(np.int32)
    p.update(gp_left=gl, gp_dt=dt[gl], gp_call=(np.arange(N - 1) >= half).astype(np.int32))
    if name in ("se2", "so3"):
        qc = np.full((N - 1, d, d), np.nan)
        for f in range(half, N - 1):
            qc[f] = np.diag(0.4 + 0.02 * f / N + rng.random(d))
            qc[f][0, 1] = qc[f][1, 0] = 0.05 + 0.05 * rng.random()
        p["gp_qc"] = qc
    at = rng.permutation(np.unique([0, max(k - 1, 0), k, N - 1])).astype(np.int32)
    p.update(prior_idx=at, prior_pose=c["truth_pose"][at].copy(), prior_sig=_spread(rng, len(at) * d, 0.05).reshape(len(at), d))
    at = rng.permutation(np.unique([0, max(k - 1, 0), k])).astype(np.int32)
    p.update(vprior_idx=at, vprior=c["truth_vel"][at].copy(), vprior_sig=_spread(rng, len(at) * d, 0.1).reshape(len(at), d))
    bl = rng.permutation(N - 1).astype(np.int32)
    p.update(between_left=bl, between_meas=between[bl], between_sig=_spread(rng, (N - 1) * d, 0.05).reshape(N - 1, d))

    def interp(pre, idx):
        M = len(idx)
        p[pre + "_dt"] = dt[idx] * _spread(rng, M, 1.0, 0.02)
        p[pre + "_tau"] = p[pre + "_dt"] * _spread(rng, M, 0.1, 8.0)

    L = {"se2": 3, "se3": 4, "r3": 3}.get(name, 0) if landmarks else 0
    roles = list(range(L))
    if L:
        ld = LD[kind]
        p["ld"] = ld
        xy = FB.positions(kind, c["truth_pose"])
        if name == "se3":
            # four landmarks 30 m out in tetrahedral directions (tests/test_gpu_robust.py): a camera looks at the one nearest its axis
            lands = xy.mean(0) + 30.0 / np.sqrt(3.0) * np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])
        else:
            ang = rng.uniform(0.0, 2.0 * np.pi) + 2.0 * np.pi * np.arange(L) / L
            lands = xy.mean(0) + rng.uniform(5.0, 8.0, L)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        p.update(landmarks=lands + 0.1 * rng.standard_normal((L, ld)), lprior_idx=np.arange(L, dtype=np.int32), lprior=lands.copy(),
                 lprior_sig=_spread(rng, L * ld, 0.5).reshape(L, ld))
    if name == "se3" and L:
        # the projection factors: the landmark nearest the camera axis (body z) of the factor's left state
        idx, call = _calls(rng, True, N, k, 2)
        tp = c["truth_pose"]
        zc = np.einsum("nj,nlj->nl", tp[idx, :9].reshape(-1, 3, 3)[:, :, 2], lands[None] - tp[idx, None, 9:12])
        plm = np.argmax(zc, axis=1).astype(np.int32)
        free = [l for l in range(L) if l not in set(plm.tolist())]
        assert len(free) >= 2, "the cameras look at more than two landmarks"
        roles = free[:2] + [l for l in range(L) if l not in free[:2]]
        M = len(idx)
        Kc = np.where((call == 0)[:, None], K_CAL, K_CAL * np.array([1.1, 0.9, 1.5, 1.02, 0.97]))
        p.update(proj_left=idx, proj_call=call, proj_lm=plm, proj_sigma=np.stack([_spread(rng, M, 20.0), _spread(rng, M, 25.0)], axis=1), proj_K=Kc,      # (0.05 rad of initial error are 25 px)
                 proj_sensor=np.where((call == 0)[:, None], np.nan, O.pose3((0.05, -0.03, 0.02), (0.1, -0.05, 0.08))))
        interp("proj", idx)
    if name in ("se2", "se3") and L:
        ncalls = 3 if name == "se2" else 2
        idx, call = _calls(rng, True, N, k, ncalls)
        M = len(idx)
        if name == "se2":
            sens = np.where((call == 0)[:, None], np.nan, np.where((call == 1)[:, None], [0.2, -0.1, 0.3], [-0.15, 0.25, -0.4]))
        else:
            sens = np.where((call == 0)[:, None], np.nan, O.pose3((0.3, -0.2, 0.1), (0.2, -0.1, 0.3)))
        p.update(range_left=idx, range_call=call, range_lm=_pick_landmarks(rng, idx, k, roles), range_sigma=_spread(rng, M, 0.1), range_sensor=sens)
        interp("range", idx)
    if name in ("se2", "r3") and L:
        idx, call = _calls(rng, False, N, k, 2)
        p.update(prange_idx=idx, prange_call=call, prange_lm=_pick_landmarks(rng, idx, k, roles), prange_sigma=_spread(rng, len(idx), 0.1))
    if name == "r3":
        idx, call = _calls(rng, False, N, k, 2)
        M = len(idx)
        p.update(brange_idx=idx, brange_call=call, brange_lm=_pick_landmarks(rng, idx, k, roles),
                 brange_sigma=np.stack([_spread(rng, M, 0.02), _spread(rng, M, 0.1)], axis=1))
        idx, call = _calls(rng, True, N, k, 2)
        p.update(odo_left=idx, odo_call=call, odo_sigma=_spread(rng, 3 * len(idx), 0.08).reshape(len(idx), 3))
    if name in ("se3", "se3_vw"):
        idx, call = _calls(rng, True, N, k, 3 if name == "se3" else 2)
        M = len(idx)
        sig = _spread(rng, 3 * M, 0.1).reshape(M, 3)
        p.update(gps_left=idx, gps_call=call, gps_sigma=sig, gps_sensor=np.where((call == 1)[:, None], O.pose3((1.4, 4.4, -0.5), (0.3, 0.6, -0.7)), np.nan))
        if name == "se3":
            Cm = np.array([[0.0, 0.3, -0.2], [0.3, 0.0, 0.25], [-0.2, 0.25, 0.0]])
            cov = np.full((M, 3, 3), np.nan)
            for f in np.nonzero(call == 2)[0]:
                cov[f] = np.outer(sig[f], sig[f]) * (np.eye(3) + (0.3 + 0.7 * (f + 1) / M) * Cm)
            p["gps_cov"] = cov
        interp("gps", idx)
    if name == "so3":
        idx, call = _calls(rng, True, N, k, 2)
        M = len(idx)
        R = c["truth_pose"][idx].reshape(M, 3, 3)
        nz = R[:, :, 2] + 0.05 * rng.standard_normal((M, 3))
        p.update(att_left=idx, att_call=call, att_nz=nz / np.linalg.norm(nz, axis=1, keepdims=True), att_bref=np.tile([0.0, 0.0, 1.0], (M, 1)),
                 att_sigma=np.stack([_spread(rng, M, 0.1), _spread(rng, M, 0.12)], axis=1))
        interp("att", idx)
    # measurements: the oracle's own prediction at the true states (its error at z = 0), noise, and on a robust graph about one factor in
    # five displaced by 30-80 sigma; the first factor of the head that carries a Tukey loss is displaced whatever the draw
    zero = dict(p, pose=c["truth_pose"], vel=c["truth_vel"])
    if L:
        zero["landmarks"] = lands
    names = {"range": "z", "prange": "z", "gps": "meas", "odo": "meas", "brange": "meas", "proj": "meas"}
    for pre, target in names.items():
        key = MEAS[pre][1]
        if key in p:
            M, rows = len(p[key]), MEAS[pre][3]
            zero["%s_%s" % (pre, target)] = np.zeros(M) if target == "z" else np.zeros((M, rows))
    orc = apply(zero, chain(zero))
    for pre, target in names.items():
        key = MEAS[pre][1]
        if key not in p:
            continue
        mk, _, _, rows = MEAS[pre][:4]
        M = len(p[key])
        pred, _ = orc.linearize_meas(mk, M)
        sig = np.asarray(p[pre + "_sigma"]).reshape(M, rows)
        z = pred + sig * rng.standard_normal((M, rows))
        if robust:
            call = p[pre + "_call"]
            loss = np.where(call == 0, 0, np.array([GC.ROBUST_HUBER, GC.ROBUST_CAUCHY, GC.ROBUST_TUKEY])[np.arange(M) % 3]).astype(np.int32)
            if pre + "_cov" in p:
                loss[call == 2] = GC.ROBUST_CAUCHY
            head = np.asarray(p[key]) < k
            if not ((loss == GC.ROBUST_TUKEY) & head).any():
                loss[np.nonzero((call == 1) & head)[0][0]] = GC.ROBUST_TUKEY
            out = rng.random(M) < 0.2
            for which in (GC.ROBUST_HUBER, GC.ROBUST_CAUCHY, GC.ROBUST_TUKEY):      # every loss sees both populations; Tukey's displaced one is in the head
                fs = np.nonzero(loss == which)[0]
                fs = np.concatenate([fs[head[fs]], fs[~head[fs]]])
                out[fs[:1]] = True
                out[fs[1:2]] = False
            disp = rng.uniform(30, 80, (M, rows)) * sig * np.where(rng.random((M, rows)) < 0.5, -1.0, 1.0)
            z = z + np.where(out[:, None], disp, 0.0)
            p[pre + "_loss"] = loss
            p[pre + "_k"] = _spread(rng, M, 3.5, 1.2)
        p["%s_%s" % (pre, target)] = z[:, 0] if target == "z" else z
    return p


def with_state_gaussians(D, g, kind, chart, pose, vel, gaussians):
    """fixed_lag_model.gn_step's way of adding state Gaussians (idx, pose_lin, vel_lin, A, c) to the oracle's D, g at (pose, vel)"""
    D, g = D.copy(), g.copy()
    for idx, pl, vl, A, c in gaussians:
        xi = FL.xi_of(kind, chart, pl, vl, pose[idx], vel[idx])
        D[idx] += A.T @ A
        g[idx] += A.T @ (c - A @ xi)
    return D, g


def with_border_gaussians(arrays, kind, chart, pose, vel, lm, gaussians):
    """fixed_lag_border_model.system's way of adding border Gaussians (idx, pose_lin, vel_lin, lm_lin, A, c) to the oracle's six arrays:
    the state block, the state-landmark block and the landmark blocks"""
    D, Om, g, B, HLL, gL = (a.copy() for a in arrays)
    b = D.shape[1]
    for idx, pl, vl, ll, A, c in gaussians:
        xi = FB.xi_of(kind, chart, pl, vl, ll, pose[idx], vel[idx], lm)
        H = A.T @ A
        rhs = A.T @ (c - A @ xi)
        D[idx] += H[:b, :b]
        B[idx] += H[:b, b:]
        HLL += H[b:, b:]
        g[idx] += rhs[:b]
        gL += rhs[b:]
    return D, Om, g, B, HLL, gL
