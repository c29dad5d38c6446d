"""Statistics of posterior draws reduced on the device (include/gpslam_hip_sampling_stats.h, gpslam_amd/csrc/sampling.hip:
k_ps_moments, k_ps_paths) against tests/posterior_stats_model.py applied to the device's own draws.

Graphs and query sets are tests/test_gpu_sampling_at.py's (posterior_stats_model.CASES names them): every manifold the bridge accepts,
SE(2) under both charts, one query on two states, 300 queries on 301 SE(2) states (one in every interval) and 64 queries in each of
the 299 intervals of the 300-state SE(3) graph -- neither a multiple of a workgroup, both more than one.  The obstacle sets are the
model module's; tests/test_posterior_stats_model.py holds them off the boundary on the CPU.

Bounds.
  Against the device's own draws (the model on sample_posterior_at's query_poses of the same noise and on interpolate_poses of the
    estimate), from POSE_TOL = 1e-11, the bar interpolated poses are held to: 1e-11 count max(1, max |eta|) for s1, that with
    max(1, max |eta|)^2 for s2, 1e-11 max(1, |x|) for clearance and length.  hits: exactly, after asserting that no clearance of the
    model on the device's draws lies within 1e-6 of zero.
  Covariance identity (vector spaces, noise = I): tests/test_gpu_sampling_at.py's rule for the diagonal blocks -- unit_noise_sum's tol
    plus 1e-9 |P|.
  Statistics at a fixed seed, 2048 draws: second moments of the whitened eta within 6 sqrt((1 + [i = j]) / K) of I, mean within 6 / sqrt(K).
Everything else is to the bit."""
import ctypes as C

import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import chain
from oracle import oracle as O
import dogleg_model as DM
import posterior_model as PM
import posterior_stats_model as SM
from test_gpu_sampling_at import graph, queries, device, reference, unit_noise_sum, check_untouched, VECTOR, VECTOR_IDS, POSE_TOL, KSLAB, _edit  # noqa: F401
from test_gpu_dogleg import ahrs_pair
from test_gpu_posterior import same_bits, SEED, FIRST, REFUSALS
from test_posterior_model import STAT_SEED, STAT_K

pytestmark = pytest.mark.gpu
KEYS = ("n", "s1", "s2", "hits", "clearance", "length")


def bits(a, b, keys=KEYS):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), k
        assert a[k] is None or np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- 1. against the device's own draws
@pytest.mark.parametrize("name,lm,N,which", SM.CASES, ids=SM.CASE_IDS)
def test_against_the_devices_own_draws(name, lm, N, which):
    p, q = SM.case(name, lm, N, which)
    kind, count = p["kind"], 3
    dev = device(p)
    nq = len(q[0])
    noise = PM.noise(SEED, FIRST, count, dev.posterior_noise_dim_at(nq))
    qp = dev.sample_posterior_at(*q, count, noise=noise)[0]
    qhat = dev.interpolate_poses(*q)
    ob = None if kind == O.ROT3 else SM.obstacles(p, *q)
    got = dev.sample_posterior_stats(*q, count, noise=noise, obstacles=ob)
    want = SM.stats(kind, p["chart"], qhat, qp, ob)
    big = max(1.0, np.abs(want["eta"]).max())
    e1, e2 = np.abs(got["s1"] - want["s1"]).max(), np.abs(got["s2"] - want["s2"]).max()
    print("%s: %d queries, %d draws: s1 %.3g of %.3g, s2 %.3g of %.3g (max |eta| %.3g)" % (name, nq, count, e1, POSE_TOL * count * big, e2, POSE_TOL * count * big ** 2, np.abs(want["eta"]).max()))
    assert got["n"] == count and got["s1"].shape == (nq, dev.d) and got["s2"].shape == (nq, dev.d * (dev.d + 1) // 2)
    assert np.abs(want["eta"]).max() > 1e-6          # (the draws moved)
    assert e1 <= POSE_TOL * count * big and e2 <= POSE_TOL * count * big ** 2
    mean, cov = SM.moments(count, got["s1"], got["s2"])
    assert np.abs(got["mean"] - mean).max() <= 1e-13 * big and np.abs(got["cov"] - cov).max() <= 1e-13 * big ** 2
    if kind == O.ROT3:
        assert got["hits"] is None and got["clearance"] is None and got["length"] is None
        return
    for key in ("clearance", "length"):
        err = (np.abs(got[key] - want[key]) / np.maximum(1.0, np.abs(want[key]))).max()
        print("  %s %s, model %s: %.3g of %.3g" % (key, got[key], want[key], err, POSE_TOL))
        assert got[key].shape == (count,) and err <= POSE_TOL
    print("  hits %d of %d, min |g| %.3g" % (want["hits"].sum(), count * nq, np.abs(want["g"]).min()))
    assert np.abs(want["g"]).min() >= 1e-6
    assert got["hits"].dtype == np.int64 and np.array_equal(got["hits"], want["hits"])
    if nq == 1:
        assert (got["length"] == 0.0).all()


# ---------------------------------------------------------------- 2. the covariance identity
@pytest.mark.parametrize("name,lm", VECTOR, ids=VECTOR_IDS)
def test_unit_noise_sums_are_the_interpolated_covariances(reference, name, lm):
    ref = reference(name, lm)
    _, tol, n_at = unit_noise_sum(ref)
    left, dt, tau = ref["q"]
    d = ref["d"]
    dev, twin = device(ref["p"]), device(ref["p"])
    got = dev.sample_posterior_stats(left, dt, tau, n_at, noise=np.eye(n_at), want=("moments",))
    twin.marginals()
    P = twin.interpolate_covariances(left, dt, tau, gp_term=True)
    worst = 0.0
    for q in range(len(left)):
        blk = SM.unpack(got["s2"][q], d)
        bound = tol + 1e-9 * np.abs(P[q]).max()
        worst = max(worst, np.abs(blk - P[q]).max() / bound)
        assert np.abs(blk - P[q]).max() <= bound, (q, np.abs(blk - P[q]).max(), bound)
    print("%s: s2 of %d unit-noise draws against interpolate_covariances(gp_term=True): worst %.3g of the bound" % (name, n_at, worst))
    assert got["n"] == n_at


# ---------------------------------------------------------------- 3. Lie groups, statistics at a fixed seed
def test_statistics_of_generated_draws_on_se3():
    p = graph("se3", False)
    q = queries(p, "runs")
    dev, twin = device(p), device(p)
    K, d = STAT_K, 6
    got = dev.sample_posterior_stats(*q, K, seed=STAT_SEED, want=("moments",))
    twin.marginals()
    P = twin.interpolate_covariances(*q, gp_term=True)
    bm, bs = PM.moment_bounds(d, K)
    wm = ws = 0.0
    for i in range(len(q[0])):
        L = np.linalg.cholesky(P[i])
        mean = np.linalg.solve(L, got["s1"][i] / K)
        S = np.linalg.solve(L, np.linalg.solve(L, SM.unpack(got["s2"][i], d) / K).T)
        wm, ws = max(wm, np.abs(mean).max() * np.sqrt(K)), max(ws, (np.abs(S - np.eye(d)) / (bs / 6.0)).max())
        assert np.abs(mean).max() <= bm, i
        assert (np.abs(S - np.eye(d)) <= bs).all(), i
    print("seed %d, %d draws, %d queries: mean at most %.2f sigma, second moments at most %.2f sigma" % (STAT_SEED, K, len(q[0]), wm, ws))
    assert got["n"] == K


# ---------------------------------------------------------------- 4. to the bit
def _small():
    p = graph("se2", True)
    q = queries(p, "runs")
    return p, q, SM.obstacles(p, *q)


def test_reruns_and_the_generators_numbers():
    p, q, ob = _small()
    out = []
    for _ in range(2):
        dev = device(p)
        out.append(dev.sample_posterior_stats(*q, 3, seed=SEED, first=FIRST, obstacles=ob, margin=0.01))
    bits(out[0], out[1])
    noise = dev.posterior_noise_at(SEED, FIRST, 3, len(q[0]))
    bits(out[0], dev.sample_posterior_stats(*q, 3, noise=noise, obstacles=ob, margin=0.01))
    assert out[0]["n"] == 3 and out[0]["hits"].sum() > 0


@pytest.mark.parametrize("name,lm", [("se2", True), ("se3", False)], ids=["se2_lm", "se3"])
def test_a_continued_call_and_single_draws(name, lm):
    p = graph(name, lm)
    q = queries(p, "runs")
    ob = SM.obstacles(p, *q)
    dev = device(p)
    five = dev.sample_posterior_stats(*q, 5, seed=SEED, first=FIRST, obstacles=ob)
    two = dev.sample_posterior_stats(*q, 2, seed=SEED, first=FIRST, obstacles=ob)
    both = dev.sample_posterior_stats(*q, 3, seed=SEED, first=FIRST + 2, obstacles=ob, resume=two)
    bits(five, both, ("n", "s1", "s2", "hits"))
    assert both["n"] == 5 and two["n"] == 2 and both["clearance"].shape == (3,)
    assert np.array_equal(five["clearance"], np.concatenate([two["clearance"], both["clearance"]]))
    assert np.array_equal(five["length"], np.concatenate([two["length"], both["length"]]))
    assert np.array_equal(five["mean"], both["mean"]) and np.array_equal(five["cov"], both["cov"])
    for k in range(5):
        one = dev.sample_posterior_stats(*q, 1, seed=SEED, first=FIRST + k, obstacles=ob)
        assert one["clearance"][0] == five["clearance"][k] and one["length"][0] == five["length"][k]
        assert one["cov"] is None and one["n"] == 1
    assert len(set(five["length"])) == 5


def test_a_call_that_spans_two_chunks():
    """ps_chunk's rule as tests/test_gpu_sampling_at.py restates it: 64 queries in every interval of the 300-state SE(3) graph make a
    chunk 17 draws; 34 draws are two chunks, against the same draws continued one per call"""
    p, q = SM.case("se3", False, 300, "dense")
    dev = device(p)
    nq = len(q[0])
    widest = max(dev.posterior_noise_dim_at(nq), dev.N * dev.b + dev.L * dev.ld, dev.N * dev.pd, nq * dev.pd)
    chunk = KSLAB // widest
    count = 34
    assert chunk < count <= 2 * chunk, chunk
    ob = SM.obstacles(p, *q)
    all_ = dev.sample_posterior_stats(*q, count, seed=SEED, first=FIRST, obstacles=ob)
    acc = None
    for k in range(count):
        acc = dev.sample_posterior_stats(*q, 1, seed=SEED, first=FIRST + k, obstacles=ob, resume=acc)
        assert acc["clearance"][0] == all_["clearance"][k] and acc["length"][0] == all_["length"][k], k
    bits(all_, acc, ("n", "s1", "s2", "hits"))
    print("chunk of %d draws (widest row %d doubles), %d draws of %d queries; hits %d" % (chunk, widest, count, nq, all_["hits"].sum()))


def test_the_handle_is_left_alone():
    p, q, ob = _small()
    dev, twin = device(p), device(p)
    before = dev.get_states() + (dev.get_landmarks(),)
    rows = dev.get_rows()
    dev.sample_posterior_stats(*q, 4, seed=3, obstacles=ob)
    same_bits(before, dev.get_states() + (dev.get_landmarks(),))
    same_bits(rows, dev.get_rows())
    same_bits(dev.sample_posterior(3, seed=SEED, first=FIRST), twin.sample_posterior(3, seed=SEED, first=FIRST))
    want = ("query_poses", "delta", "poses", "vels", "landmarks")
    same_bits(dev.sample_posterior_at(*q, 2, seed=SEED, want=want), twin.sample_posterior_at(*q, 2, seed=SEED, want=want))


# ---------------------------------------------------------------- 5. edges
def test_edges():
    p, q, ob = _small()
    dev = device(p)
    full = dev.sample_posterior_stats(*q, 3, seed=SEED, first=FIRST, obstacles=ob)
    # only what is asked for comes back, and it is what the full call returns
    parts = {("moments",): None, ("hits",): ob, ("clearance",): ob, ("length",): None, ("hits", "length"): ob, ("moments", "clearance"): ob}
    for want, obs in parts.items():
        part = dev.sample_posterior_stats(*q, 3, seed=SEED, first=FIRST, obstacles=obs, want=want)
        for key, name in (("s1", "moments"), ("s2", "moments"), ("mean", "moments"), ("cov", "moments"), ("hits", "hits"), ("clearance", "clearance"), ("length", "length")):
            assert (part[key] is None) == (name not in want), (want, key)
            assert part[key] is None or np.array_equal(part[key], full[key]), (want, key)
        assert part["n"] == 3
    # one draw
    one = dev.sample_posterior_stats(*q, 1, seed=SEED, first=FIRST, obstacles=ob)
    assert one["n"] == 1 and one["cov"] is None and np.array_equal(one["mean"], one["s1"]) and one["clearance"][0] == full["clearance"][0]
    # the margin moves every clearance by exactly its value, and only raises the counts
    for margin in (0.125, 0.3):
        m = dev.sample_posterior_stats(*q, 3, seed=SEED, first=FIRST, obstacles=ob, margin=margin)
        assert np.array_equal(m["clearance"], full["clearance"] - margin)
        assert (m["hits"] >= full["hits"]).all() and np.array_equal(m["length"], full["length"]) and np.array_equal(m["s2"], full["s2"])
    # a radius of zero and 1024 obstacles are accepted; 1025 are not
    many = np.concatenate([np.tile([[50.0, 50.0, 0.0]], (1022, 1)), ob])
    assert np.array_equal(dev.sample_posterior_stats(*q, 3, seed=SEED, first=FIRST, obstacles=many)["clearance"], full["clearance"])
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\)"):
        dev.sample_posterior_stats(*q, 1, obstacles=np.concatenate([many, many[:1]]))
    # one query: no polyline
    p2, q2 = SM.case("se3", False, 2, "one")
    st = device(p2).sample_posterior_stats(*q2, 4, seed=SEED, obstacles=SM.obstacles(p2, *q2))
    assert (st["length"] == 0.0).all() and st["length"].shape == (4,) and st["hits"].shape == (1,) and np.array_equal(st["hits"], [(st["clearance"] < 0).sum()])


# ---------------------------------------------------------------- 6. refusals
def _raw(dev, q, count=1, n_obs=0, ob=None, margin=0.0, n_draws=True, s1=True, s2=True, hits=False, clearance=False, length=False):
    """the C entry point itself (the Python call cannot ask for s1 without s2 or leave n_draws out)"""
    lib = chain._sampling_stats_lib()
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    left, dt, tau = np.ascontiguousarray(q[0], dtype=np.int32), np.ascontiguousarray(q[1]), np.ascontiguousarray(q[2])
    nq, d = len(left), dev.d
    held = dict(s1=np.zeros(nq * d), s2=np.zeros(nq * d * (d + 1) // 2), hits=np.zeros(nq, dtype=np.int64), clearance=np.zeros(count), length=np.zeros(count),
                ob=None if ob is None else np.ascontiguousarray(ob, dtype=np.float64))      # (alive until the call returns)
    ptr = lambda on, key, t=dp: held[key].ctypes.data_as(t) if on else None
    n = C.c_int64(0)
    return lib.gpslam_hip_sample_posterior_stats(dev._h, count, 1, 0, None, nq, left.ctypes.data_as(C.POINTER(C.c_int32)), dt.ctypes.data_as(dp), tau.ctypes.data_as(dp),
                                                 n_obs, ptr(ob is not None, "ob"), margin, 0, C.byref(n) if n_draws else None,
                                                 ptr(s1, "s1"), ptr(s2, "s2"), ptr(hits, "hits", lp), ptr(clearance, "clearance"), ptr(length, "length"))


def test_argument_refusals_leave_the_next_dense_call_alone():
    p, q, ob = _small()
    a, b = device(p), device(p)
    neg = ob.copy()
    neg[1, 2] = -1e-3
    calls = [
        ("every output NULL", lambda: a.sample_posterior_stats(*q, 2, want=())),
        ("hits without obstacles", lambda: a.sample_posterior_stats(*q, 2, want=("moments", "hits"))),
        ("clearance without obstacles", lambda: a.sample_posterior_stats(*q, 2, want=("clearance",))),
        ("obstacles for nothing", lambda: a.sample_posterior_stats(*q, 2, obstacles=ob, want=("moments", "length"))),
        ("negative radius", lambda: a.sample_posterior_stats(*q, 2, obstacles=neg)),
        ("negative margin", lambda: a.sample_posterior_stats(*q, 2, obstacles=ob, margin=-0.1)),
        ("count 0", lambda: a.sample_posterior_stats(*q, 0, obstacles=ob)),
        ("count < 0", lambda: a.sample_posterior_stats(*q, -2, obstacles=ob)),
        ("no queries", lambda: a.sample_posterior_stats([], [], [], 1)),
        ("unsorted left", lambda: a.sample_posterior_stats(*_edit(q, left=(9, 1)), 2)),
        ("tau = dt", lambda: a.sample_posterior_stats(*_edit(q, tau=(9, q[1][9])), 2, obstacles=ob)),
    ]
    for what, call in calls:
        with pytest.raises(gp.GpslamHipError, match=r"\(-1\)"):
            call()
        print("refused:", what)
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\).*query 9: left must be non-decreasing"):
        a.sample_posterior_stats(*_edit(q, left=(9, 1)), 2)
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\).*obstacle 1"):
        a.sample_posterior_stats(*q, 2, obstacles=neg)
    with pytest.raises(gp.GpslamHipError, match="noise must be"):
        a.sample_posterior_stats(*q, 1, noise=np.zeros((1, a.posterior_noise_dim())))
    with pytest.raises(gp.GpslamHipError, match="want"):
        a.sample_posterior_stats(*q, 1, want=("poses",))
    assert _raw(a, q, s2=False) == -1 and _raw(a, q, s1=False) == -1                   # s1 and s2 come together
    assert _raw(a, q, n_draws=False) == -1                                              # sums need the count
    assert _raw(a, q, s1=False, s2=False, hits=True, n_obs=2, ob=ob, n_draws=False) == -1
    assert _raw(a, q, s1=False, s2=False, length=True, n_draws=False) == 0              # per-draw outputs alone do not
    assert _raw(a, q) == 0
    want = ("query_poses", "delta", "poses", "vels", "landmarks")
    same_bits(a.sample_posterior_at(*q, 2, seed=SEED, first=FIRST, want=want), b.sample_posterior_at(*q, 2, seed=SEED, first=FIRST, want=want))


def test_what_the_bridge_refuses_and_rot3_positions():
    p = DM.graph("se2", True)            # GP priors with a Qc of their own: the family's se2 graph as it is
    q = queries(graph("se2", True), "runs")
    check_untouched(device(p), device(p), p, lambda s: s.sample_posterior_stats(*q, 2), r"\(-5\).*sample_posterior_stats.*Qc of their own")
    p = DM.graph("se3_vw", False)
    q = queries(p, "runs")
    check_untouched(device(p), device(p), p, lambda s: s.sample_posterior_stats(*q, 2), r"\(-5\).*sample_posterior_stats.*world-frame")
    _, dev = ahrs_pair()
    before = dev.get_states()
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*ROT3_BIAS"):
        dev.sample_posterior_stats([0], [0.1], [0.05], 1, want=("moments",))
    same_bits(before, dev.get_states())
    # a rotation has no position
    p = graph("so3", False)
    q = queries(p, "runs")
    for want, ob in ((("length",), None), (("moments", "length"), None), (("hits",), np.array([[0.0, 0.0, 1.0]])), (("clearance",), np.array([[0.0, 0.0, 1.0]]))):
        a, b = device(p), device(p)
        check_untouched(a, b, p, lambda s: s.sample_posterior_stats(*q, 2, obstacles=ob, want=want), r"\(-5\).*GPSLAM_ROT3")
        same_bits(a.sample_posterior_at(*q, 2, seed=SEED), b.sample_posterior_at(*q, 2, seed=SEED))
    assert device(p).sample_posterior_stats(*q, 2)["length"] is None


@pytest.mark.parametrize("what,kw,extra,message,lm", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_what_sample_posterior_refuses_is_refused(what, kw, extra, message, lm):
    p = DM.graph("se2", lm, 60 if what == "segmented" else None)      # (segments need a chain to cut)
    q = queries(p, "runs")
    check_untouched(device(p, extra, **kw), device(p, extra, **kw), p, lambda s: s.sample_posterior_stats(*q, 2), r"\(-5\).*sample_posterior_stats.*" + message)


def test_uncompiled_handle():
    import fixed_lag_mix_model as FM
    p = graph("se2", True)
    raw = FM.chain(p, gp.ChainSolver)
    raw.set_qc(p["qc"])
    raw.set_states(p["pose"], p["vel"])
    with pytest.raises(gp.GpslamHipError, match=r"\(-4\)"):
        raw.sample_posterior_stats(*queries(p, "runs"), 1)
