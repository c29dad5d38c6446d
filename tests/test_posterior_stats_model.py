"""tests/posterior_stats_model.py on the CPU: the sums against direct numpy on the model's own draws, the packing, the continuation,
clearance and length by hand on a small path, and the obstacle set of every case the GPU tests use -- both outcomes occur and no
clearance sits within 1e-6 of zero, so tests/test_gpu_sampling_stats.py can compare counts exactly."""
import numpy as np
import pytest

from oracle import oracle as O
import posterior_stats_model as SM


@pytest.fixture(scope="module")
def drawn():
    """per case: description, queries, reference poses, the model's draws (computed once, never written to)"""
    cache = {}

    def get(*key):
        if key not in cache:
            p, q = SM.case(*key)
            cache[key] = (p, q, SM.reference_poses(p, *q), SM.model_draws(p, *q))
        return cache[key]
    return get


@pytest.mark.parametrize("name,lm,N,which", SM.CASES, ids=SM.CASE_IDS)
def test_obstacle_sets_give_both_outcomes_and_keep_off_the_boundary(drawn, name, lm, N, which):
    p, q, qhat, qp = drawn(name, lm, N, which)
    kind = p["kind"]
    if kind == O.ROT3:
        st = SM.stats(kind, p["chart"], qhat, qp)
        assert "g" not in st and "length" not in st and st["s1"].shape == (len(q[0]), 3)
        return
    ob = SM.obstacles(p, *q)
    assert ob.shape == (1 if len(q[0]) == 1 else 2, 4 if kind == O.POSE3 else 3) and (ob[:, -1] >= 0.0).all()
    st = SM.stats(kind, p["chart"], qhat, qp, ob)
    count, n = qp.shape[:2]
    print("%s: %d queries, %d draws: hits %d of %d, min |g| %.3g, clearance %s" % (name, n, count, st["hits"].sum(), count * n, np.abs(st["g"]).min(), st["clearance"]))
    assert 0 < st["hits"].sum() < count * n
    assert np.abs(st["g"]).min() >= 1e-6
    assert (st["length"] == 0.0).all() if n == 1 else (st["length"] > 0.0).all()


@pytest.mark.parametrize("name,lm,N,which", [c for c in SM.CASES if c[3] != "dense"], ids=[i for i in SM.CASE_IDS if not i.endswith("dense")])
def test_sums_are_numpys(drawn, name, lm, N, which):
    p, q, qhat, qp = drawn(name, lm, N, which)
    kind, d = p["kind"], O.TANGENT_DIM[p["kind"]]
    st = SM.stats(kind, p["chart"], qhat, qp)
    e = st["eta"]
    assert e.shape == (qp.shape[0], len(q[0]), d) and st["n"] == qp.shape[0]
    # the tangent: q - q^ on the vector spaces, and zero at the reference itself everywhere
    if kind in (O.LINEAR2, O.LINEAR3):
        assert np.array_equal(e, qp - qhat[None])
    # (a few roundings of x^-1 x at coordinates of the size of the poses)
    assert np.abs(SM.eta(kind, qhat, qhat[None], p["chart"])).max() <= 4.0 * np.finfo(np.float64).eps * max(1.0, np.abs(qhat).max())
    assert np.abs(st["s1"] - e.sum(axis=0)).max() <= 1e-15 * qp.shape[0] * max(1.0, np.abs(e).max())
    full = np.einsum("kqr,kqc->qrc", e, e)
    for i in range(len(q[0])):
        assert np.abs(SM.unpack(st["s2"][i], d) - full[i]).max() <= 1e-15 * qp.shape[0] * max(1.0, np.abs(e).max() ** 2)
    # continued: 1 + 2 draws carry the bits of 3
    a = SM.stats(kind, p["chart"], qhat, qp[:1])
    b = SM.stats(kind, p["chart"], qhat, qp[1:], start=a)
    assert b["n"] == 3 and np.array_equal(b["s1"], st["s1"]) and np.array_equal(b["s2"], st["s2"])
    mean, cov = SM.moments(st["n"], st["s1"], st["s2"])
    want = np.array([np.cov(e[:, i, :].T) for i in range(len(q[0]))]).reshape(cov.shape)
    assert np.abs(mean - e.mean(axis=0)).max() <= 1e-15
    assert np.abs(cov - want).max() <= 1e-13 * max(1.0, np.abs(want).max())


def test_the_packing():
    M = np.arange(36.0).reshape(6, 6)
    M = M + M.T
    s = SM.pack(M)
    assert len(s) == 21 and np.array_equal(SM.unpack(s, 6), M)
    for r in range(6):
        for c in range(r + 1):
            assert s[r * (r + 1) // 2 + c] == M[r, c]


def test_clearance_hits_and_length_by_hand():
    # three draws of a three-query path in the plane; one obstacle of radius 1 at (2, 0), one of radius 0 at (0, 5)
    qp = np.array([[[0.0, 0.0], [3.0, 4.0], [3.0, 0.0]],
                   [[0.5, 0.0], [1.5, 0.0], [9.0, 0.0]],
                   [[0.0, 5.5], [0.0, 6.0], [0.0, 7.0]]])
    ob = np.array([[2.0, 0.0, 1.0], [0.0, 5.0, 0.0]])
    st = SM.stats(O.LINEAR2, O.CHART_EXPMAP, np.zeros((3, 2)), qp, ob, margin=0.25)
    g = np.array([[1.0, np.sqrt(17.0) - 1.0, 0.0], [0.5, -0.5, 6.0], [0.5, 1.0, 2.0]]) - 0.25
    assert np.abs(st["g"] - g).max() <= 1e-15
    assert np.array_equal(st["hits"], [0, 1, 1]) and np.abs(st["clearance"] - [-0.25, -0.75, 0.25]).max() <= 1e-15
    assert np.abs(st["length"] - [9.0, 8.5, 1.5]).max() <= 1e-15
    # the margin moves every clearance by exactly itself; a continued count adds
    assert np.array_equal(SM.stats(O.LINEAR2, O.CHART_EXPMAP, np.zeros((3, 2)), qp, ob)["clearance"] - 0.25, st["clearance"])
    assert np.array_equal(SM.stats(O.LINEAR2, O.CHART_EXPMAP, np.zeros((3, 2)), qp, ob, margin=0.25, start=st)["hits"], [0, 2, 2])
    # the translation of SE(3) is what counts there
    pose = np.zeros((1, 2, 12))
    pose[0, :, 9:] = [[1.0, 2.0, 2.0], [1.0, 2.0, 5.0]]
    st = SM.stats(O.POSE3, O.CHART_EXPMAP, np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]), (2, 1)),
                  pose + np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]), np.array([[0.0, 0.0, 0.0, 1.0]]))
    assert np.abs(st["clearance"] - 2.0).max() <= 1e-15 and np.abs(st["length"] - 3.0).max() <= 1e-15
