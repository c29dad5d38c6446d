"""The host arithmetic of Powell's dogleg (include/gpslam_hip_dogleg.h) on the CPU: gpslam_hip_dogleg_point and
gpslam_hip_dogleg_decide against the numpy model of tests/dogleg_model.py and against numbers written out here, and the binding's
bookkeeping (the new symbols exist in the library, the new header and the binding's own list; gpslam_hip.h and ABI 2.4 are untouched)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import chain
import dogleg_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spd_system(rng, n=8):
    """a small SPD system (condition number of order 10), its g, and the four scalars in np.longdouble"""
    A = rng.standard_normal((n, n))
    H = A.T @ A / n + np.eye(n)
    g = rng.standard_normal(n)
    L = np.longdouble
    Hl, gl = H.astype(L), g.astype(L)
    dn = np.linalg.solve(H, g).astype(L)
    for _ in range(3):      # (refined in longdouble: H dn = g to its precision)
        dn = dn + np.linalg.solve(H, (gl - Hl @ dn).astype(np.float64)).astype(L)
    return Hl, gl, dn, (gl @ gl, gl @ (Hl @ gl), gl @ dn, dn @ dn)


def radii(s4):
    gg, gHg, gn, nn = [float(v) for v in s4]
    s = gg / gHg
    return float(np.sqrt(s * s * gg)), float(np.sqrt(nn))


def test_point_on_drawn_systems_every_branch():
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(200):
        Hl, gl, dn, s4l = spd_system(rng)
        s4 = [float(v) for v in s4l]
        nu, nn = radii(s4)
        assert nu < nn
        for delta in (nu * rng.uniform(0.05, 0.99), nu + (nn - nu) * rng.uniform(0.01, 0.99), nn * rng.uniform(1.01, 5.0)):
            a, b, norm, pred, branch = gp.dogleg_point(s4, delta)
            ma, mb, mnorm, mpred, mbranch = DM.point(s4, delta)
            assert branch == mbranch
            seen.add(branch)
            assert abs(a - ma) <= 1e-12 * max(abs(ma), abs(mb)) and abs(b - mb) <= 1e-12 * max(abs(ma), abs(mb), 1e-300), (a, ma, b, mb)
            dd = np.longdouble(a) * gl + np.longdouble(b) * dn
            if branch < 2:
                assert abs(norm - delta) <= 1e-14 * delta                              # the reported norm
                assert abs(float(np.sqrt(dd @ dd)) - delta) <= 1e-14 * delta          # and the vector's own
            else:
                assert (a, b) == (0.0, 1.0)
            dense = gl @ dd - (dd @ (Hl @ dd)) / 2                                      # M(0) - M(dd), dense, in longdouble
            assert abs(pred - float(dense)) <= 1e-12 * abs(float(dense)), (pred, float(dense))
            assert abs(pred - mpred) <= 1e-12 * abs(mpred)
    assert seen == {0, 1, 2}


def test_point_at_the_branch_boundaries():
    rng = np.random.default_rng(12)
    for _ in range(50):
        s4 = [float(v) for v in spd_system(rng)[3]]
        nu, nn = radii(s4)
        a, b, norm, pred, branch = gp.dogleg_point(s4, nu)          # Delta = |du|: not below it -> the blend, at tau = 0
        assert branch == 1 == DM.point(s4, nu)[4]
        assert abs(a - s4[0] / s4[1]) <= 1e-7 * a and abs(b) <= 1e-7, (a, b)
        assert abs(norm - nu) <= 1e-14 * nu
        a, b, norm, pred, branch = gp.dogleg_point(s4, np.nextafter(nu, 0.0))
        assert branch == 0 and b == 0.0
        a, b, norm, pred, branch = gp.dogleg_point(s4, nn)          # Delta = |dn|: the Gauss-Newton step
        assert (a, b, branch) == (0.0, 1.0, 2) and DM.point(s4, nn)[4] == 2
        assert pred == s4[2] - 0.5 * s4[2]
        assert gp.dogleg_point(s4, np.nextafter(nn, 0.0))[4] == 1


@pytest.mark.parametrize("s4", [(0.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (2.0, 0.0, 1.0, 4.0), (2.0, -3.0, 1.0, 4.0), (2.0, -3.0, 1.0, 0.0)])
def test_point_degenerate(s4):
    """gg == 0 or gHg <= 0: the Gauss-Newton step clipped to Delta, nothing at all when nn == 0"""
    for delta in (0.5, 2.0, 10.0):
        a, b, norm, pred, branch = gp.dogleg_point(s4, delta)
        want = min(1.0, delta / np.sqrt(s4[3])) if s4[3] > 0 else 0.0
        assert (a, b, branch) == (0.0, want, 2)
        assert DM.point(s4, delta)[:2] == (0.0, want)
        assert norm == want * np.sqrt(s4[3])
        assert pred == want * s4[2] - 0.5 * want * want * s4[2]


def test_point_refuses_bad_arguments():
    for delta in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(gp.GpslamHipError):
            gp.dogleg_point((1.0, 1.0, 1.0, 1.0), delta)
    with pytest.raises(gp.GpslamHipError):
        gp.dogleg_decide((1.0, 0.5, 0.5, 1.0), 3, 1.0)


# ---------------------------------------------------------------- the rule table
def _s4(rho, norm, f=10.0, pred=2.0):
    return (f, f - rho * pred, pred, norm)


RULES = [
    # (rho, norm, delta, last_action, mode) -> (keep, stay, delta, last_action)
    # rho >= 0.75: Delta <- max(Delta, 3 |dd|)
    ((0.9, 1.0, 1.0, 0, 0), (True, False, 3.0, 0)), ((0.9, 1.0, 1.0, 0, 2), (True, False, 3.0, 0)),
    ((0.9, 1.0, 1.0, 0, 1), (True, True, 3.0, 1)),                      # searching: increased, try again
    ((0.9, 0.2, 1.0, 0, 1), (True, False, 1.0, 0)),                     # ... the step is inside the region: Delta stays, done
    ((0.9, 1.0, 1.0, 2, 1), (True, False, 3.0, 2)),                     # ... after a decrease: done
    ((0.75, 1.0, 1.0, 1, 1), (True, True, 3.0, 1)),
    # 0.25 <= rho < 0.75
    ((0.5, 1.0, 1.0, 0, 0), (True, False, 1.0, 0)), ((0.5, 1.0, 1.0, 1, 1), (True, False, 1.0, 1)), ((0.25, 1.0, 1.0, 2, 2), (True, False, 1.0, 2)),
    # 0 <= rho < 0.25: Delta <- Delta / 2 while above the floor
    ((0.1, 1.0, 1.0, 0, 0), (True, False, 0.5, 0)),
    ((0.1, 1.0, 1.0, 0, 1), (True, True, 0.5, 2)), ((0.1, 1.0, 1.0, 0, 2), (True, True, 0.5, 2)),
    ((0.1, 1.0, 1.0, 1, 1), (True, False, 0.5, 1)),                     # after an increase: done
    ((0.01, 1.0, 1.0, 2, 2), (True, True, 0.5, 2)),
    ((0.0, 1.0, 1.0, 2, 2), (True, False, 1.0, 2)),                     # f_new == f: rho counts as 0.5
    ((0.1, 1.0, 1e-5, 0, 1), (True, False, 1e-5, 0)), ((0.1, 1.0, 1e-5, 0, 0), (True, False, 1e-5, 0)),      # the floor: Delta stays, done
    ((0.1, 1.0, 2e-5, 0, 2), (True, True, 1e-5, 2)),
    # rho < 0: every mode tries again with half the radius, down to the floor
    ((-0.1, 1.0, 1.0, 0, 0), (False, True, 0.5, 2)), ((-0.1, 1.0, 1.0, 1, 1), (False, True, 0.5, 2)), ((-5.0, 1.0, 1.0, 0, 2), (False, True, 0.5, 2)),
    ((-0.1, 1.0, 2e-5, 0, 0), (False, True, 1e-5, 2)),
    ((-0.1, 1.0, 1e-5, 2, 0), (False, False, 1e-5, 2)), ((-0.1, 1.0, 5e-6, 2, 1), (False, False, 5e-6, 2)), ((-0.1, 1.0, 1e-5, 0, 2), (False, False, 1e-5, 0)),
]


@pytest.mark.parametrize("args,want", RULES)
def test_decide_rule_table(args, want):
    rho, norm, delta, last, mode = args
    assert gp.dogleg_decide(_s4(rho, norm), mode, delta, last) == want
    assert DM.decide(*_s4(rho, norm)[:3], norm, mode, delta, last) == want


def test_decide_against_the_model_on_a_grid():
    fs = [(10.0, 1.0), (10.0, 9.9), (10.0, 10.0), (10.0, 10.0 + 1e-16), (10.0, 12.0), (10.0, float("inf")), (10.0, float("nan")), (10.0, 8.5), (10.0, 5.0)]
    preds = [10.0, 2.0, 0.0, 1e-16, -1.0, float("nan")]
    n = 0
    for (f, f_new), pred, norm, delta, last, mode in itertools.product(fs, preds, (0.2, 1.0), (1.0, 2e-5, 1e-5, 5e-6), (0, 1, 2), (0, 1, 2)):
        got = gp.dogleg_decide((f, f_new, pred, norm), mode, delta, last)
        assert got == DM.decide(f, f_new, pred, norm, mode, delta, last), (f, f_new, pred, norm, delta, last, mode, got)
        n += 1
    assert n == 9 * 6 * 2 * 4 * 3 * 3


def test_decide_on_a_cost_that_is_not_finite():
    for f_new in (float("inf"), float("nan")):
        assert gp.dogleg_decide((10.0, f_new, 2.0, 1.0), 0, 1.0) == (False, True, 0.5, 2)
        assert gp.dogleg_decide((10.0, f_new, 2.0, 1.0), 1, 1e-5, 1) == (False, False, 1e-5, 1)


# ---------------------------------------------------------------- bookkeeping
def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        return sorted(set(re.findall(r"\b(gpslam_hip_[a-z0-9_]+)\s*\(", f.read())))


def test_symbols_exist_in_the_library_the_header_and_the_binding():
    lib = gp.load_library()
    assert _declared("gpslam_hip_dogleg.h") == sorted(chain.DOGLEG_SYMBOLS)
    assert len(chain.DOGLEG_SYMBOLS) == 5
    for name in chain.DOGLEG_SYMBOLS:
        assert hasattr(lib, name), name
        assert name not in chain.ABI_SYMBOLS
    for name in ("iterate_dogleg", "optimize_dogleg", "dogleg_last"):
        assert callable(getattr(gp.ChainSolver, name))


def test_abi_and_the_old_header_are_untouched():
    lib = gp.load_library()
    lib.gpslam_hip_abi_version.restype = C.c_uint32
    v = lib.gpslam_hip_abi_version()
    assert (v >> 16, v & 0xffff) == (2, 4)
    assert _declared("gpslam_hip.h") == sorted(chain.ABI_SYMBOLS)
    with open(os.path.join(ROOT, "include", "gpslam_hip.h")) as f:
        assert "dogleg" not in f.read().lower()


def test_null_handle():
    lib = chain._dogleg_lib()
    d, st, out = C.c_double(1.0), chain.Stats(), (C.c_double * 8)()
    p = chain.Params()
    lib.gpslam_hip_default_params(C.byref(p))
    assert lib.gpslam_hip_iterate_dogleg(None, C.byref(d), 0, C.byref(st)) == -1
    assert lib.gpslam_hip_optimize_dogleg(None, C.byref(p), 1.0, 0, C.byref(st)) == -1
    assert lib.gpslam_hip_dogleg_last(None, out) == -1
