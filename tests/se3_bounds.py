"""Rounding bounds for a float64 evaluation of the reference's SE(3) GP formulas (numpy only).

The reference's formulas are restated once below, generic in the number type, so that the same text evaluates
  * in float64 (plain Python floats),
  * in 50-digit arithmetic (tests/golden/make_se3_jac_pins.py sets `M` to mpmath: the pins' H_ref),
  * in running-bound arithmetic (`R` below): Higham's running bound.  Every operand is replaced by its absolute value
    and every subtraction by an addition (1 - th^2/2 - cos th  ->  1 + th^2/2 + |cos th|); a quotient or a function
    carries its operands' bounds through its derivative (|f'(y)| a_y + |f(y)|).  The error of a float64 evaluation
    of any entry is then at most GAMMA * a, with GAMMA = K * u and one K for every entry and every case.
Every operation adds its own |result| to the bound (Higham's running error bound, "Accuracy and Stability of Numerical
Algorithms", section 3.3), so the length of a dependence chain is counted by the arithmetic itself and K does not
grow with it.  K covers what the arithmetic does not see, fixed from these figures and not from any case: up to 4 ulp
for each of libm's sin / cos / acos / tan (host and device libraries together), where the arithmetic charges 1, and the
evaluation orders of the oracle (6x6 matrices) and the kernel (nested cross products), whose running bounds differ by
less than a factor of 2 (second-order terms are far below either): K = 4 x 2 = 8.

The finite-difference entries come out of the same arithmetic: (f(xi + h) - f(xi - h)) / 2h carries
2 GAMMA f_abs / 2h, and the right-hand factor of the Jacobian product carries it on with absolute values.

Reference file:line: Pose3utils.cpp:92-113 (rightJacobianPose3Q), :167-179 (jacobianMethodNumercialDiff),
:192-224 (rightJacobianPose3inv, rightJacobianRot3inv), GaussianProcessPriorPose3.h:60-98,
GaussianProcessInterpolatorPose3.h:57-105; GTSAM's Pose3 / Rot3 inverse, compose, Logmap, Expmap as the oracle
restates them (oracle/orc_lie.c).
"""
import math

import numpy as np

U = 2.0 ** -53
K = 8
GAMMA = K * U
H_FD = 1e-6                # jacobianMethodNumercialDiff's step (Pose3utils.h:57)
EPS = 2.220446049250313e-16


class R:
    """A float64 value x together with its running bound a (the expression evaluated in absolute values)."""
    __slots__ = ("x", "a")

    def __init__(self, x, a=0.0):
        self.x = float(x)
        self.a = float(a)

    @staticmethod
    def of(v):
        return v if isinstance(v, R) else R(v)

    def __add__(self, o):
        o = R.of(o)
        x = self.x + o.x
        return R(x, self.a + o.a + abs(x))
    __radd__ = __add__

    def __sub__(self, o):
        o = R.of(o)
        x = self.x - o.x
        return R(x, self.a + o.a + abs(x))

    def __rsub__(self, o):
        return R.of(o) - self

    def __mul__(self, o):
        o = R.of(o)
        x = self.x * o.x
        return R(x, abs(self.x) * o.a + self.a * abs(o.x) + abs(x))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = R.of(o)
        x = self.x / o.x
        return R(x, (self.a + abs(x) * o.a) / abs(o.x) + abs(x))

    def __rtruediv__(self, o):
        return R.of(o) / self

    def __neg__(self):
        return R(-self.x, self.a)

    def __abs__(self):
        return R(abs(self.x), self.a)

    def __float__(self):
        return self.x

    def __gt__(self, o):
        return self.x > float(o)

    def __lt__(self, o):
        return self.x < float(o)

    def __le__(self, o):
        return self.x <= float(o)

    def __ge__(self, o):
        return self.x >= float(o)


class _RMath:
    """the functions the formulas call, in running-bound arithmetic"""
    @staticmethod
    def sin(y):
        return R(math.sin(y.x), abs(math.cos(y.x)) * y.a + abs(math.sin(y.x)))

    @staticmethod
    def cos(y):
        return R(math.cos(y.x), abs(math.sin(y.x)) * y.a + abs(math.cos(y.x)))

    @staticmethod
    def tan(y):
        t = math.tan(y.x)
        return R(t, (1 + t * t) * y.a + abs(t))

    @staticmethod
    def sqrt(y):
        s = math.sqrt(y.x)
        return R(s, (y.a / (2 * s) if s > 0 else 0.0) + s)

    @staticmethod
    def acos(y):
        return R(math.acos(y.x), y.a / math.sqrt(max(1 - y.x * y.x, 1e-300)) + abs(math.acos(y.x)))


M = math   # the function namespace of the current arithmetic: math (float64), mpmath (pins), _RMath (bounds)


def _ns(x):
    return _RMath if isinstance(x, R) else M


def sin(x): return _ns(x).sin(x)
def cos(x): return _ns(x).cos(x)
def tan(x): return _ns(x).tan(x)
def sqrt(x): return _ns(x).sqrt(x)
def acos(x): return _ns(x).acos(x)
def val(x): return x.x if isinstance(x, R) else x


def scalar(fn, dfn, y):
    """fn(y) for a scalar coefficient the formulas evaluate in several correlated steps (1 - th^2/2 - cos th over th^4, ...):
    in running-bound arithmetic its own rounding (fn's steps with y exact) plus |fn'(y)| times y's bound, so that an error
    of y is not counted once per occurrence of y"""
    if not isinstance(y, R):
        return fn(y)
    loc = fn(R(y.x, 0.0))
    if not isinstance(loc, R):
        return R(loc, 0.0)
    return R(loc.x, loc.a + abs(dfn(y.x)) * y.a)


def _dnum(fn, y, h):
    return (float(fn(y + h)) - float(fn(y - h))) / (2 * h)


# ------------------------------------------------------------------ 3x3 / 6x6 helpers on nested lists
def zeros(n, m):
    return [[0.0] * m for _ in range(n)]


def eye(n):
    return [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]


def mm(A, B):
    n, k, m = len(A), len(B), len(B[0])
    return [[sum((A[i][l] * B[l][j] for l in range(1, k)), A[i][0] * B[0][j]) for j in range(m)] for i in range(n)]


def mv(A, x):
    return [sum((A[i][l] * x[l] for l in range(1, len(x))), A[i][0] * x[0]) for i in range(len(A))]


def madd(*Ms):
    out = [row[:] for row in Ms[0]]
    for Mx in Ms[1:]:
        out = [[a + b for a, b in zip(r, s)] for r, s in zip(out, Mx)]
    return out


def msc(c, A):
    return [[c * a for a in r] for r in A]


def tr(A):
    return [list(r) for r in zip(*A)]


def skew(w):
    return [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]


def block6(A, B, C, D):
    """[[A, B], [C, D]] of 3x3 blocks (B = None: zeros)"""
    B = B or zeros(3, 3)
    return [A[i] + B[i] for i in range(3)] + [C[i] + D[i] for i in range(3)]


def rot(T):
    return [T[0:3], T[3:6], T[6:9]]


def pose(Rm, t):
    return [v for r in Rm for v in r] + list(t)


# ------------------------------------------------------------------ GTSAM Rot3 / Pose3 (oracle/orc_lie.c)
def rot3_logmap(Rm):
    trc = Rm[0][0] + Rm[1][1] + Rm[2][2]
    assert abs(val(trc) + 1.0) >= 1e-10, "near-pi branch not restated"
    mag = scalar(_log_mag, _log_mag_d, trc)
    return [mag * (Rm[2][1] - Rm[1][2]), mag * (Rm[0][2] - Rm[2][0]), mag * (Rm[1][0] - Rm[0][1])]


def _log_mag(trc):
    tr_3 = trc - 3.0
    if val(tr_3) < -1e-7:
        th = acos((trc - 1.0) / 2.0)
        return th / (2.0 * sin(th))
    return 0.5 - tr_3 * tr_3 / 12.0


def _log_mag_d(trc):
    """d/dtr of th / (2 sin th), th = acos((tr - 1) / 2): -(sin th - th cos th) / (4 sin^3 th), -> -1/12 at 0"""
    if trc - 3.0 >= -1e-7:
        return -(trc - 3.0) / 6.0
    th = math.acos((trc - 1.0) / 2.0)
    if th < 0.1:
        return -(1.0 / 12.0) * (1.0 + th * th)
    return -(math.sin(th) - th * math.cos(th)) / (4.0 * math.sin(th) ** 3)


def _log_c(th):
    return 1.0 - th / (2.0 * tan(0.5 * th))


def _log_c_d(th):
    return th / 6.0 + th ** 3 / 90.0 if th < 0.5 else _dnum(_log_c, th, 1e-6)


def pose3_logmap(T):
    w = rot3_logmap(rot(T))
    t = T[9:12]
    th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if val(th) < 1e-10:
        return w + list(t)
    W = skew([w[0] / th, w[1] / th, w[2] / th])
    WT = mv(W, t)
    WWT = mv(W, WT)
    c = scalar(_log_c, _log_c_d, th)
    return w + [t[i] - (0.5 * th) * WT[i] + c * WWT[i] for i in range(3)]


def rot3_expmap(w):
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    W = skew(w)
    if val(th2) > EPS:
        th = sqrt(th2)
        Kx = msc(1.0 / th, W)
        s = sin(th)
        omc = 2.0 * sin(th / 2.0) * sin(th / 2.0)
        return madd(eye(3), msc(s, Kx), msc(omc, mm(Kx, Kx)))
    return madd(eye(3), W)


def pose3_expmap(xi):
    w, v = xi[:3], xi[3:]
    Rm = rot3_expmap(w)
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if val(th2) > EPS:
        wv = w[0] * v[0] + w[1] * v[1] + w[2] * v[2]
        wxv = mv(skew(w), v)
        Rwxv = mv(Rm, wxv)
        t = [(wxv[i] - Rwxv[i] + w[i] * wv) / th2 for i in range(3)]
    else:
        t = list(v)
    return pose(Rm, t)


def rot3_jr(w):
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if val(th2) <= EPS:
        return eye(3)
    th = sqrt(th2)
    Y = msc(1.0 / th, skew(w))
    return madd(eye(3), msc(-((1.0 - cos(th)) / th), Y), msc(1.0 - sin(th) / th, mm(Y, Y)))


def rot3_jrinv(w):
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if val(th2) <= EPS:
        return eye(3)
    th = sqrt(th2)
    X = skew(w)
    c = scalar(_jrinv_c, _jrinv_c_d, th)
    return madd(eye(3), msc(0.5, X), msc(c, mm(X, X)))


def _jrinv_c(th):
    return 1.0 / (th * th) - (1.0 + cos(th)) / (2.0 * th * sin(th))


def _jrinv_c_d(th):
    return th / 360.0 + th ** 3 / 7560.0 if th < 0.5 else _dnum(_jrinv_c, th, 1e-6)


def q_coefs(th, branch=1e-5):
    """rightJacobianPose3Q's coefficients with its |th| > 1e-5 branch (Pose3utils.cpp:98-112)"""
    if isinstance(th, R):
        return tuple(scalar(lambda t, i=i: _q_coefs(t, branch)[i], lambda t, i=i: _q_coefs_d(t, branch)[i], th) for i in range(3))
    return _q_coefs(th, branch)


def _q_coefs_d(th, branch):
    if th <= branch:
        return 0.0, 0.0, 0.0
    if th < 0.5:      # the Taylor series in th^2 of (th - sin th)/th^3, (1 - th^2/2 - cos th)/th^4, the third coefficient
        # qa = 1/6 - u/120 + u^2/5040, qb = -1/24 + u/720 - u^2/40320, qd = -1/120 + u/5040 - u^2/362880, qc = -(qb - 3 qd)/2
        dqb = th / 360.0 - th ** 3 / 10080.0
        dqd = th / 2520.0 - th ** 3 / 90720.0
        return -th / 60.0 + th ** 3 / 1260.0, dqb, -0.5 * (dqb - 3.0 * dqd)
    return tuple(_dnum(lambda t, i=i: _q_coefs(t, branch)[i], th, 1e-6) for i in range(3))


COEF64 = False   # see float64_coefficients()


class float64_coefficients:
    """Within this context the three closed-form coefficients of rightJacobianPose3Q are taken as a float64 evaluation
    with correctly rounded sin / cos forms them, and treated as exact inputs; everything else keeps its arithmetic.
    Near th = 1e-5 those coefficients are all rounding -- (1 - th^2/2 - cos th) is below one ulp of 1, so its float64
    value is a whole number of ulps (almost always 0) where the exact one is th^4/24 -- and their error is as large as the
    jump of the reference's branch at 1e-5.  Pinned this way (H_ref64 in tests/golden/se3_jac_pins.json), the pins
    keep that rounding and the remaining bound is small enough to see which side of 1e-5 a kernel takes."""

    def __enter__(self):
        global COEF64
        self.old, COEF64 = COEF64, True

    def __exit__(self, *exc):
        global COEF64
        COEF64 = self.old


def _q_coefs64(th):
    t = float(val(th))
    s, co = math.sin(t), math.cos(t)
    t2 = t * t
    t3 = t2 * t
    t4 = t3 * t
    t5 = t4 * t
    a = (t - s) / t3
    b = (1.0 - 0.5 * t2 - co) / t4
    c = -0.5 * ((1.0 - 0.5 * t2 - co) / t4 - 3.0 * (t - s - t3 / 6.0) / t5)
    if isinstance(th, (float, R)):
        return a, b, c
    return tuple(th * 0 + v for v in (a, b, c))       # exact in the caller's number type


def _q_coefs(th, branch):
    if COEF64 and val(th) > branch:
        return _q_coefs64(th)
    if val(th) > branch:
        s, co = sin(th), cos(th)
        t2 = th * th
        t3 = t2 * th
        t4 = t3 * th
        t5 = t4 * th
        a = (th - s) / t3
        b = (1.0 - 0.5 * t2 - co) / t4
        c = -0.5 * ((1.0 - 0.5 * t2 - co) / t4 - 3.0 * (th - s - t3 / 6.0) / t5)
        return a, b, c
    return 1.0 / 6.0, 1.0 / 24.0, -0.5 * (1.0 / 24.0 + 3.0 / 120.0)


def pose3_Q(xi):
    w, rho = xi[:3], xi[3:]
    th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    X, Y = skew(w), skew(rho)
    XY, YX = mm(X, Y), mm(Y, X)
    XYX = mm(X, YX)
    a, b, c = q_coefs(th)
    t1 = madd(XY, YX, msc(-1.0, XYX))
    t2 = madd(mm(X, XY), mm(YX, X), msc(-3.0, XYX))
    t3 = madd(mm(XYX, X), mm(X, XYX))
    return madd(msc(-0.5, Y), msc(a, t1), msc(b, t2), msc(c, t3))


def pose3_jrinv(xi):
    Jw = rot3_jrinv(xi[:3])
    Q2 = msc(-1.0, mm(mm(Jw, pose3_Q(xi)), Jw))
    return block6(Jw, None, Q2, Jw)


def pose3_jr(xi):
    Jw = rot3_jr(xi[:3])
    return block6(Jw, None, pose3_Q(xi), Jw)


def adjoint(T):
    Rm = rot(T)
    return block6(Rm, None, mm(skew(T[9:12]), Rm), Rm)


def inverse(T):
    Rt = tr(rot(T))
    t = T[9:12]
    return pose(Rt, [-(Rt[i][0] * t[0] + Rt[i][1] * t[1] + Rt[i][2] * t[2]) for i in range(3)])


def compose(A, B):
    RA = rot(A)
    return pose(mm(RA, rot(B)), [A[9 + i] + RA[i][0] * B[9] + RA[i][1] * B[10] + RA[i][2] * B[11] for i in range(3)])


def fd_jrinv_x(xi, x, h=H_FD, closed=False):
    """jacobianMethodNumercialDiff(rightJacobianPose3inv, xi, x, h) (Pose3utils.cpp:167-179).  closed=True: the
    translational columns as the fp64 kernel forms them, -Jw Q(w, e_k) Jw x_w (factors.hpp, se3_jrinv_times_x_fd_k) --
    equal to the quotient in exact arithmetic, since Jr^-1(xi) x is affine in rho.
    In running-bound arithmetic an error of xi is common to both ends of the quotient: it enters once, through the
    derivative of the quotient itself (a float64 central difference of it at step 1e-3), not once per end over 2h."""
    if any(isinstance(v, R) and v.a > 0 for v in xi):
        D = fd_jrinv_x([R(val(v)) for v in xi], x, h, closed)
        xf, xv = [val(v) for v in xi], [val(v) for v in x]
        for j in range(6):
            p, n = list(xf), list(xf)
            p[j] += 1e-3
            n[j] -= 1e-3
            Dp, Dn = fd_jrinv_x(p, xv, h, True), fd_jrinv_x(n, xv, h, True)
            for i in range(6):
                for k in range(6):
                    d0 = R.of(D[i][k])
                    D[i][k] = R(d0.x, d0.a + abs(Dp[i][k] - Dn[i][k]) / 2e-3 * xi[j].a)
        return D
    D = zeros(6, 6)
    for k in range(6):
        if closed and k >= 3:
            Jw = rot3_jrinv(xi[:3])
            top = mv(Jw, x[:3])
            e = [1.0 if i == k - 3 else 0.0 for i in range(3)]
            col = [0.0] * 3 + [-c for c in mv(Jw, mv(pose3_Q(list(xi[:3]) + e), top))]
        else:
            xp, xn = list(xi), list(xi)
            xp[k] = xp[k] + h
            xn[k] = xn[k] - h
            fp, fn = mv(pose3_jrinv(xp), x), mv(pose3_jrinv(xn), x)
            col = [(fp[i] - fn[i]) * (1.0 / (2.0 * h)) for i in range(6)]
        for i in range(6):
            D[i][k] = col[i]
    return D


def gp_prior(p1, v1, p2, v2, dt, closed=False):
    """GaussianProcessPriorPose3::evaluateError (GaussianProcessPriorPose3.h:60-98): (e[12], [H1..H4] 12x6)"""
    inv = inverse(p1)
    Hinv = msc(-1.0, adjoint(p1))
    Hc1 = adjoint(inverse(p2))
    r = pose3_logmap(compose(inv, p2))
    Hlog = pose3_jrinv(r)
    Jinv = pose3_jrinv(r)
    FD = fd_jrinv_x(r, v2, closed=closed)
    J_Ti = mm(mm(Hlog, Hc1), Hinv)
    J_Ti1 = Hlog
    H1 = J_Ti + mm(FD, J_Ti)
    H3 = J_Ti1 + mm(FD, J_Ti1)
    H2 = [[(-dt if i == j else 0.0) for j in range(6)] for i in range(6)] + [[(-1.0 if i == j else 0.0) for j in range(6)] for i in range(6)]
    H4 = zeros(6, 6) + Jinv
    Jv2 = mv(Jinv, v2)
    e = [r[i] - v1[i] * dt for i in range(6)] + [Jv2[i] - v1[i] for i in range(6)]
    return e, [H1, H2, H3, H4], r


def interpolate(Lam, Psi, p1, v1, p2, v2, closed=False):
    """GaussianProcessInterpolatorPose3::interpolatePose (GaussianProcessInterpolatorPose3.h:57-105):
    (pose[12], [H1..H4] 6x6).  Lam, Psi: the 12x12 matrices of calcLambda / calcPsi."""
    Hinv = msc(-1.0, adjoint(p1))
    Hc11 = adjoint(inverse(p2))
    r = pose3_logmap(compose(inverse(p1), p2))
    Hlog = pose3_jrinv(r)
    Jinv = pose3_jrinv(r)
    r2 = list(r) + mv(Jinv, v2)
    L6, P6 = Lam[:6], Psi[:6]
    arg = [sum((L6[i][6 + j] * v1[j] for j in range(1, 6)), L6[i][6] * v1[0]) + mv([P6[i]], r2)[0] for i in range(6)]
    E = pose3_expmap(arg)
    Hexp = pose3_jr(arg)
    out = compose(p1, E)
    Hc21 = adjoint(inverse(E))
    Hexpr1 = Hexp                                           # Hcomp22 = I
    FD = fd_jrinv_x(r, v2, closed=closed)
    tmp1 = mm(mm(Hlog, Hc11), Hinv)
    tmp3 = Hlog
    HP = mm(Hexpr1, P6)
    H1 = madd(Hc21, mm(HP, tmp1 + mm(FD, tmp1)))
    H2 = mm(Hexpr1, [row[6:12] for row in L6])
    H3 = mm(HP, tmp3 + mm(FD, tmp3))
    H4 = mm(mm(Hexpr1, [row[6:12] for row in P6]), Jinv)
    return out, [H1, H2, H3, H4], r


# ------------------------------------------------------------------ bounds as arrays
def _lift(v, rel=0.0):
    """an input read exactly (rel = 0) or with a relative error of rel units of u already in it"""
    if isinstance(v, (list, tuple, np.ndarray)):
        return [_lift(x, rel) for x in v]
    return R(v, abs(v) * rel)


def _a(v):
    if isinstance(v, list):
        return [_a(x) for x in v]
    return v.a if isinstance(v, R) else 0.0           # a constant the formulas write exactly (0, 1, -1)


def gp_prior_bound(p1, v1, p2, v2, dt, closed=False):
    """(e_bound[12], H_bound (4, 12, 6)) of a float64 evaluation: GAMMA * the running bound"""
    e, H, _ = gp_prior(_lift(p1), _lift(v1), _lift(p2), _lift(v2), R(dt), closed=closed)
    return GAMMA * np.array(_a(e)), GAMMA * np.array([_a(h) for h in H])


def interpolate_bound(Lam, Psi, p1, v1, p2, v2, closed=False, cond=1.0):
    """as gp_prior_bound; Lam and Psi come out of a matrix inverse of condition `cond` (error cond * GAMMA * its row's norm)"""
    Lam, Psi = np.asarray(Lam).tolist(), np.asarray(Psi).tolist()
    # normwise: an entry that is zero in exact arithmetic (the zeros of Qc) carries the rounding of its whole row;
    # Lambda = Phi(tau) - Psi Phi(dt) cancels to zero at tau = dt: its rows carry the rounding of Phi's ones
    Lr = [[R(x, cond * max(1.0, max(abs(y) for y in row))) for x in row] for row in Lam]
    Pr = [[R(x, cond * max(abs(y) for y in row)) for x in row] for row in Psi]
    out, H, _ = interpolate(Lr, Pr, _lift(p1), _lift(v1), _lift(p2), _lift(v2), closed=closed)
    return GAMMA * np.array(_a(out)), GAMMA * np.array([_a(h) for h in H])


def lambda_psi_cond(dt):
    """condition number of Q(dt) = [[dt^3/3, dt^2/2], [dt^2/2, dt]] (x Qc), whose inverse Lambda / Psi contain"""
    Q = np.array([[dt ** 3 / 3, dt ** 2 / 2], [dt ** 2 / 2, dt]])
    return float(np.linalg.cond(Q))
