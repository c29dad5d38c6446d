"""One row per kernel form: which launch statements an iteration reached (gpslam_hip_launch_census), then the numbers.

Every fallback form of this library is a correct solver, so a handle that quietly takes another form than the one a graph is meant
to reach still matches the oracle -- what is lost is the coverage of the form it should have taken.  Each row below therefore names
the census its graph must produce and asserts it after the first iteration, BEFORE any number is looked at; then three Gauss-Newton
iterations are judged one by one against the oracle (error_before, error_after and the states at 1e-9 relative: the per-step bound of
README / DESIGN section 2), the device restarting every step from the oracle's states so that a step's error cannot hide behind
convergence; the record forms also run one damped trial (iterate_lm at lambda = 1e-2), whose level-0 launch must be the same
instantiation with the gradient store on.

FUSED_FORMS is every k_fused_level0<SV, TR, B, DG> instantiation launch_fused_k can launch; tests/test_forms_table.py (CPU) holds it
against the launch statements of level0.hip and against the forms the rows here expect, so a thirteenth instantiation -- or a
row that goes missing -- fails without a GPU.

Shapes: chunks of 4 on 70 states (18 chunks: five workgroups of four chunks, the last one ragged, a last chunk of two states), or
chunks of 2 on 64 / 65 / 66 states where the shape of the hierarchy is what the row is about."""
import numpy as np
import pytest

from oracle import oracle as O
import test_gpu_parity as T

pytestmark = pytest.mark.gpu

REL = 1e-9          # per-step bound of the fp64 path
LM_LAMBDA = 1e-2

FUSED_FORMS = [
    (0, "double", 12, False), (1, "double", 12, False), (1, "double", 12, True), (2, "double", 12, False),
    (3, "double", 12, False), (3, "double", 12, True), (4, "double", 12, False), (4, "double", 12, True),
    (0, "double", 6, False), (1, "double", 6, False),
    (0, "float", 12, False), (0, "float", 6, False),
]

PLAN = dict(unfused=1, column=2, levels_of_four=4, gp_rows=16, generic_qc=32, meas_rows=64, separate_retract=128)


def gpu():
    import gpslam_amd
    return gpslam_amd


# ---------------------------------------------------------------- graph recipes: each returns (kind, chart, feed), feed(solver) -> solver

class _Deferred:
    """A solver whose compile() waits: lets a recipe add factors behind another recipe's feed function."""

    def __init__(self, s):
        self._s = s

    def __getattr__(self, name):
        return getattr(self._s, name)

    def compile(self):
        return 0


def make_qc(d, seed, qc):
    """'full': distinct diagonal + one off-diagonal pair (the general whitening); 'diag': six DISTINCT diagonal entries (an isotropic
    Qc would not notice a permuted diagonal)."""
    Qc = np.diag(0.01 + 0.02 * np.random.default_rng(seed + 77).random(d))
    assert len(set(np.diag(Qc))) == d
    if qc == "full":
        Qc[0, 1] = Qc[1, 0] = 0.003
    return Qc


def _between_meas(kind, c, left):
    if kind in (O.LINEAR2, O.LINEAR3):
        return np.stack([c["truth_pose"][i + 1] - c["truth_pose"][i] for i in left])
    ident = {O.POSE2: np.zeros(3), O.POSE3: O.pose3((0, 0, 0), (0, 0, 0)), O.ROT3: O.rot3_ypr(0, 0, 0)}[kind]
    return np.stack([O.retract(kind, ident, O.local(kind, c["truth_pose"][i], c["truth_pose"][i + 1])) for i in left])


def chain(kind, N, seed=1, qc="full", between="one", vpriors=0, gp="shared", world=False, skip_gp=()):
    """GP priors + a pose prior on every 20th state + between factors ('one' per left state, 'none', or 'double': a second one on
    some left states) + `vpriors` velocity priors + the GP priors through one of three calls ('shared': the handle's Qc; 'same_qc':
    add_gp_priors_qc with one Qc on every prior; 'two_qc': two distinct Qc)."""
    chart = O.CHART_FIRST_ORDER if kind == O.POSE2 else O.CHART_EXPMAP
    d = O.TANGENT_DIM[kind]
    c = T.random_chain(kind, N, seed)
    if world:
        from test_gpu_vw import world_velocities
        c.update(world_velocities(c))
    Qc = make_qc(d, seed, qc)
    left = np.array([i for i in range(N - 1) if i not in set(skip_gp)], dtype=np.int32)
    bl = {"one": np.arange(N - 1), "none": np.arange(0), "double": np.concatenate([np.arange(N - 1), np.arange(5, N - 1, 13)])}[between]
    bm = _between_meas(kind, c, bl) if len(bl) else None
    vp = np.linspace(0, N - 1, vpriors).astype(np.int32) if vpriors > 1 else np.array([N // 2] * vpriors, dtype=np.int32)
    assert len(set(vp)) == vpriors

    def feed(s):
        s.set_qc(Qc)
        s.set_states(c["pose"], c["vel"])
        if gp == "shared":
            s.add_gp_priors(left, c["dt"][left])
        elif gp == "same_qc":
            s.add_gp_priors_qc(left, c["dt"][left], np.tile(Qc, (len(left), 1, 1)))
        else:
            Q2 = np.tile(Qc, (len(left), 1, 1))
            Q2[len(left) // 2:] = 1.7 * Qc + 0.001 * np.eye(d)
            s.add_gp_priors_qc(left, c["dt"][left], Q2)
        fix = np.arange(0, N, 20)
        s.add_pose_priors(fix, c["truth_pose"][fix], np.full((len(fix), d), 0.01))
        if vpriors:
            s.add_vel_priors(vp, c["truth_vel"][vp], np.full((vpriors, d), 0.05))
        if len(bl):
            s.add_between(bl, bm, np.full((len(bl), d), 0.02))
        s.compile()
        return s
    return kind, chart, feed


def gps(N, per, qc="full", vpriors=0, skip_gp=()):
    """tests/test_gpu_irows.gps_graph (SE(3) GP chain + odometry + interpolated GPS with taus at 0, dt and outside [0, dt]), with this
    file's Qc and, optionally, one velocity prior."""
    from test_gpu_irows import gps_graph
    feed0, p = gps_graph(N, seed=N, per_interval=per, skip_gp=skip_gp)
    p["qc"] = make_qc(6, N, qc)

    def feed(s):
        feed0(_Deferred(s))
        if vpriors:
            s.add_vel_priors([N // 2], p["vel"][[N // 2]] + 0.01, np.full((1, 6), 0.05))
        s.compile()
        return s
    return O.POSE3, O.CHART_EXPMAP, feed


def landmarks(N, L):
    """SE(2) chain + odometry + interpolated ranges to L landmarks (R = 1 + 2 L right-hand-side columns).  pose2_range_chain with the
    first pose and the landmarks held firmly (its own sigmas of 1 and pi leave a gauge six orders softer than the chain's shape:
    tests/test_gpu_closure.py), so that a single step is defined to 1e-9."""
    from gpslam_amd import synthetic as S
    p = S.pose2_range_chain(N, L=L, seed=3)
    p["prior_sig"] = np.full_like(p["prior_sig"], 1e-3)
    p["lprior_sig"] = np.full_like(p["lprior_sig"], 0.01)
    p["landmarks"] = p["landmark_truth"] + 0.01 * np.random.default_rng(L).standard_normal((L, 2))
    return O.POSE2, O.CHART_FIRST_ORDER, (lambda s: S.apply(p, s))


def closure(N):
    from gpslam_amd import synthetic as S
    p = S.add_loop_closures(S.pose3_chain(N, seed=2), [[3, N - 4]], seed=8)
    return O.POSE3, O.CHART_EXPMAP, (lambda s: S.apply(p, s))


# ---------------------------------------------------------------- the rows

SE3 = 2   # census "gp": SE(3) records (1: d = 3 records, 0: rows)


def fused(sv, dg=False, b=12, tr="double", **more):
    """census of an iteration whose level 0 is ONE launch of k_fused_level0<sv, tr, b, dg>"""
    e = dict(l0_fused=1, l0_rows=0, l0_column=0, sv=sv, dg=int(dg), block=b, fp32=int(tr == "float"), gsave=0, flush=0)
    e.update(more)
    return e


class Row:
    def __init__(self, id, recipe, expect, form=None, dev=None, orc=None, lm=False):
        self.id, self.recipe, self.expect, self.form, self.dev, self.orc, self.lm = id, recipe, expect, form, dev or {}, orc or {}, lm


def _dgrows(id, recipe_of_qc, sv, expect, **kw):
    """a record form and its diagonal twin: the same graph with the general and with the diagonal Qc"""
    return [Row("%s-<%d>" % (id, sv), recipe_of_qc("full"), fused(sv, False, gp=SE3, **expect), (sv, "double", 12, False), lm=True, **kw),
            Row("%s-<%d,dg>" % (id, sv), recipe_of_qc("diag"), fused(sv, True, gp=SE3, **expect), (sv, "double", 12, True), lm=True, **kw)]


N0 = 70
ROWS = []
# ---- SE(3), fp64, fused
ROWS += _dgrows("se3-between-records", lambda q: (lambda: chain(O.POSE3, N0, qc=q)), 1, dict(btw_rec=1, lines=0, odd_rows=0, lin_rec=1, lin_rec_vp=0), dev=dict(chunk=4))
ROWS += [
    Row("se3-no-between-<1>", lambda: chain(O.POSE3, N0, between="none"), fused(1, gp=SE3, btw_rec=0, odd_rows=0, lin_rec=1), (1, "double", 12, False), dev=dict(chunk=4), lm=True),
    Row("se3-two-betweens-on-a-state-<1>", lambda: chain(O.POSE3, N0, between="double"), fused(1, gp=SE3, btw_rec=0, odd_rows=0, lin_rec=1), (1, "double", 12, False), dev=dict(chunk=4), lm=True),
    Row("se3-one-velocity-prior-<2>", lambda: chain(O.POSE3, N0, vpriors=1), fused(2, gp=SE3, btw_rec=0, odd_rows=1, lin_rec_vp=1, lin_rec=0), (2, "double", 12, False), dev=dict(chunk=4), lm=True),
    # 8 priors = 48 rows = 4 b: the last "few" of the rule other > 4 * b
    Row("se3-eight-velocity-priors-<2>", lambda: chain(O.POSE3, N0, vpriors=8), fused(2, gp=SE3, btw_rec=0, odd_rows=1, lin_rec_vp=1), (2, "double", 12, False), dev=dict(chunk=4), lm=True),
]
ROWS += _dgrows("se3-nine-velocity-priors", lambda q: (lambda: chain(O.POSE3, N0, qc=q, vpriors=9)), 3, dict(btw_rec=0, lines=0, odd_rows=2, lin_rec_vp=1), dev=dict(chunk=4))
ROWS += _dgrows("se3-gps-as-rows", lambda q: (lambda: gps(41, 4, qc=q)), 3, dict(lines=0, odd_rows=2, gps_lines=0, meas_rec=1, meas_self=0), dev=dict(chunk=4, plan=PLAN["meas_rows"]))
ROWS += _dgrows("se3-gps+velocity-prior", lambda q: (lambda: gps(41, 4, qc=q, vpriors=1)), 3, dict(lines=0, odd_rows=2, gps_lines=0, meas_rec=1, meas_self=0, lin_rec_vp=1), dev=dict(chunk=4))
# (the factor on the interval without a record forms its blocks inside k_meas: one launch, with the records attached)
ROWS += _dgrows("se3-gps-on-an-interval-without-gp-prior", lambda q: (lambda: gps(41, 4, qc=q, skip_gp=(17,))), 3, dict(lines=0, odd_rows=2, gps_lines=0, meas_rec=1, meas_self=0), dev=dict(chunk=4))
for per in (1, 4, 13):
    ROWS += _dgrows("se3-gps-lines-%d-per-interval" % per, lambda q, per=per: (lambda: gps(41, per, qc=q)), 4, dict(lines=1, btw_rec=0, gps_lines=1, meas_rec=0, meas_self=0, lin_rec=1), dev=dict(chunk=4))
ROWS += [
    # interpolated GPS beside GP priors that travel as rows: no records to read, k_meas forms every factor's blocks itself
    Row("se3-gps-plan-gp-rows-<0>", lambda: gps(41, 4), fused(0, gp=0, btw_rec=0, lines=0, gps_lines=0, meas_rec=0, meas_self=1, lin_rows=1, lin_rec=0), (0, "double", 12, False),
        dev=dict(chunk=4, plan=PLAN["gp_rows"])),
    Row("se3-plan-gp-rows-<0>", lambda: chain(O.POSE3, N0), fused(0, gp=0, btw_rec=0, lines=0, lin_rows=1, lin_rows_vp=0, lin_rec=0), (0, "double", 12, False), dev=dict(chunk=4, plan=PLAN["gp_rows"])),
    Row("se3-world-velocities-<0>", lambda: chain(O.POSE3, N0, world=True, vpriors=2), fused(0, gp=0, btw_rec=0, lin_vw_vp=1, lin_rec=0, lin_rec_vp=0, lin_rows=0), (0, "double", 12, False),
        dev=dict(chunk=4, velocity_world=True), orc=dict(velocity_world=True)),
    Row("se3-two-qc-<0>", lambda: chain(O.POSE3, N0, gp="two_qc"), fused(0, gp=0, btw_rec=0, lin_groups=2, lin_rec=0, lin_rows=0), (0, "double", 12, False), dev=dict(chunk=4)),
    Row("se3-one-qc-on-every-prior-<1>", lambda: chain(O.POSE3, N0, gp="same_qc"), fused(1, gp=SE3, btw_rec=1, lin_groups=0, lin_rec=1), (1, "double", 12, False), dev=dict(chunk=4), lm=True),
]
# ---- block size 6, fp64
for kind in (O.POSE2, O.ROT3, O.LINEAR3):
    ROWS.append(Row("b6-%s-<1,6>" % T.NAMES[kind], lambda kind=kind: chain(kind, N0), fused(1, b=6, gp=1, lin_rec=1), (1, "double", 6, False), dev=dict(chunk=4)))
ROWS.append(Row("b6-pose2-plan-gp-rows-<0,6>", lambda: chain(O.POSE2, N0), fused(0, b=6, gp=0, lin_rows=1, lin_rec=0), (0, "double", 6, False), dev=dict(chunk=4, plan=PLAN["gp_rows"])))
# ---- not fused
ROWS += [
    Row("rows-plan-unfused-b12", lambda: chain(O.POSE3, N0), dict(l0_fused=0, l0_rows=1, l0_column=0, sv=-1, bwd_rows=1), dev=dict(chunk=4, plan=PLAN["unfused"])),
    Row("rows-plan-unfused-b6", lambda: chain(O.POSE2, N0), dict(l0_fused=0, l0_rows=1, l0_column=0, sv=-1, bwd_rows=1), dev=dict(chunk=4, plan=PLAN["unfused"])),
    Row("rows-linear2-b4", lambda: chain(O.LINEAR2, N0), dict(l0_fused=0, l0_rows=1, l0_column=0, sv=-1, bwd_rows=1), dev=dict(chunk=4)),
    # A chain of a single level (no more states than the top level takes: 8): level0_mode refuses the fused kernel.  That level is
    # the top solve, which keeps no separator -- the one shape k_chunk_forward_rows does not take (launch_fwd: !a.no_sep): its
    # forward elimination is k_chunk_forward's sequential form, its back-substitution the row-layout kernel.
    Row("single-level-chain", lambda: chain(O.POSE3, 8), dict(levels=1, l0_fused=0, l0_rows=0, l0_column=0, top_chunk=1, sv=-1, bwd_rows=1, upper_cr=0, upper_chunk=0), dev=dict(chunk=16)),
    Row("column-plan-column", lambda: chain(O.POSE3, N0), dict(l0_fused=0, l0_rows=0, l0_column=1, l0_column_fast=1, sv=-1, bwd_rows=0), dev=dict(chunk=4, plan=PLAN["column"])),
    Row("column-4-landmarks-fast", lambda: landmarks(N0, 4), dict(l0_fused=0, l0_rows=0, l0_column=1, l0_column_fast=1, sv=-1, bwd_rows=0, upper_cr=0), dev=dict(chunk=4, landmark_dim=2), orc=dict(landmark_dim=2)),
    Row("column-11-landmarks", lambda: landmarks(N0, 11), dict(l0_fused=0, l0_rows=0, l0_column=1, l0_column_fast=0, sv=-1, bwd_rows=0, upper_cr=0), dev=dict(chunk=4, landmark_dim=2), orc=dict(landmark_dim=2)),
]
# ---- above level 0: chunks of 2 give two levels up to 64 states and three from 65 on, level 1 then in groups of four
for kind, b, gp_ in ((O.POSE3, 12, SE3), (O.POSE2, 6, 1)):
    form = (1, "double", b, False)
    nm = T.NAMES[kind]
    for N, tail in ((64, 0), (65, 1), (66, 1)):
        # tail on: the fused kernel reduces level 1, level 2 is one cyclic-reduction launch that also solves itself, and the row-layout
        # back-substitution solves its group of four of level 1 (fold_tail_bwd)
        ROWS.append(Row("upper-%s-%d" % (nm, N), lambda kind=kind, N=N: chain(kind, N), fused(1, b=b, gp=gp_, tail=tail, tail_launches=tail, upper_cr=1, upper_chunk=0,
                        bwd_rows=1, bwd_rows_fold=tail, upper_bwd=0, bwd_chunk=0), form, dev=dict(chunk=2)))
    ROWS += [
        Row("upper-%s-65-forced-sharded" % nm, lambda kind=kind: chain(kind, 65), fused(1, b=b, gp=gp_, tail=0, tail_launches=0, upper_cr=2, upper_chunk=0, upper_bwd=2, bwd_rows_fold=0,
                                                                                      top_chunk=1, bwd_rows=2),     # (the reduced system of the one segment: a top solve of its own)
            form,
            dev=dict(chunk=2, force_sharded=True)),
        Row("upper-%s-65-levels-of-four" % nm, lambda kind=kind: chain(kind, 65), fused(1, b=b, gp=gp_, tail=0, tail_launches=0, upper_cr=0, upper_chunk="levels-1", bwd_rows_fold=0, upper_bwd=0), form,
            dev=dict(chunk=2, plan=PLAN["levels_of_four"])),
        Row("upper-%s-65-pinned-shape" % nm, lambda kind=kind: chain(kind, 65), fused(1, b=b, gp=gp_, tail=0, tail_launches=0, upper_cr=0, upper_chunk="levels-1", bwd_rows_fold=0, upper_bwd=0), form,
            dev=dict(chunk=2, upper_chunk=4, top_blocks=8)),
    ]

FP32_ROWS = [
    Row("fp32-pose3-<0,float>", lambda: chain(O.POSE3, N0, vpriors=2), fused(0, tr="float", gp=0, btw_rec=0, lines=0, lin_rec=0, lin_rec_vp=0), (0, "float", 12, False), dev=dict(chunk=4, precision=1)),
    Row("fp32-pose2-<0,float,6>", lambda: chain(O.POSE2, N0, vpriors=2), fused(0, tr="float", b=6, gp=0, btw_rec=0, lines=0, lin_rec=0, lin_rec_vp=0), (0, "float", 6, False), dev=dict(chunk=4, precision=1)),
]


def expected_forms():
    """the k_fused_level0 instantiations the rows of this file expect (tests/test_forms_table.py)"""
    return {r.form for r in ROWS + FP32_ROWS if r.form is not None}


# ---------------------------------------------------------------- running a row

def check_census(census, expect, what, info=None):
    bad = {}
    for k, v in expect.items():
        if v == "levels-1":
            v = info["levels"] - 1
        got = info["levels"] if k == "levels" else census[k]
        if got != v:
            bad[k] = (got, v)
    assert not bad, "%s: launch census differs from the form this row is for {key: (got, expected)} %s\nwhole census: %s" % (what, bad, census)


def rel_close(a, b, rel, what):
    print("%s: device %.17g oracle %.17g (relative difference %.3e)" % (what, a, b, abs(a - b) / max(1.0, abs(b))))
    assert abs(a - b) <= rel * max(1.0, abs(b)), what


def build(row):
    kind, chart, feed = row.recipe()
    orc = feed(O.Chain(kind, chart, **row.orc))
    dev = feed(gpu().ChainSolver(kind, chart, **row.dev))
    return kind, orc, dev


def sync_states(orc, dev):
    dev.set_states(*orc.get_states())
    if getattr(dev, "L", 0):
        dev.set_landmarks(orc.get_landmarks())


def judge_step(kind, orc, dev, s0, s1, what, rel=REL):
    rel_close(s1.error_before, s0.error_before, rel, what + " error_before")
    rel_close(s1.error_after, s0.error_after, rel, what + " error_after")
    (x0, v0), (x1, v1) = orc.get_states(), dev.get_states()
    T.states_close(kind, x0, v0, x1, v1, rel)
    if getattr(dev, "L", 0):
        l0, l1 = orc.get_landmarks(), dev.get_landmarks()
        assert np.abs(l0 - l1).max() <= rel * max(1.0, np.abs(l0).max()), what + " landmarks"


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_form(row):
    kind, orc, dev = build(row)
    start = orc.get_states()
    info = dev.plan_info()
    dev.launch_census()                                   # (nothing an iteration launches has run yet: start from zero)
    rc1, s1 = dev.iterate_gn()
    check_census(dev.launch_census(), row.expect, row.id, info)      # the form first ...
    rc0, s0 = orc.iterate_gn()                            # ... then the numbers
    assert rc0 == 0 and rc1 == 0
    judge_step(kind, orc, dev, s0, s1, row.id + " step 1")
    for it in (2, 3):
        sync_states(orc, dev)
        rc0, s0 = orc.iterate_gn()
        rc1, s1 = dev.iterate_gn()
        assert rc0 == 0 and rc1 == 0
        judge_step(kind, orc, dev, s0, s1, "%s step %d" % (row.id, it))
    if row.lm:
        # The damped trial, from the recipe's initial states: there the cost moves by orders of magnitude, so keeping the step is no
        # decision of a rounding error (three steps on, at the converged point, it would be) and the trial is judged like a step.
        orc.set_states(*start); dev.set_states(*start)
        dev.launch_census()
        rc0, s0, lam0 = orc.iterate_lm(LM_LAMBDA)
        rc1, s1, lam1 = dev.iterate_lm(LM_LAMBDA)
        c = dev.launch_census()
        lm = {k: row.expect[k] for k in ("sv", "dg", "block", "fp32", "gp", "btw_rec", "lines", "odd_rows") if k in row.expect}
        lm.update(gsave=1, gsave_launches=s1.trials, l0_fused=s1.trials, l0_rows=0, l0_column=0)
        check_census(c, lm, row.id + " damped trial", info)
        assert rc0 == 0 and rc1 == 0
        what = row.id + " damped trial"
        assert s0.error_after < 0.5 * s0.error_before, (what, s0.error_before, s0.error_after)      # the cost moved: nothing here is noise
        assert (s1.accepted, s1.trials, lam1) == (s0.accepted, s0.trials, lam0) == (1, 1, LM_LAMBDA / 10.0), (what, s0.accepted, s0.trials, lam0, s1.accepted, s1.trials, lam1)
        judge_step(kind, orc, dev, s0, s1, what)
    dev.close()


@pytest.mark.parametrize("row", FP32_ROWS, ids=[r.id for r in FP32_ROWS])
def test_fp32_form(row):
    """fp32 row tables into the fused kernel: no records, TR = float.  Numbers by the rule of tests/test_gpu_fp32.py: the converged
    states against the oracle's fp64 fixed point."""
    from test_gpu_fp32 import FP32_STATE_REL, _converge, _rel_state_diff
    kind, orc, dev = build(row)
    dev.launch_census()
    dev.iterate_gn()
    check_census(dev.launch_census(), row.expect, row.id)
    for _ in range(12):
        orc.iterate_gn()
    h = _converge(dev, 11)
    rel = _rel_state_diff(kind, orc, dev)
    print("%s: relative state difference %.3e, |delta| history %s" % (row.id, rel, ["%.1e" % x for x in h]))
    assert rel <= FP32_STATE_REL, rel
    dev.close()


def test_diagonal_qc_differs_from_the_generic_form_in_dg_only_and_in_no_bit():
    """<1, double, 12, true> skips products with exact zeros: its states equal the general form's (PLAN_GENERIC_QC) bit for bit, and
    the two censuses differ in `dg` alone."""
    kind, chart, feed = chain(O.POSE3, N0, qc="diag")
    out, cen = [], []
    for plan in (0, PLAN["generic_qc"]):
        s = feed(gpu().ChainSolver(kind, chart, chunk=4, plan=plan))
        s.launch_census()
        for _ in range(3):
            s.iterate_gn()
        cen.append(s.launch_census())
        out.append(s.get_states())
        s.close()
    assert cen[0]["dg"] == 1 and cen[1]["dg"] == 0, cen
    assert {k for k in cen[0] if cen[0][k] != cen[1][k]} == {"dg"}, cen
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_set_qc_after_compile_switches_the_form_and_back():
    """diagonal -> general -> diagonal Qc on a compiled handle: `dg` of the launches follows, the states follow the oracle."""
    kind, chart, feed = chain(O.POSE3, N0, qc="diag")
    orc, dev = feed(O.Chain(kind, chart)), feed(gpu().ChainSolver(kind, chart, chunk=4))
    dev.launch_census()
    for stage, (q, dg) in enumerate((("diag", 1), ("full", 0), ("diag", 1))):
        if stage:
            Qc = make_qc(6, 10 + stage, q)
            orc.set_qc(Qc); dev.set_qc(Qc)
            sync_states(orc, dev)
        rc1, s1 = dev.iterate_gn()
        check_census(dev.launch_census(), fused(1, bool(dg), gp=SE3, btw_rec=1), "set_qc stage %d" % stage)
        rc0, s0 = orc.iterate_gn()
        assert rc0 == 0 and rc1 == 0
        judge_step(kind, orc, dev, s0, s1, "set_qc stage %d" % stage)
    dev.close()


# ---------------------------------------------------------------- the size rules of block size 6 (no oracle: it takes seconds per iteration here)

def _vs_unfused(make, feed, expect, what, iters=2):
    """census of the handle make() returns, then its states against a PLAN_UNFUSED_LEVEL0 handle of the same graph at 1e-9"""
    dev, ref = feed(make(0)), feed(make(PLAN["unfused"]))
    dev.launch_census()
    dev.iterate_gn()
    check_census(dev.launch_census(), expect, what)
    ref.iterate_gn()
    for _ in range(iters - 1):
        dev.iterate_gn(); ref.iterate_gn()
    (x0, v0), (x1, v1) = ref.get_states(), dev.get_states()
    T.states_close(dev.kind, x0, v0, x1, v1, REL)
    dev.close(); ref.close()


@pytest.mark.parametrize("N,family", [(131072, "l0_fused"), (131073, "l0_rows")])
def test_block6_size_rule(N, family):
    """SO(3) + interpolated attitude (measurement rows in the ring: not `pure6`): fused up to 131072 states, row layout beyond."""
    from gpslam_amd import synthetic as S
    p = S.rot3_attitude_chain(N, per_interval=1, refs=2)
    expect = dict(l0_fused=0, l0_rows=0, l0_column=0)
    expect[family] = 1
    _vs_unfused(lambda plan: gpu().ChainSolver(O.ROT3, plan=plan), lambda s: S.apply(p, s), expect, "block-6 size rule at %d states" % N)


@pytest.mark.parametrize("vpriors,family", [(8, "l0_fused"), (9, "l0_rows")])
def test_block6_pure_record_chain_stays_fused_beyond_the_size_rule(vpriors, family):
    """`pure6`: 131073 states of a 3-D linear chain whose full-width rows besides the GP records are 8 velocity priors (24 rows = 4 b:
    fused at every size) or 9 (the size rule applies).  Position fixes are compact rows and do not count."""
    from gpslam_amd import synthetic as S
    N = 131073
    p = S.linear_chain(N)
    idx = np.linspace(0, N - 1, vpriors).astype(np.int32)
    p.update(vprior_idx=idx, vprior=p["vel"][idx].copy(), vprior_sig=np.full((vpriors, 3), 0.05))
    expect = dict(l0_fused=0, l0_rows=0, l0_column=0, lin_rec_vp=1)
    expect[family] = 1
    if family == "l0_fused":
        expect.update(sv=1, block=6, gp=1)
    _vs_unfused(lambda plan: gpu().ChainSolver(O.LINEAR3, plan=plan), lambda s: S.apply(p, s), expect, "pure6 with %d velocity priors" % vpriors)


# ---------------------------------------------------------------- the retraction folded into the next K1 (run_gn)

def _missing_gp():
    return chain(O.POSE3, N0, skip_gp=(31,))


RETRACT = [
    ("foldable", lambda: chain(O.POSE3, N0), {}, dict(lin_pend=4, retract=1, flush=0)),
    ("foldable-d3", lambda: chain(O.POSE2, N0), {}, dict(lin_pend=4, retract=1, flush=0)),
    ("plan-separate-retract", lambda: chain(O.POSE3, N0), dict(plan=PLAN["separate_retract"]), dict(lin_pend=0, retract=5, flush=0)),
    ("a-state-without-gp-prior", _missing_gp, {}, dict(lin_pend=0, retract=5, flush=0)),
    ("a-closure", lambda: closure(N0), {}, dict(lin_pend=0, retract=5, flush=0)),
    ("a-landmark", lambda: landmarks(N0, 4), dict(landmark_dim=2), dict(lin_pend=0, retract=5, flush=0)),
]


@pytest.mark.parametrize("id,recipe,kw,expect", RETRACT, ids=[r[0] for r in RETRACT])
def test_run_gn_retraction_census(id, recipe, kw, expect):
    """run_gn(5): four k_lin launches apply the previous iteration's update and one k_retract ends the run -- where compile() found
    the chain foldable; everywhere else five k_retract launches, and never the defensive flush of launch_factors (which would make a
    library that never folds correct, and slower)."""
    kind, chart, feed = recipe()
    okw = dict(landmark_dim=kw["landmark_dim"]) if "landmark_dim" in kw else {}
    orc, dev = feed(O.Chain(kind, chart, **okw)), feed(gpu().ChainSolver(kind, chart, chunk=4, **kw))
    dev.launch_census()
    st, _ = dev.run_gn(5)
    check_census(dev.launch_census(), expect, "run_gn(5), " + id)
    for _ in range(5):
        rc0, s0 = orc.iterate_gn()
        assert rc0 == 0
    judge_step(kind, orc, dev, s0, st, "run_gn(5), " + id)
    dev.close()
