"""Do two builds of the library compute the same bits?  A fixed list of small graphs through the library named by GPSLAM_LIB (or the
tree's own build); states, landmarks, statistics, rows, weights and the launch census of each into one .npz per graph.

   GPSLAM_LIB=.../libgpslam_hip.so python scripts/ab_outputs.py OUT_DIR [--fork] [--only SUBSTRING]    (one library per process)
   python scripts/ab_outputs.py --compare DIR_A DIR_B                                                  (byte by byte; exit status 1 on any difference)

The list reaches every arm of launch_factors at the smallest size where it exists: the merged k_lin launch in its record, row and
world-velocity forms with and without velocity priors, the launch per Qc group, a chain with a GP prior missing, the eight
measurement kinds the generators have (interpolated GPS as lines and as rows), landmarks on the dense border and on segments, landmark
priors, an fp32 handle, one sharded rank through the phase calls, closures in one pass and in column passes, robust weights, state
and border Gaussians.  On each graph: iterate_gn, get_rows, run_gn(4) (the pending update, the deferred sums), error, iterate_lm from
the initial values, an iterate_lm whose every trial is rejected, the weights, linearize_meas, and the callers of the launchers in
other translation units (marginals, log_determinant, iterate_dogleg).  A call the library refuses is recorded with its message.
The segmented landmark elimination has a list of its own in cases() -- fp64 and fp32 rows, block sizes 6 and 12, the fused sweep and
its two-launch form, the fat block size NB in each of its three ranges (asserted against segment_plan()) -- and run_split() takes a
chain split in two pieces through the phase calls, in fp64 and in fp32.
--fork adds the one graph that forks onto the second stream (config 4 at 524288 states, one iteration): launch_factors and fs_forward."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

FORK_STATES = 524288      # kForkMinStates (the library's constant)


def stats_row(st):
    return np.array([st.error_before, st.error_after, st.delta_inf_norm, st.lambda_, st.iterations, st.status, st.accepted, st.trials, st.last_trial_error])


def strip_landmarks(p):
    return {k: v for k, v in p.items() if not (k.startswith("range_") or k.startswith("lprior") or k.startswith("landmark"))}


def anchored(p):
    q = dict(p)
    q["prior_sig"] = np.full_like(p["prior_sig"], 1e-3)
    return q


def with_vpriors(p):
    q = dict(p)
    d = q["vel"].shape[1]
    q.update(vprior_idx=np.array([0, q["N"] - 1], dtype=np.int32), vprior=q["vel"][[0, -1]].copy(), vprior_sig=np.full((2, d), 0.1))
    return q


def pairs(N, K, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < K:
        i, j = (int(v) for v in rng.integers(0, N, 2))
        if abs(i - j) > 1:
            out.append([i, j])
    return out


class Case:
    def __init__(self, name, problem, kw=None, feed=None, after=None, mode="local", only_gn=False, nb=None):
        self.name, self.problem, self.kw, self.feed, self.after, self.mode, self.only_gn = name, problem, kw or {}, feed, after, mode, only_gn
        self.nb = nb      # segmented graphs: (lowest, highest) fat block size NB the plan must report


def pose3_local_landmarks(N, L, half=12, seed=5):
    """an SE(3) chain (block size 12) past L point landmarks, each ranged from the states within `half` of its closest approach"""
    from gpslam_amd import synthetic as S
    rng = np.random.default_rng(seed)
    p = S.pose3_chain(N, seed=seed)
    t = p["pose"][:, 9:12]
    centre = ((np.arange(L) + 0.5) * (N / L)).astype(np.int64)
    lmk = t[centre] + np.array([0.0, 4.0, 1.0]) + rng.standard_normal((L, 3))
    idx = np.concatenate([np.arange(max(c - half, 0), min(c + half, N), 3) for c in centre]).astype(np.int32)
    lm = np.concatenate([np.full(len(np.arange(max(c - half, 0), min(c + half, N), 3)), l) for l, c in enumerate(centre)]).astype(np.int32)
    z = np.linalg.norm(lmk[lm] - t[idx], axis=1) + 0.05 * rng.standard_normal(len(idx))
    p.update(landmarks=lmk + 0.1 * rng.standard_normal((L, 3)), lprior_idx=np.arange(L, dtype=np.int32), lprior=lmk.copy(), lprior_sig=np.full((L, 3), 1.0),
             prange_idx=idx, prange_lm=lm, prange_z=z, prange_sigma=np.full(len(idx), 0.05))
    return p


def cases(gp, S, fork):
    from gpslam_amd import plaza
    C = gp.chain
    out = []
    for N in (2, 3, 64, 333, 700, 1001):
        out.append(Case("se3-%d" % N, lambda N=N: S.pose3_chain(N)))
        out.append(Case("se3-%d-vpriors" % N, lambda N=N: with_vpriors(S.pose3_chain(N))))
    out.append(Case("linear3-300", lambda: S.linear_chain(300)))
    out.append(Case("linear2-300", lambda: S.linear_chain(300, D=2)))
    out.append(Case("pose2-300", lambda: anchored(strip_landmarks(S.pose2_range_chain(300, seed=9)))))
    out.append(Case("rot3-attitude-300", lambda: S.rot3_attitude_chain(300, refs=2)))
    out.append(Case("rot3-bias-ahrs-200", lambda: S.rot3_bias_ahrs_chain(200)))
    out.append(Case("se3-world-velocity-200", lambda: with_vpriors(S.pose3_chain(200)), dict(velocity_world=True)))
    out.append(Case("se3-world-velocity-201", lambda: S.pose3_chain(201), dict(velocity_world=True)))

    def two_qc(p, s):      # synthetic.apply with the GP priors through add_gp_priors_qc, alternating between two Qc
        Qc = np.tile(p["qc"], (len(p["gp_left"]), 1, 1))
        Qc[1::2] *= 2.0
        s.set_qc(p["qc"])
        s.set_states(p["pose"], p["vel"])
        s.add_gp_priors_qc(p["gp_left"], p["gp_dt"], Qc)
        s.add_pose_priors(p["prior_idx"], p["prior_pose"], p["prior_sig"])
        if "vprior_idx" in p:
            s.add_vel_priors(p["vprior_idx"], p["vprior"], p["vprior_sig"])
        if "between_left" in p:
            s.add_between(p["between_left"], p["between_meas"], p["between_sig"])
        s.compile()
        return s
    out.append(Case("se3-two-qc-150", lambda: S.pose3_chain(150), feed=two_qc))
    out.append(Case("linear3-two-qc-150", lambda: S.linear_chain(150), feed=two_qc))

    def gap(p):
        q = dict(p)
        keep = np.arange(len(p["gp_left"])) != len(p["gp_left"]) // 2
        q["gp_left"], q["gp_dt"] = p["gp_left"][keep], p["gp_dt"][keep]
        return q
    out.append(Case("se3-missing-gp-prior-150", lambda: gap(S.pose3_chain(150))))

    def gps(N, odo):
        p = S.pose3_gps_chain(N, per_interval=2, seed=1, keep_odometry=odo)
        fix = np.arange(0, N, 15).astype(np.int32)
        p.update(prior_idx=fix, prior_pose=p["pose"][fix].copy(), prior_sig=np.full((len(fix), 6), 0.05))
        return p
    out.append(Case("se3-gps-lines-300", lambda: gps(300, False)))
    out.append(Case("se3-gps-rows-300", lambda: gps(300, False), dict(plan=C.PLAN_MEAS_ROWS)))
    out.append(Case("se3-gps-odometry-300", lambda: gps(300, True)))
    out.append(Case("se3-gps-gp-rows-300", lambda: gps(300, True), dict(plan=C.PLAN_GP_ROWS)))

    def no_lpriors(p):
        return {k: v for k, v in p.items() if not k.startswith("lprior")}
    out.append(Case("pose2-ranges-300", lambda: no_lpriors(anchored(S.pose2_range_chain(300, L=4, seed=3))), dict(landmark_dim=2)))
    out.append(Case("pose2-ranges-landmark-priors-300", lambda: anchored(S.pose2_range_chain(300, L=4, seed=3)), dict(landmark_dim=2)))
    out.append(Case("plaza2", lambda: plaza.build_problem(plaza.load(os.path.join(ROOT, "tests", "golden", "plaza2.npz"))),
                    dict(chart=gp.CHART_FIRST_ORDER, landmark_dim=2), feed=lambda p, s: plaza.apply(p, s)))
    out.append(Case("fp32-se3-64-vpriors", lambda: with_vpriors(S.pose3_chain(64)), dict(chunk=4, precision=1)))
    out.append(Case("fp32-pose2-ranges-300", lambda: anchored(S.pose2_range_chain(300, L=4, seed=3)), dict(landmark_dim=2, precision=1)))
    out.append(Case("fp32-rot3-attitude-300", lambda: S.rot3_attitude_chain(300, refs=2), dict(precision=1)))
    from gpslam_amd import sharded
    one_rank = lambda p, s: sharded.apply_local(sharded.local_problem(p, 0, 1), s)
    out.append(Case("sharded-one-rank-se3-200", lambda: S.pose3_chain(200), dict(rank=0, nranks=1, force_sharded=True), feed=one_rank, mode="sharded"))
    out.append(Case("sharded-one-rank-pose2-ranges-300", lambda: anchored(S.pose2_range_chain(300, L=4, seed=3)),
                    dict(landmark_dim=2, rank=0, nranks=1, force_sharded=True), feed=one_rank, mode="sharded"))
    out.append(Case("segmented-pose2-600", lambda: S.pose2_local_landmarks_chain(600, window=100, seed=2),
                    dict(chart=gp.CHART_FIRST_ORDER, landmark_dim=2, force_segmented=True), feed=lambda p, s: (s.marginals_on_segments(), S.apply(p, s))[1]))
    # The segmented landmark elimination (fatsep.hip), every launch of it at the smallest size that reaches it.  The graph above: block
    # size 6 with fp64 rows, NB = 16 -- k_fs_factor_rows6, k_fs_gev, k_fs_sweep_syrk<6, 3>, k_fs_lm_terms, k_fs_fat_assemble,
    # k_fat_elim_rows<16> / k_fat_update / k_fat_top / k_fat_back_rows<16>, k_fs_scatter, k_fs_rhs, k_fs_solve1; its landmark priors reach
    # k_fs_lmprior_err in every error pass, its retractions k_fs_lm_update and k_fs_max_into, its marginals fs_forward through their own
    # Y (k_fs_sweep, k_fs_syrk<7, 112>).
    seg_feed = lambda p, s: (s.marginals_on_segments(), S.apply(p, s))[1]
    seg_kw = dict(chart=gp.CHART_FIRST_ORDER, landmark_dim=2, force_segmented=True)
    local600 = lambda L=None: S.pose2_local_landmarks_chain(600, L=L, window=100, seed=2)
    out[-1].nb = (16, 16)
    # ... with fp32 rows: the <float> instantiation of every kernel above but k_fs_factor_rows6 (the generic k_fs_factor<6> instead)
    out.append(Case("segmented-fp32-pose2-600", local600, dict(precision=1, **seg_kw), feed=seg_feed, nb=(16, 16)))
    # ... and with GPSLAM_PLAN_FS_TWO_LAUNCHES: k_fs_sweep and k_fs_syrk<7, 112> through the plan's Y in place of k_fs_sweep_syrk
    out.append(Case("segmented-two-launches-pose2-600", local600, dict(plan=C.PLAN_FS_TWO_LAUNCHES, **seg_kw), feed=seg_feed, nb=(16, 16)))
    # block size 12 (SE(3), point landmarks, plain ranges): the generic k_fs_factor<12>, k_fs_gev<12>, k_fs_sweep<12> and k_fs_syrk through
    # Y, k_fs_rhs<12>, k_fs_solve1<12>
    def plain_ranges(p, s):
        s.marginals_on_segments()
        S.apply(p, s)
        s.add_range(p["prange_idx"], p["prange_lm"], p["prange_z"], p["prange_sigma"])
        s.compile()
        return s
    out.append(Case("segmented-se3-130", lambda: pose3_local_landmarks(130, 8), dict(landmark_dim=3, force_segmented=True, segment_length=64), feed=plain_ranges, nb=(24, 24)))
    # the fat block size NB in its three ranges (landmarks per window against a segment length of 128).  Up to 48: the graphs above.
    # 52 - 80: k_fat_elim_mfma, k_fat_back_w4, and at NB = 52 k_fs_sweep_syrk<6, 7> (NCP = 112), at NB = 80 k_fs_syrk<17, 176>.  Above 80:
    # k_fat_elim_wide_mfma and k_fs_syrk<20, 272> over two workgroups per segment
    wide_kw = dict(segment_length=128, **seg_kw)
    out.append(Case("segmented-nb52-pose2-600", lambda: local600(120), wide_kw, feed=seg_feed, nb=(52, 52)))
    out.append(Case("segmented-nb80-pose2-300", lambda: S.pose2_local_landmarks_chain(300, L=130, window=100, seed=2), wide_kw, feed=seg_feed, nb=(80, 80)))
    out.append(Case("segmented-nb92-pose2-400", lambda: S.pose2_local_landmarks_chain(400, L=170, window=100, seed=2), wide_kw, feed=seg_feed, nb=(92, 92)))
    out.append(Case("closure-se3-200", lambda: S.add_loop_closures(S.pose3_chain(200, seed=2), [[3, 196]], seed=8)))
    out.append(Case("closures-pose2-300", lambda: S.add_loop_closures(anchored(strip_landmarks(S.pose2_range_chain(300, seed=9))), [[3, 140], [299, 60], [61, 150]], seed=4)))
    passes = lambda p, s: (s.set_closure_passes(32), s.marginals_keep_closure_columns(), S.apply(p, s))[2]
    out.append(Case("closure-passes-pose2-300", lambda: S.add_loop_closures(anchored(strip_landmarks(S.pose2_range_chain(300, seed=9))), pairs(300, 12, 21), seed=5), feed=passes))
    out.append(Case("closure-passes-se3-200", lambda: S.add_loop_closures(S.pose3_chain(200, seed=2), pairs(200, 6, 31), seed=8), feed=passes))

    def robust(p, s):
        S.apply(p, s)
        M = len(p["range_left"])
        s.set_meas_robust(C.MEAS_INTERP_RANGE, np.full(M, C.ROBUST_HUBER, dtype=np.int32), np.full(M, 1.0))
        if "closure_first" in p:
            K = len(p["closure_first"])
            s.set_between_pairs_robust(np.full(K, C.ROBUST_CAUCHY, dtype=np.int32), np.full(K, 1.0))
        s.compile()
        return s
    out.append(Case("robust-pose2-ranges-300", lambda: anchored(S.pose2_range_chain(300, L=4, seed=3)), dict(landmark_dim=2), feed=robust))
    out.append(Case("robust-closures-pose2-ranges-300", lambda: S.add_loop_closures(anchored(S.pose2_range_chain(300, L=4, seed=3)), [[3, 140], [299, 60]], seed=4),
                    dict(landmark_dim=2), feed=robust))

    def head(onto):
        def feed(p, s):
            S.apply(p, s)
            s.iterate_gn()
            if onto:
                s.marginalize_head_onto_landmarks()
            s.marginalize_head(5)
            s.compile()
            return s
        return feed
    out.append(Case("state-gaussian-se3-100", lambda: S.pose3_chain(100), feed=head(False)))
    out.append(Case("border-gaussian-pose2-ranges-120", lambda: anchored(S.pose2_range_chain(120, L=4, seed=3)), dict(landmark_dim=2), feed=head(True)))
    if fork:
        out.append(Case("fork-config4-%d" % FORK_STATES, lambda: S.pose2_local_landmarks_chain(FORK_STATES, window=200),
                        dict(chart=gp.CHART_FIRST_ORDER, landmark_dim=2), only_gn=True))
    return out


MEAS_OF = (("range_left", 0), ("att_left", 2), ("gps_left", 3), ("ahrs_left", 7))


def run_case(gp, S, c):
    C = gp.chain
    p = c.problem()
    s = gp.ChainSolver(p["kind"], **c.kw)
    rec, log = {}, []

    def op(name, f):
        try:
            v = f()
        except gp.GpslamHipError as ex:
            log.append("%s: %s" % (name, ex))
            return None
        if v is not None:
            for k, a in (v.items() if isinstance(v, dict) else [("", v)]):
                rec[name + k] = np.ascontiguousarray(a)
        return v

    def state():
        out = dict(zip((".pose", ".vel"), s.get_states()))
        if s.L:
            out[".landmarks"] = s.get_landmarks()
        return out

    (c.feed or S.apply)(p, s)
    if c.nb:
        plan = s.segment_plan()
        assert plan["active"] == 1 and c.nb[0] <= plan["NB"] <= c.nb[1], (c.name, plan)
        rec["segment_plan"] = np.array(list(plan.values()))
    pose0, vel0 = s.get_states()
    lm0 = s.get_landmarks() if s.L else None
    op("plan", lambda: np.array(list(s.plan_info().values())))
    s.launch_census(reset=True)
    if c.mode == "sharded":
        import torch
        from gpslam_amd import sharded
        s.set_stream(torch.cuda.current_stream().cuda_stream)
        send, recv = sharded.device_tensors(s)
        sv = sharded.ShardedSolver(s, send, recv, 0, 1, dist=None, landmark_buf=sharded.landmark_tensor(s))
        for it in range(3):
            op("phase.iterate%d" % it, lambda: np.array(list(sv.iterate().values())))
        op("phase.lm", lambda: np.array([float(v) for v in sv.iterate_lm(1e-3)[0].values()]))
        torch.cuda.synchronize()
    else:
        op("iterate_gn", lambda: stats_row(s.iterate_gn()[1]))
    if not c.only_gn:
        op("rows", lambda: {".%d" % i: a for i, a in enumerate(s.get_rows()) if a is not None})
        op("run_gn", lambda: stats_row(s.run_gn(4)[0]))
        op("error", lambda: np.array([s.error()]))
        op("after_gn", state)
        s.set_states(pose0, vel0)
        if lm0 is not None:
            s.set_landmarks(lm0)
        op("lm", lambda: (lambda r: np.concatenate([stats_row(r[1]), [r[2]]]))(s.iterate_lm(1e-10)))
        reject = s.default_params(use_lm=1, min_model_fidelity=2.0, relative_error_tol=0.0, lambda_upper_bound=1e2)
        op("lm_rejecting", lambda: (lambda r: np.concatenate([stats_row(r[1]), [r[2]]]))(s.iterate_lm(1e-3, reject)))
        for key, kind in MEAS_OF:
            if key in p and s.N == len(p["pose"]):      # (not behind marginalize_head: the head's factors are gone)
                op("weights.%d" % kind, lambda: s.meas_weights(kind, len(p[key])))
                op("linearize_meas.%d" % kind, lambda: dict(zip((".e", ".J"), s.linearize_meas(kind, len(p[key])))))
        if "closure_first" in p:
            op("closure_weights", lambda: s.between_pairs_weights(len(p["closure_first"])))
        op("marginals", lambda: (s.marginals(), {".%d" % i: a for i, a in enumerate(s.get_marginals(cross=s.L > 0 and c.name[:9] != "segmented")) if a is not None})[1])
        op("log_determinant", lambda: (lambda r: np.array([r[0], *r[1]]))(s.log_determinant(parts=True)))
        op("dogleg", lambda: (lambda r: np.concatenate([stats_row(r[0]), [r[1]]]))(s.iterate_dogleg(1.0)))
    op("final", state)
    rec["census"] = np.array(list(s.launch_census().values()))
    rec["refused"] = np.frombuffer("\n".join(log).encode(), dtype=np.uint8)
    s.close()
    return rec, log


SPLIT = (("split-2-pieces-pose2-2000", 0), ("split-2-pieces-fp32-pose2-2000", 1))


def run_split(gp, S, precision):
    """A chain split in two pieces held by this process (two handles; the interface records copied between them as the all-gather
    would): fs_split_info / fs_set_top, two Gauss-Newton iterations through fs_phase1 / fs_phase2 (k_fs_pack_record, then
    k_fs_top_build, the top system through the reduction's own kernels, k_fs_top_take and the backward half), one fs_lm_trial step
    that is kept and one that gpslam_hip_lm_reject takes back (k_fs_mask_mul in the trial's scalars)."""
    from gpslam_amd import sharded
    P = 2
    problem = S.pose2_local_landmarks_chain(2000, L=100, window=200)
    pieces, rec = [], {}
    for r in range(P):
        s = gp.ChainSolver(gp.POSE2, chart=gp.CHART_FIRST_ORDER, landmark_dim=2, precision=precision)
        sharded.apply_split(sharded.split_local_problem(problem, r, P), s, r, P)
        pieces.append(sharded.SplitSolver(s, r, P))
    nb_top = max(sv.nb_local for sv in pieces)
    for r, sv in enumerate(pieces):
        sv.set_top(nb_top)
        rec["split_info.%d" % r] = np.array(list(sv.backend.fs_split_info().values()))
        sv.backend.launch_census(reset=True)

    def exchange():
        for sv in pieces:
            rv = sv.recv.view(P, -1)
            for k in range(P):
                rv[k].copy_(pieces[k].send)

    def trial(lam):
        for sv in pieces:
            sv.backend.fs_lm_trial_phase1(lam)
        exchange()
        return np.stack([sv.backend.fs_lm_trial_phase2() for sv in pieces])

    for it in range(2):
        rec["iterate%d" % it] = np.array(list(sharded.iterate_pieces(pieces).values()))
    for sv in pieces:
        sv.backend.lm_begin()
    rec["trial_kept"] = trial(1e-3)
    for sv in pieces:
        sv.backend.lm_begin()
    rec["trial_rejected"] = trial(1e2)
    for sv in pieces:
        sv.backend.lm_reject()
    for r, sv in enumerate(pieces):
        rec["final.%d.pose" % r], rec["final.%d.vel" % r] = sv.backend.get_states()
        rec["final.%d.landmarks" % r] = sv.backend.get_landmarks()
        rec["census.%d" % r] = np.array(list(sv.backend.launch_census().values()))
        sv.backend.close()
    return {k: np.ascontiguousarray(v) for k, v in rec.items()}


def compare(a, b):
    fa, fb = (sorted(f for f in os.listdir(d) if f.endswith(".npz")) for d in (a, b))
    bad = 0
    if fa != fb:
        print("different sets of graphs:", sorted(set(fa) ^ set(fb)))
        bad += 1
    narr = 0
    for f in sorted(set(fa) & set(fb)):
        za, zb = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        if sorted(za.files) != sorted(zb.files):
            print("%s: different arrays: %s" % (f, sorted(set(za.files) ^ set(zb.files))))
            bad += 1
        diff = [k for k in set(za.files) & set(zb.files)
                if za[k].dtype != zb[k].dtype or za[k].shape != zb[k].shape or za[k].tobytes() != zb[k].tobytes()]
        narr += len(set(za.files) & set(zb.files))
        for k in sorted(diff):
            same_shape = za[k].shape == zb[k].shape and za[k].dtype.kind == "f"
            print("%s: %s differs%s" % (f, k, " (max |a - b| %.3g)" % np.nanmax(np.abs(za[k] - zb[k])) if same_shape else ""))
        bad += len(diff)
        print("%-44s %3d arrays %s" % (f, len(za.files), "equal" if not diff else "DIFFERENT"))
    print("%d graphs, %d arrays: %s" % (len(fa), narr, "EVERY BYTE EQUAL" if not bad else "%d DIFFERENCES" % bad))
    return 1 if bad else 0


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--compare":
        return compare(sys.argv[2], sys.argv[3])
    import torch  # noqa: F401
    import gpslam_amd as gp
    from gpslam_amd import synthetic as S
    out = sys.argv[1]
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
    os.makedirs(out, exist_ok=True)
    print("library:", os.environ.get("GPSLAM_LIB") or "the tree's own build")
    for c in cases(gp, S, "--fork" in sys.argv):
        if only not in c.name:
            continue
        rec, log = run_case(gp, S, c)
        np.savez(os.path.join(out, c.name + ".npz"), **rec)
        cen = dict(zip(gp.chain.CENSUS_KEYS, rec["census"]))
        lm = ["%s trials %d accepted %d" % (k, rec[k][7], rec[k][6]) for k in ("lm", "lm_rejecting") if k in rec]
        print("%-44s %3d arrays; census %s; %s%s" % (c.name, len(rec), {k: int(v) for k, v in cen.items() if v > 0 and k.startswith(("lin_", "flush", "gps_", "meas_", "retract"))},
                                                  "; ".join(lm), "".join("\n      refused: " + l for l in log)), flush=True)
    for name, precision in SPLIT:
        if only in name:
            rec = run_split(gp, S, precision)
            np.savez(os.path.join(out, name + ".npz"), **rec)
            print("%-44s %3d arrays; fat block, fat blocks, segment length, top block of piece 0: %s" % (name, len(rec), list(rec["split_info.0"])), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
