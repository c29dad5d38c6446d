#!/usr/bin/env python3
"""bench.py -- Gauss-Newton iterations over the BASELINE config-3 chain (Pose3 GP prior + synthetic odometry,
1e5 states per GPU, fp64) on N GPUs of one node.

  python bench.py --gpus 1 --steps 20 --warmup 3
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W
  python bench.py --gpus N ...                      (no launcher: the script starts torch.distributed.run itself)
  ... --total-states 1000000                        (strong scaling: ONE chain of that many states cut N ways)

One "step" = one full Gauss-Newton iteration of the hot path: linearise every factor (evaluateError + Jacobians),
assemble the block-tridiagonal normal equations, solve, retract, re-evaluate the error -- exactly what
matlab/PlazaPose2.m:224-226 brackets with tic/toc around optimizer.iterate().  Inputs are resident in HBM before
the timed region.  With N > 1 the ONE chain of N x 1e5 states is cut into N contiguous segments (weak scaling) and
every iteration performs one RCCL all-gather of the 3.6 KB interface records (gpslam_amd/sharded.py).  Rank 0 prints ONE
JSON line.

A plain run sets up, warms up, times the --steps iterations and prints the headline (metric, value, unit, ms_per_step,
dtype, ...) and nothing else.  --full adds everything measured beside it, all after the timed region: the convergence runs,
the per-kernel times and the roofline, the CPU baselines (--no-cpu-baseline skips them), the extras of a one-GPU run
(--no-extras skips them), and on more than one rank the collective, the projected sharded step and `strong_scaling`:
north_star's ONE chain of 1e6 states cut N ways (--strong-states).

  ... --dump-outputs DIR    after the timed steps: the states they produced (DIR/pose.npy, DIR/vel.npy: the ranks'
                            segments joined, in state order; DIR/state_index.npy names the states, a fixed seeded sample
                            where the whole chain would exceed 64 MB) and, on one GPU, the statistics of the last step
                            (DIR/stats.npy: error before, error after, |delta|_inf); float64 throughout
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
FP64_VECTOR_PEAK_TFLOPS = 78.6   # MI355X fp64 vector (= matrix) peak: 256 CUs x 4 SIMD-16 x 2 flop x 2.4 GHz (cdna_hip_programming.md: the SIMD-16 ceiling)
# k_fused_level0<1, double, 12, true>: (900 + 411) v_fmac_f64_dpp per block step of four states x 64 lanes x 2 flop / 4 states
FUSED_FMA_FLOPS_PER_STATE = (900 + 411) * 64 * 2 // 4

# rocprofv3 kernel names of the kernels bench.py times itself (time_kernel order); the per-launch HBM traffic of the
# same kernels on the same workload comes from the committed PMC passes (scripts/collect_profiles.sh ->
# profiles/<round>_pmc.json; explicit-size L2->fabric request counters TCC_EA0_RDREQ_{32B,64B,128B}, WRREQ{,_64B}).
PMC_FILE = os.path.join(ROOT, "profiles", "latest_pmc.json")
PMC_KEYS = [("k_gp<double, 3, 0",), ("k_assemble",), ("k_fused_level0", "k_chunk_forward_rows", "k_chunk_forward<double, 12, true>"),
            ("k_chunk_backward_rows<12>", "k_chunk_backward<double, 12"), ("k_retract<double, 3>",), ("k_lin<double, 3",)]
PMC_KLIN = 5
# K1 as it runs now (round 4: records, not rows) -- its own algorithmic bytes per state, stated in DESIGN.md section 6:
#   read  144 (state, each counted once) + 8 (dt) + 96 (BetweenFactor<Pose3> measured) + 48 (its sigmas)          = 296 B
#   write 640 (the 80-double GP record: Jr^-1, J, the finite-difference block, whitened error, coefficients)
#         + 384 (the 48-double between record)                                                                       = 1024 B
K1_RECORD_BYTES_PER_STATE = 296 + 1024
K1_GP_RECORD_BYTES_PER_STATE = 152 + 640           # the GP prior alone (gpslam_hip_time_kernel(0): k_gp)


def pmc_traffic(which, n_states):
    """HBM bytes per launch of kernel `which` from the committed counter passes, or None if they do not cover it.
    The solver kernels run once per hierarchy level; level 0 is the launch with the largest grid."""
    try:
        kern = json.load(open(PMC_FILE))["kernels"]
    except (OSError, ValueError, KeyError):
        return None
    best = None
    for k, c in kern.items():
        if k.startswith(PMC_KEYS[which]) and "ea_read_bytes" in c and c.get("states", n_states) == n_states:
            grid = int(k.rsplit("@", 1)[1])
            if best is None or grid > best[0]:
                best = (grid, float(c["ea_read_bytes"] + c["ea_write_bytes"]))
    return best[1] if best else None


def frac_or_none(bytes_, ms):
    """bytes / time as a fraction of the HBM peak, or None without a byte count"""
    return (bytes_ / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if (bytes_ and ms > 0) else None


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, pose, vel, stats):
    """--dump-outputs: the states after the timed steps (and the statistics of the last step) as float64 .npy files, so that
    two builds can be compared output for output.  A chain too large for DUMP_LIMIT_BYTES keeps a fixed, seeded sample of
    its states, the same for every run of the same size; state_index.npy names them."""
    os.makedirs(dirname, exist_ok=True)
    n = pose.shape[0]
    per_state = (pose.shape[1] + vel.shape[1] + 1) * 8          # + 1: the state's entry in state_index.npy
    keep = min(n, (DUMP_LIMIT_BYTES - 4096) // per_state)      # (4096: the .npy headers and stats.npy)
    idx = np.arange(n) if keep == n else np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
    arrays = {"pose": pose[idx], "vel": vel[idx], "state_index": idx}
    if stats is not None:
        arrays["stats"] = np.array([stats.error_before, stats.error_after, stats.delta_inf_norm])
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def cpu_baseline(problem, iters=3, threads=1):
    """The oracle (CPU restatement of the reference algorithm) timed on the same workload.  threads = 1: one core;
    threads = 0: the factor evaluation on every host core (OpenMP; what GTSAM with TBB parallelises), the elimination
    stays sequential (the elimination tree of a chain is a path)."""
    from oracle import oracle as O
    from gpslam_amd import synthetic as S
    used = O.set_threads(threads)
    ch = S.apply(problem, O.Chain(problem["kind"]))
    t0 = time.perf_counter()
    for _ in range(iters):
        rc, _st = ch.iterate_gn()
        assert rc == 0
    dt = time.perf_counter() - t0
    O.set_threads(1)
    return dict(value=problem["N"] * iters / dt, unit="state-iterations/s", cores=used, kind="port",
                sample="%d Gauss-Newton iterations of the full %d-state workload, oracle/liboracle.so (gcc -O2 -fopenmp, "
                       "%s), %.1f s" % (iters, problem["N"], "1 thread" if used == 1 else
                                        "factor evaluation on %d threads, serial solve: the elimination tree of a chain is a path" % used, dt),
                seconds_per_iteration=dt / iters)


def reference_baseline(problem):
    """the real gpslam factors on real GTSAM, if (and only if) both are installed where this
    runs.  They are in neither the build image nor on the GPU box, so this normally reports that, and never a number."""
    import shutil
    import struct
    import subprocess
    import tempfile
    src = os.path.join(ROOT, "bench", "gtsam_reference.cpp")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "gtsam_reference")
        cxx = shutil.which("g++")
        if cxx is None:
            return {"available": False, "why": "no host compiler"}
        r = subprocess.run([cxx, "-O3", "-std=c++11", src, "-o", exe, "-lgpslam", "-lgtsam", "-ltbb"], capture_output=True, text=True)
        if r.returncode != 0:
            r = subprocess.run([cxx, "-O3", "-std=c++11", src, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            return {"available": False, "why": "bench/gtsam_reference.cpp did not build"}
        pb = os.path.join(td, "problem.bin")
        p = problem
        with open(pb, "wb") as f:
            f.write(struct.pack("<qdd", p["N"], float(p["gp_dt"][0]), float(p["qc"][0, 0])))
            f.write(np.ascontiguousarray(np.concatenate([p["pose"], p["vel"]], axis=1)).tobytes())
            f.write(np.ascontiguousarray(p["between_meas"]).tobytes())
            f.write(struct.pack("<d", float(p["between_sig"][0, 0])))
            f.write(np.ascontiguousarray(p["prior_pose"][0]).tobytes())
            f.write(struct.pack("<d", float(p["prior_sig"][0, 0])))
        r = subprocess.run([exe, pb, "3"], capture_output=True, text=True)
        if r.returncode != 0:
            return {"available": False, "why": r.stdout.strip() or "reference binary failed"}
        return {"available": True, "kind": "reference", "runs": [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]}


def extras(gpslam_amd, S, device):
    """Driver-visible measurements beyond the headline line: the north-star 1e6-state run, the other BASELINE configs on one
    GPU (config 5 AT ITS SIZE, 1e6 states, fp32 and fp64), the per-rank cost of the 1e6-state chain cut 2 / 4 / 8 ways.
    Everything here runs AFTER the contract's timed region, on rank 0 of a single-GPU run only, and every section is
    guarded: a failure is recorded in its place and never takes the headline line down."""
    out = {}
    tols = [1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9]

    def converge(solver, use_lm, max_it=40):
        """iterations after which |delta|_inf first fell below each tolerance (None: never within max_it)"""
        first = {t: None for t in tols}
        lam, hist = 1e-5, []
        t0 = time.perf_counter()
        for it in range(1, max_it + 1):
            if use_lm:
                _rc, st, lam = solver.iterate_lm(lam)[:3]
                dlt = st.delta_inf_norm if st.accepted else float("inf")
            else:
                _rc, st = solver.iterate_gn()
                dlt = st.delta_inf_norm
            hist.append(dlt)
            for t in tols:
                if first[t] is None and dlt < t:
                    first[t] = it
            if dlt < tols[-1]:
                break
        return first, hist, time.perf_counter() - t0, st.error_after

    def section(name, fn):
        try:
            out[name] = fn()
        except Exception as e:      # an extra: never take the headline line down with it
            out[name] = {"failed": repr(e)}

    # ---- north star: 1e6 Pose3 GP states converged (|delta|_inf < 1e-6) on ONE GPU
    def north_star():
        p = S.pose3_chain(1000000)
        s = S.apply(p, gpslam_amd.ChainSolver(gpslam_amd.POSE3, device=device))
        first, hist, wall, err = converge(s, use_lm=False, max_it=15)
        s.set_states(p["pose"], p["vel"])
        s.run_gn(2)                                  # (untimed: the first launches behind a host-side pause run on idle clocks -- the fused launch 1.77 ms for 1.39 -- and an iteration costs the same wherever it starts)
        _st, ph = s.run_gn(5, timed=True)
        ms = float(ph[4]) / 5
        it6 = first[1e-6]
        s.set_level0_stamps(True)                    # (the launch's own dispatch stamps: a run of its own, see main())
        s.run_gn(5, timed=True)
        l0_ns = s.last_level0_ms() / 5
        s.set_level0_stamps(False)
        r = {"states": 1000000, "ms_per_iteration_device": ms,
             "phase_ms": {k: float(v) / 5 for k, v in zip(["linearize", "assemble", "solve", "retract+error", "total"], ph)},
             "level0_forward_ms_in_iteration": l0_ns,
             "iterations_to_delta_inf_below_1e-6": it6, "delta_inf_history": hist,
             "seconds_to_convergence_wall_incl_host_sync": wall,
             "seconds_to_convergence_device": (it6 * ms * 1e-3) if it6 else None,
             "states_converged_per_sec": (1000000 / (it6 * ms * 1e-3)) if it6 else None,
             "hbm_roofline_frac_whole_iteration": 7.8e3 * 1000000 / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
             # north_star's "batched-Jacobian kernel >= 50 % of HBM roofline" at THIS size, on the record-form bytes K1 moves
             # (296 B read + 1024 B written per state)
             "k1_frac_of_hbm_record_form": K1_RECORD_BYTES_PER_STATE * 1000000 / (float(ph[0]) / 5 * 1e-3) / 1e9 / HBM_PEAK_GBS,
             # ... and on SURVEY 8(d)'s own figure (2552 B per GP prior, "stays as stated"): the contract's reading
             "k1_frac_of_hbm_sec8d": S.algorithmic_bytes_per_state(S.POSE3)["linearize"] * 1000000 / (float(ph[0]) / 5 * 1e-3) / 1e9 / HBM_PEAK_GBS,
             "level0_frac_of_hbm_sec8d": 4800 * 1000000 / (l0_ns * 1e-3) / 1e9 / HBM_PEAK_GBS,
             "note": "target: >= 1e6 Pose3 GP states converged in < 1 s (BASELINE north_star names 8 GPUs; this is one)"}
        s.close()
        return r
    section("north_star_1e6_pose3_1gpu", north_star)

    # ---- the 1e6-state chain cut P ways: what ONE rank of a P-GPU run does per iteration (forced sharded code path on this
    # GPU, the all-gather of the P interface records replaced by a device copy), so that the first real multi-GPU run has a
    # prediction to be checked against
    def projected():
        import torch
        from gpslam_amd import sharded
        p = S.pose3_chain(1000000)
        res = {"total_states": 1000000, "note": "per-rank device + launch time of the sharded code path without its collective; the "
               "collective is one all-gather of a 3.6 KB record per rank (latency-sized)", "ranks": {}}
        for P in (2, 4, 8):
            lp = sharded.local_problem(p, 0, P)             # rank 0's segment (every rank holds N / P states)
            sv_ = gpslam_amd.ChainSolver(gpslam_amd.POSE3, device=device, rank=0, nranks=P)
            sv_.set_stream(torch.cuda.current_stream().cuda_stream)
            sharded.apply_local(lp, sv_)
            send, recv = sharded.device_tensors(sv_)
            rv = recv.view(P, -1)

            def one():
                sv_.iterate_phase1(0.0)
                for k in range(P):                          # stand-in for the all-gather: every slot gets this rank's record
                    rv[k].copy_(send)
                sv_.iterate_phase2(False)
            for _ in range(3):
                one()
            sv_.set_states(lp["pose"], lp["vel"])
            if "halo_pose" in lp:
                sv_.set_halo_state(lp["halo_pose"], lp["halo_vel"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                one()
            torch.cuda.synchronize()
            res["ranks"][str(P)] = {"states_per_rank": int(lp["N"]), "ms_per_rank_and_iteration": (time.perf_counter() - t0) / 20 * 1e3,
                                    "record_bytes": int(send.numel() * send.element_size())}
            sv_.close()
        return res
    section("projected_sharded_1e6_pose3", projected)

    # ---- config 1 (the reference's own CPU-runnable case: matlab/PlazaPose2.m on the Plaza2 log -- 4091 SE(2) states, 1816 interpolated
    # ranges, 4 landmarks; tests/golden/plaza2.npz): wall clock per iteration of the reference's optimiser calls
    def config1():
        from gpslam_amd import plaza
        data = plaza.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "plaza2.npz"))
        p = plaza.build_problem(data)
        s = plaza.apply(p, gpslam_amd.ChainSolver(gpslam_amd.POSE2, chart=gpslam_amd.CHART_FIRST_ORDER, landmark_dim=2, device=device))
        s.run_gn(3)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            s.run_gn(50)
            dt = (time.perf_counter() - t0) / 50 * 1e3
            best = dt if best is None else min(best, dt)
        lam = 1e-5
        t0 = time.perf_counter()
        for _ in range(20):
            _rc, _st, lam = s.iterate_lm(lam)
        lm_ms = (time.perf_counter() - t0) / 20 * 1e3
        s.close()
        return {"states": int(len(p["pose"])), "ms_per_gauss_newton_iteration_wall": best, "ms_per_lm_iterate_call_wall": lm_ms,
                "note": "run_gn(50) / 20 iterate_lm calls on the recipe's graph; accuracy against ground truth: tests/test_plaza.py"}
    section("config1_plaza2_4091_pose2", config1)

    # ---- config 2 (linear GP chain) and config 4 (1e6 SE(2) poses + 5e4 locally visible range landmarks), one GPU
    def config2():
        p = S.linear_chain(100000)
        s = S.apply(p, gpslam_amd.ChainSolver(p["kind"], device=device))
        s.run_gn(2)
        _st, ph = s.run_gn(5, timed=True)
        s.close()
        return {"ms_per_iteration_device": float(ph[4]) / 5, "state_iterations_per_sec": 100000 / (float(ph[4]) / 5 * 1e-3)}
    section("config2_linear3_1e5", config2)

    def config4():
        p = S.pose2_local_landmarks_chain(1000000)
        s = S.apply(p, gpslam_amd.ChainSolver(p["kind"], chart=gpslam_amd.CHART_FIRST_ORDER, landmark_dim=2, device=device))
        first, hist, wall, err = converge(s, use_lm=False, max_it=15)
        s.set_states(p["pose"], p["vel"])
        s.set_landmarks(p["landmarks"])
        s.run_gn(2)                                  # (untimed, as in north_star)
        _st, ph = s.run_gn(3, timed=True)
        ms = float(ph[4]) / 3
        r = {"states": 1000000, "landmarks": len(p["landmarks"]), "range_factors": len(p["range_left"]), "plan": s.segment_plan(),
             "ms_per_iteration_device": ms, "phase_ms": {k: float(v) / 3 for k, v in zip(["linearize", "assemble", "solve", "retract+error", "total"], ph)},
             "iterations_to_delta_inf_below_1e-6": first[1e-6], "seconds_to_convergence_wall_incl_host_sync": wall,
             "state_iterations_per_sec": 1000000 / (ms * 1e-3),
             "landmark_elimination": "segments + fat separators, segment Schur complements on v_mfma_f64_16x16x4_f64 (fatsep.hpp)"}
        s.close()
        # the same graph across GPUs = pieces joined at shared fat separators (gpslam_amd/sharded.py: SplitSolver).  Here both
        # pieces of a 2-way cut live on this one GPU and run one after the other: per-rank work of a 2-GPU run without its
        # all-gather (2 records of ~40 KB).
        try:
            import torch
            from gpslam_amd import sharded
            pieces, locals_ = [], []
            for rk in range(2):
                lp = sharded.split_local_problem(p, rk, 2)
                sp = gpslam_amd.ChainSolver(p["kind"], chart=gpslam_amd.CHART_FIRST_ORDER, landmark_dim=2, device=device)
                sharded.apply_split(lp, sp, rk, 2)
                locals_.append(lp)
                pieces.append(sharded.SplitSolver(sp, rk, 2))
            nb_top = max(sv.nb_local for sv in pieces)
            for sv in pieces:
                sv.set_top(nb_top)
            hist2 = [sharded.iterate_pieces(pieces) for _ in range(2)]
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(3):
                for sv in pieces:
                    sv.backend.fs_phase1(0.0)
                for sv in pieces:
                    rv = sv.recv.view(2, -1)
                    for k in range(2):
                        rv[k].copy_(pieces[k].send)
                for sv in pieces:
                    sv.backend.fs_phase2(False)
            ev1.record()
            torch.cuda.synchronize()
            r["split_in_2_pieces_on_this_gpu"] = {
                "ms_per_rank_and_iteration": ev0.elapsed_time(ev1) / 3 / 2, "states_per_piece": [lp["N"] for lp in locals_],
                "interface_record_bytes": int(pieces[0].send.numel() * 8), "error_after_2_iterations": hist2[-1]["error_after"],
                "note": "unsplit: ms_per_iteration_device above (1e6 states on one GPU); a piece holds 5e5"}
            for sv in pieces:
                sv.backend.close()
        except Exception as e:
            r["split_in_2_pieces_on_this_gpu"] = {"failed": repr(e)}
        return r
    section("config4_pose2_1e6_landmarks_5e4_1gpu", config4)

    # ---- config 5 AT ITS SIZE (1e6 states): fp32 vs fp64 tolerance sweep.  fp32 = fp32 Jacobian rows (the dominant HBM traffic)
    # + fp64 residual, normal equations and solver: the update cannot fall below cond(H) * eps32 * |whitened
    # residual|, so each mix has a tolerance below which the fp32 handle never gets; above it both take the same iterations.
    def config5():
        sweep = {}
        for name, make, kind in (("rot3_gp_prior+interp_attitude_x4_(acc+mag)_1e6", lambda: S.rot3_attitude_chain(1000000, refs=2), gpslam_amd.ROT3),
                                 ("pose3_gp_prior+odometry+interp_gps_x4_1e6", lambda: S.pose3_gps_chain(1000000, keep_odometry=True), gpslam_amd.POSE3)):
            p = make()
            res = {"states": 1000000}
            finals = {}
            for prec_name, prec in (("fp64", gpslam_amd.FP64), ("fp32", gpslam_amd.FP32)):
                s = S.apply(p, gpslam_amd.ChainSolver(kind, device=device, precision=prec))
                first, hist, wall, err = converge(s, use_lm=False, max_it=16)
                finals[prec_name] = s.get_states()
                s.set_states(p["pose"], p["vel"])
                s.run_gn(2)                          # (untimed, as in north_star)
                _st, ph = s.run_gn(3, timed=True)
                res[prec_name] = {"gn_iterations_to_delta_inf_below": {("%.0e" % t): first[t] for t in tols},
                                  "final_error": err, "delta_inf_floor": min(hist), "iterations_run": len(hist),
                                  "ms_per_iteration_device": float(ph[4]) / 3,
                                  "phase_ms": {k: float(v) / 3 for k, v in zip(["linearize", "assemble", "solve", "retract+error", "total"], ph)}}
                s.close()
            (x64, v64), (x32, v32) = finals["fp64"], finals["fp32"]
            scale = max(1.0, float(np.abs(x64).max()), float(np.abs(v64).max()))
            res["fp32_vs_fp64_final_state_rel_diff"] = float(max(np.abs(x64 - x32).max(), np.abs(v64 - v32).max()) / scale)
            # say what the fp32 handle is.  Its row tables are plain fp32 Jacobian rows; the structured records that
            # make the fp64 path fast are fp64-only, so fp32 is the SLOWER of the two on every mix: a tolerance mode, never a throughput mode
            res["fp32_is"] = "tolerance mode only (north_star's 1e-5-relative sweep); slower than fp64 per iteration: %.2f x" % (
                res["fp32"]["ms_per_iteration_device"] / max(res["fp64"]["ms_per_iteration_device"], 1e-12))
            sweep[name] = res
        return sweep
    section("config5_fp32_vs_fp64_tolerance_sweep_1e6", config5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--states", type=int, default=100000, help="states per GPU (BASELINE config 3: 100k poses)")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beside the headline too (convergence, roofline, baselines, extras); a plain run times the steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed steps computed (the states, the last step's statistics) to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the beyond-the-headline measurements (profiling runs)")
    ap.add_argument("--total-states", type=int, default=0,
                    help="strong scaling: ONE chain of this many states cut into --gpus segments (the headline then says \"scaling\": \"strong\")")
    ap.add_argument("--strong-states", type=int, default=1000000,
                    help="multi-rank runs also time north_star's chain of this many states cut --gpus ways, after the timed region (0: skip)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started without a launcher: become `python -m torch.distributed.run --nproc-per-node N bench.py <same arguments>`, one
        # process per GPU over RCCL (a bare `python bench.py --gpus 8` must yield a line, not an exit code)
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.stdout.flush()
        os.execv(sys.executable, cmd)

    import torch
    import gpslam_amd
    from gpslam_amd import sharded, synthetic as S

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # GPSLAM_BENCH_BACKEND=segment_model (tests/test_bench_world_cpu.py only): the two phases of a rank are played by the
    # numpy + oracle model of tests/segment_model.py over gloo, so that THIS file's world > 1 control flow -- partitioning,
    # the one all-gather per iteration, barriers, max over ranks, the JSON line -- runs end to end on a machine without GPUs.
    # Nothing measured that way is a benchmark result: the line says "data": "model" and carries no roofline.
    model = os.environ.get("GPSLAM_BENCH_BACKEND", "hip") == "segment_model"
    if model and world == 1:
        raise SystemExit("the segment_model backend exists for the world > 1 control flow only")
    if not model:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
        torch.cuda.set_device(local_rank)
    dev = "cpu" if model else "cuda"
    dist = None
    if world > 1:
        import torch.distributed as dist
        if model:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        # one process per GPU over RCCL, exactly as many as asked for
        assert dist.get_world_size() == world == args.gpus, (dist.get_world_size(), world, args.gpus)
    elif args.gpus != 1:
        raise SystemExit("bench.py --gpus %d: launch with python -m torch.distributed.run --nproc-per-node %d (WORLD_SIZE is 1)" % (args.gpus, args.gpus))

    def device_sync():
        if not model:
            torch.cuda.synchronize()

    def barrier():
        if dist is not None:
            dist.barrier()
        device_sync()

    strong = args.total_states > 0
    if strong:
        total_states = args.total_states
        N = (total_states + world - 1) // world        # states per GPU (the segments differ by at most one state)
    else:
        N = args.states
        total_states = N * world

    def setup(total):
        """ONE Pose3 chain of `total` states on this run's ranks: world == 1: the unsharded handle; world > 1: contiguous
        segments, one all-gather of the interface records per iteration.  Returns the closures the measurements below use."""
        w = {}
        if world == 1:
            problem = S.pose3_chain(total)
            solver = S.apply(problem, gpslam_amd.ChainSolver(gpslam_amd.POSE3, device=local_rank))

            def reset():
                solver.set_states(problem["pose"], problem["vel"])

            def one_with_stats():
                _rc, st = solver.iterate_gn()
                return st.error_after, st.delta_inf_norm

            def run(k):
                return solver.run_gn(k)[0]
            w.update(problem=problem, solver=solver, sv=None, send=None, recv=None, lp=None)
        else:
            problem = S.pose3_chain(total)                  # ONE chain, cut into `world` contiguous segments
            lp = sharded.local_problem(problem, rank, world)
            if model:
                tests_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests")
                if tests_dir not in sys.path:
                    sys.path.insert(0, tests_dir)
                from segment_model import SegmentModel
                solver = sharded.apply_local(lp, SegmentModel(S.POSE3, rank, world))
                send, recv = solver.send, solver.recv
            else:
                solver = gpslam_amd.ChainSolver(gpslam_amd.POSE3, device=local_rank, rank=rank, nranks=world)
                solver.set_stream(torch.cuda.current_stream().cuda_stream)   # order kernels against the RCCL collective
                sharded.apply_local(lp, solver)
                send, recv = sharded.device_tensors(solver)
            sv = sharded.ShardedSolver(solver, send, recv, rank, world, dist=dist)

            def reset():
                solver.set_states(lp["pose"], lp["vel"])
                if "halo_pose" in lp:
                    solver.set_halo_state(lp["halo_pose"], lp["halo_vel"])

            def one_with_stats():
                st = sv.iterate()
                return st["error_after"], st["delta_inf_norm"]

            def run(k):
                for _ in range(k):
                    sv.iterate(want_stats=False)
            w.update(problem=problem, solver=solver, sv=sv, send=send, recv=recv, lp=lp)
        w.update(reset=reset, one_with_stats=one_with_stats, run=run)
        return w

    def timed(fn):
        """wall clock of fn() between barriers (+ device syncs), the maximum over the ranks"""
        barrier()
        t0 = time.perf_counter()
        fn()
        barrier()
        dt = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    W = setup(total_states)
    problem, solver, sv, send, recv, lp = W["problem"], W["solver"], W["sv"], W["send"], W["recv"], W["lp"]
    reset, one_with_stats, run = W["reset"], W["one_with_stats"], W["run"]

    # --full: convergence run (outside the contract clock): iterations until |delta|_inf < 1e-6
    conv_iters, conv_delta, final_error = 0, float("inf"), float("nan")
    if args.full:
        for _ in range(25):
            final_error, conv_delta = one_with_stats()
            conv_iters += 1
            if conv_delta < 1e-6:
                break

    # timed region: restart from the initial values so the steps do real Newton work
    reset()
    if args.warmup > 0:
        run(args.warmup)
    reset()
    barrier()
    t0 = time.perf_counter()
    last_stats = run(args.steps)
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # what the timed steps computed, before anything below moves the states again; the ranks' segments are contiguous, in rank order
    if args.dump_outputs:
        pose_out, vel_out = solver.get_states()
        if dist is not None:
            parts = [None] * world
            dist.all_gather_object(parts, (pose_out, vel_out))
            pose_out, vel_out = np.concatenate([pp for pp, _ in parts]), np.concatenate([vv for _, vv in parts])
        if rank == 0:
            dump_outputs(args.dump_outputs, pose_out, vel_out, last_stats)

    # --full: a TIMED convergence run (outside the contract clock; VERDICT r2: the headline's states-to-convergence figure was
    # derived from ms_per_step): from the initial values, the iterations the convergence run above needed, wall clock between barriers
    conv_seconds = None
    if args.full:
        reset()
        barrier()
        tc0 = time.perf_counter()
        run(conv_iters)
        barrier()
        conv_seconds = time.perf_counter() - tc0
        if dist is not None:
            t = torch.tensor([conv_seconds], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            conv_seconds = float(t.item())

    # N > 1 (--full): what the one data-path collective of an iteration costs (all ranks take part; outside the contract clock):
    # device time of `reps` all-gathers of the 3.6 KB interface records between events on the stream RCCL is ordered against
    collective_ms = None
    if world > 1 and args.full:
        reps = 50
        for _ in range(5):
            sv.exchange()
        barrier()
        if model:
            tm0 = time.perf_counter()
            for _ in range(reps):
                sv.exchange()
            local_ms = (time.perf_counter() - tm0) / reps * 1e3
        else:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                sv.exchange()
            e1.record()
            torch.cuda.synchronize()
            local_ms = e0.elapsed_time(e1) / reps
        tc = torch.tensor([local_ms], dtype=torch.float64, device=dev)
        dist.all_reduce(tc, op=dist.ReduceOp.MAX)      # (every rank executes exactly the same sequence of collectives)
        collective_ms = float(tc.item())

    # N > 1 (--full): the prediction this run is checked against -- what THIS rank's share of the sharded code path
    # costs per iteration when the all-gather is replaced by a device copy of its own record into every slot (the figure
    # `extras.projected_sharded_1e6_pose3` of the one-GPU run, for this run's segment); measured on every rank after the timed
    # region, reported as the maximum over the ranks
    projected_ms = None
    if world > 1 and not model and args.full:
        # (never allowed to cost the run its line: this branch has only ever executed on the gloo model and on one GPU; a failure
        #  of the local measurement is reported as such, and every rank still takes part in the one collective below)
        local_ms, projected_err = float("nan"), None
        try:
            rv = recv.view(world, -1)

            def one_local():
                solver.iterate_phase1(0.0)
                for k in range(world):
                    rv[k].copy_(send)
                solver.iterate_phase2(False)
            reset()
            for _ in range(3):
                one_local()
            reset()
            device_sync()
            tp0 = time.perf_counter()
            for _ in range(args.steps):
                one_local()
            device_sync()
            local_ms = (time.perf_counter() - tp0) / args.steps * 1e3
        except Exception as ex:     # noqa: BLE001
            projected_err = repr(ex)
        tp = torch.tensor([local_ms if local_ms == local_ms else -1.0], dtype=torch.float64, device=dev)
        dist.all_reduce(tp, op=dist.ReduceOp.MAX)
        projected_ms = float(tp.item()) if projected_err is None and float(tp.item()) > 0 else None

    # --full, N > 1 (and the one-GPU run unless --no-extras): north_star's STRONG-scaling point -- ONE chain of --strong-states (1e6)
    # Pose3 states cut `world` ways: iterations to |delta|_inf < 1e-6, wall clock of exactly that many iterations from the
    # initial values, and ms per iteration over `steps` iterations; every rank takes part, all of it outside the contract clock.
    strong_block = None
    want_strong = args.full and args.strong_states > 0 and not strong and (world > 1 or not (args.no_extras or model))
    if want_strong:
        Ws = setup(args.strong_states)            # (the headline's handle stays: the roofline probes below use it)
        it_s, dl_s = 0, float("inf")
        for _ in range(25):
            _e, dl_s = Ws["one_with_stats"]()
            it_s += 1
            if dl_s < 1e-6:
                break
        Ws["reset"]()
        conv_s = timed(lambda: Ws["run"](it_s))
        Ws["reset"]()
        Ws["run"](min(args.warmup, 3))
        Ws["reset"]()
        steps_s = max(1, min(args.steps, 20))
        el_s = timed(lambda: Ws["run"](steps_s))
        strong_block = {"scaling": "strong", "total_states": args.strong_states, "n_gpus": world,
                        "states_per_gpu": (args.strong_states + world - 1) // world,
                        "ms_per_iteration": el_s / steps_s * 1e3, "steps": steps_s,
                        "state_iterations_per_sec": args.strong_states * steps_s / el_s,
                        "iters_to_convergence": it_s, "delta_inf_at_convergence": dl_s, "seconds_to_convergence": conv_s,
                        "states_converged_per_sec": args.strong_states / conv_s,
                        "north_star_target": "1e6 Pose3 GP states converged (|delta|_inf < 1e-6) in < 1 s on 8 GPUs",
                        "note": "wall clock between barriers, maximum over the ranks; ONE chain cut into %d contiguous segments, one "
                                "all-gather of the interface records per iteration" % world if world > 1 else
                                "wall clock between device syncs on one GPU (the same chain as extras.north_star_1e6_pose3_1gpu)"}
        if not model:
            Ws["solver"].close()
        del Ws

    ms_per_step = elapsed / args.steps * 1e3
    if rank == 0 and model:
        # the control-flow run of the CPU test: the line a real run prints, without what only a GPU can measure
        line = {
            "metric": "GN state-iterations/sec (states x Gauss-Newton iters/sec), Pose3 GP chain",
            "value": total_states * args.steps / elapsed, "unit": "state-iterations/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong" if strong else "weak",
            "vs_baseline": None, "dtype": "f64", "data": "model",
            "config": {"workload": "control-flow test: %d poses per rank, numpy + oracle model of the two phases over gloo" % N,
                       "states_per_gpu": N, "total_states": total_states,
                       "parallelism": "1 chain in %d contiguous segments, 1 all-gather of interface records per iteration" % world},
            "ranks": world, "rccl_version": None}
        if args.full:
            line.update({
                "iters_to_convergence": conv_iters, "delta_inf_at_convergence": conv_delta,
                "final_error": final_error, "seconds_to_convergence": conv_seconds,
                "collective": {"kind": "all_gather of the interface records (gloo)", "bytes_per_rank": int(send.numel() * send.element_size()),
                               "ms_per_iteration": collective_ms, "share_of_step": collective_ms / ms_per_step},
                "strong_scaling": strong_block, "roofline": None, "cpu_baseline": None})
        print(json.dumps(line))
    if rank == 0 and not model:
        try:
            rccl = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            rccl = None
        head = {
            "metric": "GN state-iterations/sec (states x Gauss-Newton iters/sec), Pose3 GP chain",
            "value": total_states * args.steps / elapsed,
            "unit": "state-iterations/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong" if strong else "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": "BASELINE configs[2]: Pose3/SE(3) GP prior + synthetic odometry, "
                                   "%d poses per GPU, fp64, Gauss-Newton" % N,
                       "states_per_gpu": N, "total_states": total_states,
                       "factors": "N-1 GaussianProcessPriorPose3 + N-1 BetweenFactor<Pose3> + 1 PriorFactor<Pose3>",
                       "parallelism": "1 chain in %d contiguous segments, 1 all-gather of interface records per "
                                      "iteration" % world if world > 1 else "single GPU"},
            "ranks": world, "rccl_version": rccl,
            "gn_iters_per_sec": args.steps / elapsed}
        if not args.full:
            print(json.dumps(head))
    if rank == 0 and not model and args.full:
        # per-kernel device time (hipEvents on the handle's stream) of the per-GPU workload, for the roofline
        if world == 1:
            probe, pproblem = solver, problem
        else:
            pproblem = S.pose3_chain(N)
            probe = S.apply(pproblem, gpslam_amd.ChainSolver(gpslam_amd.POSE3, device=local_rank))
        names = ["k_gp (K1 linearise GP priors)", "k_assemble (K3)", "k_chunk_forward level 0 (K4)",
                 "k_chunk_backward level 0 (K4)", "k_retract (K6)"]
        kms = [probe.time_kernel(w, reps=5) for w in range(5)]
        ab = S.algorithmic_bytes_per_state(S.POSE3)
        blocks = ab["linearize"] - (18 * 8 + 8)
        fused = (kms[1] == 0.0)                    # the assembly runs inside the level-0 elimination (k_fused_level0)
        if fused:
            names[2] = "k_fused_level0 (K3 + K4 level 0: assembly + elimination)"
        sec8d_k1 = ab["linearize"] * (N - 1)       # read state + dt, write the materialised e + H1..H4 (2552 B per factor)
        alg = [K1_GP_RECORD_BYTES_PER_STATE * (N - 1),   # K1 as it is: read state + dt, write the 80-double record (the Jacobian rows are never written)
               (blocks + blocks) * N,              # K3: read rows, write blocks
               # K4 forward: SURVEY 8(d) single-pass solve figure (conservative); fused: read the rows, write the factors
               (blocks + blocks if fused else ab["solve"]) * N,
               (blocks + 12 * 8) * N,              # back-substitution: read factors, write delta
               ab["retract"] * N]
        live = [i for i in range(5) if not (fused and i == 1)]    # no k_assemble launch exists when the assembly is fused
        dom = live[int(np.argmax([kms[i] for i in live]))]
        achieved = alg[dom] / (kms[dom] * 1e-3) / 1e9
        probe.run_gn(2)
        _st, phase = probe.run_gn(6, timed=True)
        phase = phase / 2                               # (the keys below divide by 3, as before)
        # the level-0 forward launch as it runs INSIDE an iteration, from its own dispatch stamps (a second run: a stamped dispatch
        # costs the iteration ~10 us elsewhere, so the phase times above come from the run without them)
        probe.set_level0_stamps(True)
        probe.run_gn(6, timed=True)
        l0_in_iter = probe.last_level0_ms() / 6
        probe.set_level0_stamps(False)
        if dom == 2 and l0_in_iter > 0:
            achieved = alg[dom] / (l0_in_iter * 1e-3) / 1e9
        out = {
            **head,
            "iters_to_convergence": conv_iters,
            "delta_inf_at_convergence": conv_delta,
            "final_error": final_error,
            "seconds_to_convergence": conv_seconds,
            "states_to_convergence_per_sec": total_states / conv_seconds,
            "states_to_convergence_per_sec_note": "timed: %d Gauss-Newton iterations from the initial values to |delta|_inf < 1e-6, wall clock between barriers" % conv_iters,
            "phase_ms_per_iter_1gpu": {k: float(v) / 3 for k, v in
                                       zip(["linearize", "assemble", "solve", "retract+error", "total"], phase)},
            "kernel_ms": {names[i]: float(kms[i]) for i in live},
            # every hot kernel against the same roof: algorithmic GB/s (SURVEY 8(d) bytes per unit) and, where the
            # committed counter passes cover it, the HBM bytes it really moved per launch
            "kernel_roofline": {n: {"algorithmic_bytes_per_launch": alg[i],
                                    "algorithmic_GBps": alg[i] / (kms[i] * 1e-3) / 1e9,
                                    "frac_of_peak": alg[i] / (kms[i] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                    "moved_bytes_per_launch": pmc_traffic(i, N),
                                    "moved_GBps": (pmc_traffic(i, N) / (kms[i] * 1e-3) / 1e9) if pmc_traffic(i, N) else None,
                                    "frac_moved": frac_or_none(pmc_traffic(i, N), kms[i])}
                                for i, n in enumerate(names) if i in live},
            "roofline": {"bound": "hbm", "kernel": names[dom], "achieved": achieved, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": pmc_traffic(dom, N),
                         # the same launch on the bytes the counters saw it move (below the SURVEY 8(d) figure: records instead of rows)
                         "frac_moved": frac_or_none(pmc_traffic(dom, N), l0_in_iter if (dom == 2 and l0_in_iter > 0) else kms[dom]),
                         "traffic_source": "rocprofv3 --pmc TCC_EA0_RDREQ_{32B,64B,128B}_sum / TCC_EA0_WRREQ{,_64B}_sum, "
                                           "profiles/latest_pmc.json (bytes per launch, same workload)",
                         "algorithmic_bytes_per_launch": alg[dom],
                         "avg_launch_ms": l0_in_iter if (dom == 2 and l0_in_iter > 0) else kms[dom],
                         "timing": ("the launch's own start / stop HIP events (hipExtLaunchKernelGGL: the dispatch's time stamps, as in rocprofv3's "
                                    "kernel trace) INSIDE 6 consecutive Gauss-Newton iterations (gpslam_hip_last_level0_ms); the "
                                    "isolated launches of kernel_ms run on other cache contents" if (dom == 2 and l0_in_iter > 0) else "isolated launches (time_kernel)"),
                         # what actually limits the kernel the HBM fraction is quoted for: the second roof
                         "valu_fp64": ({"achieved": FUSED_FMA_FLOPS_PER_STATE * N / ((l0_in_iter if l0_in_iter > 0 else kms[dom]) * 1e-3) / 1e12,
                                        "peak": FP64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s",
                                        "frac": FUSED_FMA_FLOPS_PER_STATE * N / ((l0_in_iter if l0_in_iter > 0 else kms[dom]) * 1e-3) / 1e12 / FP64_VECTOR_PEAK_TFLOPS,
                                        "flops_per_state_issued": FUSED_FMA_FLOPS_PER_STATE,
                                        "note": "ISSUED fp64 multiply-adds: v_fmac_f64_dpp wave instructions per block step of four states in the ISA of "
                                                "the shipped kernel (elimination wave 900, assembly wave 411 with a diagonal Qc) x 64 lanes x 2 / 4; "
                                                "12 of a DPP row's 16 lanes carry matrix rows, and the two waves issue another ~830 non-FMA "
                                                "instructions per step through the same port"}
                                       if fused and dom == 2 else None),
                         "note": ("VALU-issue bound next to the HBM roof (DESIGN.md section 4 'Round 4'): two-wave workgroups (assembly + "
                                  "elimination), ~2140 wave instructions per workgroup block step, SIMDs ~88 % busy (SQ_ACTIVE_INST_ANY of two resident "
                                  "waves); measured traffic is below the SURVEY 8(d) figure because the GP priors arrive as "
                                  "80-double records of Jr^-1, J and the finite-difference block (312 doubles as rows) whose columns the "
                                  "assembly wave forms; the launch also reduces its four chunk separators"
                                  if fused and dom == 2 else None)},
        }
        # K1 (batched evaluateError + Jacobians of the GP priors) standalone and inside an iteration, where it shares the
        # launch (k_lin) with the prior and between factors
        lin_ms = float(phase[0]) / 3
        k1_bytes = K1_RECORD_BYTES_PER_STATE * (N - 1)
        k1_moved = pmc_traffic(PMC_KLIN, N)
        frac_sec8d = sec8d_k1 / (lin_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
        frac_record = k1_bytes / (lin_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
        out["k1_batched_jacobian"] = {
            "standalone_ms": float(kms[0]),
            "standalone_frac_of_hbm": alg[0] / (kms[0] * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "in_iteration_linearize_phase_ms": lin_ms,
            # north_star: "the batched-Jacobian kernel at >= 50 % of HBM roofline".  Three readings of the same launch, all printed
            # (VERDICT r5 item 7): the contract's (2552 B per GP prior, "the algorithmic figure stays as stated" whatever
            # the kernel really writes), the record form the kernel moves by design, and what the counters saw.
            "frac_sec8d": frac_sec8d,
            "frac_sec8d_bytes_per_gp_prior": ab["linearize"],
            "frac_sec8d_incl_between_factors": (sec8d_k1 + (2 * 96 + 6 * 104) * (N - 1)) / (lin_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "frac_record_form": frac_record,
            "record_form_bytes_per_state": K1_RECORD_BYTES_PER_STATE,
            "frac_moved": frac_or_none(k1_moved, lin_ms),
            "moved_bytes": k1_moved,
            "north_star_k1_at_least_half_of_hbm": bool(frac_sec8d >= 0.5),
            "north_star_k1_at_least_half_of_hbm_on_record_form": bool(frac_record >= 0.5),
            "north_star_k1_at_least_half_of_hbm_on_moved_bytes": (bool(frac_or_none(k1_moved, lin_ms) >= 0.5) if k1_moved else None),
            "sec8d_note": "SURVEY 8(d) prices K1 at 2552 B per GP prior (+ 816 B per between factor) for the API-faithful materialised e + H1..H4 and "
                          "says the figure stays as stated when symmetry / constant blocks lower the real traffic; since round 4 K1 writes 80- and "
                          "48-double records (what the Jacobian is a function of) and the assembly wave of the next launch forms the columns, so "
                          "frac_sec8d is the contract's reading, frac_record_form / frac_moved what the launch does to HBM",
            "note": ""}
        if strong_block is not None:
            out["strong_scaling"] = strong_block
        if collective_ms is not None:
            out["collective"] = {"kind": "ncclAllGather of the interface records (RCCL), one per iteration", "bytes_per_rank": int(send.numel() * send.element_size()),
                                 "ms_per_iteration": collective_ms, "share_of_step": collective_ms / ms_per_step}
        if projected_ms is not None:
            out["projected_sharded"] = {"ms_per_rank_and_iteration_without_collective": projected_ms,
                                        "measured_ms_per_step": ms_per_step, "measured_over_projected": ms_per_step / projected_ms,
                                        "note": "the same two phases per rank with the all-gather replaced by device copies of the rank's own "
                                                "record (max over ranks): measured - projected = what the collective and the rank skew cost"}
        out["k1_batched_jacobian"]["note"] = ("in-iteration = k_lin: GP priors + priors + between factors in one launch; fractions are on the RECORD-form "
                                              "bytes (read 296 B, write 1024 B per state: DESIGN.md section 6) and on the counter traffic of "
                                              "profiles/latest_pmc.json; standalone = the GP priors alone (k_gp, 152 + 640 B)")
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(problem, threads=1)
            out["cpu_baseline_all_cores"] = cpu_baseline(problem, threads=0)     # (factor evaluation on every thread, SERIAL solve)
            out["reference_gtsam_baseline"] = reference_baseline(problem)
        if world == 1 and not args.no_extras:
            out["extras"] = extras(gpslam_amd, S, local_rank)
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
