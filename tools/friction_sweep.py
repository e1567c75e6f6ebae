"""Developer tool (GPU box): what the three control pipelines do on a slippery floor (``friction_model``, include/mpc_sim_friction.h), as one
measured sweep: 64 robots per run, one robot per Coulomb coefficient, geometric from 0.02 to 1.5 and the last robot on mu = +inf (the ground every
earlier sweep stood on).  ``mu_spin = 0.05 m * mu`` (a contact patch of that effective radius).  The controllers keep their own cones (mu = 0.8 in the MPC
stages and the low-level QPs); only the simulated plant slips.  Two experiments per formulation, on the unilateral contact rule:

  walk   the script's walking schedule
  push   the same with the scripts' push (``pipeline.push_schedule``: MPC ticks 160 - 170, the script's force at the world origin)

  kinodynamic   KinodynamicPipeline, device loop (mpc_qp_low_level_steps)
  centroidal    CentroidalPipeline, device loop (mpc_qp_ikid_low_level_steps)
  fulldynamic   FullDynamicPipeline, device loop (mpc_feedback_low_level_steps)

The robots are the perturbed ensembles of tools/push_recovery.py (sigma_q 0.005, sigma_v 0.01).  Per robot: the step it fell at (-: it did not;
mpc_sim_metrics), whether its MPC solve failed before (failure isolation: it sits the rest out), the distance and the yaw each sole slipped, the steps
it slipped in, the largest force excess over the cone; with FRICTION_SWEEP_ESTIMATOR=1 the base-state estimator runs on pure leg odometry (w_p = w_v
= 1: the assumption that held soles do not move, which slip breaks) and the last column is the final error of its base position against the true
state.  Nothing is asserted: the file states what was measured.

usage: python tools/friction_sweep.py [N] [T_END] [models...]          the sweep (T_END 0: the whole schedule); FRICTION_SWEEP_OUT=file writes it;
                                                                        FRICTION_SWEEP_RUNS=walk,push restricts the experiments
       python tools/friction_sweep.py timing [N] [BLOCKS] [models...]   ms per MPC period with the contact rule on and the friction model off / on identity
                                                                        rows, in alternating blocks of 20 periods of one run (a library without the model:
                                                                        every block is off).  The trajectory keeps its bits, so the difference is the model's
                                                                        one launch per step.  Run another build through MPC_HIP_LIBRARY for the comparison"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpc_benchmark_amd import friction_model
from mpc_benchmark_amd.pipeline import PUSH_FORCE, CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline, push_schedule
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem

TIMING = len(sys.argv) > 1 and sys.argv[1] == "timing"
ARGS = sys.argv[2:] if TIMING else sys.argv[1:]
N = int(ARGS[0]) if len(ARGS) > 0 else 100
SECOND = int(ARGS[1]) if len(ARGS) > 1 else (8 if TIMING else 200)
MODELS = ARGS[2:] or ["kinodynamic", "centroidal", "fulldynamic"]
RUNS = tuple(r for r in (os.environ.get("FRICTION_SWEEP_RUNS") or "walk,push").split(",") if r)
ESTIMATOR = os.environ.get("FRICTION_SWEEP_ESTIMATOR", "") not in ("", "0")
B = 64
SPIN_RADIUS = 0.05
MU = np.concatenate((np.geomspace(0.02, 1.5, B - 1), [np.inf]))


def problem(model):
    return {"kinodynamic": KinodynamicProblem, "fulldynamic": FullDynamicsProblem}.get(model, CentroidalProblem)(horizon=N)


def make_pipeline(model, t_end, friction=None):
    """-> (pipeline with the contact rule on after its cold solve, periods of the run)"""
    kw = dict(batch=B, walk={}, sigma_q=0.005, sigma_v=0.01, tick_reuse=True, contact_rule={}, friction=friction)
    if ESTIMATOR and not TIMING:
        kw["estimator"] = {"w_p": 1.0, "w_v": 1.0}
    pd = problem(model)
    if model == "kinodynamic":
        p = KinodynamicPipeline(pd, perturb=True, **kw)
    elif model == "fulldynamic":
        p = FullDynamicPipeline(pd, **kw)
    else:
        p = CentroidalPipeline(pd, **kw)
    T = t_end if t_end > 0 else pd.t_mpc - 1
    p.mpc.prepare_schedule(T + 16)
    p.cold_solve()
    p.mpc.enable_failure_isolation(auto_revive=False)
    return p, T


def section(model, run, T, substeps, ms, fall_step, lost, st, est_err):
    fell = fall_step >= 0
    out = ["== %s, %s: %d periods (%d steps), %.2f ms per period; fallen %d, lost %d of %d; robots that slipped: %d ==" % (
        model, run, T, T * substeps, ms, int(fell.sum()), int(lost.sum()), B, int(np.any(st["slip_steps"] > 0, axis=1).sum()))]
    up = MU[~fell]
    out.append("  nobody fell" if not fell.any() else "  fell: %d robots, earliest at step %d; still up: %s" % (
        int(fell.sum()), int(fall_step[fell].min()), "mu %s (%d robots)" % (", ".join("%.3g" % v for v in up[:12]) + (" ..." if up.size > 12 else ""), up.size)
        if up.size else "nobody"))
    out.append("  robot |     mu | fall | slip_dist L, R [m] | slip_yaw L, R [rad] | slip_steps L, R | peak excess L, R [N]%s" % (" | estimator base error [m]" if est_err is not None else ""))
    for b in range(B):
        out.append("  %5d | %6.3g | %6s%s | %8.4f %8.4f | %8.4f %8.4f | %6d %6d | %8.1f %8.1f%s" % (
            b, MU[b], "%d" % fall_step[b] if fell[b] else "-", " lost" if lost[b] else "", st["slip_dist"][b, 0], st["slip_dist"][b, 1], st["slip_yaw"][b, 0],
            st["slip_yaw"][b, 1], st["slip_steps"][b, 0], st["slip_steps"][b, 1], st["peak_excess"][b, 0], st["peak_excess"][b, 1],
            "" if est_err is None else " | %10.4f" % est_err[b]))
    out.append("")
    return out


def sweep():
    lines = ["Friction sweep (tools/friction_sweep.py %d %d): 64 robots per run on the unilateral contact rule, one robot per Coulomb coefficient (0.02 .. 1.5 "
             "geometric, robot 63 on +inf), mu_spin = %.2f m * mu, slider masses of friction_model.defaults; N = %d.  MI355X.  Measured; nothing here is an "
             "expectation." % (N, SECOND, SPIN_RADIUS, N),
             "fall: the 1 kHz step the robot fell at (- : it did not); lost: its MPC solve failed before (it sits the rest out).", ""]
    for model in MODELS:
        for run in RUNS:
            p, T = make_pipeline(model, SECOND, friction={"mu": MU, "mu_spin": SPIN_RADIUS * MU})
            p.sim.metrics({})
            t0 = time.perf_counter()
            for t in range(T):
                f = push_schedule(p.mpc.tick, PUSH_FORCE[model]) if run == "push" else None
                p.tick(push=None if f is None else np.tile(np.concatenate([f, np.zeros(3)]), (B, 1)))
            wall = time.perf_counter() - t0
            m, st = p.sim.read_metrics(), p.friction_state()
            lost = np.isin(np.arange(B), [b for (_, b, _, _) in p.mpc.lost])
            err = np.linalg.norm(p.x_est[:, :3] - p.x[:, :3], axis=1) if ESTIMATOR else None
            lines += section(model, run, T, p.substeps, 1e3 * wall / T, m["fall_step"], lost, st, err)
            print("\n".join(lines[-(B + 4):]), flush=True)
            del p
            out = os.environ.get("FRICTION_SWEEP_OUT")
            if out:   # (after every run: a run cut short keeps what it measured)
                with open(out, "w") as fh:
                    fh.write("\n".join(lines) + "\n")


def timing():
    """one run per model: blocks of 20 periods, alternately off and on identity rows from period 20 on (the first 20 warm up); p50 of each kind"""
    if SECOND < 2:
        sys.exit("timing: BLOCKS must be >= 2 (an off block and an on block after the warm-up)")
    for model in MODELS:
        p, _ = make_pipeline(model, 20 * (SECOND + 1))
        has = hasattr(p.sim.lib, "mpc_sim_friction")
        ms = {"off": [], "on": []}
        for blk in range(SECOND + 1):
            kind = "on" if (blk > 0 and blk % 2 == 0) else "off"
            if has and blk > 0:
                p.set_friction(friction_model.IDENTITY if kind == "on" else None)
            for _ in range(20):
                t0 = time.perf_counter()
                p.tick()
                if blk > 0:
                    ms[kind].append((time.perf_counter() - t0) * 1e3)
        off, on = np.array(ms["off"]), np.array(ms["on"])
        print("%s: ms per MPC period (N = %d, 64 robots, contact rule on, %d blocks of 20 periods): odd blocks (model off) p50 %.3f (p10 %.3f, p90 %.3f); even "
              "blocks (%s) p50 %.3f (p10 %.3f, p90 %.3f)" % (model, N, SECOND, np.percentile(off, 50), np.percentile(off, 10), np.percentile(off, 90),
                                                             "model on, identity rows" if has else "model off too: this library has none",
                                                             np.percentile(on, 50), np.percentile(on, 10), np.percentile(on, 90)), flush=True)
        del p


if __name__ == "__main__":
    timing() if TIMING else sweep()
