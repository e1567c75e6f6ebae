"""Developer tool (GPU box): what the three control pipelines need of the sole they plan with (``tipping_model``, include/mpc_sim_tipping.h), as one
measured sweep: 64 robots per run, one robot per plant sole size.  Robot b's plant has ``half_length = s_b 0.1`` and ``half_width = s_b 0.075``, the
controllers' sole (``FOOT_HALF_LENGTH``, ``FOOT_HALF_WIDTH``) scaled by ``s_b``, geometric from 1 down to 0.05, and the last robot on +inf (the
ground every earlier sweep stood on: a sole that transmits any moment).  The controllers keep their own sole in the MPC stages and the low-level
QPs; only the simulated plant tips.  Two experiments per formulation, on the unilateral contact rule:

  walk   the script's walking schedule
  push   the same with the scripts' push (``pipeline.push_schedule``: MPC ticks 160 - 170, the script's force at the world origin)

  kinodynamic   KinodynamicPipeline, device loop (mpc_qp_low_level_steps)
  centroidal    CentroidalPipeline, device loop (mpc_qp_ikid_low_level_steps)
  fulldynamic   FullDynamicPipeline, device loop (mpc_feedback_low_level_steps)

The robots are the perturbed ensembles of tools/push_recovery.py (sigma_q 0.005, sigma_v 0.01).  Per robot: the step it fell at (-: it did not;
mpc_sim_metrics), whether its MPC solve failed before (failure isolation: it sits the rest out), the largest angle each sole reached, the steps it
tipped in, its landings, the largest moment excess over the sole (the plant of a lost robot is integrated on under its last torques, so its excess
after the fall can be any size).  Nothing is asserted: the file states what was measured.

usage: python tools/tipping_sweep.py [N] [T_END] [models...]          the sweep (T_END 0: the whole schedule); TIPPING_SWEEP_OUT=file writes it;
                                                                       TIPPING_SWEEP_RUNS=walk,push restricts the experiments
       python tools/tipping_sweep.py timing [N] [BLOCKS] [models...]   ms per MPC period with the contact rule on and the tipping model off / on identity
                                                                       rows, in alternating blocks of 20 periods of one run (a library without the model:
                                                                       every block is off).  The trajectory keeps its bits, so the difference is the model's
                                                                       one launch per step.  Run another build through MPC_HIP_LIBRARY for the comparison"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpc_benchmark_amd import tipping_model
from mpc_benchmark_amd.pipeline import PUSH_FORCE, CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline, push_schedule
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.common import FOOT_HALF_LENGTH, FOOT_HALF_WIDTH
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem

TIMING = len(sys.argv) > 1 and sys.argv[1] == "timing"
ARGS = sys.argv[2:] if TIMING else sys.argv[1:]
N = int(ARGS[0]) if len(ARGS) > 0 else 100
SECOND = int(ARGS[1]) if len(ARGS) > 1 else (8 if TIMING else 200)
MODELS = ARGS[2:] or ["kinodynamic", "centroidal", "fulldynamic"]
RUNS = tuple(r for r in (os.environ.get("TIPPING_SWEEP_RUNS") or "walk,push").split(",") if r)
B = 64
SCALE = np.concatenate((np.geomspace(1.0, 0.05, B - 1), [np.inf]))


def problem(model):
    return {"kinodynamic": KinodynamicProblem, "fulldynamic": FullDynamicsProblem}.get(model, CentroidalProblem)(horizon=N)


def make_pipeline(model, t_end, tipping=None):
    """-> (pipeline with the contact rule on after its cold solve, periods of the run)"""
    kw = dict(batch=B, walk={}, sigma_q=0.005, sigma_v=0.01, tick_reuse=True, contact_rule={})
    if tipping is not None:
        kw["tipping"] = tipping
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


def section(model, run, T, substeps, ms, fall_step, lost, st):
    fell = fall_step >= 0
    out = ["== %s, %s: %d periods (%d steps), %.2f ms per period; fallen %d, lost %d of %d; robots that tipped: %d ==" % (
        model, run, T, T * substeps, ms, int(fell.sum()), int(lost.sum()), B, int(np.any(st["tip_steps"] > 0, axis=1).sum()))]
    up = SCALE[~fell]
    out.append("  nobody fell" if not fell.any() else "  fell: %d robots, earliest at step %d; still up: %s" % (
        int(fell.sum()), int(fall_step[fell].min()), "scale %s (%d robots)" % (", ".join("%.3g" % v for v in up[:12]) + (" ..." if up.size > 12 else ""), up.size)
        if up.size else "nobody"))
    out.append("  robot |  scale | half_width [m] | fall | peak_angle L, R [rad] | tip_steps L, R | landings L, R | peak excess L, R [N m]")
    for b in range(B):
        out.append("  %5d | %6.3g | %14.4g | %6s%s | %8.4f %8.4f | %6d %6d | %5d %5d | %9.3g %9.3g" % (
            b, SCALE[b], SCALE[b] * FOOT_HALF_WIDTH, "%d" % fall_step[b] if fell[b] else "-", " lost" if lost[b] else "", st["peak_angle"][b, 0],
            st["peak_angle"][b, 1], st["tip_steps"][b, 0], st["tip_steps"][b, 1], st["landings"][b, 0], st["landings"][b, 1], st["peak_excess"][b, 0],
            st["peak_excess"][b, 1]))
    out.append("")
    return out


def sweep():
    lines = ["Tipping sweep (tools/tipping_sweep.py %d %d): 64 robots per run on the unilateral contact rule, one robot per plant sole size (the controllers' "
             "%.3g x %.3g m half extents scaled by 1 .. 0.05 geometric, robot 63 on +inf), slider inertia of tipping_model.defaults; N = %d.  MI355X.  "
             "Measured; nothing here is an expectation." % (N, SECOND, FOOT_HALF_LENGTH, FOOT_HALF_WIDTH, N),
             "fall: the 1 kHz step the robot fell at (- : it did not); lost: its MPC solve failed before (it sits the rest out).", ""]
    for model in MODELS:
        for run in RUNS:
            p, T = make_pipeline(model, SECOND, tipping={"half_length": SCALE * FOOT_HALF_LENGTH, "half_width": SCALE * FOOT_HALF_WIDTH})
            p.sim.metrics({})
            t0 = time.perf_counter()
            for t in range(T):
                f = push_schedule(p.mpc.tick, PUSH_FORCE[model]) if run == "push" else None
                p.tick(push=None if f is None else np.tile(np.concatenate([f, np.zeros(3)]), (B, 1)))
            wall = time.perf_counter() - t0
            m, st = p.sim.read_metrics(), p.tipping_state()
            lost = np.isin(np.arange(B), [b for (_, b, _, _) in p.mpc.lost])
            lines += section(model, run, T, p.substeps, 1e3 * wall / T, m["fall_step"], lost, st)
            print("\n".join(lines[-(B + 4):]), flush=True)
            del p
            out = os.environ.get("TIPPING_SWEEP_OUT")
            if out:   # (after every run: a run cut short keeps what it measured)
                with open(out, "w") as fh:
                    fh.write("\n".join(lines) + "\n")


def timing():
    """one run per model: blocks of 20 periods, alternately off and on identity rows from period 20 on (the first 20 warm up); p50 of each kind"""
    if SECOND < 2:
        sys.exit("timing: BLOCKS must be >= 2 (an off block and an on block after the warm-up)")
    for model in MODELS:
        p, _ = make_pipeline(model, 20 * (SECOND + 1))
        has = hasattr(p.sim.lib, "mpc_sim_tipping")
        ms = {"off": [], "on": []}
        for blk in range(SECOND + 1):
            kind = "on" if (blk > 0 and blk % 2 == 0) else "off"
            if has and blk > 0:
                p.set_tipping(tipping_model.IDENTITY if kind == "on" else None)
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
