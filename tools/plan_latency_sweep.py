"""Developer tool (GPU box): how much hand-over latency of the plan each of the three control pipelines tolerates, as one measured sweep per
formulation (``plan_latency``, include/mpc_plan_latency.h): one ensemble per formulation walking the script's schedule under the unilateral contact
rule, one robot per latency value.  After every publication robot b keeps running knot 1 of the plan before for its first L_b low-level steps; the
countdown and the held records live on the device, the host does nothing inside a period.

  latency    0, 2, 4, 6, 8, 10 steps of 1 ms (10 = a whole MPC period), and the same with a jitter of JITTER steps on top, drawn per publication
  robots     the SAME initial state for every robot of an ensemble (no perturbation): the rows differ by their latency alone

  kinodynamic   KinodynamicPipeline, device loop (mpc_qp_low_level_steps)
  centroidal    CentroidalPipeline, device loop (mpc_qp_ikid_low_level_steps)
  fulldynamic   FullDynamicPipeline, device loop (mpc_feedback_low_level_steps)

The locomotion metrics (mpc_sim_metrics) accumulate on the device and are read once at the end, with the model's own counters.  Nothing is asserted:
the file states what was measured.  ``plan_latency.from_solve_ms`` turns a measured solve time into steps.

usage: python tools/plan_latency_sweep.py [N] [T_END] [models...]           the sweep (T_END 0: the whole schedule); PLAN_LATENCY_SWEEP_OUT=file writes it
       python tools/plan_latency_sweep.py timing [N] [BLOCKS] [models...]    ms per MPC period of 64 robots with the model off, armed with rows all 0
                                                                             and armed with L = 5, in rotating blocks of 20 periods of one run (a
                                                                             library without the model: every block is off).  Run another build of the
                                                                             library through MPC_HIP_LIBRARY for the comparison against it."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpc_benchmark_amd.pipeline import CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem

TIMING = len(sys.argv) > 1 and sys.argv[1] == "timing"
ARGS = sys.argv[2:] if TIMING else sys.argv[1:]
N = int(ARGS[0]) if len(ARGS) > 0 else 100
SECOND = int(ARGS[1]) if len(ARGS) > 1 else (9 if TIMING else 0)
MODELS = ARGS[2:] or ["kinodynamic", "centroidal", "fulldynamic"]
STEPS = (0, 2, 4, 6, 8, 10)
JITTER = 4
ROWS = np.array([[s, j, 100 + i, 0] for j in (0, JITTER) for i, s in enumerate(STEPS)], dtype=float)


def problem(model):
    return {"kinodynamic": KinodynamicProblem, "fulldynamic": FullDynamicsProblem}.get(model, CentroidalProblem)(horizon=N)


def make_pipeline(model, t_end, batch, **kw):
    """-> (pipeline after its cold solve, periods of the run)"""
    kw = dict(dict(batch=batch, walk={}, tick_reuse=True), **kw)
    pd = problem(model)
    if model == "kinodynamic":
        p = KinodynamicPipeline(pd, **kw)
    elif model == "fulldynamic":
        p = FullDynamicPipeline(pd, **kw)
    else:
        p = CentroidalPipeline(pd, **kw)
    T = t_end if t_end > 0 else pd.t_mpc - 1
    p.mpc.prepare_schedule(T + 16)
    p.cold_solve()
    p.mpc.enable_failure_isolation(auto_revive=False)
    return p, T


def sweep():
    B = len(ROWS)
    lines = ["Plan latency sweep (tools/plan_latency_sweep.py %d %d): %d robots per formulation from ONE initial state walking the script's schedule (N = %d) "
             "under the contact rule, robot b with the hand-over latency of its row (steps, and steps + a jitter of 0 .. %d drawn per publication).  "
             "Metrics of mpc_sim_metrics read once at the end, MI355X.  Measured; nothing here is an expectation." % (N, SECOND, B, N, JITTER),
             "late: low-level steps run on the held record, of all steps; max: the largest latency drawn; fall: the step the robot fell at (- : it did "
             "not); lost: its MPC solve failed before (it sits the rest out); energy [J]; peak power [W]; CoP margin: minimum and mean [m]; com: "
             "displacement of the centre of mass [m].", ""]
    for model in MODELS:
        p, T = make_pipeline(model, SECOND, B, contact_rule={}, latency=ROWS, perturb=False)
        p.sim.metrics({})
        t0 = time.perf_counter()
        for t in range(T):
            p.tick()
        wall = time.perf_counter() - t0
        met, st = p.sim.read_metrics(), p.latency_state()
        lost = np.isin(np.arange(B), [b for (_, b, _, _) in p.mpc.lost])
        fell = met["fall_step"] >= 0
        lines.append("== %s: %d periods (%d steps), %.2f ms per period; fallen %d, lost %d of %d ==" % (
            model, T, T * p.substeps, 1e3 * wall / T, int(fell.sum()), int(lost.sum()), B))
        lines.append("  robot | steps | jitter | late / steps | max | fall   | energy   | peak power | CoP margin min / mean | com dx, dy, dz")
        for b in range(B):
            n = max(float(met["cop_steps"][b]), 1.0)
            d = met["com_last"][b] - met["com_first"][b]
            lines.append("  %5d | %5d | %6d | %5d / %5d | %3d | %6s | %8.2f | %10.1f | %8.4f / %8.4f | %7.3f %7.3f %7.3f%s" % (
                b, ROWS[b, 0], ROWS[b, 1], st["late_steps"][b], st["steps_total"][b], st["max_drawn"][b],
                "%d" % met["fall_step"][b] if fell[b] else "-", met["energy"][b], met["peak_power"][b], met["margin_min"][b],
                met["margin_sum"][b] / n, d[0], d[1], d[2], " lost" if lost[b] else ""))
        lines.append("")
        print("\n".join(lines[-(B + 3):]), flush=True)
        del p
        out = os.environ.get("PLAN_LATENCY_SWEEP_OUT")
        if out:   # (after every run: a run cut short keeps what it measured)
            with open(out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


def timing():
    """one run per model: blocks of 20 periods, in rotation off / armed with rows all 0 / armed with L = 5, from period 20 on (the first 20 warm up)"""
    if SECOND < 3:
        sys.exit("timing: BLOCKS must be >= 3 (one block of each kind after the warm-up)")
    kinds = (("off", None), ("zero", 0), ("five", 5))
    for model in MODELS:
        p, _ = make_pipeline(model, 20 * (SECOND + 1), 64, sigma_q=0.005, sigma_v=0.01, **(dict(perturb=True) if model == "kinodynamic" else {}))
        has = hasattr(p.lib, "mpc_plan_latency")
        ms = {k: [] for k, _ in kinds}
        for blk in range(SECOND + 1):
            kind, rows = kinds[(blk - 1) % 3] if blk > 0 else kinds[0]
            if has and blk > 0:
                p.set_latency(rows)
            for _ in range(20):
                t0 = time.perf_counter()
                p.tick()
                if blk > 0:
                    ms[kind].append((time.perf_counter() - t0) * 1e3)
        q = lambda a: "p50 %.3f (p10 %.3f, p90 %.3f)" % tuple(np.percentile(np.array(a), [50, 10, 90]))
        print("%s: ms per MPC period (N = %d, 64 robots, %d blocks of 20 periods)%s: off %s; armed, rows all 0 %s; armed, L = 5 %s" % (
            model, N, SECOND, "" if has else " [this library has no latency model: every block is off]", q(ms["off"]), q(ms["zero"]), q(ms["five"])),
            flush=True)
        del p


if __name__ == "__main__":
    timing() if TIMING else sweep()
