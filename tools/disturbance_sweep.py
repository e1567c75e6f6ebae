"""Developer tool (GPU box): which pushes the three control pipelines recover from, as one measured sweep per formulation (``disturbance_model``,
include/mpc_sim_disturbances.h): 64 robots walking the script's schedule under the unilateral contact rule, each robot with its own push: 8
magnitudes x 4 delays after its own first left touchdown, on the base and on one arm link.  The device times every robot's push on that robot's
gait; the host does nothing inside a period.

  push       a horizontal world force along theta = 3 pi / 2 (the scripts' direction), half sine over 100 steps, at the link's origin, carried with it
  magnitude  8 values, 50 .. 400 N
  delay      0, 100, 200, 300 steps after the robot's first left touchdown
  link       the base (root_joint), the last moving joint of the left arm

  kinodynamic   KinodynamicPipeline, device loop (mpc_qp_low_level_steps)
  centroidal    CentroidalPipeline, device loop (mpc_qp_ikid_low_level_steps)
  fulldynamic   FullDynamicPipeline, device loop (mpc_feedback_low_level_steps)

The robots are the perturbed ensembles of tools/push_recovery.py (sigma_q 0.005, sigma_v 0.01).  The locomotion metrics (mpc_sim_metrics) accumulate
on the device and their fall verdict is read once at the end, with the schedule's own state rows (when each robot's push began, its impulse).
Nothing is asserted: the file states what was measured.

usage: python tools/disturbance_sweep.py [N] [T_END] [models...]          the sweep (T_END 0: the whole schedule); DISTURBANCE_SWEEP_OUT=file writes it
       python tools/disturbance_sweep.py timing [N] [BLOCKS] [models...]   ms per MPC period with the model off and with a table armed (a push train
                                                                           on the arm link: body-fixed frames, the kinematics run), in alternating
                                                                           blocks of 20 periods of one run (a library without the model: every block
                                                                           is off).  Run another build of the library through MPC_HIP_LIBRARY for the
                                                                           comparison against it; DISTURBANCE_SWEEP_IDLE=1 arms a table that never
                                                                           fires (the launches alone, on the unchanged trajectory)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpc_benchmark_amd import disturbance_model as dm
from mpc_benchmark_amd.pipeline import PUSH_THETA, CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem

TIMING = len(sys.argv) > 1 and sys.argv[1] == "timing"
ARGS = sys.argv[2:] if TIMING else sys.argv[1:]
N = int(ARGS[0]) if len(ARGS) > 0 else 100
SECOND = int(ARGS[1]) if len(ARGS) > 1 else (8 if TIMING else 0)
MODELS = ARGS[2:] or ["kinodynamic", "centroidal", "fulldynamic"]
B = 64
MAGNITUDES = np.linspace(50.0, 400.0, 8)
DELAYS = (0, 100, 200, 300)
PUSH_STEPS = 100


def problem(model):
    return {"kinodynamic": KinodynamicProblem, "fulldynamic": FullDynamicsProblem}.get(model, CentroidalProblem)(horizon=N)


def make_pipeline(model, t_end, **kw):
    """-> (pipeline after its cold solve, periods of the run)"""
    kw = dict(dict(batch=B, walk={}, sigma_q=0.005, sigma_v=0.01, tick_reuse=True), **kw)
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


def arm_link(m):
    """table joint index of the last moving joint of the left arm"""
    return m.getJointId([n for n in m.names if n.startswith("arm_left_")][-1]) - 1


def tables(m):
    """-> (tables (B, 1, 16), grid (B, 3): magnitude, delay, link)"""
    grid = np.array([(f, d, l) for l in (0, arm_link(m)) for f in MAGNITUDES for d in DELAYS], dtype=float)
    d = np.array([np.cos(PUSH_THETA), np.sin(PUSH_THETA), 0.0])
    ev = np.array([[dm.event("left_touchdown", start=1, delay=int(dl), steps=PUSH_STEPS, shape=1, link=int(l), point_frame=1, force=f * d)] for f, dl, l in grid])
    return ev, grid


def sweep():
    lines = ["Disturbance sweep (tools/disturbance_sweep.py %d %d): 64 robots per formulation walking the script's schedule (N = %d) under the contact rule, "
             "every robot with its own push (half sine, %d steps, along theta = 3 pi / 2 at the link's origin), timed by the device on the robot's first left "
             "touchdown.  The fall verdict of mpc_sim_metrics read once at the end, MI355X.  Measured; nothing here is an expectation." % (N, SECOND, N, PUSH_STEPS),
             "began: the 1 kHz step the push began at (- : the robot's left sole never touched down in the run); impulse [N s]; fall: the step the robot fell "
             "at (- : it did not); lost: its MPC solve failed before (it sits the rest out).", ""]
    for model in MODELS:
        m = problem(model).robot.model
        ev, grid = tables(m)
        p, T = make_pipeline(model, SECOND, contact_rule={}, disturbances=ev)
        p.sim.metrics({})
        t0 = time.perf_counter()
        for t in range(T):
            p.tick()
        wall = time.perf_counter() - t0
        met, st = p.sim.read_metrics(), p.disturbance_state()
        lost = np.isin(np.arange(B), [b for (_, b, _, _) in p.mpc.lost])
        fell = met["fall_step"] >= 0
        lines.append("== %s: %d periods (%d steps), %.2f ms per period; fallen %d, lost %d of %d ==" % (
            model, T, T * p.substeps, 1e3 * wall / T, int(fell.sum()), int(lost.sum()), B))
        for l in sorted(set(grid[:, 2])):
            on = grid[:, 2] == l
            ok = on & ~fell & ~lost
            lines.append("  link %d (%s): recovered %d of %d; largest magnitude every delay recovered from: %s" % (
                l, m.names[int(l) + 1], int(ok.sum()), int(on.sum()),
                ("%.0f N" % max([f for f in MAGNITUDES if all(ok[on & (grid[:, 0] == f)])], default=0.0))))
        lines.append("  robot | link | magnitude | delay | began | impulse | fall")
        for b in range(B):
            began = st["fire_step"][b, 0]
            lines.append("  %5d | %4d | %9.1f | %5d | %5s | %7.2f | %6s%s" % (
                b, grid[b, 2], grid[b, 0], grid[b, 1], "%d" % began if began >= 0 else "-", float(np.linalg.norm(st["impulse"][b])),
                "%d" % met["fall_step"][b] if fell[b] else "-", " lost" if lost[b] else ""))
        lines.append("")
        print("\n".join(lines[-(B + 6):]), flush=True)
        del p
        out = os.environ.get("DISTURBANCE_SWEEP_OUT")
        if out:   # (after every run: a run cut short keeps what it measured)
            with open(out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


def timing():
    """one run per model: blocks of 20 periods, alternately off and on (a push train on the arm link) from period 20 on (the first 20 warm up)"""
    if SECOND < 2:
        sys.exit("timing: BLOCKS must be >= 2 (an off block and an on block after the warm-up)")
    for model in MODELS:
        p, _ = make_pipeline(model, 20 * (SECOND + 1))
        has = hasattr(p.sim.lib, "mpc_sim_disturbances")
        idle = bool(os.environ.get("DISTURBANCE_SWEEP_IDLE"))   # the table never fires: the trajectory keeps its bits, the launches stay
        train = dm.event("step", start=10 ** 9 if idle else 0, steps=3, period=7, shape=1, link=arm_link(p.model), force_frame=1, point_frame=1, force=(0.0, -5.0, 0.0),
                         point=(0.0, 0.0, -0.1))
        ms = {"off": [], "on": []}
        for blk in range(SECOND + 1):
            kind = "on" if (blk > 0 and blk % 2 == 0) else "off"
            if has and blk > 0:
                p.set_disturbances(train if kind == "on" else None)
            for _ in range(20):
                t0 = time.perf_counter()
                p.tick()
                if blk > 0:
                    ms[kind].append((time.perf_counter() - t0) * 1e3)
        off, on = np.array(ms["off"]), np.array(ms["on"])
        print("%s: ms per MPC period (N = %d, 64 robots, %d blocks of 20 periods): odd blocks (model off) p50 %.3f (p10 %.3f, p90 %.3f); even blocks (%s) p50 %.3f "
              "(p10 %.3f, p90 %.3f)" % (model, N, SECOND, np.percentile(off, 50), np.percentile(off, 10), np.percentile(off, 90),
                                        ("a table armed that never fires" if idle else "a table armed, 5 N push train on the arm link") if has else "model off too: this library has none",
                                        np.percentile(on, 50), np.percentile(on, 10), np.percentile(on, 90)), flush=True)
        del p


if __name__ == "__main__":
    timing() if TIMING else sweep()
