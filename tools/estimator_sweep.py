"""Developer tool (GPU box): what the base-state estimator (``state_estimator``, include/mpc_sim_estimator.h) buys the three control pipelines under
floating-base noise, as one measured sweep: 64 robots walking the script's schedule per run with the contact rule and the sensor model on, one axis of
base noise per run, the values spread over the robots, each axis run three times.

  base_v   base linear velocity noise sigma_base_v 0 .. 0.2 m/s, one robot per value, seed = the robot's index
  base_p   base position noise sigma_base_p 0 .. 2e-2 m, one robot per value, seed = the robot's index

  off          the controllers read the raw measurement (what tools/sensor_sweep.py measures)
  (0, 1)       w_p = 0, w_v = 1: the base linear velocity by leg odometry alone, the base position as measured
  (0.98, 1)    w_p = 0.98, w_v = 1: the base position by leg odometry, pulled to the measurement by 2 % per 1 kHz event

  kinodynamic   KinodynamicPipeline, device loop (mpc_qp_low_level_steps)
  centroidal    CentroidalPipeline, device loop (mpc_qp_ikid_low_level_steps)
  fulldynamic   FullDynamicPipeline, device loop (mpc_feedback_low_level_steps)

The robots are the perturbed ensembles of tools/push_recovery.py (sigma_q 0.005, sigma_v 0.01).  The locomotion metrics (mpc_sim_metrics) accumulate on
the device, from the TRUE states; the estimator's statistics (RMS and largest error of the base position and linear velocity against the true state,
of the estimate and of the raw measurement) accumulate in its rows.  Both are read once at the end.  A robot whose MPC solve failed sits the rest of
the run out (failure isolation) and is marked.  Nothing is asserted: the file states what was measured.

usage: python tools/estimator_sweep.py [N] [T_END] [models...]          the sweep (T_END 0: the whole schedule); ESTIMATOR_SWEEP_OUT=file writes it
       python tools/estimator_sweep.py timing [N] [BLOCKS] [models...]   ms per MPC period with the estimator off and on, in alternating blocks of 20
                                                                         periods of one run (a library without the estimator — the parent commit's
                                                                         through MPC_HIP_LIBRARY —: every block is off).  Off launches what the commit
                                                                         before the estimator launched.  On = identity rows: the kernel runs after every
                                                                         step and the trajectory keeps its bits, so the difference is the event alone
       python tools/estimator_sweep.py profile [N] [PERIODS] [models...]  PERIODS periods with identity rows, for
                                                                         rocprofv3 --kernel-trace --stats -- python tools/estimator_sweep.py profile ...:
                                                                         k_sim_estimator per launch beside k_sim_contacts and k_sim_sensors"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpc_benchmark_amd import sensor_model, state_estimator
from mpc_benchmark_amd.pipeline import CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem

MODE = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] in ("timing", "profile") else "sweep"
ARGS = sys.argv[2:] if MODE != "sweep" else sys.argv[1:]
N = int(ARGS[0]) if len(ARGS) > 0 else 100
SECOND = int(ARGS[1]) if len(ARGS) > 1 else {"sweep": 0, "timing": 8, "profile": 30}[MODE]
MODELS = ARGS[2:] or ["kinodynamic", "centroidal", "fulldynamic"]
B = 64
AXES = ("base_v", "base_p")
SETTINGS = (("off", None), ("(0, 1)", {"w_p": 0.0, "w_v": 1.0}), ("(0.98, 1)", {"w_p": 0.98, "w_v": 1.0}))


def make_pipeline(model, t_end, sensors=None, estimator=None):
    """-> (pipeline with the contact rule after its cold solve, periods of the run)"""
    kw = dict(batch=B, walk={}, sigma_q=0.005, sigma_v=0.01, tick_reuse=True, contact_rule={}, sensors=sensors, estimator=estimator)
    if model == "kinodynamic":
        pd = KinodynamicProblem(horizon=N)
        p = KinodynamicPipeline(pd, perturb=True, **kw)
    elif model == "fulldynamic":
        pd = FullDynamicsProblem(horizon=N)
        p = FullDynamicPipeline(pd, **kw)
    else:
        pd = CentroidalProblem(horizon=N)
        p = CentroidalPipeline(pd, **kw)
    T = t_end if t_end > 0 else pd.t_mpc - 1
    p.mpc.prepare_schedule(T + 16)
    p.cold_solve()
    p.mpc.enable_failure_isolation(auto_revive=False)
    return p, T


def axis_rows(axis):
    """-> (values (B,), what they are, the ``sensors`` dict of the run)"""
    seeds = np.arange(B, dtype=float)
    if axis == "base_v":
        v = np.linspace(0.0, 0.2, B)
        return v, "sigma_base_v [m/s]", {"sigma_base_v": v, "seed": seeds}
    v = np.linspace(0.0, 2e-2, B)
    return v * 1e3, "sigma_base_p [mm]", {"sigma_base_p": v, "seed": seeds}


def section(model, what, setting, T, substeps, ms, vals, fall_step, lost, stats, count):
    """the lines of one run: the header, where the first robot fell along the axis, one line per robot in the order of the values"""
    fell = fall_step >= 0
    out = ["== %s, %s, estimator %s: %d periods (%d steps), %.2f ms per period; walked %d, fallen %d, lost %d of %d ==" % (
        model, what, setting, T, T * substeps, ms, int((~fell & ~lost).sum()), int(fell.sum()), int(lost.sum()), len(vals))]
    if not fell.any():
        out.append("  nobody fell")
    else:
        first = vals[fell].min()
        below = vals[vals < first]
        out.append("  the smallest value at which a robot fell: %.3f%s; robots still up at larger values: %d; earliest fall at step %d" % (
            first, " (every robot up to %.3f stayed up)" % below.max() if below.size else " (the smallest of the axis)", int((~fell & (vals > first)).sum()),
            int(fall_step[fell].min())))
    if stats is None:
        out.append("  robot | %s | fall" % what)
    else:
        out.append("  robot | %s | fall | estimate: RMS p [mm], RMS v [mm/s], max p, max v | measurement: the same four" % what)
    for b in np.argsort(vals, kind="stable"):
        line = "  %5d | %8.3f | %6s%s" % (b, vals[b], "%d" % fall_step[b] if fell[b] else "-", " lost" if lost[b] else "")
        if stats is not None:
            n = max(count[b] - 1.0, 1.0)
            s = stats[b]
            with np.errstate(invalid="ignore", over="ignore"):
                f = [1e3 * np.sqrt(s[0] / n), 1e3 * np.sqrt(s[1] / n), 1e3 * s[2], 1e3 * s[3], 1e3 * np.sqrt(s[4] / n), 1e3 * np.sqrt(s[5] / n), 1e3 * s[6], 1e3 * s[7]]
            line += " | " + " ".join("%9.3f" % v if (np.isfinite(v) and abs(v) < 1e6) else "%9.2e" % v for v in f[:4])
            line += " | " + " ".join("%9.3f" % v if (np.isfinite(v) and abs(v) < 1e6) else "%9.2e" % v for v in f[4:])
        out.append(line)
    out.append("")
    return out


def sweep():
    lines = ["Estimator sweep (tools/estimator_sweep.py %d %d): 64 robots per run walking the script's schedule (N = %d) with the contact rule and the sensor "
             "model on, one axis of floating-base noise per run, each with the estimator off, with (w_p, w_v) = (0, 1) and with (0.98, 1); the metrics of "
             "mpc_sim_metrics and the estimator's statistics read once at the end, MI355X.  Measured; nothing here is an expectation." % (N, SECOND, N),
             "fall: the 1 kHz step the robot fell at (- : it did not); lost: its MPC solve failed before (it sits the rest out); the errors are those of the "
             "base position and the base linear velocity against the true state over the run (a robot that fell keeps being integrated and counted).", ""]
    out = os.environ.get("ESTIMATOR_SWEEP_OUT")
    for model in MODELS:
        for axis in AXES:
            vals, what, sen = axis_rows(axis)
            for setting, est in SETTINGS:
                p, T = make_pipeline(model, SECOND, sensors=sen, estimator=est)
                p.sim.metrics({})
                t0 = time.perf_counter()
                for t in range(T):
                    p.tick()
                wall = time.perf_counter() - t0
                m = p.sim.read_metrics()
                r = p.sim.read_estimator() if est is not None else None
                lost = np.isin(np.arange(B), [b for (_, b, _, _) in p.mpc.lost])
                lines += section(model, what, setting, T, p.substeps, 1e3 * wall / T, vals, m["fall_step"], lost, None if r is None else r["stats"],
                                 None if r is None else r["count"])
                print("\n".join(lines[-(B + 4):]), flush=True)
                del p
                if out:  # (after every run: a sweep that is cut short leaves what it measured)
                    with open(out, "w") as fh:
                        fh.write("\n".join(lines) + "\n")


def timing():
    """one run per model: blocks of 20 periods, alternately off and on from period 20 on (the first 20 warm up); p50 of the periods of each kind"""
    for model in MODELS:
        p, _ = make_pipeline(model, 20 * (SECOND + 1))
        has = hasattr(p.sim.lib, "mpc_sim_estimator")
        ms = {"off": [], "on": []}
        for blk in range(SECOND + 1):
            kind = "on" if (blk > 0 and blk % 2 == 0) else "off"
            if has and blk > 0:
                p.set_estimator(state_estimator.IDENTITY if kind == "on" else None)
            for _ in range(20):
                t0 = time.perf_counter()
                p.tick()
                if blk > 0:
                    ms[kind].append((time.perf_counter() - t0) * 1e3)
        off, on = np.array(ms["off"]), np.array(ms["on"])
        print("%s: ms per MPC period (N = %d, 64 robots, contact rule on, %d blocks of 20 periods): odd blocks (estimator off) p50 %.3f (p10 %.3f, p90 %.3f); "
              "even blocks (%s) p50 %.3f (p10 %.3f, p90 %.3f)" % (model, N, SECOND, np.percentile(off, 50), np.percentile(off, 10), np.percentile(off, 90),
                                                                  "estimator on, identity rows" if has else "estimator off too: this library has none",
                                                                  np.percentile(on, 50), np.percentile(on, 10), np.percentile(on, 90)), flush=True)
        del p


def profile():
    """SECOND periods per model with identity sensors and identity estimator rows: every simulator kernel runs after every step"""
    for model in MODELS:
        p, _ = make_pipeline(model, SECOND + 4, sensors=sensor_model.IDENTITY, estimator=state_estimator.IDENTITY)
        for _ in range(SECOND):
            p.tick()
        print("%s: %d periods, %d launches of each simulator kernel" % (model, SECOND, SECOND * p.substeps), flush=True)
        del p


if __name__ == "__main__":
    {"sweep": sweep, "timing": timing, "profile": profile}[MODE]()
