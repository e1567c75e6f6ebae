"""Developer tool (GPU box): what the three control pipelines tolerate of their sensors (``sensor_model``, include/mpc_sim_sensors.h), as one measured
sweep: 64 robots walking the script's schedule per run, one axis of the sensor model per run, the values spread over the robots.

  delay        latency of the whole measurement 0 .. 15 ms (steps of the 1 kHz loop): robot b has delay b mod 16, four robots per value
  quantum      encoder resolution: robot 0 none, the others 1e-6 .. 1e-2 rad (evenly spaced in the logarithm), velocities as the simulator gives them
  joint_noise  joint position noise sigma_q 0 .. 5e-3 rad with velocity noise sigma_v = 10 sigma_q rad/s, one robot per value, seed = the robot's index
  base_noise   floating-base noise: position sigma 0 .. 1e-2 m, orientation the same number in rad, linear and angular velocity 10 times it, one robot
               per value, seed = the robot's index

  kinodynamic   KinodynamicPipeline, device loop (mpc_qp_low_level_steps)
  centroidal    CentroidalPipeline, device loop (mpc_qp_ikid_low_level_steps)
  fulldynamic   FullDynamicPipeline, device loop (mpc_feedback_low_level_steps)

The robots are the perturbed ensembles of tools/push_recovery.py (sigma_q 0.005, sigma_v 0.01) on the schedule's contact set.  The locomotion metrics
(mpc_sim_metrics) accumulate on the device, from the TRUE states, and are read once at the end.  Per robot: the step it fell at (-: it did not), the joint
energy, the share of loaded steps with the CoP outside the support box, the RMS of the angular momentum about z.  A robot whose MPC solve failed sits the
rest of the run out (failure isolation) and is marked.  Nothing is asserted: the file states what was measured.

usage: python tools/sensor_sweep.py [N] [T_END] [models...]          the sweep (T_END 0: the whole schedule); SENSOR_SWEEP_OUT=file writes it
       python tools/sensor_sweep.py timing [N] [BLOCKS] [models...]   ms per MPC period with the model off and on, in alternating blocks of 20 periods of
                                                                      one run (a library without the model: every block is off).  Off launches what the
                                                                      commit before the model launched.  On = identity rows: the kernel runs after every
                                                                      step and the trajectory keeps its bits, so the difference is the event alone
       python tools/sensor_sweep.py timing-acting [N] [BLOCKS] [models...]   the same with a row that acts (every branch of the kernel): the robots then move
                                                                      differently, and the iteration counts of the QPs and the solves move with them"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpc_benchmark_amd import sensor_model
from mpc_benchmark_amd.pipeline import CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem

TIMING = len(sys.argv) > 1 and sys.argv[1] in ("timing", "timing-acting")
ACTING = TIMING and sys.argv[1] == "timing-acting"
ARGS = sys.argv[2:] if TIMING else sys.argv[1:]
N = int(ARGS[0]) if len(ARGS) > 0 else 100
SECOND = int(ARGS[1]) if len(ARGS) > 1 else (8 if TIMING else 0)
MODELS = ARGS[2:] or ["kinodynamic", "centroidal", "fulldynamic"]
B = 64
AXES = ("delay", "quantum", "joint_noise", "base_noise")
TIMING_ROW = {"delay": 1.0, "sigma_q": 1e-4, "sigma_v": 1e-3, "sigma_base_p": 1e-4, "sigma_base_r": 1e-4, "sigma_base_v": 1e-3, "sigma_base_w": 1e-3,
              "quantum": 1e-5, "q_bias": 1e-4, "v_from_q": 1.0, "v_time_constant": 2e-3, "seed": 1.0}   # every branch of the kernel


def make_pipeline(model, t_end, sensors=None):
    """-> (pipeline after its cold solve, periods of the run)"""
    kw = dict(batch=B, walk={}, sigma_q=0.005, sigma_v=0.01, tick_reuse=True, sensors=sensors)
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
    if axis == "delay":
        v = (np.arange(B) % sensor_model.RING).astype(float)
        return v, "latency [ms]", {"delay": v}
    if axis == "quantum":
        v = np.concatenate([[0.0], np.logspace(-6.0, -2.0, B - 1)])
        return v * 1e3, "encoder resolution [mrad]", {"quantum": v}
    if axis == "joint_noise":
        v = np.linspace(0.0, 5e-3, B)
        return v * 1e3, "joint noise sigma_q [mrad] (sigma_v = 10 sigma_q / s)", {"sigma_q": v, "sigma_v": 10.0 * v, "seed": seeds}
    v = np.linspace(0.0, 1e-2, B)
    return v * 1e3, "base noise [mm, mrad] (velocities 10 times it / s)", {"sigma_base_p": v, "sigma_base_r": v, "sigma_base_v": 10.0 * v,
                                                                           "sigma_base_w": 10.0 * v, "seed": seeds}


def _num(v, width, dec):
    """a metric of a robot that is still up, or the runaway value of one that fell (the simulator keeps integrating a fallen robot)"""
    return "%*.*f" % (width, dec, v) if (np.isfinite(v) and abs(v) < 1e6) else "%*.2e" % (width, v)


def section(model, what, T, substeps, ms, vals, fall_step, lost, energy, share, rms):
    """the lines of one run: the header, where the first robot fell along the axis, one line per robot in the order of the values"""
    fell = fall_step >= 0
    out = ["== %s, %s: %d periods (%d steps), %.2f ms per period; fallen %d, lost %d of %d ==" % (
        model, what, T, T * substeps, ms, int(fell.sum()), int(lost.sum()), len(vals))]
    if not fell.any():
        out.append("  nobody fell")
    else:
        first = vals[fell].min()
        below = vals[vals < first]
        out.append("  the smallest value at which a robot fell: %.3f%s; robots still up at larger values: %d; earliest fall at step %d" % (
            first, " (every robot up to %.3f stayed up)" % below.max() if below.size else " (the smallest of the axis)", int((~fell & (vals > first)).sum()),
            int(fall_step[fell].min())))
    out.append("  robot | %s | fall | energy | CoP outside | RMS L_z" % what)
    for b in np.argsort(vals, kind="stable"):
        out.append("  %5d | %8.3f | %6s%s | %s | %6.3f | %s" % (b, vals[b], "%d" % fall_step[b] if fell[b] else "-", " lost" if lost[b] else "",
                                                         _num(energy[b], 10, 2), share[b], _num(rms[b], 8, 4)))
    out.append("")
    return out


def sweep():
    lines = ["Sensor sweep (tools/sensor_sweep.py %d %d): 64 robots per run walking the script's schedule (N = %d), one axis of the sensor model per run, "
             "the metrics of mpc_sim_metrics read once at the end, MI355X.  Measured; nothing here is an expectation." % (N, SECOND, N),
             "fall: the 1 kHz step the robot fell at (- : it did not); lost: its MPC solve failed before (it sits the rest out); energy [J]; CoP outside: share "
             "of the loaded steps with the CoP outside the support box; RMS L_z [N m s].", ""]
    for model in MODELS:
        for axis in AXES:
            vals, what, sen = axis_rows(axis)
            p, T = make_pipeline(model, SECOND, sensors=sen)
            p.sim.metrics({})
            t0 = time.perf_counter()
            for t in range(T):
                p.tick()
            wall = time.perf_counter() - t0
            m = p.sim.read_metrics()
            lost = np.isin(np.arange(B), [b for (_, b, _, _) in p.mpc.lost])
            with np.errstate(invalid="ignore", divide="ignore"):
                share = m["cop_outside"] / m["cop_steps"]
                rms = np.sqrt(m["h_ang_z_sq"] / m["steps"])
            lines += section(model, what, T, p.substeps, 1e3 * wall / T, vals, m["fall_step"], lost, m["energy"], share, rms)
            print("\n".join(lines[-(B + 4):]), flush=True)
            del p
    out = os.environ.get("SENSOR_SWEEP_OUT")
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def timing():
    """one run per model: blocks of 20 periods, alternately off and on from period 20 on (the first 20 warm up); p50 of the periods of each kind"""
    for model in MODELS:
        p, _ = make_pipeline(model, 20 * (SECOND + 1))
        has = hasattr(p.sim.lib, "mpc_sim_sensors")
        ms = {"off": [], "on": []}
        for blk in range(SECOND + 1):
            kind = "on" if (blk > 0 and blk % 2 == 0) else "off"
            if has and blk > 0:
                p.set_sensors((TIMING_ROW if ACTING else sensor_model.IDENTITY) if kind == "on" else None)
            for _ in range(20):
                t0 = time.perf_counter()
                p.tick()
                if blk > 0:
                    ms[kind].append((time.perf_counter() - t0) * 1e3)
        off, on = np.array(ms["off"]), np.array(ms["on"])
        print("%s: ms per MPC period (N = %d, 64 robots, %d blocks of 20 periods): odd blocks (model off) p50 %.3f (p10 %.3f, p90 %.3f); even blocks (%s) p50 %.3f "
              "(p10 %.3f, p90 %.3f)" % (model, N, SECOND, np.percentile(off, 50), np.percentile(off, 10), np.percentile(off, 90),
                                        ("model on, a row that acts" if ACTING else "model on, identity rows") if has else "model off too: this library has none", np.percentile(on, 50), np.percentile(on, 10),
                                        np.percentile(on, 90)), flush=True)
        del p


if __name__ == "__main__":
    timing() if TIMING else sweep()
