"""Developer tool (GPU box): what contact DETECTION costs the three control pipelines, as one measured sweep: 64 robots walking the script's schedule
per run with the contact rule, the foot force sensors (``foot_sensors``, include/mpc_sim_foot_sensors.h) and the base-state estimator on, the
estimator — and where the pipeline has low-level QPs, the QPs (``contact_source="plant"``) — fed by the detected contacts instead of the plant's.
One axis per run, the values spread over the robots:

  noise      force noise sigma_f 0 .. 100 N (sigma_m = sigma_f / 20), seed = the robot's index
  offset     constant force offsets, bias_f 0 .. 100 N (bias_m = bias_f / 20), seed = the robot's index
  latency    delay 0 .. 15 steps
  threshold  f_on 10 .. 400 N, f_off = f_on / 2
  debounce   on_steps = off_steps 1 .. 16

Off the axis every robot has the baseline row: no latency, noise or offset, f_on 50 N, f_off 25 N, 2 steps each way.  The estimator runs with
(w_p, w_v) = (0.98, 1) on the exact state (no sensor model), so its errors are those of anchoring and releasing the wrong soles.

  kinodynamic   KinodynamicPipeline, device loop (mpc_qp_low_level_steps), estimator and QPs fed by detection
  centroidal    CentroidalPipeline, device loop (mpc_qp_ikid_low_level_steps), estimator and QPs fed by detection
  fulldynamic   FullDynamicPipeline, device loop (mpc_feedback_low_level_steps), estimator fed by detection (it has no QP)

Per robot: the confusion counts of both soles summed (agree free, detected but released by the plant, held by the plant but not detected, agree
standing), the touchdowns of the plant, the steps a held sole went undetected per touchdown (the mean detection lag where the detector never lets go
in stance; false releases in stance count into it), the estimator's error statistics and the fall verdict of the metrics (mpc_sim_metrics, from the
TRUE states).  A robot whose MPC solve failed sits the rest of the run out (failure isolation) and is marked.  Nothing is asserted: the file states
what was measured.

usage: python tools/foot_sensor_sweep.py [N] [T_END] [models...]          the sweep (T_END 0: the whole schedule); FOOT_SENSOR_SWEEP_OUT=file writes it
                                                                           FOOT_SENSOR_SWEEP_AXES=latency,debounce runs those axes only
       python tools/foot_sensor_sweep.py timing [N] [BLOCKS] [models...]   ms per MPC period with the detector off and on, in alternating blocks of 20
                                                                           periods of one run (a library without the detector — the parent commit's
                                                                           through MPC_HIP_LIBRARY —: every block is off).  Off launches what the commit
                                                                           before launched.  On = baseline rows, feed mask 0: the kernel runs after every
                                                                           step and the trajectory keeps its bits, so the difference is the event alone"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpc_benchmark_amd.pipeline import CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem

MODE = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] == "timing" else "sweep"
ARGS = sys.argv[2:] if MODE != "sweep" else sys.argv[1:]
N = int(ARGS[0]) if len(ARGS) > 0 else 100
SECOND = int(ARGS[1]) if len(ARGS) > 1 else {"sweep": 0, "timing": 8}[MODE]
MODELS = ARGS[2:] or ["kinodynamic", "centroidal", "fulldynamic"]
B = 64
AXES = tuple(os.environ["FOOT_SENSOR_SWEEP_AXES"].split(",")) if os.environ.get("FOOT_SENSOR_SWEEP_AXES") else ("noise", "offset", "latency", "threshold", "debounce")
BASELINE = {"f_on": 50.0, "f_off": 25.0, "on_steps": 2.0, "off_steps": 2.0}
ESTIMATOR = {"w_p": 0.98, "w_v": 1.0}


def make_pipeline(model, t_end, **kw):
    """-> (pipeline with the contact rule after its cold solve, periods of the run)"""
    kw = dict(batch=B, walk={}, sigma_q=0.005, sigma_v=0.01, tick_reuse=True, contact_rule={}, **kw)
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
    """-> (values (B,), what they are, the ``foot_sensors`` dict of the run)"""
    row = dict(BASELINE, seed=np.arange(B, dtype=float))
    if axis == "noise":
        v = np.linspace(0.0, 100.0, B)
        return v, "sigma_f [N]", dict(row, sigma_f=v, sigma_m=v / 20.0)
    if axis == "offset":
        v = np.linspace(0.0, 100.0, B)
        return v, "bias_f [N]", dict(row, bias_f=v, bias_m=v / 20.0)
    if axis == "latency":
        v = np.floor(np.linspace(0.0, 15.99, B))
        return v, "delay [steps]", dict(row, delay=v)
    if axis == "threshold":
        v = np.linspace(10.0, 400.0, B)
        return v, "f_on [N]", dict(row, f_on=v, f_off=v / 2.0)
    v = np.floor(np.linspace(1.0, 16.99, B))
    return v, "on_steps = off_steps", dict(row, on_steps=v, off_steps=v)


def section(model, what, fed, T, substeps, ms, vals, fall_step, lost, counts, touchdowns, stats, count):
    """the lines of one run: the header, where the first robot fell along the axis, one line per robot in the order of the values"""
    fell = fall_step >= 0
    out = ["== %s, %s, fed by detection: %s: %d periods (%d steps), %.2f ms per period; walked %d, fallen %d, lost %d of %d ==" % (
        model, what, " + ".join(fed), T, T * substeps, ms, int((~fell & ~lost).sum()), int(fell.sum()), int(lost.sum()), len(vals))]
    if not fell.any():
        out.append("  nobody fell")
    else:
        first = vals[fell].min()
        below = vals[vals < first]
        out.append("  the smallest value at which a robot fell: %.3f%s; robots still up at larger values: %d; earliest fall at step %d" % (
            first, " (every robot up to %.3f stayed up)" % below.max() if below.size else " (the smallest of the axis)", int((~fell & (vals > first)).sum()),
            int(fall_step[fell].min())))
    out.append("  robot | %s | fall | confusion, both soles: free/free, detected/released, missed/held, standing/standing | touchdowns | missed steps per "
               "touchdown | estimate: RMS p [mm], RMS v [mm/s], max p, max v" % what)
    for b in np.argsort(vals, kind="stable"):
        c = counts[b].sum(axis=0).astype(int)
        td = int(touchdowns[b].sum())
        n = max(count[b] - 1.0, 1.0)
        s = stats[b]
        with np.errstate(invalid="ignore", over="ignore"):
            f = [1e3 * np.sqrt(s[0] / n), 1e3 * np.sqrt(s[1] / n), 1e3 * s[2], 1e3 * s[3]]
        out.append("  %5d | %8.3f | %6s%s | %6d %6d %6d %6d | %3d | %7.2f | %s" % (
            b, vals[b], "%d" % fall_step[b] if fell[b] else "-", " lost" if lost[b] else "", c[0], c[1], c[2], c[3], td, c[2] / max(td, 1),
            " ".join("%9.3f" % v if (np.isfinite(v) and abs(v) < 1e6) else "%9.2e" % v for v in f)))
    out.append("")
    return out


def sweep():
    lines = ["Foot sensor sweep (tools/foot_sensor_sweep.py %d %d): 64 robots per run walking the script's schedule (N = %d) with the contact rule, the foot "
             "force sensors and the base-state estimator (w_p, w_v) = (0.98, 1) on; the estimator and, where there is one, the low-level QPs "
             "(contact_source \"plant\") work from the DETECTED contacts; one axis of the detector per run, baseline f_on 50 N, f_off 25 N, 2 steps each way; "
             "the metrics of mpc_sim_metrics, the detector's confusion counts and the estimator's statistics read once at the end, MI355X.  Measured; "
             "nothing here is an expectation." % (N, SECOND, N),
             "fall: the 1 kHz step the robot fell at (- : it did not); lost: its MPC solve failed before (it sits the rest out); confusion: steps counted "
             "over both soles; the errors are those of the base position and the base linear velocity against the true state over the run (a robot that "
             "fell keeps being integrated and counted).", ""]
    out = os.environ.get("FOOT_SENSOR_SWEEP_OUT")
    for model in MODELS:
        fed = ("estimator",) if model == "fulldynamic" else ("estimator", "qp")
        extra = {} if model == "fulldynamic" else {"contact_source": "plant"}
        for axis in AXES:
            vals, what, rows = axis_rows(axis)
            p, T = make_pipeline(model, SECOND, foot_sensors=rows, detected_contacts=fed, estimator=ESTIMATOR, **extra)
            p.sim.metrics({})
            t0 = time.perf_counter()
            for t in range(T):
                p.tick()
            wall = time.perf_counter() - t0
            m, r, e, c = p.sim.read_metrics(), p.sim.read_foot_sensors(), p.sim.read_estimator(), p.sim.read_contacts()
            lost = np.isin(np.arange(B), [b for (_, b, _, _) in p.mpc.lost])
            lines += section(model, what, fed, T, p.substeps, 1e3 * wall / T, vals, m["fall_step"], lost, r["counts"], c["touchdowns"], e["stats"], e["count"])
            print("\n".join(lines[-(B + 4):]), flush=True)
            del p
            if out:  # (after every run: a sweep that is cut short leaves what it measured)
                with open(out, "w") as fh:
                    fh.write("\n".join(lines) + "\n")


def timing():
    """one run per model: blocks of 20 periods, alternately off and on from period 20 on (the first 20 warm up); p50 of the periods of each kind"""
    for model in MODELS:
        p, _ = make_pipeline(model, 20 * (SECOND + 1))
        has = hasattr(p.sim.lib, "mpc_sim_foot_sensors")
        ms = {"off": [], "on": []}
        for blk in range(SECOND + 1):
            kind = "on" if (blk > 0 and blk % 2 == 0) else "off"
            if has and blk > 0:
                p.set_foot_sensors(BASELINE if kind == "on" else None)
            for _ in range(20):
                t0 = time.perf_counter()
                p.tick()
                if blk > 0:
                    ms[kind].append((time.perf_counter() - t0) * 1e3)
        off, on = np.array(ms["off"]), np.array(ms["on"])
        print("%s: ms per MPC period (N = %d, 64 robots, contact rule on, %d blocks of 20 periods): odd blocks (detector off) p50 %.3f (p10 %.3f, p90 %.3f); "
              "even blocks (%s) p50 %.3f (p10 %.3f, p90 %.3f)" % (model, N, SECOND, np.percentile(off, 50), np.percentile(off, 10), np.percentile(off, 90),
                                                                  "detector on, feed mask 0" if has else "detector off too: this library has none",
                                                                  np.percentile(on, 50), np.percentile(on, 10), np.percentile(on, 90)), flush=True)
        del p


if __name__ == "__main__":
    {"sweep": sweep, "timing": timing}[MODE]()
