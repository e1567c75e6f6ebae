"""Developer tool (GPU box): plot.py's comparison of the three formulations (centre of pressure against the support box, angular momentum, joint
power and energy) over 64 robots per formulation and the scripts' whole loops, from the device metrics of the simulator handle (mpc_sim_metrics,
include/mpc_sim_metrics.h) read once at the end of each run.

  kinodynamic   KinodynamicPipeline, device loop (mpc_qp_low_level_steps), 820 MPC periods (kinodynamic_talos.py)
  centroidal    CentroidalPipeline, device loop (mpc_qp_ikid_low_level_steps), 420 periods (centroidal_talos.py)
  fulldynamic   FullDynamicPipeline, device loop (mpc_feedback_low_level_steps), 1000 periods (fulldynamic_talos.py)

Built as tools/push_recovery.py builds them: 64 perturbed robots, the scripts' walks, N = 100, the reduced model, failure isolation (a robot whose MPC
fails sits the rest out and counts as fallen).  Unpushed.  The cost: ms per MPC period (one tick: the ten low-level steps and the solve) at p50 over
periods 100 - 199, once with metrics off (a run of its own over the first 200 periods) and once with metrics on (the whole run).
usage: python tools/locomotion_metrics.py [--horizon N] [--ticks T (every formulation; default: the script's)] [--centroidal-per-robot host|device]
       [--out PATH | --out -]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpc_benchmark_amd.pipeline import CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem

B = 64
G = 9.81
SCRIPT_TICKS = {"kinodynamic": 820, "centroidal": 420, "fulldynamic": 1000}
STEADY = slice(100, 200)
CENTROIDAL_WALK = {}   # --centroidal-per-robot: per_instance / generator of the centroidal pipeline's walk (every robot plans from its own soles)


def make_pipeline(model, N, T):
    kw = dict(batch=B, walk={}, sigma_q=0.005, sigma_v=0.01, tick_reuse=True)
    if model == "kinodynamic":
        p = KinodynamicPipeline(KinodynamicProblem(horizon=N), perturb=True, **kw)
    elif model == "centroidal":
        p = CentroidalPipeline(CentroidalProblem(horizon=N), **dict(kw, walk=dict(CENTROIDAL_WALK)))
    else:
        p = FullDynamicPipeline(FullDynamicsProblem(horizon=N), **kw)
    p.mpc.prepare_schedule(T + 16)
    p.cold_solve()
    p.mpc.enable_failure_isolation(auto_revive=False)
    return p


def run(model, N, T, metrics=False):
    """-> (per-period wall times [ms], the metric rows or None, robots whose MPC was lost, total mass)"""
    p = make_pipeline(model, N, T)
    if metrics:
        p.sim.metrics({})
    ms = []
    for _ in range(T):
        t0 = time.perf_counter()
        p.tick()
        ms.append((time.perf_counter() - t0) * 1e3)
    met = p.sim.read_metrics() if metrics else None
    lost = np.isin(np.arange(B), [b for (_, b, _, _) in p.mpc.lost])
    mass = sum(i.mass for i in p.model.inertias)
    return np.array(ms), met, lost, mass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--ticks", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "locomotion_metrics.txt"))
    ap.add_argument("--centroidal-per-robot", choices=["host", "device"], default=None,
                    help="the centroidal pipeline plans every robot's footholds from its own measured soles (enable_walk(per_instance=True, generator=...))")
    ap.add_argument("models", nargs="*", default=["kinodynamic", "centroidal", "fulldynamic"])
    a = ap.parse_args()
    if a.centroidal_per_robot:
        CENTROIDAL_WALK.update(per_instance=True, generator=a.centroidal_per_robot)
    N = a.horizon
    rows, cost = [], []
    for model in a.models:
        T = a.ticks or SCRIPT_TICKS[model]
        ms_off, _, _, _ = run(model, N, min(T, STEADY.stop))
        ms_on, m, lost, mass = run(model, N, T, True)
        fallen = (m["fall_step"] >= 0) | lost
        fs = m["fall_step"][m["fall_step"] >= 0]
        fell = "%2d of %2d (%2d lost; fall_step min %s, median %s)" % (int(fallen.sum()), B, int(lost.sum()), "%d" % fs.min() if fs.size else "-",
                                                                       "%d" % np.median(fs) if fs.size else "-")
        up = ~fallen
        if not up.any():  # (nobody is left to average over)
            rows.append("%-12s | %4d | %s | " % (model, T, fell) + " | ".join(["-"] * 9))
        else:
            d = np.linalg.norm(m["com_last"][:, :2] - m["com_first"][:, :2], axis=1)
            cot = m["energy"] / (mass * G * d)
            rms_lz = np.sqrt(m["h_ang_z_sq"] / m["steps"])
            share = m["cop_outside"][up].sum() / max(1.0, m["cop_steps"][up].sum())
            rows.append("%-12s | %4d | %s | %6.1f | %7.1f | %6.3f | %6.3f | %6.2f %% | %+7.2f | %6.2f | %6.2f | %6.3f" % (
                model, T, fell, np.mean(m["energy"][up] / m["time"][up]), np.mean(m["energy"][up]), np.mean(d[up]), np.mean(cot[up]),
                100.0 * share, 1e3 * np.percentile(m["margin_min"][up], 5), np.max(m["peak_h_lin"][up]), np.max(m["peak_h_ang"][up]),
                np.mean(rms_lz[up])))
        off, on = np.percentile(ms_off[STEADY], 50), np.percentile(ms_on[STEADY], 50)
        cost.append("%-12s ms per MPC period, p50 over periods %d - %d: metrics off %.3f, on %.3f (%+.3f)" % (model, STEADY.start, STEADY.stop - 1, off, on, on - off))
        print(rows[-1], "\n", cost[-1], flush=True)
    lines = ["Locomotion metrics of the three formulations (tools/locomotion_metrics.py, N = %d): %d robots each, perturbed (sigma_q 0.005, sigma_v 0.01), "
             "the scripts' walks, unpushed, device loops, reduced model, MI355X.  Read once per run from the simulator handle's metrics "
             "(mpc_sim_metrics, defaults: 1 N, plot.py's 0.1 x 0.05 m box, fall 0.2 m / 0.02 m)." % (N, B), "",
             "Columns over the robots that did not fall: mean power = energy / time [W] (mean over robots), energy [J] (mean), distance walked = |CoM xy "
             "last - first| [m] (mean), cost of transport E / (m g d) (mean), share of the CoP steps outside the support box (all their steps), "
             "margin_min [mm] (5th percentile over robots), peak |h_lin| [N s] and |h_ang| [N m s] (max over robots), RMS L_z [N m s] (mean).", "",
             "formulation  | MPC periods | fallen (fall_step >= 0 or MPC lost) | mean power | energy | distance | CoT | CoP outside | margin_min p5 | "
             "peak h_lin | peak h_ang | RMS L_z"] + rows + ["", "Cost (the same runs; metrics off: a run of its own over the first %d periods):" % STEADY.stop] + cost
    text = "\n".join(lines) + "\n"
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
