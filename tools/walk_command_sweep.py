"""Developer tool (GPU box): which formulation still walks at which walk command?  One ensemble per formulation, one robot per command value
(``walk=dict(per_instance=True, commands=...)``, include/mpc_walk_commands.h): 64 values of ONE axis, everything else the script's walk.

  --axis step      step length x_forward: 0 .. 1.5 x the script's (kinodynamic 0.3 m, centroidal 0.2 m; the full-dynamics script steps in place: 0.2 m here)
  --axis yaw       foot yaw per step: 0 .. 0.3 rad, at the step length above
  --axis lateral   lateral step y_forward: 0 .. 0.1 m, at the step length above

  kinodynamic   KinodynamicPipeline, device loop, host generator (planned from every robot's measured state), 820 MPC periods
  centroidal    CentroidalPipeline, device loop, device generator (k_walk_poses reads the measurement where the loop kept it), 420 periods
  fulldynamic   FullDynamicPipeline, device loop, host generator, 1000 periods

Built as tools/locomotion_metrics.py builds them (64 perturbed robots, N = 100, the reduced model, failure isolation), with the unilateral contact rule
(``contact_rule={}``) and the device metrics (mpc_sim_metrics) on, over the script's schedule.  Per robot: the command, the distance the schedule's
swings command (x_forward (swings - 1/2): the first swing starts beside the stance foot), the distance walked (|CoM xy last - first|), the fall
verdict (fall_step >= 0 or the MPC lost), the energy and the worst CoP margin.  No threshold is set on the outcome.
usage: python tools/walk_command_sweep.py [--axis step|yaw|lateral] [--horizon N] [--ticks T] [--out PATH | --out -] [models...]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpc_benchmark_amd import references
from mpc_benchmark_amd.pipeline import CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem

B = 64
SCRIPT_TICKS = {"kinodynamic": 820, "centroidal": 420, "fulldynamic": 1000}
PROBLEM = {"kinodynamic": KinodynamicProblem, "centroidal": CentroidalProblem, "fulldynamic": FullDynamicsProblem}
PIPELINE = {"kinodynamic": KinodynamicPipeline, "centroidal": CentroidalPipeline, "fulldynamic": FullDynamicPipeline}
IN_PLACE_STEP = 0.2   # the nominal step length of a formulation whose script steps in place
AXES = {"step": ("x_forward", "m"), "yaw": ("foot_yaw", "rad"), "lateral": ("y_forward", "m")}


def command_table(axis, nominal):
    values = {"step": np.linspace(0.0, 1.5 * nominal, B), "yaw": np.linspace(0.0, 0.3, B), "lateral": np.linspace(0.0, 0.1, B)}[axis]
    kw = {"x_forward": nominal}
    kw[AXES[axis][0]] = values
    return values, references.walk_commands(B, **kw)


def swings_within(pd, ticks):
    """landings of the schedule's first `ticks` indices: the swings a run of that many periods completes"""
    ph = [tuple(c) for c in pd.contact_phases[:ticks]]
    return sum(1 for a, b in zip(ph[:-1], ph[1:]) if sum(a) == 1 and sum(b) == 2)


def run(model, axis, N, T):
    pd = PROBLEM[model](horizon=N)
    nominal = pd.walk_spec()["x_forward"] or IN_PLACE_STEP
    values, cmd = command_table(axis, nominal)
    walk = dict(per_instance=True, generator=("device" if model == "centroidal" else "host"), commands=cmd)
    kw = dict(batch=B, walk=walk, sigma_q=0.005, sigma_v=0.01, tick_reuse=True, contact_rule={})
    if model == "kinodynamic":
        kw["perturb"] = True
    p = PIPELINE[model](pd, **kw)
    p.mpc.prepare_schedule(T + 16)
    p.cold_solve()
    p.mpc.enable_failure_isolation(auto_revive=False)   # (a robot whose MPC fails sits the rest out and counts as fallen)
    p.sim.metrics({})
    ms = []
    for _ in range(T):
        t0 = time.perf_counter()
        p.tick()
        ms.append((time.perf_counter() - t0) * 1e3)
    m = p.sim.read_metrics()
    lost = np.isin(np.arange(B), [b for (_, b, _, _) in p.mpc.lost])
    return dict(values=values, cmd=cmd, m=m, lost=lost, ms=np.array(ms), swings=swings_within(pd, T), nominal=nominal, final=p.mpc.walk_commands())


def report(model, axis, N, T, r):
    m, x = r["m"], r["cmd"][:, 0]
    fallen = (m["fall_step"] >= 0) | r["lost"]
    walked = np.linalg.norm(m["com_last"][:, :2] - m["com_first"][:, :2], axis=1)
    commanded = x * max(0.0, r["swings"] - 0.5)
    name, unit = AXES[axis]
    up = np.flatnonzero(~fallen)
    lines = ["== %s: %s 0 .. %.3g %s over %d robots, step length %s, %d MPC periods (%d swings), N = %d ==" % (
        model, name, r["values"][-1], unit, B, "swept" if axis == "step" else "%.2f m" % r["nominal"], T, r["swings"], N)]
    first = np.flatnonzero(fallen)
    reach = "no robot fell" if not first.size else ("the first command fell" if first[0] == 0 else "every robot below %s = %.4f %s walked" % (name, r["values"][first[0]], unit))
    lines.append("fallen: %d of %d (%d lost their MPC) ; %s ; ms per MPC period p50 %.2f" % (int(fallen.sum()), B, int(r["lost"].sum()), reach, np.percentile(r["ms"], 50)))
    lines.append("robot | %s [%s] | commanded distance [m] | walked distance [m] | verdict (fall_step) | energy [J] | worst CoP margin [mm]" % (name, unit))
    for b in range(B):
        verdict = "walked" if not fallen[b] else ("lost" if m["fall_step"][b] < 0 else "fallen (%d)" % m["fall_step"][b])
        lines.append("  %2d | %7.4f | %6.3f | %6.3f | %-14s | %8.1f | %+7.2f" % (b, r["values"][b], commanded[b], walked[b], verdict, m["energy"][b], 1e3 * m["margin_min"][b]))
    moving = up[commanded[up] > 0]
    if moving.size:
        ratio = walked[moving] / commanded[moving]
        lines.append("over the %d robots that walked a command above 0: walked / commanded distance %.3f .. %.3f, energy %.1f .. %.1f J, worst CoP margin %+.2f mm" % (
            moving.size, ratio.min(), ratio.max(), m["energy"][moving].min(), m["energy"][moving].max(), 1e3 * m["margin_min"][moving].min()))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--axis", choices=sorted(AXES), default="step")
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--ticks", type=int, default=0, help="MPC periods of every formulation (default: the script's)")
    ap.add_argument("--out", default="-", help="a file for the table (profiles/walk_commands.txt keeps the measured one beside the benchmark record); default: standard output")
    ap.add_argument("models", nargs="*", default=["kinodynamic", "centroidal", "fulldynamic"])
    a = ap.parse_args()
    lines = ["Walk command sweep (tools/walk_command_sweep.py --axis %s --horizon %d%s): one robot per command value, %d robots per formulation, perturbed "
             "(sigma_q 0.005, sigma_v 0.01), contact rule and device metrics on, device loops, reduced model, MI355X." % (
                 a.axis, a.horizon, " --ticks %d" % a.ticks if a.ticks else "", B), ""]
    for model in a.models:
        T = a.ticks or SCRIPT_TICKS[model]
        part = report(model, a.axis, a.horizon, T, run(model, a.axis, a.horizon, T))
        print("\n".join(part[:2]), file=sys.stderr, flush=True)
        lines += part + [""]
    text = "\n".join(lines) + "\n"
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
