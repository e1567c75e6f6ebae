"""Developer tool (GPU box): the cost of the unilateral contact rule of the torque-driven simulator (mpc_sim_contacts, include/mpc_sim_contacts.h) in the
three device loops, 64 robots each, the scripts' walks, N = 100: ms per MPC period (one tick: the ten low-level steps and the solve) at p50 over
periods 20 .. T-1, with the rule off (the schedule's contact set) and on (``contact_rule={}``), and the rows of the rule at the end of the run-with-rule.

``--complete``: the complete model (38 dofs) where the problem has it.  For the time of k_sim_contacts per launch, run this under
``rocprofv3 --kernel-trace --stats -d DIR -- python tools/sim_contacts_cost.py --ticks 30 --models fulldynamic --complete``.
usage: python tools/sim_contacts_cost.py [--horizon N] [--ticks T] [--models kinodynamic centroidal fulldynamic] [--complete] [--out PATH]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpc_benchmark_amd.pipeline import CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.common import Robot
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem

B = 64


def make_pipeline(model, N, T, complete, rule):
    kw = dict(batch=B, walk={}, sigma_q=0.005, sigma_v=0.01, tick_reuse=True, contact_rule=rule)
    if model == "kinodynamic":
        p = KinodynamicPipeline(KinodynamicProblem(horizon=N, complete_model=complete), perturb=True, **kw)
    elif model == "centroidal":
        p = CentroidalPipeline(CentroidalProblem(horizon=N, robot=Robot(complete=complete)), **kw)
    else:
        p = FullDynamicPipeline(FullDynamicsProblem(horizon=N, complete_model=complete), **kw)
    p.mpc.prepare_schedule(T + 16)
    p.cold_solve()
    p.mpc.enable_failure_isolation(auto_revive=False)
    return p


def run(model, N, T, complete, rule):
    p = make_pipeline(model, N, T, complete, rule)
    ms = []
    for _ in range(T):
        t0 = time.perf_counter()
        p.tick()
        ms.append((time.perf_counter() - t0) * 1e3)
    rows = p.sim.read_contacts() if rule is not None else None
    return np.array(ms), rows, len(p.mpc.lost)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--ticks", type=int, default=80)
    ap.add_argument("--models", nargs="*", default=["kinodynamic", "centroidal", "fulldynamic"])
    ap.add_argument("--complete", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["Contact rule cost (tools/sim_contacts_cost.py --horizon %d --ticks %d%s): %d robots per pipeline, perturbed (sigma_q 0.005, sigma_v 0.01), "
             "the scripts' walks, device loops, %s model, MI355X.  ms per MPC period (ten low-level steps + the solve), p50 over periods 20 - %d." % (
                 a.horizon, a.ticks, " --complete" if a.complete else "", B, "complete" if a.complete else "reduced", a.ticks - 1), ""]
    for model in a.models:
        off, _, lost_off = run(model, a.horizon, a.ticks, a.complete, None)
        on, rows, lost_on = run(model, a.horizon, a.ticks, a.complete, {})
        s = slice(20, a.ticks)
        lines.append("%-12s rule off %.3f ms, on %.3f ms (%+.3f) ; MPC instances lost: off %d, on %d ; rule rows after %d periods: right lift-offs "
                     "%d of %d robots (max %d), touchdowns %d (max %d), left lift-offs %d" % (
                         model, np.percentile(off[s], 50), np.percentile(on[s], 50), np.percentile(on[s], 50) - np.percentile(off[s], 50), lost_off, lost_on,
                         a.ticks, int((rows["liftoffs"][:, 1] > 0).sum()), B, int(rows["liftoffs"][:, 1].max()), int((rows["touchdowns"][:, 1] > 0).sum()),
                         int(rows["touchdowns"][:, 1].max()), int((rows["liftoffs"][:, 0] > 0).sum())))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
