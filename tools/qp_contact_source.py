"""Developer tool (GPU box): what the contact source of the low-level QPs (``contact_source=``, mpc_qp_contact_source, include/mpc_qp_contacts.h) does
to the closed-loop walks under the unilateral contact rule.  64 perturbed robots per run on the device loops, the three sources side by side:

  kinodynamic flat    the kinodynamic script's walk at N = 100 through two landings (320 periods)
  centroidal N=40     the centroidal walk at N = 40 for 150 periods (the fall at the landing recorded in profiles/sim_contacts.txt)
  centroidal N=100    the centroidal walk at N = 100 for 210 periods
  kinodynamic stairs  the shared staircase of tools/stairs_walk.py with swing_apex 0.35, the whole schedule

Per run: robots fallen (mpc_sim_metrics), MPC instances lost (failure isolation: a robot whose MPC fails sits the rest out), lift-offs and touchdowns per
robot (more than the schedule has: chatter), for every scheduled take-off the delay of the plant's lift-off and for every scheduled landing the plant's
last touchdown against it (from the rows of the rule, read between the periods), the counts of plan against plant summed over the robots
(``qp_contacts()``: robot-steps with s, p = 00, 01 (the plant holds a foot the plan has in the air), 10 (the plan stands on a foot the plant has released),
11), and p50 ms per MPC period over periods 20 .. T-1 (the reads between the periods not timed).

``--cost``: ms per MPC period of both device loops, 64 robots, N = 100, as tools/sim_contacts_cost.py measures it, for the sources named by ``--sources``;
a build of the parent commit is measured beside it with ``MPC_HIP_LIBRARY=<that build> python tools/qp_contact_source.py --cost --sources none``
(``none``: the pipelines are built without the argument).  For the time of k_pipe_contact_states per launch run
``rocprofv3 --kernel-trace --stats -d DIR -- python tools/qp_contact_source.py --cost --sources both --ticks 30``.
usage: python tools/qp_contact_source.py [--walks ...] [--sources schedule plant both] [--out PATH] [--cost [--ticks T]]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from mpc_benchmark_amd.pipeline import CentroidalPipeline, KinodynamicPipeline
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem
from stairs_walk import Z_HEIGHT, staircase

B = 64
WALKS = {  # name: (pipeline, horizon, periods (None: the whole schedule), stairs)
    "kinodynamic-flat": ("kinodynamic", 100, 320, False),
    "centroidal-40": ("centroidal", 40, 150, False),
    "centroidal-100": ("centroidal", 100, 210, False),
    "kinodynamic-stairs": ("kinodynamic", 100, None, True),
}


def make_pipeline(model, N, T, source, stairs=False, rule=True):
    pd = KinodynamicProblem(horizon=N) if model == "kinodynamic" else CentroidalProblem(horizon=N)
    if T is None:
        T = len(pd.contact_phases) - N
    kw = dict(batch=B, walk={}, sigma_q=0.005, sigma_v=0.01, tick_reuse=True, contact_rule={} if rule else None)
    if stairs:
        boxes, _, xf = staircase(pd)
        kw.update(walk=dict(z_height=Z_HEIGHT, x_forward=xf, swing_apex=0.35), terrain=boxes)
    if source != "none":
        kw["contact_source"] = source
    p = KinodynamicPipeline(pd, perturb=True, **kw) if model == "kinodynamic" else CentroidalPipeline(pd, **kw)
    p.mpc.prepare_schedule(T + 16)
    p.cold_solve()
    p.mpc.enable_failure_isolation(auto_revive=False)
    return p, T


def walk(name, source):
    """-> lines of the report"""
    model, N, T, stairs = WALKS[name]
    p, T = make_pipeline(model, N, T, source, stairs)
    p.sim.metrics({})
    S = p.substeps
    sched, prev_cs = [], (True, True)              # (period, foot, "off" / "on") of the schedule the low-level loop works with
    events = [[[] for _ in range(2)] for _ in range(B)]   # per robot and foot: (kind, step) of the plant
    prev = p.sim.read_contacts()
    ms = []
    for t in range(T):
        cs = tuple(bool(c) for c in p.contact_state())
        for f in range(2):
            if cs[f] != prev_cs[f]:
                sched.append((t, f, "on" if cs[f] else "off"))
        prev_cs = cs
        t0 = time.perf_counter()
        p.tick()
        ms.append((time.perf_counter() - t0) * 1e3)
        r = p.sim.read_contacts()
        for kind, cnt, last in (("off", "liftoffs", "last_liftoff"), ("on", "touchdowns", "last_touchdown")):
            for b, f in zip(*np.nonzero(r[cnt] > prev[cnt])):
                events[b][f].append((kind, float(r[last][b, f])))   # (several in one period: the last one's step; the counters below keep the number)
        prev = r
    met, q = p.sim.read_metrics(), p.qp_contacts()
    fallen = met["fall_step"] >= 0
    lost = sorted({b for (_, b, _, _) in p.mpc.lost})
    n_off, n_on = sum(1 for e in sched if e[2] == "off"), sum(1 for e in sched if e[2] == "on")
    lo, td = prev["liftoffs"].sum(axis=1), prev["touchdowns"].sum(axis=1)
    c = q["counts"].sum(axis=0).sum(axis=0)
    out = ["  %-18s %-8s %d periods: fallen %d of %d%s ; MPC instances lost %d ; p50 %.3f ms per period" % (
        name, source, T, int(fallen.sum()), B, "" if not fallen.any() else " (first at step %d, median %d)" % (met["fall_step"][fallen].min(), np.median(met["fall_step"][fallen])),
        len(lost), np.percentile(np.array(ms)[20:], 50)),
           "      lift-offs per robot min %d median %d max %d (scheduled %d) ; touchdowns min %d median %d max %d (scheduled %d) ; robots with more of either than scheduled: %d" % (
               lo.min(), np.median(lo), lo.max(), n_off, td.min(), np.median(td), td.max(), n_on, int(np.sum((lo > n_off) | (td > n_on)))),
           "      plan against plant, robot-steps (s p): 00 %d, 01 %d (the plant holds a foot the plan has in the air), 10 %d (the plan stands on a released foot), 11 %d%s" % (
               c[0], c[1], c[2], c[3], " (nothing is read from the plant with this source)" if source in ("schedule", "none") else "")]
    for k, (t, f, kind) in enumerate(sched):
        nxt = next((t2 for (t2, f2, _) in sched[k + 1:] if f2 == f), T)
        got = []
        for b in range(B):
            if kind == "off":   # the first lift-off of this foot from 5 periods before the scheduled take-off to its scheduled landing
                steps = [s for (kd, s) in events[b][f] if kd == "off" and S * (t - 5) <= s < S * nxt]
                got.append(steps[0] if steps else np.nan)
            else:               # the last touchdown of this foot between its scheduled take-off and its next one
                before = max((t2 for (t2, f2, kd2) in sched[:k] if f2 == f and kd2 == "off"), default=0)
                steps = [s for (kd, s) in events[b][f] if kd == "on" and S * before <= s < S * nxt]
                got.append(steps[-1] if steps else np.nan)
        got = np.array(got)
        ok = np.isfinite(got)
        d = (got[ok] - S * t) / S
        out.append("      scheduled %s of the %s foot at period %d: %s by %d of %d robots%s" % (
            "take-off" if kind == "off" else "landing", "LR"[f], t, "lift-off" if kind == "off" else "last touchdown", int(ok.sum()), B,
            "" if not ok.any() else ", %+.1f / %+.1f / %+.1f periods (min / median / max) against the schedule" % (d.min(), np.median(d), d.max())))
    return out


def cost(model, source, N, T):
    p, _ = make_pipeline(model, N, T, source)
    ms = []
    for _ in range(T):
        t0 = time.perf_counter()
        p.tick()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.percentile(np.array(ms)[20:], 50))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walks", nargs="*", default=list(WALKS))
    ap.add_argument("--sources", nargs="*", default=["schedule", "plant", "both"])
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--ticks", type=int, default=80)
    ap.add_argument("--models", nargs="*", default=["kinodynamic", "centroidal"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    if a.cost:
        for model in a.models:
            for source in a.sources:
                say("cost %-12s %-8s %s: p50 %.3f ms per MPC period over periods 20 - %d (N = 100, %d robots, contact rule on)" % (
                    model, source, os.environ.get("MPC_HIP_LIBRARY", "this build"), cost(model, source, 100, a.ticks), a.ticks - 1, B))
    else:
        say("QP contact source (tools/qp_contact_source.py): %d robots per run, perturbed (sigma_q 0.005, sigma_v 0.01), device loops, reduced model, contact "
            "rule on, MI355X." % B)
        for name in a.walks:
            for source in a.sources:
                for s in walk(name, source):
                    say(s)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
