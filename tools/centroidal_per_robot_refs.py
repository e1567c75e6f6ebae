"""Developer tool (GPU box): what per-robot foot references cost and change in the centroidal pipeline (CentroidalPipeline(walk=dict(per_instance=True,
generator=...)), include/mpc_walk_poses.h).  64 perturbed robots, N = 100, the reduced model, device loops.

  timing MODE   ms per MPC period at p50 over periods 20 - 79 (as tools/sim_contacts_cost.py takes it), MODE = shared | host | device.  One figure per
                process, so that a build of another commit can be timed in the same session (``MPC_HIP_LIBRARY=<that build> ... timing shared``).
  walk          the script's whole schedule (420 periods), shared against per-robot references (device generator), the schedule-driven plant and the
                unilateral contact rule (``contact_rule={}``): falls by the device metrics (mpc_sim_metrics), MPC instances lost, advance of the
                centre of mass, where the soles ended and how far apart across the robots.
  profile       130 periods with the device generator, for ``rocprofv3 --kernel-trace --stats -d DIR -- python tools/centroidal_per_robot_refs.py profile``
                (k_walk_poses: one launch per period; the last 29 are replanning ticks, which run the forward kinematics).
usage: python tools/centroidal_per_robot_refs.py timing shared|host|device | walk [--ticks T] | profile"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpc_benchmark_amd.pipeline import CentroidalPipeline, centroidal_state
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.robot import minipin as pin

B, N = 64, 100
WALKS = {"shared": {}, "host": dict(per_instance=True), "device": dict(per_instance=True, generator="device")}


def make_pipeline(mode, T, rule=None):
    p = CentroidalPipeline(CentroidalProblem(horizon=N), batch=B, walk=dict(WALKS[mode]), sigma_q=0.005, sigma_v=0.01, tick_reuse=True, contact_rule=rule)
    p.mpc.prepare_schedule(T + 16)
    p.cold_solve()
    p.mpc.enable_failure_isolation(auto_revive=False)
    return p


def timing(mode, T=80):
    p = make_pipeline(mode, T)
    ms = []
    for _ in range(T):
        t0 = time.perf_counter()
        p.tick()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms)[20:]
    print("timing %-6s library %s: p50 %.3f ms per MPC period (p10 %.3f, p90 %.3f) over periods 20 - %d, %d robots, N = %d" % (
        mode, os.environ.get("MPC_HIP_LIBRARY", "(this build)"), np.percentile(ms, 50), np.percentile(ms, 10), np.percentile(ms, 90), T - 1, B, N), flush=True)


def walk(T):
    for rule in (None, {}):
        for mode in ("shared", "device"):
            p = make_pipeline(mode, T, rule)
            p.sim.metrics({})
            rb = p.pd.robot
            com0 = centroidal_state(p.model, p.x)[:, :3]
            for _ in range(T):
                p.tick()
            met = p.sim.read_metrics()
            fall = np.asarray(met["fall_step"])
            fell = fall >= 0
            lost = sorted((t, b) for (t, b, _, _) in p.mpc.lost)
            ok = ~fell & ~np.isin(np.arange(B), [b for _, b in lost]) & np.all(np.isfinite(p.x), axis=1)
            adv = centroidal_state(p.model, p.x[ok])[:, 0] - com0[ok, 0] if ok.any() else np.zeros(1)
            (_, Lp), (_, Rp) = pin.frame_placements_batch(rb.model, p.x[ok][:, :rb.model.nq], rb.foot_frame_ids)
            print("walk %-6s references, %-13s %d periods: fallen %d of %d (first fall in period %s) ; MPC instances lost %d (first at tick %s) ; of the %d robots "
                  "standing: CoM advance %.3f .. %.3f m ; final soles x left %.3f .. %.3f right %.3f .. %.3f m ; spread across robots (max - min) left "
                  "%.1f x %.1f mm, right %.1f x %.1f mm" % (
                      mode, "contact rule," if rule is not None else "schedule," , T, int(fell.sum()), B, (int(fall[fell].min()) // p.substeps if fell.any() else "-"), len(lost),
                      (lost[0][0] if lost else "-"), int(ok.sum()), adv.min(), adv.max(), Lp[:, 0].min(), Lp[:, 0].max(), Rp[:, 0].min(), Rp[:, 0].max(),
                      1e3 * np.ptp(Lp[:, 0]), 1e3 * np.ptp(Lp[:, 1]), 1e3 * np.ptp(Rp[:, 0]), 1e3 * np.ptp(Rp[:, 1])), flush=True)


def profile(T=130):
    p = make_pipeline("device", T)
    for _ in range(T):
        p.tick()
    print("profile: %d periods with the device generator" % T)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "walk"
    if what == "timing":
        timing(sys.argv[2])
    elif what == "profile":
        profile()
    else:
        walk(int(sys.argv[sys.argv.index("--ticks") + 1]) if "--ticks" in sys.argv else 420)
