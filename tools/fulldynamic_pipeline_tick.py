"""Developer tool (GPU box): one MPC period of the full-dynamics pipeline (mpc_benchmark_amd/pipeline.py FullDynamicPipeline) for an ensemble of robots —
MPC tick + 10 x (feedback law, simulator step) — with the low-level loop inside the library (mpc_feedback_low_level_steps), record off and on, against
the host glue (numpy law, one mpc_simulate_torque per step) and against the closed loop inside the MPC's own handle (EnsembleMPC(closed_loop=(10, dt / 10)):
mpc_simulate, knot 0's model integrated from xs[0]).  Complete model, the script's walk, the bench's solver configuration (tick reuse, 4 legs).
usage: python tools/fulldynamic_pipeline_tick.py [B] [N] [ticks] ; HOST=0 skips the host glue and the closed-loop comparison (profiler runs)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpc_benchmark_amd.ensemble import EnsembleMPC
from mpc_benchmark_amd.pipeline import FullDynamicPipeline
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100
T = int(sys.argv[3]) if len(sys.argv) > 3 else 30
LEGS = 4
host = bool(int(os.environ.get("HOST", "1")))
pd = FullDynamicsProblem(horizon=N, complete_model=True)
p = FullDynamicPipeline(pd, batch=B, walk={}, sigma_q=0.005, sigma_v=0.01, tick_reuse=True)
p.mpc.options.riccati_legs = LEGS
p.mpc.native.set_options(p.mpc.options)
p.mpc.prepare_schedule(4 * T + 16)
p.cold_solve()
for _ in range(3):
    p.tick()


def periods(n, read=False, **kw):
    lat = []
    for _ in range(n):
        t0 = time.perf_counter()
        p.tick(**kw)
        if read:
            p.sim.read_record()
        lat.append((time.perf_counter() - t0) * 1e3)
    return np.array(lat)


dev = periods(T)
p.sim.record(p.substeps)
rec = periods(T, read=True)
p.sim.record(0)
# the low-level part alone (no MPC solve): one device-loop call of ten steps
cs = p.contact_state()
p._set_sim_contacts(cs)
p.low_level_loop(cs)
t0 = time.perf_counter()
for _ in range(10):
    p.low_level_loop(cs)
ll = (time.perf_counter() - t0) / 10 * 1e3
line = ("full-dynamics pipeline, complete model, N = %d, %d robots, tick reuse, %d legs: MPC period with the device loop p50 %.2f ms p90 %.2f ms ; "
        "with the record on (every step recorded, read once per period) p50 %.2f ms p90 %.2f ms ; low-level loop of one period (%d x (feedback law, "
        "simulator step), one synchronisation) %.3f ms" % (N, B, LEGS, np.percentile(dev, 50), np.percentile(dev, 90), np.percentile(rec, 50),
                                                             np.percentile(rec, 90), p.substeps, ll))
if host:
    hst = periods(max(1, T // 3), host_glue=True)
    p._fetch()
    t0 = time.perf_counter()
    for _ in range(p.substeps):
        p.low_level_step(cs)
    lh = (time.perf_counter() - t0) * 1e3
    line += " ; MPC period with the host glue p50 %.2f ms (its low-level loop %.2f ms)" % (np.percentile(hst, 50), lh)
print(line + " ; base heights %.4f .. %.4f" % (p.x[:, 2].min(), p.x[:, 2].max()), flush=True)
if host:
    del p
    e = EnsembleMPC(pd, batch=B, sigma_q=0.005, sigma_v=0.01, tick_reuse=True, closed_loop=(10, pd.dt / 10))
    e.options.riccati_legs = LEGS
    e.native.set_options(e.options)
    e.prepare_schedule(4 * T + 16)
    e.cold_solve()
    e.enable_walk()
    for _ in range(3):
        e.step()
    lat = []
    for _ in range(T):
        t0 = time.perf_counter()
        e.step()
        lat.append((time.perf_counter() - t0) * 1e3)
    print("EnsembleMPC(closed_loop=(10, dt / 10)), the same ensemble and solver configuration: MPC period (mpc_simulate of 10 sub-steps + tick) p50 %.2f ms "
          "p90 %.2f ms" % (np.percentile(lat, 50), np.percentile(lat, 90)), flush=True)
