"""Developer tool (GPU box): one MPC period of the centroidal pipeline (mpc_benchmark_amd/pipeline.py CentroidalPipeline) for an ensemble of robots —
MPC tick + task errors + 10 x (centroidal state and feedback, IK + ID QP, simulator step) — with the low-level loop inside the library
(mpc_qp_ikid_low_level_steps) against the host glue (compute_ID_references, minipin's centre of mass and centroidal momentum, one library call per
QP and per simulator step).  usage: python tools/centroidal_pipeline_tick.py [B] [N] [ticks] ; HOST=0 skips the host-glue periods (profiler runs)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpc_benchmark_amd.pipeline import CentroidalPipeline
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100
T = int(sys.argv[3]) if len(sys.argv) > 3 else 30
host = bool(int(os.environ.get("HOST", "1")))
p = CentroidalPipeline(CentroidalProblem(horizon=N), batch=B, walk={}, sigma_q=0.005, sigma_v=0.01, tick_reuse=True)
p.mpc.prepare_schedule(2 * T + 16)
p.cold_solve()
for _ in range(3):
    p.tick()


def periods(host_glue, n):
    lat = []
    for _ in range(n):
        t0 = time.perf_counter()
        p.tick(host_glue=host_glue)
        lat.append((time.perf_counter() - t0) * 1e3)
    return np.array(lat)


dev = periods(False, T)
hst = periods(True, max(1, T // 3)) if host else None
# the low-level part alone (no MPC solve): the device loop, and the host glue's task errors + ten steps
cs, refs = p.contact_state(), p.foot_refs()
p._set_sim_contacts(cs)
p.low_level_loop(cs, refs)
t0 = time.perf_counter()
for _ in range(10):
    p.low_level_loop(cs, refs)
ll = (time.perf_counter() - t0) / 10 * 1e3
line = ("centroidal pipeline, reduced model, N = %d, %d robots: MPC period with the device loop p50 %.2f ms p90 %.2f ms ; low-level loop of one period "
        "(task errors + %d x (centroidal state and feedback, IK + ID QP assembled + solved, simulator step), one synchronisation) %.3f ms" % (
            N, B, np.percentile(dev, 50), np.percentile(dev, 90), p.substeps, ll))
if host:
    p._fetch()
    t0 = time.perf_counter()
    ik = p.qp.task_errors(p.x_prev, p.x_posture, refs, p.ref_dt, p.dH)
    te = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for _ in range(p.substeps):
        p.low_level_step(cs, ik)
    lh = (time.perf_counter() - t0) * 1e3
    line += " ; MPC period with the host glue p50 %.2f ms (its low-level loop %.2f ms: task errors %.2f ms + %d steps %.2f ms)" % (
        np.percentile(hst, 50), te + lh, te, p.substeps, lh)
print(line + " ; base heights %.4f .. %.4f" % (p.x[:, 2].min(), p.x[:, 2].max()))
