"""Developer tool (GPU box): the push experiment of the three scripts (commented out there: device.apply_force(f_disturbance, [0, 0, 0]) on MPC ticks
160 - 170, theta = 3 pi / 2) as one measured sweep over 64 robots per formulation: 8 directions x 8 magnitudes from 0 to twice the script's force.

  kinodynamic   KinodynamicPipeline, device loop (mpc_qp_low_level_steps), push armed per period (mpc_sim_set_push), 300 N in the script
  centroidal    CentroidalPipeline, device loop (mpc_qp_ikid_low_level_steps), the same, 100 N in the script
  fulldynamic   EnsembleMPC closed loop (mpc_simulate_push: the force at the base origin), 300 N in the script
  fulldynamic_pipeline  (opt-in: name it on the command line) FullDynamicPipeline, device loop (mpc_feedback_low_level_steps), 300 N in the script

The pipelines push at the script's point, the world origin (width 6); the full-dynamics loop at the base origin, the only form mpc_simulate_push has.
The pipelines' 1 kHz response comes from the simulator record (mpc_sim_record); the full-dynamics loop is sampled once per MPC period.
Per robot: recovered or fallen (fallen: the base more than 0.2 m below its start, or both soles more than 2 cm above theirs, or a non-finite state, or its
MPC solve failed — failure isolation, the robot sits the rest of the run out),
the peak CoM deviation from the unpushed run of the same robot, the peak centroidal momentum (linear, N s; angular, N m s).  Per pipeline: ms per MPC
period with record off (unpushed, and push armed) and with record on.  usage: python tools/push_recovery.py [N] [T_END] [models...]

PUSH_RECOVERY_CONTACT_RULE=1 (opt-in): the pipelines' simulator with the unilateral contact rule on the device (``contact_rule={}``: every robot's feet
decided by its own state, mpc_sim_contacts) instead of the schedule's contact set; the default models are then the three pipelines (kinodynamic,
centroidal, fulldynamic_pipeline), and the EnsembleMPC closed loop (fulldynamic), which has no torque-driven simulator, is refused.

PUSH_RECOVERY_CENTROIDAL_PER_ROBOT=host|device (opt-in; 1 = device): the centroidal pipeline plans every robot's footholds from the soles of its own
measured state (``walk=dict(per_instance=True, generator=...)``) instead of one plan for all 64: a pushed robot steps from where it stands."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpc_benchmark_amd.pipeline import PUSH_FORCE, PUSH_THETA, PUSH_TICKS, CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline, centroidal_state
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem
from mpc_benchmark_amd.robot import minipin as pin

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100
T_END = int(sys.argv[2]) if len(sys.argv) > 2 else 200
RULE = os.environ.get("PUSH_RECOVERY_CONTACT_RULE", "") not in ("", "0")
MODELS = sys.argv[3:] or (["kinodynamic", "centroidal", "fulldynamic_pipeline"] if RULE else ["kinodynamic", "centroidal", "fulldynamic"])
if RULE and "fulldynamic" in MODELS:
    sys.exit("PUSH_RECOVERY_CONTACT_RULE: the EnsembleMPC closed loop (fulldynamic) has no torque-driven simulator; name fulldynamic_pipeline")
KW = {"contact_rule": {}} if RULE else {}
PER_ROBOT = os.environ.get("PUSH_RECOVERY_CENTROIDAL_PER_ROBOT", "")
if PER_ROBOT not in ("", "0", "1", "host", "device"):
    sys.exit("PUSH_RECOVERY_CENTROIDAL_PER_ROBOT: host, device (or 1), or unset")
CENTROIDAL_WALK = {} if PER_ROBOT in ("", "0") else dict(per_instance=True, generator=("host" if PER_ROBOT == "host" else "device"))
B = 64
DIRS = 8
MAGS = 8


def grid(fd):
    """robot r = 8 i + j: direction theta_i = theta_script + i 2 pi / 8, magnitude j / 7 * 2 fd"""
    th = PUSH_THETA + 2 * np.pi * np.arange(DIRS) / DIRS
    mag = np.linspace(0.0, 2.0 * fd, MAGS)
    f = np.zeros((B, 3))
    for i in range(DIRS):
        for j in range(MAGS):
            f[MAGS * i + j] = mag[j] * np.array([np.cos(th[i]), np.sin(th[i]), 0.0])
    return f, th, mag


def make_pipeline(model):
    if model == "kinodynamic":
        p = KinodynamicPipeline(KinodynamicProblem(horizon=N), batch=B, walk={}, perturb=True, sigma_q=0.005, sigma_v=0.01, tick_reuse=True, **KW)
    elif model == "fulldynamic_pipeline":
        from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
        p = FullDynamicPipeline(FullDynamicsProblem(horizon=N), batch=B, walk={}, sigma_q=0.005, sigma_v=0.01, tick_reuse=True, **KW)
    else:
        p = CentroidalPipeline(CentroidalProblem(horizon=N), batch=B, walk=dict(CENTROIDAL_WALK), sigma_q=0.005, sigma_v=0.01, tick_reuse=True, **KW)
    p.mpc.prepare_schedule(T_END + 16)
    p.cold_solve()
    p.mpc.enable_failure_isolation(auto_revive=False)  # (a robot whose MPC fails sits the rest out and counts as fallen)
    return p


def run_pipeline(model, f, record):
    """-> per-tick wall times [ms], and with ``record`` the 1 kHz traces (steps, B, ...) of com, momentum, base height, sole heights"""
    p = make_pipeline(model)
    push = None if f is None else np.concatenate([f, np.zeros((B, 3))], axis=1)  # (force, world origin): device.apply_force(f, [0, 0, 0])
    if record:
        p.sim.record(p.substeps)
    ms, tr = [], {"com": [], "momentum": [], "z": [], "soles": [], "finite": []}
    for t in range(T_END):
        on = PUSH_TICKS[0] <= p.mpc.tick < PUSH_TICKS[1]
        t0 = time.perf_counter()
        p.tick(push=push if on else None)
        if record:
            r = p.sim.read_record()
        ms.append((time.perf_counter() - t0) * 1e3)
        if record:
            tr["com"].append(r["com"]); tr["momentum"].append(r["momentum"]); tr["z"].append(r["x"][:, :, 2]); tr["soles"].append(r["sole_p"][:, :, :, 2])
            tr["finite"].append(np.all(np.isfinite(r["x"]), axis=2))
    if record:
        p.sim.record(0)
        tr = {k: np.concatenate(v, axis=0) for k, v in tr.items()}
        tr["lost"] = np.isin(np.arange(B), [b for (_, b, _, _) in p.mpc.lost])
    return np.array(ms), tr


def run_fulldynamic(f):
    from mpc_benchmark_amd.ensemble import EnsembleMPC
    from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
    pd = FullDynamicsProblem(horizon=N)
    e = EnsembleMPC(pd, batch=B, sigma_q=0.005, sigma_v=0.01, tick_reuse=True)
    e.prepare_schedule(T_END + 16)
    e.cold_solve()
    e.enable_walk()
    e.enable_failure_isolation(auto_revive=False)
    m = pd.robot.model
    data = m.createData()
    feet = list(pd.robot.foot_frame_ids)
    ms, tr = [], {"com": [], "momentum": [], "z": [], "soles": [], "finite": []}
    for t in range(T_END):
        on = PUSH_TICKS[0] <= e.tick < PUSH_TICKS[1]
        t0 = time.perf_counter()
        if on and f is not None:
            e.native.simulate_push(10, pd.dt / 10, f)
        else:
            e.native.simulate(10, pd.dt / 10)
        e.step()
        x = e.native.get_x0()
        ms.append((time.perf_counter() - t0) * 1e3)
        c = centroidal_state(m, x)
        soles = np.zeros((B, 2))
        for b in range(B):
            pin.framesForwardKinematics(m, data, x[b, :m.nq])
            soles[b] = [data.oMf[fi].translation[2] for fi in feet]
        tr["com"].append(c[None, :, :3]); tr["momentum"].append(c[None, :, 3:]); tr["z"].append(x[None, :, 2]); tr["soles"].append(soles[None])
        tr["finite"].append(np.all(np.isfinite(x), axis=1)[None])
    tr = {k: np.concatenate(v, axis=0) for k, v in tr.items()}
    tr["lost"] = np.isin(np.arange(B), [b for (_, b, _, _) in e.lost])
    return np.array(ms), tr


def verdict(tr, ref):
    z0, s0 = tr["z"][0], tr["soles"][0]
    with np.errstate(invalid="ignore"):
        fallen = ((tr["z"] < z0 - 0.2).any(axis=0) | ((tr["soles"] > s0 + 0.02).all(axis=2)).any(axis=0) | ~tr["finite"].all(axis=0) | tr["lost"])
    dcom = np.nanmax(np.linalg.norm(tr["com"] - ref["com"], axis=2), axis=0)
    hl = np.nanmax(np.linalg.norm(tr["momentum"][:, :, :3], axis=2), axis=0)
    ha = np.nanmax(np.linalg.norm(tr["momentum"][:, :, 3:], axis=2), axis=0)
    return fallen, dcom, hl, ha


lines = ["Push recovery sweep (tools/push_recovery.py %d %d): 64 robots per formulation, 8 directions (theta = 3 pi / 2 + k pi / 4) x 8 magnitudes (0 .. 2 fd,"
         " evenly spaced), pushed on MPC ticks %d - %d, run to tick %d, the script's walk, N = %d, MI355X." % (N, T_END, PUSH_TICKS[0], PUSH_TICKS[1] - 1, T_END, N), ""]
if RULE:
    lines[0] = "PUSH_RECOVERY_CONTACT_RULE=1 " + lines[0]
    lines.insert(1, "Simulator: the unilateral contact rule on the device (contact_rule={}: release after 5 pulling steps at -1 N, catch within 5 mm of "
                    "the ground at the lower initial foothold), not the schedule's contact set.")
if CENTROIDAL_WALK:
    lines.insert(1, "Centroidal pipeline: every robot's footholds planned from its own measured soles (PUSH_RECOVERY_CENTROIDAL_PER_ROBOT, generator %s)." % CENTROIDAL_WALK["generator"])
for model in MODELS:
    fd = PUSH_FORCE["fulldynamic" if model == "fulldynamic_pipeline" else model]
    f, th, mag = grid(fd)
    W, P = slice(100, PUSH_TICKS[0]), slice(*PUSH_TICKS)
    lines.append("== %s (script: %g N, %s) ==" % (model, fd, "device loop, push at the world origin" if model != "fulldynamic"
                                                   else "EnsembleMPC closed loop, mpc_simulate_push at the base origin"))
    if model == "fulldynamic":
        ms_off, ref = run_fulldynamic(None)
        ms_push, tr = run_fulldynamic(f)
        lines.append("ms per MPC period (10 simulator sub-steps + tick): p50 %.2f (ticks 100 - %d) ; ticks %d - %d: p50 %.2f unpushed, %.2f pushed" % (
            np.percentile(ms_off[W], 50), PUSH_TICKS[0] - 1, PUSH_TICKS[0], PUSH_TICKS[1] - 1, np.percentile(ms_off[P], 50), np.percentile(ms_push[P], 50)))
    else:
        ms_off, _ = run_pipeline(model, None, False)                 # unpushed, record off
        ms_zero, _ = run_pipeline(model, np.zeros((B, 3)), False)    # a zero push armed on ticks 160 - 170, record off: the cost of arming
        ms_ref, ref = run_pipeline(model, None, True)                # unpushed, record on: the reference traces, the cost of recording
        ms_push, tr = run_pipeline(model, f, True)                   # the sweep, record on
        lines.append("ms per MPC period, record off: p50 %.2f (ticks 100 - %d) ; ticks %d - %d: p50 %.2f unarmed, %.2f with a (zero) push armed" % (
            np.percentile(ms_off[W], 50), PUSH_TICKS[0] - 1, PUSH_TICKS[0], PUSH_TICKS[1] - 1, np.percentile(ms_off[P], 50), np.percentile(ms_zero[P], 50)))
        lines.append("ms per MPC period, record on (every step recorded, read once per period): p50 %.2f (ticks 100 - %d, unpushed) ; the sweep's pushed "
                     "ticks %d - %d: p50 %.2f" % (np.percentile(ms_ref[W], 50), PUSH_TICKS[0] - 1, PUSH_TICKS[0], PUSH_TICKS[1] - 1, np.percentile(ms_push[P], 50)))
    fallen, dcom, hl, ha = verdict(tr, ref)
    lines.append("fallen: %d of %d robots" % (int(fallen.sum()), B))
    lines.append("per magnitude (8 directions each): N | fallen | over the recovered robots: peak CoM deviation from the unpushed run [mm] max | peak |h_lin| "
                 "[N s] max | peak |h_ang| [N m s] max")
    all_up = 0.0
    for j in range(MAGS):
        rows = [MAGS * i + j for i in range(DIRS) if not fallen[MAGS * i + j]]
        nf = DIRS - len(rows)
        if rows:
            lines.append("  %7.1f | %d | %8.2f | %7.2f | %7.2f" % (mag[j], nf, 1e3 * dcom[rows].max(), hl[rows].max(), ha[rows].max()))
        else:
            lines.append("  %7.1f | %d | - | - | -" % (mag[j], nf))
        if not fallen[[MAGS * i + k for i in range(DIRS) for k in range(j + 1)]].any():
            all_up = mag[j]
    lines.append("every robot recovered up to: %.1f N (%s)" % (all_up, model))
    lines.append("per robot (rows: direction; columns: the 8 magnitudes; peak CoM deviation from the unpushed run in mm, or fallen):")
    for i in range(DIRS):
        lines.append("  %5.0f deg: " % np.degrees(th[i] % (2 * np.pi)) + " ".join("fallen" if fallen[MAGS * i + j] else "%.1f" % (1e3 * dcom[MAGS * i + j])
                                                                               for j in range(MAGS)))
    lines.append("")
    print("\n".join(lines[-(MAGS + DIRS + 8):]), flush=True)
out = os.environ.get("PUSH_RECOVERY_OUT")
if out:
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
