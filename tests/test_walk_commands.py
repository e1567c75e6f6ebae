"""A walk command per robot (include/mpc_walk_commands.h) without a GPU: the table's definition (``references.walk_commands`` / ``stopped_commands``),
the numpy generator with a table against one scalar ``FootTrajectory`` per robot, the host generator of an ensemble against the foothold rule itself,
and what is refused.  The device side is held to these in tests/test_gpu_walk_commands.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mpc_benchmark_amd import _capi, references
from mpc_benchmark_amd.ensemble import EnsembleMPC
from mpc_benchmark_amd.pipeline import CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem
from mpc_benchmark_amd.robot import minipin as pin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALK_COMMANDS = ("mpc_walk_get_commands", "mpc_walk_poses_get_commands", "mpc_walk_poses_set_commands", "mpc_walk_set_commands")

# three robots: the full-dynamics script's default walk (0 m steps, apex 0.15), and two that differ from it and from each other in step length, lateral
# step, yaw per step, height per step and apex
ARGS = dict(x_forward=np.array([0.0, 0.12, 0.25]), y_forward=np.array([0.0, 0.03, -0.02]), foot_yaw=np.array([0.0, 0.08, -0.05]),
            y_gap=0.18, z_height=np.array([0.0, 0.04, 0.1]), swing_apex=np.array([0.15, 0.1, 0.2]))
B = 3


def three_rows():
    return references.walk_commands(B, **ARGS)


def row_args(b):
    return {k: (float(v[b]) if np.ndim(v) else float(v)) for k, v in ARGS.items()}


def yaw_of(R):
    return np.arctan2(R[..., 1, 0], R[..., 0, 0])


def rz(yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def plan_identities(plan, cmd, right_first):
    """Worst violation of the foothold rule (walk_beside of csrc/walk_generator.h, FootTrajectory._plan_*) on a plan [B][4][12] = start / final pose of the
    left foot, start / final pose of the right foot, made with robot b's row of ``cmd`` at a take-off of the right (``right_first``) or the left foot."""
    worst = 0.0
    for b in range(plan.shape[0]):
        P = [(plan[b, i, :9].reshape(3, 3), plan[b, i, 9:]) for i in range(4)]
        sL, fL, sR, fR = P
        tl, tr, rd = cmd[b, 0:3], cmd[b, 3:6], cmd[b, 6:15].reshape(3, 3)
        if right_first:   # the right foot beside the measured left one, the left foot beside that foothold
            errs = [fR[1] - sL[1] - rz(yaw_of(sL[0])) @ tr, fR[0] - rd @ sL[0], fL[1] - fR[1] - rz(yaw_of(fR[0])) @ tl, fL[0] - fR[0]]
        else:             # the left foot beside the measured right one, the right foot beside that foothold
            errs = [fL[1] - sR[1] - rz(yaw_of(sR[0])) @ tl, fL[0] - sR[0], fR[1] - fL[1] - rz(yaw_of(fL[0])) @ tr, fR[0] - rd @ fL[0]]
        worst = max(worst, max(float(np.max(np.abs(e))) for e in errs))
    return worst


# -- 1. the definition -------------------------------------------------------------------------------------------------------------------------------
def test_row_layout_and_the_bits_of_the_shared_configuration():
    assert references.WALK_COMMAND_WIDTH == 16 == _capi.WALK_COMMAND_WIDTH
    cmd = three_rows()
    assert cmd.shape == (B, 16) and cmd.dtype == np.float64
    for b in range(B):
        a = row_args(b)
        assert cmd[b, 0:3].tolist() == [a["x_forward"], a["y_gap"], a["z_height"]]
        assert cmd[b, 3:6].tolist() == [a["x_forward"], -a["y_gap"] - a["y_forward"], a["z_height"]]
        assert np.array_equal(cmd[b, 6:15].reshape(3, 3), references.yaw_rotation(a["foot_yaw"]))
        assert cmd[b, 15] == a["swing_apex"]
        lf, rf = pin.SE3(np.eye(3), np.zeros(3)), pin.SE3(np.eye(3), np.zeros(3))
        gen = references.FootTrajectory(lf, rf, 8, 4, 6, a["swing_apex"], a["x_forward"], a["y_forward"], a["foot_yaw"], a["y_gap"], a["z_height"])
        want = np.concatenate([gen.translationLeft, gen.translationRight, gen.rotationDiff.ravel(), [gen.swing_apex]])
        assert np.array_equal(cmd[b], want)
    # scalars are every robot's; the scripts' arguments (0.3 m steps, the defaults otherwise)
    shared = references.walk_commands(4, 0.3)
    gen = references.FootTrajectory(lf, rf, 8, 4, 6, 0.15, 0.3, 0.0, 0.0, 0.18, 0.0)
    for b in range(4):
        assert np.array_equal(shared[b], np.concatenate([gen.translationLeft, gen.translationRight, gen.rotationDiff.ravel(), [0.15]]))


def test_stopped_commands_is_update_forward_per_robot():
    cmd = three_rows()
    stopped = references.stopped_commands(cmd, -0.01)
    assert stopped is not cmd and np.array_equal(cmd, three_rows())   # (a new table)
    for b in range(B):
        a = row_args(b)
        gen = references.FootTrajectory(pin.SE3(np.eye(3), np.zeros(3)), pin.SE3(np.eye(3), np.zeros(3)), 8, 4, 6, a["swing_apex"], a["x_forward"],
                                        a["y_forward"], a["foot_yaw"], a["y_gap"], a["z_height"])
        gen.updateForward(0, 0, a["y_gap"], a["y_forward"], -0.01, 0, a["swing_apex"])
        assert np.array_equal(stopped[b], np.concatenate([gen.translationLeft, gen.translationRight, gen.rotationDiff.ravel(), [gen.swing_apex]]))
    assert np.array_equal(references.stopped_commands(stopped, -0.01), stopped)   # (stopping twice changes nothing)


def test_errors_of_the_definition():
    with pytest.raises(ValueError):
        references.walk_commands(3, np.zeros(4))                    # B mismatch
    with pytest.raises(ValueError):
        references.walk_commands(3, np.zeros((3, 1)))               # wrong shape
    with pytest.raises(ValueError):
        references.walk_commands(3, 0.1, foot_yaw=np.array([0.0, np.nan, 0.0]))
    with pytest.raises(ValueError):
        references.walk_commands(3, np.inf)
    with pytest.raises(ValueError):
        references.stopped_commands(np.zeros((3, 15)), 0.0)
    bad = three_rows()
    bad[1, 4] = np.nan
    with pytest.raises(ValueError):
        references.stopped_commands(bad, 0.0)
    g = batch_generator()
    for table in (np.zeros((B, 15)), np.zeros((B + 1, 16)), bad, np.zeros(16)):
        with pytest.raises(ValueError):
            g.set_commands(table)
    assert g.commands is None


# -- 2. the numpy generator with a table against one scalar generator per robot --------------------------------------------------------------------------
T_SS, T_DS, N = 8, 4, 6


def start_poses():
    return pin.SE3(rz(0.02), np.array([0.0, 0.09, 0.0])), pin.SE3(rz(-0.01), np.array([0.0, -0.09, 0.0]))


def batch_generator():
    lf, rf = start_poses()
    bc = lambda M: (np.tile(M.rotation, (B, 1, 1)), np.tile(M.translation, (B, 1)))
    (LR, Lp), (RR, Rp) = bc(lf), bc(rf)
    return references.FootTrajectoryBatch(LR, Lp, RR, Rp, T_SS, T_DS, N, 0.15, 0.3, 0.0, 0.0, 0.18, 0.0)


def measured_poses(t):
    """soles of three robots at tick t: a yaw, an offset and a drift per robot -> ((LR, Lp), (RR, Rp))"""
    lf, rf = start_poses()
    out = []
    for M, side in ((lf, 1.0), (rf, -1.0)):
        R = np.array([rz(0.05 * b - 0.03 + 2e-3 * t * side) @ M.rotation for b in range(B)])
        p = np.array([M.translation + [0.01 * b + 3e-3 * t, -0.02 * b + 1e-3 * t * side, 1e-3 * b] for b in range(B)])
        out.append((R, p))
    return out


def flat(M):
    return np.concatenate([np.asarray(M.rotation, dtype=float).reshape(-1), np.asarray(M.translation, dtype=float)])


def test_batch_generator_with_a_table_equals_one_scalar_generator_per_robot():
    """One walk of a step per foot (planning windows of both feet, two take-offs, two landings) and the ticks after it, on which the table is stopped
    as the scripts stop the walk: robot b's [N, 12] references are those of ``FootTrajectory`` built with robot b's arguments on robot b's poses."""
    cmd = three_rows()
    gen, untouched, same = batch_generator(), batch_generator(), batch_generator()
    gen.set_commands(cmd)
    lf, rf = start_poses()
    singles = []
    for b in range(B):
        a = row_args(b)
        singles.append(references.FootTrajectory(lf.copy(), rf.copy(), T_SS, T_DS, N, a["swing_apex"], a["x_forward"], a["y_forward"], a["foot_yaw"],
                                                 a["y_gap"], a["z_height"]))
    phases = references.walking_contact_phases(T_DS, T_SS, 1, N)
    lists = [list(v) for v in references.contact_event_times(phases, N)]
    seen = set()
    worst = spread = 0.0
    for t in range(len(phases) + N + 4):
        ev = references.update_timings(lists[3], lists[2], lists[1], lists[0])
        takeoff_RF, takeoff_LF, land_RF, land_LF = ev
        stop = land_LF == -1 and land_RF == -1 and t > T_DS   # the walk is over
        if stop:
            gen.set_commands(references.stopped_commands(gen.commands, -0.01))
            seen.add("stop")
        seen |= {name for name, on in (("plan_R", 0 <= takeoff_RF < T_DS), ("plan_L", 0 <= takeoff_LF < T_DS), ("takeoff_R", takeoff_RF == 0),
                                       ("takeoff_L", takeoff_LF == 0), ("land_R", land_RF == 0), ("land_L", land_LF == 0)) if on}
        (LR, Lp), (RR, Rp) = measured_poses(t)
        Lb, Rb = gen.updateTrajectory(*ev, LR, Lp, RR, Rp)
        assert Lb.shape == Rb.shape == (B, N, 12)
        spread = max(spread, float(np.max(np.abs(Rb[0, :, 9] - Rb[2, :, 9]))))
        for b in range(B):
            a = row_args(b)
            if stop:
                singles[b].updateForward(0, 0, a["y_gap"], a["y_forward"], -0.01, 0, a["swing_apex"])
            L, R = singles[b].updateTrajectory(*ev, pin.SE3(LR[b], Lp[b]), pin.SE3(RR[b], Rp[b]))
            worst = max(worst, float(np.max(np.abs(Lb[b] - np.array([flat(M) for M in L])))), float(np.max(np.abs(Rb[b] - np.array([flat(M) for M in R])))))
        assert worst <= 1e-12, (t, worst)
        # no table: nothing changed (a generator that never saw one, and one whose table was taken away again before its first tick)
        if t == 0:
            same.set_commands(cmd)
            same.set_commands(None)
        U, S = untouched.updateTrajectory(*ev, LR, Lp, RR, Rp), same.updateTrajectory(*ev, LR, Lp, RR, Rp)
        assert np.array_equal(U[0], S[0]) and np.array_equal(U[1], S[1])
    assert seen == {"plan_R", "plan_L", "takeoff_R", "takeoff_L", "land_R", "land_L", "stop"}, seen
    assert spread > 0.2   # (the robots did walk different gaits: steps of 0 and of 0.25 m)
    with pytest.raises(ValueError, match="stopped_commands"):
        gen.updateForward(0, 0, 0.18, 0.0, -0.01, 0, 0.15)
    untouched.updateForward(0, 0, 0.18, 0.0, -0.01, 0, 0.15)   # (without a table: as before)
    print("batch generator with a table vs scalar generators: %.2e" % worst)


# -- 3. the host generator of an ensemble -----------------------------------------------------------------------------------------------------------------
def test_host_generator_plans_every_robot_with_its_row(oracle_lib):
    """The plan of the first planning tick against the foothold rule itself (no second generator): robot b's next footholds lie beside its stance foot
    by ITS offsets, turned by ITS rot_diff.  Then the end of the walk: the scripts' updateForward rule becomes the stopped table, once."""
    cmd = three_rows()
    e = EnsembleMPC(FullDynamicsProblem(horizon=8), batch=B, library=oracle_lib, sigma_q=0.0, sigma_v=0.0)
    e.options.riccati_legs, e.options.num_threads = 1, 8
    e.native.set_options(e.options)
    e.prepare_schedule(8)
    e.cold_solve(max_iters=20)
    e.enable_walk(per_instance=True, commands=cmd)
    assert np.array_equal(e.walk_commands(), cmd)
    T_ds = e._walk["spec"]["T_DS"]
    checked = None
    for t in range(45):   # (the first take-off enters the double-support window within the first T_DS + N ticks)
        lists = [list(v) for v in e._walk["lists"]]
        takeoff_RF, takeoff_LF, land_RF, land_LF = references.update_timings(lists[3], lists[2], lists[1], lists[0])
        e.step()
        if 0 <= takeoff_RF < T_ds or 0 <= takeoff_LF < T_ds:
            g = e._walk["batch"]
            plan = np.stack([np.concatenate([P[0].reshape(B, 9), P[1]], axis=1) for P in (g.sL, g.fL, g.sR, g.fR)], axis=1)
            right_first = 0 <= takeoff_RF < T_ds
            assert right_first != (0 <= takeoff_LF < T_ds)
            checked = plan_identities(plan, cmd, right_first)
            assert checked <= 1e-12, (t, checked)
            wrong = plan_identities(plan, cmd[::-1], right_first)
            assert wrong > 1e-2   # (the check does tell the rows apart)
            break
    assert checked is not None
    # the walk is over: every countdown has run out, the forward rule fires on every tick
    for lst in e._walk["lists"]:
        del lst[:]
    uploads = []
    apply = e._apply_walk_commands
    e._apply_walk_commands = lambda c: (uploads.append(c.copy()), apply(c))[1]
    for _ in range(3):
        e.step()
    want = references.stopped_commands(cmd, e._walk["spec"]["forward_z_left"])
    assert len(uploads) == 1 and np.array_equal(uploads[0], want) and np.array_equal(e.walk_commands(), want)
    assert np.array_equal(e._walk["batch"].tL, want[:, 0:3]) and np.array_equal(e._walk["batch"].swing_apex, want[:, 15])
    del e._apply_walk_commands
    e.set_walk_commands(None)
    assert e.walk_commands() is None and e._walk["batch"].commands is None and e._walk["batch"].tL.shape == (3,)
    print("host generator, foothold identities per robot: %.2e" % checked)


def test_contact_pose_problem_takes_a_table_on_the_host_generator(oracle_lib):
    """The centroidal problem's per-robot references with a table (host generator, measured soles): the right foothold planned in the window before the
    first take-off obeys robot b's row."""
    from tests.test_centroidal_walk_per_robot import T0, generator_plan, make_ensemble, measured_states
    cmd = references.walk_commands(B, np.array([0.2, 0.0, 0.1]), foot_yaw=np.array([0.0, 0.05, -0.05]), swing_apex=np.array([0.15, 0.1, 0.2]))
    e = make_ensemble(oracle_lib, per_instance=True, commands=cmd)
    for t in range(T0, T0 + 8):   # (the planning window of the right foot opens at tick 21)
        e._walk["x_measured_all"] = measured_states(e.pd, t)
        e.plan_tick()
        e.solve_tick()
    assert e._walk["replanning"]
    assert plan_identities(generator_plan(e), cmd, True) <= 1e-12


# -- 4. misuse ----------------------------------------------------------------------------------------------------------------------------------------
def test_commands_need_per_instance_references_and_the_hip_library_on_the_device(oracle_lib):
    cmd = three_rows()
    for name in WALK_COMMANDS:
        assert not hasattr(oracle_lib, name)
    e = EnsembleMPC(FullDynamicsProblem(horizon=8), batch=B, library=oracle_lib, sigma_q=0.0, sigma_v=0.0)
    with pytest.raises(ValueError, match="per_instance=True"):
        e.enable_walk(commands=cmd)
    with pytest.raises(RuntimeError, match="not exported"):
        e.enable_walk(per_instance=True, generator="device", commands=cmd)
    with pytest.raises(ValueError):
        e.enable_walk(per_instance=True, commands=cmd[:2])
    with pytest.raises(ValueError, match="floor"):
        e.enable_walk(per_instance=True, floor=True, commands=cmd)   # rows that climb have no flat floor
    assert e._walk is None
    with pytest.raises(ValueError):
        e.set_walk_commands(cmd)   # no walk yet
    for call in (lambda: e.native.walk_set_commands(cmd), lambda: e.native.walk_get_commands(), lambda: e.native.walk_poses_set_commands(None),
                 lambda: e.native.walk_poses_get_commands()):
        with pytest.raises(NotImplementedError, match="mpc_walk_commands.h"):
            call()
    c = EnsembleMPC(CentroidalProblem(horizon=8), batch=B, library=oracle_lib)
    with pytest.raises(RuntimeError, match="not exported"):
        c.enable_walk(per_instance=True, generator="device", commands=cmd)
    flat_rows = references.walk_commands(B, np.array([0.0, 0.1, 0.2]))
    e.enable_walk(per_instance=True, commands=flat_rows)
    with pytest.raises(ValueError, match="climb"):
        e.set_walk_commands(cmd)   # the posture reference of this walk does not follow the feet
    assert np.array_equal(e.walk_commands(), flat_rows)


@pytest.mark.parametrize("pipeline,problem", [(KinodynamicPipeline, KinodynamicProblem), (CentroidalPipeline, CentroidalProblem), (FullDynamicPipeline, FullDynamicsProblem)])
def test_pipelines_check_the_table_early(pipeline, problem):
    class NoLibrary:   # (nothing of it may be touched before the argument is refused)
        pass
    pd = problem(horizon=8)
    with pytest.raises(ValueError, match=pipeline.__name__):
        pipeline(pd, batch=B, library=NoLibrary(), walk=dict(commands=three_rows()))
    with pytest.raises(ValueError, match=pipeline.__name__):
        pipeline(pd, batch=B, library=NoLibrary(), walk=dict(per_instance=True, commands=three_rows()[:2]))


def test_header_compiles_as_c_and_agrees_with_the_bindings():
    from tests.test_abi_library import _declared_functions
    assert _declared_functions("mpc_walk_commands.h") == sorted(_capi._WALK_COMMANDS_SIGNATURES) == list(WALK_COMMANDS)
    for other in ("mpc_abi.h", "mpc_walk_poses.h", "mpc_sim_ext.h", "mpc_sim_terrain.h"):
        assert not set(WALK_COMMANDS) & set(_declared_functions(other))
    text = open(os.path.join(ROOT, "include", "mpc_walk_commands.h")).read()
    assert int(re.search(r"#define MPC_WALK_COMMAND_WIDTH (\d+)", text).group(1)) == 16 == references.WALK_COMMAND_WIDTH
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = '#include "mpc_walk_commands.h"\nint width(void) { return MPC_WALK_COMMAND_WIDTH; }\nint (*set)(mpc_solver*, const double*) = mpc_walk_set_commands;\n'
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, text=True, check=True)


def test_hip_library_exports_the_entry_points():
    import ctypes
    lib = ctypes.CDLL(_capi.HIP_LIBRARY_PATH)
    for name in WALK_COMMANDS:
        assert hasattr(lib, name), name
