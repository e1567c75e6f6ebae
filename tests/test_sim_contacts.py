"""The unilateral contact rule of the torque-driven simulator (include/mpc_sim_contacts.h) without a GPU: the header, the bindings and the libraries
agree, the oracle refuses the rule, and the numpy mirror (mpc_benchmark_amd/contact_rule.py) is the headless BulletRobot's rule: on hand-made
sequences, and step by step against BulletRobot itself on the oracle while one sole is lifted and set down again."""
import ctypes
import os
import re

import numpy as np
import pytest

from mpc_benchmark_amd import _capi
from mpc_benchmark_amd import contact_rule as cr
from mpc_benchmark_amd.pipeline import CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline, build_torque_simulator
from mpc_benchmark_amd.problems.common import Robot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_CONTACTS = ("mpc_sim_contacts", "mpc_sim_contacts_read", "mpc_sim_contacts_set", "mpc_sim_contacts_width")


def _header():
    return open(os.path.join(ROOT, "include", "mpc_sim_contacts.h")).read()


def test_header_declares_the_entry_points_the_bindings_know():
    from tests.test_abi_library import _declared_functions
    assert _declared_functions("mpc_sim_contacts.h") == sorted(_capi._SIM_CONTACTS_SIGNATURES) == list(SIM_CONTACTS)
    for other in ("mpc_abi.h", "mpc_sim_ext.h", "mpc_sim_metrics.h"):
        assert not set(SIM_CONTACTS) & set(_declared_functions(other))


def test_width_fields_and_config_match_the_header():
    text = _header()
    assert int(re.search(r"#define MPC_SIM_CONTACTS_WIDTH (\d+)", text).group(1)) == 41 == cr.WIDTH
    assert len({n for n, _ in cr.FIELDS}) == len(cr.FIELDS)
    body = re.search(r"typedef struct mpc_sim_contacts_config \{(.*?)\} mpc_sim_contacts_config;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(double|int32_t)\s+([a-z_]+)\s*;", body)
    assert [n for _, n in fields] == list(cr.DEFAULTS) + ["reserved"] == [n for n, _ in _capi.MpcSimContactsConfig._fields_]
    ctypes_of = {"double": ctypes.c_double, "int32_t": ctypes.c_int32}
    for (ty, name), (cname, cty) in zip(fields, _capi.MpcSimContactsConfig._fields_):
        assert ctypes_of[ty] is cty, name
    assert ctypes.sizeof(_capi.MpcSimContactsConfig) == 3 * 8 + 2 * 4
    o = 0
    for name, w in cr.FIELDS:  # the row layout documented in the header is FIELDS
        assert re.search(r"\b%d\b[^\n]*\b%s\b" % (o, name), text), (o, name)
        o += w


def test_hip_library_exports_the_entry_points():
    lib = ctypes.CDLL(_capi.HIP_LIBRARY_PATH)
    for name in SIM_CONTACTS:
        assert hasattr(lib, name), name


def test_oracle_refuses_the_rule(oracle_lib):
    for name in SIM_CONTACTS:
        assert not hasattr(oracle_lib, name)
    sim, tables = build_torque_simulator(oracle_lib, Robot(), 2, 1e-3, 0)
    sim.set_stage(0, *tables[(True, True)])
    for call in (lambda: sim.contacts({}), lambda: sim.contacts(None), lambda: sim.read_contacts(),
                 lambda: sim.set_contacts(np.zeros((2, cr.WIDTH)))):
        with pytest.raises(RuntimeError, match="not exported by this library"):
            call()


def test_config_defaults_and_unknown_keys():
    c = cr.config()
    assert c == {"ground_z": 0.0, "ground_tol": 5e-3, "release_force": 1.0, "release_steps": 5}
    assert cr.config({"release_steps": 3.0}, ground_z=0.1) == {"ground_z": 0.1, "ground_tol": 5e-3, "release_force": 1.0, "release_steps": 3}
    assert cr.config({"ground_z": -1.0}, ground_z=0.1)["ground_z"] == -1.0
    with pytest.raises(ValueError, match="unknown"):
        cr.config({"ground_height": 0.0})


# -- the mirror on hand-made sequences ----------------------------------------------------------------------------------------------------------
I3 = np.eye(3)


def _rows(B=1):
    return cr.reset_rows(np.broadcast_to(I3, (B, 2, 3, 3)), np.array([[0.0, 0.1, 0.0], [0.0, -0.1, 0.0]]))


def _step(rows, z, fz, R=None, p=None, **cfg):
    B = rows.shape[0]
    z = np.broadcast_to(np.asarray(z, dtype=float), (B, 2))
    R = np.broadcast_to(I3, (B, 2, 3, 3)) if R is None else R
    p = np.concatenate([np.zeros((B, 2, 2)), z[..., None]], axis=-1) if p is None else p
    return cr.step(rows, z, np.broadcast_to(np.asarray(fz, dtype=float), (B, 2)), R, p, cfg)


def test_reset_rows():
    u = cr.unpack(_rows(3))
    np.testing.assert_array_equal(u["in_contact"], 1.0)
    np.testing.assert_array_equal(u["last_touchdown"], -1.0)
    np.testing.assert_array_equal(u["last_liftoff"], -1.0)
    np.testing.assert_array_equal(u["steps"], 0.0)
    np.testing.assert_array_equal(u["anchor_R"], np.broadcast_to(I3, (3, 2, 3, 3)))
    np.testing.assert_array_equal(u["anchor_p"][0], [[0.0, 0.1, 0.0], [0.0, -0.1, 0.0]])


def test_four_pulling_steps_and_a_recovery_do_not_release():
    r = _rows()
    for _ in range(4):
        r = _step(r, [0.0, 0.0], [100.0, -50.0])
    assert cr.unpack(r)["pulling"][0].tolist() == [0.0, 4.0]
    r = _step(r, [0.0, 0.0], [100.0, -0.5])   # (above -release_force: an unloaded sole rests)
    for _ in range(4):
        r = _step(r, [0.0, 0.0], [100.0, -50.0])
    u = cr.unpack(r)
    assert u["in_contact"][0].tolist() == [1.0, 1.0] and u["pulling"][0].tolist() == [0.0, 4.0] and u["liftoffs"][0].tolist() == [0.0, 0.0]


def test_five_pulling_steps_release():
    r = _rows()
    for k in range(5):
        r = _step(r, [0.0, 0.0], [100.0, -50.0])
        assert cr.unpack(r)["in_contact"][0].tolist() == ([1.0, 1.0] if k < 4 else [1.0, 0.0])
    u = cr.unpack(r)
    assert u["pulling"][0].tolist() == [0.0, 0.0] and u["liftoffs"][0].tolist() == [0.0, 1.0] and u["last_liftoff"][0].tolist() == [-1.0, 4.0]
    assert u["steps"][0] == 5.0


def test_the_last_contact_is_never_released():
    r = _rows()
    for _ in range(5):
        r = _step(r, [0.0, 0.0], [100.0, -50.0])
    for _ in range(20):
        r = _step(r, [0.0, 0.03], [-80.0, 0.0])
    u = cr.unpack(r)
    assert u["in_contact"][0].tolist() == [1.0, 0.0] and u["pulling"][0][0] == 20.0 and u["liftoffs"][0].tolist() == [0.0, 1.0]


def test_both_feet_pulling_in_one_step_release_foot_0_only():
    r = _rows()
    for _ in range(5):
        r = _step(r, [0.0, 0.0], [-50.0, -50.0])
    u = cr.unpack(r)
    assert u["in_contact"][0].tolist() == [0.0, 1.0] and u["pulling"][0].tolist() == [0.0, 5.0] and u["liftoffs"][0].tolist() == [1.0, 0.0]


def test_release_steps_is_a_setting():
    r = _rows()
    r = _step(r, [0.0, 0.0], [100.0, -50.0], release_steps=1)
    assert cr.unpack(r)["in_contact"][0].tolist() == [1.0, 0.0]
    r = _rows()
    r = _step(r, [0.0, 0.0], [100.0, -5.0], release_steps=1, release_force=10.0)
    assert cr.unpack(r)["in_contact"][0].tolist() == [1.0, 1.0]


def _released_right():
    r = _rows()
    for _ in range(5):
        r = _step(r, [0.0, 0.0], [100.0, -50.0])
    return r


def test_lifted_then_caught_within_the_tolerance():
    r = _released_right()
    r = _step(r, [0.0, 0.004], [100.0, 0.0])   # within 2 tol: not lifted, not caught (it did not sink)
    u = cr.unpack(r)
    assert u["in_contact"][0].tolist() == [1.0, 0.0] and u["lifted"][0].tolist() == [0.0, 0.0]
    r = _step(r, [0.0, 0.0101], [100.0, 0.0])  # above 2 tol: lifted
    assert cr.unpack(r)["lifted"][0].tolist() == [0.0, 1.0]
    r = _step(r, [0.0, 0.0052], [100.0, 0.0])  # between tol and 2 tol, coming down: still free
    assert cr.unpack(r)["in_contact"][0].tolist() == [1.0, 0.0]
    r = _step(r, [0.0, 0.005], [100.0, 0.0])   # z <= ground_z + tol and lifted: caught
    u = cr.unpack(r)
    assert u["in_contact"][0].tolist() == [1.0, 1.0] and u["touchdowns"][0].tolist() == [0.0, 1.0] and u["last_touchdown"][0].tolist() == [-1.0, 8.0]
    assert u["lifted"][0].tolist() == [0.0, 1.0]   # (BulletRobot clears it on the release, not on the catch)
    assert u["z_prev"][0].tolist() == [0.0, 0.005]


def test_caught_when_sinking_without_having_lifted():
    r = _released_right()
    r = _step(r, [0.0, 0.003], [100.0, 0.0])
    r = _step(r, [0.0, 0.001], [100.0, 0.0])    # coming down, above the plane: free
    assert cr.unpack(r)["in_contact"][0].tolist() == [1.0, 0.0]
    r = _step(r, [0.0, -0.0005], [100.0, 0.0])  # below the plane and lower than before: caught
    assert cr.unpack(r)["in_contact"][0].tolist() == [1.0, 1.0]
    r = _released_right()
    r = _step(r, [0.0, -0.002], [100.0, 0.0])   # (the release step left z_prev = 0: sinking)
    assert cr.unpack(r)["in_contact"][0].tolist() == [1.0, 1.0]
    r = _released_right()
    r[0, cr.O_ZPREV + 1] = -0.004
    r = _step(r, [0.0, -0.002], [100.0, 0.0])   # below the plane but rising, not lifted: stays free
    assert cr.unpack(r)["in_contact"][0].tolist() == [1.0, 0.0]


def test_the_anchor_is_flattened_to_yaw_at_ground_z():
    r = _released_right()
    yaw, tilt = 0.3, 0.2
    Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(tilt), -np.sin(tilt)], [0.0, np.sin(tilt), np.cos(tilt)]])
    R = np.stack([I3, Rz @ Rx])[None]
    p = np.array([[[0.0, 0.1, 0.01], [0.25, -0.12, 0.008]]])
    r = _step(r, [0.0, 0.025], [100.0, 0.0], ground_z=0.01)   # lifted above ground_z + 2 tol
    r = _step(r, [0.0, 0.008], [100.0, 0.0], R=R, p=p, ground_z=0.01)
    u = cr.unpack(r)
    assert u["in_contact"][0].tolist() == [1.0, 1.0]
    np.testing.assert_allclose(u["anchor_R"][0, 1], Rz, atol=1e-15)
    np.testing.assert_array_equal(u["anchor_p"][0, 1], [0.25, -0.12, 0.01])
    np.testing.assert_array_equal(u["anchor_p"][0, 0], [0.0, 0.1, 0.0])   # (the other anchor untouched)


def test_robots_are_independent():
    r = _rows(3)
    fz = np.array([[100.0, -50.0], [-50.0, 100.0], [100.0, 100.0]])
    for _ in range(5):
        r = cr.step(r, np.zeros((3, 2)), fz, np.broadcast_to(I3, (3, 2, 3, 3)), np.zeros((3, 2, 3)))
    assert cr.unpack(r)["in_contact"].tolist() == [[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]


# -- the mirror against BulletRobot on the oracle: one sole lifted and set down -------------------------------------------------------------------
def lift_torques(robot, q0, k, amp=150.0, span=15, kp=300.0, kd=3.0):
    """Joint torques of step k of the lift sequence (also the GPU tests'): a posture PD, plus ``amp`` N m flexing the right hip and knee for ``span`` steps
    and extending them for the next ``span`` (the right sole pulls, is released, lifts, comes down and is caught)."""
    m = robot.model if hasattr(robot, "model") else robot
    nq = m.nq
    x = robot.x
    tau = kp * (q0[7:] - x[7:nq]) - kd * x[nq + 6:]
    names = list(m.names[2:])
    s = -1.0 if k < span else (1.0 if k < 2 * span else 0.0)
    tau[names.index("leg_right_3_joint")] += s * amp
    tau[names.index("leg_right_4_joint")] -= s * amp
    return tau


def test_mirror_follows_bullet_robot_on_the_oracle(oracle_lib):
    from mpc_benchmark_amd.bullet_robot import BulletRobot
    from mpc_benchmark_amd.robot import minipin as pin
    rb = Robot()
    m = rb.model
    robot = BulletRobot([n for n in m.names], None, None, 1e-3, m, library=oracle_lib)
    robot.initializeJoints(rb.x0[:m.nq])
    q0 = robot.x[:robot.model.nq].copy()
    seen = []
    orig = robot._update_contacts
    robot._update_contacts = lambda wr: (seen.append(np.array(wr)), orig(wr))
    mm, data = robot.model, robot.model.createData()
    cfg = {"ground_z": robot.ground_z, "ground_tol": robot.ground_tol, "release_force": robot.release_force, "release_steps": robot.release_steps}
    anchors = [robot.data.oMf[f] for f in robot.frame_ids]
    rows = cr.reset_rows(np.array([[M.rotation for M in anchors]]), np.array([[M.translation for M in anchors]]))
    flags = []
    for k in range(60):
        robot.execute(lift_torques(robot, q0, k))
        pin.framesForwardKinematics(mm, data, robot.x[:mm.nq])
        R = np.array([[data.oMf[f].rotation for f in robot.frame_ids]])
        p = np.array([[data.oMf[f].translation for f in robot.frame_ids]])
        rows = cr.step(rows, p[..., 2], seen[-1][None, :, 2], R, p, cfg)
        u = cr.unpack(rows)
        assert u["in_contact"][0].tolist() == [float(c) for c in robot.in_contact], k
        assert u["lifted"][0].tolist() == [float(c) for c in robot._lifted], k
        assert u["pulling"][0].tolist() == [float(c) for c in robot._pulling], k
        flags.append(tuple(robot.in_contact))
    assert (True, False) in flags and flags[-1] == (True, True)        # released, then caught
    u = cr.unpack(rows)
    assert u["liftoffs"][0].tolist() == [0.0, 1.0] and u["touchdowns"][0].tolist() == [0.0, 1.0]
    for i, pose in enumerate(robot._contact_pose):                      # the catch re-captured the same anchor
        np.testing.assert_allclose(u["anchor_R"][0, i], pose.rotation, atol=1e-12)
        np.testing.assert_allclose(u["anchor_p"][0, i], pose.translation, atol=1e-12)


# -- the pipelines: with a rule, the schedule no longer sets the simulator's contacts --------------------------------------------------------------
class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s)" % name)


@pytest.mark.parametrize("cls", [KinodynamicPipeline, CentroidalPipeline, FullDynamicPipeline])
def test_pipelines_with_a_rule_leave_the_simulator_stage_alone(cls):
    p = cls.__new__(cls)
    p.contact_rule = {}
    p.sim = _Untouchable()
    p._sim_mask = None
    for mask in ((True, False), (False, True), (True, True)):
        p._set_sim_contacts(mask)
