"""The box terrain under the contact rule of the torque-driven simulator (include/mpc_sim_terrain.h) without a GPU: the header, the bindings and the
libraries agree, the oracle refuses it, the height function and the staircase of mpc_benchmark_amd/contact_rule.py are what the header says, the rule
with a terrain is today's rule with the ground under the sole's origin in place of ground_z (bit for bit the same without one), the mirror follows
the headless BulletRobot's host rule on the oracle over a box, the metrics' fall verdict is taken above the ground, and the Python layers accept
or refuse a terrain as documented.  ``LIFTS`` / ``lift_boxes`` are the inputs of the GPU test of the kernel (tests/test_gpu_sim_terrain.py): their
conditions are checked here, robot by robot, with the host rule on the oracle."""
import ctypes
import os
import re

import numpy as np
import pytest

from mpc_benchmark_amd import _capi
from mpc_benchmark_amd import contact_rule as cr
from mpc_benchmark_amd import locomotion_metrics as lm
from mpc_benchmark_amd.pipeline import CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline, build_torque_simulator
from mpc_benchmark_amd.problems.common import Robot
from tests.test_sim_contacts import I3, _released_right, _rows, _step, lift_torques
from tests.test_sim_metrics import _synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_TERRAIN = ("mpc_sim_terrain", "mpc_sim_terrain_height", "mpc_sim_terrain_read")


# -- 1. header, bindings, libraries ------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_the_bindings_know():
    from tests.test_abi_library import _declared_functions
    assert _declared_functions("mpc_sim_terrain.h") == sorted(_capi._SIM_TERRAIN_SIGNATURES) == list(SIM_TERRAIN)
    for other in ("mpc_abi.h", "mpc_sim_ext.h", "mpc_sim_metrics.h", "mpc_sim_contacts.h"):
        assert not set(SIM_TERRAIN) & set(_declared_functions(other))


def test_defines_and_config_match_the_header():
    text = open(os.path.join(ROOT, "include", "mpc_sim_terrain.h")).read()
    assert int(re.search(r"#define MPC_SIM_TERRAIN_MAX_BOXES (\d+)", text).group(1)) == 16 == cr.TERRAIN_MAX_BOXES
    assert int(re.search(r"#define MPC_SIM_TERRAIN_BOX_WIDTH (\d+)", text).group(1)) == 5 == cr.TERRAIN_BOX_WIDTH
    body = re.search(r"typedef struct mpc_sim_terrain_config \{(.*?)\} mpc_sim_terrain_config;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(double|int32_t)\s+([a-z_]+)\s*;", body)
    assert fields == [("int32_t", "n_boxes"), ("int32_t", "per_robot")]
    assert [(n, t) for n, t in _capi.MpcSimTerrainConfig._fields_] == [("n_boxes", ctypes.c_int32), ("per_robot", ctypes.c_int32)]
    assert ctypes.sizeof(_capi.MpcSimTerrainConfig) == 8


def test_hip_library_exports_the_entry_points():
    lib = ctypes.CDLL(_capi.HIP_LIBRARY_PATH)
    for name in SIM_TERRAIN:
        assert hasattr(lib, name), name


def test_oracle_refuses_the_terrain(oracle_lib):
    for name in SIM_TERRAIN:
        assert not hasattr(oracle_lib, name)
    sim, tables = build_torque_simulator(oracle_lib, Robot(), 2, 1e-3, 0)
    sim.set_stage(0, *tables[(True, True)])
    for call in (lambda: sim.terrain(cr.stairs([0.3, 0.0, 0.05], 0.1)), lambda: sim.terrain(None), lambda: sim.read_terrain(),
                 lambda: sim.terrain_height(np.zeros((2, 3, 2)))):
        with pytest.raises(NotImplementedError, match="HIP library"):
            call()


# -- 2. the definition -------------------------------------------------------------------------------------------------------------------------------
BOX = [0.2, 0.6, -0.1, 0.3, 0.04]


def test_height_inside_outside_and_on_the_closed_edges():
    h = lambda pts, boxes=(BOX,), gz=0.0: cr.terrain_height(np.array(boxes), np.array(pts, dtype=float), gz).tolist()
    assert h([[0.4, 0.1], [0.21, -0.09]]) == [0.04, 0.04]
    assert h([[0.19, 0.1], [0.61, 0.1], [0.4, -0.11], [0.4, 0.31], [0.7, 0.5]]) == [0.0] * 5
    # every edge and every corner belongs to the box
    assert h([[0.2, 0.1], [0.6, 0.1], [0.4, -0.1], [0.4, 0.3], [0.2, -0.1], [0.2, 0.3], [0.6, -0.1], [0.6, 0.3]]) == [0.04] * 8
    eps = np.nextafter(0.2, 0.0), np.nextafter(0.6, 1.0)
    assert h([[eps[0], 0.1], [eps[1], 0.1], [0.4, np.nextafter(-0.1, -1.0)], [0.4, np.nextafter(0.3, 1.0)]]) == [0.0] * 4
    assert h([[0.4, 0.1]], gz=-0.5) == [0.04] and h([[0.0, 0.0]], gz=-0.5) == [-0.5]
    assert cr.terrain_height(np.zeros((0, 5)), np.zeros((3, 2)), 0.25).tolist() == [0.25] * 3
    assert cr.terrain_height(np.array([BOX]), np.array([0.4, 0.1]), 0.0) == 0.04   # (a single point)


def test_overlapping_boxes_the_higher_wins_and_a_box_below_the_ground_has_no_effect():
    boxes = np.array([BOX, [0.5, 0.9, -0.1, 0.3, 0.14], [0.0, 1.0, -1.0, 1.0, -0.2]])
    pts = np.array([[0.3, 0.0], [0.55, 0.0], [0.8, 0.0], [0.95, 0.0], [0.5, 0.0], [0.6, 0.0]])
    assert cr.terrain_height(boxes, pts, 0.0).tolist() == [0.04, 0.14, 0.14, 0.0, 0.14, 0.14]
    assert cr.terrain_height(boxes[::-1], pts, 0.0).tolist() == [0.04, 0.14, 0.14, 0.0, 0.14, 0.14]   # (the order of the boxes does not matter)
    assert cr.terrain_height(boxes, pts, -0.3).tolist() == [0.04, 0.14, 0.14, -0.2, 0.14, 0.14]
    assert cr.terrain_height(boxes, pts, 0.1).tolist() == [0.1, 0.14, 0.14, 0.1, 0.14, 0.14]


def test_shared_against_per_robot():
    rng = np.random.default_rng(3)
    B, n = 4, 6
    lo = rng.uniform(-1.0, 0.5, size=(B, n, 2))
    boxes = np.stack([lo[..., 0], lo[..., 0] + rng.uniform(0.1, 1.0, (B, n)), lo[..., 1], lo[..., 1] + rng.uniform(0.1, 1.0, (B, n)),
                      rng.uniform(-0.05, 0.3, (B, n))], axis=-1)
    pts = rng.uniform(-1.2, 1.7, size=(B, 50, 2))
    per = cr.terrain_height(boxes, pts, 0.0)
    assert per.shape == (B, 50)
    for b in range(B):
        np.testing.assert_array_equal(per[b], cr.terrain_height(boxes[b], pts[b], 0.0))
        want = [max([0.0] + [bx[4] for bx in boxes[b] if bx[0] <= x <= bx[1] and bx[2] <= y <= bx[3]]) for x, y in pts[b]]
        assert per[b].tolist() == want
    assert len(set(per.reshape(-1).tolist())) > 5
    np.testing.assert_array_equal(cr.terrain_height(boxes[0], pts, 0.0)[1], cr.terrain_height(boxes[0], pts[1], 0.0))   # (shared: any leading shape)
    with pytest.raises(ValueError, match="per-robot"):
        cr.terrain_height(boxes, pts[:3], 0.0)


def test_boxes_are_checked():
    for bad, what in ((np.zeros((17, 5)), "at most 16"), (np.zeros((2, 4)), "shape"), ([[0.0, 1.0, 0.0, 1.0, np.nan]], "finite"),
                      ([[0.0, 1.0, 0.0, np.inf, 0.1]], "finite"), ([[1.0, 0.0, 0.0, 1.0, 0.1]], "x_lo <= x_hi"), ([[0.0, 1.0, 1.0, 0.0, 0.1]], "y_lo <= y_hi")):
        with pytest.raises(ValueError, match=what):
            cr.terrain_boxes(bad)
    with pytest.raises(ValueError, match="3 robots"):
        cr.terrain_boxes(np.zeros((2, 1, 5)), batch=3)
    assert cr.terrain_boxes([]).shape == (0, 5) and cr.terrain_boxes(np.zeros((3, 0, 5)), batch=3).shape == (3, 0, 5)
    assert cr.terrain_boxes([[0.0, 0.0, 1.0, 1.0, 0.1]]).shape == (1, 5)   # (a degenerate box, a line or a point, is a box)


def test_stairs_is_the_reference_geometry():
    pose, h = np.array([0.45, -0.02, 0.03]), 0.1
    s = cr.stairs(pose, h)
    assert s.shape == (3, 5)
    for k in range(3):
        np.testing.assert_allclose(s[k, :2], [pose[0] + 0.3 * k - 0.2, pose[0] + 0.3 * k + 0.2], rtol=0, atol=1e-15)
        np.testing.assert_allclose(s[k, 2:4], [pose[1] - 0.5, pose[1] + 0.5], rtol=0, atol=1e-15)
        np.testing.assert_allclose(s[k, 4], pose[2] + k * h + h / 2, rtol=0, atol=1e-15)
    # consecutive steps overlap by 0.1 m: the visible tread is 0.3 m, and in the overlap the higher step is the ground
    assert cr.terrain_height(s, np.array([[0.45, 0.0], [0.70, 0.0], [0.80, 0.0], [1.10, 0.0], [1.26, 0.0], [0.2, 0.0]]), 0.0).tolist() == \
        [s[0, 4], s[1, 4], s[1, 4], s[2, 4], 0.0, 0.0]
    assert cr.stairs(pose, 0.07, n_steps=16).shape == (16, 5) and cr.stairs(pose, 0.07, n_steps=0).shape == (0, 5)
    np.testing.assert_allclose(cr.stairs(pose, 0.07, n_steps=5, pitch=0.25, half_extents=(0.15, 0.4))[4],
                               [pose[0] + 1.0 - 0.15, pose[0] + 1.0 + 0.15, pose[1] - 0.4, pose[1] + 0.4, pose[2] + 4 * 0.07 + 0.035], rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="steps"):
        cr.stairs(pose, 0.1, n_steps=17)


# -- 3. without a terrain the rule keeps its bits ----------------------------------------------------------------------------------------------------------
def _sequence():
    """(z, fz) of a sequence that releases the right sole, lifts it, catches it within the tolerance, releases it again and catches it sinking"""
    seq = [([0.0, 0.0], [100.0, -50.0])] * 5
    seq += [([0.0, z], [100.0, 0.0]) for z in (0.004, 0.0101, 0.02, 0.0052, 0.005)]
    seq += [([0.0, 0.005], [100.0, -50.0])] * 5
    seq += [([0.0, z], [100.0, 0.0]) for z in (0.003, 0.001, -0.0005)]
    seq += [([0.0, 0.0], [-50.0, -50.0])] * 6
    return seq


def test_no_terrain_and_zero_boxes_are_todays_rule_bit_for_bit():
    for B, cfg in ((1, {}), (3, {"ground_z": 0.001, "release_steps": 4})):
        today, none, zero, zero_per = _rows(B), _rows(B), _rows(B), _rows(B)
        for z, fz in _sequence():
            today = _step(today, z, fz, **cfg)
            zz = np.broadcast_to(np.asarray(z, dtype=float), (B, 2))
            R, p = np.broadcast_to(I3, (B, 2, 3, 3)), np.concatenate([np.zeros((B, 2, 2)), zz[..., None]], axis=-1)
            f = np.broadcast_to(np.asarray(fz, dtype=float), (B, 2))
            none = cr.step(none, zz, f, R, p, cfg, terrain=None)
            zero = cr.step(zero, zz, f, R, p, cfg, terrain=np.zeros((0, 5)))
            zero_per = cr.step(zero_per, zz, f, R, p, cfg, terrain=np.zeros((B, 0, 5)))
            for other in (none, zero, zero_per):
                assert other.tobytes() == today.tobytes()
        u = cr.unpack(today)
        assert u["touchdowns"][0, 1] == 2.0 and u["liftoffs"][0].tolist() == [1.0, 2.0]   # (the sequence does what its docstring says)
    r = _released_right()
    p = np.array([[[0.0, 0.0, 0.0], [0.0, 0.0, 0.02]]])
    assert cr.step(r, p[..., 2], [[100.0, 0.0]], np.broadcast_to(I3, (1, 2, 3, 3)), p, {}, terrain=[]).tobytes() == _step(r, [0.0, 0.02], [100.0, 0.0]).tobytes()


# -- 4. hand-made sequences over a box ----------------------------------------------------------------------------------------------------------------
def _over(rows, z_right, xy_right, terrain, xy_left=(0.0, 0.1), z_left=0.0, fz=(100.0, 0.0)):
    p = np.array([[[xy_left[0], xy_left[1], z_left], [xy_right[0], xy_right[1], z_right]]])
    return cr.step(rows, p[..., 2], np.array([fz]), np.broadcast_to(I3, (1, 2, 3, 3)), p, {}, terrain=terrain)


LOW_BOX = np.array([[0.2, 0.6, -0.3, 0.1, 0.04]])   # a 4 cm box in front of the right foot


def test_a_descending_foot_is_caught_on_the_box_and_beside_it_on_the_plane():
    for xy, ground in (((0.4, -0.1), 0.04), ((0.4, -0.31), 0.0), ((0.19, -0.1), 0.0)):
        r = _released_right()
        r = _over(r, 0.08, xy, LOW_BOX)                         # above g + 2 tol for either ground: lifted
        assert cr.unpack(r)["lifted"][0].tolist() == [0.0, 1.0]
        r = _over(r, 0.0452, xy, LOW_BOX)                       # 5.2 mm above the box: not yet (and 45 mm above the plane)
        assert cr.unpack(r)["in_contact"][0].tolist() == [1.0, 0.0]
        r = _over(r, 0.0449, xy, LOW_BOX)                       # within the tolerance of the box top
        u = cr.unpack(r)
        if ground == 0.04:
            assert u["in_contact"][0].tolist() == [1.0, 1.0] and u["touchdowns"][0].tolist() == [0.0, 1.0]
            assert u["anchor_p"][0, 1].tolist() == [xy[0], xy[1], 0.04]    # exactly the box top, not the plane
        else:
            assert u["in_contact"][0].tolist() == [1.0, 0.0]               # beside the box: 45 mm above the only ground there
            r = _over(r, 0.0049, xy, LOW_BOX)
            u = cr.unpack(r)
            assert u["in_contact"][0].tolist() == [1.0, 1.0] and u["anchor_p"][0, 1].tolist() == [xy[0], xy[1], 0.0]
        np.testing.assert_array_equal(u["anchor_R"][0, 1], I3)
        np.testing.assert_array_equal(u["anchor_p"][0, 0], [0.0, 0.1, 0.0])


def test_lifted_is_taken_above_the_ground_under_the_foot():
    r = _released_right()
    r = _over(r, 0.0499, (0.4, -0.1), LOW_BOX)   # 9.9 mm above the box: not lifted there (49.9 mm above the plane would be)
    assert cr.unpack(r)["lifted"][0].tolist() == [0.0, 0.0]
    r = _over(r, 0.0449, (0.4, -0.1), LOW_BOX)   # within the tolerance but never lifted, above the box: free
    assert cr.unpack(r)["in_contact"][0].tolist() == [1.0, 0.0]
    r = _over(r, 0.0399, (0.4, -0.1), LOW_BOX)   # sinks into the box: caught on it
    u = cr.unpack(r)
    assert u["in_contact"][0].tolist() == [1.0, 1.0] and u["anchor_p"][0, 1, 2] == 0.04


def test_the_origin_of_the_sole_decides_not_its_toe():
    """The sole is 0.2 m long: at x = 0.15 its toe (x + 0.1) is 5 cm over the box that begins at 0.2, its origin is not.  It goes down past the box top
    and is caught on the plane."""
    r = _released_right()
    r = _over(r, 0.08, (0.15, -0.1), LOW_BOX)
    for z in (0.045, 0.04, 0.03, 0.0051):
        r = _over(r, z, (0.15, -0.1), LOW_BOX)
        assert cr.unpack(r)["in_contact"][0].tolist() == [1.0, 0.0], z
    r = _over(r, 0.005, (0.15, -0.1), LOW_BOX)
    u = cr.unpack(r)
    assert u["in_contact"][0].tolist() == [1.0, 1.0] and u["anchor_p"][0, 1].tolist() == [0.15, -0.1, 0.0]


def test_released_on_a_box_and_set_down_on_the_plane():
    r = _released_right()
    r = _over(r, 0.08, (0.4, -0.1), LOW_BOX)
    r = _over(r, 0.044, (0.4, -0.1), LOW_BOX)
    assert cr.unpack(r)["anchor_p"][0, 1, 2] == 0.04
    for _ in range(5):   # the in-contact branch does not look at the ground: five pulling steps release the sole that stands on the box
        r = _over(r, 0.04, (0.4, -0.1), LOW_BOX, fz=(100.0, -50.0))
    u = cr.unpack(r)
    assert u["in_contact"][0].tolist() == [1.0, 0.0] and u["lifted"][0].tolist() == [0.0, 0.0] and u["liftoffs"][0].tolist() == [0.0, 2.0]
    r = _over(r, 0.06, (0.5, -0.1), LOW_BOX)     # lifted over the box (2 cm above it)
    r = _over(r, 0.05, (0.7, -0.1), LOW_BOX)     # past the box: 5 cm above the plane, free
    assert cr.unpack(r)["in_contact"][0].tolist() == [1.0, 0.0]
    r = _over(r, 0.004, (0.75, -0.1), LOW_BOX)
    u = cr.unpack(r)
    assert u["in_contact"][0].tolist() == [1.0, 1.0] and u["anchor_p"][0, 1].tolist() == [0.75, -0.1, 0.0] and u["touchdowns"][0].tolist() == [0.0, 2.0]


def test_robots_on_their_own_terrain():
    r = np.concatenate([_released_right()] * 3)
    per = np.array([[[0.2, 0.6, -0.3, 0.1, 0.04]], [[0.2, 0.6, -0.3, 0.1, 0.07]], [[2.0, 3.0, -0.3, 0.1, 0.07]]])
    p = np.tile(np.array([[[0.0, 0.1, 0.0], [0.4, -0.1, 0.1]]]), (3, 1, 1))
    R = np.broadcast_to(I3, (3, 2, 3, 3))
    fz = np.tile([[100.0, 0.0]], (3, 1))
    r = cr.step(r, p[..., 2], fz, R, p, {}, terrain=per)
    p[:, 1, 2] = 0.072
    r = cr.step(r, p[..., 2], fz, R, p, {}, terrain=per)
    u = cr.unpack(r)
    assert u["in_contact"].tolist() == [[1.0, 0.0], [1.0, 1.0], [1.0, 0.0]] and u["anchor_p"][1, 1, 2] == 0.07
    with pytest.raises(ValueError, match="3 robots"):
        cr.step(r, p[..., 2], fz, R, p, {}, terrain=per[:2])


# -- 5. the mirror against BulletRobot's host rule on the oracle, over a box -----------------------------------------------------------------------------
def _bullet(lib, **kw):
    from mpc_benchmark_amd.bullet_robot import BulletRobot
    rb = Robot()
    m = rb.model
    robot = BulletRobot([n for n in m.names], None, None, 1e-3, m, library=lib, **kw)
    robot.initializeJoints(rb.x0[:m.nq])
    return rb, robot


def box_at_the_right_sole(p_sole, z_top, kind):
    """One box at height ``z_top`` placed against the nominal right-sole origin ``p_sole``: ``under`` covers the origin with room for the sole's drift
    while it is in the air (25 mm measured); ``beside`` lies 10 cm to the robot's right of it; ``toe`` begins 5 cm in front of the origin, under the
    front half of the 0.2 m sole but not under its origin."""
    x, y = float(p_sole[0]), float(p_sole[1])
    return {"under": [x - 0.15, x + 0.15, y - 0.08, y + 0.08, z_top], "beside": [x - 0.15, x + 0.15, y - 0.30, y - 0.10, z_top],
            "toe": [x + 0.05, x + 0.35, y - 0.08, y + 0.08, z_top]}[kind]


@pytest.mark.parametrize("height", [0.005, 0.015, 0.024])
def test_mirror_follows_bullet_robot_on_the_oracle_over_a_box(oracle_lib, height):
    """``lift_torques`` with span 25 (apex of the right sole 36.9 mm; the stock span 15 lifts it 12.1 mm, less than the 10 mm that ``lifted`` needs over
    any box).  The box is pushed under the lifted foot: installed at the first step at which the released sole is above z_top + 2 ground_tol.  Flags
    equal at every step, released then caught, the caught anchor exactly at the box top."""
    from mpc_benchmark_amd.robot import minipin as pin
    rb, robot = _bullet(oracle_lib)
    q0 = robot.x[:robot.model.nq].copy()
    seen = []
    orig = robot._update_contacts
    robot._update_contacts = lambda wr: (seen.append(np.array(wr)), orig(wr))
    mm, data = robot.model, robot.model.createData()
    cfg = {"ground_z": robot.ground_z, "ground_tol": robot.ground_tol, "release_force": robot.release_force, "release_steps": robot.release_steps}
    anchors = [robot.data.oMf[f] for f in robot.frame_ids]
    rows = cr.reset_rows(np.array([[M.rotation for M in anchors]]), np.array([[M.translation for M in anchors]]))
    z_top = robot.ground_z + height
    assert z_top + 2 * robot.ground_tol <= robot.ground_z + 0.0369 - 0.002   # at least 2 mm under the apex
    box = box_at_the_right_sole(anchors[1].translation, z_top, "under")
    terrain, installed, flags, first_catch = None, None, [], None
    for k in range(100):
        robot.execute(lift_torques(robot, q0, k, span=25))
        pin.framesForwardKinematics(mm, data, robot.x[:mm.nq])
        R = np.array([[data.oMf[f].rotation for f in robot.frame_ids]])
        p = np.array([[data.oMf[f].translation for f in robot.frame_ids]])
        rows = cr.step(rows, p[..., 2], seen[-1][None, :, 2], R, p, cfg, terrain=terrain)
        u = cr.unpack(rows)
        assert u["in_contact"][0].tolist() == [float(c) for c in robot.in_contact], k
        assert u["lifted"][0].tolist() == [float(c) for c in robot._lifted], k
        assert u["pulling"][0].tolist() == [float(c) for c in robot._pulling], k
        if flags and not flags[-1][1] and robot.in_contact[1] and first_catch is None:
            first_catch = k
            assert installed is not None and u["anchor_p"][0, 1, 2] == z_top == robot._contact_pose[1].translation[2]   # on the box, not the plane
            assert box[0] < u["anchor_p"][0, 1, 0] < box[1] and box[2] < u["anchor_p"][0, 1, 1] < box[3]
        flags.append(tuple(robot.in_contact))
        if installed is None and not robot.in_contact[1] and p[0, 1, 2] > z_top + 2 * robot.ground_tol:
            robot.setTerrain([box])       # (the rule of step k has run: the box is there from step k + 1 on)
            terrain, installed = [box], k
    print("box of %.0f mm installed after step %s, the sole caught on it at step %s; touchdowns %s" % (1e3 * height, installed, first_catch, u["touchdowns"][0]))
    assert (True, False) in flags and flags[-1] == (True, True) and first_catch is not None
    for i, pose in enumerate(robot._contact_pose):
        np.testing.assert_allclose(u["anchor_R"][0, i], pose.rotation, atol=1e-12)
        np.testing.assert_allclose(u["anchor_p"][0, i], pose.translation, atol=1e-12)
    assert u["anchor_p"][0, 1, 2] == z_top and u["anchor_p"][0, 0, 2] == robot.ground_z
    robot.close()


# The inputs of tests/test_gpu_sim_terrain.py::test_kernel_equals_the_mirror_over_boxes: per robot (amp, span) of its lift pulse, where its box lies and
# the height of the box above the ground.  Apexes of the right sole measured with the host rule on the oracle: 36.9, 37.0, 35.9, 33.3, 45.6 mm for the
# five ``under`` robots, so z_top + 2 ground_tol stays at least 2 mm under each (heights <= apex - 12 mm), between 5 mm and that bound; all five are
# above their boxes by 2 ground_tol together from step 26 to step 30.
LIFTS = ((150.0, 25, "under", 0.005), (160.0, 24, "under", 0.024), (180.0, 22, "under", 0.015), (200.0, 20, "under", 0.020), (220.0, 22, "under", 0.030),
         (250.0, 15, "toe", 0.008), (170.0, 23, "beside", 0.010), (200.0, 22, "beside", 0.012))
LIFT_STEPS = 100


def lift_boxes(p_sole, ground_z):
    """(8, 1, 5): the box of every robot of ``LIFTS`` against the nominal right-sole origin"""
    return np.array([[box_at_the_right_sole(p_sole, ground_z + h, kind)] for _, _, kind, h in LIFTS])


def boxes_can_go_in(in_contact_right, z_right, boxes, ground_tol):
    """the moment of the one terrain() call: every robot whose box lies under its sole has that sole released and above z_top + 2 ground_tol (the others'
    soles never come over their boxes, whenever these appear)"""
    under = np.array([kind == "under" for _, _, kind, _ in LIFTS])
    return bool(np.all(~under | (~np.asarray(in_contact_right, dtype=bool) & (np.asarray(z_right) > boxes[:, 0, 4] + 2 * ground_tol))))


def test_the_inputs_of_the_gpu_kernel_test_meet_its_conditions(oracle_lib):
    """The host rule of BulletRobot on the oracle, robot by robot, on the pulses and boxes of ``LIFTS``, the boxes installed at the common step the GPU test
    finds: every robot is released and caught, five catches are on a box top (exactly), three on the plane (two boxes beside the foot, one under
    the toe only), every robot stands at the end, and every height keeps z_top + 2 ground_tol at least 2 mm under that robot's apex."""
    robots = [_bullet(oracle_lib)[1] for _ in LIFTS]
    q0 = robots[0].x[:robots[0].model.nq].copy()
    gz, tol = robots[0].ground_z, robots[0].ground_tol
    boxes = lift_boxes(robots[0].data.oMf[robots[0].frame_ids[1]].translation.copy(), gz)
    installed, apex, catches, prev = None, np.zeros(len(LIFTS)), [[] for _ in LIFTS], [True] * len(LIFTS)
    for k in range(LIFT_STEPS):
        for b, (robot, (amp, span, _, _)) in enumerate(zip(robots, LIFTS)):
            robot.execute(lift_torques(robot, q0, k, amp=amp, span=span))
            if not robot.in_contact[1]:
                apex[b] = max(apex[b], robot._z_prev[1] - gz)
            if robot.in_contact[1] and not prev[b]:
                catches[b].append((k, robot._contact_pose[1].translation[2]))
            prev[b] = robot.in_contact[1]
        if installed is None and boxes_can_go_in([r.in_contact[1] for r in robots], [r._z_prev[1] for r in robots], boxes, tol):
            for b, robot in enumerate(robots):
                robot.setTerrain(boxes[b])
            installed = k
    print("boxes installed after step %s; apex (mm) %s; first catches %s" % (installed, np.round(1e3 * apex, 1), [c[0] for c in catches]))
    assert installed is not None
    on_box = on_plane = 0
    for b, (robot, (_, _, kind, h)) in enumerate(zip(robots, LIFTS)):
        assert catches[b] and catches[b][0][0] > installed and robot.in_contact == [True, True], b
        z_first = catches[b][0][1]
        if kind == "under":
            assert 0.005 <= h and h + 2 * tol <= apex[b] - 0.002, (b, h, apex[b])
            assert z_first == boxes[b, 0, 4], b
            on_box += 1
        else:
            assert z_first == gz, b
            on_plane += 1
        robot.close()
    assert on_box == 5 and on_plane == 3


# -- 6. the metrics mirror: the fall verdict above the ground ------------------------------------------------------------------------------------------
def _climb(S=8, B=2):
    """a record in which both soles end 10 cm higher, each on its own step (the right one first), and the base rises with them; the contact rows the
    steps were integrated with; the two steps as boxes"""
    rec, x_start, nq = _synthetic(S=S, B=B)
    boxes = np.array([[0.2, 0.6, -0.3, 0.0, 0.1], [0.2, 0.6, 0.0, 0.3, 0.1]])
    rows = np.zeros((S, B, cr.WIDTH))
    rows[..., cr.O_ANCHOR:cr.O_ANCHOR + 9] = rows[..., cr.O_ANCHOR + 12:cr.O_ANCHOR + 21] = np.eye(3).reshape(-1)
    for k in range(S):
        right_up, left_up = k >= 2, k >= 5
        rec["sole_p"][k, :, 1] = [0.4, -0.09, 0.1] if right_up else [0.0, -0.09, 0.0]
        rec["sole_p"][k, :, 0] = [0.4, 0.09, 0.1] if left_up else [0.0, 0.09, 0.0]
        rec["x"][k, :, 2] = 1.0 + 0.05 * right_up + 0.05 * left_up
        rows[k, :, cr.O_IN:cr.O_IN + 2] = 1.0
        rows[k, :, cr.O_ANCHOR + 23] = 0.1 if right_up else 0.0
        rows[k, :, cr.O_ANCHOR + 11] = 0.1 if left_up else 0.0
    return rec, x_start, boxes, rows


def test_a_robot_that_climbed_is_not_fallen_with_the_terrain_and_is_without():
    rec, x_start, boxes, rows = _climb()
    flat = lm.from_record(rec, x_start, 1e-3)
    assert flat["fall_step"].tolist() == [5.0, 5.0]   # both soles 10 cm above their latched heights: today's verdict, and it stays
    up = lm.from_record(rec, x_start, 1e-3, terrain=boxes, contact_rows=rows)
    assert up["fall_step"].tolist() == [-1.0, -1.0]
    assert up["base_z0"].tolist() == [1.0, 1.0] and up["sole_z0"].tolist() == [[0.0, 0.0]] * 2
    for k in flat:   # nothing else in a row changes
        if k not in ("fall_step", "base_z0", "sole_z0"):
            np.testing.assert_array_equal(flat[k], up[k], err_msg=k)
    with pytest.raises(ValueError, match="contact_rows"):
        lm.from_record(rec, x_start, 1e-3, terrain=boxes)


def test_a_base_that_drops_relative_to_the_anchors_is_fallen_on_a_step_as_on_the_plane():
    rec, x_start, boxes, rows = _climb()
    rec["x"][6:, 1, 2] -= 0.25           # robot 1's base drops 0.25 m after both feet are up: 1.1 -> 0.85, 0.75 above the anchors against 1.0 latched
    up = lm.from_record(rec, x_start, 1e-3, terrain=boxes, contact_rows=rows)
    assert up["fall_step"].tolist() == [-1.0, 6.0]
    rec, x_start, _, _ = _climb()
    rec["sole_p"][..., 2] = 0.0
    rec["x"][..., 2] = 1.0
    rec["x"][6:, 1, 2] -= 0.25
    assert lm.from_record(rec, x_start, 1e-3)["fall_step"].tolist() == [-1.0, 6.0]
    # both soles 3 cm above the steps they stood on: fallen by the sole rule, relative to the ground under them
    rec, x_start, boxes, rows = _climb()
    rec["sole_p"][7, 0, :, 2] = 0.13
    assert lm.from_record(rec, x_start, 1e-3, terrain=boxes, contact_rows=rows)["fall_step"].tolist() == [7.0, -1.0]
    # in single support the base is measured against the one anchor in contact
    rec, x_start, boxes, rows = _climb()
    rows[3:5, :, cr.O_IN] = 0.0          # the left sole in the air while the right stands on its step: base 1.05 - 0.1 = 0.95, no fall
    rows[3:5, :, cr.O_ANCHOR + 11] = -5.0  # (the anchor of a free sole is not read)
    assert lm.from_record(rec, x_start, 1e-3, terrain=boxes, contact_rows=rows)["fall_step"].tolist() == [-1.0, -1.0]


def test_without_a_terrain_from_record_returns_what_it_returns_today():
    rec, x_start, _, rows = _climb()
    rec["x"][4, 1, 5] = np.nan
    today = lm.from_record(rec, x_start, 1e-3)
    for other in (lm.from_record(rec, x_start, 1e-3, terrain=None, contact_rows=None), lm.from_record(rec, x_start, 1e-3, terrain=None, contact_rows=rows),
                  lm.from_record(rec, x_start, 1e-3, terrain=np.zeros((0, 5)), contact_rows=rows)):
        for k in today:
            assert np.asarray(other[k]).tobytes() == np.asarray(today[k]).tobytes(), k


# -- 7. BulletRobot and the pipelines ------------------------------------------------------------------------------------------------------------------
def test_create_stairs_on_the_headless_bullet_robot(oracle_lib):
    rb, robot = _bullet(oracle_lib)
    assert robot.terrain is None
    robot.createStairs([0.6, 0.0, 0.05], 0.1)
    np.testing.assert_array_equal(robot.terrain, cr.stairs([0.6, 0.0, 0.05], 0.1))
    assert robot._ground_under([0.6, 0.0, 7.0]) == robot.terrain[0, 4] and robot._ground_under([0.0, 0.0, 0.0]) == robot.ground_z
    robot.execute(np.zeros(robot.model.nv - 6))      # the host rule runs with the terrain (both soles stand beside it)
    assert robot.in_contact == [True, True]
    robot.setTerrain([[0.0, 1.0, 0.0, 1.0, 0.02]])
    assert robot.terrain.shape == (1, 5)
    with pytest.raises(ValueError, match=r"\(n, 5\)"):
        robot.setTerrain(np.zeros((2, 1, 5)))
    robot.setTerrain(None)
    assert robot.terrain is None
    with pytest.raises(NotImplementedError):
        robot.addStairs("stairs.urdf", [0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0])
    robot.close()


@pytest.mark.parametrize("cls", [KinodynamicPipeline, CentroidalPipeline, FullDynamicPipeline])
def test_pipelines_refuse_a_terrain_without_the_rule(cls):
    with pytest.raises(ValueError, match="terrain needs contact_rule"):
        cls(None, batch=2, terrain=cr.stairs([0.3, 0.0, 0.05], 0.1))
    with pytest.raises(ValueError, match="2 robots"):
        cls(None, batch=2, contact_rule={}, terrain=np.zeros((3, 1, 5)))
