"""Per-robot sole tipping of the torque-driven simulator in numpy (mpc_benchmark_amd/tipping_model.py): the definition the device kernel
(include/mpc_sim_tipping.h, csrc/sim_tipping.h) is held to in tests/test_gpu_sim_tipping.py.  Here the definition itself: the layout and the
bindings, the identity, the sign of the onset on each of the four edges, the steady tip, the landing, free soles, the clamps, the anchor, the default
slider inertia, the refusals; and the scenarios of the GPU tests on the CPU reference (tests/_tipping_reference.py)."""
import glob
import os
import re

import numpy as np
import pytest

from mpc_benchmark_amd import _capi
from mpc_benchmark_amd import tipping_model as tm
from mpc_benchmark_amd.problems.common import FOOT_FRAMES, Robot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mpc_sim_tipping", "mpc_sim_tipping_read", "mpc_sim_tipping_set", "mpc_sim_tipping_width")
DT = 1e-3
L, W = 0.1, 0.075


def _params(half_length=np.inf, half_width=np.inf, I_tip=10.0, w_max=tm.W_MAX, th_max=tm.TH_MAX, batch=1):
    return tm.rows({"half_length": half_length, "half_width": half_width, "I_tip": I_tip, "w_max": w_max, "th_max": th_max}, batch)


def _wrench(fz=0.0, tx=0.0, ty=0.0):
    """sole 0 carries the wrench, sole 1 a copy with the moments negated"""
    return np.array([[[3.0, -2.0, fz, tx, ty, 0.7], [3.0, -2.0, fz, -tx, -ty, 0.7]]])


def _anchor(R=None, p=(0.1, 0.2, 0.0), batch=1):
    return np.tile(np.concatenate(((np.eye(3) if R is None else R).reshape(9), p)), (batch, 2, 1))


def test_header_and_bindings_agree():
    text = open(os.path.join(ROOT, "include", "mpc_sim_tipping.h")).read()
    assert set(re.findall(r"^(?:int|int32_t) (mpc_\w+)\(", text, re.M)) == set(SYMBOLS) == set(_capi._SIM_TIPPING_SIGNATURES)
    for name, val in (("PARAMS", tm.PARAMS), ("WIDTH", tm.WIDTH)):
        assert int(re.search(r"#define MPC_SIM_TIPPING_%s (\d+)" % name, text).group(1)) == val, name
    assert tm.O_STEPS + 1 == tm.WIDTH == 21 and len(tm.IDENTITY) == tm.PARAMS == 8
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if not path.endswith("mpc_sim_tipping.h"):
            assert "mpc_sim_tipping(" not in open(path).read(), path


def test_hip_library_exports_the_entry_points():
    lib = _capi.bind_library(_capi.HIP_LIBRARY_PATH)   # (dlopen works without a GPU; nothing is computed)
    assert all(hasattr(lib, n) for n in SYMBOLS)


def test_the_oracle_does_not_export_the_tipping_model(oracle_lib):
    from mpc_benchmark_amd.pipeline import build_torque_simulator
    sim, _ = build_torque_simulator(oracle_lib, Robot(), 2, DT, 0)
    for call in (lambda: sim.tipping(tm.IDENTITY), lambda: sim.read_tipping(), lambda: sim.set_tipping(tm.reset(2))):
        with pytest.raises(RuntimeError, match="HIP only"):
            call()
    sim.close()


def test_identity_rows_leave_a_row_untouched_bit_for_bit():
    """arbitrary wrenches, held and free soles: only ``steps`` counts, and the anchors keep every bit"""
    rng = np.random.default_rng(1)
    B = 3
    rows, p, anchors = tm.reset(B), tm.rows(tm.IDENTITY, B), _anchor(batch=B)
    for k in range(6):
        w = rng.normal(size=(B, 2, 6)) * 1e4
        tm.step(rows, p, (rng.uniform(size=(B, 2)) > 0.3).astype(float), w, DT, anchors=anchors)
    assert np.all(rows[:, :tm.O_STEPS] == 0.0) and not np.any(np.signbit(rows)) and np.all(rows[:, tm.O_STEPS] == 6.0)
    assert np.array_equal(anchors, _anchor(batch=B))


@pytest.mark.parametrize("axis, sign", [(0, -1.0), (0, 1.0), (1, -1.0), (1, 1.0)])
def test_the_onset_has_the_sign_of_the_edge_where_the_cop_saturates(axis, sign):
    """tau_x < -W n: w_x > 0, the edge y = -W; tau_x > W n: w_x < 0, y = +W; tau_y < -L n: w_y > 0, x = +L; tau_y > L n: w_y < 0, x = -L.  A normal
    force n at the point r gives the moment r x (0, 0, n) = (r_y n, -r_x n, 0) about the origin: the CoP saturates at the edge whose r has that
    sign, and the origin's velocity is -w x r_edge, upwards"""
    n, excess, I = 400.0, 7.0, 10.0
    h = (W, L)[axis]
    tau = sign * (h * n + excess)
    rows, p = tm.reset(1), _params(L, W, I_tip=I)
    tm.step(rows, p, np.ones((1, 2)), _wrench(fz=n, **{("tx", "ty")[axis]: tau}), DT)
    r = tm.unpack(rows)
    w = r["v"][0, 0, 1 + axis]
    assert np.isclose(w, -sign * (DT / I) * excess, rtol=1e-12) and r["v"][0, 0, 2 - axis] == 0.0
    assert np.isclose(r["v"][0, 1, 1 + axis], -w, rtol=1e-12)   # (sole 1 carries the negated moment)
    # the edge where the CoP saturates: tau_x = r_y n, tau_y = -r_x n
    r_edge = np.array([0.0, sign * W, 0.0]) if axis == 0 else np.array([-sign * L, 0.0, 0.0])
    omega = np.zeros(3)
    omega[axis] = w
    v = -np.cross(omega, r_edge)
    assert v[0] == 0.0 and v[1] == 0.0 and v[2] > 0.0 and np.isclose(r["v"][0, 0, 0], v[2], rtol=1e-12)
    assert np.all(r["tipping"] == 1.0) and np.all(r["tip_steps"] == 0.0) and np.all(r["th"] == 0.0) and np.allclose(r["peak_excess"], excess)
    # the step integrated with that rate: the angle takes the sign the docstring gives the edge (th_x > 0: y = -W, th_y > 0: x = +L)
    tm.step(rows, p, np.ones((1, 2)), _wrench(fz=n, **{("tx", "ty")[axis]: tau}), DT)
    th = tm.unpack(rows)["th"][0, 0, axis]
    assert th == w * DT and np.sign(th) == (-np.sign(r_edge[1]) if axis == 0 else np.sign(r_edge[0]))


def test_inside_the_sole_nothing_moves():
    rows, p = tm.reset(1), _params(L, W)
    for k in range(5):
        tm.step(rows, p, np.ones((1, 2)), _wrench(fz=400.0, tx=29.0 * np.cos(k), ty=39.0 * np.sin(k)), DT)
    assert np.all(rows[0, :tm.O_STEPS] == 0.0) and rows[0, tm.O_STEPS] == 5.0   # (the excess stayed negative: the peak keeps its 0)


def test_a_steady_tip_transmits_exactly_the_edge_moment():
    """the rate does not change while tau = -s lim, on either edge of either axis, tipping on or tipping back"""
    n = 300.0
    for axis, h in ((0, W), (1, L)):
        for s in (1.0, -1.0):
            for w0 in (0.2, -0.2):
                rows, p = tm.reset(1), _params(L, W)
                rows[0, 1 + axis], rows[0, tm.O_TH + axis], rows[0, tm.O_TIPPING] = w0, s * 0.1, 1.0
                tm.step(rows, p, np.array([[1.0, 0.0]]), _wrench(fz=n, **{("tx", "ty")[axis]: -s * h * n}), DT)
                r = tm.unpack(rows)
                assert r["v"][0, 0, 1 + axis] == w0 and np.isclose(r["th"][0, 0, axis], s * 0.1 + w0 * DT, rtol=1e-15)
                assert np.isclose(r["v"][0, 0, 0], s * h * w0, rtol=1e-15) and r["tip_steps"][0, 0] == 1.0 and r["landings"][0, 0] == 0.0
                # a moment beyond the edge's accelerates the tip, one short of it brings the sole back
                for extra in (5.0, -5.0):
                    again = rows.copy()
                    tm.step(again, p, np.array([[1.0, 0.0]]), _wrench(fz=n, **{("tx", "ty")[axis]: -s * (h * n + extra)}), DT)
                    assert np.isclose(again[0, 1 + axis] - w0, s * (DT / 10.0) * extra, rtol=1e-9)


def test_a_tip_back_lands_and_the_same_update_may_start_the_opposite_tip():
    n = 300.0
    rows, p = tm.reset(1), _params(L, W)
    rows[0, 1], rows[0, tm.O_TH], rows[0, tm.O_TIPPING] = -0.5, 0.2e-3, 1.0   # th_x = 0.2 mrad on y = -W, coming back at 0.5 rad/s
    anchors = _anchor()
    tm.step(rows, p, np.array([[1.0, 0.0]]), _wrench(fz=n, tx=10.0), DT, anchors=anchors)   # inside the sole: it stays down
    r = tm.unpack(rows)
    assert r["th"][0, 0, 0] == 0.0 and np.all(r["v"][0, 0] == 0.0) and r["landings"][0, 0] == 1.0 and r["tipping"][0, 0] == 0.0
    assert r["tip_steps"][0, 0] == 1.0 and r["peak_angle"][0, 0] == 0.0
    # (the anchor followed the whole step's twist: a landing does not snap it)
    assert np.allclose(anchors[0, 0, :9].reshape(3, 3), tm.exp_rotation(-0.5 * DT, 0.0), rtol=0, atol=1e-15)
    # the same, but the moment of the landing step already leaves the sole on the other side: the opposite tip starts in the same update
    rows = tm.reset(1)
    rows[0, 1], rows[0, tm.O_TH], rows[0, tm.O_TIPPING] = -0.5, 0.2e-3, 1.0
    tm.step(rows, p, np.array([[1.0, 0.0]]), _wrench(fz=n, tx=W * n + 20.0), DT)
    r = tm.unpack(rows)
    assert r["th"][0, 0, 0] == 0.0 and r["landings"][0, 0] == 1.0 and np.isclose(r["v"][0, 0, 1], -(DT / 10.0) * 20.0) and r["tipping"][0, 0] == 1.0
    assert r["v"][0, 0, 0] > 0.0   # (w_x < 0 from the flat: the edge y = +W, the origin rises)
    # an angle that only comes closer does not land
    rows = tm.reset(1)
    rows[0, 1], rows[0, tm.O_TH], rows[0, tm.O_TIPPING] = -0.5, 0.2, 1.0
    tm.step(rows, p, np.array([[1.0, 0.0]]), _wrench(fz=n, tx=-W * n), DT)
    assert np.isclose(rows[0, tm.O_TH], 0.2 - 0.5 * DT) and rows[0, tm.O_LANDINGS] == 0.0 and rows[0, 1] == -0.5 and rows[0, 0] < 0.0


def test_a_free_sole_is_cleared():
    rows, p = tm.reset(1), _params(L, W)
    tm.step(rows, p, np.ones((1, 2)), _wrench(fz=100.0, tx=50.0, ty=-60.0), DT)
    tm.step(rows, p, np.ones((1, 2)), _wrench(fz=100.0, tx=50.0, ty=-60.0), DT)
    assert np.all(rows[0, :tm.O_TIPPING] != 0.0) and np.all(rows[0, tm.O_TIPPING:tm.O_TIP_STEPS] == 1.0)
    tm.step(rows, p, np.array([[1.0, 0.0]]), _wrench(fz=100.0, tx=50.0, ty=-60.0), DT)
    r = tm.unpack(rows)
    assert np.all(r["v"][0, 1] == 0.0) and np.all(r["th"][0, 1] == 0.0) and r["tipping"][0, 1] == 0.0
    assert np.all(r["v"][0, 0] != 0.0) and np.all(r["th"][0, 0] != 0.0) and r["tipping"][0, 0] == 1.0
    assert np.all(r["tip_steps"] == 2.0) and np.all(r["peak_angle"] > 0.0)   # (the steps both were integrated with)


def test_the_clamps_hold():
    rows, p = tm.reset(1), _params(L, W, I_tip=1e-3, w_max=0.7, th_max=2.5e-3)
    seen = []
    for _ in range(6):
        tm.step(rows, p, np.ones((1, 2)), _wrench(fz=100.0, tx=-90.0, ty=80.0), DT)
        r = tm.unpack(rows)
        assert np.all(np.abs(r["v"][0, :, 1:]) <= 0.7)
        seen.append(r["v"][0, 0, 1:].copy())
    assert np.array_equal(seen[0], [0.7, -0.7]) and np.array_equal(seen[2], [0.7, -0.7])
    # th reaches th_max after 4 steps at w_max: the rate that would carry it further is cleared, one that brings it back is kept
    assert np.all(np.abs(r["th"]) >= 2.5e-3) and np.all(np.abs(r["th"]) <= 2.5e-3 + 0.7 * DT) and np.all(r["v"] == 0.0) and np.all(r["tipping"] == 1.0)
    tm.step(rows, p, np.ones((1, 2)), _wrench(fz=100.0, tx=0.0, ty=0.0), DT)
    r = tm.unpack(rows)
    assert np.all(r["v"][0, 0, 1:] * r["th"][0, 0] < 0.0)


def test_the_anchor_follows_the_tip():
    """N steps of constant w_x on the edge y = -W (the steady tip's moment): the anchor's rotation is R2_0 Exp(th_x e_x) to rounding (rotations about
    one axis commute), and its origin has risen by W sin(th_x) within the error of the explicit integration.  p advances by
    R2[:, 2] W w dt before R2 turns, i.e. the height by the left Riemann sum of W cos(th) over N steps of h = w dt: each step errs by at most
    max|d/dth W cos| h^2 / 2 <= W h^2 / 2, so the bound is c N (w dt)^2 with c = W / 2."""
    N, w, n = 200, 0.8, 300.0
    c0, s0 = np.cos(0.3), np.sin(0.3)
    R0 = np.array([[c0, -s0, 0.0], [s0, c0, 0.0], [0.0, 0.0, 1.0]])
    rows, p, anchors = tm.reset(1), _params(L, W), _anchor(R0)
    rows[0, 0], rows[0, 1], rows[0, tm.O_TH], rows[0, tm.O_TIPPING] = W * w, w, 1e-9, 1.0   # (an angle that marks the edge y = -W)
    for _ in range(N):
        tm.step(rows, p, np.array([[1.0, 0.0]]), _wrench(fz=n, tx=-W * n), DT, anchors=anchors)
    r = tm.unpack(rows)
    th = r["th"][0, 0, 0]
    assert r["v"][0, 0, 1] == w and np.isclose(th, 1e-9 + N * w * DT, rtol=1e-13) and r["tip_steps"][0, 0] == N and r["peak_angle"][0, 0] == th
    want = R0 @ tm.exp_rotation(th - 1e-9, 0.0)
    assert np.max(np.abs(anchors[0, 0, :9].reshape(3, 3) - want)) < 1e-13
    rise = anchors[0, 0, 11] - 0.0
    bound = 0.5 * W * N * (w * DT) ** 2
    assert 0.0 < rise - W * np.sin(th - 1e-9) <= bound, (rise, W * np.sin(th), bound)
    assert abs(rise - W * np.sin(th - 1e-9)) > 0.01 * bound   # (the bound is of the error's order: the check could fail)
    assert np.array_equal(anchors[0, 1], _anchor(R0)[0, 1])   # (the free sole's anchor is the contact rule's business)


def test_robots_are_independent_and_reversed_rows_give_reversed_results():
    rng = np.random.default_rng(3)
    B = 5
    p = _params(np.array([0.1, 0.05, np.inf, 0.02, 0.1]), np.array([0.075, np.inf, 0.01, 0.03, 0.005]), batch=B)
    a, b = tm.reset(B), tm.reset(B)
    one = [tm.reset(1) for _ in range(B)]
    for k in range(40):
        w = rng.normal(size=(B, 2, 6)) * np.array([60.0, 60.0, 0.0, 30.0, 30.0, 3.0]) * (1.0 if k < 20 else 0.1)
        w[:, :, 2] = rng.uniform(50.0, 400.0, size=(B, 2))
        t = (rng.uniform(size=(B, 2)) > 0.1).astype(float)
        tm.step(a, p, t, w, DT)
        tm.step(b, p[::-1], t[::-1], w[::-1], DT)
        for i in range(B):
            tm.step(one[i], p[i:i + 1], t[i:i + 1], w[i:i + 1], DT)
    assert np.array_equal(a, b[::-1]) and np.array_equal(a, np.concatenate(one))
    r = tm.unpack(a)
    assert np.any(r["tip_steps"] > 0) and np.any(r["landings"] > 0) and np.all(r["th"][2, :, 1] == 0.0) and np.all(r["th"][1, :, 0] == 0.0)


def test_the_default_slider_inertia_is_stable_for_the_whole_robot():
    """G dt / I_tip <= 0.5 for G = Kd (the inertia bound), which exceeds the robot's roll and pitch inertia about either sole origin"""
    from mpc_benchmark_amd.robot import minipin as pin
    rb = Robot()
    m = rb.model
    row = tm.defaults(m, rb.x0[:m.nq], FOOT_FRAMES, DT)
    assert np.all(np.isinf(row[:4])) and tm.validate(row[None, :]).shape == (1, tm.PARAMS) and row[tm.P_W_MAX] == 5.0 and row[tm.P_TH_MAX] == 0.5
    data = m.createData()
    pin.framesForwardKinematics(m, data, rb.x0[:m.nq])
    for fid in rb.foot_frame_ids:
        o = data.oMf[fid].translation
        for axis in (0, 1):
            inertia = 0.0
            for j in range(1, m.njoints):
                Y, M = m.inertias[j], data.oMi[j]
                c = M.rotation @ Y.lever + M.translation - o
                inertia += Y.mass * (c @ c - c[axis] ** 2) + (M.rotation @ Y.inertia @ M.rotation.T)[axis, axis]
            assert tm.KD * inertia * DT / row[tm.P_I_TIP] <= 0.5, (axis, inertia, row)
    # a dict over the defaults, and the refusal of a finite extent without the slider's inertia
    p = tm.rows({"half_width": 0.03, "half_length_right": 0.08}, 2, base=row)
    assert np.array_equal(p[0], [np.inf, 0.08, 0.03, 0.03, row[4], row[5], row[6], 0.0])
    with pytest.raises(ValueError, match="I_tip"):
        tm.rows({"half_width": 0.03}, 2)
    assert np.array_equal(tm.rows({}, 3), np.tile(tm.IDENTITY, (3, 1)))


def test_validate_rows_and_unpack_refuse_what_they_should():
    row = np.array(tm.IDENTITY)
    for bad in ({"half_width": -0.1}, {"half_length": np.nan}, {"half_width_left": -np.inf}, {"I_tip": 0.0}, {"I_tip": np.inf}, {"w_max": -1.0},
                {"w_max": np.nan}, {"th_max": 0.0}, {"th_max": np.inf}, {"reserved": 1.0}):
        with pytest.raises(ValueError):
            tm.validate(tm.rows(bad, 1, base=row))
    assert tm.validate(tm.rows({"half_width": 0.0, "half_length": np.inf}, 2, base=row)).shape == (2, tm.PARAMS)
    with pytest.raises(ValueError, match="unknown"):
        tm.rows({"width": 0.1}, 1, base=row)
    with pytest.raises(ValueError, match="shape"):
        tm.rows({"half_width": np.ones(3)}, 2, base=row)
    with pytest.raises(ValueError, match="expected"):
        tm.rows(np.ones((2, 7)), 2)
    with pytest.raises(ValueError, match="expected"):
        tm.validate(np.ones((2, 7)))
    with pytest.raises(ValueError, match="expected"):
        tm.unpack(np.zeros((2, tm.WIDTH - 1)))
    for bad_rows in (np.zeros((1, tm.WIDTH - 1)), np.zeros((1, tm.WIDTH), dtype=np.float32), [[0.0] * tm.WIDTH]):
        with pytest.raises(ValueError, match="rows"):
            tm.step(bad_rows, tm.rows(tm.IDENTITY, 1), np.ones((1, 2)), np.zeros((1, 12)), DT)
    with pytest.raises(ValueError, match="in_contact"):
        tm.step(tm.reset(1), tm.rows(tm.IDENTITY, 1), np.ones((1, 3)), np.zeros((1, 12)), DT)
    with pytest.raises(ValueError, match="anchors"):
        tm.step(tm.reset(1), tm.rows(tm.IDENTITY, 1), np.ones((1, 2)), np.zeros((1, 12)), DT, anchors=np.zeros((1, 2, 9)))
    assert set(tm.unpack(tm.reset(2))) == {"v", "th", "tipping", "tip_steps", "peak_angle", "peak_excess", "landings", "steps"}


def test_the_tipping_reference_without_a_tip_is_the_friction_reference():
    """tests/_tipping_reference.py restates the step for a full 6-vector: with friction's components alone it is tests/_friction_reference.step to
    rounding, and a tip velocity changes the step at first order in Kd vs dt"""
    from tests import _friction_reference as fr
    from tests import _plant_cases as cases
    from tests import _tipping_reference as tr
    rb = Robot()
    x, tau = cases.states(rb, 1)
    slip = np.array([[0.05, -0.02, 0.1], [-0.03, 0.04, -0.2]])
    for mask in cases.MASKS:
        want = fr.step(rb.model, rb.foot_frame_ids, rb.foot_placements, mask, x[0], tau[0], slip, DT)
        got = tr.step(rb.model, rb.foot_frame_ids, rb.foot_placements, mask, x[0], tau[0], [tr.slip_vector(s) for s in slip], DT)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        tipped = tr.step(rb.model, rb.foot_frame_ids, rb.foot_placements, mask, x[0], tau[0],
                         [tr.slip_vector(slip[0]) + tr.tip_vector((0.0, 0.2, 0.0)), tr.slip_vector(slip[1])], DT)
        v0 = tr.sole_state(rb.model, rb.foot_frame_ids, got[0])[1][0, 3]
        v1 = tr.sole_state(rb.model, rb.foot_frame_ids, tipped[0])[1][0, 3]
        assert abs((v1 - v0) - 50.0 * DT * 0.2) < 0.05 * 50.0 * DT * 0.2, (v0, v1)


def test_the_mirror_scenario_meets_its_conditions_on_the_reference():
    """The inputs of the GPU comparison of kernel and mirror, run as a simulation on the CPU reference: at least half of the 8 robots tip, at least
    one lands again, the robot of infinite extents never tips, and no branch comes closer than 1e-6 (relative) to its threshold"""
    from tests import _tipping_reference as tr
    rb = Robot()
    m = rb.model
    params = tr.mirror_params(tm.defaults(m, rb.x0[:m.nq], FOOT_FRAMES, DT))
    q0 = rb.x0[:m.nq].copy()
    gz = min(float(M.translation[2]) for M in rb.foot_placements)
    push = tr.lateral_push(rb.x0, gz, tr.MIRROR_FORCE)
    tipped, landed, margin = [], [], np.inf
    for p in params:
        out = tr.simulate(m, rb.foot_frame_ids, rb.foot_placements, rb.x0, p, DT, tr.MIRROR_STEPS, lambda x, k: tr.posture_torques(m, q0, x, 300.0, 3.0),
                          push=lambda k: push if k < tr.MIRROR_PUSH_STEPS else None, cfg={"ground_z": gz})
        r = tm.unpack(out["rows"][-1:])
        tipped.append(bool(np.any(r["tip_steps"] > 0))), landed.append(bool(np.any(r["landings"] > 0)))
        margin = min(margin, out["margin"])
        assert np.all(out["in_contact"] == 1.0)
    print("mirror scenario on the reference: tipped %s, landed %s, the closest branch %.1e" % (tipped, landed, margin))
    assert sum(tipped) >= 4 and sum(landed) >= 1 and not tipped[-1] and margin > 1e-6, (tipped, landed, margin)


def test_the_mechanism_scenario_meets_its_conditions_on_the_reference():
    """The inputs of the GPU test of the mechanism on the CPU reference.  Its figures (printed): the narrow robot's soles roll by -5.99e-3 and
    -5.81e-3 rad, towards the push; a sole's LOCAL angular velocity lies within 0.293 of the state's w_x once the axis has tipped for 5 / Kd; the
    carrying edge stays within 1.7e-5 m of ground height while the origin rises by 6.0e-5 m (0.285 of the rise); the robot of infinite extents
    rolls by 4e-12 rad.  The conditions are about twice these figures: 0.6, 0.6 of the rise, and a roll 1000 times below the narrow robot's"""
    from tests import _tipping_reference as tr
    rb = Robot()
    m, fids = rb.model, rb.foot_frame_ids
    base = tm.defaults(m, rb.x0[:m.nq], FOOT_FRAMES, DT)
    q0, tau0 = rb.x0[:m.nq].copy(), tr.static_torques(m, fids, rb.x0[:m.nq])
    gz = min(float(M.translation[2]) for M in rb.foot_placements)
    fig = {}
    for half_width in (tr.DIR_HALF_WIDTH, np.inf):
        p = base.copy()
        p[tm.P_WIDTH:tm.P_WIDTH + 2] = half_width
        out = tr.simulate(m, fids, rb.foot_placements, rb.x0, p, DT, tr.DIR_STEPS, lambda x, k: tr.posture_torques(m, q0, x, tr.DIR_KP, tr.DIR_KD, tau0),
                          push=lambda k: tr.lateral_push(rb.x0, gz, tr.DIR_FORCE), cfg={"ground_z": gz})
        fig[half_width] = tr.mechanism_figures(m, fids, out["x"], out["rows"], half_width, gz, DT)
        fig[half_width]["th"] = out["rows"][-1, [tm.O_TH, tm.O_TH + 2]]
        assert np.all(out["in_contact"] == 1.0) and out["margin"] > 1e-6
    a, b = fig[tr.DIR_HALF_WIDTH], fig[np.inf]
    print("mechanism scenario on the reference: roll %s (narrow), %s (inf); th_x %s; lag %.3f; edge %.2e rise %.2e" % (a["roll"], b["roll"], a["th"], a["lag"], a["edge"], a["rise"]))
    assert np.all(a["roll"] < 0.0) and np.all(a["th"] < 0.0) and np.all(np.abs(b["roll"]) <= 1e-3 * np.abs(a["roll"]))
    assert 0.0 < a["lag"] <= 0.6 and a["rise"] > 0.0 and a["edge"] <= 0.6 * a["rise"]
