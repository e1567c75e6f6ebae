"""Per-robot joint end-stops of the torque-driven simulator in numpy (mpc_benchmark_amd/joint_stops.py): the definition the device kernel
(include/mpc_sim_joint_stops.h, csrc/sim_joint_stops.h) is held to in tests/test_gpu_sim_joint_stops.py.  Here the definition itself: the layout and
the bindings, infinite limits, the sign, the limit itself, the cap, a seized joint, the counters on a hand-written sequence, ``limits``, the
refusals, and one physical check: a 1-DoF joint of unit inertia running into a stop."""
import glob
import os
import re

import numpy as np
import pytest

from mpc_benchmark_amd import _capi
from mpc_benchmark_amd import joint_stops as js
from mpc_benchmark_amd.problems.common import Robot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mpc_sim_joint_stops", "mpc_sim_joint_stops_read", "mpc_sim_joint_stops_set", "mpc_sim_joint_stops_width")
INF = np.inf


def _row(k=0.0, d=0.0, cap=INF, batch=1):
    return js.rows({"k": k, "d": d, "cap": cap}, batch)


def test_header_and_bindings_agree():
    text = open(os.path.join(ROOT, "include", "mpc_sim_joint_stops.h")).read()
    assert set(re.findall(r"^(?:int|int32_t) (mpc_\w+)\(", text, re.M)) == set(SYMBOLS) == set(_capi._SIM_JOINT_STOPS_SIGNATURES)
    assert int(re.search(r"#define MPC_SIM_JOINT_STOPS_PARAMS (\d+)", text).group(1)) == js.PARAMS == len(js.IDENTITY) == len(js.DEFAULTS) == 8
    assert js.width(22) == 5 * 22 + 2 and js.reset(3, 22).shape == (3, 112) and not js.reset(3, 22).any()
    assert [e for e in _capi._HIP_ONLY if e[0] == "mpc_sim_joint_stops.h"][0][1] is _capi._SIM_JOINT_STOPS_SIGNATURES
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if not path.endswith("mpc_sim_joint_stops.h"):
            assert "mpc_sim_joint_stops(" not in open(path).read(), path


def test_hip_library_exports_the_entry_points():
    lib = _capi.bind_library(_capi.HIP_LIBRARY_PATH)   # (dlopen works without a GPU; nothing is computed)
    assert all(hasattr(lib, n) for n in SYMBOLS)


def test_the_oracle_does_not_export_the_joint_stops(oracle_lib):
    from mpc_benchmark_amd.pipeline import build_torque_simulator
    sim, _ = build_torque_simulator(oracle_lib, Robot(), 2, 1e-3, 0)
    nu = sim.dims.nu
    for call in (lambda: sim.joint_stops(js.IDENTITY, np.zeros(nu), np.zeros(nu)), lambda: sim.read_joint_stops(),
                 lambda: sim.set_joint_stops(js.reset(2, nu))):
        with pytest.raises(RuntimeError, match="HIP only"):
            call()
    sim.close()


def test_rows_take_the_three_forms():
    assert np.array_equal(js.rows({}, 3), np.tile(js.DEFAULTS, (3, 1)))
    assert np.array_equal(js.rows({"k": [1.0, 2.0, 3.0]}, 3)[:, 0], [1.0, 2.0, 3.0])
    assert np.array_equal(js.rows(js.IDENTITY, 2), np.tile(js.IDENTITY, (2, 1)))
    for bad in ({"stiffness": 1.0}, {"k": [1.0, 2.0]}, np.zeros((2, 8)), np.zeros(7)):
        with pytest.raises(ValueError, match="joint_stops"):
            js.rows(bad, 3)


def test_infinite_limits_give_exactly_zero():
    rng = np.random.default_rng(0)
    B, nu = 3, 5
    state, rows = js.reset(B, nu), _row(50.0, 3.0, 2.0, B)
    lo, hi = np.full((B, nu), -INF), np.full((B, nu), INF)
    for _ in range(4):
        tau = js.step(state, rows, lo, hi, rng.normal(size=(B, nu)) * 1e3, rng.normal(size=(B, nu)) * 1e3)
        assert np.all(tau == 0.0) and not np.any(np.signbit(tau))
    s = js.unpack(state, nu)
    assert not state[:, :5 * nu + 1].any() and not np.any(np.signbit(state)) and np.array_equal(s["steps"], np.full(B, 4.0))
    u = rng.normal(size=(B, nu))
    u[0, 0] = -0.0
    got = js.integrated(u, tau)
    assert np.array_equal(got, u) and np.signbit(got[0, 0])   # (an assignment: -0 stays -0)


def test_the_sign_always_points_into_the_range_and_nothing_acts_on_a_limit():
    rng = np.random.default_rng(1)
    B, nu = 2, 64
    lo, hi = np.full((B, nu), -0.3), np.full((B, nu), 0.7)
    q, v = rng.uniform(-1.0, 1.5, size=(B, nu)), rng.normal(size=(B, nu)) * 5.0
    q[0, :4], v[0, :4] = (0.7, -0.3, 0.7, -0.3), (9.0, -9.0, -9.0, 9.0)   # exactly on a limit, moving outwards and inwards
    state = js.reset(B, nu)
    tau = js.step(state, _row(20.0, 1.0, INF, B), lo, hi, q, v)
    above, below, inside = q > 0.7, q < -0.3, (q >= -0.3) & (q <= 0.7)
    assert above.any() and below.any() and inside.any()
    assert np.all(tau[above] <= 0.0) and np.all(tau[below] >= 0.0) and np.all(tau[inside] == 0.0)
    assert np.any(tau[above] < 0.0) and np.any(tau[below] > 0.0)
    assert np.any(tau[above] == 0.0) and np.any(tau[below] == 0.0)   # (the damper never pulls: a joint leaving fast enough gets nothing)
    s = js.unpack(state, nu)
    assert np.array_equal(s["pen"][above], (q - 0.7)[above]) and np.array_equal(s["pen"][below], (q + 0.3)[below]) and np.all(s["pen"][inside] == 0.0)
    assert np.all(tau[0, :4] == 0.0) and np.all(s["hits"][0, :4] == 0.0)
    want = -(20.0 * (q - 0.7) + 1.0 * v)
    assert np.allclose(tau[above & (tau != 0.0)], want[above & (tau != 0.0)], rtol=1e-15, atol=0.0)


def test_the_cap_and_the_scale():
    nu = 4
    scale = np.array([1.0, 10.0, 100.0, 0.5])
    lo, hi = np.full((1, nu), -1.0), np.full((1, nu), 1.0)
    q = np.array([[1.01, 1.2, -1.2, -1.001]])
    state = js.reset(1, nu)
    tau = js.step(state, _row(10.0, 0.0, 0.5), lo, hi, q, np.zeros((1, nu)), scale)
    # t = 10 p = 0.1, 2, 2, 0.01: joints 1 and 2 clip at cap = 0.5
    assert np.allclose(tau, [[-0.1, -5.0, 50.0, 0.005]], rtol=1e-12) and np.all(np.abs(tau) <= 0.5 * scale)
    assert tau[0, 1] == -5.0 and tau[0, 2] == 50.0
    free = js.step(js.reset(1, nu), _row(10.0, 0.0, INF), lo, hi, q, np.zeros((1, nu)), scale)
    assert np.allclose(free, [[-0.1, -20.0, 200.0, 0.005]], rtol=1e-12)


def test_a_seized_joint_is_a_two_sided_spring():
    lo = hi = np.full((1, 3), 0.25)
    tau = js.step(js.reset(1, 3), _row(8.0, 0.5), lo, hi, np.array([[0.35, 0.25, 0.15]]), np.array([[0.0, 3.0, 0.0]]))
    assert np.allclose(tau, [[-0.8, 0.0, 0.8]], rtol=1e-12) and tau[0, 1] == 0.0
    # the damper of each side acts only against motion away from the angle
    tau = js.step(js.reset(1, 3), _row(0.0, 2.0), lo, hi, np.array([[0.35, 0.35, 0.15]]), np.array([[1.0, -1.0, -1.0]]))
    assert np.array_equal(tau, [[-2.0, 0.0, 2.0]])


def test_counters_and_hits_on_a_hand_written_sequence():
    """joint 0 in [-1, 1], joint 1 free, joint 2 seized at 0.5; k = 10, d = 1.  Step 4: joint 0 is beyond hi but leaves at -1 rad/s, 10 * 0.03 - 1 < 0:
    the damper is cut off, pen != 0 and no torque.  Step 7: joint 0 goes from below lo to above hi without a step inside: no new hit."""
    lo, hi = np.array([[-1.0, -INF, 0.5]]), np.array([[1.0, INF, 0.5]])
    q0 = [0.0, 1.0, 1.02, 1.03, 0.5, -1.01, 1.01]
    v0 = [0.0, 5.0, 0.0, -1.0, 0.0, 0.0, 0.0]
    q2 = [0.5, 0.5, 0.6, 0.4, 0.5, 0.5, 0.45]
    state, rows = js.reset(1, 3), _row(10.0, 1.0)
    taus = np.array([js.step(state, rows, lo, hi, np.array([[a, 7.0, c]]), np.array([[b, -3.0, 0.0]]))[0] for a, b, c in zip(q0, v0, q2)])
    s = js.unpack(state, 3)
    assert np.array_equal(taus[:, 0] != 0.0, [False, False, True, False, False, True, True]) and not taus[:, 1].any()
    assert np.array_equal(taus[:, 2] != 0.0, [False, False, True, True, False, False, True])
    assert np.array_equal(s["hits"], [[2.0, 0.0, 2.0]]) and np.array_equal(s["stop_steps"], [[3.0, 0.0, 3.0]])
    assert s["any_steps"][0] == 4.0 and s["steps"][0] == 7.0
    assert np.allclose(s["peak_pen"], [[0.03, 0.0, 0.1]], rtol=1e-12) and np.allclose(s["pen"], [[0.01, 0.0, -0.05]], rtol=1e-12)
    assert np.array_equal(s["tau_stop"][0], taus[-1]) and taus[-1, 0] < 0.0 < taus[-1, 2]


def test_limits_scale_about_the_middle_and_lock_what_they_are_told_to():
    m = Robot().model
    lo0, hi0 = np.asarray(m.lowerPositionLimit)[7:], np.asarray(m.upperPositionLimit)[7:]
    nu = lo0.shape[0]
    lo, hi = js.limits(m, 3)
    assert lo.shape == hi.shape == (3, nu) and np.array_equal(lo, np.tile(lo0, (3, 1))) and np.array_equal(hi, np.tile(hi0, (3, 1)))
    knee = m.joints[m.getJointId("leg_left_4_joint")].idx_q - 7
    lo, hi = js.limits(m, 3, range_scale=[1.0, 0.9, 1.0], margin=0.01, lock={2: {"leg_left_6_joint": 0.1, 0: -0.2}})
    assert np.allclose(lo[0], lo0 + 0.01) and np.allclose(hi[0], hi0 - 0.01)
    assert np.allclose(0.5 * (lo[1] + hi[1]), 0.5 * (lo0 + hi0)) and np.allclose(hi[1] - lo[1], 0.9 * (hi0 - lo0) - 0.02)
    assert np.isclose(hi[1, knee] - lo[1, knee], 0.9 * (hi0[knee] - lo0[knee]) - 0.02)
    ankle = m.joints[m.getJointId("leg_left_6_joint")].idx_q - 7
    assert lo[2, ankle] == hi[2, ankle] == 0.1 and lo[2, 0] == hi[2, 0] == -0.2
    free = np.ones(nu, dtype=bool)
    free[[ankle, 0]] = False
    assert np.allclose(lo[2, free], lo0[free] + 0.01) and np.allclose(hi[2, free], hi0[free] - 0.01)
    per_joint = np.ones((3, nu))
    per_joint[0, knee] = 0.5
    lo, hi = js.limits(m, 3, range_scale=per_joint)
    assert np.isclose(hi[0, knee] - lo[0, knee], 0.5 * (hi0[knee] - lo0[knee])) and np.array_equal(lo[1], lo0)
    for kw in (dict(margin=5.0), dict(range_scale=-1.0), dict(range_scale=[1.0, 1.0]), dict(lock={3: {0: 0.0}}), dict(lock={0: {nu: 0.0}}),
               dict(lock={0: {"no_such_joint": 0.0}}), dict(lock={0: {0: np.nan}})):
        with pytest.raises(ValueError, match="joint_stops"):
            js.limits(m, 3, **kw)


def test_refusals():
    lo, hi = np.full((2, 3), -1.0), np.full((2, 3), 1.0)
    ok = _row(1.0, 1.0, 1.0, 2)
    js.validate(ok, lo, hi, np.ones(3))
    js.validate(ok, lo, lo)   # (lo == hi is a seized joint)

    def bad_row(col, val):
        r = ok.copy()
        r[1, col] = val
        return r

    cases = [(bad_row(0, -1.0), lo, hi, None, "k and d"), (bad_row(1, -1.0), lo, hi, None, "k and d"), (bad_row(0, INF), lo, hi, None, "k and d"),
             (bad_row(2, 0.0), lo, hi, None, "cap"), (bad_row(2, np.nan), lo, hi, None, "cap"), (bad_row(5, 1.0), lo, hi, None, "reserved"),
             (ok, hi, lo, None, "lo > hi"), (ok, np.where(np.eye(2, 3) > 0, np.nan, lo), hi, None, "NaN"), (ok, np.full((2, 3), -INF), np.full((2, 3), -INF), None, "inf"),
             (ok, np.full((2, 3), INF), np.full((2, 3), INF), None, "inf"),
             (ok, lo, hi, np.array([1.0, 0.0, 1.0]), "scale"), (ok, lo, hi, np.array([1.0, INF, 1.0]), "scale"), (ok, lo, hi, np.ones(2), "scale"),
             (ok, lo[:1], hi[:1], None, "shape")]
    for p, a, b, sc, match in cases:
        with pytest.raises(ValueError, match=match):
            js.validate(p, a, b, sc)


def _bounce(k, d, v_in, stop=None):
    """A joint of unit inertia, no other torque, integrated semi-implicitly (v += dt tau, q += dt v) at 1 ms from 1 mm inside hi = 0 at speed v_in
    into the stop, until it is inside again -> (v_out, peak penetration).  ``stop``: the torque as a function of (q, v); None: the mirror."""
    dt, q, v = 1e-3, np.array([[-1e-3]]), np.array([[v_in]])
    lo, hi = np.array([[-INF]]), np.array([[0.0]])
    state, rows = js.reset(1, 1), _row(k, d)
    peak, entered = 0.0, False
    for _ in range(20000):
        tau = js.step(state, rows, lo, hi, q, v) if stop is None else stop(q, v)
        v = v + dt * tau
        q = q + dt * v
        peak = max(peak, float(q[0, 0]))
        entered = entered or q[0, 0] > 0.0
        if entered and q[0, 0] <= 0.0:
            return float(v[0, 0]), peak
    raise AssertionError("the joint never left the stop")


@pytest.mark.parametrize("v_in", [0.3, 1.0, 3.0])
def test_a_unit_inertia_joint_bounces_off_a_stop(v_in):
    """With d = 0 the stop is a spring: the joint leaves with |v_out| = |v_in| to within the integrator's error.  That error is measured here, on a
    one-sided spring written out in the test and integrated by the same scheme (the symplectic scheme keeps a modified energy; what is left comes from
    the fractions of a step at entry and exit, O(k dt p)), and the mirror is allowed 10 % over it.  With d > 0 the joint leaves strictly slower, by
    more than that error, and never faster than it came."""
    k = 400.0   # (k dt^2 = 4e-4 of the unit inertia: far inside the scheme's stability bound of 4)
    ideal, _ = _bounce(k, 0.0, v_in, stop=lambda q, v: np.where(q > 0.0, -k * q, 0.0))
    err = abs(abs(ideal) - v_in)
    v_out, peak = _bounce(k, 0.0, v_in)
    print("v_in %.1f: spring alone leaves at %.6f (integrator error %.2e), the mirror at %.6f, peak penetration %.4f" % (v_in, ideal, err, v_out, peak))
    assert v_out < 0.0 and abs(abs(v_out) - v_in) <= 1.1 * err + 4 * np.finfo(float).eps * v_in
    assert np.isclose(peak, v_in / np.sqrt(k), rtol=0.05)   # (energy: k p^2 = v^2)
    last = v_in
    for d in (1.0, 4.0, 16.0):   # (under the critical damping 2 sqrt(k) = 40, from which on the joint creeps back and never leaves)
        vd, _ = _bounce(k, d, v_in)
        print("   d %.0f: leaves at %.6f" % (d, vd))
        assert vd < 0.0 and abs(vd) < v_in - err and abs(vd) < last
        last = abs(vd)
