"""The per-robot actuator model of the torque-driven simulator in numpy (mpc_benchmark_amd/actuator_model.py): the definition the device kernel
(include/mpc_sim_actuators.h, csrc/sim_actuators.h) is held to in tests/test_gpu_sim_actuators.py.  Here the definition itself: identity, delay,
lag, saturation, friction, the checks, and the bindings (HIP library only)."""
import os
import re

import numpy as np
import pytest

from mpc_benchmark_amd import _capi
from mpc_benchmark_amd import actuator_model as am
from mpc_benchmark_amd.pipeline import build_torque_simulator
from mpc_benchmark_amd.problems.common import Robot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, DT = 5, 1e-3
SYMBOLS = ("mpc_sim_actuators", "mpc_sim_actuators_read", "mpc_sim_actuators_set", "mpc_sim_actuators_width")


def _row(**kw):
    return am.rows(kw, 1)


def _commands(n, B=1, seed=3):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, B, NU)) * 20.0, rng.normal(size=(n, B, NU))


def test_layout():
    assert am.PARAMS == 8 == len(am.FIELDS) and am.RING == 16 and am.width(NU) == 18 * NU + 2
    s = am.reset(3, NU)
    assert s.shape == (3, 18 * NU + 2) and not s.any()
    u = am.unpack(s, NU)
    assert u["ring"].shape == (3, 16, NU) and u["y"].shape == u["applied"].shape == (3, NU) and u["head"].shape == u["count"].shape == (3,)
    assert np.array_equal(am.rows(am.IDENTITY, 2), am.rows({}, 2)) and am.rows({"delay": [1, 2]}, 2)[:, 0].tolist() == [1.0, 2.0]
    with pytest.raises(ValueError, match="unknown"):
        am.rows({"lag": 1.0}, 2)
    with pytest.raises(ValueError, match="shape"):
        am.rows(np.zeros((3, 8)), 2)


def test_identity_row_is_the_command_bit_for_bit():
    """40 steps (past one wrap of the ring), v_eps arbitrary: applied == u, array_equal."""
    us, vs = _commands(40, B=2)
    p = am.rows({"v_eps": [0.0, 0.3]}, 2)
    s = am.reset(2, NU)
    for k in range(40):
        out = am.step(s, p, us[k], vs[k], DT)
        assert np.array_equal(out, us[k]) and np.array_equal(am.unpack(s, NU)["applied"], us[k]), k
    assert am.unpack(s, NU)["count"].tolist() == [40.0, 40.0]
    assert np.array_equal(am.commands(s, NU, 16), us[24:])


@pytest.mark.parametrize("d", [1, 3, 15])
def test_delay_alone(d):
    """output at step k >= d: command k - d bit for bit; before that command 0 (the line is primed with the first command)"""
    us, vs = _commands(40)
    s = am.reset(1, NU)
    for k in range(40):
        out = am.step(s, _row(delay=d), us[k], vs[k], DT)
        assert np.array_equal(out, us[max(0, k - d)]), k


def test_lag_alone_follows_the_exponential():
    """constant command w after a first command w0: after n further steps y = w + (w0 - w) exp(-n dt / tc), to 1e-13 relative"""
    rng = np.random.default_rng(5)
    w0, w = rng.normal(size=(1, NU)) * 30.0, rng.normal(size=(1, NU)) * 30.0
    tc = 4e-3
    s = am.reset(1, NU)
    out = am.step(s, _row(time_constant=tc), w0, np.zeros((1, NU)), DT)
    assert np.array_equal(out, w0)   # (primed)
    for n in range(1, 31):
        out = am.step(s, _row(time_constant=tc), w, np.zeros((1, NU)), DT)
        want = w + (w0 - w) * np.exp(-n * DT / tc)
        assert np.max(np.abs(out - want)) <= 1e-13 * np.max(np.abs(want)), n
    # the step length is the argument: twice the step, half the count
    s2 = am.reset(1, NU)
    am.step(s2, _row(time_constant=tc), w0, np.zeros((1, NU)), 2 * DT)
    for n in range(15):
        out2 = am.step(s2, _row(time_constant=tc), w, np.zeros((1, NU)), 2 * DT)
    assert np.max(np.abs(out2 - out)) <= 1e-13 * np.max(np.abs(out))


def test_saturation_clamps_the_output_and_not_the_state():
    limit = np.array([10.0, 20.0, 30.0, 40.0, 50.0])
    u = np.array([[100.0, -100.0, 5.0, -19.0, 26.0]])
    p = _row(sat=0.5, time_constant=2e-3)
    s = am.reset(1, NU)
    out = am.step(s, p, u, np.zeros((1, NU)), DT, limit=limit)
    assert np.array_equal(out, [[5.0, -10.0, 5.0, -19.0, 25.0]])
    assert np.array_equal(am.unpack(s, NU)["y"], u)             # the lag state keeps the unclamped value
    out = am.step(s, p, np.zeros((1, NU)), np.zeros((1, NU)), DT, limit=limit)
    want = u * np.exp(-DT / 2e-3)                                # ... and decays from it, not from the clamp
    assert np.allclose(am.unpack(s, NU)["y"], want, rtol=1e-13, atol=0.0)
    assert np.array_equal(out, np.clip(am.unpack(s, NU)["y"], -0.5 * limit, 0.5 * limit))


def test_friction_opposes_the_velocity():
    shape = np.array([1.0, 2.0, 0.5, 1.0, 0.0])
    v = np.array([[3.0, -2.0, 50.0, -1e-6, 4.0]])
    u = np.zeros((1, NU))
    out = am.step(am.reset(1, NU), _row(damping=0.7), u, v, DT, shape=shape)
    assert np.allclose(out, -shape * 0.7 * v, rtol=1e-15, atol=0.0)
    out = am.step(am.reset(1, NU), _row(coulomb=2.0, v_eps=1e-2), u, v, DT, shape=shape)
    assert np.all(out[0, :4] * v[0, :4] < 0.0) and out[0, 4] == 0.0       # the sign opposes v; a joint with shape 0 has none
    assert np.allclose(np.abs(out[0, :3]), 2.0 * shape[:3], rtol=1e-12)   # |v| >> v_eps: coulomb * s_j
    assert abs(out[0, 3]) < 2.0 * 1e-6 / 1e-2 * 1.0001                     # |v| << v_eps: smooth through zero
    both = am.step(am.reset(1, NU), _row(damping=0.7, coulomb=2.0, v_eps=1e-2), u + 1.0, v, DT)
    assert np.allclose(both, 1.0 - (0.7 * v + 2.0 * np.tanh(v / 1e-2)), rtol=1e-14)


@pytest.mark.parametrize("bad, match", [({"delay": 1.5}, "delay"), ({"delay": 16}, "delay"), ({"delay": -1}, "delay"), ({"scale": 0.0}, "scale"),
                                        ({"scale": np.nan}, "finite"), ({"time_constant": -1e-3}, "time_constant"), ({"damping": -1.0}, "damping"),
                                        ({"coulomb": -1.0}, "coulomb"), ({"sat": -0.1}, "sat"), ({"coulomb": 1.0, "v_eps": 0.0}, "v_eps"),
                                        ({"sat": 0.5}, "limit")])
def test_validate_rejects(bad, match):
    with pytest.raises(ValueError, match=match):
        am.validate(am.rows(bad, 2))
    with pytest.raises(ValueError, match=match):
        am.step(am.reset(2, NU), am.rows(bad, 2), np.zeros((2, NU)), np.zeros((2, NU)), DT)


def test_validate_accepts():
    p, lim, sh = am.validate(am.rows({"delay": 15, "scale": 0.5, "time_constant": 0.02, "damping": 1.0, "coulomb": 1.0, "v_eps": 0.1, "sat": 0.5}, 3),
                             np.ones(NU), None)
    assert p.shape == (3, 8) and lim.shape == (NU,) and sh is None
    with pytest.raises(ValueError, match="limit"):
        am.validate(am.rows({}, 1), -np.ones(NU), None)


def test_header_declares_the_entry_points_the_bindings_know():
    text = open(os.path.join(ROOT, "include", "mpc_sim_actuators.h")).read()
    assert set(re.findall(r"^(?:int|int32_t) (mpc_\w+)\(", text, re.M)) == set(SYMBOLS) == set(_capi._SIM_ACTUATORS_SIGNATURES)
    assert int(re.search(r"#define MPC_SIM_ACTUATORS_PARAMS (\d+)", text).group(1)) == am.PARAMS
    assert int(re.search(r"#define MPC_SIM_ACTUATORS_RING (\d+)", text).group(1)) == am.RING


def test_hip_library_exports_the_entry_points():
    lib = _capi.bind_library(_capi.HIP_LIBRARY_PATH)   # (dlopen works without a GPU; nothing is computed)
    assert all(hasattr(lib, n) for n in SYMBOLS)


def test_the_oracle_does_not_export_the_model(oracle_lib):
    """the model is HIP only: on an oracle handle the calls raise the error of the other simulator extensions"""
    sim, _ = build_torque_simulator(oracle_lib, Robot(), 2, DT, 0)
    assert not any(hasattr(oracle_lib, n) for n in SYMBOLS)
    for call in (lambda: sim.actuators(am.IDENTITY), lambda: sim.actuators(None), lambda: sim.read_actuators(),
                 lambda: sim.set_actuators(am.reset(2, sim.dims.nu))):
        with pytest.raises(RuntimeError, match="HIP only"):
            call()
