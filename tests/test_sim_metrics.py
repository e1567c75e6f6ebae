"""Locomotion metrics of the torque-driven simulator (include/mpc_sim_metrics.h) without a GPU: the header, the bindings and the libraries agree, the
oracle refuses them, and the numpy mirror (mpc_benchmark_amd/locomotion_metrics.py) follows the reference's definitions: talos_utils.computeCoP,
plot.py's support box (plot.py:145-164), joint power and energy (plot.py:488-520) and the fall rule of tools/push_recovery.py."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from mpc_benchmark_amd import _capi
from mpc_benchmark_amd import locomotion_metrics as lm
from mpc_benchmark_amd import trajectory_log as tl
from mpc_benchmark_amd.pipeline import build_torque_simulator
from mpc_benchmark_amd.problems.common import Robot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_METRICS = ("mpc_sim_metrics", "mpc_sim_metrics_read", "mpc_sim_metrics_width")


def _header():
    return open(os.path.join(ROOT, "include", "mpc_sim_metrics.h")).read()


def test_header_declares_the_entry_points_the_bindings_know():
    from tests.test_abi_library import _declared_functions
    assert _declared_functions("mpc_sim_metrics.h") == sorted(_capi._SIM_METRICS_SIGNATURES) == list(SIM_METRICS)
    assert not set(SIM_METRICS) & set(_declared_functions("mpc_abi.h"))
    assert not set(SIM_METRICS) & set(_declared_functions("mpc_sim_ext.h"))
    assert not set(SIM_METRICS) & set(_capi._SIM_EXT_SIGNATURES)


def test_width_fields_and_config_match_the_header():
    text = _header()
    assert int(re.search(r"#define MPC_SIM_METRICS_WIDTH (\d+)", text).group(1)) == 21 == lm.WIDTH
    assert sum(w for _, w in lm.FIELDS) == 21 and len({n for n, _ in lm.FIELDS}) == len(lm.FIELDS)
    body = re.search(r"typedef struct mpc_sim_metrics_config \{(.*?)\} mpc_sim_metrics_config;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"double\s+([a-z_]+)\s*;", body)
    assert names == list(lm.DEFAULTS) == [n for n, _ in _capi.MpcSimMetricsConfig._fields_]
    assert ctypes.sizeof(_capi.MpcSimMetricsConfig) == 8 * len(names)
    # the row layout documented in the header is FIELDS
    o = 0
    for name, w in lm.FIELDS:
        assert re.search(r"\b%d\b[^\n]*\b%s\b" % (o, name), text), (o, name)
        o += w


def test_hip_library_exports_the_entry_points():
    lib = ctypes.CDLL(_capi.HIP_LIBRARY_PATH)
    for name in SIM_METRICS:
        assert hasattr(lib, name), name


def test_oracle_refuses_the_metrics(oracle_lib):
    for name in SIM_METRICS:
        assert not hasattr(oracle_lib, name)
    sim, tables = build_torque_simulator(oracle_lib, Robot(), 2, 1e-3, 0)
    sim.set_stage(0, *tables[(True, True)])
    for call in (lambda: sim.metrics({}), lambda: sim.metrics(None), lambda: sim.read_metrics(), lambda: sim.read_metrics(reset=True)):
        with pytest.raises(RuntimeError, match="not exported by this library"):
            call()


def test_config_defaults_and_unknown_keys():
    assert lm.config(None) == lm.DEFAULTS == {"min_force": 1.0, "half_length": 0.1, "half_width": 0.05, "fall_drop": 0.2, "sole_lift": 0.02}
    assert lm.config({"half_width": 0.075})["half_width"] == 0.075
    with pytest.raises(ValueError, match="unknown"):
        lm.config({"foot_width": 0.05})


def _pose(R, p):
    return SimpleNamespace(rotation=np.asarray(R), translation=np.asarray(p))


def _rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def test_vectorised_cop_equals_compute_cop():
    rng = np.random.default_rng(3)
    n = 400
    R = np.array([[_rot(rng), _rot(rng)] for _ in range(n)])
    p = rng.normal(size=(n, 2, 3))
    w = rng.normal(size=(n, 2, 6)) * 50.0
    w[:, :, 2] = rng.choice([-20.0, 0.0, 0.5, 1.0, 1.5, 300.0, 700.0], size=(n, 2))  # around the 1 N threshold, both ways
    got, loaded = lm.cop(R, p, w)
    for i in range(n):
        want = tl.compute_cop(_pose(R[i, 0], p[i, 0]), _pose(R[i, 1], p[i, 1]), w[i, 0, :3], w[i, 0, 3:], w[i, 1, :3], w[i, 1, 3:])
        assert np.array_equal(loaded[i], w[i, :, 2] > 1.0)
        if not loaded[i].any():
            assert np.all(np.isnan(want)) and np.all(np.isnan(got[i]))
        else:
            np.testing.assert_allclose(got[i], want, rtol=1e-14, atol=1e-14)


def test_vectorised_cop_equals_the_reference_function_on_the_goldens():
    path = os.path.join(ROOT, "tests", "golden", "talos_utils_vectors.npz")
    g = np.load(path)
    rows = g["cop_in"]
    R = np.stack([rows[:, 0:9].reshape(-1, 3, 3), rows[:, 12:21].reshape(-1, 3, 3)], axis=1)
    p = np.stack([rows[:, 9:12], rows[:, 21:24]], axis=1)
    w = np.stack([rows[:, 24:30], rows[:, 30:36]], axis=1)
    got, _ = lm.cop(R, p, w)
    np.testing.assert_allclose(got, g["cop_out"], rtol=0, atol=1e-15)


def test_support_box_is_plot_py():
    L, W = 0.1, 0.05
    pl, pr = np.array([0.30, 0.09, 0.0]), np.array([0.10, -0.08, 0.02])
    soles = np.array([[pl, pr]] * 4)
    loaded = np.array([[True, True], [True, False], [False, True], [False, False]])
    x_lo, x_hi, y_lo, y_hi = lm.support_box(soles, loaded, L, W)
    both = (0.10 - L, 0.30 + L, -0.08 - W, 0.09 + W)   # plot.py:145-149, and the else branch (:160-164)
    want = [both, (0.30 - L, 0.30 + L, 0.09 - W, 0.09 + W), (0.10 - L, 0.10 + L, -0.08 - W, -0.08 + W), both]
    for i, box in enumerate(want):
        np.testing.assert_allclose((x_lo[i], x_hi[i], y_lo[i], y_hi[i]), box, rtol=0, atol=1e-15)
    # the signed margin: positive inside, the nearest edge
    m = lm.margin(np.array([[0.25, 0.0, 0.0], [0.45, 0.0, 0.0]]), tuple(np.array([b[i] for b in (both, both)]) for i in range(4)))
    np.testing.assert_allclose(m, [0.13 - 0.0, -0.05], rtol=0, atol=1e-15)


def _synthetic(S=6, B=3, nq=9, nv=8, seed=5):
    """a record of S steps for B robots of a model with nq, nv: standing states 1 m high, soles on the ground, double support"""
    rng = np.random.default_rng(seed)
    nx, nu = nq + nv, nv - 6
    x = rng.normal(size=(S, B, nx))
    x[:, :, 2] = 1.0
    tau = rng.normal(size=(S, B, nu)) * 20.0
    soles = np.zeros((S, B, 2, 3))
    soles[:, :, 0] = [0.0, 0.09, 0.0]
    soles[:, :, 1] = [0.0, -0.09, 0.0]
    wr = np.zeros((S, B, 2, 6))
    wr[:, :, :, 2] = 400.0
    wr[:, :, :, 3:5] = rng.normal(size=(S, B, 2, 2)) * 10.0
    rec = {"x": x, "tau": tau, "wrenches": wr, "com": rng.normal(size=(S, B, 3)), "momentum": rng.normal(size=(S, B, 6)),
           "sole_R": np.broadcast_to(np.eye(3), (S, B, 2, 3, 3)).copy(), "sole_p": soles}
    return rec, rng.normal(size=(B, nx)), nq


def test_power_and_energy_pair_torque_with_the_state_it_started_from():
    rec, x_start, nq = _synthetic()
    S, B = rec["x"].shape[:2]
    dt = np.array([1e-3, 1e-3, 2e-3, 1e-3, 5e-3, 1e-3])
    got, e1 = lm.from_record(rec, x_start, dt), lm.from_record(rec, x_start, 1e-3)
    # plot.py:494-520 per robot: us[i] with xs[i], the measurement before the step (xs[0] = x_start)
    for b in range(B):
        xs = [x_start[b]] + [rec["x"][k, b] for k in range(S - 1)]
        power = np.array([np.sum(np.abs(rec["tau"][k, b] * xs[k][nq + 6:])) for k in range(S)])
        assert got["steps"][b] == S and got["time"][b] == pytest.approx(dt.sum(), rel=1e-15)
        assert got["energy"][b] == pytest.approx(np.sum(power * dt), rel=1e-13)
        assert got["peak_power"][b] == pytest.approx(power.max(), rel=1e-15)
        assert e1["energy"][b] == pytest.approx(np.sum(power) * 0.001, rel=1e-13)  # the script's 1 ms steps: sum(power) * 0.001
        # the other pairing (the state after the step) is a different number
        wrong = sum(np.sum(np.abs(rec["tau"][k, b] * rec["x"][k, b, nq + 6:])) * dt[k] for k in range(S))
        assert abs(wrong - got["energy"][b]) > 1e-6


def test_momentum_cop_and_latches():
    rec, x_start, _ = _synthetic()
    S, B = rec["x"].shape[:2]
    got = lm.from_record(rec, x_start, 1e-3)
    h = rec["momentum"]
    np.testing.assert_allclose(got["peak_h_lin"], np.max(np.linalg.norm(h[:, :, :3], axis=2), axis=0), rtol=1e-15)
    np.testing.assert_allclose(got["peak_h_ang"], np.max(np.linalg.norm(h[:, :, 3:], axis=2), axis=0), rtol=1e-15)
    np.testing.assert_allclose(got["h_ang_z_sq"], np.sum(h[:, :, 5] ** 2, axis=0), rtol=1e-14)
    c, loaded = lm.cop(rec["sole_R"], rec["sole_p"], rec["wrenches"])
    mg = lm.margin(c, lm.support_box(rec["sole_p"], loaded))
    assert np.all(got["cop_steps"] == S)
    np.testing.assert_array_equal(got["cop_outside"], np.sum(mg < 0, axis=0))
    np.testing.assert_allclose(got["margin_min"], mg.min(axis=0), rtol=0, atol=1e-15)
    np.testing.assert_allclose(got["margin_sum"], mg.sum(axis=0), rtol=0, atol=1e-14)
    np.testing.assert_array_equal(got["base_z0"], rec["x"][0, :, 2])
    np.testing.assert_array_equal(got["sole_z0"], rec["sole_p"][0, :, :, 2])
    np.testing.assert_array_equal(got["com_first"], rec["com"][0])
    np.testing.assert_array_equal(got["com_last"], rec["com"][-1])
    assert np.all(got["fall_step"] == -1)
    # no sole loaded: no CoP, margin_min NaN, nothing counted
    rec["wrenches"][:, :, :, 2] = 0.5
    got = lm.from_record(rec, x_start, 1e-3)
    assert np.all(got["cop_steps"] == 0) and np.all(np.isnan(got["margin_min"])) and np.all(got["margin_sum"] == 0)
    # nothing recorded: the rows of a reset
    empty = lm.from_record({k: v[:0] for k, v in rec.items()}, x_start, 1e-3)
    assert np.all(empty["steps"] == 0) and np.all(empty["fall_step"] == -1) and np.all(np.isnan(empty["base_z0"])) and np.all(np.isnan(empty["com_last"]))


def test_the_three_fall_rules_and_the_freeze():
    rec, x_start, _ = _synthetic(S=8, B=4)
    # robot 0: the base sinks 0.2 m + at step 5 (and not before: exactly 0.2 is not below)
    rec["x"][3, 0, 2] = 0.8
    rec["x"][5:, 0, 2] = 0.79
    # robot 1: both soles 2 cm + above their heights at step 4; at step 2 only one sole is
    rec["sole_p"][2, 1, 0, 2] = 0.05
    rec["sole_p"][4:, 1, :, 2] = 0.0201
    rec["sole_p"][3, 1, :, 2] = 0.02
    # robot 2: a non-finite state at step 6, finite again afterwards: the row freezes before step 6
    rec["x"][6, 2, 7] = np.nan
    got = lm.from_record(rec, x_start, 1e-3)
    np.testing.assert_array_equal(got["fall_step"], [5, 4, 6, -1])
    np.testing.assert_array_equal(got["steps"], [8, 8, 6, 8])
    assert np.all(np.isfinite(got["energy"])) and np.all(np.isfinite(got["margin_sum"]))
    six = lm.from_record({k: v[:6] for k, v in rec.items()}, x_start, 1e-3)
    for name in ("steps", "time", "energy", "peak_power", "cop_steps", "margin_sum", "peak_h_lin", "h_ang_z_sq", "com_last"):
        np.testing.assert_array_equal(got[name][2], six[name][2])
    # the fall of robots 0 and 1 does not stop the accumulation
    assert got["steps"][0] == got["steps"][1] == 8 and np.array_equal(got["com_last"][:2], rec["com"][-1, :2])
    # a non-finite state at the very first step: nothing latched
    rec["x"][0, 3, 0] = np.inf
    got = lm.from_record(rec, x_start, 1e-3)
    assert got["fall_step"][3] == 0 and got["steps"][3] == 0 and np.isnan(got["base_z0"][3])
