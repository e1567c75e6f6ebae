"""Locomotion metrics of the torque-driven simulator on the device (include/mpc_sim_metrics.h: mpc_sim_metrics, mpc_sim_metrics_read; csrc/sim_metrics.h)
against the numpy mirror (mpc_benchmark_amd/locomotion_metrics.py) applied to the per-step record of the same steps: mpc_simulate_torque and the
three device loops, a push, accumulation across calls and the reset, a fall; metrics on or off do not change what the simulator computes."""
import numpy as np
import pytest

from mpc_benchmark_amd import locomotion_metrics as lm
from mpc_benchmark_amd.pipeline import PUSH_FORCE, PUSH_THETA, build_torque_simulator
from mpc_benchmark_amd.problems.common import Robot
from tests.test_centroidal_pipeline import centroidal_pipeline
from tests.test_fulldynamic_pipeline import fulldynamic_pipeline
from tests.test_pipeline import _pipeline as kinodynamic_pipeline

DT = 1e-3
EXACT = ("steps", "cop_steps", "fall_step")
RELATIVE = ("time", "energy", "peak_power", "peak_h_lin", "peak_h_ang", "h_ang_z_sq")
METRES = ("margin_min", "margin_sum", "base_z0", "sole_z0", "com_first", "com_last")


def _sim(lib, mask=(True, True), batch=2, seed=7):
    rb = Robot()
    sim, tables = build_torque_simulator(lib, rb, batch, DT, 0)
    sim.set_stage(0, *tables[mask])
    rng = np.random.default_rng(seed)
    x = np.tile(rb.x0, (batch, 1))
    x[:, rb.model.nq:] += rng.normal(size=(batch, rb.model.nv)) * 0.05
    return rb, sim, tables, x, rng


def _near_zero_margins(recs, x_start, cfg=None):
    """per robot: steps with a CoP whose margin lies within 1e-12 m of zero (the device may count them either way)"""
    c = lm.config(cfg)
    n = 0
    for rec in recs:
        cp, loaded = lm.cop(rec["sole_R"], rec["sole_p"], rec["wrenches"], c["min_force"])
        mg = lm.margin(cp, lm.support_box(rec["sole_p"], loaded, c["half_length"], c["half_width"]))
        n = n + np.sum(loaded.any(axis=2) & (np.abs(mg) < 1e-12), axis=0)
    return n


def _agree(got, want, excused=0):
    for k in EXACT:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert np.all(np.abs(got["cop_outside"] - want["cop_outside"]) <= excused), (got["cop_outside"], want["cop_outside"])
    for k in RELATIVE:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    for k in METRES:
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-12, err_msg=k)


def _cat(recs):
    return {k: np.concatenate([r[k] for r in recs], axis=0) for k in recs[0]}


@pytest.mark.gpu
def test_simulate_torque_equals_the_mirror(hip_lib):
    """2 robots, double then single support, random torques, one call of two sub-steps, a push on some steps; record and metrics on together."""
    rb, sim, tables, x, rng = _sim(hip_lib)
    nu = rb.model.nv - 6
    sim.record(40)
    sim.metrics({})
    x_start, dts, xi = x.copy(), [], x
    for k in range(24):
        if k == 12:
            sim.set_stage(0, *tables[(True, False)])
        sim.set_push(np.array([[0.0, -150.0, 0.0, 0.0, 0.0, 0.0], [60.0, 30.0, 0.0, 0.1, 0.0, 0.9]]) if 4 <= k < 9 else None)
        sub = 2 if k == 7 else 1
        xi = sim.simulate_torque(xi if k == 0 else None, rng.normal(size=(2, nu)) * 8.0, sub, DT)
        dts.append(sub * DT)
    rec = sim.read_record()
    got, want = sim.read_metrics(), lm.from_record(rec, x_start, np.array(dts))
    print("simulate_torque: steps %s, cop_steps %s, energy %s" % (got["steps"], got["cop_steps"], got["energy"]))
    assert np.all(got["steps"] == 24) and np.all(got["cop_steps"] > 0)
    _agree(got, want, _near_zero_margins([rec], x_start))
    sim.record(0)
    sim.metrics(None)


def _loop_agrees(p, periods, push_periods=(), batch_push=None):
    """``periods`` ticks of pipeline p with record and metrics on, the metrics accumulated across the calls; then the reset and two more ticks"""
    p.sim.record(periods * p.substeps)
    p.sim.metrics({})
    x_start = p.x.copy()
    recs = []
    for t in range(periods):
        p.tick(push=batch_push if t in push_periods else None)
        recs.append(p.sim.read_record())
    got = p.sim.read_metrics(reset=True)
    _agree(got, lm.from_record(_cat(recs), x_start, p.sim_dt), _near_zero_margins(recs, x_start))
    assert np.all(got["steps"] == periods * p.substeps)
    # after the reset: nothing accumulated, nothing latched; the next steps latch again
    fresh = p.sim.read_metrics()
    assert np.all(fresh["steps"] == 0) and np.all(fresh["fall_step"] == -1) and np.all(np.isnan(fresh["base_z0"])) and np.all(np.isnan(fresh["margin_min"]))
    x_start, recs2 = p.x.copy(), []
    for _ in range(2):
        p.tick()
        recs2.append(p.sim.read_record())
    got2 = p.sim.read_metrics()
    _agree(got2, lm.from_record(_cat(recs2), x_start, p.sim_dt), _near_zero_margins(recs2, x_start))
    np.testing.assert_array_equal(got2["base_z0"], recs2[0]["x"][0, :, 2])
    p.sim.record(0)
    p.sim.metrics(None)
    return got


@pytest.mark.gpu
def test_device_loops_equal_the_mirror(hip_lib):
    """the three device loops with the scripts' walks, 6 periods at batch 8 (the kinodynamic one pushed in periods 2 - 3 with the script's force at the
    world origin), and the centroidal loop at batch 64"""
    B = 8
    push = np.tile(np.concatenate([PUSH_FORCE["kinodynamic"] * np.array([np.cos(PUSH_THETA), np.sin(PUSH_THETA), 0.0]), np.zeros(3)]), (B, 1))
    k = _loop_agrees(kinodynamic_pipeline(hip_lib, batch=B, walk={}), 6, (2, 3), push)
    c = _loop_agrees(centroidal_pipeline(hip_lib, batch=B, walk={}), 6)
    f = _loop_agrees(fulldynamic_pipeline(hip_lib, batch=B, walk={}), 6)
    for name, g in (("kinodynamic", k), ("centroidal", c), ("fulldynamic", f)):
        print("%s: energy %.3f J, peak power %.1f W, CoP steps %d of %d" % (name, g["energy"].mean(), g["peak_power"].max(), g["cop_steps"].sum(), g["steps"].sum()))
    wide = _loop_agrees(centroidal_pipeline(hip_lib, batch=64, walk={}), 3)
    assert wide["steps"].shape == (64,)


@pytest.mark.gpu
def test_metrics_do_not_perturb(hip_lib):
    """with metrics on, then off: the same bits as handles that never turned them on (simulate_torque, and the three loops over 3 periods)"""
    rb, a, _, x, rng = _sim(hip_lib)
    _, b, _, _, _ = _sim(hip_lib)
    tau = rng.normal(size=(2, rb.model.nv - 6)) * 5.0
    want = a.simulate_torque(x, tau, 1, DT, wrenches=True)
    for arm in (lambda: b.metrics({}), lambda: b.metrics(None)):
        arm()
        got = b.simulate_torque(x, tau, 1, DT, wrenches=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for make, out in ((lambda: kinodynamic_pipeline(hip_lib, walk={}), "forces"), (lambda: centroidal_pipeline(hip_lib, walk={}), "forces"),
                      (lambda: fulldynamic_pipeline(hip_lib, walk={}), "wrenches")):
        pa, pb = make(), make()
        pb.sim.metrics({})
        for t in range(3):
            if t == 2:
                pb.sim.metrics(None)
            pa.tick()
            pb.tick()
            assert np.array_equal(pa.x, pb.x) and np.array_equal(pa.torques, pb.torques) and np.array_equal(getattr(pa, out), getattr(pb, out)), t


@pytest.mark.gpu
def test_a_fall_is_detected(hip_lib):
    """zero torques in double support: the robots sink until the mirror says fallen (at most 1000 steps); the device agrees"""
    rb, sim, _, x, _ = _sim(hip_lib)
    tau = np.zeros((2, rb.model.nv - 6))
    sim.record(1000)
    sim.metrics({})
    recs, want = [], None
    sim.simulate_torque(x, tau, 1, DT)
    for _ in range(40):
        for _ in range(24):
            sim.simulate_torque(None, tau, 1, DT)
        recs.append(sim.read_record())
        want = lm.from_record(_cat(recs), x, DT)
        if np.all(want["fall_step"] >= 0):
            break
    got = sim.read_metrics()
    print("fall: steps %s, fall_step %s, base z %s -> %s" % (got["steps"], got["fall_step"], got["base_z0"], recs[-1]["x"][-1, :, 2]))
    assert np.all(want["fall_step"] >= 0)
    _agree(got, want, _near_zero_margins(recs, x))
    sim.record(0)


@pytest.mark.gpu
def test_errors(hip_lib):
    rb, sim, _, x, _ = _sim(hip_lib)
    assert hip_lib.mpc_sim_metrics_width(sim._h) == lm.WIDTH == 21
    with pytest.raises(RuntimeError, match="metrics are off"):
        sim.read_metrics()
    with pytest.raises(RuntimeError, match="finite and >= 0"):
        sim.metrics({"half_width": -0.05})
    sim.metrics({})
    sim.simulate_torque(x, np.zeros((2, rb.model.nv - 6)), 1, DT)
    assert np.all(sim.read_metrics()["steps"] == 1)
    sim.metrics({"min_force": 5.0})   # on again: reset
    got = sim.read_metrics()
    assert np.all(got["steps"] == 0) and np.all(got["fall_step"] == -1) and np.all(np.isnan(got["com_first"]))
    sim.metrics(None)
    with pytest.raises(RuntimeError, match="metrics are off"):
        sim.read_metrics()
