"""The per-robot actuator model of the torque-driven simulator on the device (include/mpc_sim_actuators.h: mpc_sim_actuators; csrc/sim_actuators.h
k_sim_actuators) against its numpy definition (mpc_benchmark_amd/actuator_model.py), in mpc_simulate_torque and in the three device loops; off and
identity mean unchanged bits; device loop against host glue with the model on; robots are independent; the state rows travel; the checks."""
import ctypes as C

import numpy as np
import pytest

from mpc_benchmark_amd import actuator_model as am
from tests._metrics import rel_cols
from tests.test_centroidal_pipeline import centroidal_pipeline
from tests.test_fulldynamic_pipeline import fulldynamic_pipeline
from tests.test_gpu_sim_push import DT, _sim
from tests.test_pipeline import _pipeline as kinodynamic_pipeline

B = 4
# identity | delay 3, lag 4 ms, gain 0.9 | delay 15, friction, saturation at half the limit | delay 1 with everything on
ROWS = np.array([am.IDENTITY,
                 (3.0, 0.9, 4e-3, 0.0, 0.0, 0.0, 0.0, 0.0),
                 (15.0, 1.0, 0.0, 0.1, 1.0, 0.05, 0.5, 0.0),
                 (1.0, 1.1, 2e-3, 0.05, 0.5, 0.1, 0.8, 0.0)])
PIPELINES = {"kinodynamic": kinodynamic_pipeline, "centroidal": centroidal_pipeline, "fulldynamic": fulldynamic_pipeline}


def _limit(nu):
    """effort limits for the random torques of ``_sim`` (sigma 5 N m): half of them, row 2's clamp, runs from 2 to 8 N m, so some joints clamp and some do not"""
    return np.linspace(4.0, 16.0, nu)


def _shape(nu):
    return np.linspace(0.5, 1.5, nu)


def _rows(batch):
    return ROWS[np.arange(batch) % len(ROWS)]


def _second(p):
    """the per-robot output beside x and torques: the QP's forces, or the full-dynamics pipeline's contact wrenches"""
    return p.forces if hasattr(p, "forces") else p.wrenches.reshape(p.batch, 12)


@pytest.mark.gpu
def test_off_and_identity_mean_unchanged_in_simulate_torque(hip_lib):
    """a handle that never armed the model, one that armed it and turned it off, one armed with identity rows: the same bits over 3 steps"""
    _, a, x, tau = _sim(hip_lib, batch=B)
    nu = tau.shape[1]
    handles = [a] + [_sim(hip_lib, batch=B)[1] for _ in range(2)]
    handles[1].actuators(_rows(B), limit=_limit(nu), friction_shape=_shape(nu))
    handles[1].actuators(None)
    handles[2].actuators(am.IDENTITY)
    xs = [x, x, x]
    for k in range(3):
        got = [h.simulate_torque(xi, tau * (1.0 + k), 1, DT, wrenches=True) for h, xi in zip(handles, xs)]
        for g in got[1:]:
            assert np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1]), k
        xs = [g[0] for g in got]
    with pytest.raises(RuntimeError, match="off"):
        handles[1].read_actuators()
    assert np.array_equal(handles[2].read_actuators()["applied"], tau * 3.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PIPELINES))
def test_off_and_identity_mean_unchanged_in_the_pipelines(hip_lib, name):
    """the same for 3 ticks of a pipeline: x, torques and forces (full dynamics: wrenches), as test_unarmed_means_unchanged does for the push"""
    make = lambda: PIPELINES[name](hip_lib, walk={})
    pa, pb, pc = make(), make(), make()
    pb.set_actuators(_rows(pb.batch))
    pb.set_actuators(None)
    pc.set_actuators(am.IDENTITY)
    for t in range(3):
        pa.tick(), pb.tick(), pc.tick()
        for p in (pb, pc):
            assert np.array_equal(pa.x, p.x) and np.array_equal(pa.torques, p.torques) and np.array_equal(_second(pa), _second(p)), t


def _drive(sim, x, substeps, steps=20, seed=11):
    """``steps`` calls of simulate_torque with a fresh random command each -> (commands (S, B, nu), start states (S, B, nx), final states)"""
    rng = np.random.default_rng(seed)
    us, xs = [], []
    for _ in range(steps):
        u = rng.normal(size=(x.shape[0], sim.dims.nu)) * 5.0
        us.append(u), xs.append(x)
        x = sim.simulate_torque(x, u, substeps, DT)
    return np.array(us), np.array(xs), x


def _mirror(rows, us, vs, dt, limit, shape):
    state = am.reset(us.shape[1], us.shape[2])
    out = np.array([am.step(state, rows, u, v, dt, limit=limit, shape=shape) for u, v in zip(us, vs)])
    return out, state


@pytest.mark.gpu
@pytest.mark.parametrize("substeps", [1, 4])
def test_kernel_equals_mirror(hip_lib, substeps):
    """20 calls of mpc_simulate_torque (the ring of 16 wraps), a fresh random command each, the record on: the applied torque of every step (the
    record's torque columns) and the state rows after the last are ``actuator_model.step`` driven with the same commands and the velocities of the
    states the steps started from, to 1e-12 of the largest |torque| (exp and tanh differ by a few ulp between numpy and the device; an indexing
    mistake is O(1)).  Robot 0, on the identity row, is its commands bit for bit.  substeps = 4: the lag sees substeps * dt, and the mirror driven
    with dt alone is far away.  Measured: applied 6e-17 (substeps 4: 1.5e-16), state rows 6e-17 of the largest |torque| (14.5 N m)."""
    rb, sim, x, _ = _sim(hip_lib, batch=B)
    nq, nu = rb.model.nq, sim.dims.nu
    limit, shape = _limit(nu), _shape(nu)
    sim.actuators(ROWS, limit=limit, friction_shape=shape)
    assert np.array_equal(sim.read_actuators(raw=True), am.reset(B, nu)) and np.array_equal(sim.read_actuators()["params"], ROWS)
    sim.record(20)
    us, xs, _ = _drive(sim, x, substeps)
    rec = sim.read_record()
    sim.record(0)
    assert np.array_equal(rec["x"][:-1], xs[1:])
    vs = xs[:, :, nq + 6:]
    want, state = _mirror(ROWS, us, vs, substeps * DT, limit, shape)
    scale = np.max(np.abs(want))
    e_tau = np.max(np.abs(rec["tau"] - want)) / scale
    got = sim.read_actuators(raw=True)
    e_state = np.max(np.abs(got - state)) / scale
    print("actuator kernel against the mirror, substeps %d: applied %.2e, state rows %.2e (largest |torque| %.1f)" % (substeps, e_tau, e_state, scale))
    assert e_tau < 1e-12 and e_state < 1e-12, (e_tau, e_state)
    assert np.array_equal(rec["tau"][:, 0], us[:, 0])
    assert np.array_equal(got[:, -2:], state[:, -2:])                       # head and count are exact
    assert np.array_equal(am.commands(got, nu, am.RING), us[-am.RING:])     # the rings hold the commands themselves
    for b in range(1, B):
        assert np.max(np.abs(rec["tau"][:, b] - us[:, b])) / scale > 1e-2, b   # (every other row acts)
    clamp = 0.5 * limit
    assert np.any(np.abs(state[2, 16 * nu:17 * nu]) > clamp) and np.any(np.abs(state[2, 16 * nu:17 * nu]) < clamp)   # row 2: some joints clamp, some do not
    if substeps > 1:
        wrong, _ = _mirror(ROWS, us, vs, DT, limit, shape)
        assert np.max(np.abs(rec["tau"] - wrong)) / scale > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PIPELINES))
def test_the_hook_is_in_every_loop(hip_lib, name):
    """One tick of the device loop with the record on: the rings hold the 10 commands of the period, the record the applied torques and the states.
    Commands and velocities replayed through the mirror reproduce the applied torques to 1e-12 of the largest |torque|; a non-identity robot's applied
    torques differ from its commands by more than 1e-6.  Measured: 4e-18 / 9e-19 / 0 against the mirror (kinodynamic, centroidal, full dynamics),
    0.12 / 0.15 / 0.14 between applied and commanded."""
    p = PIPELINES[name](hip_lib, walk={})
    nq, nu, n = p.nq, p.nv - 6, p.substeps
    rows, limit = _rows(p.batch), np.asarray(p.model.effortLimit, dtype=float)[6:]
    p.set_actuators(rows)
    p.sim.record(n)
    x0 = p.x.copy()
    p.tick()
    rec = p.sim.read_record()
    p.sim.record(0)
    got = p.sim.read_actuators(raw=True)
    assert rec["tau"].shape[0] == n == 10 and np.array_equal(am.unpack(got, nu)["count"], np.full(p.batch, float(n)))
    us = am.commands(got, nu, n)
    vs = np.concatenate([x0[None], rec["x"][:-1]])[:, :, nq + 6:]
    want, state = _mirror(rows, us, vs, p.sim_dt, limit, None)
    scale = np.max(np.abs(want))
    e = np.max(np.abs(rec["tau"] - want)) / scale
    acts = np.max(np.abs(rec["tau"][:, 1:] - us[:, 1:])) / scale
    print("%s device loop, applied torques against the mirror: %.2e; applied against commanded, robots 1..: %.2e" % (name, e, acts))
    assert e < 1e-12, e
    assert np.array_equal(rec["tau"][:, 0], us[:, 0]) and np.array_equal(rec["tau"][-1], p.torques)
    assert acts > 1e-6, acts
    assert np.max(np.abs(got - state)) / scale < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PIPELINES))
def test_device_loop_equals_host_glue_with_the_model_on(hip_lib, name):
    """4 ticks, device loop against host glue, both with the model on: x and torques (rel_cols, floors 1e-3 / 1).  No new number: each pipeline's own
    device-against-host tolerance without actuators.  Kinodynamic 2e-6 and centroidal 1e-12: tests/test_gpu_sim_push.py
    test_device_loops_equal_host_glue_under_a_push; full dynamics 1e-12 in the first period and 1e-10 after it: tests/test_gpu_fulldynamic_pipeline.py
    test_device_loop_equals_host_glue (TOL_FIRST, TOL_GLUE).  The host glue's ``torques`` is the applied torque read back after each step.
    Measured, per period: kinodynamic 3.6e-14 7.5e-14 3.5e-10 1.4e-10, centroidal 4.1e-13 2.7e-13 1.7e-13 1.0e-13, full dynamics 2.2e-14 3.4e-14
    1.9e-13 5.2e-12."""
    from tests.test_gpu_fulldynamic_pipeline import TOL_FIRST, TOL_GLUE
    tol = {"kinodynamic": (2e-6, 2e-6), "centroidal": (1e-12, 1e-12), "fulldynamic": (TOL_FIRST, TOL_GLUE)}[name]
    pd, ph = (PIPELINES[name](hip_lib, walk={}) for _ in range(2))
    for p in (pd, ph):
        p.set_actuators(_rows(p.batch))
    worst = []
    for t in range(4):
        pd.tick(), ph.tick(host_glue=True)
        worst.append(max(rel_cols(pd.x, ph.x, 1e-3), rel_cols(pd.torques, ph.torques, 1.0)))
    print("%s with actuators: device loop against host glue, per period: %s" % (name, " ".join("%.1e" % w for w in worst)))
    assert np.array_equal(ph.torques, ph.sim.read_actuators()["applied"])
    for t, w in enumerate(worst):
        assert w < tol[0 if t == 0 else 1], (t, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PIPELINES))
def test_robots_are_independent(hip_lib, name):
    """4 robots, robot 0 on the identity row and the others not: after 5 ticks robot 0 is bit for bit robot 0 of the same ensemble without the model,
    every other robot differs by more than 1e-6."""
    pa, pf = (PIPELINES[name](hip_lib, batch=B, walk={}) for _ in range(2))
    pa.set_actuators(ROWS)
    for _ in range(5):
        pa.tick(), pf.tick()
    assert np.array_equal(pa.x[0], pf.x[0]) and np.array_equal(pa.torques[0], pf.torques[0])
    diff = np.max(np.abs(pa.x[1:] - pf.x[1:]), axis=1)
    print("%s: robots 1 - 3 with against without the model after 5 ticks: %s" % (name, diff))
    assert np.all(diff > 1e-6), diff


@pytest.mark.gpu
def test_state_rows_round_trip(hip_lib):
    """7 steps, read, 5 more; a second handle after the same 7 steps and a third, freshly armed, take the rows read and give the same bits over the 5.
    Malformed rows are rejected and the rows in force stay."""
    rb, a, x, _ = _sim(hip_lib, batch=B)
    nu = a.dims.nu
    arm = lambda s: s.actuators(ROWS, limit=_limit(nu), friction_shape=_shape(nu))
    arm(a)
    _, _, x7 = _drive(a, x, 1, steps=7)
    rows7 = a.read_actuators(raw=True)
    us, _, want = _drive(a, x7, 1, steps=5, seed=12)
    b, c = _sim(hip_lib, batch=B)[1], _sim(hip_lib, batch=B)[1]
    arm(b), arm(c)
    _drive(b, x, 1, steps=7)
    for h in (b, c):
        h.set_actuators(rows7)
        assert np.array_equal(h.read_actuators(raw=True), rows7)
        assert np.array_equal(_drive(h, x7, 1, steps=5, seed=12)[2], want)
        assert np.array_equal(h.read_actuators(raw=True), a.read_actuators(raw=True))
    _, _, other = _drive(_sim(hip_lib, batch=B)[1], x7, 1, steps=5, seed=12)
    assert not np.array_equal(other[1:], want[1:])   # (the rows matter)
    held = b.read_actuators(raw=True)
    for col, val, match in ((3, np.nan, "finite"), (-2, 16.0, "head"), (-2, 1.5, "head"), (-1, -1.0, "count")):
        bad = rows7.copy()
        bad[2, col] = val
        with pytest.raises(RuntimeError, match=match):
            b.set_actuators(bad)
        assert np.array_equal(b.read_actuators(raw=True), held)
    with pytest.raises(ValueError, match="shape"):
        b.set_actuators(rows7[:, :-1])


@pytest.mark.gpu
def test_errors(hip_lib):
    """a bad parameter row, a handle of the wrong kind (a centroidal plan) and sat > 0 without limits: -1 with a message, the configuration in force unchanged"""
    _, sim, _, _ = _sim(hip_lib, batch=B)
    nu = sim.dims.nu
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    sim.actuators(ROWS, limit=_limit(nu))
    sim.simulate_torque(_sim(hip_lib, batch=B)[2], np.ones((B, nu)), 1, DT)
    held = sim.read_actuators()
    cases = [({"delay": 1.5}, True, "delay"), ({"delay": 16.0}, True, "delay"), ({"scale": 0.0}, True, "scale"), ({"damping": -1.0}, True, ">= 0"),
             ({"coulomb": 1.0, "v_eps": 0.0}, True, "v_eps"), ({"scale": np.inf}, True, "finite"), ({"sat": 0.5}, False, "limit")]
    for fields, with_limit, match in cases:
        bad = am.rows({k: [1.0 if k == "scale" else 0.0] * (B - 1) + [v] for k, v in fields.items()}, B)   # (the last row is the bad one)
        rc = hip_lib.mpc_sim_actuators(sim._h, dp(bad), dp(_limit(nu)) if with_limit else None, None)
        msg = hip_lib.mpc_last_error(sim._h).decode()
        assert rc == -1 and match in msg and (not with_limit or "row %d" % (B - 1) in msg), (fields, rc, msg)
        now = sim.read_actuators()
        assert all(np.array_equal(now[k], held[k]) for k in held), fields
    with pytest.raises(RuntimeError, match="limit"):
        sim.actuators({"sat": 0.5})
    plan = centroidal_pipeline(hip_lib, walk={}).mpc.native
    good = am.rows({}, plan.dims.batch)
    assert hip_lib.mpc_sim_actuators(plan._h, dp(good), None, None) == -1 and "simulator handle" in hip_lib.mpc_last_error(plan._h).decode()
    assert hip_lib.mpc_sim_actuators_width(plan._h) == -1 and hip_lib.mpc_sim_actuators_width(sim._h) == am.width(nu)
    for call in (lambda: plan.actuators(None), lambda: plan.read_actuators(), lambda: plan.set_actuators(np.zeros((plan.dims.batch, am.width(plan.dims.nu))))):
        with pytest.raises(RuntimeError, match="simulator handle"):
            call()
