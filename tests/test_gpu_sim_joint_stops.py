"""The per-robot joint end-stops of the torque-driven simulator on the device (include/mpc_sim_joint_stops.h: mpc_sim_joint_stops, _read, _set,
_width; csrc/sim_joint_stops.h k_sim_joint_stops) against their numpy definition (mpc_benchmark_amd/joint_stops.py), in mpc_simulate_torque and in
the three device loops: off and infinite limits mean unchanged bits; the kernel against the mirror on imposed states; the dynamics integrate the sum
while everything else keeps the actuators' torque; device loop against host glue with the model on; robots are independent; the state rows travel;
the checks."""
import ctypes as C

import numpy as np
import pytest

from mpc_benchmark_amd import joint_stops as js
from tests._metrics import rel_cols
from tests.test_centroidal_pipeline import centroidal_pipeline
from tests.test_fulldynamic_pipeline import fulldynamic_pipeline
from tests.test_gpu_sim_push import DT, _sim
from tests.test_pipeline import _pipeline as kinodynamic_pipeline

B = 4
INF = np.inf
PIPELINES = {"kinodynamic": kinodynamic_pipeline, "centroidal": centroidal_pipeline, "fulldynamic": fulldynamic_pipeline}
# robot 0: whatever row, it has no limits | a spring only | spring, damper and a cap that some joints reach and some do not | spring and damper, two
# seized joints
ROWS = np.array([(20.0, 0.1, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                 (20.0, 0.0, INF, 0.0, 0.0, 0.0, 0.0, 0.0),
                 (20.0, 0.1, 0.45, 0.0, 0.0, 0.0, 0.0, 0.0),
                 (10.0, 0.05, INF, 0.0, 0.0, 0.0, 0.0, 0.0)])
SEIZED = (3, 17)      # robot 3: the left knee and the left elbow
# what a joint goes through, one entry per call; joint j starts at entry j, so every call holds every case and every joint sees all of them twice in
# 20 calls (a second hit): inside, exactly on hi, 0.02 rad beyond hi, deeper, back inside, 0.01 rad below lo, exactly on lo, inside, beyond hi, inside
SWEEP = ("in", "hi", "above", "deeper", "in", "below", "lo", "in", "above", "in")


def _second(p):
    """the per-robot output beside x and torques: the QP's forces, or the full-dynamics pipeline's contact wrenches"""
    return p.forces if hasattr(p, "forces") else p.wrenches.reshape(p.batch, 12)


def _effort(rb):
    return np.asarray(rb.model.effortLimit, dtype=float)[6:]


def _tables(rb, x):
    """the limits of the four robots: robot 0 none, 1 and 2 the model's, 3 the model's with two joints seized where ``x`` has them"""
    lo, hi = js.limits(rb.model, B, lock={3: {j: float(x[3, 7 + j]) for j in SEIZED}})
    lo[0], hi[0] = -INF, INF
    return lo, hi


def _designed_states(rb, x, steps=20, seed=5):
    """``steps`` start states (S, B, nx): the base and the base velocity of ``x``, every joint placed by SWEEP against its robot's own limits (robot
    0, without limits, against the model's), joint velocities of both signs (sigma 2 rad/s: with d = 0.1 against k 0.02 = 0.4 the damper is cut
    off in some entries and drives others into the cap)"""
    rng = np.random.default_rng(seed)
    nq, nu = rb.model.nq, rb.model.nv - 6
    lo, hi = _tables(rb, x)
    lo[0], hi[0] = js.limits(rb.model, 1)
    out = np.tile(x, (steps, 1, 1))
    for s in range(steps):
        for j in range(nu):
            place = SWEEP[(s + j) % len(SWEEP)]
            u = rng.uniform(0.2, 0.8, size=B)
            out[s, :, 7 + j] = {"in": lo[:, j] + u * (hi[:, j] - lo[:, j]), "hi": hi[:, j], "lo": lo[:, j], "above": hi[:, j] + 0.02,
                                "deeper": hi[:, j] + 0.02 + 0.03 * u, "below": lo[:, j] - 0.01}[place]
        out[s, :, nq + 6:] = rng.normal(size=(B, nu)) * 2.0
    return out


def _beyond(x, nq, depth=0.01, reach=0.5, free=(0,)):
    """tables relative to the postures ``x`` (B, nx): every joint has ``reach`` rad to either side, but joints 2 and 15 begin ``depth`` beyond hi
    and joint 8 begins ``depth`` below lo; the robots in ``free`` have no limits"""
    q = x[:, 7:nq]
    lo, hi = q - reach, q + reach
    hi[:, [2, 15]] = q[:, [2, 15]] - depth
    lo[:, 8] = q[:, 8] + depth
    for b in free:
        lo[b], hi[b] = -INF, INF
    return lo, hi


@pytest.mark.gpu
def test_off_and_infinite_limits_mean_unchanged_in_simulate_torque(hip_lib):
    """a handle that never armed the model, one that armed it and turned it off, one armed with every limit infinite: the same bits over 3 steps"""
    rb, a, x, tau = _sim(hip_lib, batch=B)
    nu = tau.shape[1]
    handles = [a] + [_sim(hip_lib, batch=B)[1] for _ in range(2)]
    lo, hi = _beyond(x, rb.model.nq)
    handles[1].joint_stops(ROWS, lo, hi, _effort(rb))
    handles[1].joint_stops(None)
    handles[2].joint_stops(ROWS, np.full(nu, -INF), np.full(nu, INF), _effort(rb))
    xs = [x, x, x]
    for k in range(3):
        got = [h.simulate_torque(xi, tau * (1.0 + k), 1, DT, wrenches=True) for h, xi in zip(handles, xs)]
        for g in got[1:]:
            assert np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1]), k
        xs = [g[0] for g in got]
    with pytest.raises(RuntimeError, match="off"):
        handles[1].read_joint_stops()
    s = handles[2].read_joint_stops()
    assert not s["tau_stop"].any() and not s["hits"].any() and np.array_equal(s["steps"], np.full(B, 3.0)) and not s["any_steps"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PIPELINES))
def test_off_and_infinite_limits_mean_unchanged_in_the_pipelines(hip_lib, name):
    """the same for 3 ticks of a pipeline: x, torques and forces (full dynamics: wrenches)"""
    make = lambda: PIPELINES[name](hip_lib, walk={})
    pa, pb, pc = make(), make(), make()
    pb.set_joint_stops({})
    pb.set_joint_stops(None)
    pc.set_joint_stops({"lo": -INF, "hi": INF})
    assert pb.joint_stop_state() is None
    for t in range(3):
        pa.tick(), pb.tick(), pc.tick()
        for p in (pb, pc):
            assert np.array_equal(pa.x, p.x) and np.array_equal(pa.torques, p.torques) and np.array_equal(_second(pa), _second(p)), t
    assert np.array_equal(pc.joint_stop_state()["steps"], np.full(pc.batch, 3.0 * pc.substeps)) and not pc.joint_stop_state()["stop_steps"].any()


def test_the_designed_states_hold_every_case():
    """the mirror alone, on the CPU: the 20 imposed states of test_kernel_equals_mirror_on_imposed_states really contain a clipped and an unclipped
    stop torque, a damper cut off at 0, a second hit, joints exactly on a limit, and both signs; robot 0 is never touched"""
    rb = _sim_robot()
    x = np.tile(rb.x0, (B, 1))
    nq, nu = rb.model.nq, rb.model.nv - 6
    lo, hi = _tables(rb, x)
    xs = _designed_states(rb, x)
    state, scale = js.reset(B, nu), _effort(rb)
    taus = np.array([js.step(state, ROWS, lo, hi, xi[:, 7:nq], xi[:, nq + 6:], scale) for xi in xs])
    pens = np.array([np.where(xi[:, 7:nq] > hi, xi[:, 7:nq] - hi, np.where(xi[:, 7:nq] < lo, xi[:, 7:nq] - lo, 0.0)) for xi in xs])
    s = js.unpack(state, nu)
    assert not taus[:, 0].any() and not state[0, :5 * nu + 1].any()
    t2 = np.abs(taus[:, 2]) / scale
    assert np.any(np.isclose(t2, ROWS[2, 2], rtol=1e-14, atol=0.0)) and np.any((t2 > 0.0) & (t2 < 0.99 * ROWS[2, 2]))   # clipped and unclipped
    assert np.any((pens[:, 2] != 0.0) & (taus[:, 2] == 0.0))                                   # the damper cut off at 0
    assert np.all(s["hits"][1:] >= 2.0)                                                        # a second hit of every joint
    on = (xs[:, 1:, 7:nq] == hi[1:]) | (xs[:, 1:, 7:nq] == lo[1:])
    assert on.any() and not taus[:, 1:][on].any() and not pens[:, 1:][on].any()                # exactly on a limit: nothing
    assert np.any(taus > 0.0) and np.any(taus < 0.0)
    for j in SEIZED:
        assert np.any(taus[:, 3, j] > 0.0) and np.any(taus[:, 3, j] < 0.0)                     # a seized joint is held from both sides
    assert np.all(s["any_steps"][1:] == 20.0) and np.all(s["steps"] == 20.0)


def _sim_robot():
    from mpc_benchmark_amd.problems.common import Robot
    return Robot()


@pytest.mark.gpu
def test_kernel_equals_mirror_on_imposed_states(hip_lib):
    """20 calls of mpc_simulate_torque, each from a designed start state (test_the_designed_states_hold_every_case), a random command each: after
    every call the state rows are ``joint_stops.step`` of the same states: tau_stop, pen and peak_pen to 1e-12 of the largest |tau_stop| (the
    arithmetic differs by fused multiply-adds at the most; an indexing mistake is O(1)), stop_steps, hits, any_steps and steps exactly.
    Measured: 1.1e-16 of the largest |tau_stop| (261.2 N m)."""
    rb, sim, x, _ = _sim(hip_lib, batch=B)
    nq, nu = rb.model.nq, sim.dims.nu
    lo, hi = _tables(rb, x)
    scale = _effort(rb)
    sim.joint_stops(ROWS, lo, hi, scale)
    first = sim.read_joint_stops()
    assert np.array_equal(sim.read_joint_stops(raw=True), js.reset(B, nu))
    assert np.array_equal(first["params"], ROWS) and np.array_equal(first["lo"], lo) and np.array_equal(first["hi"], hi)
    assert hip_lib.mpc_sim_joint_stops_width(sim._h) == js.width(nu)
    xs = _designed_states(rb, x)
    rng = np.random.default_rng(11)
    state = js.reset(B, nu)
    wants = [js.step(state, ROWS, lo, hi, xi[:, 7:nq], xi[:, nq + 6:], scale).copy() for xi in xs]   # (the largest |tau_stop| of the sequence)
    big = np.max(np.abs(wants))
    state = js.reset(B, nu)
    worst = 0.0
    for k, xi in enumerate(xs):
        js.step(state, ROWS, lo, hi, xi[:, 7:nq], xi[:, nq + 6:], scale)
        out = sim.simulate_torque(xi, rng.normal(size=(B, nu)) * 5.0, 1, DT)
        assert np.all(np.isfinite(out))
        got = sim.read_joint_stops(raw=True)
        e = np.max(np.abs(got[:, :3 * nu] - state[:, :3 * nu])) / big
        worst = max(worst, e)
        assert e < 1e-12, (k, e)
        assert np.array_equal(got[:, 3 * nu:], state[:, 3 * nu:]), k
        assert np.array_equal(got[:, :nu] != 0.0, state[:, :nu] != 0.0) and np.array_equal(got[:, nu:2 * nu] != 0.0, state[:, nu:2 * nu] != 0.0), k
    print("joint stops against the mirror over 20 imposed states: %.2e of the largest |tau_stop| (%.1f N m)" % (worst, big))
    assert not got[0, :5 * nu + 1].any()


@pytest.mark.gpu
@pytest.mark.parametrize("with_actuators", [False, True])
def test_the_dynamics_integrate_the_sum_and_the_record_keeps_the_actuators_torque(hip_lib, with_actuators):
    """One step with the stops on under the command u; a second handle without any model, given applied + tau_stop (an assignment in place of an
    add where tau_stop == 0), gives the same state and wrenches bit for bit; the record's torque columns of the first handle are the applied torque:
    u itself, or with the actuator model on what that model applied."""
    rb, a, x, u = _sim(hip_lib, batch=B)
    b = _sim(hip_lib, batch=B)[1]
    lo, hi = _beyond(x, rb.model.nq)
    a.joint_stops(ROWS, lo, hi, _effort(rb))
    if with_actuators:
        a.actuators({"scale": [1.0, 0.9, 1.1, 0.8], "damping": 0.1, "sat": 0.5}, limit=np.linspace(4.0, 16.0, a.dims.nu))
    a.record(1)
    xa, wa = a.simulate_torque(x, u, 1, DT, wrenches=True)
    rec = a.read_record()
    a.record(0)
    tau_stop = a.read_joint_stops()["tau_stop"]
    applied = a.read_actuators()["applied"] if with_actuators else u
    assert with_actuators == (not np.array_equal(applied, u))
    assert np.array_equal(rec["tau"][0], applied)
    acts = tau_stop != 0.0
    assert not acts[0].any() and np.all(acts[1:, [2, 8, 15]]) and acts.sum() == 3 * (B - 1)
    assert np.all(tau_stop[1:, [2, 15]] < 0.0) and np.all(tau_stop[1:, 8] > 0.0)
    xb, wb = b.simulate_torque(x, js.integrated(applied, tau_stop), 1, DT, wrenches=True)
    assert np.array_equal(xa, xb) and np.array_equal(wa, wb)
    xc, _ = b.simulate_torque(x, applied, 1, DT, wrenches=True)
    assert np.array_equal(xa[0], xc[0]) and np.all(np.max(np.abs(xa[1:] - xc[1:]), axis=1) > 1e-6)


def _arm_beyond(p, free=(0,)):
    lo, hi = _beyond(p.x, p.nq, free=free)
    p.set_joint_stops({"lo": lo, "hi": hi})
    return js.rows({}, p.batch), lo, hi


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PIPELINES))
def test_the_hook_is_in_every_loop(hip_lib, name):
    """One tick of the device loop with the record on, three joints of every robot but robot 0 beginning 0.01 rad beyond a stop: the true states of
    the record replayed through the mirror give the state rows after the tick to 1e-12 of the largest |tau_stop|, the counters exactly, steps == 10;
    ``torques`` is the record's last torque row (the actuators' torque, not the sum); the robots with stops differ from a run without the model by
    more than 1e-6.  Measured: 0 / 0 / 5.6e-17 against the mirror (kinodynamic, centroidal, full dynamics; the largest |tau_stop| 32 N m),
    0.80 / 1.23 / 0.80 between with and without the model."""
    p, plain = (PIPELINES[name](hip_lib, walk={}) for _ in range(2))
    nq, nu, n = p.nq, p.nv - 6, p.substeps
    rows, lo, hi = _arm_beyond(p)
    scale = np.asarray(p.model.effortLimit, dtype=float)[6:]
    p.sim.record(n)
    x0 = p.x.copy()
    p.tick(), plain.tick()
    rec = p.sim.read_record()
    p.sim.record(0)
    got = p.sim.read_joint_stops(raw=True)
    xs = np.concatenate([x0[None], rec["x"][:-1]])
    state = js.reset(p.batch, nu)
    taus = np.array([js.step(state, rows, lo, hi, xi[:, 7:nq], xi[:, nq + 6:], scale) for xi in xs])
    big = np.max(np.abs(taus))
    e = np.max(np.abs(got[:, :3 * nu] - state[:, :3 * nu])) / big
    s = js.unpack(got, nu)
    diff = np.max(np.abs(p.x - plain.x), axis=1)
    print("%s device loop, state rows against the mirror: %.2e of the largest |tau_stop| (%.1f N m); with against without the model: %s" % (name, e, big, diff))
    assert rec["tau"].shape[0] == n == 10 and np.array_equal(s["steps"], np.full(p.batch, 10.0))
    assert e < 1e-12, e
    assert np.array_equal(got[:, 3 * nu:], state[:, 3 * nu:])
    assert np.array_equal(rec["tau"][-1], p.torques)
    assert np.all(s["hits"][1:, [2, 8, 15]] >= 1.0) and not s["hits"][0].any()
    assert p.batch > 1 and np.array_equal(p.x[0], plain.x[0]) and np.all(diff[1:] > 1e-6), diff


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PIPELINES))
def test_device_loop_equals_host_glue_with_the_model_on(hip_lib, name):
    """4 ticks, device loop against host glue, both with the stops on and three joints of every robot beginning beyond a stop: x and torques
    (rel_cols, floors 1e-3 / 1).  No new number: each pipeline's own device-against-host tolerance, as
    tests/test_gpu_sim_actuators.py test_device_loop_equals_host_glue_with_the_model_on cites them (kinodynamic 2e-6, centroidal 1e-12, full
    dynamics TOL_FIRST in the first period and TOL_GLUE after it).  Measured, per period: kinodynamic 1.1e-13 2.4e-13 3.0e-10 1.4e-09, centroidal
    4.6e-14 5.2e-14 8.9e-14 4.4e-14, full dynamics 1.4e-14 4.2e-14 7.8e-13 3.9e-12."""
    from tests.test_gpu_fulldynamic_pipeline import TOL_FIRST, TOL_GLUE
    tol = {"kinodynamic": (2e-6, 2e-6), "centroidal": (1e-12, 1e-12), "fulldynamic": (TOL_FIRST, TOL_GLUE)}[name]
    pd, ph = (PIPELINES[name](hip_lib, walk={}) for _ in range(2))
    for p in (pd, ph):
        _arm_beyond(p, free=())
    worst = []
    for t in range(4):
        pd.tick(), ph.tick(host_glue=True)
        worst.append(max(rel_cols(pd.x, ph.x, 1e-3), rel_cols(pd.torques, ph.torques, 1.0)))
    print("%s with joint stops: device loop against host glue, per period: %s" % (name, " ".join("%.1e" % w for w in worst)))
    sd, sh = pd.joint_stop_state(), ph.joint_stop_state()
    assert np.all(sd["steps"] == 40.0) and np.array_equal(sd["steps"], sh["steps"]) and np.all(sd["stop_steps"][:, [2, 8, 15]] > 0.0)
    for t, w in enumerate(worst):
        assert w < tol[0 if t == 0 else 1], (t, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PIPELINES))
def test_robots_are_independent(hip_lib, name):
    """4 robots, robot 0 without limits and the others with three joints beyond a stop: after 5 ticks robot 0 is bit for bit robot 0 of the same
    ensemble without the model, every other robot differs by more than 1e-6."""
    pa, pf = (PIPELINES[name](hip_lib, batch=B, walk={}) for _ in range(2))
    _arm_beyond(pa)
    for _ in range(5):
        pa.tick(), pf.tick()
    assert np.array_equal(pa.x[0], pf.x[0]) and np.array_equal(pa.torques[0], pf.torques[0])
    diff = np.max(np.abs(pa.x[1:] - pf.x[1:]), axis=1)
    print("%s: robots 1 - 3 with against without the model after 5 ticks: %s" % (name, diff))
    assert np.all(diff > 1e-6), diff


def _drive(sim, x, steps, seed):
    """``steps`` calls of simulate_torque with a fresh random command each, every call from the state the one before produced -> the final states"""
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        x = sim.simulate_torque(x, rng.normal(size=(x.shape[0], sim.dims.nu)) * 5.0, 1, DT)
    return x


@pytest.mark.gpu
def test_state_rows_travel(hip_lib):
    """7 steps, read, 5 more; a second handle, freshly armed and given the rows read by set_joint_stops, gives the same states and the same rows over
    those 5 steps bit for bit; a freshly armed handle without them the same states (the stop torque has no memory) and other rows.  Malformed rows
    are refused and the rows in force stay."""
    rb, a, x, _ = _sim(hip_lib, batch=B)
    nu = a.dims.nu
    lo, hi = _beyond(x, rb.model.nq, reach=0.02)
    arm = lambda s: s.joint_stops(ROWS, lo, hi, _effort(rb))
    arm(a)
    x7 = _drive(a, x, 7, 11)
    rows7 = a.read_joint_stops(raw=True)
    s7 = js.unpack(rows7, nu)
    assert np.all(s7["steps"] == 7.0) and np.all(s7["any_steps"][1:] > 0.0) and np.any(s7["pen"] != 0.0) and np.any(s7["peak_pen"] > np.abs(s7["pen"]))
    want = _drive(a, x7, 5, 12)
    b, c = _sim(hip_lib, batch=B)[1], _sim(hip_lib, batch=B)[1]
    arm(b), arm(c)
    b.set_joint_stops(rows7)
    assert np.array_equal(b.read_joint_stops(raw=True), rows7)
    assert np.array_equal(_drive(b, x7, 5, 12), want) and np.array_equal(b.read_joint_stops(raw=True), a.read_joint_stops(raw=True))
    assert np.array_equal(_drive(c, x7, 5, 12), want) and not np.array_equal(c.read_joint_stops(raw=True), a.read_joint_stops(raw=True))
    held = b.read_joint_stops(raw=True)
    pen_col = nu + int(np.argmax(np.abs(held[2, nu:2 * nu])))
    for col, val, match in ((3, np.nan, "finite"), (nu + 1, INF, "finite"), (5 * nu + 1, -1.0, ">= 0"), (4 * nu + 2, -2.0, ">= 0"),
                            (2 * nu + 4, -0.5, ">= 0"), (pen_col, 2.0 * held[2, pen_col + nu] + 1.0, "peak_pen")):
        bad = held.copy()
        bad[2, col] = val
        with pytest.raises(RuntimeError, match=match):
            b.set_joint_stops(bad)
        assert np.array_equal(b.read_joint_stops(raw=True), held)
    with pytest.raises(ValueError, match="shape"):
        b.set_joint_stops(held[:, :-1])


@pytest.mark.gpu
def test_refusals(hip_lib):
    """lo > hi, a NaN limit, a negative k or d, cap <= 0, a reserved entry, a non-positive scale, null tables, a handle of the wrong kind (a
    centroidal plan): each -1 with a message, and the configuration in force unchanged"""
    rb, sim, x, _ = _sim(hip_lib, batch=B)
    nu = sim.dims.nu
    dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=float).ctypes.data_as(C.POINTER(C.c_double))
    lo, hi = _beyond(x, rb.model.nq)
    scale = _effort(rb)
    sim.joint_stops(ROWS, lo, hi, scale)
    sim.simulate_torque(x, np.ones((B, nu)), 1, DT)
    held = sim.read_joint_stops()
    assert held["any_steps"][1:].all()

    def changed(what, b, col, val):
        out = {"rows": ROWS.copy(), "lo": lo.copy(), "hi": hi.copy(), "scale": scale.copy()}
        if what == "scale":
            out[what][col] = val
        else:
            out[what][b, col] = val
        return out

    cases = [(changed("lo", 3, 5, hi[3, 5] + 0.1), "lo > hi"), (changed("hi", 3, 5, np.nan), "NaN"), (changed("lo", 1, 0, np.nan), "NaN"),
             (dict(changed("lo", 2, 4, INF), hi=changed("hi", 2, 4, INF)["hi"]), "inf"), (changed("rows", 3, 0, -1.0), ">= 0"), (changed("rows", 3, 1, -0.5), ">= 0"),
             (changed("rows", 3, 0, INF), "finite"), (changed("rows", 3, 2, 0.0), "cap"), (changed("rows", 3, 2, -1.0), "cap"),
             (changed("rows", 3, 2, np.nan), "cap"), (changed("rows", 3, 6, 1.0), "reserved"), (changed("scale", 0, 7, 0.0), "scale"),
             (changed("scale", 0, 7, -3.0), "scale"), (changed("scale", 0, 7, INF), "scale")]
    for c, match in cases:
        rc = hip_lib.mpc_sim_joint_stops(sim._h, dp(c["rows"]), dp(c["lo"]), dp(c["hi"]), dp(c["scale"]))
        msg = hip_lib.mpc_last_error(sim._h).decode()
        assert rc == -1 and match in msg and ("scale" in match or "row " in msg), (match, rc, msg)
        now = sim.read_joint_stops()
        assert all(np.array_equal(now[k], held[k]) for k in held), match
    assert hip_lib.mpc_sim_joint_stops(sim._h, dp(ROWS), None, dp(hi), None) == -1 and "null" in hip_lib.mpc_last_error(sim._h).decode()
    assert hip_lib.mpc_sim_joint_stops_set(sim._h, None) == -1 and "null" in hip_lib.mpc_last_error(sim._h).decode()
    now = sim.read_joint_stops()
    assert all(np.array_equal(now[k], held[k]) for k in held)
    seized = np.where(np.isfinite(lo), lo, hi)
    assert hip_lib.mpc_sim_joint_stops(sim._h, dp(ROWS), dp(lo), dp(seized), None) == 0   # (lo == hi, seized joints, and no scale: accepted)
    for call, match in ((lambda: sim.joint_stops(ROWS, lo[:, :-1], hi), "shape"), (lambda: sim.joint_stops(ROWS, None, hi), "needed"),
                        (lambda: sim.joint_stops(ROWS, lo, hi, scale[:-1]), "shape")):
        with pytest.raises(ValueError, match=match):
            call()
    plan = centroidal_pipeline(hip_lib, walk={}).mpc.native
    pb, pnu = plan.dims.batch, plan.dims.nu
    good = js.rows({}, pb)
    assert hip_lib.mpc_sim_joint_stops(plan._h, dp(good), dp(np.zeros((pb, pnu))), dp(np.ones((pb, pnu))), None) == -1
    assert "simulator handle" in hip_lib.mpc_last_error(plan._h).decode()
    assert hip_lib.mpc_sim_joint_stops_width(plan._h) == -1 and hip_lib.mpc_sim_joint_stops_width(sim._h) == js.width(nu)
    for call in (lambda: plan.joint_stops(None), lambda: plan.read_joint_stops(), lambda: plan.set_joint_stops(np.zeros((pb, js.width(pnu))))):
        with pytest.raises(RuntimeError, match="simulator handle"):
            call()


@pytest.mark.gpu
def test_bullet_robot_runs_into_a_stop(hip_lib):
    """BulletRobot(joint_stops=...) holding its posture with the left elbow's range ending 0.05 rad short of it: the stop acts and pushes the elbow
    back; without the argument there is no state, and setJointStops arms it later"""
    from mpc_benchmark_amd.bullet_robot import BulletRobot
    rb = _sim_robot()
    m = rb.model
    q0 = rb.x0[:m.nq]
    elbow = 17
    lo, hi = js.limits(m, 1)
    hi[0, elbow] = q0[7 + elbow] - 0.05
    posture = lambda r: 300.0 * (q0[7:] - r.x[7:m.nq]) - 3.0 * r.x[m.nq + 6:]
    robot = BulletRobot([n for n in m.names], None, None, DT, m, library=hip_lib, joint_stops={"lo": lo, "hi": hi})
    plain = BulletRobot([n for n in m.names], None, None, DT, m, library=hip_lib)
    for r in (robot, plain):
        r.initializeJoints(q0)
    assert plain.jointStopState() is None and np.array_equal(robot.jointStopState()["params"][0], js.DEFAULTS)
    for _ in range(20):
        robot.execute(posture(robot)), plain.execute(posture(plain))
    s = robot.jointStopState()
    print("BulletRobot: elbow %.4f with the stop, %.4f without (stop at %.4f), stop_steps %s" % (robot.x[7 + elbow], plain.x[7 + elbow], hi[0, elbow], s["stop_steps"][0, elbow]))
    assert s["steps"][0] == 20.0 and s["hits"][0, elbow] >= 1.0 and s["stop_steps"][0, elbow] > 0.0 and s["tau_stop"][0, elbow] <= 0.0
    assert robot.x[7 + elbow] < plain.x[7 + elbow] - 1e-4
    plain.setJointStops({"k": 5.0, "lo": lo, "hi": hi})
    assert plain.jointStopState()["params"][0, 0] == 5.0
    plain.setJointStops(None)
    assert plain.jointStopState() is None
    robot.close(), plain.close()
