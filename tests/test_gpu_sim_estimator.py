"""The per-robot base-state estimator of the torque-driven simulator on the device (include/mpc_sim_estimator.h: mpc_sim_estimator;
csrc/sim_estimator.h k_sim_estimator) against its numpy definition (mpc_benchmark_amd/state_estimator.py), in mpc_simulate_torque and in the three
device loops; off and identity mean unchanged bits; the controllers of every device loop read the estimate, as the host glue does; robots are
independent of their place in the batch; leg odometry beats a noisy velocity measurement on standing robots; the state rows travel; the checks."""
import ctypes as C

import numpy as np
import pytest

from mpc_benchmark_amd import contact_rule as cr
from mpc_benchmark_amd import sensor_model as sm
from mpc_benchmark_amd import state_estimator as se
from tests._metrics import rel_cols
from tests.test_centroidal_pipeline import centroidal_pipeline
from tests.test_fulldynamic_pipeline import fulldynamic_pipeline
from tests.test_gpu_sim_contacts import _batch_lift, _kino
from tests.test_gpu_sim_push import DT, _sim
from tests.test_gpu_sim_sensors import _drive, _second, _sim_complete

B = 4
W = ((0.0, 0.0), (1.0, 1.0), (0.9, 0.5), (0.0, 1.0))   # (w_p, w_v): identity | pure odometry | a complementary filter | velocity odometry alone
PIPELINES = {"kinodynamic": lambda lib, **kw: _kino(lib, 2, **kw), "centroidal": lambda lib, **kw: centroidal_pipeline(lib, walk={}, **kw),
             "fulldynamic": lambda lib, **kw: fulldynamic_pipeline(lib, walk={}, **kw)}


def _rows(batch):
    w = np.array(W)[np.arange(batch) % len(W)]
    return se.rows({"w_p": w[:, 0], "w_v": w[:, 1]}, batch)


def _noisy(batch):
    """sensor rows: the even robots exact, the odd ones with base noise and a latency of two steps"""
    odd = (np.arange(batch) % 2).astype(float)
    return sm.rows({"delay": 2.0 * odd, "sigma_base_p": 1e-3 * odd, "sigma_base_v": 1e-2 * odd, "seed": 5.0 + np.arange(batch)}, batch)


def _rule(sim, rb):
    """the contact rule on, the ground at the lower initial foothold"""
    sim.contacts(cr.config({}, ground_z=min(float(M.translation[2]) for M in rb.foot_placements)))


def _compare(got, want, xs_scale, nq, label):
    """device rows against mirror rows (both unpacked) -> the four differences; asserts the bounds of the module's kernel-against-mirror tests"""
    assert np.array_equal(got["held"], want["held"]) and np.array_equal(got["count"], want["count"]), label
    e_a = np.max(np.abs(got["anchor"] - want["anchor"]))
    e_p = np.max(np.abs(got["est"][:, 0:3] - want["est"][:, 0:3]))
    e_v = np.max(np.abs(got["est"][:, nq:nq + 3] - want["est"][:, nq:nq + 3]))
    e_s = np.max(np.abs(got["stats"] - want["stats"]))
    s_scale = max(1.0, np.max(np.abs(want["stats"])))
    assert e_a <= 1e-12 and e_p <= 1e-12, (label, e_a, e_p)
    assert e_v <= 1e-12 * xs_scale and e_s <= 1e-12 * s_scale, (label, e_v, xs_scale, e_s, s_scale)
    rest = np.ones(got["est"].shape[1], dtype=bool)
    rest[0:3] = rest[nq:nq + 3] = False
    assert np.array_equal(got["est"][:, rest], want["est"][:, rest]), label       # (everything but the base position and linear velocity: copied)
    return e_a, e_p, e_v / xs_scale, e_s / s_scale


@pytest.mark.gpu
def test_off_and_identity_mean_unchanged_in_simulate_torque(hip_lib):
    """the contact rule on everywhere; a handle that never armed the estimator, one that armed it and turned it off, one armed with identity rows: the
    same bits over 3 steps"""
    rb, a, x, tau = _sim(hip_lib, batch=B)
    handles = [a] + [_sim(hip_lib, batch=B)[1] for _ in range(2)]
    for h in handles:
        _rule(h, rb)
    handles[1].estimator(_rows(B), x)
    handles[1].estimator(None)
    handles[2].estimator(se.IDENTITY, x)
    xs = [x, x, x]
    for k in range(3):
        got = [h.simulate_torque(xi, tau * (1.0 + k), 1, DT, wrenches=True) for h, xi in zip(handles, xs)]
        for g in got[1:]:
            assert np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1]), k
        xs = [g[0] for g in got]
    with pytest.raises(RuntimeError, match="off"):
        handles[1].read_estimator()
    r = handles[2].read_estimator()
    assert np.array_equal(r["x"], xs[0]) and np.array_equal(r["est"], xs[0]) and np.array_equal(r["count"], np.full(B, 4.0))
    assert np.all(r["stats"] == 0.0)                                             # (est = xm = xt: no error)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PIPELINES))
def test_off_and_identity_mean_unchanged_in_the_pipelines(hip_lib, name):
    """the same for 3 ticks of a pipeline with the contact rule: x, torques, forces (full dynamics: wrenches) and x_prev"""
    pa, pb, pc = (PIPELINES[name](hip_lib, contact_rule={}) for _ in range(3))
    pb.set_estimator(_rows(pb.batch))
    pb.set_estimator(None)
    pc.set_estimator(se.IDENTITY)
    for t in range(3):
        pa.tick(), pb.tick(), pc.tick()
        for p in (pb, pc):
            assert np.array_equal(pa.x, p.x) and np.array_equal(pa.torques, p.torques) and np.array_equal(_second(pa), _second(p)), t
            assert np.array_equal(pa.x_prev, p.x_prev), t
    assert np.array_equal(pc.x_est, pc.x) and pb.x_est is pb.x
    with pytest.raises(RuntimeError, match="off"):
        pb.sim.read_estimator()


@pytest.mark.gpu
def test_kernel_equals_mirror(hip_lib):
    """The 70-step scenario of tests/test_gpu_sim_contacts.py test_kernel_equals_the_mirror: 8 robots, each its own right-leg pulse, released and caught.
    Estimator rows identity | (1, 1) | (0.9, 0.5) | (0, 1); the odd robots measure through a sensor model with base noise and a latency of two steps.
    After every step the device rows equal ``state_estimator.estimate`` fed with ``read_sensors()["x"]``, the ``in_contact`` pair of ``read_contacts()``
    and the true state: held and count exactly, the identity robots' estimate their measurement bit for bit, the copied entries bit for bit, anchors and
    base position within 1e-12 (the bound the contact test holds forward-kinematics positions to), the base linear velocity within 1e-12 of the
    largest |state entry| and the statistics within 1e-12 of their largest entry (floors 1).  Every right sole lifts off and touches down at least
    once: each touchdown latches a new anchor.  The mirror's rows are never re-synchronised with the device's.
    Measured over the 70 steps: anchors 4.4e-16, base position 4.4e-16, base velocity 1.0e-16 of the largest entry, statistics 1.2e-15 of theirs;
    the right soles lift off and touch down 1 to 4 times."""
    Bk = 8
    rb, sim, x, _ = _sim(hip_lib, batch=Bk)
    m, fids, nq = rb.model, list(rb.foot_frame_ids), rb.model.nq
    x = np.tile(rb.x0, (Bk, 1))
    _rule(sim, rb)
    rows, srows = _rows(Bk), _noisy(Bk)
    sim.sensors(srows, x)
    sim.estimator(rows, sim.read_sensors()["x"])
    c0 = sim.read_contacts()["in_contact"]
    state = se.reset(rows, sim.read_sensors()["x"], c0, m, fids)
    r0 = sim.read_estimator()
    assert np.array_equal(r0["params"], rows) and np.array_equal(r0["count"], np.ones(Bk)) and np.array_equal(r0["x"], r0["est"])
    lin = np.arange(nq, nq + 3)                                                  # (armed: the measurement, but for the velocity odometry)
    assert np.array_equal(np.delete(r0["x"], lin, axis=1), np.delete(sim.read_sensors()["x"], lin, axis=1))
    assert np.array_equal(r0["x"][0::4], sim.read_sensors()["x"][0::4])
    worst = np.maximum(np.zeros(4), _compare(r0, se.unpack(state, m.nv), 1.0, nq, "armed"))
    amps, spans = 120.0 + 10.0 * np.arange(Bk), 12 + np.arange(Bk) % 4
    q0 = rb.x0[:nq].copy()
    scale = 1.0
    for k in range(70):
        x = sim.simulate_torque(x, _batch_lift(m, q0, x, k, amps, spans), 1, DT)
        xm, con = sim.read_sensors()["x"], sim.read_contacts()
        want = se.estimate(state, rows, xm, con["in_contact"], x, m, fids)
        got = sim.read_estimator()
        scale = max(scale, np.max(np.abs(x)), np.max(np.abs(xm)))
        worst = np.maximum(worst, _compare(got, se.unpack(state, m.nv), scale, nq, "step %d" % k))
        assert np.array_equal(got["x"], got["est"])
        assert np.array_equal(got["x"][0::4], xm[0::4])                          # (the identity rows)
        np.testing.assert_allclose(got["x"], want, rtol=0, atol=1e-12 * scale)
    print("estimator kernel against the mirror over 70 steps: anchors %.1e, base position %.1e, base velocity %.1e of the largest entry, "
          "statistics %.1e; lift-offs %s touchdowns %s" % (*worst, con["liftoffs"][:, 1], con["touchdowns"][:, 1]))
    assert np.all(con["liftoffs"][:, 1] >= 1) and np.all(con["touchdowns"][:, 1] >= 1)
    assert np.max(np.abs(xm[1::2] - x[1::2])) > 1e-4                             # (the sensors act: xm != xt)
    assert np.all(np.max(np.abs(got["x"][1::4] - xm[1::4]), axis=1) > 1e-6)      # (the estimator acts)


@pytest.mark.gpu
def test_kernel_equals_mirror_complete_model(hip_lib):
    """the complete model (B = 2, 5 steps of random torques): nx = 77 is beyond the wavefront, the strided second pass builds xk and stores the
    estimate.  Measured: anchors 2.2e-16, base position 4.4e-16, base velocity 2.4e-18 of the largest entry, statistics 1.4e-16."""
    rb, sim, x, _ = _sim_complete(hip_lib, batch=2)
    m, fids, nq = rb.model, list(rb.foot_frame_ids), rb.model.nq
    assert nq + m.nv == 77
    _rule(sim, rb)
    rows = se.rows({"w_p": [1.0, 0.9], "w_v": [1.0, 0.5]}, 2)
    sim.sensors(_noisy(2), x)
    sim.estimator(rows, sim.read_sensors()["x"])
    state = se.reset(rows, sim.read_sensors()["x"], sim.read_contacts()["in_contact"], m, fids)
    rng = np.random.default_rng(11)
    worst, scale = np.zeros(4), 1.0
    for k in range(5):
        x = sim.simulate_torque(x, rng.normal(size=(2, sim.dims.nu)) * 5.0, 1, DT)
        xm = sim.read_sensors()["x"]
        se.estimate(state, rows, xm, sim.read_contacts()["in_contact"], x, m, fids)
        scale = max(scale, np.max(np.abs(x)), np.max(np.abs(xm)))
        worst = np.maximum(worst, _compare(sim.read_estimator(), se.unpack(state, m.nv), scale, nq, "step %d" % k))
    print("estimator kernel against the mirror, complete model: anchors %.1e, base position %.1e, base velocity %.1e of the largest entry, "
          "statistics %.1e" % tuple(worst))
    assert np.array_equal(sim.read_estimator()["count"], np.full(2, 6.0))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PIPELINES))
def test_device_loops_equal_host_glue(hip_lib, name):
    """Each pipeline with the contact rule, noisy sensors on the odd robot and the estimator (0.9, 1) on, three periods: the device loop equals the
    host glue (which reads ``x_est`` back before each step and applies nothing else) in x, x_prev and torques (rel_cols, floors 1e-3 / 1) at the
    bound tests/test_gpu_sim_sensors.py test_the_hook_is_in_every_loop uses for the same comparison: kinodynamic 2e-6, centroidal 1e-12, full
    dynamics TOL_FIRST = 1e-12.  The torques differ from a run without the estimator by more than 1e-6 of their largest: a loop that still read
    the measurement would give that run's bits.  Measured, per period: kinodynamic 2.0e-13 7.8e-14 9.1e-11, centroidal 2.2e-13 1.5e-13 1.4e-13, full
    dynamics 5.3e-14 1.0e-13 3.7e-13; torques against the run without the estimator 7.1e-2 / 1.4e-1 / 1.2e-1 of their largest."""
    from tests.test_gpu_fulldynamic_pipeline import TOL_FIRST
    tol = {"kinodynamic": 2e-6, "centroidal": 1e-12, "fulldynamic": TOL_FIRST}[name]
    rows = se.rows({"w_p": 0.9, "w_v": 1.0}, 2)
    pd, ph = (PIPELINES[name](hip_lib, contact_rule={}, sensors=_noisy(2), estimator=rows) for _ in range(2))   # (armed by the constructors)
    po = PIPELINES[name](hip_lib, contact_rule={}, sensors=_noisy(2))
    lin = np.arange(pd.nq, pd.nq + 3)                                             # (armed: the measurement, but for the velocity odometry)
    assert np.array_equal(np.delete(pd.x_est, lin, axis=1), np.delete(pd.x_meas, lin, axis=1)) and np.array_equal(pd.x_prev, pd.x_est)
    worst = []
    for t in range(3):
        pd.tick(), ph.tick(host_glue=True), po.tick()
        worst.append(max(rel_cols(pd.x, ph.x, 1e-3), rel_cols(pd.x_prev, ph.x_prev, 1e-3), rel_cols(pd.torques, ph.torques, 1.0)))
    acts = np.max(np.abs(pd.torques - po.torques)) / np.max(np.abs(po.torques))
    print("%s with the estimator: device loop against host glue, per period: %s; torques against the run without the estimator %.2e"
          % (name, " ".join("%.1e" % w for w in worst), acts))
    for p in (pd, ph):
        r = p.sim.read_estimator()
        assert np.array_equal(r["count"], np.full(p.batch, 3 * p.substeps + 1.0)) and np.array_equal(r["x"], p.x_est)
        assert np.array_equal(p.x_meas, p.sim.read_sensors()["x"]) and not np.array_equal(p.x_est[1], p.x_meas[1])
    assert max(worst) <= tol, worst
    assert acts > 1e-6, acts


@pytest.mark.gpu
def test_place_in_the_batch(hip_lib):
    """a batch with its robots permuted gives the permuted rows and estimates bit for bit (5 steps, noisy sensors, every kind of row)"""
    rb, a, x, _ = _sim(hip_lib, batch=B)
    b = _sim(hip_lib, batch=B)[1]
    perm = np.array([2, 0, 3, 1])
    rows, srows = _rows(B), _noisy(B)
    for h, o in ((a, np.arange(B)), (b, perm)):
        _rule(h, rb)
        h.sensors(srows[o], x[o])
        h.estimator(rows[o], h.read_sensors()["x"])
    ea, eb = _drive(a, x, steps=5), _drive(b, x[perm], steps=5, order=perm)
    assert np.array_equal(eb, ea[perm])
    assert np.array_equal(b.read_estimator(raw=True), a.read_estimator(raw=True)[perm])
    assert np.array_equal(b.read_estimator()["x"], a.read_estimator()["x"][perm])
    assert not np.array_equal(a.read_estimator()["x"][1:], a.read_sensors()["x"][1:])


@pytest.mark.gpu
def test_leg_odometry_beats_velocity_noise_on_standing_robots(hip_lib):
    """4 robots standing under a posture PD for 30 steps, base velocity noise sigma_base_v = 0.01 .. 0.1, w_v = 1: for every robot the statistics' sum
    of |v error|^2 of the estimate is below that of the measurement.  No factor fixed in advance.  Measured (estimate / measurement):
    6.3e-07 / 9.4e-03, 6.3e-07 / 3.7e-02, 6.3e-07 / 1.9e-01, 6.3e-07 / 1.0e+00."""
    rb, sim, _, _ = _sim(hip_lib, batch=B)
    m = rb.model
    x = np.tile(rb.x0, (B, 1))
    _rule(sim, rb)
    sim.sensors({"sigma_base_v": [0.01, 0.02, 0.05, 0.1], "seed": [1, 2, 3, 4]}, x)
    sim.estimator({"w_v": 1.0}, sim.read_sensors()["x"])
    q0 = rb.x0[:m.nq].copy()
    for k in range(30):
        x = sim.simulate_torque(x, _batch_lift(m, q0, x, k, np.zeros(B), np.full(B, 15)), 1, DT)
    r, con = sim.read_estimator(), sim.read_contacts()
    print("standing robots, sum of |v error|^2 over 30 steps, estimate / measurement: %s"
          % ", ".join("%.1e / %.1e" % (e, w) for e, w in zip(r["stats"][:, 1], r["stats"][:, 5])))
    assert np.all(con["in_contact"] == 1.0) and np.all(con["liftoffs"] == 0.0) and np.array_equal(r["count"], np.full(B, 31.0))
    assert np.all(r["stats"][:, 5] > 0.0) and np.all(r["stats"][:, 1] < r["stats"][:, 5]), r["stats"]
    assert np.all(r["stats"][:, 0] == 0.0) and np.all(r["stats"][:, 4] == 0.0)     # (w_p = 0 and no position noise: est = xm = xt there)


@pytest.mark.gpu
def test_state_rows_travel(hip_lib):
    """10 steps, read; the estimator goes off and is armed again (rows reset), takes the rows back; a second handle in the same plant state takes them
    too; 10 more steps on a handle that never stopped and on these two give the same bits.  Malformed rows are rejected and the rows in force stay."""
    rb, a, x, _ = _sim(hip_lib, batch=B)
    handles = [a] + [_sim(hip_lib, batch=B)[1] for _ in range(2)]
    rows = _rows(B)
    for h in handles:
        _rule(h, rb)
        h.sensors(sm.IDENTITY, x)
        h.estimator(rows, x)
    x10 = [_drive(h, x, steps=10) for h in handles]
    assert np.array_equal(x10[0], x10[1]) and np.array_equal(x10[0], x10[2])
    rows10 = handles[1].read_estimator(raw=True)
    assert np.array_equal(rows10, handles[0].read_estimator(raw=True)) and rows10.shape == (B, se.width(rb.model.nv))
    handles[1].estimator(None)
    handles[1].estimator(rows, x10[1])
    fresh = handles[1].read_estimator(raw=True)
    assert np.array_equal(se.unpack(fresh, rb.model.nv)["count"], np.ones(B)) and not np.array_equal(fresh, rows10)
    handles[1].set_estimator(rows10)
    assert np.array_equal(handles[1].read_estimator(raw=True), rows10)
    assert np.array_equal(handles[1].read_estimator()["x"], handles[0].read_estimator()["x"])
    handles[2].estimator(rows, x10[2])                                           # (re-armed, and left with the fresh rows)
    x20 = [_drive(h, x10[0], steps=10, seed=12) for h in handles]
    assert np.array_equal(x20[0], x20[1]) and np.array_equal(x20[0], x20[2])      # (the plant does not see the estimator)
    assert np.array_equal(handles[0].read_estimator(raw=True), handles[1].read_estimator(raw=True))
    assert np.array_equal(handles[0].read_estimator()["x"], handles[1].read_estimator()["x"])
    assert not np.array_equal(handles[0].read_estimator(raw=True), handles[2].read_estimator(raw=True))   # (the rows matter)
    held = handles[1].read_estimator(raw=True)
    nx = handles[1].dims.nx
    for col, val, match in ((3, np.nan, "finite"), (nx + 8, np.inf, "finite"), (nx, 0.5, "held"), (nx + 1, 2.0, "held"), (-1, 0.0, "count")):
        bad = held.copy()
        bad[2, col] = val
        with pytest.raises(RuntimeError, match=match):
            handles[1].set_estimator(bad)
        assert np.array_equal(handles[1].read_estimator(raw=True), held)
    with pytest.raises(ValueError, match="shape"):
        handles[1].set_estimator(held[:, :-1])


@pytest.mark.gpu
def test_errors(hip_lib):
    """every rejection of the three entry points: a bad parameter row, x0 NULL or non-finite, the contact rule off, a handle of the wrong kind (a
    centroidal plan), read and set while off: -1 with a message, the configuration in force unchanged; turning the contact rule off drops the
    estimator"""
    rb, sim, x, _ = _sim(hip_lib, batch=B)
    dp = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(C.c_double))
    rows = _rows(B)
    with pytest.raises(RuntimeError, match="off"):
        sim.read_estimator()
    with pytest.raises(RuntimeError, match="off"):
        sim.set_estimator(np.zeros((B, se.width(rb.model.nv))))
    sim.estimator(None)   # (off while off: nothing to do)
    with pytest.raises(RuntimeError, match="contact rule is off on this handle .turn it on with mpc_sim_contacts first."):
        sim.estimator(rows, x)
    with pytest.raises(RuntimeError, match="off"):
        sim.read_estimator()
    _rule(sim, rb)
    sim.estimator(rows, x)
    _drive(sim, x, steps=2)
    held = sim.read_estimator()
    unchanged = lambda: all(np.array_equal(sim.read_estimator()[k], held[k]) for k in held)
    for fields, match in (({"w_p": -0.1}, "[0, 1]"), ({"w_p": 1.5}, "[0, 1]"), ({"w_v": -1e-9}, "[0, 1]"), ({"w_v": 2.0}, "[0, 1]"),
                          ({"w_p": np.nan}, "finite"), ({"w_v": np.inf}, "finite")):
        bad = se.rows({k: [0.0] * (B - 1) + [v] for k, v in fields.items()}, B)   # (the last row is the bad one)
        rc = hip_lib.mpc_sim_estimator(sim._h, dp(bad), dp(x))
        msg = hip_lib.mpc_last_error(sim._h).decode()
        assert rc == -1 and match in msg and "row %d" % (B - 1) in msg, (fields, rc, msg)
        assert unchanged(), fields
        with pytest.raises(RuntimeError):
            sim.estimator(bad, x)
        assert unchanged(), fields
    bad = rows.copy()
    bad[1, 9] = 1.0
    assert hip_lib.mpc_sim_estimator(sim._h, dp(bad), dp(x)) == -1 and "reserved" in hip_lib.mpc_last_error(sim._h).decode() and unchanged()
    assert hip_lib.mpc_sim_estimator(sim._h, dp(rows), None) == -1 and "x0" in hip_lib.mpc_last_error(sim._h).decode() and unchanged()
    xbad = x.copy()
    xbad[1, 5] = np.nan
    assert hip_lib.mpc_sim_estimator(sim._h, dp(rows), dp(xbad)) == -1 and "x0" in hip_lib.mpc_last_error(sim._h).decode() and unchanged()
    with pytest.raises(ValueError, match="x0"):
        sim.estimator(rows)
    zero = sim.read_estimator(raw=True)
    zero[:, -1] = 0.0
    assert hip_lib.mpc_sim_estimator_set(sim._h, dp(zero)) == -1 and "count" in hip_lib.mpc_last_error(sim._h).decode() and unchanged()
    assert hip_lib.mpc_sim_estimator_set(sim._h, None) == -1 and unchanged()
    assert hip_lib.mpc_sim_estimator_read(sim._h, None, None, None) == 0
    plan = centroidal_pipeline(hip_lib, walk={}).mpc.native
    good = se.rows({}, plan.dims.batch)
    assert hip_lib.mpc_sim_estimator(plan._h, dp(good), dp(np.zeros((plan.dims.batch, plan.dims.nx)))) == -1
    assert "simulator handle" in hip_lib.mpc_last_error(plan._h).decode()
    assert hip_lib.mpc_sim_estimator_width(plan._h) == -1 and hip_lib.mpc_sim_estimator_width(sim._h) == se.width(sim.dims.ndx // 2)
    for call in (lambda: plan.estimator(None), lambda: plan.read_estimator(), lambda: plan.set_estimator(np.zeros((plan.dims.batch, 3)))):
        with pytest.raises(RuntimeError, match="simulator handle"):
            call()
    # the contact rule goes: the estimator goes with it, as the terrain does; the rule back on does not bring it back
    sim.contacts(None)
    with pytest.raises(RuntimeError, match="off"):
        sim.read_estimator()
    _rule(sim, rb)
    with pytest.raises(RuntimeError, match="off"):
        sim.read_estimator()
    sim.simulate_torque(x, np.zeros((B, sim.dims.nu)), 1, DT)
