"""Per-robot push schedules of the torque-driven simulator on the device (include/mpc_sim_disturbances.h: mpc_sim_disturbances, _read, _reset,
_width; csrc/sim_disturbances.h k_sim_disturbances and the linked push term of k_eval_multibody<2>): off and idle mean unchanged bits; a schedule
on the base is host re-arming of mpc_sim_set_push bit for bit; the kernel is the numpy mirror (mpc_benchmark_amd/disturbance_model.py); a pushed
link obeys the equation of motion on all nv rows; contact triggers fire on the transitions the contact rule makes; the device loops time a push
inside a period as host glue does; and the conflicts with mpc_sim_set_push and the contact rule are refused."""
import numpy as np
import pytest

from mpc_benchmark_amd import contact_rule as cr
from mpc_benchmark_amd import disturbance_model as dm
from mpc_benchmark_amd.pipeline import PUSH_FORCE, PUSH_THETA, KinodynamicPipeline, build_torque_simulator
from mpc_benchmark_amd.problems.common import Robot
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem
from mpc_benchmark_amd.robot import minipin as pin
from tests._metrics import rel_cols
from tests.test_centroidal_pipeline import centroidal_pipeline

DT = 1e-3
BASE, SHANK, TORSO, ARM = 0, 4, 14, 18   # table joint indices: root_joint, leg_left_4_joint, torso_2_joint, arm_left_4_joint (minipin id - 1)
INT_COLS = [dm.O_STEP, dm.O_ACTING] + list(range(dm.O_OCC, dm.O_IMPULSE)) + [dm.O_PUSHED, dm.O_SHADOWED, dm.O_LINK, dm.O_SEEN, dm.O_SEEN + 1]
REAL_COLS = {"impulse": slice(dm.O_IMPULSE, dm.O_PUSHED), "peak_force": slice(dm.O_PEAK, dm.O_PEAK + 1), "applied": slice(dm.O_APPLIED, dm.O_LINK)}


def _sim(lib, mask=(True, True), batch=2):
    """the default ``Robot()`` simulator of tests/test_gpu_sim_push.py::_sim"""
    rb = Robot()
    sim, tables = build_torque_simulator(lib, rb, batch, DT, 0)
    sim.set_stage(0, *tables[mask])
    rng = np.random.default_rng(7)
    x = np.tile(rb.x0, (batch, 1))
    x[:, rb.model.nq:] += rng.normal(size=(batch, rb.model.nv)) * 0.05
    tau = rng.normal(size=(batch, rb.model.nv - 6)) * 5.0
    return rb, sim, x, tau


def _kinodynamic_pipeline(lib, **kw):
    """tests/test_pipeline.py::_pipeline with keyword arguments passed on"""
    p = KinodynamicPipeline(KinodynamicProblem(horizon=40), batch=2, library=lib, walk={}, perturb=True, sigma_q=0.005, sigma_v=0.01, **kw)
    p.mpc.options.num_threads = 8
    p.mpc.native.set_options(p.mpc.options)
    p.mpc.prepare_schedule(80)
    assert all(s.converged >= 0 for s in p.cold_solve())
    return p


def _assert_rows_equal_the_mirror(got, want, what):
    np.testing.assert_array_equal(got[:, INT_COLS], want[:, INT_COLS], err_msg="%s: integer fields" % what)
    for name, cols in REAL_COLS.items():
        scale = max(np.max(np.abs(want[:, cols])), 1e-300)
        err = np.max(np.abs(got[:, cols] - want[:, cols])) / scale
        assert err <= 1e-12, (what, name, err)


# -- 1. off and idle keep every bit -------------------------------------------------------------------------------------------------------------------
IDLE = [dm.event("step", start=1000, steps=5, link=ARM, force_frame=1, point_frame=1, force=(100.0, 50.0, -20.0), point=(0.1, 0.0, 0.05)),
        dm.event("step", start=2000, steps=5, period=2000, shape=1, force=(0.0, -300.0, 0.0))]


@pytest.mark.gpu
def test_off_and_idle_keep_every_bit(hip_lib):
    """A handle that never armed, one armed then disarmed, one armed with a table whose events never fire in the window: 3 steps of simulate_torque
    with wrenches and 3 ticks of the centroidal pipeline give the same bits."""
    _, a, x, tau = _sim(hip_lib)
    _, b, _, _ = _sim(hip_lib)
    _, c, _, _ = _sim(hip_lib)
    b.disturbances(IDLE)
    b.disturbances(None)
    c.disturbances(IDLE)
    xa = xb = xc = x
    for k in range(3):
        (xa, wa), (xb, wb), (xc, wc) = (s.simulate_torque(xs, tau, 1, DT, wrenches=True) for s, xs in ((a, xa), (b, xb), (c, xc)))
        assert np.array_equal(xa, xb) and np.array_equal(wa, wb), k
        assert np.array_equal(xa, xc) and np.array_equal(wa, wc), k
    st = c.read_disturbances()
    assert np.all(st["step"] == 3) and np.all(st["acting"] == -1) and np.all(st["pushed_steps"] == 0) and np.all(st["applied_now"][:, 6] == -1)
    pa, pb, pc = (centroidal_pipeline(hip_lib, walk={}) for _ in range(3))
    pb.set_disturbances(IDLE)
    pb.set_disturbances(None)
    pc.set_disturbances(IDLE)
    for t in range(3):
        for p in (pa, pb, pc):
            p.tick()
        for p in (pb, pc):
            assert np.array_equal(pa.x, p.x) and np.array_equal(pa.torques, p.torques) and np.array_equal(pa.forces, p.forces), t
    assert np.all(pc.disturbance_state()["step"] == 3 * pc.substeps) and pb.disturbance_state() is None


# -- 2. a schedule is host re-arming, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_schedule_equals_host_rearming_bit_for_bit(hip_lib):
    """Batch 3, base link, world force, world point: robot 0 one event on steps 1 - 2, robot 1 one at step 0 and one on steps 3 - 4, robot 2 none.
    Five single steps on the scheduled handle against five on a handle that gets set_push (width 6) before each step with the mirror's applied rows:
    x, wrenches and the record's push equal at every step."""
    rb, a, x, tau = _sim(hip_lib, batch=3)
    _, b, _, _ = _sim(hip_lib, batch=3)
    table = [[dm.event("step", start=1, steps=2, force=(30.0, -250.0, 40.0), point=(0.0, 0.0, 0.0))],
             [dm.event("step", start=0, steps=1, force=(-120.0, 80.0, -15.0), point=(0.1, 0.2, 0.9)),
              dm.event("step", start=3, steps=2, force=(0.0, 150.0, 60.0), point=(-0.3, 0.1, 1.2))],
             []]
    ev = dm.rows(table, 3)
    a.disturbances(ev)
    a.record(5)
    b.record(5)
    st = dm.reset(3)
    xa = xb = x
    acted = []
    for k in range(5):
        applied = dm.step(ev, st, None, xa, rb.model, DT)
        acted.append(applied[:, 6].tolist())
        b.set_push(applied[:, :6])
        xa, wa = a.simulate_torque(xa, tau, 1, DT, wrenches=True)
        xb, wb = b.simulate_torque(xb, tau, 1, DT, wrenches=True)
        assert np.array_equal(xa, xb) and np.array_equal(wa, wb), k
    assert acted == [[-1, 0, -1], [0, -1, -1], [0, -1, -1], [-1, 0, -1], [-1, 0, -1]]
    ra, rb_ = a.read_record(), b.read_record()
    assert np.array_equal(ra["push"], rb_["push"]) and np.array_equal(ra["x"], rb_["x"]) and np.array_equal(ra["wrenches"], rb_["wrenches"])
    assert np.any(ra["push"][1, 0] != 0.0) and not np.any(ra["push"][:, 2])


@pytest.mark.gpu
def test_a_schedule_on_periods_equals_tick_push_bit_for_bit(hip_lib):
    """A schedule laid on periods 3 - 5 of a centroidal pipeline (``from_push_schedule``) against ``tick(push=...)`` over 8 periods: x, torques and
    forces equal in every bit."""
    fd = PUSH_FORCE["centroidal"]
    ph = centroidal_pipeline(hip_lib, walk={})
    ps = centroidal_pipeline(hip_lib, walk={}, disturbances=dm.from_push_schedule(fd, PUSH_THETA, (3, 6), 10))
    assert ps.substeps == 10 and np.all(ps.disturbance_state()["step"] == 0)
    push = np.tile(np.concatenate([fd * np.array([np.cos(PUSH_THETA), np.sin(PUSH_THETA), 0.0]), np.zeros(3)]), (ph.batch, 1))
    for t in range(8):
        ph.tick(push=push if 3 <= t < 6 else None)
        ps.tick()
        assert np.array_equal(ph.x, ps.x) and np.array_equal(ph.torques, ps.torques) and np.array_equal(ph.forces, ps.forces), t
    st = ps.disturbance_state()
    assert np.all(st["pushed_steps"] == 30) and np.all(st["step"] == 80)
    with pytest.raises(ValueError, match="conflicts with the push schedule"):
        ps.tick(push=push)


# -- 3. the kernel is the mirror ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_kernel_is_the_mirror(hip_lib):
    """Batch 3, 8 steps, a table with link-frame forces at link-frame points on an arm link and on the torso, a half sine, a periodic event and an
    overlap: after every step the integer fields of the state rows are the mirror's exactly; applied, impulse and peak_force within 1e-12 relative
    (the bound at which the device kinematics are held to minipin: test_record, the walk generator)."""
    rb, sim, x, tau = _sim(hip_lib, batch=3)
    table = [[dm.event("step", start=0, steps=3, shape=1, link=ARM, force_frame=1, point_frame=1, force=(40.0, -25.0, 10.0), point=(0.02, -0.01, -0.2)),
              dm.event("step", start=2, steps=4, link=TORSO, force_frame=1, point_frame=1, force=(-60.0, 15.0, 5.0), point=(0.05, 0.1, 0.3))],
             [dm.event("step", start=1, steps=2, period=3, link=TORSO, force_frame=1, point_frame=0, force=(0.0, 80.0, 0.0), point=(0.1, 0.0, 1.1)),
              dm.event("step", start=4, steps=3, shape=1, link=BASE, force=(0.0, 0.0, 50.0))],
             [dm.event("step", start=5, steps=2, link=BASE, force=(100.0, 0.0, 0.0), point_frame=1, point=(0.0, 0.05, 0.1)),
              dm.event("step", start=0, steps=1, period=4, link=SHANK, force_frame=0, point_frame=1, force=(10.0, 20.0, 30.0), point=(0.0, 0.0, -0.1))]]
    ev = dm.rows(table, 3)
    sim.disturbances(ev)
    np.testing.assert_array_equal(sim.read_disturbances(raw=True), dm.reset(3))
    np.testing.assert_array_equal(sim.read_disturbances()["events"], ev)
    st = dm.reset(3)
    for k in range(8):
        applied = dm.step(ev, st, None, x, rb.model, DT)
        x = sim.simulate_torque(x, tau, 1, DT)
        got = sim.read_disturbances()
        _assert_rows_equal_the_mirror(sim.read_disturbances(raw=True), st, "step %d" % k)
        np.testing.assert_array_equal(got["applied_now"][:, 6], applied[:, 6], err_msg="step %d" % k)
        np.testing.assert_array_equal(got["applied_now"][:, :6], got["applied"], err_msg="step %d" % k)
    u = dm.unpack(st)
    assert u["shadowed_steps"][0] == 1 and u["shadowed_steps"][1] >= 1 and np.all(u["pushed_steps"] >= 4)   # (the overlaps happened)
    sim.reset_disturbances()
    np.testing.assert_array_equal(sim.read_disturbances(raw=True), dm.reset(3))
    np.testing.assert_array_equal(sim.read_disturbances()["events"], ev)   # (a reset keeps the table)


# -- 4. a pushed link obeys the equation of motion on all nv rows -----------------------------------------------------------------------------------
def _point_jacobian(m, q, joint, p_world):
    """(3, nv) Jacobian of the world point ``p_world`` carried by joint ``joint`` (minipin id), world axes"""
    data = m.createData()
    pin.forwardKinematics(m, data, q)
    M = data.oMi[joint]
    m2 = m.copy()
    fid = m2.addFrame(pin.Frame("pushed_point", joint, pin.SE3(np.eye(3), np.asarray(M.rotation).T @ (p_world - np.asarray(M.translation)))))
    d2 = m2.createData()
    pin.framesForwardKinematics(m2, d2, q)
    return pin.getFrameJacobian(m2, d2, fid, pin.LOCAL_WORLD_ALIGNED)[:3]


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [(True, True), (True, False)])
def test_a_pushed_link_obeys_the_equation_of_motion(hip_lib, mask):
    """For the base, the torso, an arm link and the shank of the stance leg: one pushed and one free step from the same (x, tau).  With minipin's crba
    and Jacobians  M (dv_push - dv_free) / dt - sum_i Jc_i^T (wr_push - wr_free)_i = J_p^T f,  J_p the Jacobian of the world point on that link,
    within 1e-9 of max |rhs| on all nv rows (the bound of test_pushed_step_obeys_the_momentum_law, the same construction on 6 rows).  For a link
    other than the base the same residual with the base's Jacobian is above 1e-3: the link matters."""
    rb, sim, x, tau = _sim(hip_lib, mask)
    m, nq = rb.model, rb.model.nq
    f = np.array([[30.0, -250.0, 40.0], [-120.0, 80.0, -15.0]])
    p_local = np.array([0.03, -0.02, -0.1])
    x_free, wr_free = sim.simulate_torque(x, tau, 1, DT, wrenches=True)
    for link in (BASE, TORSO, ARM, SHANK):
        sim.disturbances([[dm.event("step", link=link, point_frame=1, force=f[b], point=p_local)] for b in range(2)])
        x_push, wr_push = sim.simulate_torque(x, tau, 1, DT, wrenches=True)
        st = sim.read_disturbances()
        assert np.array_equal(st["link"], [link, link]) and np.array_equal(st["applied"][:, :3], f)
        for b in range(2):
            q = x[b, :nq]
            data = m.createData()
            pin.framesForwardKinematics(m, data, q)
            M = pin.crba(m, data, q)
            lhs = M @ (x_push[b, nq:] - x_free[b, nq:]) / DT
            for i, fid in enumerate(rb.foot_frame_ids):
                lhs -= pin.getFrameJacobian(m, data, fid, pin.LOCAL).T @ (wr_push[b, i] - wr_free[b, i])
            p = st["applied"][b, 3:6]
            Mi = data.oMi[link + 1]
            assert np.max(np.abs(p - (np.asarray(Mi.rotation) @ p_local + np.asarray(Mi.translation)))) < 1e-12
            rhs = _point_jacobian(m, q, link + 1, p).T @ f[b]
            err = np.max(np.abs(lhs - rhs)) / np.max(np.abs(rhs))
            print("equation of motion, contacts %s, link %d, robot %d: %.2e" % (mask, link, b, err))
            assert err < 1e-9, (link, b, err)
            if link != BASE:
                wrong = _point_jacobian(m, q, 1, p).T @ f[b]
                assert np.max(np.abs(lhs - wrong)) / np.max(np.abs(wrong)) > 1e-3, (link, b)
    sim.disturbances(None)
    x_off, wr_off = sim.simulate_torque(x, tau, 1, DT, wrenches=True)
    assert np.array_equal(x_off, x_free) and np.array_equal(wr_off, wr_free)


# -- 5. contact triggers on the device ----------------------------------------------------------------------------------------------------------------
LIFT = 80000.0   # N upward on the base for one step (80 N s).  The legs extend under it, so a sole's normal force falls by only 0.0126 N per N (measured:
                 # 91 N under 3000 N, 28 N under 8000 N; a standing robot carries about 480 N per sole): at 80 kN both soles pull in that step and the
                 # rule releases the left one
LIFTOFF_TABLE = [dm.event("step", start=0, steps=1, force=(0.0, 0.0, LIFT), point_frame=1),
                 dm.event("left_liftoff", start=1, delay=3, steps=2, force=(0.0, -80.0, 0.0), point_frame=1)]


def _contact_sim(lib, batch, cfg):
    rb, sim, x, tau = _sim(lib, batch=batch)
    sim.contacts(cr.config(cfg, ground_z=min(float(M.translation[2]) for M in rb.foot_placements)))
    return rb, sim, x, tau


def _run_against_the_mirror(rb, sim, ev, x, tau, steps, plant=None):
    """``steps`` single steps; before each the mirror is fed with read_contacts(), after each the device rows must be the mirror's.
    ``plant(k, sim)``: called before step k (imposes rows).  -> (acting per step (steps, B), wrenches per step)"""
    st = dm.reset(x.shape[0])
    acting, wrenches = [], []
    for k in range(steps):
        if plant is not None:
            plant(k, sim)
        dm.step(ev, st, sim.read_contacts()["in_contact"], x, rb.model, DT)
        x, wr = sim.simulate_torque(x, tau, 1, DT, wrenches=True)
        _assert_rows_equal_the_mirror(sim.read_disturbances(raw=True), st, "step %d" % k)
        acting.append(st[:, dm.O_ACTING].copy())
        wrenches.append(wr)
    return np.array(acting), np.array(wrenches)


@pytest.mark.gpu
def test_liftoff_trigger_on_the_device(hip_lib):
    """release_steps = 1.  Event 0 pushes the base upward at step 0 so that the left sole's normal force is below -release_force there (it is above
    without the push): the rule releases the sole after step 0, the kernel sees the lift-off at step 1, and event 1 (left lift-off, occurrence 1,
    delay 3, 2 steps) acts on exactly steps 4 and 5.  State rows and applied equal the mirror fed with read_contacts() after each of 7 steps."""
    cfg = {"release_steps": 1}
    rb, free, x, tau = _contact_sim(hip_lib, 2, cfg)
    _, wr_free = free.simulate_torque(x, tau, 1, DT, wrenches=True)
    assert np.all(wr_free[:, 0, 2] > cr.DEFAULTS["release_force"])
    _, sim, _, _ = _contact_sim(hip_lib, 2, cfg)
    ev = dm.rows(LIFTOFF_TABLE, 2)
    sim.disturbances(ev)
    acting, wr = _run_against_the_mirror(rb, sim, ev, x, tau, 7)
    assert np.all(wr[0, :, 0, 2] < -cr.DEFAULTS["release_force"]), wr[0, :, 0, 2]
    assert acting.T.tolist() == [[0, -1, -1, -1, 1, 1, -1]] * 2
    st = sim.read_disturbances()
    assert np.all(st["occurrences"][:, 1] == 1) and np.all(st["fire_step"][:, 1] == 4) and np.all(sim.read_contacts()["liftoffs"][:, 0] == 1)


@pytest.mark.gpu
def test_touchdown_trigger_on_the_device(hip_lib):
    """The in_contact flip planted through set_contacts: the left sole taken out of the rows before step 1 and put back before step 2.  Event 0
    (left touchdown, occurrence 1, delay 1, 2 steps) acts on exactly steps 3 and 4; rows equal the mirror after each of 7 steps."""
    rb, sim, x, tau = _contact_sim(hip_lib, 2, {})
    ev = dm.rows([dm.event("left_touchdown", start=1, delay=1, steps=2, link=TORSO, force=(50.0, 0.0, 0.0), point_frame=1)], 2)
    sim.disturbances(ev)

    def plant(k, s):
        if k in (1, 2):
            rows = s.read_contacts(raw=True)
            rows[:, cr.O_IN] = 0.0 if k == 1 else 1.0
            s.set_contacts(rows)

    acting, _ = _run_against_the_mirror(rb, sim, ev, x, tau, 7, plant)
    assert acting.T.tolist() == [[-1, -1, -1, 0, 0, -1, -1]] * 2
    st = sim.read_disturbances()
    assert np.all(st["occurrences"][:, 0] == 1) and np.all(st["occurrences"][:, 1] == 1) and np.all(st["fire_step"][:, 0] == 3)


@pytest.mark.gpu
def test_liftoff_trigger_inside_one_device_loop_call(hip_lib):
    """The lift-off table through one device-loop call (a period of the centroidal pipeline, 10 steps): the record's push rows show the steps the
    step-by-step run pushed: 0, then 4 and 5."""
    p = centroidal_pipeline(hip_lib, walk={}, contact_rule={"release_steps": 1}, disturbances=LIFTOFF_TABLE)
    p.sim.record(p.substeps)
    p.tick()
    r = p.sim.read_record()
    print("left normal force in step 0 of the device loop:", r["wrenches"][0, :, 0, 2])
    assert np.all(r["wrenches"][0, :, 0, 2] < -cr.DEFAULTS["release_force"])
    pushed = np.any(r["push"][:, :, :3] != 0.0, axis=2)
    assert pushed.T.tolist() == [[k in (0, 4, 5) for k in range(p.substeps)]] * p.batch
    assert np.all(r["push"][0, :, 2] == LIFT) and np.all(r["push"][4:6, :, 1] == -80.0)
    st = p.disturbance_state()
    assert np.all(st["occurrences"][:, 1] >= 1) and np.all(st["fire_step"][:, 1] == 4) and np.all(st["step"] == p.substeps)


# -- 6. sub-period timing in the device loops ---------------------------------------------------------------------------------------------------------
def _sub_period(make, fd, periods=3):
    table = dm.event("step", start=13, steps=4, force=fd * np.array([np.cos(PUSH_THETA), np.sin(PUSH_THETA), 0.0]))
    pd, ph = make(), make()
    for p in (pd, ph):
        p.set_disturbances(table)
    pd.sim.record(periods * pd.substeps)
    worst = 0.0
    for t in range(periods):
        pd.tick()
        ph.tick(host_glue=True)
        worst = max(worst, rel_cols(pd.x, ph.x, 1e-3), rel_cols(pd.torques, ph.torques, 1.0), rel_cols(pd.forces, ph.forces, 1.0))
    pushed = np.any(pd.sim.read_record()["push"] != 0.0, axis=2)
    assert pushed.T.tolist() == [[13 <= k < 17 for k in range(periods * pd.substeps)]] * pd.batch
    return worst


@pytest.mark.gpu
def test_device_loops_time_a_push_inside_a_period_as_host_glue_does(hip_lib):
    """A schedule that starts at step 13 and lasts 4 steps (steps 3 - 6 of period 1): device loop against host glue with the same table at the bounds
    of test_device_loops_equal_host_glue_under_a_push (centroidal 1e-12, kinodynamic 2e-6; a shorter scenario, not a harsher one), and the record
    shows a push in those four steps only."""
    c = _sub_period(lambda: centroidal_pipeline(hip_lib, walk={}), PUSH_FORCE["centroidal"])
    k = _sub_period(lambda: _kinodynamic_pipeline(hip_lib), PUSH_FORCE["kinodynamic"])
    print("device loop vs host glue under a sub-period push: centroidal %.2e, kinodynamic %.2e" % (c, k))
    assert c < 1e-12 and k < 2e-6, (c, k)


# -- 7. conflicts -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_conflicts_are_refused(hip_lib):
    rb, sim, x, tau = _sim(hip_lib)
    sim.disturbances(dm.event())
    with pytest.raises(RuntimeError, match="sim_set_push: the disturbance schedule is on"):
        sim.set_push(np.zeros((2, 6)))
    sim.set_push(None)   # (disarming is always allowed)
    sim.disturbances(None)
    sim.set_push(np.zeros((2, 3)))
    with pytest.raises(RuntimeError, match="sim_disturbances: a push is armed on this handle"):
        sim.disturbances(dm.event())
    sim.set_push(None)
    with pytest.raises(RuntimeError, match="a contact trigger .* needs the contact rule"):
        sim.disturbances(dm.event("left_liftoff", start=1))
    with pytest.raises(RuntimeError, match="disturbance schedule is off"):
        sim.read_disturbances()
    bad = dm.rows(dm.event(), 2)
    bad[1, 0, dm.E_STEPS] = 0.0
    with pytest.raises(RuntimeError, match="robot 1, event 0: steps must be >= 1"):
        sim.disturbances(bad)
    bad[1, 0, dm.E_STEPS], bad[1, 0, dm.E_LINK] = 1.0, rb.model.njoints - 1
    with pytest.raises(RuntimeError, match="robot 1, event 0: link must be in"):
        sim.disturbances(bad)
    with pytest.raises(RuntimeError, match="n_events must be 1 .. 8"):
        sim.disturbances(np.zeros((2, 9, dm.EVENT)))
    # the rule off drops a table that uses it, and keeps one that does not
    sim.contacts(cr.config({}, ground_z=min(float(M.translation[2]) for M in rb.foot_placements)))
    sim.disturbances(dm.event("right_touchdown", start=1))
    assert sim.read_disturbances()["events"][0, 0, 0] == 4
    sim.contacts(None)
    with pytest.raises(RuntimeError, match="disturbance schedule is off"):
        sim.read_disturbances()
    sim.contacts({})
    sim.disturbances(dm.event("step", start=5))
    sim.contacts(None)
    assert sim.read_disturbances()["events"][0, 0, 0] == 1
    a = sim.simulate_torque(x, tau, 1, DT)
    sim.disturbances(None)
    assert np.array_equal(a, sim.simulate_torque(x, tau, 1, DT))
