"""The unilateral contact rule of the torque-driven simulator on the device (include/mpc_sim_contacts.h; csrc/sim_contacts.h k_sim_contacts and the rows
read by the simulation form of the stage kernel): the kernel against the numpy mirror (mpc_benchmark_amd/contact_rule.py), mixed contact sets in one
launch against the per-stage path, the device rule of BulletRobot against its host rule, nothing changed with the rule off, the three device loops
against their host glue with the rule on, walks with the rule, and the error paths."""
import types

import numpy as np
import pytest

from mpc_benchmark_amd import contact_rule as cr
from mpc_benchmark_amd.pipeline import KinodynamicPipeline, build_torque_simulator
from mpc_benchmark_amd.problems.common import Robot
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem
from mpc_benchmark_amd.robot import minipin as pin
from tests._metrics import rel_cols
from tests.test_centroidal_pipeline import centroidal_pipeline
from tests.test_fulldynamic_pipeline import fulldynamic_pipeline
from tests.test_pipeline import _pipeline as kinodynamic_pipeline
from tests.test_sim_contacts import lift_torques

DT = 1e-3
FLAGS = ("in_contact", "lifted", "pulling", "touchdowns", "liftoffs", "last_touchdown", "last_liftoff", "steps")


def _sim(lib, batch, robot=None):
    rb = robot or Robot()
    sim, tables = build_torque_simulator(lib, rb, batch, DT, 0)
    sim.set_stage(0, *tables[(True, True)])
    return rb, sim, tables


def _soles(m, fids, x):
    """sole placements of every robot's state: R (B, 2, 3, 3), p (B, 2, 3) (minipin)"""
    data = m.createData()
    R, p = np.zeros((x.shape[0], 2, 3, 3)), np.zeros((x.shape[0], 2, 3))
    for b in range(x.shape[0]):
        pin.framesForwardKinematics(m, data, x[b, :m.nq])
        for i, f in enumerate(fids):
            R[b, i], p[b, i] = data.oMf[f].rotation, data.oMf[f].translation
    return R, p


def _batch_lift(m, q0, x, k, amps, spans):
    """lift_torques of every robot, robot b with its own pulse"""
    return np.stack([lift_torques(types.SimpleNamespace(model=m, x=x[b]), q0, k, amp=amps[b], span=spans[b]) for b in range(x.shape[0])])


@pytest.mark.gpu
def test_kernel_equals_the_mirror(hip_lib):
    """8 robots, each its own right-leg pulse, 70 one-step calls of mpc_simulate_torque: after every step the device rows equal the mirror fed with the
    step's wrenches and the minipin sole placements (flags and counters exactly, anchors within 1e-12); every robot is released and caught."""
    B = 8
    rb, sim, _ = _sim(hip_lib, B)
    m, fids = rb.model, list(rb.foot_frame_ids)
    gz = min(float(M.translation[2]) for M in rb.foot_placements)
    cfg = cr.config({}, ground_z=gz)
    sim.contacts(cfg)
    rows = sim.read_contacts(raw=True)
    want = cr.reset_rows(np.array([M.rotation for M in rb.foot_placements]), np.array([M.translation for M in rb.foot_placements]))
    np.testing.assert_array_equal(rows, np.broadcast_to(want, rows.shape))
    amps, spans = 120.0 + 10.0 * np.arange(B), 12 + np.arange(B) % 4
    q0 = rb.x0[:m.nq].copy()
    x = np.tile(rb.x0, (B, 1))
    want = rows
    for k in range(70):
        x, wr = sim.simulate_torque(x, _batch_lift(m, q0, x, k, amps, spans), 1, DT, wrenches=True)
        R, p = _soles(m, fids, x)
        want = cr.step(want, p[..., 2], wr[:, :, 2], R, p, cfg)
        got, w = cr.unpack(sim.read_contacts(raw=True)), cr.unpack(want)
        for f in FLAGS:
            np.testing.assert_array_equal(got[f], w[f], err_msg="step %d: %s" % (k, f))
        np.testing.assert_allclose(got["anchor_R"], w["anchor_R"], rtol=0, atol=1e-12, err_msg="step %d" % k)
        np.testing.assert_allclose(got["anchor_p"], w["anchor_p"], rtol=0, atol=1e-12, err_msg="step %d" % k)
        np.testing.assert_allclose(got["z_prev"], w["z_prev"], rtol=0, atol=1e-12, err_msg="step %d" % k)
    print("lift-offs %s touchdowns %s (right sole: steps %s -> %s)" % (got["liftoffs"][:, 1], got["touchdowns"][:, 1], got["last_liftoff"][:, 1],
                                                                       got["last_touchdown"][:, 1]))
    assert np.all(got["liftoffs"][:, 1] >= 1) and np.all(got["touchdowns"][:, 1] >= 1)


def _yawed(M, dx, dy, yaw):
    Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
    return pin.SE3(Rz @ np.asarray(M.rotation), np.asarray(M.translation) + np.array([dx, dy, 0.0]))


@pytest.mark.gpu
def test_mixed_contact_sets_in_one_launch_equal_the_per_stage_path(hip_lib):
    """One launch with robots in (both), (left), (right) and (both, the right anchor moved by 2 cm and yawed by 0.1 rad) against separate handles given
    the matching stage, and a model whose contact placement holds that anchor: states and wrenches within 1e-12, two sub-steps."""
    B = 4
    rb, sim, tables = _sim(hip_lib, B)
    m = rb.model
    rng = np.random.default_rng(11)
    x = np.tile(rb.x0, (B, 1))
    x[:, m.nq:] += rng.normal(size=(B, m.nv)) * 0.05
    tau = rng.normal(size=(B, m.nv - 6)) * 10.0
    moved = _yawed(rb.foot_placements[1], 0.02, -0.01, 0.1)
    sim.contacts({"ground_z": 0.0})
    rows = sim.read_contacts(raw=True)
    rows[1, cr.O_IN + 1] = 0.0
    rows[2, cr.O_IN] = 0.0
    rows[3, cr.O_ANCHOR + 12:cr.O_ANCHOR + 24] = np.concatenate([np.asarray(moved.rotation).reshape(-1), moved.translation])
    sim.set_contacts(rows)
    got_x, got_w = sim.simulate_torque(x, tau, 2, DT, wrenches=True)
    shifted = types.SimpleNamespace(model=m, foot_frame_ids=rb.foot_frame_ids, foot_joint_ids=rb.foot_joint_ids, foot_placements=[rb.foot_placements[0], moved])
    for b, (robot, mask) in enumerate(((rb, (True, True)), (rb, (True, False)), (rb, (False, True)), (shifted, (True, True)))):
        ref, rt = build_torque_simulator(hip_lib, robot, B, DT, 0)
        ref.set_stage(0, *rt[mask])
        want_x, want_w = ref.simulate_torque(x, tau, 2, DT, wrenches=True)
        ex, ew = np.max(np.abs(got_x[b] - want_x[b])), np.max(np.abs(got_w[b] - want_w[b]))
        print("robot %d %s: states %.1e wrenches %.1e" % (b, mask, ex, ew))
        assert ex <= 1e-12 and ew <= 1e-12 * max(1.0, np.max(np.abs(want_w[b]))), (b, ex, ew)
        for i in range(2):
            if not mask[i]:
                assert np.all(got_w[b, i] == 0.0)
        ref.close()


@pytest.mark.gpu
def test_device_rule_equals_the_host_rule(hip_lib):
    """BulletRobot(device_contacts=True) against BulletRobot() under the lift sequence (a release and a catch): the same in_contact after every step,
    states within 1e-9."""
    from mpc_benchmark_amd.bullet_robot import BulletRobot
    rb = Robot()
    m = rb.model
    host = BulletRobot([n for n in m.names], None, None, 1e-3, m, library=hip_lib)
    dev = BulletRobot([n for n in m.names], None, None, 1e-3, m, library=hip_lib, device_contacts=True)
    for r in (host, dev):
        r.initializeJoints(rb.x0[:m.nq])
    q0 = host.x[:host.model.nq].copy()
    flags, worst = [], 0.0
    for k in range(70):
        tau = lift_torques(host, q0, k)
        host.execute(tau)
        dev.execute(tau)
        assert dev.in_contact == host.in_contact, (k, dev.in_contact, host.in_contact)
        worst = max(worst, np.max(np.abs(dev.x - host.x)))
        assert worst <= 1e-9, (k, worst)
        flags.append(tuple(host.in_contact))
    print("device rule vs host rule over 70 steps: states %.1e; contact sets %s" % (worst, sorted(set(flags))))
    assert (True, False) in flags and flags[-1] == (True, True)
    r = dev._native.read_contacts()
    assert r["liftoffs"][0].tolist() == [0.0, 1.0] and r["touchdowns"][0].tolist() == [0.0, 1.0]
    np.testing.assert_allclose(r["anchor_p"][0, 1], host._contact_pose[1].translation, atol=1e-12)


@pytest.mark.gpu
def test_off_means_unchanged(hip_lib):
    """Rule never on, or on and then off: simulate_torque and the three device loops (with record and metrics) give the same bits as fresh handles."""
    rb, a, _ = _sim(hip_lib, 2)
    _, b, _ = _sim(hip_lib, 2)
    rng = np.random.default_rng(5)
    x = np.tile(rb.x0, (2, 1))
    tau = rng.normal(size=(2, rb.model.nv - 6)) * 5.0
    want = a.simulate_torque(x, tau, 1, DT, wrenches=True)
    b.contacts({})
    b.contacts(None)
    got = b.simulate_torque(x, tau, 1, DT, wrenches=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for make, out in ((lambda: kinodynamic_pipeline(hip_lib, walk={}), "forces"), (lambda: centroidal_pipeline(hip_lib, walk={}), "forces"),
                      (lambda: fulldynamic_pipeline(hip_lib, walk={}), "wrenches")):
        pa, pb = make(), make()
        pb.sim.contacts({})
        pb.sim.contacts(None)
        for p in (pa, pb):
            p.sim.record(3 * p.substeps)
            p.sim.metrics({})
        for t in range(3):
            pa.tick()
            pb.tick()
            assert np.array_equal(pa.x, pb.x) and np.array_equal(pa.torques, pb.torques) and np.array_equal(getattr(pa, out), getattr(pb, out)), t
        ra, rb_ = pa.sim.read_record(), pb.sim.read_record()
        for k in ra:
            assert np.array_equal(ra[k], rb_[k]), k
        ma, mb = pa.sim.read_metrics(), pb.sim.read_metrics()
        for k in ma:
            np.testing.assert_array_equal(ma[k], mb[k], err_msg=k)


def _kino(lib, batch, horizon=40, periods=80, **kw):
    p = KinodynamicPipeline(KinodynamicProblem(horizon=horizon), batch=batch, library=lib, walk={}, perturb=True, sigma_q=0.005, sigma_v=0.01, **kw)
    p.mpc.options.num_threads = 8
    p.mpc.native.set_options(p.mpc.options)
    p.mpc.prepare_schedule(periods)
    assert all(s.converged >= 0 for s in p.cold_solve())
    return p


@pytest.mark.gpu
def test_device_loops_equal_host_glue_with_the_rule(hip_lib):
    """The three pipelines with the rule on, batch 8, 6 periods: device loop against host glue (one mpc_simulate_torque per step, the rule after each)
    within the tolerances of the existing loop tests (kinodynamic and centroidal 1e-9, full dynamics 1e-12 / 1e-10), the same rows of the rule."""
    B, rule = 8, {}
    cases = ((lambda: _kino(hip_lib, B, contact_rule=rule), "forces", 1e-9, 1e-9),
             (lambda: centroidal_pipeline(hip_lib, batch=B, walk={}, contact_rule=rule), "forces", 1e-9, 1e-9),
             (lambda: fulldynamic_pipeline(hip_lib, batch=B, walk={}, contact_rule=rule), "wrenches", 1e-12, 1e-10))
    for make, out, tol0, tol in cases:
        pl, ph = make(), make()
        worst = []
        for t in range(6):
            pl.tick()
            ph.tick(host_glue=True)
            ol, oh = getattr(pl, out).reshape(B, -1), getattr(ph, out).reshape(B, -1)
            e = max(rel_cols(pl.x, ph.x, 1e-3), rel_cols(pl.x_prev, ph.x_prev, 1e-3), rel_cols(pl.torques, ph.torques, 1.0), rel_cols(ol, oh, 1.0))
            assert e <= (tol0 if t == 0 else tol), (type(pl).__name__, t, e)
            worst.append(e)
            rl, rh = cr.unpack(pl.sim.read_contacts(raw=True)), cr.unpack(ph.sim.read_contacts(raw=True))
            for f in FLAGS:
                np.testing.assert_array_equal(rl[f], rh[f], err_msg="%s period %d %s" % (type(pl).__name__, t, f))
        print("%s with the rule: device loop vs host glue %s; steps %s" % (type(pl).__name__, " ".join("%.1e" % w for w in worst), rl["steps"][0]))


WALK = {  # pipeline: (horizon, periods through the first landing, scheduled take-off period, scheduled landing period)
    "kinodynamic": (40, 150, 59, 139),
    "centroidal": (100, 210, 120, 200),   # (at N = 40 the centroidal robots fall at the landing with the rule: DESIGN.md, profiles/sim_contacts.txt)
    "fulldynamic": (40, 160, 69, 149),
}


def walk_with_the_rule(lib, name, batch):
    """the pipeline with the rule through the first take-off (right foot) and landing -> (rows of the rule, metrics, pipeline, periods)"""
    N, T, _, _ = WALK[name]
    kw = dict(contact_rule={})
    if name == "kinodynamic":
        p = _kino(lib, batch, horizon=N, periods=T + 16, **kw)
    elif name == "centroidal":
        p = centroidal_pipeline(lib, batch=batch, horizon=N, walk={}, **kw)
        p.mpc.prepare_schedule(T + 16)
    else:
        p = fulldynamic_pipeline(lib, batch=batch, horizon=N, walk={}, **kw)
        p.mpc.prepare_schedule(T + 16)
    p.sim.metrics({})
    for _ in range(T):
        p.tick()
    return p.sim.read_contacts(), p.sim.read_metrics(), p, T


def _walk_verdict(name, r, met, p):
    """-> list of failed expectations (empty: the swing foot lifted off and touched down near the schedule, the stance foot stayed, nobody fell)"""
    _, T, t_off, t_on = WALK[name]
    S = p.substeps
    bad = []
    print("%s with the rule, %d robots: right lift-offs %s touchdowns %s ; first lift-off step %s (scheduled %d) ; last touchdown step %s (scheduled %d) ; "
          "left lift-offs %s ; fall_step %s" % (name, p.batch, r["liftoffs"][:, 1], r["touchdowns"][:, 1], r["last_liftoff"][:, 1], S * t_off,
                                                r["last_touchdown"][:, 1], S * t_on, r["liftoffs"][:, 0], met["fall_step"]))
    if not np.all(r["liftoffs"][:, 0] == 0):
        bad.append("the stance (left) foot left the ground")
    if not (np.all(r["liftoffs"][:, 1] >= 1) and np.all(r["touchdowns"][:, 1] >= 1) and np.all(r["in_contact"][:, 1] == 1)):
        bad.append("the swing (right) foot did not lift off and touch down again")
    # windows (steps): the lift-off within 8 periods after the scheduled take-off (the QP unloads the sole, the rule waits release_steps); the last
    # touchdown from 20 periods before to 2 after the scheduled landing (the swing foot is back within the tolerance before its phase ends).  A second
    # lift-off of the swing foot (chatter) is printed, not asserted away: profiles/sim_contacts.txt explains the one seen
    lo, td = r["last_liftoff"][:, 1], r["last_touchdown"][:, 1]
    if not np.all((lo >= S * t_off) & (lo <= S * (t_off + 8))):
        bad.append("a lift-off outside [%d, %d]" % (S * t_off, S * (t_off + 8)))
    if not np.all((td >= S * (t_on - 20)) & (td <= S * (t_on + 2))):
        bad.append("a last touchdown outside [%d, %d]" % (S * (t_on - 20), S * (t_on + 2)))
    if not np.all(met["fall_step"] == -1):
        bad.append("a robot fell")
    return bad


@pytest.mark.gpu
def test_kinodynamic_walk_with_the_rule(hip_lib):
    """8 robots of the kinodynamic pipeline (N = 40) with the rule through the first take-off of the right foot (period 59) and its landing (period
    139): the swing foot lifts off within 8 periods after the scheduled take-off and touches down last from 20 periods before to 2 periods after
    the scheduled landing (measured: 0.4 - 3.4 periods after the take-off, 3.8 - 16.3 periods before the landing, one lift-off and one touchdown per
    robot); the stance foot never leaves the ground; nobody falls."""
    r, met, p, _ = walk_with_the_rule(hip_lib, "kinodynamic", 8)
    assert not _walk_verdict("kinodynamic", r, met, p)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["centroidal", "fulldynamic"])
def test_other_walks_with_the_rule(hip_lib, name):
    """the same walk for the centroidal pipeline at the script's horizon N = 100 (take-off 120, landing 200) and the full-dynamics pipeline at N = 40
    (take-off 69, landing 149)"""
    r, met, p, _ = walk_with_the_rule(hip_lib, name, 8)
    assert not _walk_verdict(name, r, met, p)


@pytest.mark.gpu
def test_errors(hip_lib):
    rb, sim, tables = _sim(hip_lib, 2)
    m = rb.model
    x, tau = np.tile(rb.x0, (2, 1)), np.zeros((2, m.nv - 6))
    assert hip_lib.mpc_sim_contacts_width(sim._h) == cr.WIDTH == 41
    with pytest.raises(RuntimeError, match="rule is off"):
        sim.read_contacts()
    with pytest.raises(RuntimeError, match="rule is off"):
        sim.set_contacts(np.zeros((2, cr.WIDTH)))
    with pytest.raises(RuntimeError, match="release_steps"):
        sim.contacts({"release_steps": 0})
    for bad in ({"ground_z": np.nan}, {"ground_tol": np.inf}, {"release_force": -np.inf}):
        with pytest.raises((RuntimeError, ValueError), match="finite"):
            sim.contacts(bad)
    with pytest.raises(RuntimeError, match=">= 0"):
        sim.contacts({"ground_tol": -1e-3})
    sim.contacts({})
    # a stage 0 without both contacts: every stepping call refuses it
    sim.set_stage(0, *tables[(True, False)])
    with pytest.raises(RuntimeError, match="double-support"):
        sim.simulate_torque(x, tau, 1, DT)
    sim.set_stage(0, *tables[(True, True)])
    sim.simulate_torque(x, tau, 1, DT)
    assert np.all(sim.read_contacts()["steps"] == 1)
    p = fulldynamic_pipeline(hip_lib, walk={})
    p.sim.contacts({})
    p._set_sim_contacts((True, False))   # (without contact_rule the pipeline still sets the schedule's stage: here a single-support stage 0)
    with pytest.raises(RuntimeError, match="double-support"):
        p.low_level_loop(p.contact_state())
    # rows: none in contact, non-finite, a flag other than 0 / 1, an anchor that is not a rotation
    rows = sim.read_contacts(raw=True)
    for edit, what in ((lambda r: r.__setitem__((1, slice(0, 2)), 0.0), "no sole in contact"), (lambda r: r.__setitem__((0, 6), np.nan), "non-finite"),
                       (lambda r: r.__setitem__((0, 2), 0.5), "0 or 1"), (lambda r: r.__setitem__((1, 8), 2.0), "not a rotation"),
                       (lambda r: r.__setitem__((0, slice(20, 29)), np.diag([1.0, 1.0, -1.0]).reshape(-1)), "not a rotation")):
        bad = rows.copy()
        edit(bad)
        with pytest.raises(RuntimeError, match=what):
            sim.set_contacts(bad)
    np.testing.assert_array_equal(sim.read_contacts(raw=True), rows)   # (a refused row changes nothing)
    sim.set_contacts(rows)
    # the rule on a handle that is not a simulator (a centroidal plan)
    from mpc_benchmark_amd.ensemble import EnsembleMPC
    from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
    plan = EnsembleMPC(CentroidalProblem(horizon=10), batch=2, library=hip_lib).native
    with pytest.raises(RuntimeError, match="simulator handle"):
        plan.contacts({})
    with pytest.raises(RuntimeError, match="simulator handle"):
        plan.read_contacts()
    sim.contacts(None)
    with pytest.raises(RuntimeError, match="rule is off"):
        sim.read_contacts()
