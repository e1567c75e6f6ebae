"""The box terrain under the contact rule of the torque-driven simulator on the device (include/mpc_sim_terrain.h; csrc/sim_terrain.h, the terrain
part of k_sim_contacts and k_sim_metrics): the device height function against the numpy definition bit for bit, the kernel against the mirror with
every robot on its own box, nothing changed without a terrain, the device rule of BulletRobot against its host rule on stairs, the three device
loops against their host glue over a catch on a box, the metrics' fall verdict above the ground against the mirror, a walk onto the first step of a
staircase (and the same walk without the staircase, which finds no ground up there), and the error paths."""
import numpy as np
import pytest

from mpc_benchmark_amd import contact_rule as cr
from mpc_benchmark_amd import locomotion_metrics as lm
from mpc_benchmark_amd.pipeline import KinodynamicPipeline, stairs_under_walk
from mpc_benchmark_amd.problems.common import Robot
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem
from tests._metrics import rel_cols
from tests.test_centroidal_pipeline import centroidal_pipeline
from tests.test_fulldynamic_pipeline import fulldynamic_pipeline
from tests.test_gpu_sim_contacts import DT, FLAGS, _batch_lift, _sim, _soles
from tests.test_gpu_sim_metrics import _agree, _cat, _near_zero_margins
from tests.test_sim_contacts import lift_torques
from tests.test_sim_terrain import LIFT_STEPS, LIFTS, box_at_the_right_sole, boxes_can_go_in, lift_boxes


def _random_boxes(rng, B, n):
    lo = rng.uniform(-1.0, 0.6, size=(B, n, 2))
    return np.stack([lo[..., 0], lo[..., 0] + rng.uniform(0.05, 0.9, (B, n)), lo[..., 1], lo[..., 1] + rng.uniform(0.05, 0.9, (B, n)),
                     rng.uniform(-0.05, 0.4, (B, n))], axis=-1)


def _points(rng, boxes, n_random):
    """per robot: random points, and points exactly on the edges and corners of its boxes (closed intervals) and one ulp outside them"""
    B = boxes.shape[0]
    pts = [rng.uniform(-1.2, 1.7, size=(B, n_random, 2))]
    for k in range(boxes.shape[1]):
        bx = boxes[:, k]
        ym, xm = 0.5 * (bx[:, 2] + bx[:, 3]), 0.5 * (bx[:, 0] + bx[:, 1])
        for x, y in ((bx[:, 0], ym), (bx[:, 1], ym), (xm, bx[:, 2]), (xm, bx[:, 3]), (bx[:, 0], bx[:, 2]), (bx[:, 1], bx[:, 3]), (bx[:, 0], bx[:, 3]),
                     (bx[:, 1], bx[:, 2]), (np.nextafter(bx[:, 0], -np.inf), ym), (np.nextafter(bx[:, 1], np.inf), ym), (xm, np.nextafter(bx[:, 3], np.inf))):
            pts.append(np.stack([x, y], axis=-1)[:, None])
    return np.concatenate(pts, axis=1)


@pytest.mark.gpu
def test_device_height_equals_the_definition_bit_for_bit(hip_lib):
    """mpc_sim_terrain_height against contact_rule.terrain_height: 8 robots, 16 random overlapping boxes each (tops from below the ground to 0.4 m), 200
    random points per robot plus 11 points per box on its edges, corners and one ulp outside; per-robot and shared form, a point count that is not a
    multiple of the four points a wavefront takes at a time, zero boxes, no terrain, and a ground above some of the tops."""
    B = 8
    rb, sim, _ = _sim(hip_lib, B)
    rng = np.random.default_rng(17)
    boxes = _random_boxes(rng, B, 16)
    pts = _points(rng, boxes, 200)
    assert pts.shape == (B, 200 + 11 * 16, 2)
    for gz in (0.0, 0.11):
        sim.contacts({"ground_z": gz})
        np.testing.assert_array_equal(sim.terrain_height(pts), np.full(pts.shape[:2], gz))          # no terrain: the plane
        sim.terrain(boxes)
        got, want = sim.terrain_height(pts), cr.terrain_height(boxes, pts, gz)
        assert got.tobytes() == want.tobytes(), np.max(np.abs(got - want))
        assert len(np.unique(got)) > 40 and np.mean(got > gz) > 0.2                                 # (the boxes are hit)
        np.testing.assert_array_equal(sim.read_terrain(), boxes)
        assert sim.terrain_height(pts[:, :37]).tobytes() == want[:, :37].tobytes()
        assert sim.terrain_height(pts[:, :1]).tobytes() == want[:, :1].tobytes()
        assert sim.terrain_height(pts[:, :0]).shape == (B, 0)
        for n in (1, 3, 5, 16):                                                                      # shared: robot 3's first n boxes for everybody
            sim.terrain(boxes[3, :n])
            assert sim.terrain_height(pts).tobytes() == cr.terrain_height(boxes[3, :n], pts, gz).tobytes(), n
            assert sim.read_terrain().shape == (n, 5)
        for zero in (np.zeros((0, 5)), np.zeros((B, 0, 5))):
            sim.terrain(zero)
            np.testing.assert_array_equal(sim.terrain_height(pts), np.full(pts.shape[:2], gz))
            assert sim.read_terrain().shape == zero.shape
        sim.terrain(boxes)
        sim.terrain(None)
        np.testing.assert_array_equal(sim.terrain_height(pts), np.full(pts.shape[:2], gz))
        assert sim.read_terrain().shape == (0, 5)
    sim.close()


def _run_lifts(sim, rb, cfg, on_install=None):
    """``LIFTS``: 8 robots, each its own right-leg pulse and its own box, installed by ONE per-robot terrain() call once every sole that has a box under
    it is above that box by 2 ground_tol.  One-step calls of mpc_simulate_torque; after every step the device rows against the mirror.
    ``on_install(x)``: called right after the terrain() call with the states at that moment.
    -> (rows, first catches [(step, anchor z)], boxes, step of the installation, the rows each step was integrated with)"""
    B = len(LIFTS)
    m, fids = rb.model, list(rb.foot_frame_ids)
    boxes = lift_boxes(np.asarray(rb.foot_placements[1].translation, dtype=float), cfg["ground_z"])
    amps, spans = np.array([a for a, _, _, _ in LIFTS]), np.array([s for _, s, _, _ in LIFTS])
    q0 = rb.x0[:m.nq].copy()
    x = np.tile(rb.x0, (B, 1))
    want = raw = sim.read_contacts(raw=True)
    terrain, installed, first, before = None, None, [None] * B, []
    for k in range(LIFT_STEPS):
        before.append(raw)
        prev_in = raw[:, cr.O_IN + 1].copy()
        x, wr = sim.simulate_torque(x, _batch_lift(m, q0, x, k, amps, spans), 1, DT, wrenches=True)
        R, p = _soles(m, fids, x)
        want = cr.step(want, p[..., 2], wr[:, :, 2], R, p, cfg, terrain=terrain)
        raw = sim.read_contacts(raw=True)
        got, w = cr.unpack(raw), cr.unpack(want)
        for f in FLAGS:
            np.testing.assert_array_equal(got[f], w[f], err_msg="step %d: %s" % (k, f))
        np.testing.assert_allclose(got["anchor_R"], w["anchor_R"], rtol=0, atol=1e-12, err_msg="step %d" % k)
        np.testing.assert_allclose(got["anchor_p"], w["anchor_p"], rtol=0, atol=1e-12, err_msg="step %d" % k)
        np.testing.assert_allclose(got["z_prev"], w["z_prev"], rtol=0, atol=1e-12, err_msg="step %d" % k)
        for b in range(B):
            if prev_in[b] == 0.0 and got["in_contact"][b, 1] == 1.0:
                z = got["anchor_p"][b, 1, 2]
                # a catch lands on the height function, exactly: the box top where the origin of the sole is over the box, the plane elsewhere
                assert z == cr.terrain_height(boxes[b] if terrain is not None else np.zeros((0, 5)), p[b, 1, :2], cfg["ground_z"]), (k, b)
                if first[b] is None:
                    first[b] = (k, z)
        if installed is None and boxes_can_go_in(got["in_contact"][:, 1], p[:, 1, 2], boxes, cfg["ground_tol"]):
            sim.terrain(boxes)
            np.testing.assert_array_equal(sim.read_contacts(raw=True), raw)   # (setting a terrain does not touch the rows)
            terrain, installed = boxes, k
            if on_install is not None:
                on_install(x.copy())
    return got, first, boxes, installed, np.array(before)


@pytest.mark.gpu
def test_kernel_equals_the_mirror_over_boxes(hip_lib):
    """The kernel against the mirror with a terrain, as test_kernel_equals_the_mirror does without: 8 robots, every robot its own pulse and its own box
    (tests/test_sim_terrain.py ``LIFTS``: five boxes under the sole with heights of 5 - 30 mm, each at least 2 mm under apex - 2 ground_tol of its pulse;
    two beside the foot; one under the toe only).  After every step flags and counters exactly, anchors within 1e-12, and the anchor z of every catch
    equal to the height function under the sole's origin.  Every robot is released and caught and stands at the end; the first catch of the five
    is on its box top (==), of the other three on the plane (==).  That these inputs meet the conditions was checked without a GPU, with the host rule
    of BulletRobot on the oracle run robot by robot on the same pulses and boxes
    (tests/test_sim_terrain.py::test_the_inputs_of_the_gpu_kernel_test_meet_its_conditions: installed after step 26, first catches at steps 30 - 47)."""
    rb, sim, _ = _sim(hip_lib, len(LIFTS))
    gz = min(float(M.translation[2]) for M in rb.foot_placements)
    cfg = cr.config({}, ground_z=gz)
    sim.contacts(cfg)
    got, first, boxes, installed, _ = _run_lifts(sim, rb, cfg)
    print("boxes installed after step %s; first catches %s; lift-offs %s touchdowns %s" % (installed, first, got["liftoffs"][:, 1], got["touchdowns"][:, 1]))
    assert installed is not None
    assert np.all(got["liftoffs"][:, 1] >= 1) and np.all(got["touchdowns"][:, 1] >= 1) and np.all(got["in_contact"] == 1.0)
    on_box = [b for b, (_, _, kind, _) in enumerate(LIFTS) if first[b] is not None and first[b][0] > installed and first[b][1] == boxes[b, 0, 4]]
    on_plane = [b for b in range(len(LIFTS)) if first[b] is not None and first[b][1] == gz]
    assert on_box == [b for b, l in enumerate(LIFTS) if l[2] == "under"] and len(on_box) >= 5
    assert on_plane == [b for b, l in enumerate(LIFTS) if l[2] != "under"] and len(on_plane) >= 2
    assert np.all(boxes[on_box, 0, 4] > gz + 0.004)
    sim.close()


@pytest.mark.gpu
def test_nothing_changes_without_a_terrain(hip_lib):
    """Rule on and metrics on, 70 steps of the flat test's pulses: no terrain call, terrain(None) after a terrain, and zero boxes give the same bits in
    states, wrenches, rows of the rule and rows of the metrics."""
    B = 8
    runs = []
    for variant in ("never", "set and dropped", "zero boxes", "zero boxes per robot"):
        rb, sim, _ = _sim(hip_lib, B)
        m = rb.model
        gz = min(float(M.translation[2]) for M in rb.foot_placements)
        sim.contacts(cr.config({}, ground_z=gz))
        if variant == "set and dropped":
            sim.terrain(cr.stairs([0.0, 0.0, gz + 0.02], 0.04))
            sim.terrain(None)
        elif variant != "never":
            sim.terrain(np.zeros((0, 5)) if variant == "zero boxes" else np.zeros((B, 0, 5)))
        sim.metrics({})
        amps, spans = 120.0 + 10.0 * np.arange(B), 12 + np.arange(B) % 4
        q0 = rb.x0[:m.nq].copy()
        x = np.tile(rb.x0, (B, 1))
        out = []
        for k in range(70):
            x, wr = sim.simulate_torque(x, _batch_lift(m, q0, x, k, amps, spans), 1, DT, wrenches=True)
            out += [x.copy(), wr.copy(), sim.read_contacts(raw=True)]
        met = sim.read_metrics()
        out += [np.asarray(met[k]) for k in sorted(met)]
        assert np.all(cr.unpack(out[-len(met) - 1])["touchdowns"][:, 1] >= 1)
        runs.append(out)
        sim.close()
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        for a, b in zip(runs[0], other):
            assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_device_rule_equals_the_host_rule_on_stairs(hip_lib):
    """BulletRobot(device_contacts=True) against BulletRobot() under the lift sequence with span 25, createStairs (a 2 cm rise whose first step lies under
    the feet) called on both once the released right sole is above the step by 2 ground_tol: the same in_contact after every step, states within 1e-9
    (the flat test's bound), the sole caught on the first step's top by both."""
    from mpc_benchmark_amd.bullet_robot import BulletRobot
    rb = Robot()
    m = rb.model
    host = BulletRobot([n for n in m.names], None, None, 1e-3, m, library=hip_lib)
    dev = BulletRobot([n for n in m.names], None, None, 1e-3, m, library=hip_lib, device_contacts=True)
    for r in (host, dev):
        r.initializeJoints(rb.x0[:m.nq])
    q0 = host.x[:host.model.nq].copy()
    sole = host.data.oMf[host.frame_ids[1]].translation.copy()
    rise = 0.02
    pose = [sole[0] + 0.05, 0.0, host.ground_z + rise / 2]
    top = cr.stairs(pose, rise)[0, 4]
    flags, worst, installed, caught = [], 0.0, None, None
    for k in range(100):
        tau = lift_torques(host, q0, k, span=25)
        host.execute(tau)
        dev.execute(tau)
        assert dev.in_contact == host.in_contact, (k, dev.in_contact, host.in_contact)
        worst = max(worst, np.max(np.abs(dev.x - host.x)))
        assert worst <= 1e-9, (k, worst)
        if flags and not flags[-1][1] and host.in_contact[1] and caught is None:
            caught = k
            assert installed is not None and host._contact_pose[1].translation[2] == top
            assert dev._native.read_contacts()["anchor_p"][0, 1, 2] == top
        flags.append(tuple(host.in_contact))
        if installed is None and not host.in_contact[1] and host._z_prev[1] > top + 2 * host.ground_tol:
            host.createStairs(pose, rise)
            dev.createStairs(pose, rise)
            np.testing.assert_array_equal(dev._native.read_terrain(), cr.stairs(pose, rise))
            installed = k
    print("device rule vs host rule on stairs over 100 steps: states %.1e; installed after step %s, caught at step %s" % (worst, installed, caught))
    assert (True, False) in flags and flags[-1] == (True, True) and caught is not None
    r = dev._native.read_contacts()
    np.testing.assert_allclose(r["anchor_p"][0, 1], host._contact_pose[1].translation, atol=1e-12)
    assert r["anchor_p"][0, 1, 2] == top
    for r in (host, dev):
        r.close()


def _kino(lib, batch, horizon=40, periods=80, walk=None, **kw):
    p = KinodynamicPipeline(KinodynamicProblem(horizon=horizon), batch=batch, library=lib, walk={} if walk is None else walk, perturb=True, sigma_q=0.005,
                            sigma_v=0.01, **kw)
    p.mpc.options.num_threads = 8
    p.mpc.native.set_options(p.mpc.options)
    p.mpc.prepare_schedule(periods)
    assert all(s.converged >= 0 for s in p.cold_solve())
    return p


SHIM = 0.002   # m: the thin box pushed under the right sole of a standing robot


def _shim(rb):
    """a 2 mm box under the right sole (and not under the left)"""
    gz = min(float(M.translation[2]) for M in rb.foot_placements)
    return np.array([box_at_the_right_sole(np.asarray(rb.foot_placements[1].translation, dtype=float), gz + SHIM, "under")]), gz


def _free_the_right_sole(p):
    """the rows of a standing pipeline with the right sole released and marked lifted: the first step's rule finds it within ground_tol of the box
    under it and catches it there, 2 mm above where it stands"""
    rows = p.sim.read_contacts(raw=True)
    rows[:, cr.O_IN + 1] = 0.0
    rows[:, cr.O_LIFTED + 1] = 1.0
    p.sim.set_contacts(rows)
    return rows


@pytest.mark.gpu
def test_device_loops_equal_host_glue_with_rule_and_terrain(hip_lib):
    """The three pipelines with rule and terrain, batch 8, 6 periods, the first of which contains a catch on a box (a 2 mm box under the right sole, the
    sole released by hand: caught on the box top at the first step, then pulled up to it): device loop against host glue within the bounds of the
    flat-ground test (kinodynamic and centroidal 1e-9, full dynamics 1e-12 / 1e-10), the same rows of the rule."""
    B, rule = 8, {}
    shim, gz = _shim(Robot())
    cases = ((lambda: _kino(hip_lib, B, contact_rule=rule, terrain=shim), "forces", 1e-9, 1e-9),
             (lambda: centroidal_pipeline(hip_lib, batch=B, walk={}, contact_rule=rule, terrain=shim), "forces", 1e-9, 1e-9),
             (lambda: fulldynamic_pipeline(hip_lib, batch=B, walk={}, contact_rule=rule, terrain=np.tile(shim, (B, 1, 1))), "wrenches", 1e-12, 1e-10))
    for make, out, tol0, tol in cases:
        pl, ph = make(), make()
        for p in (pl, ph):
            _free_the_right_sole(p)
        worst = []
        for t in range(6):
            pl.tick()
            ph.tick(host_glue=True)
            ol, oh = getattr(pl, out).reshape(B, -1), getattr(ph, out).reshape(B, -1)
            e = max(rel_cols(pl.x, ph.x, 1e-3), rel_cols(pl.x_prev, ph.x_prev, 1e-3), rel_cols(pl.torques, ph.torques, 1.0), rel_cols(ol, oh, 1.0))
            worst.append(e)
            rl, rh = cr.unpack(pl.sim.read_contacts(raw=True)), cr.unpack(ph.sim.read_contacts(raw=True))
            for f in FLAGS:
                np.testing.assert_array_equal(rl[f], rh[f], err_msg="%s period %d %s" % (type(pl).__name__, t, f))
            if t == 0:
                assert np.all(rl["touchdowns"][:, 1] >= 1) and np.all(rl["anchor_p"][:, 1, 2] == gz + SHIM) and np.all(rl["anchor_p"][:, 0, 2] == gz)
                assert np.all(rh["anchor_p"][:, 1, 2] == gz + SHIM)
        print("%s with rule and terrain: device loop vs host glue %s; touchdowns %s" % (type(pl).__name__, " ".join("%.1e" % w for w in worst), rl["touchdowns"][0]))
        for t, e in enumerate(worst):
            assert e <= (tol0 if t == 0 else tol), (type(pl).__name__, t, e)


def _mirror_rows(start_rows, rec, cfg, terrain):
    """the rows of the rule each recorded step was integrated with, and the rows after the last: the mirror run over the record"""
    rows, before = start_rows, []
    for k in range(rec["x"].shape[0]):
        before.append(rows)
        rows = cr.step(rows, rec["sole_p"][k][..., 2], rec["wrenches"][k][..., 2], rec["sole_R"][k], rec["sole_p"][k], cfg, terrain=terrain)
    return np.array(before), rows


@pytest.mark.gpu
def test_metrics_with_terrain_equal_the_mirror(hip_lib):
    """Device metric rows against from_record(..., terrain=, contact_rows=): mpc_simulate_torque over the eight lifts onto their boxes, and the kinodynamic
    device loop over a catch on a box; counts exactly, the rest at the 1e-12 of test_gpu_sim_metrics.py.  The latched heights are heights above the
    ground, and standing on a box is no fall."""
    rb, sim, _ = _sim(hip_lib, len(LIFTS))
    gz = min(float(M.translation[2]) for M in rb.foot_placements)
    cfg = cr.config({}, ground_z=gz)
    sim.contacts(cfg)
    start = []

    def measure_from_here(x):   # record and metrics from the step after the installation: every step they see has the terrain
        sim.record(LIFT_STEPS)
        sim.metrics({})
        start.append(x)

    rows, first, boxes, installed, before = _run_lifts(sim, rb, cfg, on_install=measure_from_here)
    rec, got = sim.read_record(), sim.read_metrics()
    S = LIFT_STEPS - installed - 1
    assert rec["x"].shape[0] == S and np.all(got["steps"] == S)
    want = lm.from_record(rec, start[0], DT, terrain=boxes, contact_rows=before[installed + 1:], ground_z=gz)
    _agree(got, want, _near_zero_margins([rec], start[0]))
    flat = lm.from_record(rec, start[0], DT)
    on = [b for b, l in enumerate(LIFTS) if l[2] == "under"]
    print("simulate_torque with terrain, %d steps: sole_z0 right %s (absolute %s), fall_step %s" % (S, got["sole_z0"][:, 1], flat["sole_z0"][:, 1], got["fall_step"]))
    # latched above the ground: the right soles over their boxes by the boxes' heights less than the absolute latch
    np.testing.assert_allclose(got["sole_z0"][on, 1], flat["sole_z0"][on, 1] - boxes[on, 0, 4], rtol=0, atol=1e-12)
    assert np.all(got["fall_step"] == -1) and np.all(rows["in_contact"] == 1.0)
    sim.close()
    # a device loop: the kinodynamic pipeline over the catch on the 2 mm box
    shim, gz = _shim(Robot())
    p = _kino(hip_lib, 8, contact_rule={}, terrain=shim)
    start = _free_the_right_sole(p)
    p.sim.record(4 * p.substeps)
    p.sim.metrics({})
    x_start, recs = p.x.copy(), []
    for _ in range(4):
        p.tick()
        recs.append(p.sim.read_record())
    rec = _cat(recs)
    rule_cfg = cr.config({}, ground_z=gz)
    before, end = _mirror_rows(start, rec, rule_cfg, shim)
    dev = cr.unpack(p.sim.read_contacts(raw=True))
    for f in FLAGS:
        np.testing.assert_array_equal(dev[f], cr.unpack(end)[f], err_msg=f)
    assert np.all(dev["anchor_p"][:, 1, 2] == gz + SHIM)
    got = p.sim.read_metrics()
    _agree(got, lm.from_record(rec, x_start, p.sim_dt, terrain=shim, contact_rows=before, ground_z=gz), _near_zero_margins(recs, x_start))
    assert np.all(got["steps"] == 4 * p.substeps)


WALK_PERIODS, LANDING = 150, 139   # the kinodynamic walk at N = 40: the right foot's first landing is scheduled at period 139 (test_gpu_sim_contacts.WALK)


def _stairs_walk(lib, terrain):
    """-> (pipeline, boxes, footholds, ground_z, per robot the first touchdown of the right sole (step, anchor z, anchor x), the highest anchor z seen at the
    end of any period).  Failure isolation as in the tools: a robot whose MPC fails sits the rest out instead of ending the run."""
    rb = Robot()
    boxes, holds = stairs_under_walk(rb, 0.3, 0.10)
    p = _kino(lib, 8, periods=WALK_PERIODS + 16, walk=dict(z_height=0.10), contact_rule={}, terrain=boxes if terrain else None)
    p.mpc.enable_failure_isolation(auto_revive=False)
    p.sim.metrics({})
    gz = min(float(M.translation[2]) for M in rb.foot_placements)
    highest = np.full((8, 2), -np.inf)
    first = [None] * 8
    for _ in range(WALK_PERIODS):
        p.tick()
        r = p.sim.read_contacts()
        highest = np.maximum(highest, r["anchor_p"][..., 2])
        for b in range(8):
            if first[b] is None and r["touchdowns"][b, 1] >= 1:
                first[b] = (r["last_touchdown"][b, 1], r["anchor_p"][b, 1, 2], r["anchor_p"][b, 1, 0]) if r["touchdowns"][b, 1] == 1 else (np.nan, np.nan, np.nan)
    return p, boxes, holds, gz, first, highest


@pytest.mark.gpu
def test_kinodynamic_walk_onto_the_first_step(hip_lib):
    """8 perturbed robots of the kinodynamic pipeline walk with z_height = 0.10 through the first scheduled landing (period 139) plus 11 periods, the
    reference's staircase laid under the generator's footholds (``stairs_under_walk``: each landing point in the middle of the visible tread, the top of
    step k at ground_z + (k + 1) 0.10 exactly).

    Terrain side (asserted): every robot's swing (right) foot has a touchdown whose anchor z is exactly the top of the first step, every anchor of the
    window lies on the height function, the stance foot's anchor stays on the plane, and no robot is fallen by the verdict above the ground when its
    swing foot touches the step.  The same robots on the same walk WITHOUT the staircase have no anchor above ground_z at the end of any period of the
    window: the foot aims 10 cm above the only ground there is.

    Controller side (a finding, printed, not asserted; profiles/stairs_walk.txt): the walk does not survive that landing.  The generator's swing curve
    (swing_apex = 0.15 is a Bezier control height) passes the front edge of the tread, 0.15 m before the foothold, at a planned 0.09 m: below the tread.
    The rule catches the sole there at once, at mid-swing, 35 - 39 periods before the scheduled landing (64 robots: steps 1003 - 1037 against 1390), the
    MPC goes on planning a swing, and every robot then loses its MPC (periods 120 - 148) and falls (first at step 1299).  Nothing in the terrain code
    can or should change that: risers are not modelled, and the walk generators are not part of this change."""
    p, boxes, holds, gz, first, _ = _stairs_walk(hip_lib, True)
    assert boxes[0, 4] == gz + 0.10 and boxes[0, 0] < holds[0, 0] < boxes[1, 0] and abs(holds[0, 0] - 0.5 * (boxes[0, 0] + boxes[1, 0])) < 1e-12
    r, met = p.sim.read_contacts(), p.sim.read_metrics()
    print("stairs walk, 8 robots: first right touchdown (step, anchor z, anchor x) %s (scheduled step %d, planned x %.3f, tread from x %.3f); at the end of "
          "period %d: right touchdowns %s, anchors z right %s left %s, fall_step %s, MPC lost %s"
          % ([tuple(np.round(f, 3)) for f in first], p.substeps * LANDING, holds[0, 0], boxes[0, 0], WALK_PERIODS, r["touchdowns"][:, 1], r["anchor_p"][:, 1, 2],
             r["anchor_p"][:, 0, 2], met["fall_step"], sorted((t, b) for (t, b, _, _) in p.mpc.lost)))
    for b in range(8):
        assert first[b] is not None and first[b][1] == boxes[0, 4], (b, first[b])                       # caught on the first step's top, exactly
        assert boxes[0, 0] <= first[b][2] <= boxes[0, 1]
        assert met["fall_step"][b] == -1 or met["fall_step"][b] > first[b][0], (b, met["fall_step"][b])   # standing when the foot touched the step
    h = p.sim.terrain_height(np.ascontiguousarray(r["anchor_p"][..., :2]))
    assert np.all(r["anchor_p"][..., 2] == h)                                                           # whatever was caught later lies on h too
    q, _, _, gz, first_flat, highest = _stairs_walk(hip_lib, False)
    rq = q.sim.read_contacts()
    print("the same walk without the staircase: right touchdowns %s in_contact %s; highest anchor above ground_z %s" % (rq["touchdowns"][:, 1], rq["in_contact"][:, 1],
                                                                                                                    np.max(highest - gz)))
    assert np.all(highest <= gz)


@pytest.mark.gpu
def test_errors(hip_lib):
    rb, sim, tables = _sim(hip_lib, 2)
    box = np.array([[0.0, 1.0, 0.0, 1.0, 0.1]])
    lib, C = hip_lib, __import__("ctypes")
    from mpc_benchmark_amd._capi import MpcSimTerrainConfig, _dp

    def raw(n, per, boxes):
        cfg = MpcSimTerrainConfig(n, per)
        rc = lib.mpc_sim_terrain(sim._h, C.byref(cfg), None if boxes is None else _dp(np.ascontiguousarray(boxes, dtype=float)))
        return rc, (lib.mpc_last_error(sim._h) or b"").decode()

    # terrain without the rule
    for call in (lambda: sim.terrain(box), lambda: sim.terrain(None), lambda: sim.read_terrain(), lambda: sim.terrain_height(np.zeros((2, 1, 2)))):
        with pytest.raises(RuntimeError, match="rule is off"):
            call()
    sim.contacts({})
    # each rejection of the header (the raw entry point: the binding checks most of them before the library does)
    for n, per, boxes, what in ((-1, 0, box, "n_boxes"), (17, 0, np.zeros((17, 5)), "n_boxes"), (1, 2, box, "per_robot"), (1, -1, box, "per_robot"),
                                (1, 0, None, "null"), (1, 0, [[0.0, 1.0, 0.0, 1.0, np.nan]], "non-finite"), (1, 0, [[-np.inf, 1.0, 0.0, 1.0, 0.1]], "non-finite"),
                                (1, 0, [[1.0, 0.0, 0.0, 1.0, 0.1]], "x_lo > x_hi"), (1, 1, [[[0.0, 1.0, 0.0, 1.0, 0.1]], [[0.0, 1.0, 1.0, 0.0, 0.1]]], "y_lo > y_hi")):
        rc, err = raw(n, per, boxes)
        assert rc == -1 and what in err, (n, per, what, rc, err)
    assert sim.read_terrain().shape == (0, 5)   # (a refused terrain changes nothing)
    with pytest.raises(ValueError):
        sim.terrain(np.zeros((3, 1, 5)))        # per robot, for another batch
    with pytest.raises(RuntimeError, match="non-finite"):
        sim.terrain_height(np.full((2, 1, 2), np.nan))
    with pytest.raises(ValueError):
        sim.terrain_height(np.zeros((3, 1, 2)))
    # a reset keeps the terrain and uses the new ground_z; the rule off drops it
    sim.terrain(box)
    pts = np.array([[[0.5, 0.5], [2.0, 2.0]]] * 2)
    np.testing.assert_array_equal(sim.terrain_height(pts), [[0.1, 0.0]] * 2)
    sim.contacts({"ground_z": 0.05})
    np.testing.assert_array_equal(sim.read_terrain(), box)
    np.testing.assert_array_equal(sim.terrain_height(pts), [[0.1, 0.05]] * 2)
    sim.contacts({"ground_z": 0.25})
    np.testing.assert_array_equal(sim.terrain_height(pts), [[0.25, 0.25]] * 2)
    sim.contacts(None)
    with pytest.raises(RuntimeError, match="rule is off"):
        sim.read_terrain()
    sim.contacts({})
    assert sim.read_terrain().shape == (0, 5)
    np.testing.assert_array_equal(sim.terrain_height(pts), [[0.0, 0.0]] * 2)
    # a handle that is not a torque-driven simulator (a centroidal plan)
    from mpc_benchmark_amd.ensemble import EnsembleMPC
    from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
    plan = EnsembleMPC(CentroidalProblem(horizon=10), batch=2, library=hip_lib).native
    for call in (lambda: plan.terrain(box), lambda: plan.read_terrain(), lambda: plan.terrain_height(np.zeros((2, 1, 2)))):
        with pytest.raises(RuntimeError, match="simulator handle"):
            call()
    sim.close()
