"""The device generator of the centroidal walk's per-robot references (include/mpc_walk_poses.h, k_walk_poses) against the numpy generator, and the
centroidal pipeline with it: the measurements the plans are made from never leave the device."""
import numpy as np
import pytest

from mpc_benchmark_amd import references
from mpc_benchmark_amd.pipeline import CentroidalPipeline
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.robot import minipin as pin
from tests._metrics import rel_cols
from tests.test_centroidal_pipeline import centroidal_pipeline, reference_task_errors
from tests.test_centroidal_walk_per_robot import run_measured

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if np.size(a) else 0.0


def test_device_generator_equals_host_generator(hip_lib):
    """The driver of the CPU test (measured soles with a base yaw, an offset and a drift per robot, through the planning window, the take-off, the
    landing and the forward rule) once per generator, measurements from the host in both: every instance table, the plan and the 48 sample doubles per
    robot after every tick within 1e-12 max(1, |value|) (the inputs do not depend on the solver state: no lock-step is needed)."""
    worst = {"tables": 0.0, "plan": 0.0, "samples": 0.0}
    ticks = 0
    for host, dev in zip(run_measured(hip_lib, "host"), run_measured(hip_lib, "device")):
        (_, t, Xh, tabs_h, plan_h, samples_h), (_, td, Xd, tabs_d, plan_d, samples_d) = host, dev
        assert t == td and np.array_equal(Xh, Xd)
        for key, a, b in (("tables", tabs_d, tabs_h), ("plan", plan_d, plan_h), ("samples", samples_d, samples_h)):
            worst[key] = max(worst[key], rel(a, b))
        assert max(worst.values()) <= 1e-12, (t, worst)
        ticks += 1
    assert ticks == 110
    assert np.max(np.abs(plan_d[0, 3, 9:] - plan_d[1, 3, 9:])) > 1e-3   # the robots did plan different footholds
    print("device generator vs host generator over %d ticks: tables %.2e plan %.2e samples %.2e" % (ticks, worst["tables"], worst["plan"], worst["samples"]))


class ShadowGenerator:
    """The numpy generator carried along a pipeline whose generator runs on the device: the same countdowns, the plan seeded from the device's once,
    fed the measurements the pipeline returned to the host; keeps the 18 pose doubles (2 feet x 3 places x 3) of every knot of every robot as the
    rule leaves them (written for the feet that stand in the knot's stage, the shared table's at the appended knot)."""

    def __init__(self, p):
        e = self.e = p.mpc
        w, B, N = e._walk, e.batch, e.problem.num_steps
        self.B, self.N, self.offs = B, N, np.array(w["pose_offs"])
        g = w["batch"]   # (enable_walk builds the numpy generator in either mode: the same constants)
        self.gen = references.FootTrajectoryBatch(g.sL[0], g.sL[1], g.sR[0], g.sR[1], g.T_ss, g.T_ds, N, g.swing_apex, 0.0, 0.0, 0.0, 0.0, 0.0)
        self.gen.tL, self.gen.tR, self.gen.rotationDiff, self.gen.floor_z = g.tL.copy(), g.tR.copy(), g.rotationDiff.copy(), g.floor_z
        plan = e.native.walk_poses_get_state()
        for name, k in (("sL", 0), ("fL", 1), ("sR", 2), ("fR", 3)):
            setattr(self.gen, name, (plan[:, k, :9].reshape(B, 3, 3).copy(), plan[:, k, 9:].copy()))
        self.lists = [list(v) for v in w["lists"]]
        self.poses = np.array([[self.table_poses(e.native.debug_get("inst_params", k, b)) for k in range(N)] for b in range(B)])

    def table_poses(self, tab):
        return np.array([[tab[o:o + 3] for o in self.offs[i]] for i in (0, 1)])

    def update(self, X, tick):
        """the references of `tick` from the measurements X -> samples [B][2][2][12]; self.poses as the tables must hold them before the rotation"""
        e, spec = self.e, self.e._walk["spec"]
        rb = e.pd.robot
        (LR, Lp), (RR, Rp) = pin.frame_placements_batch(rb.model, X[:, :rb.model.nq], rb.foot_frame_ids)
        ev = references.update_timings(self.lists[3], self.lists[2], self.lists[1], self.lists[0])
        if spec["forward_rule"](*ev):
            st = e._walk["step"]
            self.gen.updateForward(0, 0, st["y_gap"], st["y_forward"], spec["forward_z_left"], 0, st["swing_apex"])
        Lb, Rb = self.gen.updateTrajectory(*ev, LR, Lp, RR, Rp)
        for j in range(self.N):
            cs = e.pd.contact_phases[max(0, j - self.N + tick) % e.pd.t_mpc]
            for i, refs in ((0, Lb), (1, Rb)):
                if cs[i]:
                    self.poses[:, j, i, :, :] = refs[:, j, None, 9:12]
        return np.stack([Lb[:, :2], Rb[:, :2]], axis=1)

    def rotate(self, tick):
        """mpc_cycle: knot j takes the table of knot j + 1, the appended knot the shared table of the stage of `tick`"""
        self.poses[:, :-1] = self.poses[:, 1:].copy()
        self.poses[:, -1] = self.table_poses(self.e._table_for_tick(tick % self.e.pd.t_mpc)[1])


def test_pipeline_walks_on_references_planned_on_the_device(hip_lib):
    """Eight perturbed robots, N = 100, device loops, 210 periods (take-off 120, landing 200), the generator on the device reading x_prev where the
    device loop kept it.  Every period the numpy generator, fed the x_prev the previous tick() returned to the host, says what the device must hold:
    the pose doubles of every knot of every robot and the samples within 1e-12 max(1, |value|); the device loop's task errors equal
    compute_ID_references on the device's samples (1e-12 relative to max(1, |value|)); all states finite, every solve returns, nobody falls (base
    height within 0.05 m of its start)."""
    p = centroidal_pipeline(hip_lib, batch=8, horizon=100, walk=dict(per_instance=True, generator="device"))
    T = 210
    p.mpc.prepare_schedule(T + 16)
    e, N = p.mpc, 100
    shadow = ShadowGenerator(p)
    z0 = p.x[:, 2].copy()
    worst = {"tables": 0.0, "samples": 0.0, "ik": 0.0}
    kept = 0
    for t in range(T):
        stale = p.x_prev.copy()
        p._fetch()   # dH of the plan the loop of this period runs on
        dH = p.dH.copy()
        tick = e.tick
        kept += int(p._xik_on_device)
        st = p.tick()
        assert all(s.converged >= 0 for s in st), (t, [s.converged for s in st])
        assert np.all(np.isfinite(p.x)) and np.all(np.abs(p.x[:, 2] - z0) < 0.05), (t, p.x[:, 2] - z0)
        want_samples = shadow.update(stale, tick)
        samples = p.foot_refs()
        worst["samples"] = max(worst["samples"], rel(samples, want_samples))
        shadow.rotate(tick)   # (the tables are read after the tick: one rotation later)
        got = np.array([[shadow.table_poses(e.native.debug_get("inst_params", k, b)) for k in range(N)] for b in range(p.batch)])
        worst["tables"] = max(worst["tables"], rel(got, shadow.poses))
        want_ik = reference_task_errors(p, stale, samples, dH)
        worst["ik"] = max(worst["ik"], rel(p.ik, want_ik))
        assert max(worst.values()) <= 1e-12, (t, worst)
    assert kept == T - 1   # (only the first period's measurement came from the host)
    plan = e.native.walk_poses_get_state()
    spread = np.ptp(plan[:, 3, 9:11], axis=0)
    walked = p.x[:, 0] - p.x_posture[0]
    print("per-robot references on the device over %d periods: tables %.2e samples %.2e task errors %.2e ; base advanced %.3f .. %.3f m, height within %.1f mm ; "
          "spread of the right footholds %.1f x %.1f mm" % (T, worst["tables"], worst["samples"], worst["ik"], walked.min(), walked.max(),
                                                            1e3 * np.max(np.abs(p.x[:, 2] - z0)), 1e3 * spread[0], 1e3 * spread[1]))
    assert np.max(spread) > 1e-4   # the robots do not share one plan


def test_device_loop_equals_host_glue_with_per_robot_references(hip_lib):
    """Device generator + device loop against host generator + host glue, 8 robots, 6 periods, rule off: the comparison and the 1e-9 of the loop
    tests (tests/test_gpu_sim_contacts.py, centroidal row).  The countdowns are advanced so that the last four periods lie in the planning window of
    the right foot, where the plans follow the measurements."""
    B = 8
    pl = centroidal_pipeline(hip_lib, batch=B, walk=dict(per_instance=True, generator="device"))
    ph = centroidal_pipeline(hip_lib, batch=B, walk=dict(per_instance=True))
    for p in (pl, ph):
        lists = p.mpc._walk["lists"]
        for _ in range(38):
            references.update_timings(lists[3], lists[2], lists[1], lists[0])
    worst = []
    for t in range(6):
        pl.tick()
        ph.tick(host_glue=True)
        err = max(rel_cols(pl.x, ph.x, 1e-3), rel_cols(pl.x_prev, ph.x_prev, 1e-3), rel_cols(pl.torques, ph.torques, 1.0),
                  rel_cols(pl.forces.reshape(B, -1), ph.forces.reshape(B, -1), 1.0))
        assert err <= 1e-9, (t, err)
        worst.append(err)
    assert pl.mpc._walk["replanning"] and np.max(np.abs(pl.foot_refs()[0] - pl.foot_refs()[1])) > 1e-5
    print("per-robot references, device loop vs host glue: %s" % " ".join("%.1e" % w for w in worst))
