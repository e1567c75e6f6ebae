"""Per-robot foot references of the centroidal walk (EnsembleMPC.enable_walk(per_instance=True) of the contact-pose problem, and CentroidalPipeline with
it): every robot's footholds are planned from the soles of ITS measured whole-body state (centroidal_talos.py:369-384), the translations are written
into the instance's own stage tables for the feet that stand in a knot's stage, and the low-level task errors are taken against the robot's own samples.
Host generator on the oracle (CPU); the device generator is held to it in tests/test_gpu_centroidal_walk_per_robot.py."""
import numpy as np
import pytest

from mpc_benchmark_amd import references
from mpc_benchmark_amd.aligator import manifolds
from mpc_benchmark_amd.ensemble import EnsembleMPC, ensemble_initial_states
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.robot import minipin as pin
from tests.test_centroidal_pipeline import centroidal_pipeline, reference_task_errors

N, B = 20, 3
# The schedule's first take-off is at index 20, its landing at 100 (20 ticks of double support, 80 of swing).  The runs start at tick 15 — every
# knot of the cold-solved horizon still holds a double-support stage, as the tables do — with the generator's countdowns advanced to that tick, and
# end after tick 124: the planning window of the right foot (ticks 21 - 40), its take-off at knot 0 (40), its landing (120), the forward rule after it.
T0, T1 = 15, 125
YAW = (0.1, -0.1, 0.05)
OFFSET = ((0.0, 0.0), (0.03, -0.02), (-0.02, 0.04))
DRIFT = ((1e-3, 0.0), (0.0, 1e-3), (-6e-4, -8e-4))   # a millimetre per tick


def flat(M):
    return np.concatenate([np.asarray(M.rotation, dtype=float).reshape(-1), np.asarray(M.translation, dtype=float)])


def make_ensemble(lib, batch=B, **walk):
    e = EnsembleMPC(CentroidalProblem(horizon=N), batch=batch, library=lib, seed=3)
    e.x0 = e.x0 + 1e-3 * np.arange(batch)[:, None] * np.array([1.0, -1.0, 0.5, 0, 0, 0, 0, 0, 0])   # perturbed centroidal states
    e.options.tol = 0.0
    e.native.set_options(e.options)
    e.prepare_schedule(T1 + 1)
    e.cold_solve(max_iters=8)
    e.tick = T0
    e.enable_walk(**walk)
    for _ in range(T0):
        references.update_timings(e._walk["lists"][3], e._walk["lists"][2], e._walk["lists"][1], e._walk["lists"][0])
    return e


def measured_states(pd, t):
    """Whole-body states of B robots at tick t: perturbed joints, a base yaw and an x, y offset per robot, drifting a millimetre per tick."""
    m = pd.robot.model
    X = ensemble_initial_states(pd.robot.x0, manifolds.MultibodyPhaseSpace(m), B, 7, 0.01, 0.02)
    for b in range(B):
        X[b, 0] += OFFSET[b][0] + DRIFT[b][0] * t
        X[b, 1] += OFFSET[b][1] + DRIFT[b][1] * t
        X[b, 3:7] = (0.0, 0.0, np.sin(0.5 * YAW[b]), np.cos(0.5 * YAW[b]))
    return X


class SingleRobotReference:
    """references.FootTrajectory (the class the drop-in fixtures hold to talos_utils.py) for one robot on pin.framesForwardKinematics poses."""

    def __init__(self, pd, horizon, skip=0):
        spec, rb = pd.walk_spec(), pd.robot
        lf, rf = rb.foot_placements
        self.pd, self.spec, self.data = pd, spec, rb.model.createData()
        self.gen = references.FootTrajectory(lf.copy(), rf.copy(), spec["T_SS"], spec["T_DS"], horizon, 0.15, spec["x_forward"], 0.0, 0.0, 0.18, 0.0)
        self.lists = [list(v) for v in references.contact_event_times(pd.contact_phases, horizon)]
        for _ in range(skip):
            self.timings()

    def timings(self):
        return references.update_timings(self.lists[3], self.lists[2], self.lists[1], self.lists[0])

    def update(self, x):
        rb = self.pd.robot
        pin.framesForwardKinematics(rb.model, self.data, np.asarray(x, dtype=float)[:rb.model.nq])
        LF, RF = (self.data.oMf[f].copy() for f in rb.foot_frame_ids)
        ev = self.timings()
        if self.spec["forward_rule"](*ev):
            self.gen.updateForward(0, 0, 0.18, 0.0, self.spec["forward_z_left"], 0, 0.15)
        L, R = self.gen.updateTrajectory(*ev, LF, RF)
        return np.array([flat(M) for M in L]), np.array([flat(M) for M in R])


def stance_of_knots(pd, tick):
    """[N][2]: contact flags of the stage knot j holds before the rotation of `tick`"""
    return np.array([pd.contact_phases[max(0, j - N + tick) % pd.t_mpc] for j in range(N)], dtype=bool)


def instance_tables(e):
    """[B][N][max_stage_doubles]: the parameter table every instance uses at every knot (a stage's own table is shorter: zeros behind it)"""
    out = np.zeros((e.batch, N, e.dims.max_stage_doubles))
    for b in range(e.batch):
        for k in range(N):
            tab = e.native.debug_get("inst_params", k, b)
            out[b, k, :tab.size] = tab
    return out


def generator_plan(e):
    """[B][4][12] start / final pose of the left foot, start / final pose of the right foot: the generator's plan, wherever it runs"""
    w = e._walk
    if w["poses"] == "device":
        return e.native.walk_poses_get_state()
    g = w["batch"]
    return np.stack([np.concatenate([P[0].reshape(e.batch, 9), P[1]], axis=1) for P in (g.sL, g.fL, g.sR, g.fR)], axis=1)


def run_measured(lib, generator, ticks=(T0, T1)):
    """The ensemble walked on per-tick measurements; after the references of every tick were written (before the rotation): (tick, X, instance
    tables [B][N][P], plan [B][4][12], samples [B][2][2][12]).  Also what the GPU test runs once per generator."""
    e = make_ensemble(lib, per_instance=True, generator=generator)
    for t in range(*ticks):
        assert e.tick == t
        X = measured_states(e.pd, t)
        e._walk["x_measured_all"] = X
        e.plan_tick()
        samples = e.native.walk_poses_samples() if generator == "device" else e._walk["refs_all"].copy()
        yield e, t, X, instance_tables(e), generator_plan(e), samples
        st = e.solve_tick()
        assert all(s.converged >= 0 for s in st)


def test_without_a_plant_every_instance_carries_the_shared_references(oracle_lib):
    """No measurement: every instance's feet are where its own previous references put them, so the per-instance tables hold exactly the shared
    run's references and the solves agree."""
    shared, per = make_ensemble(oracle_lib), make_ensemble(oracle_lib, per_instance=True)
    assert per._walk["x_measured_all"] is None
    single = SingleRobotReference(shared.pd, N, skip=T0)   # the shared path feeds the generator its own references back: so does this one
    feet = [M.copy() for M in shared.pd.robot.foot_placements]
    offs = per._walk["pose_offs"]
    worst_ref = worst_sol = 0.0
    for t in range(T0, T1):
        for e in (shared, per):
            e.plan_tick()
        ev = single.timings()
        if single.spec["forward_rule"](*ev):
            single.gen.updateForward(0, 0, 0.18, 0.0, single.spec["forward_z_left"], 0, 0.15)
        L, R = single.gen.updateTrajectory(*ev, feet[0].copy(), feet[1].copy())
        feet = [L[1], R[1]]
        stance = stance_of_knots(per.pd, t)
        tabs = instance_tables(per)
        for j in range(N):
            want_tab = shared.native.debug_get("inst_params", j, 0)
            for i, refs in ((0, L), (1, R)):
                if stance[j, i]:
                    for off in offs[i]:
                        assert np.array_equal(want_tab[off:off + 3], np.asarray(refs[j].translation))   # (the shared run writes what the single class gives)
                        worst_ref = max(worst_ref, float(np.max(np.abs(tabs[:, j, off:off + 3] - refs[j].translation))))
        assert worst_ref <= 1e-13, (t, worst_ref)
        for e in (shared, per):
            e.solve_tick()
        rs, rp = shared.results(gains=False), per.results(gains=False)
        for key in ("xs", "us"):
            worst_sol = max(worst_sol, float(np.max(np.abs(rp[key] - rs[key]) / np.maximum(1.0, np.abs(rs[key])))))
        assert worst_sol <= 1e-8, (t, worst_sol)
    assert per.replanning_ticks == shared.replanning_ticks >= 20
    print("worst reference difference %.3g, worst xs / us difference %.3g" % (worst_ref, worst_sol))


def test_measured_soles_give_every_robot_its_own_plan(oracle_lib):
    singles = None
    worst = worst_samples = 0.0
    for e, t, X, tabs, plan, samples in run_measured(oracle_lib, "host"):
        if singles is None:
            singles = [SingleRobotReference(e.pd, N, skip=T0) for _ in range(B)]
            offs = e._walk["pose_offs"]
        stance = stance_of_knots(e.pd, t)
        for b in range(B):
            L, R = singles[b].update(X[b])
            for j in range(N):
                shared_tab = e._table_for_tick(max(0, j - N + t) % e.pd.t_mpc)[1]
                for i, refs in ((0, L), (1, R)):
                    for off in offs[i]:
                        got = tabs[b, j, off:off + 3]
                        if stance[j, i]:
                            worst = max(worst, float(np.max(np.abs(got - refs[j, 9:12]))))
                        else:   # a foot that does not stand in that stage: nothing was written (centroidal_talos.py:376, 381)
                            assert np.array_equal(got, shared_tab[off:off + 3]), (t, b, j, i)
            worst_samples = max(worst_samples, float(np.max(np.abs(samples[b, 0] - L[:2]))), float(np.max(np.abs(samples[b, 1] - R[:2]))))
        assert worst <= 1e-12 and worst_samples <= 1e-12, (t, worst, worst_samples)
    final = plan[:, 3, 9:12]   # final foothold of the right foot of every robot
    for a in range(B):
        for b in range(a + 1, B):
            assert np.linalg.norm(final[a] - final[b]) > 1e-3, (a, b, final)
    assert e.replanning_ticks >= 20 and not np.any(stance_of_knots(e.pd, 60).all(axis=1))   # (single-support knots were part of the run)
    print("worst stance offset difference %.3g, worst sample difference %.3g" % (worst, worst_samples))


@pytest.mark.parametrize("fast_forward", [0, 38])
def test_pipeline_plans_from_the_stale_measurement(oracle_lib, fast_forward):
    """centroidal_talos.py:369-371, 408: the references of period t are planned from the soles of x_prev as it stood before the tick, and the task
    errors are taken against each robot's own samples.  ``fast_forward``: the generator's countdowns advanced so that the four periods end inside the
    planning window of the right foot (horizon 40: ticks 41 - 60), where the plan does follow the measurement."""
    p = centroidal_pipeline(oracle_lib, walk=dict(per_instance=True))
    horizon = p.mpc.problem.num_steps
    w = p.mpc._walk
    for _ in range(fast_forward):
        references.update_timings(w["lists"][3], w["lists"][2], w["lists"][1], w["lists"][0])
    singles = [SingleRobotReference(p.pd, horizon, skip=fast_forward) for _ in range(p.batch)]
    for t in range(4):
        stale = p.x_prev.copy()
        p.tick(host_glue=True)
        refs = p.foot_refs()
        assert refs.shape == (p.batch, 2, 2, 12)
        for b in range(p.batch):
            L, R = singles[b].update(stale[b])
            assert np.max(np.abs(refs[b, 0] - L[:2])) <= 1e-12 and np.max(np.abs(refs[b, 1] - R[:2])) <= 1e-12, (t, b)
        want = reference_task_errors(p, stale, refs, p.dH)
        assert np.max(np.abs(p.ik - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), t
    if fast_forward:
        assert w["replanning"] and np.max(np.abs(refs[0] - refs[1])) > 1e-4   # the two robots do track different references


def test_device_generator_is_not_exported_by_the_oracle(oracle_lib):
    """The device generator is HIP only: the oracle says why it cannot run, and the ensemble walks on with the host generator."""
    e = EnsembleMPC(CentroidalProblem(horizon=N), batch=2, library=oracle_lib)
    e.prepare_schedule(8)
    e.cold_solve(max_iters=8)
    assert not hasattr(oracle_lib, "mpc_walk_poses_init")
    with pytest.raises(RuntimeError, match="not exported"):
        e.enable_walk(per_instance=True, generator="device")
    assert e._walk is None
    with pytest.raises(RuntimeError, match="not exported"):
        e.native.walk_poses_samples()
    e.enable_walk(per_instance=True)
    for _ in range(3):
        assert all(s.converged >= 0 for s in e.step())
