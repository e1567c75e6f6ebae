"""The centroidal control pipeline (mpc_benchmark_amd/pipeline.py CentroidalPipeline: MPC tick -> task errors -> centroidal state and K_0 feedback ->
IK + ID QP assembled on the library -> torque-driven simulator step, centroidal_talos.py:353-468) with the host glue on the oracle (CPU)."""
import numpy as np
import pytest

from mpc_benchmark_amd import references
from mpc_benchmark_amd.aligator import manifolds
from mpc_benchmark_amd.pipeline import CentroidalPipeline, centroidal_state
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.robot import minipin as pin


def centroidal_pipeline(lib, batch=2, horizon=40, walk=None, **kw):
    p = CentroidalPipeline(CentroidalProblem(horizon=horizon), batch=batch, library=lib, walk=walk, sigma_q=0.005, sigma_v=0.01, **kw)
    p.mpc.options.num_threads = 8
    p.mpc.native.set_options(p.mpc.options)
    p.mpc.prepare_schedule(80)
    assert all(s.converged >= 0 for s in p.cold_solve())
    return p


def reference_task_errors(p, x_ik, refs, dH):
    """references.compute_ID_references (talos_utils.py:375-402) robot by robot, with dH appended: the layout of mpc_qp_solve_ikid."""
    m = p.model
    space, data = manifolds.MultibodyPhaseSpace(m), m.createData()
    out = []
    for x, r, h in zip(x_ik, refs, dH):
        pin.forwardKinematics(m, data, x[:m.nq], x[m.nq:])
        pin.updateFramePlacements(m, data)
        se3 = [[pin.SE3(r[f, k, :9].reshape(3, 3), r[f, k, 9:]) for k in range(2)] for f in range(2)]
        e = references.compute_ID_references(space, m, data, p.qp.contact_ids[0], p.qp.contact_ids[1], p.qp.base_id, p.qp.torso_id, p.x_posture, x,
                                             se3[0], se3[1], p.ref_dt)
        out.append(np.concatenate([np.asarray(a, dtype=float).reshape(-1) for a in e] + [h]))
    return np.array(out)


def test_centroidal_pipeline_keeps_the_robots_standing_on_the_oracle(oracle_lib):
    """25 MPC periods (250 IK + ID QPs and simulator steps) of two perturbed robots, the script's walk planned: every solve returns, nobody falls
    (base height within 5e-3 of the start; measured: 2e-4), both soles carry weight, the torques stay in the QP's box (to its eps_abs)."""
    p = centroidal_pipeline(oracle_lib, walk={})
    z0 = p.x[:, 2].copy()
    lim = np.asarray(p.model.effortLimit, dtype=float)[6:]
    for _ in range(25):
        st = p.tick(host_glue=True)
        assert all(s.converged >= 0 for s in st)
        assert all(i.status != 2 for i in p.qp.last_info)
    assert list(p.contact_state()) == [True, True]
    assert np.all(np.abs(p.x[:, 2] - z0) < 5e-3), p.x[:, 2] - z0
    assert np.all(p.forces[:, 2] > 100.0) and np.all(p.forces[:, 8] > 100.0)
    assert np.all(np.abs(p.torques) <= lim + p.qp.qp.settings.eps_abs)


def test_centroidal_pipeline_follows_the_order_of_the_script(oracle_lib):
    """centroidal_talos.py:408-462: the task errors of period t are taken at the measurement before the last execute of period t - 1; the x0 of the
    solve that closes period t is new_x of the measurement before ITS last execute; that measurement is the one the last simulator step started from."""
    p = centroidal_pipeline(oracle_lib, walk={})
    for t in range(4):
        stale = p.x_prev.copy()
        p.tick(host_glue=True)
        want = reference_task_errors(p, stale, p.foot_refs(), p.dH)
        assert np.max(np.abs(p.ik - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), t
        c = centroidal_state(p.model, p.x_prev)
        for b in range(p.batch):  # (minipin itself, robot by robot)
            d = p.model.createData()
            com = pin.centerOfMass(p.model, d, p.x_prev[b, :p.nq])
            hg = pin.computeCentroidalMomentum(p.model, d, p.x_prev[b, :p.nq], p.x_prev[b, p.nq:])
            assert np.max(np.abs(c[b] - np.concatenate([com, hg.linear, hg.angular]))) < 1e-12
        assert np.max(np.abs(p.c_prev - c)) < 1e-12
        assert np.max(np.abs(p.mpc.native.get_x0() - c)) < 1e-12   # handed to the solve
        assert np.array_equal(p.sim.simulate_torque(p.x_prev, p.torques, 1, p.sim_dt), p.x)


def test_ensemble_step_halves_compose_to_step(oracle_lib):
    """EnsembleMPC.step = plan_tick + solve_tick, bit for bit (the pipeline runs its loop between the two halves)."""
    from mpc_benchmark_amd.ensemble import EnsembleMPC
    out = []
    for split in (False, True):
        e = EnsembleMPC(CentroidalProblem(horizon=20), batch=2, library=oracle_lib)
        e.prepare_schedule(10)
        e.cold_solve()
        e.enable_walk()
        for _ in range(5):
            if split:
                e.plan_tick()
                e.solve_tick()
            else:
                e.step()
        r = e.results(gains=False)
        out.append((r["xs"], r["us"]))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_device_loop_is_not_exported_by_the_oracle(oracle_lib):
    """The centroidal device loop is HIP only: the oracle still loads and binds, the call says why it cannot run."""
    p = CentroidalPipeline(CentroidalProblem(horizon=20), batch=2, library=oracle_lib)
    assert not hasattr(oracle_lib, "mpc_qp_ikid_low_level_steps")
    with pytest.raises(RuntimeError, match="not exported"):
        p.qp.qp.ikid_low_level_steps(p.mpc.native, p.sim, p.qp._frame_idx, p.qp._base_idx, p.qp._torso_idx, p.qp.weights, p.qp._gains, p.qp.Cmin,
                                     p.qp.l_box, p.qp.u_box, p.x_posture, p.foot_refs(), p.ref_dt, np.ones((2, 2), dtype=np.int32), 1, 1e-3, x=p.x, x_ik=p.x)
    with pytest.raises(RuntimeError, match="not exported"):
        p.tick()
