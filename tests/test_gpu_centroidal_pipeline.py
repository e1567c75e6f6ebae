"""The centroidal control pipeline on the device (mpc_qp_ikid_low_level_steps: csrc/pipeline_ikid_glue.h between the centroidal plan, the IK + ID QP and
the simulator step) against the host glue on HIP and on the oracle, centroidal_talos.py:353-468."""
import numpy as np
import pytest

from mpc_benchmark_amd.pipeline import CentroidalPipeline
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.common import Robot
from mpc_benchmark_amd.robot import minipin as pin
from tests._metrics import rel_cols
from tests.test_centroidal_pipeline import centroidal_pipeline, reference_task_errors


@pytest.mark.gpu
@pytest.mark.parametrize("complete", [False, True])
def test_device_task_errors_equal_compute_ID_references(hip_lib, complete):
    """k_ikid_task_errors: forward kinematics, LOCAL frame velocities, log3 of the orientation errors, the multibody difference of the posture and the
    rates of two reference samples, robot by robot, equal references.compute_ID_references to 1e-12 (relative to max(1, |value|))."""
    cp = CentroidalProblem(horizon=20, robot=Robot(complete=complete))
    p = CentroidalPipeline(cp, batch=4, library=hip_lib, sigma_q=0.02, sigma_v=0.1)
    p.mpc.prepare_schedule(10)
    p.cold_solve()
    rng = np.random.default_rng(3)
    refs = p.foot_refs().copy()
    for b in range(p.batch):  # distinct second samples: nonzero rates, a yaw rate
        for f in range(2):
            R = pin.exp3(rng.normal(size=3) * 0.05) @ refs[b, f, 0, :9].reshape(3, 3)
            refs[b, f, 1, :9], refs[b, f, 1, 9:] = R.reshape(-1), refs[b, f, 0, 9:] + rng.normal(size=3) * 0.01
    x_ik = p.x.copy()
    x_ik[:, p.nq:] += rng.normal(size=(p.batch, p.nv)) * 0.1
    out = p.qp.low_level_steps(p.mpc.native, p.sim, p.x_posture, refs, p.ref_dt, np.ones((p.batch, 2), dtype=np.int32), 1, p.sim_dt, x=p.x, x_ik=x_ik,
                               want_ik=True)
    want = reference_task_errors(p, x_ik, refs, p.dH)
    err = np.max(np.abs(out[5] - want) / np.maximum(1.0, np.abs(want)))
    assert err < 1e-12, err
    print("task errors (%s model): %.2e" % ("complete" if complete else "reduced", err))


def _device_vs_host(lib, ticks, tol):
    pd, ph = centroidal_pipeline(lib, walk={}), centroidal_pipeline(lib, walk={})
    worst = 0.0
    for t in range(ticks):
        sd, sh = pd.tick(), ph.tick(host_glue=True)
        e = {"x": rel_cols(pd.x, ph.x, 1e-3), "x_prev": rel_cols(pd.x_prev, ph.x_prev, 1e-3), "c_prev": rel_cols(pd.c_prev, ph.c_prev, 1e-3),
             "ik": rel_cols(pd.ik, ph.ik, 1.0), "torques": rel_cols(pd.torques, ph.torques, 1.0), "forces": rel_cols(pd.forces, ph.forces, 1.0)}
        assert max(e.values()) < tol, "tick %d: %s" % (t, e)
        assert [i.iters for i in pd.qp.last_info] == [i.iters for i in ph.qp.last_info]
        assert [s.num_iters for s in sd] == [s.num_iters for s in sh]
        worst = max(worst, max(e.values()))
    return worst


@pytest.mark.gpu
def test_device_loop_equals_host_glue_on_the_device(hip_lib):
    """The three glue kernels (csrc/pipeline_ikid_glue.h) against the numpy glue around the same library calls, 8 periods: states, the states and
    centroidal states before the last period, task errors, torques and forces within 1e-9, equal QP and MPC iteration counts."""
    print("HIP: centroidal device loop against host glue over 8 periods: %.3e" % _device_vs_host(hip_lib, 8, 1e-9))


@pytest.mark.gpu
def test_centroidal_pipeline_hip_matches_oracle(hip_lib, oracle_lib):
    """Eight MPC periods of two perturbed robots from the same cold-solved state: the HIP pipeline (device loop) against the oracle pipeline (host
    glue), tick by tick — the kinodynamic pipeline test's tolerances: states 1e-6, torques and forces 1e-5 (rel_cols with floors 1e-3 / 1)."""
    ph, po = centroidal_pipeline(hip_lib, walk={}), centroidal_pipeline(oracle_lib, walk={})
    ph.mpc.native.set_state(po.mpc.native.get_state())
    ph._fetch()
    worst = 0.0
    for t in range(8):
        ph.tick(), po.tick(host_glue=True)
        ex = rel_cols(ph.x, po.x, 1e-3)
        et = rel_cols(ph.torques, po.torques, 1.0)
        ef = rel_cols(ph.forces, po.forces, 1.0)
        assert ex < 1e-6 and et < 1e-5 and ef < 1e-5, "tick %d: states %.2e torques %.2e forces %.2e" % (t, ex, et, ef)
        worst = max(worst, ex, et, ef)
    print("centroidal pipeline: worst deviation over 8 ticks %.3e" % worst)


@pytest.mark.gpu
def test_device_loop_rejects_mismatches(hip_lib):
    p = centroidal_pipeline(hip_lib)
    q = p.qp
    refs = p.foot_refs()

    def call(plan=None, sim=None, frames=None, steps=1, x_ik=p.x):
        fr = q._frame_idx if frames is None else frames
        return q.qp.ikid_low_level_steps(plan or p.mpc.native, sim or p.sim, fr, q._base_idx, q._torso_idx, q.weights, q._gains, q.Cmin, q.l_box, q.u_box,
                                         p.x_posture, refs, p.ref_dt, np.ones((2, len(fr)), dtype=np.int32), steps, 1e-3, x=p.x, x_ik=x_ik)
    with pytest.raises(RuntimeError, match="no earlier call kept"):
        call(x_ik=None)
    with pytest.raises(RuntimeError, match="positive"):
        call(steps=0)
    with pytest.raises(RuntimeError, match="two contacts"):
        call(frames=np.array(list(q._frame_idx) + [q._base_idx], dtype=np.int32))
    with pytest.raises(RuntimeError, match="centroidal problem"):
        call(plan=p.sim)
    with pytest.raises(RuntimeError, match="simulator handle"):
        call(sim=p.mpc.native)
    other = CentroidalPipeline(CentroidalProblem(horizon=20), batch=3, library=hip_lib)
    with pytest.raises(RuntimeError, match="same batch size"):
        call(sim=other.sim)
    p.mpc.step_async()
    with pytest.raises(RuntimeError, match="in flight"):
        call()
    p.mpc.wait()
    call()  # (and the handles still work)


@pytest.mark.gpu
def test_centroidal_pipeline_walks_through_a_step(hip_lib):
    """64 robots (the bench ensemble), horizon 100, the script's walk: 205 MPC periods = 2 050 IK + ID QPs and simulator steps, through the take-off of
    the right foot (period 120) and its landing (period 200).  Nobody falls (base height within 5e-2 of the start), no QP factorisation fails."""
    p = CentroidalPipeline(CentroidalProblem(horizon=100), batch=64, library=hip_lib, walk={}, sigma_q=0.005, sigma_v=0.01, tick_reuse=True)
    p.mpc.prepare_schedule(210)
    p.cold_solve()
    z0 = p.x[:, 2].copy()
    seen = set()
    for t in range(205):
        p.tick()
        seen.add(tuple(p.contact_state()))
        assert all(i.status != 2 for i in p.qp.last_info), t
        assert np.all(np.abs(p.x[:, 2] - z0) < 5e-2), (t, np.max(np.abs(p.x[:, 2] - z0)))
    assert (True, False) in seen and list(p.contact_state()) == [True, True]
    print("centroidal walk, 64 robots: base height change %.2e .. %.2e" % (np.min(p.x[:, 2] - z0), np.max(p.x[:, 2] - z0)))
