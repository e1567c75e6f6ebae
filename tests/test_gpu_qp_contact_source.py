"""The contact source of the low-level QPs on the device (include/mpc_qp_contacts.h; csrc/pipeline_contacts.h k_pipe_contact_states, the `used` form of
the two torque kernels): the selection of one step of both device loops against the numpy mirror (mpc_benchmark_amd/contact_rule.py) and a cold QP
given the mirror's set, the rows a step reads, the device loops against their host glue for the three sources, the default untouched, and the error
paths."""
import numpy as np
import pytest

from mpc_benchmark_amd import contact_rule as cr
from mpc_benchmark_amd import qp_utils
from mpc_benchmark_amd.pipeline import CentroidalPipeline, centroidal_state, posture_gains
from mpc_benchmark_amd.problems import common
from mpc_benchmark_amd.robot import minipin as pin
from tests._metrics import rel_cols
from tests.test_centroidal_pipeline import centroidal_pipeline
from tests.test_gpu_sim_contacts import FLAGS, _kino

N = 20
SOURCES = ("schedule", "plant", "both")
# the four robots of the selection test: schedule pair ; plant pair
SCHED = np.array([[1, 1], [1, 0], [0, 1], [1, 0]], dtype=np.int32)
PLANT = np.array([[1, 1], [1, 1], [1, 0], [0, 1]], dtype=np.int32)


def _make(lib, name, batch, **kw):
    if name == "kinodynamic":
        return _kino(lib, batch, horizon=N, contact_rule={}, **kw)
    return centroidal_pipeline(lib, batch=batch, horizon=N, walk={}, contact_rule={}, **kw)


def _rows_with(p, in_contact, lifted=None):
    """the rows of the pipeline's rule with the in_contact (and lifted) pairs replaced"""
    rows = p.sim.read_contacts(raw=True)
    rows[:, cr.O_IN:cr.O_IN + 2] = in_contact
    if lifted is not None:
        rows[:, cr.O_LIFTED:cr.O_LIFTED + 2] = lifted
    return rows


def _cold_qp(p, lib):
    """a second QP handle of the pipeline's QP, never solved on"""
    m, rb = p.model, p.pd.robot
    if isinstance(p, CentroidalPipeline):
        gains = [posture_gains(m.nv), (np.eye(6) * p.G_FOOT, np.eye(6) * 2 * np.sqrt(p.G_FOOT)), None, (np.eye(3) * p.G_ROT, np.eye(3) * 2 * np.sqrt(p.G_ROT))]
        qp = qp_utils.IKIDSolver_f6(m, list(p.WEIGHTS), gains, 2, common.FRICTION_MU, common.FOOT_HALF_LENGTH, common.FOOT_HALF_WIDTH, list(rb.foot_frame_ids),
                                    m.getFrameId("base_link"), m.getFrameId("torso_2_link"), 6, library=lib, batch=p.batch)
    else:
        qp = qp_utils.IDSolver_ulim(m, [1.0, 10000.0], 2, common.FRICTION_MU, common.FOOT_HALF_LENGTH, common.FOOT_HALF_WIDTH, list(rb.foot_frame_ids), 6,
                                    library=lib, batch=p.batch)
    qp.enable_device_assembly()
    return qp


def _one_step(p, sched, x0, x_ik=None, refs=None):
    """one step of the pipeline's device loop from x0 with a per-robot schedule -> torques, forces"""
    if isinstance(p, CentroidalPipeline):
        out = p.qp.low_level_steps(p.mpc.native, p.sim, p.x_posture, refs, p.ref_dt, sched, 1, p.sim_dt, x=x0, x_ik=x_ik)
        return out[3], out[4]
    out = p.qp.low_level_steps(p.mpc.native, p.sim, sched, p.umax, 1, p.sim_dt, x=x0)
    return out[2], out[3]


def _reference_step(p, ref, used, x0, x_ik=None, refs=None):
    """the same QP on the cold handle `ref`, the feedback terms from the host glue's formulas (KinodynamicPipeline / CentroidalPipeline.low_level_step)
    -> torques (clamped, kinodynamic), forces + df"""
    if isinstance(p, CentroidalPipeline):
        ik = p.qp.task_errors(x_ik, p.x_posture, refs, p.ref_dt, p.dH)
        new_x = centroidal_state(p.model, x0)
        forces = p.us0 - np.einsum("bij,bj->bi", p.K0, p.xs0 - new_x)
        _, f_new, tau = ref.solve_batch_device_ik(x0, ik, forces, used)
        return tau, f_new
    nq, nv = p.nq, p.nv
    d = np.concatenate([pin.difference_batch(p.model, x0[:, :nq], p.xs0[:, :nq]), p.xs0[:, nq:] - x0[:, nq:]], axis=1)
    a0 = p.xdot0[:, nv:].copy()
    a0[:, 6:] = p.us0[:, 12:] - np.einsum("bij,bj->bi", p.K0[:, 12:], d)
    forces = p.us0[:, :12] - np.einsum("bij,bj->bi", p.K0[:, :12], d)
    _, f_new, tau = ref.solve_batch_device(x0, a0, forces, used)
    return np.clip(tau, -p.umax, p.umax), f_new


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kinodynamic", "centroidal"])
def test_selection_of_one_step(hip_lib, name):
    """Four robots with (s; p) = (11; 11), (10; 11), (01; 10), (10; 01): for each source one step of the device loop from the same state.  `used` is the
    mirror's; torques and forces (zeros included) are those of a cold QP handle given the mirror's set, within the 1e-9 of the loop tests against
    host glue; and wherever `used` differs from the schedule pair the torque differs from the "schedule" run by more than 1e-6 (1000 times the
    comparison tolerance: a selection that did nothing cannot pass)."""
    B = 4
    p = _make(hip_lib, name, B)
    ref = _cold_qp(p, hip_lib)
    x0 = p.x.copy()
    kw = dict(x_ik=p.x_prev.copy(), refs=p.foot_refs()) if name == "centroidal" else {}
    rows = _rows_with(p, PLANT)
    got = {}
    for source in SOURCES:
        p.sim.set_contacts(rows)
        p.qp.qp.contact_source(source)
        tau, forces = _one_step(p, SCHED, x0, **kw)
        r = p.qp.qp.read_contact_source()
        used = cr.qp_contact_states(source, SCHED, PLANT)
        assert r["source"] == source
        np.testing.assert_array_equal(r["used"], used, err_msg=source)
        want_counts = cr.qp_contact_counts(None, SCHED, PLANT) if source != "schedule" else np.zeros((B, 2, 4), dtype=np.int32)
        np.testing.assert_array_equal(r["counts"], want_counts, err_msg=source)
        tau_ref, f_ref = _reference_step(p, ref, used, x0, **kw)
        if source != "schedule":
            f_ref = cr.qp_zero_unused(f_ref, used)
            assert np.all(forces.reshape(B, 2, 6)[used == 0] == 0.0), source
        et, ef = rel_cols(tau, tau_ref, 1.0), rel_cols(forces, f_ref, 1.0)
        print("%s, source %s: used %s ; torques %.2e forces %.2e against the cold QP given the mirror's set" % (name, source, used.tolist(), et, ef))
        assert et <= 1e-9 and ef <= 1e-9, (source, et, ef)
        got[source] = tau
    for source in ("plant", "both"):
        used = cr.qp_contact_states(source, SCHED, PLANT)
        changed = np.flatnonzero(np.any(used != SCHED, axis=1))
        assert changed.tolist() == ([1, 2, 3] if source == "plant" else [2, 3])
        diff = np.max(np.abs(got[source] - got["schedule"]), axis=1)
        print("%s, source %s: max |tau - tau(schedule)| per robot %s" % (name, source, " ".join("%.3e" % v for v in diff)))
        assert np.all(diff[changed] > 1e-6), (source, diff)


@pytest.mark.gpu
def test_a_step_reads_the_rows_the_step_before_left(hip_lib):
    """Two calls of one step with "both".  Robots 1 and 2 start with one sole free but marked lifted (the rule may catch it after the first step), and
    between the calls robot 0's left sole is taken out of its row: the rows R1 read between the calls differ from the rows R0 the first call started
    from.  `used` of the second call is the mirror on R1 (not R0), and the counts are the mirror's accumulation over R0 and then R1."""
    B = 4
    p = _make(hip_lib, "kinodynamic", B)
    sched = np.array([[1, 1], [1, 0], [1, 1], [0, 1]], dtype=np.int32)
    p0 = np.array([[1, 1], [1, 0], [0, 1], [1, 1]], dtype=np.int32)
    p.sim.set_contacts(_rows_with(p, p0, lifted=1 - p0))
    p.qp.qp.contact_source("both")
    _one_step(p, sched, p.x.copy())
    r = p.qp.qp.read_contact_source()
    np.testing.assert_array_equal(r["used"], cr.qp_contact_states("both", sched, p0))
    rows = p.sim.read_contacts(raw=True)
    rows[0, cr.O_IN] = 0.0
    p.sim.set_contacts(rows)
    p1 = p.sim.read_contacts()["in_contact"].astype(np.int32)
    print("in_contact before the first step %s, before the second %s" % (p0.tolist(), p1.tolist()))
    assert np.any(cr.qp_contact_states("both", sched, p1) != cr.qp_contact_states("both", sched, p0))
    _one_step(p, sched, None)
    r = p.qp.qp.read_contact_source()
    np.testing.assert_array_equal(r["used"], cr.qp_contact_states("both", sched, p1))
    np.testing.assert_array_equal(r["counts"], cr.qp_contact_counts(cr.qp_contact_counts(None, sched, p0), sched, p1))
    p.qp.qp.contact_source("both")   # (sticky, and the call zeroes the counts)
    assert not np.any(p.qp.qp.read_contact_source()["counts"])


@pytest.mark.gpu
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name", ["kinodynamic", "centroidal"])
def test_device_loop_equals_host_glue(hip_lib, name, source):
    """Batch 8, 6 periods, the robots standing in double support as in test_gpu_sim_contacts.test_device_loops_equal_host_glue_with_the_rule (whose
    1e-9 is the bound here: it is the bound of that situation, so nothing else is imposed on the plant): the device loop against the host glue (the rows
    read before every step, the mirror per robot), the same flags of the rule, the same qp_contacts().  Plan and plant are expected to agree on the steps of these
    periods, so the three sources select the same set: what differs between them is the path (the kernel, the schedule buffer, the `used` form of
    the torque kernels against the mirror on the host).  Sets that differ are test_selection_of_one_step and
    test_a_step_reads_the_rows_the_step_before_left."""
    B = 8
    pl, ph = _make(hip_lib, name, B, contact_source=source), _make(hip_lib, name, B, contact_source=source)
    worst = []
    for t in range(6):
        pl.tick()
        ph.tick(host_glue=True)
        e = max(rel_cols(pl.x, ph.x, 1e-3), rel_cols(pl.x_prev, ph.x_prev, 1e-3), rel_cols(pl.torques, ph.torques, 1.0), rel_cols(pl.forces, ph.forces, 1.0))
        worst.append(e)
        assert e <= 1e-9, (name, source, t, e)
        rl, rh = cr.unpack(pl.sim.read_contacts(raw=True)), cr.unpack(ph.sim.read_contacts(raw=True))
        for f in FLAGS:
            np.testing.assert_array_equal(rl[f], rh[f], err_msg="%s %s period %d %s" % (name, source, t, f))
        ql, qh = pl.qp_contacts(), ph.qp_contacts()
        np.testing.assert_array_equal(ql["used"], qh["used"], err_msg="%s %s period %d" % (name, source, t))
        np.testing.assert_array_equal(ql["counts"], qh["counts"], err_msg="%s %s period %d" % (name, source, t))
    print("%s, source %s: device loop vs host glue %s; counts summed over the robots %s" % (name, source, " ".join("%.1e" % w for w in worst),
                                                                                         ql["counts"].sum(axis=0).tolist()))
    assert ql["used"].shape == (B, 2) and ql["counts"].shape == (B, 2, 4)
    if source == "schedule":
        assert not np.any(ql["counts"])
    else:
        assert np.all(ql["counts"].sum(axis=2) == 6 * pl.substeps)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kinodynamic", "centroidal"])
def test_default_untouched(hip_lib, name):
    """contact_source="schedule" and no argument at all: bitwise equal states, torques, forces and rows of the rule over 3 periods"""
    pa, pb = _make(hip_lib, name, 4), _make(hip_lib, name, 4, contact_source="schedule")
    for t in range(3):
        pa.tick()
        pb.tick()
        assert np.array_equal(pa.x, pb.x) and np.array_equal(pa.x_prev, pb.x_prev) and np.array_equal(pa.torques, pb.torques), t
        assert np.array_equal(pa.forces, pb.forces), t
        np.testing.assert_array_equal(pa.sim.read_contacts(raw=True), pb.sim.read_contacts(raw=True))
    assert pa.contact_source == "schedule" and not np.any(pb.qp_contacts()["counts"])
    np.testing.assert_array_equal(pb.qp_contacts()["used"], np.ones((4, 2), dtype=np.int32))
    np.testing.assert_array_equal(pa.qp.qp.read_contact_source()["used"], np.ones((4, 2), dtype=np.int32))   # (the handle: the last QP's contact states)


@pytest.mark.gpu
def test_errors(hip_lib):
    p = _make(hip_lib, "kinodynamic", 2)
    c = _make(hip_lib, "centroidal", 2)
    qp = p.qp.qp
    with pytest.raises(ValueError, match="contact_source"):
        qp.contact_source("measured")
    assert hip_lib.mpc_qp_contact_source(qp._h, 7) == -1 and b"unknown source" in hip_lib.mpc_qp_last_error(qp._h)
    assert qp.read_contact_source()["source"] == "schedule"
    qp.contact_source("plant")
    assert hip_lib.mpc_qp_contact_source(qp._h, -1) == -1 and qp.read_contact_source()["source"] == "plant"   # (a refused value changes nothing)
    # nk != 2 is reachable through the binding of the kinodynamic loop
    with pytest.raises(RuntimeError, match="nk = 2"):
        qp.low_level_steps(p.mpc.native, p.sim, p.qp._frame_idx[:1], p.qp._weights, p.qp.Cmin, 1.0, np.ones((2, 1), dtype=np.int32), p.umax, 1, 1e-3, x=p.x)
    # a simulator without the rule
    cs = p.contact_state()
    x = p.x.copy()
    p.sim.contacts(None)
    with pytest.raises(RuntimeError, match="mpc_sim_contacts"):
        p.low_level_loop(cs)
    c.qp.qp.contact_source("both")
    c.sim.contacts(None)
    with pytest.raises(RuntimeError, match="mpc_sim_contacts"):
        c.low_level_loop(c.contact_state(), c.foot_refs())
    np.testing.assert_array_equal(p.x, x)   # (a refused call leaves the pipeline's state alone)
    qp.contact_source("schedule")            # ... and the schedule needs no rule
    p.low_level_loop(cs)
    assert np.all(np.isfinite(p.x))
