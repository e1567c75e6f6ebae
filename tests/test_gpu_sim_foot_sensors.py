"""The per-robot foot force sensors and contact detector of the torque-driven simulator on the device (include/mpc_sim_foot_sensors.h:
mpc_sim_foot_sensors, mpc_sim_foot_sensors_feed; csrc/sim_foot_sensors.h k_sim_foot_sensors) against their numpy definition
(mpc_benchmark_amd/foot_sensors.py): off and unconsumed mean unchanged bits, the kernel against the mirror, the two consumers of the detected pair
(the base-state estimator, the low-level QPs), robots independent of their place in the batch, the state rows travel, re-arming and dropping, the
checks."""
import ctypes as C

import numpy as np
import pytest

from mpc_benchmark_amd import contact_rule as cr
from mpc_benchmark_amd import foot_sensors as fs
from mpc_benchmark_amd import state_estimator as se
from tests._metrics import rel_cols
from tests.test_centroidal_pipeline import centroidal_pipeline
from tests.test_fulldynamic_pipeline import fulldynamic_pipeline
from tests.test_gpu_qp_contact_source import SCHED, _one_step
from tests.test_gpu_sim_contacts import _batch_lift, _kino
from tests.test_gpu_sim_estimator import _compare
from tests.test_gpu_sim_push import DT, _sim
from tests.test_gpu_sim_sensors import _second

B = 4
PIPELINES = {"kinodynamic": lambda lib, **kw: _kino(lib, 2, **kw), "centroidal": lambda lib, **kw: centroidal_pipeline(lib, walk={}, **kw),
             "fulldynamic": lambda lib, **kw: fulldynamic_pipeline(lib, walk={}, **kw)}
QP_PIPELINES = {"kinodynamic": lambda lib, **kw: _kino(lib, B, horizon=20, **kw),
                "centroidal": lambda lib, **kw: centroidal_pipeline(lib, batch=B, horizon=20, walk={}, **kw)}


def _rows(batch):
    """the four kinds of row, robot b of kind b % 4: exact | noise and offsets | delay 3 with a low-pass | debounce of 3 with hysteresis"""
    k = np.arange(batch) % 4
    return fs.rows({"delay": 3.0 * (k == 2), "sigma_f": 2.0 * (k == 1), "sigma_m": 0.1 * (k == 1), "bias_f": 3.0 * (k == 1), "bias_m": 0.2 * (k == 1),
                    "time_constant": 0.004 * (k == 2), "f_on": np.choose(k, [10.0, 40.0, 10.0, 60.0]), "f_off": np.choose(k, [10.0, 15.0, 10.0, 20.0]),
                    "on_steps": 1.0 + 2.0 * (k == 3), "off_steps": 1.0 + 2.0 * (k == 3), "seed": 5.0 + np.arange(batch)}, batch)


def _rule(sim, rb):
    """the contact rule on, the ground at the lower initial foothold"""
    sim.contacts(cr.config({}, ground_z=min(float(M.translation[2]) for M in rb.foot_placements)))


def _scenario(sim, rb, Bk, steps, each):
    """the release-and-catch scenario of tests/test_gpu_sim_contacts.py: Bk robots from the initial state, each its own right-leg pulse; ``each(k, x,
    wr)`` after every step with the new true states and the step's wrenches -> the final states"""
    m = rb.model
    x = np.tile(rb.x0, (Bk, 1))
    amps, spans = 120.0 + 10.0 * np.arange(Bk), 12 + np.arange(Bk) % 4
    q0 = rb.x0[:m.nq].copy()
    for k in range(steps):
        x, wr = sim.simulate_torque(x, _batch_lift(m, q0, x, k, amps, spans), 1, DT, wrenches=True)
        each(k, x, wr)
    return x


def _margins(state, rows, wr, dt):
    """|z - threshold| of the event the mirror is about to run, per robot and sole (the threshold the sole's decision is taken against): computed
    on a copy of the mirror's rows"""
    trial = state.copy()
    det0 = fs.unpack(state)["det"].copy()
    fs.detect(trial, rows, wr, dt, np.ones((state.shape[0], 2)))
    z = fs.unpack(trial)["wf"][:, [2, 8]]
    thr = np.where(det0 != 0.0, rows[:, fs.P_F_OFF, None], rows[:, fs.P_F_ON, None])
    return np.abs(z - thr)


@pytest.mark.gpu
def test_off_and_unconsumed_mean_unchanged_in_simulate_torque(hip_lib):
    """the contact rule on everywhere; a handle that never armed the model, one that armed it and turned it off, one armed with noisy rows and mask 0,
    one with the estimator also on and mask 0: the same states and wrenches, bit for bit, over 3 steps"""
    rb, a, x, tau = _sim(hip_lib, batch=B)
    handles = [a] + [_sim(hip_lib, batch=B)[1] for _ in range(3)]
    for h in handles:
        _rule(h, rb)
    handles[1].foot_sensors(_rows(B))
    handles[1].foot_sensors(None)
    handles[2].foot_sensors(_rows(B))
    handles[3].foot_sensors(_rows(B))
    handles[3].foot_sensors_feed(())
    handles[3].estimator({"w_p": 0.9, "w_v": 1.0}, x)
    xs = [x] * 4
    for k in range(3):
        got = [h.simulate_torque(xi, tau * (1.0 + k), 1, DT, wrenches=True) for h, xi in zip(handles, xs)]
        for g in got[1:]:
            assert np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1]), k
        xs = [g[0] for g in got]
    with pytest.raises(RuntimeError, match="off"):
        handles[1].read_foot_sensors()
    r = handles[2].read_foot_sensors()
    assert np.array_equal(r["count"], np.full(B, 3.0)) and np.array_equal(r["ring"][:, 3], got[0][1].reshape(B, 12))
    assert np.array_equal(handles[2].read_foot_sensors(raw=True), handles[3].read_foot_sensors(raw=True))
    # a step that did not ask for the wrenches feeds the detector the same ones
    for h in handles[2:]:
        h.simulate_torque(xs[0], tau, 1, DT)
    want = handles[0].simulate_torque(xs[0], tau, 1, DT, wrenches=True)[1]
    assert np.array_equal(handles[2].read_foot_sensors()["ring"][:, 4], want.reshape(B, 12))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PIPELINES))
def test_off_and_unconsumed_mean_unchanged_in_the_pipelines(hip_lib, name):
    """the same four for 3 ticks of a pipeline with the contact rule: x, torques, forces (full dynamics: wrenches) and x_prev.  The estimator of the
    fourth has identity rows: what it reads from the contact rows does not reach the state then, and mask 0 keeps it on the rule's rows anyway."""
    pa, pb, pc, pd = (PIPELINES[name](hip_lib, contact_rule={}) for _ in range(4))
    pb.set_foot_sensors(_rows(pb.batch))
    pb.set_foot_sensors(None)
    pc.set_foot_sensors(_rows(pc.batch))
    pd.set_foot_sensors(_rows(pd.batch), ())
    pd.set_estimator(se.IDENTITY)
    for t in range(3):
        pa.tick(), pb.tick(), pc.tick(), pd.tick()
        for p in (pb, pc, pd):
            assert np.array_equal(pa.x, p.x) and np.array_equal(pa.torques, p.torques) and np.array_equal(_second(pa), _second(p)), t
            assert np.array_equal(pa.x_prev, p.x_prev), t
    assert np.array_equal(pc.sim.read_foot_sensors()["count"], np.full(pc.batch, 3.0 * pc.substeps))
    assert np.array_equal(pc.detected, pc.sim.read_foot_sensors()["det"]) and np.array_equal(pb.detected, pb.sim.read_contacts()["in_contact"])
    with pytest.raises(RuntimeError, match="off"):
        pb.sim.read_foot_sensors()


@pytest.mark.gpu
def test_kernel_equals_mirror(hip_lib):
    """The 70-step scenario of tests/test_gpu_sim_contacts.py test_kernel_equals_the_mirror: 8 robots, each its own right-leg pulse, released and caught.
    Rows exact | noise and offsets | delay 3 with a low-pass | debounce of 3 with hysteresis.  The mirror is fed the device's own wrenches
    (``simulate_torque(..., wrenches=True)``), the step length and ``read_contacts()["in_contact"]`` and is never re-synchronised.  After every step
    det, above, below, head, count and counts are equal exactly; wm, wf and the ring within 1e-12 of the largest |wrench entry| seen so far (floor
    1: the bound tests/test_gpu_sim_sensors.py holds its noise to: the normals differ by a few ulp between numpy and the device).  On every step, for
    every robot and sole, the mirror's z is further than 1e-6 N from the threshold it is compared with — a condition on the inputs, asserted: a
    last-bit difference cannot flip a decision.  Every right sole of the exact rows is released and detected again at least once.
    Measured over the 70 steps: wm 3.1e-18, wf 1.2e-16, ring 0 of the largest wrench entry (2297 N); the smallest |z - threshold| 0.12 N; the
    right soles are lifted and caught 1 to 4 times, and the delayed and debounced rows miss the plant's contact on 8 to 21 of the 70 steps."""
    Bk = 8
    rb, sim, _, _ = _sim(hip_lib, batch=Bk)
    _rule(sim, rb)
    rows = _rows(Bk)
    sim.foot_sensors(rows)
    c0 = sim.read_contacts()["in_contact"]
    state = fs.reset(c0)
    r0 = sim.read_foot_sensors()
    assert np.array_equal(r0["params"], rows) and np.array_equal(sim.read_foot_sensors(raw=True), state) and np.array_equal(r0["det"], c0)
    seen = {"scale": 1.0, "worst": np.zeros(3), "margin": np.inf, "dets": []}

    def each(k, x, wr):
        t = sim.read_contacts()["in_contact"]
        seen["scale"] = max(seen["scale"], np.max(np.abs(wr)))
        mg = _margins(state, rows, wr, DT)
        seen["margin"] = min(seen["margin"], np.min(mg))
        assert np.all(mg > 1e-6), (k, mg)
        det = fs.detect(state, rows, wr, DT, t)
        got, want = sim.read_foot_sensors(), fs.unpack(state)
        for f in ("det", "above", "below", "head", "count", "counts"):
            assert np.array_equal(got[f], want[f]), (k, f, got[f], want[f])
        assert np.array_equal(got["det"], det)
        e = np.array([np.max(np.abs(got[f] - want[f])) for f in ("wm", "wf", "ring")])
        seen["worst"] = np.maximum(seen["worst"], e / seen["scale"])
        assert np.all(e <= 1e-12 * seen["scale"]), (k, e, seen["scale"])
        seen["dets"].append(det.copy())

    _scenario(sim, rb, Bk, 70, each)
    dets = np.array(seen["dets"])                                              # (70, Bk, 2)
    con, got = sim.read_contacts(), sim.read_foot_sensors()
    print("foot sensors kernel against the mirror over 70 steps: wm %.1e wf %.1e ring %.1e of the largest wrench entry (%.0f); smallest "
          "|z - threshold| %.2e N; right-sole confusion counts per robot %s; lift-offs %s touchdowns %s"
          % (*seen["worst"], seen["scale"], seen["margin"], got["counts"][:, 1].astype(int).tolist(), con["liftoffs"][:, 1], con["touchdowns"][:, 1]))
    for b in (0, 4):                                                           # the exact rows: released and detected again
        d = dets[:, b, 1]
        first_off = int(np.argmax(d == 0.0))
        assert d[first_off] == 0.0 and np.any(d[first_off:] == 1.0), (b, d)
    assert np.array_equal(got["count"], np.full(Bk, 70.0)) and np.array_equal(got["head"], np.full(Bk, 70.0 % 16))
    assert np.all(got["counts"].sum(axis=2) == 70.0)
    assert np.any(got["counts"][[2, 3, 6, 7]][:, 1, 1:3] > 0)                  # (latency and debounce disagree with the plant somewhere)
    assert np.max(np.abs(got["wm"][1::4] - got["ring"][1::4, 70 % 16])) > 0.1  # (the noise acts)


@pytest.mark.gpu
def test_the_estimator_reads_the_detected_pair(hip_lib):
    """Bit 0 of the feed, over the same scenario: the estimator's rows equal ``state_estimator.estimate`` fed with the detector's ``det`` pair as this
    step's detection event left it, within the bounds of tests/test_gpu_sim_estimator.py (held and count exactly, anchors and base position 1e-12,
    ...); and on at least one step those rows differ from a mirror fed with the rule's pair: a feed that still read the truth would pass otherwise.
    Measured: anchors 4.4e-16, base position 6.7e-16, base velocity 2.4e-16 of the largest entry, statistics 1.1e-15 of theirs; the held pair is
    another than the rule's on 35 of the 70 steps."""
    Bk = 8
    rb, sim, _, _ = _sim(hip_lib, batch=Bk)
    m, fids, nq = rb.model, list(rb.foot_frame_ids), rb.model.nq
    x0 = np.tile(rb.x0, (Bk, 1))
    _rule(sim, rb)
    sim.foot_sensors(_rows(Bk))
    sim.foot_sensors_feed(("estimator",))
    erows = se.rows({"w_p": 0.9, "w_v": 1.0}, Bk)
    sim.estimator(erows, x0)
    c0 = sim.read_contacts()["in_contact"]
    fed, truth = se.reset(erows, x0, c0, m, fids), se.reset(erows, x0, c0, m, fids)
    seen = {"worst": np.zeros(4), "scale": 1.0, "differ": 0}

    def each(k, x, wr):
        det, t = sim.read_foot_sensors()["det"], sim.read_contacts()["in_contact"]
        se.estimate(fed, erows, x, det, x, m, fids)
        se.estimate(truth, erows, x, t, x, m, fids)
        seen["scale"] = max(seen["scale"], np.max(np.abs(x)))
        got = sim.read_estimator()
        seen["worst"] = np.maximum(seen["worst"], _compare(got, se.unpack(fed, m.nv), seen["scale"], nq, "step %d" % k))
        seen["differ"] += int(not np.array_equal(got["held"], se.unpack(truth, m.nv)["held"]))

    _scenario(sim, rb, Bk, 70, each)
    print("estimator fed by detection against the mirror: anchors %.1e, base position %.1e, base velocity %.1e, statistics %.1e; steps with a held "
          "pair other than the rule's: %d" % (*seen["worst"], seen["differ"]))
    assert seen["differ"] >= 1
    assert np.max(np.abs(se.unpack(fed, m.nv)["est"] - se.unpack(truth, m.nv)["est"])) > 1e-9   # (and the estimate itself went another way)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(QP_PIPELINES))
def test_the_qps_read_the_detected_pair(hip_lib, name):
    """Bit 1 of the feed, contact_source="plant".  One step of the device loop with detector rows imposed whose pairs differ from the rule's (which
    holds both soles of every robot): ``used`` and the counts are the mirror's selection from ``det``, not from the truth.  Then 3 periods of a device
    tick against the host-glue tick, which reads the detector rows back before each step, in x, x_prev, torques and forces (rel_cols, floors 1e-3 /
    1) within the 1e-9 tests/test_gpu_qp_contact_source.py test_device_loop_equals_host_glue holds the pair to; the same ``used`` and counts.  Robot
    1's thresholds are out of reach (1e4 N), so its detector keeps one sole by the never-empty rule and its QP works with one contact while the
    plant holds two.  Measured, per period: kinodynamic 3.7e-14 4.4e-14 1.2e-10, centroidal 7.8e-14 6.4e-14 8.5e-14."""
    det = np.array([[1, 1], [1, 1], [1, 0], [0, 1]], dtype=float)
    frows = fs.rows({"delay": [0, 0, 0, 3.0], "sigma_f": [0, 0, 0, 5.0], "f_on": [10.0, 1e4, 10.0, 10.0], "f_off": [10.0, 1e4, 10.0, 10.0],
                     "seed": 3.0 + np.arange(B)}, B)
    make = lambda: QP_PIPELINES[name](hip_lib, contact_rule={}, contact_source="plant", foot_sensors=frows, detected_contacts=("qp",))
    p = make()
    assert np.all(p.sim.read_contacts()["in_contact"] == 1.0) and np.array_equal(p.detected, np.ones((B, 2)))
    rows = p.sim.read_foot_sensors(raw=True)
    rows[:, :2] = det
    p.sim.set_foot_sensors(rows)
    p.qp.qp.contact_source("plant")
    kw = dict(x_ik=p.x_prev.copy(), refs=p.foot_refs()) if name == "centroidal" else {}
    _one_step(p, SCHED, p.x.copy(), **kw)
    r = p.qp.qp.read_contact_source()
    np.testing.assert_array_equal(r["used"], cr.qp_contact_states("plant", SCHED, det.astype(np.int32)))
    np.testing.assert_array_equal(r["counts"], cr.qp_contact_counts(None, SCHED, det.astype(np.int32)))
    assert np.any(r["used"] != cr.qp_contact_states("plant", SCHED, np.ones((B, 2), dtype=np.int32)))
    pl, ph = make(), make()
    worst = []
    for t in range(3):
        pl.tick()
        ph.tick(host_glue=True)
        worst.append(max(rel_cols(pl.x, ph.x, 1e-3), rel_cols(pl.x_prev, ph.x_prev, 1e-3), rel_cols(pl.torques, ph.torques, 1.0),
                         rel_cols(pl.forces, ph.forces, 1.0)))
        ql, qh = pl.qp_contacts(), ph.qp_contacts()
        np.testing.assert_array_equal(ql["used"], qh["used"], err_msg="period %d" % t)
        np.testing.assert_array_equal(ql["counts"], qh["counts"], err_msg="period %d" % t)
        np.testing.assert_array_equal(pl.detected, ph.detected, err_msg="period %d" % t)
    print("%s, QPs fed by detection: device loop against host glue per period %s; used %s; detected %s; in_contact %s"
          % (name, " ".join("%.1e" % w for w in worst), ql["used"].tolist(), pl.detected.tolist(), pl.sim.read_contacts()["in_contact"].tolist()))
    assert max(worst) <= 1e-9, worst
    assert ql["used"][1].sum() == 1 and np.all(pl.sim.read_contacts()["in_contact"][1] == 1.0)   # (robot 1: one contact detected, two held)
    assert np.all(ql["counts"].sum(axis=2) == 3 * pl.substeps)


@pytest.mark.gpu
def test_place_in_the_batch(hip_lib):
    """a batch with its robots permuted gives the permuted rows bit for bit (20 steps of the scenario: the ring wraps, every kind of row)"""
    Bk = 4
    perm = np.array([2, 0, 3, 1])
    rb, a, _, _ = _sim(hip_lib, batch=Bk)
    b = _sim(hip_lib, batch=Bk)[1]
    rows = _rows(Bk)
    m, q0 = rb.model, rb.x0[:rb.model.nq].copy()
    amps, spans = 120.0 + 10.0 * np.arange(Bk), 12 + np.arange(Bk) % 4
    for h, o in ((a, np.arange(Bk)), (b, perm)):
        _rule(h, rb)
        h.foot_sensors(rows[o])
        x = np.tile(rb.x0, (Bk, 1))
        for k in range(20):
            x = h.simulate_torque(x, _batch_lift(m, q0, x, k, amps[o], spans[o]), 1, DT)
    ra, rbb = a.read_foot_sensors(raw=True), b.read_foot_sensors(raw=True)
    assert np.array_equal(rbb, ra[perm])
    assert np.array_equal(fs.unpack(ra)["count"], np.full(Bk, 20.0)) and np.any(fs.unpack(ra)["wm"][1] != fs.unpack(ra)["ring"][1, 4])


@pytest.mark.gpu
def test_state_rows_travel(hip_lib):
    """12 steps of the scenario, read; a fresh handle takes the rule's rows, then the detector's; 5 more steps on both give the same bits (delay line,
    filter state, counters and counts included).  Malformed rows are rejected and the rows in force stay."""
    Bk = 4
    rb, a, _, _ = _sim(hip_lib, batch=Bk)
    b = _sim(hip_lib, batch=Bk)[1]
    rows = _rows(Bk)
    m, q0 = rb.model, rb.x0[:rb.model.nq].copy()
    amps, spans = 120.0 + 10.0 * np.arange(Bk), 12 + np.arange(Bk) % 4
    _rule(a, rb), _rule(b, rb)
    a.foot_sensors(rows)
    x = np.tile(rb.x0, (Bk, 1))
    for k in range(12):
        x = a.simulate_torque(x, _batch_lift(m, q0, x, k, amps, spans), 1, DT)
    held = a.read_foot_sensors(raw=True)
    assert held.shape == (Bk, fs.WIDTH)
    b.foot_sensors(rows)
    b.set_contacts(a.read_contacts(raw=True))                                 # (arms the detector again ...)
    assert not np.array_equal(b.read_foot_sensors(raw=True), held)
    b.set_foot_sensors(held)                                                   # (... so the detector's rows go last)
    assert np.array_equal(b.read_foot_sensors(raw=True), held)
    xa = xb = x
    for k in range(12, 17):
        xa = a.simulate_torque(xa, _batch_lift(m, q0, xa, k, amps, spans), 1, DT)
        xb = b.simulate_torque(xb, _batch_lift(m, q0, xb, k, amps, spans), 1, DT)
    assert np.array_equal(xa, xb) and np.array_equal(a.read_foot_sensors(raw=True), b.read_foot_sensors(raw=True))
    assert not np.array_equal(a.read_foot_sensors(raw=True), held)
    held = b.read_foot_sensors(raw=True)
    for col, val, match in ((7, np.nan, "finite"), (fs.O_RING + 5, np.inf, "finite"), (0, 0.5, "det"), (1, 2.0, "det"), (fs.O_ABOVE, -1.0, "above"),
                            (fs.O_BELOW + 1, -1.0, "below"), (fs.O_COUNTS + 3, -1.0, "counts"), (fs.O_HEAD, 16.0, "head"), (fs.O_HEAD, 1.5, "head"),
                            (fs.O_COUNT, -1.0, "count")):
        bad = held.copy()
        bad[2, col] = val
        with pytest.raises(RuntimeError, match=match):
            b.set_foot_sensors(bad)
        assert np.array_equal(b.read_foot_sensors(raw=True), held)
    bad = held.copy()
    bad[1, :2] = 0.0
    with pytest.raises(RuntimeError, match="no sole detected"):
        b.set_foot_sensors(bad)
    with pytest.raises(ValueError, match="shape"):
        b.set_foot_sensors(held[:, :-1])


@pytest.mark.gpu
def test_rearming_and_dropping(hip_lib):
    """a reset of the rule's rows (mpc_sim_contacts with a configuration) and rows imposed (mpc_sim_contacts_set) arm the detector again, on the new
    in_contact pairs; turning the rule off drops the detector and clears the mask: the rule back on brings neither back, and a detector armed
    afterwards feeds nobody."""
    rb, sim, x, tau = _sim(hip_lib, batch=B)
    _rule(sim, rb)
    out_of_reach = fs.rows({"f_on": 1e4, "f_off": 1e4}, B)                    # (every robot keeps one sole by the never-empty rule)
    sim.foot_sensors(out_of_reach)
    sim.foot_sensors_feed(("estimator", "qp"))
    for k in range(3):
        x = sim.simulate_torque(x, tau, 1, DT)
    r = sim.read_foot_sensors()
    assert np.array_equal(r["count"], np.full(B, 3.0)) and np.all(r["det"].sum(axis=1) == 1.0) and np.all(sim.read_contacts()["in_contact"] == 1.0)
    _rule(sim, rb)                                                             # a reset of the rule: armed again
    assert np.array_equal(sim.read_foot_sensors(raw=True), fs.reset(np.ones((B, 2))))
    assert np.array_equal(sim.read_foot_sensors()["params"], out_of_reach)
    x = sim.simulate_torque(x, tau, 1, DT)
    rows = sim.read_contacts(raw=True)
    pairs = np.array([[1, 0], [0, 1], [1, 1], [1, 0]], dtype=float)
    rows[:, cr.O_IN:cr.O_IN + 2] = pairs
    sim.set_contacts(rows)                                                     # rows imposed: armed again, on them
    assert np.array_equal(sim.read_foot_sensors(raw=True), fs.reset(pairs))
    # the mask survived both (sticky): the estimator's arming event latches the detected pair, not the rule's ...
    det = pairs.copy()
    det[2] = [0, 1]
    imposed = fs.reset(det)
    sim.set_foot_sensors(imposed)
    sim.estimator({"w_p": 1.0}, x)
    assert np.array_equal(sim.read_estimator()["held"], det) and not np.array_equal(det, sim.read_contacts()["in_contact"])
    # ... the rule off: the detector and the mask go with it
    sim.contacts(None)
    with pytest.raises(RuntimeError, match="off"):
        sim.read_foot_sensors()
    with pytest.raises(RuntimeError, match="off"):
        sim.foot_sensors_feed(("estimator",))
    _rule(sim, rb)
    with pytest.raises(RuntimeError, match="off"):
        sim.read_foot_sensors()
    sim.foot_sensors(out_of_reach)                                             # armed afterwards: mask 0 again
    sim.set_foot_sensors(fs.reset(det))
    sim.estimator({"w_p": 1.0}, x)
    assert np.array_equal(sim.read_estimator()["held"], sim.read_contacts()["in_contact"]) and np.all(sim.read_estimator()["held"] == 1.0)
    sim.simulate_torque(x, tau, 1, DT)


@pytest.mark.gpu
def test_errors(hip_lib):
    """every refusal of the parameter table, the feed while off, an unknown bit, arming without the rule, a handle of the wrong kind, read and set
    while off: -1 with a message, the configuration in force unchanged"""
    rb, sim, x, tau = _sim(hip_lib, batch=B)
    dp = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(C.c_double))
    rows = _rows(B)
    for call in (lambda: sim.read_foot_sensors(), lambda: sim.set_foot_sensors(np.zeros((B, fs.WIDTH))), lambda: sim.foot_sensors_feed(("qp",)),
                 lambda: sim.foot_sensors_feed(0)):
        with pytest.raises(RuntimeError, match="off"):
            call()
    sim.foot_sensors(None)   # (off while off: nothing to do)
    with pytest.raises(RuntimeError, match="contact rule is off on this handle .turn it on with mpc_sim_contacts first."):
        sim.foot_sensors(rows)
    with pytest.raises(RuntimeError, match="off"):
        sim.read_foot_sensors()
    _rule(sim, rb)
    sim.foot_sensors(rows)
    sim.foot_sensors_feed(("estimator",))
    for k in range(2):
        x = sim.simulate_torque(x, tau, 1, DT)
    held = sim.read_foot_sensors()
    unchanged = lambda: all(np.array_equal(sim.read_foot_sensors()[k], held[k]) for k in held)
    for fields, match in (({"delay": -1.0}, "delay"), ({"delay": 16.0}, "delay"), ({"delay": 0.5}, "delay"), ({"sigma_f": -1.0}, ">= 0"),
                          ({"sigma_m": -1.0}, ">= 0"), ({"bias_f": -1.0}, ">= 0"), ({"bias_m": -1.0}, ">= 0"), ({"time_constant": -1.0}, ">= 0"),
                          ({"f_on": 5.0, "f_off": 6.0}, "f_off"), ({"f_on": np.inf}, "finite"), ({"f_off": -np.inf}, "finite"),
                          ({"f_on": np.nan}, "finite"), ({"on_steps": 0.0}, "on_steps"), ({"on_steps": 1.5}, "on_steps"), ({"off_steps": 0.0}, "off_steps"),
                          ({"off_steps": 2.5}, "off_steps"), ({"seed": -1.0}, "seed"), ({"seed": 2.0 ** 32}, "seed"), ({"seed": 0.5}, "seed")):
        bad = fs.rows({}, B)
        for k, v in fields.items():
            bad[B - 1, fs.FIELDS.index(k)] = v                                 # (the last row is the bad one)
        with pytest.raises(ValueError):
            fs.validate(bad)                                                   # (the mirror refuses what the library refuses)
        rc = hip_lib.mpc_sim_foot_sensors(sim._h, dp(bad))
        msg = hip_lib.mpc_last_error(sim._h).decode()
        assert rc == -1 and match in msg and "row %d" % (B - 1) in msg, (fields, rc, msg)
        assert unchanged(), fields
    bad = rows.copy()
    bad[1, 12] = 1.0
    assert hip_lib.mpc_sim_foot_sensors(sim._h, dp(bad)) == -1 and "reserved" in hip_lib.mpc_last_error(sim._h).decode() and unchanged()
    for mask in (4, 7, -1, 1 << 16):
        assert hip_lib.mpc_sim_foot_sensors_feed(sim._h, mask) == -1 and "unknown consumer bit" in hip_lib.mpc_last_error(sim._h).decode(), mask
    with pytest.raises(ValueError, match="unknown consumers"):
        sim.foot_sensors_feed(("planner",))
    # ... and changed nothing: the estimator still reads the detected pair
    imposed = sim.read_foot_sensors(raw=True)
    imposed[:, :2] = [1.0, 0.0]
    sim.set_foot_sensors(imposed)
    sim.estimator({"w_p": 1.0}, x)
    assert np.array_equal(sim.read_estimator()["held"], np.tile([1.0, 0.0], (B, 1)))
    assert hip_lib.mpc_sim_foot_sensors_set(sim._h, None) == -1 and hip_lib.mpc_sim_foot_sensors_read(sim._h, None, None) == 0
    plan = centroidal_pipeline(hip_lib, walk={}).mpc.native
    assert hip_lib.mpc_sim_foot_sensors(plan._h, dp(fs.rows({}, plan.dims.batch))) == -1
    assert "simulator handle" in hip_lib.mpc_last_error(plan._h).decode()
    assert hip_lib.mpc_sim_foot_sensors_width(plan._h) == -1 and hip_lib.mpc_sim_foot_sensors_width(sim._h) == fs.WIDTH
    for call in (lambda: plan.foot_sensors(None), lambda: plan.read_foot_sensors(), lambda: plan.foot_sensors_feed(())):
        with pytest.raises(RuntimeError, match="simulator handle"):
            call()
    # the pipelines check their arguments before any library call
    from mpc_benchmark_amd.pipeline import FullDynamicPipeline, KinodynamicPipeline
    for cls, kw, match in ((KinodynamicPipeline, dict(foot_sensors={}), "needs contact_rule"),
                           (KinodynamicPipeline, dict(contact_rule={}, detected_contacts=("estimator",)), "needs foot_sensors"),
                           (KinodynamicPipeline, dict(contact_rule={}, foot_sensors={}, detected_contacts=("qp",)), "contact_source"),
                           (KinodynamicPipeline, dict(contact_rule={}, foot_sensors={}, detected_contacts=("planner",)), "unknown consumers"),
                           (FullDynamicPipeline, dict(contact_rule={}, foot_sensors={}, detected_contacts=("qp",)), "contact_source")):
        with pytest.raises(ValueError, match=match):
            cls(None, batch=2, library=hip_lib, **kw)
