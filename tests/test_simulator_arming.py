"""The host side of the torque-driven simulator's models, pinned without a GPU: in which order the three pipelines and the headless BulletRobot arm
contact rule, terrain, plant, friction, actuators, sensors, foot sensors and estimator on their simulator handle, what arms again when a model
changes, what the controllers read when a model is off, and that the pipelines and BulletRobot upload the same tables for the same robot.  The
``NativeSolver`` methods of the models are replaced by recorders, so everything runs on the oracle; the kernels behind them are held to their numpy
mirrors in the tests/test_gpu_sim_*.py files.  The expected sequences were taken from the code before the arming rules were written once
(mpc_benchmark_amd/torque_simulator.py); one difference is permitted and stated where it applies: BulletRobot may arm the sensors before the foot
sensors, as the pipelines do (the two calls are independent: mpc_sim_sensors reads x0 and writes the sensor rows, mpc_sim_foot_sensors reads the
contact rows and writes the detector rows, and both come before the estimator either way)."""
import numpy as np
import pytest

from mpc_benchmark_amd import _capi
from mpc_benchmark_amd.bullet_robot import BulletRobot
from mpc_benchmark_amd.pipeline import CentroidalPipeline, FullDynamicPipeline, KinodynamicPipeline
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.common import Robot
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem

MODELS = ("contacts", "terrain", "plant", "friction", "actuators", "sensors", "foot_sensors", "foot_sensors_feed", "estimator")
X_SENSED, X_ESTIMATED = 7.0, 9.0     # what the recorders' read_sensors / read_estimator deliver
ON, OFF = False, True                # the ``turned_off`` flag of a recorded call
PIPELINE_ORDER = [(n, ON) for n in MODELS]
BULLET_ORDER = [(n, ON) for n in ("contacts", "plant", "friction", "actuators", "foot_sensors", "foot_sensors_feed", "sensors", "estimator")]
BULLET_ORDER_UNIFIED = [(n, ON) for n in MODELS if n != "terrain"]      # (the permitted difference: the pipelines' order)
BOX = np.array([[1.0, 1.4, -0.5, 0.5, 0.1]])
PIPELINES = ((KinodynamicPipeline, KinodynamicProblem), (CentroidalPipeline, CentroidalProblem), (FullDynamicPipeline, FullDynamicsProblem))
EVERY_MODEL = dict(contact_rule={}, terrain=BOX, plant={}, friction={}, actuators={}, sensors={}, foot_sensors={}, detected_contacts=("estimator",),
                   estimator={})


@pytest.fixture
def calls(monkeypatch):
    """-> the list the recorders append ``(name, turned_off)`` to; ``calls.feeds`` keeps the consumers handed to ``foot_sensors_feed``"""
    class Calls(list):
        feeds = []
    log = Calls()
    log.feeds = []

    def recorder(name):
        def record(self, arg, *a, **kw):
            log.append((name, arg is None))
            if name == "foot_sensors_feed":
                log.feeds.append(tuple(arg))
        return record
    for name in MODELS:
        monkeypatch.setattr(_capi.NativeSolver, name, recorder(name))
    full = lambda v: (lambda self, raw=False: {"x": np.full((self.dims.batch, self.dims.nx), v)})
    monkeypatch.setattr(_capi.NativeSolver, "read_sensors", full(X_SENSED))
    monkeypatch.setattr(_capi.NativeSolver, "read_estimator", full(X_ESTIMATED))
    return log


def _pipeline(cls, problem, lib, **kw):
    return cls(problem(horizon=20), batch=2, library=lib, **kw)


def _bullet(lib, **kw):
    rb = Robot()
    m = rb.model
    robot = BulletRobot([n for n in m.names], None, None, 1e-3, m, library=lib, **kw)
    robot.initializeJoints(rb.x0[:m.nq])
    return rb, robot


# -- 1. the order of a constructor ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,problem", PIPELINES)
def test_a_pipeline_arms_its_models_in_one_order(oracle_lib, calls, cls, problem):
    p = _pipeline(cls, problem, oracle_lib, **EVERY_MODEL)
    assert calls == PIPELINE_ORDER and calls.feeds == [("estimator",)]
    assert np.all(p.x_prev == X_ESTIMATED) and p.x_prev.shape == p.x.shape     # the next solve starts from what the controllers read
    assert not np.any(p.x == X_ESTIMATED) and np.all(p.x_meas == X_SENSED) and np.all(p.x_est == X_ESTIMATED)


def test_bullet_robot_arms_its_models_in_one_order(oracle_lib, calls):
    _, robot = _bullet(oracle_lib, device_contacts=True, plant={}, friction={}, actuators={}, sensors={}, foot_sensors={}, estimator={})
    assert calls in (BULLET_ORDER, BULLET_ORDER_UNIFIED) and calls.feeds == [()]
    q, v = robot.measureState()
    assert np.all(q == X_ESTIMATED) and np.all(v == X_ESTIMATED)     # (every joint is controlled: the whole complete state is the estimate)


# -- 2. what arms again ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,problem", PIPELINES)
def test_the_estimator_arms_again_whenever_the_sensors_change(oracle_lib, calls, cls, problem):
    p = _pipeline(cls, problem, oracle_lib, **EVERY_MODEL)
    del calls[:]
    p.set_sensors(None)
    assert calls == [("sensors", OFF), ("estimator", ON)]
    assert p.x_meas is p.x and np.all(p.x_est == X_ESTIMATED)
    del calls[:]
    p.set_sensors(None)          # (off already: the library is not touched for the sensors)
    assert calls == [("estimator", ON)]
    del calls[:]
    p.set_sensors({})
    assert calls == [("sensors", ON), ("estimator", ON)]
    del calls[:]
    p.set_estimator(None)
    p.set_estimator(None)
    assert calls == [("estimator", OFF)]
    assert np.all(p.x_est == X_SENSED)
    del calls[:]
    p.set_sensors({})            # (no estimator in force: nothing follows)
    assert calls == [("sensors", ON)]


@pytest.mark.parametrize("cls,problem", PIPELINES)
def test_turning_the_foot_sensors_off_resets_the_consumers(oracle_lib, calls, cls, problem):
    p = _pipeline(cls, problem, oracle_lib, **EVERY_MODEL)
    del calls[:], calls.feeds[:]
    p.set_foot_sensors({})       # (detected_contacts None: as before)
    assert calls == [("foot_sensors", ON), ("foot_sensors_feed", ON)] and calls.feeds == [("estimator",)]
    del calls[:], calls.feeds[:]
    p.set_foot_sensors(None)
    p.set_foot_sensors(None)
    assert calls == [("foot_sensors", OFF)]
    p.set_foot_sensors({})
    assert calls[1:] == [("foot_sensors", ON), ("foot_sensors_feed", ON)] and calls.feeds == [()]


@pytest.mark.parametrize("cls,problem", PIPELINES)
def test_a_model_that_is_off_is_not_turned_off_again(oracle_lib, calls, cls, problem):
    p = _pipeline(cls, problem, oracle_lib, contact_rule={})
    del calls[:]
    for off in (p.set_plant, p.set_friction, p.set_actuators, p.set_sensors, p.set_foot_sensors, p.set_estimator):
        off(None)
    assert calls == []
    p.set_plant({}), p.set_friction({}), p.set_actuators({})
    for off in (p.set_plant, p.set_friction, p.set_actuators):
        off(None)
    assert calls == [("plant", ON), ("friction", ON), ("actuators", ON), ("plant", OFF), ("friction", OFF), ("actuators", OFF)]
    assert p.friction_state() is None and p.plant_models() == [p.model] * 2


def test_bullet_robot_sensors_off_on_a_library_without_them(oracle_lib, calls):
    """the sensors were never armed (the oracle has no mpc_sim_sensors): removing them only arms the estimator again, on the true state"""
    assert not hasattr(oracle_lib, "mpc_sim_sensors")
    _, robot = _bullet(oracle_lib, device_contacts=True, estimator={})
    assert calls == [("contacts", ON), ("estimator", ON)]
    del calls[:]
    robot.setSensors(None)
    assert calls == [("estimator", ON)]


def test_bullet_robot_reset_state_arms_sensors_then_estimator(oracle_lib, calls):
    rb, robot = _bullet(oracle_lib, device_contacts=True, sensors={}, estimator={})
    assert calls == [("contacts", ON), ("sensors", ON), ("estimator", ON)]
    del calls[:]
    robot.resetState(rb.x0[:rb.model.nq])
    assert calls == [("sensors", ON), ("estimator", ON)]
    del calls[:]
    robot.setEstimator(None)
    robot.setSensors(None)
    del calls[:]
    robot.resetState(rb.x0[:rb.model.nq])
    assert calls == []


# -- 3. what the controllers read when a model is off ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,problem", PIPELINES)
def test_measurement_and_estimate_fall_back(oracle_lib, calls, cls, problem):
    p = _pipeline(cls, problem, oracle_lib)
    assert calls == []
    assert p.x_meas is p.x and p.x_est is p.x
    assert np.array_equal(p.x_prev, p.x) and p.x_prev is not p.x
    p = _pipeline(cls, problem, oracle_lib, sensors={})
    assert np.all(p.x_meas == X_SENSED) and np.all(p.x_est == X_SENSED) and np.all(p.x_prev == X_SENSED)
    p = _pipeline(cls, problem, oracle_lib, contact_rule={}, estimator={})
    assert p.x_meas is p.x and np.all(p.x_est == X_ESTIMATED) and np.all(p.x_prev == X_ESTIMATED)


def test_the_centroidal_x_prev_is_the_true_state_without_sensors_or_estimator(oracle_lib, calls):
    """(the other two start from ``mpc.x0``; the centroidal pipeline draws its own whole-body states and overwrites ``x_prev`` only for a model)"""
    p = _pipeline(CentroidalPipeline, CentroidalProblem, oracle_lib, contact_rule={}, actuators={}, plant={}, foot_sensors={})
    assert np.array_equal(p.x_prev, p.x) and p.x_prev is not p.x and p.x.shape == (2, p.nq + p.nv)
    for cls, problem in PIPELINES[::2]:
        q = _pipeline(cls, problem, oracle_lib)
        assert np.array_equal(q.x, np.array(q.mpc.x0, dtype=float)) and np.array_equal(q.x_prev, q.x)


def test_bullet_robot_measures_the_true_state_without_models(oracle_lib, calls):
    rb, robot = _bullet(oracle_lib)
    assert calls == []
    q, v = robot.measureState()
    assert np.array_equal(q, rb.x0[:rb.model.nq]) and not np.any(v)
    _, robot = _bullet(oracle_lib, sensors={})
    q, v = robot.measureState()
    assert np.all(q == X_SENSED) and np.all(v == X_SENSED)
    assert robot.detectedContacts() == [True, True] and robot.frictionState() is None and robot.plantModel() is robot.model


def test_a_contact_source_of_none_is_refused_before_any_library_call():
    """(the two pipelines with a low-level QP: None is no way to say "no QP")"""
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the library was touched: " + name)
    for cls, problem in PIPELINES[:2]:
        with pytest.raises(ValueError, match="contact_source"):
            _pipeline(cls, problem, Untouchable(), contact_source=None)


def test_a_dropped_pipeline_frees_its_handles_at_once(oracle_lib, calls):
    """no reference cycle through the models: the handles (device memory at batch B) go when the last reference to their owner goes"""
    import gc
    import weakref
    owners = [_pipeline(cls, problem, oracle_lib, sensors={}) for cls, problem in PIPELINES] + [_bullet(oracle_lib, sensors={})[1]]
    handles = [weakref.ref(getattr(o, "sim", None) or o._native) for o in owners]
    gc.collect()
    gc.disable()
    try:
        del owners
        assert [h() for h in handles] == [None] * 4
    finally:
        gc.enable()


# -- 4. one robot, one set of tables --------------------------------------------------------------------------------------------------------------------
def test_pipelines_and_bullet_robot_upload_the_same_tables(oracle_lib, monkeypatch):
    """``Robot()`` through a pipeline (``foot_joint_ids``, ``foot_placements``) and through BulletRobot with every joint controlled (the sole frames'
    parent joints, the soles' placements at ``x0``): the same model tables, terminal stage and stage 0 of every contact mask."""
    log = []
    set_model, set_stage = _capi.NativeSolver.set_model, _capi.NativeSolver.set_stage
    monkeypatch.setattr(_capi.NativeSolver, "set_model", lambda self, i, d: (log.append((self, "model", np.array(i), np.array(d))), set_model(self, i, d))[1])
    monkeypatch.setattr(_capi.NativeSolver, "set_stage", lambda self, k, i, d: (log.append((self, k, np.array(i), np.array(d))), set_stage(self, k, i, d))[1])
    p = _pipeline(FullDynamicPipeline, FullDynamicsProblem, oracle_lib)
    _, robot = _bullet(oracle_lib)
    masks = ((True, True), (True, False), (False, True), (True, True))
    for mask in masks:
        p._set_sim_contacts(mask)
        robot.in_contact = list(mask)
        robot._upload_mask()
    mine, theirs = ([u[1:] for u in log if u[0] is h] for h in (p.sim, robot._native))
    assert [u[0] for u in mine] == [u[0] for u in theirs] == ["model", 1, 0, 0, 0, 0]
    for a, b in zip(mine, theirs):
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), a[0]
    same = lambda a, b: a[1].shape == b[1].shape and a[2].shape == b[2].shape and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert not same(mine[2], mine[3]) and not same(mine[3], mine[4]) and not same(mine[2], mine[4]) and same(mine[2], mine[5])
