"""The Python side of the torque-driven simulator (the plant of the three control pipelines and of the headless BulletRobot), written once; the
C++ side is include/sim_host.h.  ``build_simulator`` lowers the contact-mask stages of a model and opens the handle, ``upload_stage0`` keeps stage 0
on the contact mask, and ``SimulatorModels`` owns the rules by which the per-robot models of a handle are armed, armed again and turned off.  A new
extension of the plant is added here once: its rule in ``SimulatorModels`` (and in ``arm``, at its place in the order); ``pipeline.py`` and
``bullet_robot.py`` only pass their argument through."""
from __future__ import annotations

import numpy as np

from . import _capi as K
from . import actuator_model as _actuator_model
from . import disturbance_model as _disturbance_model
from . import foot_sensors as _foot_sensors
from . import friction_model as _friction_model
from . import joint_stops as _joint_stops
from . import tipping_model as _tipping_model
from . import plant_model as _plant_model
from . import sensor_model as _sensor_model
from . import state_estimator as _state_estimator
from .aligator import _core as core
from .aligator import dynamics as _dyn
from .aligator import manifolds as _manifolds
from .robot import minipin as pin

CONTACT_MASKS = ((True, True), (True, False), (False, True))   # (left, right): the stages a simulator handle can have as its stage 0


def _sim_options():
    """option block of a simulator handle (never solves: only the library's own consistency checks look at it)"""
    o = K.default_options(1e-5, 1e-8)
    o.force_initial_condition, o.rollout_linear = 1, 1
    return o


def build_simulator(lib, model, contacts, batch, sim_dt, device, sim=None):
    """One simulator handle: horizon 1, the whole-body contact dynamics of ``model`` under the three contact masks, 6-D rigid contacts with Baumgarte
    correction.  ``contacts``: (name, parent joint, local placement, world anchor) of the left and the right sole.  ``sim``: None opens the handle
    on ``lib`` (None: the HIP library); an existing handle gets the model and the terminal stage again (anchors moved: the library rebuilds an armed
    plant model from ``set_model``).  -> (NativeSolver with ``ctx``, the lowering context, {(left, right): lowered stage 0})."""
    m = model
    nu = m.nv - 6
    space = _manifolds.MultibodyPhaseSpace(m)
    ctx = core.LoweringContext()
    cms = []
    for name, jid, placement, anchor in contacts:
        cm = pin.RigidConstraintModel(pin.ContactType.CONTACT_6D, m, jid, placement, 0, anchor, pin.LOCAL)
        cm.corrector.Kp[:] = (0, 0, 10, 0, 0, 0)      # fulldynamic_talos.py:93-94
        cm.corrector.Kd[:] = (50, 50, 50, 50, 50, 50)
        cm.name = name
        cms.append(cm)
    act, prox = np.eye(m.nv, nu, -6), pin.ProximalSettings(1e-9, 1e-10, 1)
    tables = {}
    for mask in CONTACT_MASKS:
        ode = _dyn.MultibodyConstraintFwdDynamics(space, act, [c for c, on in zip(cms, mask) if on], prox)
        cost = core.CostStack(space, nu)
        cost.addCost(core.QuadraticControlCost(space, np.zeros(nu), np.eye(nu)))
        st = core.StageModel(cost, _dyn.IntegratorSemiImplEuler(ode, sim_dt))
        tables[mask] = core.lower_stage(ctx, st.cost, st.dynamics, st.constraints)
    tcost = core.CostStack(space, nu)
    tcost.addCost(core.QuadraticStateCost(space, nu, space.neutral(), np.eye(space.ndx)))
    term = core.lower_stage(ctx, tcost, None, core._ConstraintStack())
    if sim is None:
        d = K.MpcDims()
        d.horizon, d.batch, d.space = 1, batch, K.SPACE_MULTIBODY
        d.nx, d.ndx, d.nu, d.nc_max = space.nx, space.ndx, nu, 1
        d.max_stage_ints = 8 + 8 * 24
        d.max_stage_doubles = max(t[1].size for t in tables.values()) + term[1].size + 1024
        d.device = device
        sim = K.NativeSolver(lib if lib is not None else K.load_hip_library(), d)
        sim.set_options(_sim_options())
    sim.set_model(*ctx.model_tables())
    sim.set_stage(1, *term)
    sim.ctx = ctx   # (whoever needs a frame of this handle's model tables adds it here: EnsembleMPC.enable_walk(model_handle=...))
    return sim, tables


def upload_stage0(sim, tables, mask, uploaded):
    """stage 0 of a simulator handle follows the contact mask: uploaded when it changed.  -> the mask in force"""
    mask = (bool(mask[0]), bool(mask[1]))
    if mask != uploaded:
        sim.set_stage(0, *tables[mask])
    return mask


def checked_plant(rows, link_scale, batch, nj):
    """the rows of a plant model (a dict may carry ``link_scale``) -> (rows (B, 16), link_scale (B, nj) or None) by ``plant_model.validate``"""
    if isinstance(rows, dict):
        rows = dict(rows)
        link_scale = rows.pop("link_scale", link_scale)
    return _plant_model.validate(_plant_model.rows(rows, batch), nj, link_scale)


class SimulatorModels:
    """The per-robot models of one simulator handle of batch B (module docstring of pipeline.py): which are in force, and the rules of arming them.
    The caller hands in what is its own: ``x``, the true states (B, nx) (or (nx,) for B = 1) as they stand, wherever a model arms at them or falls
    back to them, and ``q``, the configuration the defaults of the friction and tipping models are taken at (nothing here refers back to the caller).
    ``rows[name]`` is what model ``name`` was armed with, None while it is off; turning a model off touches the library only if it was on.  Refusals that name their caller (a model that needs the contact rule) are the caller's, before it calls here."""
    NAMES = ("disturbances", "plant", "friction", "tipping", "actuators", "joint_stops", "sensors", "foot_sensors", "estimator")

    def __init__(self, sim, model, sole_frames, sim_dt):
        self.sim, self.model, self.batch = sim, model, sim.dims.batch
        self._sole_frames, self._sim_dt = sole_frames, sim_dt
        self.rows = dict.fromkeys(self.NAMES)
        self.consumers = ()      # who works from the detected contacts (``foot_sensors.CONSUMERS``)

    def arm(self, x, q, plant=None, friction=None, actuators=None, sensors=None, foot_sensors=None, estimator=None, disturbances=None,
            tipping=None, joint_stops=None):
        """Arm the models that are given, in the one order.  ``plant``, ``actuators``, ``joint_stops`` and ``foot_sensors``: the argument tuples of their
        ``set_*``; ``disturbances``: (events, contact_rule) of ``set_disturbances``."""
        if disturbances is not None:
            self.set_disturbances(*disturbances)
        if plant is not None:
            self.set_plant(*plant)
        if friction is not None:
            self.set_friction(friction, q)
        if tipping is not None:
            self.set_tipping(tipping, q)
        if actuators is not None:
            self.set_actuators(*actuators)
        if joint_stops is not None:
            self.set_joint_stops(*joint_stops)
        if sensors is not None:
            self.set_sensors(sensors, x)
        if foot_sensors is not None:   # (before the estimator: its arming event already reads the pair it will be fed)
            self.set_foot_sensors(*foot_sensors)
        if estimator is not None:
            self.set_estimator(estimator, x)

    def _turn_off(self, name):
        if self.rows[name] is not None:
            getattr(self.sim, name)(None)
        self.rows[name] = None

    def set_disturbances(self, events, contact_rule=True):
        """``events`` in the forms of ``NativeSolver.disturbances``; ``contact_rule``: is the contact rule on (contact triggers are refused without
        it).  Checked before any library call; arms the schedule and resets its clock.  None: off."""
        if events is None:
            return self._turn_off("disturbances")
        checked = _disturbance_model.validate(_disturbance_model.rows(events, self.batch), self.model.njoints - 1, contact_rule)
        self.sim.disturbances(checked)
        self.rows["disturbances"] = checked

    def disturbance_state(self):
        """the state rows of the push schedule by ``disturbance_model.unpack`` (``step``, ``acting``, ``impulse`` ...); None while it is off"""
        return None if self.rows["disturbances"] is None else self.sim.read_disturbances()

    def set_plant(self, rows, link_scale=None):
        """``rows`` in the forms of ``NativeSolver.plant``, a dict may also carry ``link_scale``; checked before any library call.  None: off."""
        if rows is None:
            return self._turn_off("plant")
        checked = checked_plant(rows, link_scale, self.batch, self.model.njoints - 1)
        self.sim.plant(checked[0], link_scale=checked[1])
        self.rows["plant"] = checked

    def plant_models(self):
        """one ``minipin.Model`` per robot: what the simulator integrates (``plant_model.models``; the nominal model B times without a plant model)"""
        if self.rows["plant"] is None:
            return [self.model] * self.batch
        return _plant_model.models(self.model, *self.rows["plant"])

    def set_friction(self, rows, q=None):
        """``rows`` in the forms of ``NativeSolver.friction``, a dict's missing fields from ``friction_model.defaults`` of the nominal robot at ``q`` and the
        simulator's step length; checked before any library call; every sole at rest.  None: off."""
        if rows is None:
            return self._turn_off("friction")
        base = _friction_model.defaults(self.model, q, self._sole_frames, self._sim_dt)
        checked = _friction_model.validate(_friction_model.rows(rows, self.batch, base))
        self.sim.friction(checked)
        self.rows["friction"] = checked

    def friction_state(self):
        """the state rows of the friction model by ``friction_model.unpack`` (``v``, ``sliding``, ``slip_dist`` ...); None while it is off"""
        return None if self.rows["friction"] is None else self.sim.read_friction()

    def set_tipping(self, rows, q=None):
        """``rows`` in the forms of ``NativeSolver.tipping``, a dict's missing fields from ``tipping_model.defaults`` of the nominal robot at ``q`` and the
        simulator's step length; checked before any library call; every sole flat and at rest.  None: off."""
        if rows is None:
            return self._turn_off("tipping")
        base = _tipping_model.defaults(self.model, q, self._sole_frames, self._sim_dt)
        checked = _tipping_model.validate(_tipping_model.rows(rows, self.batch, base))
        self.sim.tipping(checked)
        self.rows["tipping"] = checked

    def tipping_state(self):
        """the state rows of the tipping model by ``tipping_model.unpack`` (``v``, ``th``, ``tipping``, ``peak_angle`` ...); None while it is off"""
        return None if self.rows["tipping"] is None else self.sim.read_tipping()

    def set_actuators(self, params, limit=None, friction_shape=None):
        """``params`` in the forms of ``NativeSolver.actuators``, a dict may also carry ``limit`` and ``friction_shape``; ``limit`` defaults to the
        model's effort limits.  Arms and resets the model.  None: off."""
        if params is None:
            return self._turn_off("actuators")
        if isinstance(params, dict):
            params = dict(params)
            limit = params.pop("limit", limit)
            friction_shape = params.pop("friction_shape", friction_shape)
        if limit is None:
            limit = np.asarray(self.model.effortLimit, dtype=float)[6:]
        rows = _actuator_model.rows(params, self.batch)
        self.sim.actuators(rows, limit=limit, friction_shape=friction_shape)
        self.rows["actuators"] = rows

    def applied_torques(self, tau):
        """after a simulator step under ``tau``: what the step integrated (the actuator model's output; ``tau`` itself while it is off)"""
        return tau if self.rows["actuators"] is None else self.sim.read_actuators()["applied"].copy()

    def set_joint_stops(self, params, lo=None, hi=None, scale=None):
        """``params`` in the forms of ``NativeSolver.joint_stops``; a dict may also carry ``lo``, ``hi``, ``scale`` and the ``range_scale``,
        ``margin`` and ``lock`` of ``joint_stops.limits``, which builds the tables from the model's position limits when ``lo`` / ``hi`` are not
        given.  ``scale`` defaults to the model's effort limits.  Checked before any library call; arms and resets the model.  None: off."""
        if params is None:
            return self._turn_off("joint_stops")
        lim = {}
        if isinstance(params, dict):
            params = dict(params)
            lo, hi, scale = params.pop("lo", lo), params.pop("hi", hi), params.pop("scale", scale)
            lim = {k: params.pop(k) for k in ("range_scale", "margin", "lock") if k in params}
        if lim and (lo is not None or hi is not None):
            raise ValueError("joint_stops: range_scale, margin and lock build the tables: give them or lo / hi, not both")
        if lo is None or hi is None:   # (the model's limits for the table that is not given)
            nominal = _joint_stops.limits(self.model, self.batch, **lim)
            lo, hi = (t if a is None else a for a, t in zip((lo, hi), nominal))
        lo, hi = (np.broadcast_to(np.asarray(a, dtype=float), (self.batch, self.model.nv - 6)) for a in (lo, hi))
        if scale is None:
            scale = np.asarray(self.model.effortLimit, dtype=float)[6:]
        checked = _joint_stops.validate(_joint_stops.rows(params, self.batch), lo, hi, scale)
        self.sim.joint_stops(*checked)
        self.rows["joint_stops"] = checked

    def joint_stop_state(self):
        """the state rows of the joint stops by ``joint_stops.unpack`` (``tau_stop``, ``pen``, ``peak_pen``, ``hits`` ...); None while they are off"""
        return None if self.rows["joint_stops"] is None else self.sim.read_joint_stops()

    def set_sensors(self, params, x):
        """``params`` in the forms of ``NativeSolver.sensors``.  Arms and resets the model at the true states ``x``; an estimator in force arms again, after
        the sensors, on what they deliver now.  None: off (the estimator then arms again on the true states)."""
        if params is None:
            self._turn_off("sensors")
        else:
            rows = _sensor_model.rows(params, self.batch)
            self.sim.sensors(rows, x)
            self.rows["sensors"] = rows
        if self.rows["estimator"] is not None:
            self.set_estimator(self.rows["estimator"], x)

    def set_estimator(self, params, x=None):
        """``params`` in the forms of ``NativeSolver.estimator``.  Arms and resets the estimator at ``x_meas(x)``.  None: off."""
        if params is None:
            return self._turn_off("estimator")
        rows = _state_estimator.rows(params, self.batch)
        self.sim.estimator(rows, self.x_meas(x))
        self.rows["estimator"] = rows

    def set_foot_sensors(self, params, consumers=None):
        """``params`` in the forms of ``NativeSolver.foot_sensors``; ``consumers``: who works from the detected pair (None: as before).  Arms the
        detector on the rule's ``in_contact`` pairs and sets the feed.  None: off, and the consumers go back to the plant's pair."""
        if params is None:
            self.consumers = ()
            return self._turn_off("foot_sensors")
        if consumers is None:
            consumers = self.consumers
        rows = _foot_sensors.rows(params, self.batch)
        self.sim.foot_sensors(rows)
        self.sim.foot_sensors_feed(consumers)
        self.rows["foot_sensors"], self.consumers = rows, consumers

    def x_meas(self, x):
        """what the sensors deliver: the measurement of the sensor model, the true states ``x`` themselves without one"""
        return self.sim.read_sensors()["x"] if self.rows["sensors"] is not None else x

    def x_est(self, x):
        """the state the controllers read: the estimate of the base-state estimator, ``x_meas(x)`` without one"""
        return self.sim.read_estimator()["x"] if self.rows["estimator"] is not None else self.x_meas(x)

    @property
    def detected(self):
        """(B, 2) the pair every robot's detector reports; without foot sensors the ``in_contact`` pair of the contact rule"""
        if self.rows["foot_sensors"] is not None:
            return self.sim.read_foot_sensors()["det"].copy()
        return self.sim.read_contacts()["in_contact"].copy()
