"""The control pipelines of the three scripts for an ensemble of robots (``KinodynamicPipeline`` below; ``CentroidalPipeline``,
centroidal_talos.py:353-468, and ``FullDynamicPipeline``, fulldynamic_talos.py:437-550, at the end of the file).

The kinodynamic control pipeline of kinodynamic_talos.py:361-497, every stage on the solver library:

    MPC tick (kinodynamic OCP, one ProxDDP iteration)                                   kinodynamic_talos.py:482-490
      -> 10 low-level steps of 1 ms, each:
           measured state of every robot                                                 :412-418
           a0, forces = xdot(knot 0), us[0] corrected by the Riccati feedback K_0        :420-434
           whole-body inverse-dynamics QP (IDSolver_ulim), assembled and solved on the device  (mpc_qp_solve_id)   :438-446
           torque clamped to the effort limits                                           :448-450
           one simulator step under that torque                  (mpc_simulate_torque)   :458 (device.execute)
      -> the measurement of the tick before becomes the initial condition of the next solve   :484-486

The three native pieces are the library's own (include/mpc_abi.h, include/mpc_qp_abi.h); between them travel the small per-robot
vectors (states, K_0, torques), not problem data.  The simulator is the stand-in of ``mpc_simulate_torque``: the whole-body contact
dynamics of the CONTACT STATE OF KNOT 0 of the schedule (what ``problem.stages[0]`` says, :419) — rigid contacts at the measured-at-start
foot placements, no physics engine.  ``library``: the HIP library by default; tests pass the oracle to get the reference run.  The handle, its
contact-mask stages and the rules by which the models below are armed are ``torque_simulator``'s, shared with the headless BulletRobot.

``contact_rule`` (all three pipelines): None, the simulator of the schedule above; or a dict over ``contact_rule.DEFAULTS`` ({} for the defaults,
the ground at the lower initial foothold): the simulator's stage 0 is double support and the unilateral rule of the headless BulletRobot decides
every robot's contacts on the device after every step (mpc_sim_contacts, include/mpc_sim_contacts.h; HIP library only).  By default the low-level
QPs keep the schedule's ``contact_state``, as the scripts do with ``problem.stages[0]``; ``contact_source`` changes that.

``contact_source`` (``KinodynamicPipeline`` and ``CentroidalPipeline``; the full-dynamics pipeline has no QP): ``"schedule"``, the default: every
robot's low-level QP works with ``contact_state()``, bit for bit what the pipelines did without the argument.  With ``contact_rule``, ``"plant"``: each
robot's QP takes the contact set of its own row of the rule, as it stands before the step; ``"both"``: the intersection of the two, and the plant's
set for a robot whose intersection is empty (``contact_rule.qp_contact_states`` is the definition).  The six ``forces`` components of a contact the QP
did not use are then 0.  ``tick()`` selects on the device, step by step, with no host round trip inside the period (mpc_qp_contact_source,
include/mpc_qp_contacts.h; HIP library only); ``tick(host_glue=True)`` reads the rows before every step and applies the numpy mirror.
``qp_contacts()`` returns the set of the last QP and the counts of plan against plant on either path.

``terrain`` (all three pipelines, with ``contact_rule`` only): None, the ground is the plane; or boxes ``(n, 5)`` for every robot / ``(B, n, 5)`` per
robot under the rule (mpc_sim_terrain, include/mpc_sim_terrain.h; ``contact_rule.stairs`` lays the reference's staircase).  Nothing else about a
tick changes: the planner keeps the schedule's footholds, the low-level QPs the contact set ``contact_source`` names (by default the schedule's
``contact_state``); the plant decides where a foot is caught.

``walk=dict(per_instance=True, commands=table)`` (all three pipelines): a walk command per robot, a (B, 16) table of ``references.walk_commands`` that
``EnsembleMPC.enable_walk`` takes (include/mpc_walk_commands.h) — one robot per step length, turn rate or lateral step in one ensemble.  The table is
checked when the pipeline is built; ``pipeline.mpc.set_walk_commands`` changes it mid-walk.

``actuators`` (all three pipelines): None, the simulator integrates the torque the controller computed; or the parameter rows of the per-robot actuator
model (``actuator_model``: transport delay, gain error, first-order lag, saturation, joint friction; (B, 8), one row of 8 for every robot, or a dict by
field name of scalars or (B,) arrays, which may also carry ``limit`` and ``friction_shape``), armed on the simulator handle when the pipeline is built
(mpc_sim_actuators, include/mpc_sim_actuators.h; HIP library only).  ``limit`` defaults to the model's effort limits.  ``torques`` is then the APPLIED
torque of the last step on both forms of a tick (the device loop returns it; the host glue reads it back after each step), and so are the record's
torque columns and the metrics' power and energy.  ``set_actuators`` changes or removes the model later.

``joint_stops`` (all three pipelines): None, every joint of the plant turns freely; or the parameter rows of the per-robot joint end-stops
(``joint_stops``: stiffness ``k``, damping ``d`` and ``cap`` in units of ``scale``; (B, 8), one row of 8 for every robot, or a dict by field name of
scalars or (B,) arrays, which may also carry the tables ``lo`` / ``hi`` (B, nu), or the ``range_scale``, ``margin`` and ``lock`` that
``joint_stops.limits`` builds them from, and ``scale``), armed on the simulator handle after the actuators (mpc_sim_joint_stops,
include/mpc_sim_joint_stops.h; HIP library only).  The tables default to the model's position limits, ``scale`` to its effort limits.  Only the plant
changes: a joint beyond its range is pushed back by a one-sided spring and damper that the dynamics integrate with the actuators' torque.
``torques``, the record's torque columns and the metrics' power stay the actuators' torque: a stop is not a motor.  ``joint_stop_state()`` returns
the stop torques, penetrations and counters; ``set_joint_stops`` changes or removes the model later.

``sensors`` (all three pipelines): None, the controllers read the simulator's exact state; or the parameter rows of the per-robot sensor model
(``sensor_model``: latency, encoder resolution, calibration offsets, joint and floating-base noise, finite-difference joint velocities, their low-pass;
(B, 16), one row of 16 for every robot, or a dict by field name of scalars or (B,) arrays), armed on the simulator handle at the pipeline's true
states (mpc_sim_sensors, include/mpc_sim_sensors.h; HIP library only).  ``x`` stays the TRUE state, and the plant, its record, its metrics, its contact
rule and the QPs' contact source keep it; ``x_meas`` is the measurement.  The feedback laws, the low-level QPs and the task errors work at the
measurement, and ``x_prev`` / ``c_prev`` (the next solve's initial condition, the state the walk references are planned from) are measured ones, on
both forms of a tick: the device loops read the measurement where the kernel left it, the host glue reads it back before each step.
``set_sensors`` changes or removes the model later (it arms at the current ``x``).

``estimator`` (all three pipelines, with ``contact_rule``): None, the controllers read what the sensors deliver; or the parameter rows of the per-robot
base-state estimator (``state_estimator``: ``w_p``, ``w_v``, the weights of leg odometry through the soles the contact rule holds in the base position
and the base linear velocity; (B, 16), one row of 16 for every robot, or a dict by field name of scalars or (B,) arrays), armed on the simulator
handle after the sensors, at ``x_meas`` (mpc_sim_estimator, include/mpc_sim_estimator.h; HIP library only).  ``x`` stays the TRUE state, ``x_meas``
the sensor measurement, ``x_est`` is the estimate: what the feedback laws, the low-level QPs and the task errors work at and what ``x_prev`` /
``c_prev`` hold, on both forms of a tick (the host glue reads ``x_est`` back before each step and applies nothing else).  ``set_estimator`` changes or
removes the estimator later (it arms at the current ``x_meas``); ``set_sensors`` arms it again, after the sensors.

``foot_sensors`` (all three pipelines, with ``contact_rule``): None, nobody measures the contact wrenches; or the parameter rows of the per-robot foot
force sensors and contact detector (``foot_sensors``: latency, noise, offsets, a low-pass, thresholds with hysteresis and debounce; (B, 16), one row
of 16 for every robot, or a dict by field name of scalars or (B,) arrays), armed on the simulator handle on the rule's ``in_contact`` pairs
(mpc_sim_foot_sensors, include/mpc_sim_foot_sensors.h; HIP library only).  On its own the model only observes: ``detected`` is the pair every robot
takes to stand, ``sim.read_foot_sensors()["counts"]`` the confusion against the plant.  ``detected_contacts``: a subset of ``("estimator", "qp")``
naming who works from the detected pair instead of the plant's: the events of the base-state estimator, and the "plant" rows of ``contact_source``
(``"qp"``: ``KinodynamicPipeline`` and ``CentroidalPipeline`` with a ``contact_source`` other than ``"schedule"``; ``qp_contacts()`` then counts plan
against detection).  The selection is made on the device on both forms of a tick for the estimator (its kernel runs inside every simulator step);
for the QPs ``tick()`` selects on the device and ``tick(host_glue=True)`` reads the detector rows back before each step.  The plant, its record, its
metrics and its contact rule keep the truth.  ``set_foot_sensors`` changes or removes the model later.

``plant`` (all three pipelines): None, every robot's simulator is integrated with the inertias its MPC and its low-level QPs were built from; or the
parameter rows of the per-robot plant model (``plant_model``: mass and inertia scales, a displaced centre of mass, a payload; (B, 16), one row of 16 for
every robot, or a dict by field name of scalars or (B,) arrays, which may also carry ``link_scale`` (B, nj)), checked before any library call and armed
on the simulator handle when the pipeline is built (mpc_sim_plant, include/mpc_sim_plant.h; HIP library only).  Only the plant changes: the dynamics of
every simulator step, and the centre of mass and centroidal momentum of the record and the metrics, are those of robot b's own inertias; the MPC, the
low-level QPs, the contact rule, the estimator and the walk generators keep the nominal model.  ``plant_models()`` returns the perturbed models;
``set_plant`` changes or removes the model later.

``friction`` (all three pipelines, with ``contact_rule``): None, every held sole transmits whatever tangential force and yaw moment it takes; or the
parameter rows of the per-robot ground friction (``friction_model``: ``mu`` and ``mu_spin`` of each sole, the slider's masses and bounds; (B, 8), one
row of 8 for every robot, or a dict by field name whose missing fields are the identity coefficients and ``friction_model.defaults`` of the robot),
armed on the simulator handle when the pipeline is built (mpc_sim_friction, include/mpc_sim_friction.h; HIP library only).  Only the plant changes: a
sole whose force leaves its cone slips.  The MPC stages and the low-level QPs keep their own cones (``mu = 0.8``).  ``friction_state()`` returns the
slip velocities and counters; ``set_friction`` changes or removes the model later.

``tipping`` (all three pipelines, with ``contact_rule``): None, every held sole transmits whatever roll and pitch moment it takes; or the parameter
rows of the per-robot sole tipping (``tipping_model``: ``half_length`` and ``half_width`` of each sole, the slider's inertia and bounds; (B, 8), one
row of 8 for every robot, or a dict by field name whose missing fields are the identity extents and ``tipping_model.defaults`` of the robot), armed
on the simulator handle when the pipeline is built (mpc_sim_tipping, include/mpc_sim_tipping.h; HIP library only).  Only the plant changes: a sole
whose centre of pressure leaves its rectangle rolls about that edge.  The MPC stages and the low-level QPs keep their own sole
(``FOOT_HALF_LENGTH``, ``FOOT_HALF_WIDTH``).  ``tipping_state()`` returns the tip velocities, angles and counters; ``set_tipping`` changes or
removes the model later.

``disturbances`` (all three pipelines): None, the only push is the one ``tick(push=...)`` arms for a whole period; or every robot's own schedule of
pushes (``disturbance_model``: up to 8 events per robot, each an absolute step of the simulator's clock or the n-th touchdown or lift-off of a sole
plus a delay, a duration, a rectangular or half-sine shape, and a force and point on any link in world or link axes; (B, n, 16) tables, one table for
every robot, or one list of events per robot), armed on the simulator handle when the pipeline is built (mpc_sim_disturbances,
include/mpc_sim_disturbances.h; HIP library only).  The device times the events step by step inside the low-level loop; contact triggers need
``contact_rule``.  ``disturbance_state()`` returns the clock, the counters and what acted; ``set_disturbances`` changes or removes the table later.
While a table is armed ``tick(push=...)`` raises.

``latency`` (all three pipelines): None, every robot follows knot 0 of a new plan from the first low-level step after the solve; or the rows of the
plan's per-robot hand-over latency (``plan_latency``: ``steps``, ``jitter``, ``seed``; an int, (B,) steps, (B, 4) rows or a dict).  Directly after the
low-level loop of a tick, before the next plan is solved, the pipeline publishes: knot 1 of the outgoing plan is held by value for every robot and
its latency L_b drawn; for its first L_b low-level steps after the solve the robot's controller reads that held record, then knot 0 of the new
plan.  The device loops read the held record and keep the countdown on the device (mpc_plan_latency, include/mpc_plan_latency.h; HIP library
only); ``tick(host_glue=True)`` applies the same rule with calls both libraries have and the mirror's clock.  ``plan_latency.from_solve_ms`` turns a
measured solve time into steps.  ``latency_state()`` returns the countdown and the counters; ``set_latency`` arms again or removes the model."""
from __future__ import annotations

import contextlib

import numpy as np

from . import _capi as K
from . import contact_rule as _contact_rule
from . import disturbance_model as _disturbance_model
from . import foot_sensors as _foot_sensors
from . import plan_latency as _plan_latency
from . import qp_utils
from . import torque_simulator as _tsim
from .aligator import manifolds as _manifolds
from .ensemble import EnsembleMPC
from .problems import common
from .robot import minipin as pin


# -- the push experiment of the scripts (commented out there): device.apply_force(f_disturbance, [0, 0, 0]) on ticks 160 - 170 -------------------------
PUSH_TICKS = (160, 171)        # `if t >= 160 and t < 171` (centroidal_talos.py:450-452, kinodynamic_talos.py:459-461, fulldynamic_talos.py:524-526)
PUSH_THETA = 6 * np.pi / 4     # theta of all three scripts
PUSH_FORCE = {"fulldynamic": 300.0, "kinodynamic": 300.0, "centroidal": 100.0}   # fd (fulldynamic_talos.py:433, kinodynamic_talos.py:357, centroidal_talos.py:350)


def push_schedule(t, fd, theta=PUSH_THETA, ticks=PUSH_TICKS):
    """The scripts' disturbance at MPC tick ``t`` (the script's loop index; a pipeline's ``mpc.tick`` before its ``tick()``): the world-frame force
    [cos theta, sin theta, 0] fd inside ticks 160 - 170, else None.  Pass it as ``tick(push=...)`` (tiled to (B, 3): at the base origin, or with a
    world point to (B, 6)); the pipelines arm it for the ten low-level steps of that period.

    The offset this leaves: the script calls ``device.apply_force`` AFTER each ``device.execute`` of the window, and PyBullet applies an external
    force during the next simulation step only, so there the push acts on steps 2 - 10 of tick 160, ..., steps 1 - 10 of tick 170 and step 1 of tick 171:
    one 1 ms step later than the per-period arm here (steps 1 - 10 of ticks 160 - 170).  The same impulse, not emulated (``BulletRobot.apply_force``
    reproduces the script's timing exactly)."""
    if not (ticks[0] <= t < ticks[1]):
        return None
    return np.array([np.cos(theta), np.sin(theta), 0.0]) * float(fd)


def _push_array(push, batch):
    """``tick(push=...)``: None, or (B, 3) (force at the base origin) / (B, 6) (force, world point), checked before any library call"""
    if push is None:
        return None
    p = np.asarray(push, dtype=float)
    if p.ndim != 2 or p.shape[0] != batch or p.shape[1] not in (3, 6):
        raise ValueError("push: (B, 3) (force at the base origin) or (B, 6) (force, world point) expected with B = %d, got shape %s" % (batch, p.shape))
    if not np.all(np.isfinite(p)):
        raise ValueError("push: non-finite entries")
    return np.ascontiguousarray(p)


def build_torque_simulator(lib, robot, batch, sim_dt, device):
    """The simulator stand-in of the three pipelines: one handle, horizon 1, whole-body contact dynamics of the three contact patterns (rigid contacts
    at the robot's initial foot placements; ``torque_simulator.build_simulator``).  -> (NativeSolver, {(left, right): lowered stage 0})."""
    frames = robot.model.frames
    contacts = [(name, jid, frames[fid].placement, oMf)
                for name, fid, jid, oMf in zip(common.FOOT_FRAMES, robot.foot_frame_ids, robot.foot_joint_ids, robot.foot_placements)]
    return _tsim.build_simulator(lib, robot.model, contacts, batch, sim_dt, device)


def _checked_terrain(name, terrain, contact_rule, batch):
    """``terrain`` of a pipeline: checked boxes or None; refused without ``contact_rule`` (the terrain is an input of the rule)"""
    if terrain is None:
        return None
    if contact_rule is None:
        raise ValueError("%s: terrain needs contact_rule (the terrain is the ground of the unilateral contact rule; contact_rule={} turns it on)" % name)
    return _contact_rule.terrain_boxes(terrain, batch)


def _checked_plant(plant, batch, problem_def):
    """``plant`` of a pipeline: None, or (rows (B, 16), link_scale (B, nj) or None) checked before any library call (``plant_model.validate``)"""
    return None if plant is None else _tsim.checked_plant(plant, None, batch, problem_def.robot.model.njoints - 1)


def _checked_friction(name, friction, contact_rule):
    """``friction`` of a pipeline needs the contact rule: checked before any library call (the rows themselves when the model is armed)"""
    if friction is not None and contact_rule is None:
        raise ValueError("%s: friction needs contact_rule (the model slides the soles the unilateral contact rule holds; contact_rule={} turns it on)" % name)


def _checked_tipping(name, tipping, contact_rule):
    """``tipping`` of a pipeline needs the contact rule: checked before any library call (the rows themselves when the model is armed)"""
    if tipping is not None and contact_rule is None:
        raise ValueError("%s: tipping needs contact_rule (the model tips the soles the unilateral contact rule holds; contact_rule={} turns it on)" % name)


def _checked_disturbances(name, events, contact_rule, batch, problem_def):
    """``disturbances`` of a pipeline: None, or the tables (B, n, 16) checked before any library call (``disturbance_model.validate``); contact
    triggers are refused without ``contact_rule``"""
    if events is None:
        return None
    try:
        return _disturbance_model.validate(_disturbance_model.rows(events, batch), problem_def.robot.model.njoints - 1, contact_rule is not None)
    except ValueError as e:
        raise ValueError("%s: %s" % (name, e)) from None


def _checked_walk(name, walk, batch):
    """``walk`` of a pipeline: the ``commands`` table in it is checked before any library call (shape, finite values, ``per_instance=True``)"""
    if walk is None or walk.get("commands") is None:
        return walk
    from . import references as refgen
    if not walk.get("per_instance"):
        raise ValueError("%s: walk commands need walk=dict(per_instance=True, commands=...) (the shared stage tables cannot carry per-robot references)" % name)
    walk = dict(walk)
    walk["commands"] = refgen.check_commands(walk["commands"], batch, "%s: walk commands" % name)
    return walk


def stairs_under_walk(robot, x_forward, z_height, y_gap=0.18, n_steps=3, half_extents=(0.2, 0.5)):
    """The reference's staircase (``contact_rule.stairs``, pitch = the step length) laid under the footholds the walk generator plans for the nominal
    robot: right foot first, every swing ``x_forward`` ahead of the stance foot and ``z_height`` above it (``references.FootTrajectory``).  The
    planned landing point of swing k lies in the middle of the visible tread of step k (with the reference's 0.4 m boxes at a pitch of 0.3 m: 5 cm
    behind the box's centre, 15 cm from the edge in front and from the riser of the next step), and the top of step k is exactly
    ``ground_z + (k + 1) z_height``, ``ground_z`` the lower initial foothold (where the pipelines put the rule's plane).
    -> (boxes (n_steps, 5), footholds (n_steps, 3))."""
    from . import references as refgen
    lf, rf = (M.copy() for M in robot.foot_placements)
    gz = min(float(np.asarray(M.translation)[2]) for M in (lf, rf))
    traj = refgen.FootTrajectory(lf.copy(), rf.copy(), 1, 1, 1, 0.0, x_forward, 0.0, 0.0, y_gap, z_height)
    holds = []
    while len(holds) < n_steps:   # (the generator's own foothold rule, two landings per call: right beside left, then left beside the new right)
        traj._plan_right_then_left(lf, rf)
        lf, rf = traj.final_pose_left.copy(), traj.final_pose_right.copy()
        holds += [np.array(rf.translation, dtype=float), np.array(lf.translation, dtype=float)]
    holds = np.array(holds[:n_steps])
    y_mid = 0.5 * float(np.asarray(robot.foot_placements[0].translation)[1] + np.asarray(robot.foot_placements[1].translation)[1])
    pose = np.array([holds[0, 0] + half_extents[0] - 0.5 * x_forward, y_mid, gz + 0.5 * z_height]) if n_steps else np.zeros(3)
    boxes = _contact_rule.stairs(pose, z_height, n_steps=n_steps, pitch=x_forward, half_extents=half_extents)
    boxes[:, 4] = gz + (np.arange(n_steps) + 1.0) * z_height
    return boxes, holds


class _Pipeline:
    """What the three pipelines share: the argument checks of a constructor, the simulator handle with its contact rule and its models
    (``torque_simulator.SimulatorModels``; module docstring), and the frame of a tick around the low-level loop."""
    contact_source = None     # (a pipeline without a low-level QP has none)

    def _init_contact_source(self, name, source, contact_rule):
        """(the hook of the pipelines with a low-level QP, ``_QpContactSource``)"""

    def _check_arguments(self, problem_def, batch, contact_rule, terrain, walk, friction, foot_sensors, detected_contacts, contact_source=None,
                         disturbances=None, latency=None, tipping=None):
        """the arguments every pipeline takes, checked before the library is loaded -> (walk, detected_contacts)"""
        name = type(self).__name__
        self.pd, self.batch = problem_def, int(batch)
        self._latency = _plan_latency.rows(latency, self.batch)
        self._init_contact_source(name, contact_source, contact_rule)
        detected_contacts = self._check_detected(name, foot_sensors, detected_contacts, contact_rule, self.contact_source)
        self.terrain = _checked_terrain(name, terrain, contact_rule, self.batch)
        walk = _checked_walk(name, walk, self.batch)
        _checked_friction(name, friction, contact_rule)
        _checked_tipping(name, tipping, contact_rule)
        self._disturbances = _checked_disturbances(name, disturbances, contact_rule, self.batch, problem_def)
        self.contact_rule = None if contact_rule is None else dict(contact_rule)
        return walk, detected_contacts

    def _check_detected(self, name, foot_sensors, detected_contacts, contact_rule, contact_source=None):
        """``foot_sensors`` / ``detected_contacts`` of a pipeline, checked before any library call -> the consumers as a tuple"""
        names = () if detected_contacts is None else ((detected_contacts,) if isinstance(detected_contacts, str) else tuple(detected_contacts))
        _foot_sensors.feed_mask(names)
        if foot_sensors is not None and contact_rule is None:
            raise ValueError("%s: foot_sensors needs contact_rule (the detector is armed on the rows of the unilateral contact rule; contact_rule={} "
                             "turns it on)" % name)
        if names and foot_sensors is None:
            raise ValueError("%s: detected_contacts=%r needs foot_sensors (the rows of the detector)" % (name, names))
        if "qp" in names and contact_source in (None, "schedule"):
            raise ValueError("%s: detected_contacts \"qp\" needs a low-level QP with contact_source \"plant\" or \"both\" (the detected pair takes the "
                             "place of the plant's rows there)" % name)
        return tuple(n for n in _foot_sensors.CONSUMERS if n in names)

    def _load(self, library, substeps, sim_dt):
        self.lib = library if library is not None else K.load_hip_library()
        m = self.model = self.pd.robot.model
        self.nq, self.nv = m.nq, m.nv
        self.substeps, self.sim_dt = int(substeps), float(sim_dt)

    def _build_simulator(self, plant, friction, actuators, sensors, foot_sensors, detected_contacts, estimator, stage0=None, tipping=None,
                         joint_stops=None):
        """The simulator stand-in (``build_torque_simulator``) with its contact rule and terrain, stage 0 on ``stage0`` if one is given, and the
        models armed at ``self.x``; ``x_prev`` starts from what the controllers read then."""
        rb = self.pd.robot
        self.sim, self._sim_tables = build_torque_simulator(self.lib, rb, self.batch, self.sim_dt, self.mpc.dims.device)
        self._sim_mask = None
        if self.contact_rule is not None:   # stage 0 is the double-support stage once; the rule is on from the initial footholds (the ground
            self.sim.set_stage(0, *self._sim_tables[(True, True)])   # plane at the lower one unless the config names ``ground_z``)
            gz = min(float(np.asarray(M.translation)[2]) for M in rb.foot_placements)
            self.sim.contacts(_contact_rule.config(self.contact_rule, ground_z=gz))
            if self.terrain is not None:
                self.sim.terrain(self.terrain)
        if stage0 is not None:
            self._set_sim_contacts(stage0)
        self.sim_models = _tsim.SimulatorModels(self.sim, self.model, rb.foot_frame_ids, self.sim_dt)
        self.sim_models.arm(self.x, rb.x0[:self.nq], plant, friction, None if actuators is None else (actuators,), sensors,
                            None if foot_sensors is None else (foot_sensors, detected_contacts), estimator,
                            None if self._disturbances is None else (self._disturbances, self.contact_rule is not None), tipping=tipping,
                            joint_stops=None if joint_stops is None else (joint_stops,))
        self.x_prev = self.x_est.copy()      # the measurement of the period before (the solve's initial condition)
        self.torques = np.zeros((self.batch, self.nv - 6))
        self._plan_stale = True
        self._reset_latency()

    def _set_sim_contacts(self, mask):
        if self.contact_rule is None:   # (else the rule decides every robot's contacts on the device)
            self._sim_mask = _tsim.upload_stage0(self.sim, self._sim_tables, mask, self._sim_mask)

    # -- the models of the plant (module docstring): ``None`` turns a model off ------------------------------------------------------------------------
    def set_plant(self, rows, link_scale=None):
        """Arm the per-robot plant model on ``self.sim``: ``rows`` in the forms of ``NativeSolver.plant``, a dict may also carry ``link_scale``."""
        self.sim_models.set_plant(rows, link_scale)

    def set_disturbances(self, events):
        """Arm the per-robot push schedule on ``self.sim`` and reset its clock: ``events`` in the forms of ``NativeSolver.disturbances``; contact
        triggers need ``contact_rule``.  None: off.  While a table is armed ``tick(push=...)`` is refused."""
        checked = _checked_disturbances(type(self).__name__, events, self.contact_rule, self.batch, self.pd)
        self.sim_models.set_disturbances(checked, self.contact_rule is not None)
        self._disturbances = checked   # (after the library took it: a refused table leaves the pipeline as it was)

    def disturbance_state(self):
        """the state rows of the push schedule by ``disturbance_model.unpack`` (``step``, ``acting``, ``impulse`` ...); None without ``disturbances``"""
        return self.sim_models.disturbance_state()

    def _checked_push(self, push):
        """``tick(push=...)`` checked before any library call: the array, and that no push schedule is armed (its events are the pushes)"""
        push = _push_array(push, self.batch)
        if push is not None and getattr(self, "_disturbances", None) is not None:
            raise ValueError("%s: tick(push=...) conflicts with the push schedule armed on this pipeline (disturbances=...): the schedule's events are "
                             "the pushes; set_disturbances(None) turns it off" % type(self).__name__)
        return push

    def set_friction(self, rows):
        """Arm the per-robot ground friction on ``self.sim`` with every sole at rest: ``rows`` in the forms of ``NativeSolver.friction``, a dict's
        missing fields from ``friction_model.defaults`` of the nominal robot; needs ``contact_rule``."""
        _checked_friction(type(self).__name__, rows, self.contact_rule)
        self.sim_models.set_friction(rows, self.pd.robot.x0[:self.nq])   # (a simulator step is one low-level period)

    def set_tipping(self, rows):
        """Arm the per-robot sole tipping on ``self.sim`` with every sole flat and at rest: ``rows`` in the forms of ``NativeSolver.tipping``, a
        dict's missing fields from ``tipping_model.defaults`` of the nominal robot; needs ``contact_rule``."""
        _checked_tipping(type(self).__name__, rows, self.contact_rule)
        self.sim_models.set_tipping(rows, self.pd.robot.x0[:self.nq])   # (a simulator step is one low-level period)

    def set_actuators(self, params, limit=None, friction_shape=None):
        """Arm (and reset) the per-robot actuator model on ``self.sim``: ``params`` in the forms of ``NativeSolver.actuators``, a dict may also carry
        ``limit`` and ``friction_shape``; ``limit`` defaults to the model's effort limits."""
        self.sim_models.set_actuators(params, limit, friction_shape)

    def set_joint_stops(self, params, lo=None, hi=None, scale=None):
        """Arm (and reset) the per-robot joint end-stops on ``self.sim``: ``params`` in the forms of ``NativeSolver.joint_stops``, a dict may also
        carry ``lo``, ``hi``, ``scale``, ``range_scale``, ``margin`` and ``lock``; the tables default to the model's position limits, ``scale`` to
        its effort limits."""
        self.sim_models.set_joint_stops(params, lo, hi, scale)

    def set_sensors(self, params):
        """Arm (and reset) the per-robot sensor model on ``self.sim`` at the current true states ``self.x``: ``params`` in the forms of
        ``NativeSolver.sensors``.  An estimator in force arms again, after the sensors."""
        self.sim_models.set_sensors(params, self.x)

    def set_estimator(self, params):
        """Arm (and reset) the per-robot base-state estimator on ``self.sim`` at the current measured states ``self.x_meas``: ``params`` in the
        forms of ``NativeSolver.estimator``; needs ``contact_rule``."""
        self.sim_models.set_estimator(params, self.x)

    def set_foot_sensors(self, params, detected_contacts=None):
        """Arm (and reset) the per-robot foot force sensors and contact detector on ``self.sim``: ``params`` in the forms of
        ``NativeSolver.foot_sensors``; needs ``contact_rule``.  ``detected_contacts``: who works from the detected pair (None: as before).  ``params``
        None turns the model off, and the consumers go back to the plant's pair."""
        if params is not None and detected_contacts is not None:
            detected_contacts = self._check_detected(type(self).__name__, params, detected_contacts, self.contact_rule, self.contact_source)
        self.sim_models.set_foot_sensors(params, detected_contacts)

    @property
    def x_meas(self):
        """what the sensors deliver: the measurement of the sensor model, ``x`` itself without one"""
        return self.sim_models.x_meas(self.x)

    @property
    def x_est(self):
        """the state the controllers read: the estimate of the base-state estimator, ``x_meas`` without one"""
        return self.sim_models.x_est(self.x)

    @property
    def detected(self):
        """(B, 2) the pair every robot's detector reports; without ``foot_sensors`` the ``in_contact`` pair of the contact rule"""
        return self.sim_models.detected

    def plant_models(self):
        """one ``minipin.Model`` per robot: what the simulator integrates (``plant_model.models``; the nominal model B times without ``plant``)"""
        return self.sim_models.plant_models()

    def friction_state(self):
        """the state rows of the friction model by ``friction_model.unpack`` (``v``, ``sliding``, ``slip_dist`` ...); None without ``friction``"""
        return self.sim_models.friction_state()

    def tipping_state(self):
        """the state rows of the tipping model by ``tipping_model.unpack`` (``v``, ``th``, ``tipping``, ``peak_angle`` ...); None without ``tipping``"""
        return self.sim_models.tipping_state()

    def joint_stop_state(self):
        """the state rows of the joint stops by ``joint_stops.unpack`` (``tau_stop``, ``pen``, ``peak_pen``, ``hits`` ...); None without ``joint_stops``"""
        return self.sim_models.joint_stop_state()

    # -- the hand-over latency of the plan (``plan_latency``, include/mpc_plan_latency.h): ``None`` turns it off ------------------------------------
    def _reset_latency(self):
        """the mirror's state rows as after arming; the device model, if a device tick armed one, is armed again with the rows in force (or off)"""
        self._lat_state = None if self._latency is None else _plan_latency.initial_state(self.batch)
        self._lat_held = None
        self._lat_form = None          # "host" or "device": the form of the ticks since arming (the two clocks are not one)
        if getattr(self, "_lat_on_device", False):
            self.mpc.native.plan_latency(None)
        self._lat_on_device = False

    def set_latency(self, rows):
        """Arm (and reset) the per-robot hand-over latency of the plan: ``rows`` in the forms of ``plan_latency.rows`` (None: off; an int; (B,)
        steps; (B, 4) rows; a dict of ``steps`` / ``jitter`` / ``seed``).  After every publication — directly after the low-level loop of a tick,
        before the next plan is solved — robot b keeps running knot 1 of the outgoing plan for its first L_b low-level steps.  Checked before
        anything changes."""
        self._latency = _plan_latency.rows(rows, self.batch)
        self._reset_latency()

    def latency_state(self):
        """the state rows of the latency model by ``plan_latency.unpack`` (``remaining``, ``drawn``, ``plans``, ``late_steps``, ``steps_total``,
        ``max_drawn``, ``held_valid``): the device's after device ticks, the mirror's after host-glue ticks; None without ``latency``"""
        if self._latency is None:
            return None
        if self._lat_on_device:
            r = self.mpc.native.read_plan_latency()
            return {k: r[k] for k in _plan_latency.STATE_FIELDS[:7]}
        return _plan_latency.unpack(self._lat_state)

    def _latency_tick(self, host_glue):
        """at the head of a tick: the two forms keep two clocks (the mirror's on the host, the kernels' on the device), so a pipeline with a latency
        armed runs one form until it is armed again; the first device tick arms the model on the plan handle"""
        if self._latency is None:
            return
        form = "host" if host_glue else "device"
        if self._lat_form not in (None, form):
            raise RuntimeError("%s: latency is armed and the ticks so far were %s ticks: the %s form keeps a clock of its own (set_latency arms "
                               "again, for either form)" % (type(self).__name__, self._lat_form, form))
        if form == "device" and not self._lat_on_device:
            self.mpc.native.plan_latency(self._latency)
            self._lat_on_device = True
        self._lat_form = form

    def _latency_publish(self, host_glue):
        """directly after the low-level loop of a tick, the outgoing plan still in the handle: every robot's held record and its draw.  Device: one
        kernel (mpc_plan_latency_publish).  Host glue: knot 1 fetched by calls both libraries have, the draw and the countdown by the mirror."""
        if self._latency is None:
            return
        if not host_glue:
            self.mpc.native.publish_plan()
            return
        nat = self.mpc.native
        r = nat.get_results(gains=False)
        o = _plan_latency.xdot_offset(nat.dims.space == K.SPACE_MULTIBODY, nat.dims.ndx)
        self._lat_held = dict(xs=r["xs"][:, 1].copy(), us=r["us"][:, 1].copy(), K=nat.get_gain(1)[0],
                              xdot=nat.get_stage_data(1)[0][:, o:o + _plan_latency.XDOT_PART].copy())
        self._lat_state = _plan_latency.publish(self._lat_state, self._latency)

    def _latency_first(self):
        """host glue: (B,) bool, who reads the held record on the next low-level step (nothing counted); None without ``latency``"""
        return None if self._latency is None else _plan_latency.step(self._lat_state)[0]

    def _knot_in_force(self, xdot0=None):
        """host glue, once per low-level step: the clock of every robot advances, and -> (xs, us, K[, xdot part]) of the record each robot's
        controller reads on this step: knot 0 of the plan, or the held record while the robot's countdown runs"""
        plan = (self.xs0, self.us0, self.K0) + (() if xdot0 is None else (xdot0,))
        if self._latency is None:
            return plan
        use, self._lat_state = _plan_latency.step(self._lat_state)
        if not use.any():
            return plan
        h = self._lat_held
        held = (h["xs"], h["us"], h["K"]) + (() if xdot0 is None else (h["xdot"],))
        return tuple(np.where(use.reshape((-1,) + (1,) * (a.ndim - 1)), a, b) for a, b in zip(held, plan))

    # -- the loop ---------------------------------------------------------------------------------------------------------------------
    def _walk_kwargs(self):
        return self._walk_args

    def cold_solve(self, max_iters=100):
        st = self.mpc.cold_solve(max_iters=max_iters)
        if self._walk_args is not None:
            self.mpc.enable_walk(**self._walk_kwargs())
        self._fetch()
        return st

    def _fetch(self):
        self._plan_stale = False
        r = self.mpc.native.get_results(gains=False)
        self.xs0, self.us0 = r["xs"][:, 0].copy(), r["us"][:, 0].copy()
        self.K0 = self.mpc.native.get_gain(0)[0]

    def contact_state(self):
        """[left, right] the low-level loop of this MPC period works with: ``problem.stages[0]`` AFTER this period's
        ``replaceStageCircular(stages_full[t])`` (kinodynamic_talos.py:393, 419-420) — the stage that was appended at tick t + 1 - N (the
        initial double support before that), one rotation later than knot 0 of the solution the feedback terms come from."""
        N, t = self.mpc.problem.num_steps, self.mpc.tick
        return self.pd.contact_phases[max(0, t + 1 - N) % self.pd.t_mpc]

    @contextlib.contextmanager
    def _pushed(self, push):
        """``push`` (checked, or None) armed on the simulator for the low-level steps inside the block only"""
        if push is not None:
            self.sim.set_push(push)
        try:
            yield
        finally:
            if push is not None:
                self.sim.set_push(None)

    def _solve_from_x_prev(self, x_last):
        """the tail of a tick: the walk references planned from the state that becomes the initial condition (walking_loop.py,
        fulldynamic_talos.py:440-462), the solve from ``x_prev``, and ``x_last`` the ``x_prev`` of the next tick"""
        e = self.mpc
        if e._walk is not None:
            e._walk["x_measured"] = self.x_prev[0].copy()
            if "x_measured_all" in e._walk:
                e._walk["x_measured_all"] = self.x_prev.copy()
        e.native.set_x0(self.x_prev)
        st = e.step()
        self.x_prev = x_last
        self._plan_stale = True   # (knot 0 of the new plan is read on the device; the host copies only when the host glue asks)
        return st


class _QpContactSource(_Pipeline):
    """``contact_source`` of the two pipelines with a low-level QP (module docstring): the checks, the host-glue form of the selection (the numpy mirror
    ``contact_rule.qp_contact_states`` on the rows read before every step) and ``qp_contacts``."""

    def _init_contact_source(self, name, source, contact_rule):
        """checked before any library call"""
        _contact_rule.qp_source(source)
        if source != "schedule" and contact_rule is None:
            raise ValueError("%s: contact_source=%r needs contact_rule (the plant's contact set is a row of the unilateral contact rule; "
                             "contact_rule={} turns it on)" % (name, source))
        self.contact_source = source
        self._qp_used = np.zeros((self.batch, 2), dtype=np.int32)          # the set of the last QP on the host-glue path (and of "schedule")
        self._qp_counts = np.zeros((self.batch, 2, 4), dtype=np.int32)     # counted on the host-glue path
        self._qp_last_on_device = False
        self._qp_source_on_device = False

    def _host_contact_set(self, cs):
        """host glue, before a low-level step: the contact set of every robot's QP from the rows as they stand -> (B, 2) int32"""
        self._qp_last_on_device = False
        if self.contact_source == "schedule":
            self._qp_used = _contact_rule.qp_contact_states("schedule", cs, np.ones((self.batch, 2)))
            return self._qp_used
        p = self.detected if "qp" in self.sim_models.consumers else self.sim.read_contacts()["in_contact"]   # (the detector's rows, read back)
        self._qp_used = _contact_rule.qp_contact_states(self.contact_source, cs, p)
        self._qp_counts = _contact_rule.qp_contact_counts(self._qp_counts, cs, p)
        return self._qp_used

    def _device_contact_source(self, cs):
        """device loop: the mode is set once on the QP handle (never for "schedule": the handle's default, and the call is HIP only)"""
        if self.contact_source == "schedule":
            self._qp_used = _contact_rule.qp_contact_states("schedule", cs, np.ones((self.batch, 2)))
            return
        if not self._qp_source_on_device:
            self.qp.qp.contact_source(self.contact_source)
            self._qp_source_on_device = True
        self._qp_last_on_device = True

    def qp_contacts(self):
        """-> dict(used=(B, 2) int32: the contact set of every robot's last low-level QP; counts=(B, 2, 4) int32: ``counts[b, c, 2 s + p]``, how many
        steps the schedule (s) and the plant (p) had contact c of robot b off / on (``contact_rule.qp_contact_counts``)).  With ``"schedule"`` nothing
        is read from the plant and the counts stay 0."""
        used, counts = self._qp_used.copy(), self._qp_counts.copy()
        if self._qp_source_on_device:
            r = self.qp.qp.read_contact_source()
            counts += r["counts"]
            if self._qp_last_on_device:
                used = r["used"]
        return dict(used=used, counts=counts)


class KinodynamicPipeline(_QpContactSource):
    def __init__(self, problem_def, batch=1, library=None, walk=None, weights_id=(1.0, 10000.0), substeps=10, sim_dt=1e-3, x0=None, contact_rule=None,
                 terrain=None, contact_source="schedule", actuators=None, sensors=None, estimator=None, foot_sensors=None,
                 detected_contacts=(), plant=None, friction=None, disturbances=None, latency=None, tipping=None, joint_stops=None, **ens_kw):
        """``problem_def``: a KinodynamicProblem.  ``walk``: keyword arguments of ``EnsembleMPC.enable_walk`` ({} = the script's 0.3 m steps)
        or None (references frozen at the initial footholds).  ``contact_rule``: None or a config dict, ``terrain``: None or boxes,
        ``contact_source``: "schedule", "plant" or "both", ``actuators``: None or the rows of the actuator model, ``sensors``: None or the rows of the
        sensor model, ``estimator``: None or the rows of the base-state estimator, ``foot_sensors``: None or the rows of the foot force sensors,
        ``detected_contacts``: who works from the detected contacts, ``plant``: None or the rows of the plant model, ``friction``: None or the rows of
        the ground friction, ``tipping``: None or the rows of the sole tipping, ``joint_stops``: None or the rows of the joint end-stops, ``latency``: None or the rows of the plan's hand-over latency (module
        docstring)."""
        walk, detected_contacts = self._check_arguments(problem_def, batch, contact_rule, terrain, walk, friction, foot_sensors, detected_contacts,
                                                        contact_source, disturbances=disturbances, latency=latency, tipping=tipping)
        plant = _checked_plant(plant, self.batch, problem_def)
        self._load(library, substeps, sim_dt)
        rb, m = problem_def.robot, self.model
        self.mpc = EnsembleMPC(problem_def, batch=batch, library=self.lib, x0=x0, **ens_kw)
        self._walk_args = walk
        # the low-level QP of the script: weights [1, 10000] on acceleration / force increments (kinodynamic_talos.py:350-351)
        self.qp = qp_utils.IDSolver_ulim(m, list(weights_id), 2, common.FRICTION_MU, common.FOOT_HALF_LENGTH, common.FOOT_HALF_WIDTH,
                                         list(rb.foot_frame_ids), 6, library=self.lib, batch=self.batch)
        self.qp.enable_device_assembly()
        self.umax = np.asarray(m.effortLimit, dtype=float)[6:]
        self.x = np.array(self.mpc.x0, dtype=float)      # measured states, one row per robot
        self._build_simulator(plant, friction, actuators, sensors, foot_sensors, detected_contacts, estimator, tipping=tipping,
                              joint_stops=joint_stops)
        self.forces = np.zeros((self.batch, 12))

    def _fetch(self):
        super()._fetch()
        self.xdot0 = self.mpc.native.get_stage_data(0)[0]

    def low_level_step(self, cs):
        """One 1 kHz step of kinodynamic_talos.py:411-462 for every robot, the glue between the library calls on the host.  ``cs``: (2,) for every
        robot or (B, 2) per robot."""
        if self._plan_stale:
            self._fetch()
        nq, nv = self.nq, self.nv
        x = self.x_est
        xs0, us0, K0, ab = self._knot_in_force(self.xdot0[:, nv:nv + 6])
        d = np.concatenate([pin.difference_batch(self.model, x[:, :nq], xs0[:, :nq]), xs0[:, nq:] - x[:, nq:]], axis=1)  # space.difference(x_measured, xs[0])
        a0 = self.xdot0[:, nv:].copy()
        a0[:, :6] = ab
        a0[:, 6:] = us0[:, 12:] - np.einsum("bij,bj->bi", K0[:, 12:], d)
        forces = us0[:, :12] - np.einsum("bij,bj->bi", K0[:, :12], d)
        a_new, f_new, tau = self.qp.solve_batch_device(x, a0, forces, np.broadcast_to(np.asarray(cs, dtype=np.int32), (self.batch, 2)))
        tau = np.clip(tau, -self.umax, self.umax)
        self.x = self.sim.simulate_torque(self.x, tau, 1, self.sim_dt)
        self.torques, self.forces = self.sim_models.applied_torques(tau), f_new
        return tau

    def low_level_loop(self, cs):
        """The ``substeps`` low-level periods of one MPC period inside the library (mpc_qp_low_level_steps: feedback terms, QP, clamp and simulator step chained
        on the device, one synchronisation).  -> the measured states before the last period (the script reads x_measured BEFORE the last execute of the tick)."""
        self._device_contact_source(cs)
        cs_all = np.tile(np.asarray(cs, dtype=np.int32), (self.batch, 1))
        x_last, self.x, self.torques, self.forces = self.qp.low_level_steps(self.mpc.native, self.sim, cs_all, self.umax, self.substeps, self.sim_dt, x=self.x)
        return x_last

    def tick(self, host_glue=False, push=None):
        """One MPC period: the low-level loop on the current plan, then the next solve from the measurement of the tick before.  ``host_glue``: the low-level
        periods one at a time with the small vectors travelling through the host (``low_level_step``: the readable form, what the library call is tested against).
        ``push``: (B, 3) world force at the base origin or (B, 6) (force, world point), armed on the simulator for the low-level steps of this period
        only (mpc_sim_set_push, HIP library; ``push_schedule``)."""
        push = self._checked_push(push)
        self._latency_tick(host_glue)
        cs = self.contact_state()
        self._set_sim_contacts(cs)
        with self._pushed(push):
            if host_glue:
                if self._plan_stale:
                    self._fetch()
                for _ in range(self.substeps):
                    x_last = self.x_est.copy()    # (the script's x_measured is read BEFORE the last execute of the tick)
                    used = self._host_contact_set(cs)
                    self.low_level_step(used)
                    if self.contact_source != "schedule":
                        self.forces = _contact_rule.qp_zero_unused(self.forces, used)
            else:
                x_last = self.low_level_loop(cs)
        self._latency_publish(host_glue)
        return self._solve_from_x_prev(x_last)


# -- the centroidal pipeline ------------------------------------------------------------------------------------------------------------
def centroidal_state(model, x):
    """new_x = [com(q) ; hg.linear ; hg.angular] of whole-body states x [B][nq+nv] (centroidal_talos.py:420-424) -> [B][9]."""
    x = np.atleast_2d(np.asarray(x, dtype=float))
    data = model.createData()
    out = np.zeros((x.shape[0], 9))
    for b, xb in enumerate(x):
        out[b, :3] = pin.centerOfMass(model, data, xb[:model.nq])
        hg = pin.computeCentroidalMomentum(model, data, xb[:model.nq], xb[model.nq:])
        out[b, 3:6], out[b, 6:] = hg.linear, hg.angular
    return out


def posture_gains(nv):
    """Kp, Kd of the posture task (centroidal_talos.py:309-319: g_q * 10 and 2 sqrt(g_q * 10)).  The script's diagonal is written for the 28 dofs of
    the reduced model; for another model the base keeps the script's entries and every joint gets 1."""
    if nv == 28:
        g = np.array([0, 0, 0, 10, 10, 10] + [0.1] * 12 + [1, 1] + [10] * 8, dtype=float)
    else:
        g = np.array([0, 0, 0, 10, 10, 10] + [1.0] * (nv - 6), dtype=float)
    G = np.diag(g * 10)
    return G, 2 * np.sqrt(G)


class CentroidalPipeline(_QpContactSource):
    """The centroidal control pipeline of centroidal_talos.py:353-468 for an ensemble of robots, every stage on the solver library:

        MPC tick (centroidal OCP, x = [com ; h_lin ; h_ang], one ProxDDP iteration)
        -> the task errors of the IK + ID QP, once per period, at the stale measurement                        centroidal_talos.py:408-409
        -> 10 low-level steps of 1 ms, each:
             new_x = [com ; hg] of the measured whole-body state                                              :420-424
             forces = us[0] - K_0 (xs[0] - new_x)                                                             :434
             IK + ID QP (IKIDSolver_f6) assembled and solved on the device, no clamp (the QP's torque box)    :435-446
             one simulator step under the QP's torque                                   (mpc_simulate_torque) :447 (device.execute)
        -> x0 = new_x of the measurement before the last execute, then the solve                              :454-462

    The order of one period is the script's, which is not the kinodynamic one (``tick``):
      1. the foot references of tick t are planned and written into the contact maps (``EnsembleMPC.plan_tick``, :357-384); ``contact_state``
         is read from ``problem.stages[0]`` BEFORE ``replaceStageCircular(stages_full[t])`` (:386);
      2. the task errors are computed at the stale measurement — the one taken before the last execute of the previous period (``x_prev``),
         with the reference samples LF_refs[0:2], RF_refs[0:2] of this tick and dH = xdot[3:9] of the current plan's knot 0 (:408-409);
      3. the ten steps run on the current (previous tick's) plan;
      4. only then is x0 = new_x of this period's last measurement set (``c_prev``), the stage of tick t rotated in and the solve run
         (``EnsembleMPC.solve_tick``, :454-462).
    The centroidal OCP has no whole-body model: by default one set of references, which follows the previous references, serves every robot
    (``EnsembleMPC.enable_walk``).  ``walk=dict(per_instance=True)``: every robot's footholds are planned from the soles of ITS stale measurement
    ``x_prev``, as the script plans from ``rdata.oMf`` (:369-371), and its task errors are taken against its own samples; with ``generator="device"``
    the generator is one kernel per tick that reads ``x_prev`` where the device loop kept it (include/mpc_walk_poses.h).  The measured robots
    start from ``robot.x0``, perturbed as the kinodynamic pipeline's ensemble (``ensemble_initial_states``); the MPC starts from their centroidal
    states.  The simulator is the kinodynamic pipeline's stand-in (``build_torque_simulator``).  ``library``: the HIP library by default; the device
    loop (``low_level_loop``) is HIP only, the host glue (``tick(host_glue=True)``) runs on either library."""

    WEIGHTS = (500.0, 50000.0, 10.0, 1000.0, 100.0)   # posture, foot pose, centroidal, base / torso rotation, force (centroidal_talos.py:325)
    G_FOOT, G_ROT = 400.0, 10.0                        # g_p, g_b (:305-307)

    def __init__(self, problem_def, batch=1, library=None, walk=None, substeps=10, sim_dt=1e-3, x0=None, seed=20250304, perturb=True, sigma_q=0.02,
                 sigma_v=0.05, perturb_dofs=None, contact_rule=None, terrain=None, contact_source="schedule", actuators=None, sensors=None,
                 estimator=None, foot_sensors=None, detected_contacts=(), plant=None, friction=None, disturbances=None, latency=None, tipping=None, joint_stops=None, **ens_kw):
        """``problem_def``: a CentroidalProblem.  ``walk``: keyword arguments of ``EnsembleMPC.enable_walk`` ({} = the script's 0.2 m steps, one plan for
        every robot; ``dict(per_instance=True)``: every robot's own, from its measured soles; with ``generator="device"`` planned on the device) or None
        (references frozen at the initial footholds).  ``x0``: explicit whole-body initial states [B][nq+nv].  ``contact_rule``: None or a config
        dict, ``terrain``: None or boxes, ``contact_source``: "schedule", "plant" or "both", ``actuators``: None or the rows of the actuator model,
        ``sensors``: None or the rows of the sensor model, ``estimator``: None or the rows of the base-state estimator, ``foot_sensors``: None or the
        rows of the foot force sensors, ``detected_contacts``: who works from the detected contacts, ``plant``: None or the rows of the plant model,
        ``friction``: None or the rows of the ground friction, ``tipping``: None or the rows of the sole tipping, ``joint_stops``: None or the rows of the joint end-stops, ``latency``: None or the rows of
        the plan's hand-over latency (module docstring)."""
        from .ensemble import ensemble_initial_states
        walk, detected_contacts = self._check_arguments(problem_def, batch, contact_rule, terrain, walk, friction, foot_sensors, detected_contacts,
                                                        contact_source, disturbances=disturbances, latency=latency, tipping=tipping)
        plant = _checked_plant(plant, self.batch, problem_def)
        self._load(library, substeps, sim_dt)
        rb, m = problem_def.robot, self.model
        self.ref_dt = float(problem_def.dt)
        if x0 is not None:
            self.x = np.array(np.broadcast_to(np.asarray(x0, dtype=float), (self.batch, m.nq + m.nv)))
        elif perturb:
            self.x = ensemble_initial_states(rb.x0, _manifolds.MultibodyPhaseSpace(m), self.batch, seed, sigma_q, sigma_v, perturb_dofs)
        else:
            self.x = np.tile(rb.x0, (self.batch, 1))
        self.x_posture = np.array(rb.x0, dtype=float)     # x0_multibody: the posture reference of compute_ID_references
        self.c_prev = centroidal_state(m, self.x)          # the next solve's initial condition
        self.mpc = EnsembleMPC(problem_def, batch=batch, library=self.lib, x0=self.c_prev, **ens_kw)
        self._walk_args = walk
        Kq = posture_gains(m.nv)
        gains = [Kq, (np.eye(6) * self.G_FOOT, np.eye(6) * 2 * np.sqrt(self.G_FOOT)), None,
                 (np.eye(3) * self.G_ROT, np.eye(3) * 2 * np.sqrt(self.G_ROT))]
        self.qp = qp_utils.IKIDSolver_f6(m, list(self.WEIGHTS), gains, 2, common.FRICTION_MU, common.FOOT_HALF_LENGTH, common.FOOT_HALF_WIDTH,
                                         list(rb.foot_frame_ids), m.getFrameId("base_link"), m.getFrameId("torso_2_link"), 6, library=self.lib,
                                         batch=self.batch)
        self.qp.enable_device_assembly()
        # (the schedule starts in double support; ``x_prev`` is the stale measurement the task errors are taken at)
        self._build_simulator(plant, friction, actuators, sensors, foot_sensors, detected_contacts, estimator, stage0=(True, True), tipping=tipping,
                              joint_stops=joint_stops)
        self.forces = np.zeros((self.batch, 12))
        self.ik = None                 # the task errors of the last period
        self._xik_on_device = False    # the QP handle keeps x_prev of its last device loop

    def _walk_kwargs(self):
        kw = dict(self._walk_args)
        if kw.get("per_instance") and kw.get("generator") == "device":
            kw.setdefault("model_handle", self.sim)   # the forward kinematics of the soles run on the simulator handle's model tables
        return kw

    def _fetch(self):
        super()._fetch()
        self.dH = self.mpc.native.get_stage_data(0)[0][:, 3:9].copy()

    def contact_state(self):
        """[left, right] of ``problem.stages[0]`` as the script reads it (centroidal_talos.py:386): after the references of tick t are written and
        BEFORE ``replaceStageCircular(stages_full[t])`` — the stage that was appended at tick t - N (the initial double support before that), the
        stage of knot 0 of the plan the feedback terms come from."""
        N, t = self.mpc.problem.num_steps, self.mpc.tick
        return self.pd.contact_phases[max(0, t - N) % self.pd.t_mpc]

    def foot_refs(self):
        """[B][2 feet][2 samples][12]: LF_refs[0:2], RF_refs[0:2] of this tick (R row-major, p); without a walk the initial footholds, twice.  With
        ``walk=dict(per_instance=True)`` every robot's own (``generator="device"``: fetched from the device, where the device loop reads them)."""
        w = self.mpc._walk
        if w is not None and w.get("poses"):
            if w["poses"] == "device":
                return self.mpc.native.walk_poses_samples()
            if w["refs_all"] is not None:
                return w["refs_all"]
        pair = w["refs"] if (w is not None and "refs" in w) else tuple([M, M] for M in self.pd.robot.foot_placements)
        flat = lambda M: np.concatenate([np.asarray(M.rotation, dtype=float).reshape(-1), np.asarray(M.translation, dtype=float)])
        one = np.array([[flat(M) for M in pair[f][:2]] for f in range(2)])
        return np.ascontiguousarray(np.broadcast_to(one, (self.batch, 2, 2, 12)))

    def low_level_step(self, cs, ik):
        """One 1 kHz step of centroidal_talos.py:420-447 for every robot, the glue between the library calls on the host (``cs``: (2,) for every
        robot or (B, 2) per robot).  -> new_x of the measurement the step started from."""
        if self._plan_stale:
            self._fetch()
        x = self.x_est
        new_x = centroidal_state(self.model, x)
        xs0, us0, K0 = self._knot_in_force()
        forces = us0 - np.einsum("bij,bj->bi", K0, xs0 - new_x)   # us[0] - K_0 difference(new_x, xs[0])
        _, f_new, tau = self.qp.solve_batch_device_ik(x, ik, forces, np.broadcast_to(np.asarray(cs, dtype=np.int32), (self.batch, 2)))
        self.x = self.sim.simulate_torque(self.x, tau, 1, self.sim_dt)
        self.torques, self.forces = self.sim_models.applied_torques(tau), f_new
        return new_x

    def low_level_loop(self, cs, refs):
        """The ``substeps`` low-level periods of one MPC period inside the library (mpc_qp_ikid_low_level_steps: task errors, centroidal state,
        feedback forces, QP and simulator step chained on the device, one synchronisation)."""
        self._device_contact_source(cs)
        cs_all = np.tile(np.asarray(cs, dtype=np.int32), (self.batch, 1))
        x_ik = None if self._xik_on_device else self.x_prev
        self.x_prev, self.c_prev, self.x, self.torques, self.forces, self.ik = self.qp.low_level_steps(
            self.mpc.native, self.sim, self.x_posture, refs, self.ref_dt, cs_all, self.substeps, self.sim_dt, x=self.x, x_ik=x_ik, want_ik=True)
        self._xik_on_device = True

    def tick(self, host_glue=False, push=None):
        """One MPC period in the script's order (class docstring).  ``host_glue``: the task errors from ``references.compute_ID_references`` and
        the low-level periods one at a time with the small vectors travelling through the host (``low_level_step``: the readable form, what the
        library call is tested against).  ``push``: (B, 3) world force at the base origin or (B, 6) (force, world point), armed on the simulator for
        the low-level steps of this period only (mpc_sim_set_push, HIP library; ``push_schedule``)."""
        push = self._checked_push(push)
        self._latency_tick(host_glue)
        e = self.mpc
        cs = self.contact_state()
        w = e._walk
        on_device = w is not None and w.get("poses") == "device"
        if w is not None and w.get("poses"):
            # every robot plans from the soles of its stale measurement (what rdata holds at centroidal_talos.py:369-371); the device generator reads
            # it where the device loop kept it, so nothing per robot travels for the references
            keep = on_device and not host_glue and self._xik_on_device
            w["x_measured_all"], w["xik_from"] = (None, self.qp.qp) if keep else (self.x_prev, None)
        e.plan_tick()
        refs = None if (on_device and not host_glue) else self.foot_refs()
        self._set_sim_contacts(cs)
        with self._pushed(push):
            if host_glue:
                if self._plan_stale:
                    self._fetch()
                first = self._latency_first()    # (dH of the record every robot's first step of the period reads)
                dH = self.dH if first is None or not first.any() else np.where(first[:, None], self._lat_held["xdot"], self.dH)
                self.ik = self.qp.task_errors(self.x_prev, self.x_posture, refs, self.ref_dt, dH)
                for _ in range(self.substeps):
                    x_last = self.x_est.copy()    # (the script's x_measured is read BEFORE the last execute of the period)
                    used = self._host_contact_set(cs)
                    c_last = self.low_level_step(used, self.ik)
                    if self.contact_source != "schedule":
                        self.forces = _contact_rule.qp_zero_unused(self.forces, used)
                self.x_prev, self.c_prev = x_last, c_last
                self._xik_on_device = False
            else:
                self.low_level_loop(cs, refs)
        self._latency_publish(host_glue)
        e.native.set_x0(self.c_prev)
        st = e.solve_tick()
        self._plan_stale = True   # (knot 0 of the new plan is read on the device; the host copies only when the host glue asks)
        return st


# -- the full-dynamics pipeline ---------------------------------------------------------------------------------------------------------
class FullDynamicPipeline(_Pipeline):
    """The full-dynamics control pipeline of fulldynamic_talos.py:437-550 for an ensemble of robots, every stage on the solver library:

        MPC tick (full-dynamics OCP, one ProxDDP iteration)                                                    fulldynamic_talos.py:536-541
        -> 10 low-level steps of 1 ms, each:
             measured state of every robot                                                                     :514-520
             tau = us[0] - K_0 difference(x_measured, xs[0]), no clamp                                         :522
             one simulator step under that torque                                       (mpc_simulate_torque)  :523 (device.execute)
        -> the measurement of the period before becomes the initial condition of the next solve               :534-546

    The order of one period (``tick``) is the script's: the loop runs on the previous plan; the walk references are planned from ``x_prev`` (the
    measurement before the last execute of the period before, :440-462); x0 = ``x_prev`` and the solve; ``x_prev`` becomes the measurement
    before the last execute of this period.  Unlike ``EnsembleMPC(closed_loop=...)`` (mpc_simulate: knot 0's own model integrated from xs[0]) the
    measured robots carry over from period to period on the torque-driven simulator the other two pipelines use (``build_torque_simulator``, the
    contact set of ``contact_state``).  ``library``: the HIP library by default; the device loop (``low_level_loop``,
    mpc_feedback_low_level_steps) is HIP only, the host glue (``tick(host_glue=True)``) runs on either library."""

    def __init__(self, problem_def, batch=1, library=None, walk=None, substeps=10, sim_dt=1e-3, x0=None, contact_rule=None, terrain=None, actuators=None,
                 sensors=None, estimator=None, foot_sensors=None, detected_contacts=(), plant=None, friction=None, disturbances=None, latency=None, tipping=None,
                 joint_stops=None, **ens_kw):
        """``problem_def``: a FullDynamicsProblem (reduced or complete model).  ``walk``: keyword arguments of ``EnsembleMPC.enable_walk``
        ({} = the script's steps) or None (references frozen at the initial footholds).  ``ens_kw``: EnsembleMPC's, but not ``closed_loop``:
        the pipeline is the closed loop.  ``contact_rule``: None or a config dict, ``terrain``: None or boxes, ``actuators``: None or the rows of the
        actuator model, ``sensors``: None or the rows of the sensor model, ``estimator``: None or the rows of the base-state
        estimator, ``foot_sensors``: None or the rows of the foot force sensors, ``detected_contacts``: () or ("estimator",), ``plant``: None or the rows of the plant
        model, ``friction``: None or the rows of the ground friction, ``tipping``: None or the rows of the sole tipping, ``joint_stops``: None or the rows of the joint end-stops, ``latency``: None or the rows of the plan's hand-over latency (module docstring
        of pipeline.py)."""
        walk, detected_contacts = self._check_arguments(problem_def, batch, contact_rule, terrain, walk, friction, foot_sensors, detected_contacts,
                                                        disturbances=disturbances, latency=latency, tipping=tipping)
        if ens_kw.get("closed_loop") is not None:
            raise ValueError("FullDynamicPipeline: closed_loop is not an option here (the pipeline's simulator is the closed loop; "
                             "EnsembleMPC(closed_loop=...) would simulate a second time)")
        ens_kw.pop("closed_loop", None)
        plant = _checked_plant(plant, self.batch, problem_def)
        self._load(library, substeps, sim_dt)
        self.mpc = EnsembleMPC(problem_def, batch=batch, library=self.lib, x0=x0, **ens_kw)
        self._walk_args = walk
        self.x = np.array(self.mpc.x0, dtype=float)      # measured states, one row per robot
        self._build_simulator(plant, friction, actuators, sensors, foot_sensors, detected_contacts, estimator, tipping=tipping,
                              joint_stops=joint_stops)
        self.wrenches = np.zeros((self.batch, 2, 6))     # contact wrenches of the last simulator step (LOCAL frame of the sole)

    def low_level_step(self, cs):
        """One 1 kHz step of fulldynamic_talos.py:514-523 for every robot, the feedback law on the host (``cs``: the simulator's contact set is
        set by ``tick``).  -> the torques."""
        if self._plan_stale:
            self._fetch()
        nq = self.nq
        x = self.x_est
        xs0, us0, K0 = self._knot_in_force()
        d = np.concatenate([pin.difference_batch(self.model, x[:, :nq], xs0[:, :nq]), xs0[:, nq:] - x[:, nq:]], axis=1)  # space.difference(x_measured, xs[0])
        tau = us0 - np.einsum("bij,bj->bi", K0, d)
        self.x, wr = self.sim.simulate_torque(self.x, tau, 1, self.sim_dt, wrenches=True)
        self.torques, self.wrenches = self.sim_models.applied_torques(tau), wr
        return tau

    def low_level_loop(self, cs):
        """The ``substeps`` low-level periods of one MPC period inside the library (mpc_feedback_low_level_steps: feedback kernel and simulator step
        chained on the device, one synchronisation).  -> the measured states before the last period."""
        x_last, self.x, self.torques, self.wrenches = self.mpc.native.feedback_low_level_steps(self.sim, self.substeps, self.sim_dt, x=self.x)
        return x_last

    def tick(self, host_glue=False, push=None):
        """One MPC period in the script's order (class docstring).  ``host_glue``: the low-level periods one at a time with the small vectors
        travelling through the host (``low_level_step``: the readable form, what the library call is tested against).  ``push``: (B, 3) world force
        at the base origin or (B, 6) (force, world point), armed on the simulator for the low-level steps of this period only (mpc_sim_set_push,
        HIP library; ``push_schedule``)."""
        push = self._checked_push(push)
        self._latency_tick(host_glue)
        cs = self.contact_state()
        self._set_sim_contacts(cs)
        with self._pushed(push):
            if host_glue:
                if self._plan_stale:
                    self._fetch()
                for _ in range(self.substeps):
                    x_last = self.x_est.copy()    # (x_measured_prev is read BEFORE the last execute of the period)
                    self.low_level_step(cs)
            else:
                x_last = self.low_level_loop(cs)
        self._latency_publish(host_glue)
        return self._solve_from_x_prev(x_last)
