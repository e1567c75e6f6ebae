"""Headless stand-in for the reference's ``bullet_robot.BulletRobot`` ("next" row N2 of SURVEY.md §8f): the methods the three scripts call
(bullet_robot.py:15-24 constructor, :90 initializeJoints, :138-145 execute, :157-162 apply_force, :164-168 changeCamera, :172-196
measureState, plus the marker calls) with the PyBullet physics replaced by the solver library's own rigid-contact dynamics
(``mpc_simulate_torque``, include/mpc_abi.h): no GUI, no URDF, no PyBullet.

What it simulates: the CONTROLLED joints of the complete model (the others stay locked at the configuration handed to
``initializeJoints`` — in PyBullet they are held by the default position controller, bullet_robot.py:71-73), one semi-implicit Euler step
of ``simuStep`` per ``execute(torques)``, with the feet that stand on the ground held by 6-D rigid contacts with Baumgarte correction
(the contact model of fulldynamic_talos.py:84-96).  A foot is "on the ground" while its sole is within ``ground_tol`` of the ground
plane z = 0 ... and pushes on it: a contact whose normal force stays below ``-release_force`` for ``release_steps`` consecutive steps is released (a one-step
transient — the torque jump of the low-level QP when a stage changes its contact state — only unloads a real sole for a millisecond, it does not
lift it), a free foot that has left the ground and comes back to it, or that sinks below the ground plane, is caught there (its world-side
placement is re-captured at the landing pose).  That is a deliberately simple contact rule — enough to close the loop around the MPC headlessly
and deterministically; it is not a physics engine.  ``device_contacts=True`` (HIP library only) runs the same rule on the device after every step
(mpc_sim_contacts, include/mpc_sim_contacts.h): stage 0 stays the double-support stage, the rule picks the contacts and their ground-side
placements, and a catch needs no new model.  ``createStairs(pose_stairs, height_step)`` (the reference's three boxes) and ``setTerrain(boxes)`` put a
box terrain under the rule, host or device: a foot is caught on the highest box top under the ORIGIN of its sole frame (``contact_rule.terrain_height``);
risers, soles hanging over an edge and slopes are not modelled.  ``addStairs`` (a URDF in the reference) stays unavailable.
``actuators=`` / ``setActuators(params, limit=None, friction_shape=None)`` (HIP library only) put the actuator model of ``actuator_model`` between
``execute(torques)`` and the dynamics (mpc_sim_actuators, include/mpc_sim_actuators.h): delay, gain error, lag, saturation, joint friction.
``joint_stops=`` / ``setJointStops(params, lo=None, hi=None, scale=None)`` (HIP library only) give every controlled joint the end-stops of
``joint_stops`` (mpc_sim_joint_stops, include/mpc_sim_joint_stops.h), which Bullet applies to the revolute joints of the reference's URDF: a joint
beyond its range is pushed back by a one-sided spring and damper.  The range defaults to the model's position limits.  ``jointStopState()`` returns
the stop torques, penetrations and counters.  Without it every joint turns freely, as before.
``sensors=`` / ``setSensors(params)`` (HIP library only) put the sensor model of ``sensor_model`` between the dynamics and ``measureState()``
(mpc_sim_sensors, include/mpc_sim_sensors.h): latency, encoder resolution, calibration offsets, noise, finite-difference velocities.  ``x``, the
contact rule and ``history`` stay the true state; ``measureState()`` returns the measurement.
``estimator=`` / ``setEstimator(params)`` (HIP library only, with ``device_contacts=True``) put the base-state estimator of ``state_estimator`` after
the sensors (mpc_sim_estimator, include/mpc_sim_estimator.h): the base position and linear velocity by leg odometry through the soles the rule
holds, blended with the measurement; ``measureState()`` then returns the estimate.
``foot_sensors=`` / ``setFootSensors(params, detected_contacts=())`` (HIP library only, with ``device_contacts=True``) measure the contact wrenches of
every step and run the contact detector of ``foot_sensors`` on them (mpc_sim_foot_sensors, include/mpc_sim_foot_sensors.h); ``detectedContacts()``
is the pair the robot takes to stand, and ``detected_contacts=("estimator",)`` lets the estimator work from it.  ``in_contact`` stays the plant's.
``plant=`` / ``setPlant(rows, link_scale=None)`` (HIP library only) give the simulated robot other link inertias than ``model`` holds (``plant_model``:
a payload, a mass error, a displaced centre of mass; mpc_sim_plant, include/mpc_sim_plant.h).  ``model`` stays the nominal one, what a controller is
built from; ``plantModel()`` is what is integrated.  The host contact rule lowers the model again at every catch: the library rebuilds the plant's
table from the rows in force.
``friction=`` / ``setFriction(rows)`` (HIP library only, with ``device_contacts=True``) make every held sole a Coulomb slider (``friction_model``;
mpc_sim_friction, include/mpc_sim_friction.h): a sole whose tangential force leaves the cone ``mu f_z`` slips, and turns when its yaw moment leaves
``mu_spin f_z``.  ``setFrictionCoefficients(link_id, lateral, spinning)``, the reference's knob, sets ``mu`` and ``mu_spin`` of one sole.  Without
either every sole holds whatever force it takes, as before.
``tipping=`` / ``setTipping(rows)`` (HIP library only, with ``device_contacts=True``) make every held sole a rectangle that rolls about an edge
(``tipping_model``; mpc_sim_tipping, include/mpc_sim_tipping.h): a sole whose roll moment leaves ``half_width f_z`` or whose pitch moment leaves
``half_length f_z`` tips about the edge where the centre of pressure saturates.  ``tippingState()`` returns the tip velocities, angles and counters.
Without it every sole transmits whatever moment it takes, as before.
``disturbances=`` / ``setDisturbances(events)`` (HIP library only) give the robot a schedule of pushes on any link, timed on the device by the
simulator's step clock or by the touchdowns and lift-offs of its soles (``disturbance_model``; mpc_sim_disturbances,
include/mpc_sim_disturbances.h; contact triggers need ``device_contacts=True``).  ``disturbanceState()`` returns the clock, the counters and what
acted.  While a schedule is armed ``apply_force`` is refused: its events are the pushes.

Differences from PyBullet worth knowing: ``measureState`` returns the base velocity in the LOCAL frame of the base (Pinocchio's
convention, which is what the scripts assume when they copy it into the state, talos_utils.py:337-348); PyBullet reports it in the
world frame."""
from __future__ import annotations

import numpy as np

from . import contact_rule as _contact_rule
from . import friction_model as _friction_model
from . import plant_model as _plant_model
from . import torque_simulator as _tsim
from .robot import minipin as pin


class BulletRobot:
    record_default = False  # tools: keep (state, contact flags, sole heights) of every step in ``history``

    def __init__(self, controlledJoints, modelPath=None, URDF_filename=None, simuStep=1e-3, rmodelComplete=None, robotPose=(0.0, 0.0, 1.01927),
                 inertiaOffset=True, talos=True, library=None, contact_frames=("left_sole_link", "right_sole_link"), ground_tol=5e-3, release_steps=5, release_force=1.0,
                 device_contacts=False, actuators=None, sensors=None, estimator=None, foot_sensors=None, plant=None, friction=None, disturbances=None,
                 tipping=None, joint_stops=None):
        if rmodelComplete is None:
            raise ValueError("the complete robot model is needed (5th positional argument, as in the scripts)")
        self._lib = library
        self.dt = float(simuStep)
        self.complete = rmodelComplete
        self.controlled = [n for n in controlledJoints if n not in ("universe", "root_joint")]
        self.contact_frames = tuple(contact_frames)
        self.ground_tol = float(ground_tol)
        self.release_steps = int(release_steps)
        self.release_force = float(release_force)  # N: the ground "pulls" when the normal force is below minus this
        self.device_contacts = bool(device_contacts)  # the contact rule on the device (in_contact and the rest are read back after every step)
        self.terrain = None  # boxes (n, 5) under the contact rule (setTerrain / createStairs); None: the plane z = ground_z
        self._actuators = None if actuators is None else (actuators, None, None)  # (params, limit, friction_shape) of setActuators, armed at initializeJoints
        self._sensors = sensors  # params of setSensors, armed at initializeJoints
        self._estimator = estimator  # params of setEstimator, armed at initializeJoints after the sensors
        self._foot_sensors = None if foot_sensors is None else (foot_sensors, ())  # (params, detected_contacts) of setFootSensors, armed at initializeJoints
        self._plant = None if plant is None else (plant, None)  # (rows, link_scale) of setPlant, armed at initializeJoints
        self._friction = friction  # rows of setFriction, armed at initializeJoints
        self._tipping = tipping  # rows of setTipping, armed at initializeJoints
        self._joint_stops = None if joint_stops is None else (joint_stops, None, None, None)  # (params, lo, hi, scale) of setJointStops, armed at initializeJoints
        self._disturbances = disturbances  # events of setDisturbances, armed at initializeJoints
        self.robotPose = np.asarray(robotPose, dtype=float)
        self.localInertiaPos = np.zeros(3)
        self._native = None       # the simulator handle, and ``_sim_models``, the models armed on it (``torque_simulator.SimulatorModels``)
        self._sim_models = None
        self._pending_force = None
        self.markers = None
        self.camera = None
        self.steps = 0
        self.trace_from = None     # tools: print contact forces from this step on
        self.max_steps = None      # tools: stop a script's endless loop after this many execute() calls
        self.history = []          # (q, v) after every step when ``record`` is set
        self.record = bool(self.record_default)

    # -- model ------------------------------------------------------------------------------------------------------------------
    def initializeJoints(self, q0CompleteStart):
        mc = self.complete
        q0 = np.array(q0CompleteStart, dtype=float).reshape(-1)
        self.q_complete = q0.copy()
        self.v_complete = np.zeros(mc.nv)
        keep = set(self.controlled)
        locked = [j for j in range(2, mc.njoints) if mc.names[j] not in keep]
        self.model = pin.buildReducedModel(mc, locked, q0) if locked else mc
        m = self.model
        # complete <-> reduced coordinate maps (joint i >= 2 of the complete model has q index i + 5, v index i + 4)
        self._qmap = [(mc.joints[mc.getJointId(n)].idx_q, m.joints[m.getJointId(n)].idx_q) for n in m.names[2:]]
        self._vmap = [(mc.joints[mc.getJointId(n)].idx_v, m.joints[m.getJointId(n)].idx_v) for n in m.names[2:]]
        self.x = np.zeros(m.nq + m.nv)
        self.x[:7] = q0[:7]
        for src, dst in self._qmap:
            self.x[dst] = q0[src]
        self.data = m.createData()
        pin.framesForwardKinematics(m, self.data, self.x[:m.nq])
        self.frame_ids = [m.getFrameId(n) for n in self.contact_frames]
        self.ground_z = min(float(self.data.oMf[f].translation[2]) for f in self.frame_ids)
        self.in_contact = [True, True]
        self._z_prev = [float(self.data.oMf[f].translation[2]) for f in self.frame_ids]
        self._lifted = [False, False]
        self._pulling = [0, 0]   # consecutive steps with a negative normal force
        self._contact_pose = [self.data.oMf[f].copy() for f in self.frame_ids]
        self._refuse_friction_without_rule(self._friction)
        self._refuse_tipping_without_rule(self._tipping)
        self._build_native()
        if self.device_contacts:  # stage 0 is double support once; the rule on the device picks each step's contacts
            self._upload_mask()
            self._native.contacts({"ground_z": self.ground_z, "ground_tol": self.ground_tol, "release_force": self.release_force,
                                   "release_steps": self.release_steps})
            if self.terrain is not None:
                self._native.terrain(self.terrain)
        self._sim_models = _tsim.SimulatorModels(self._native, m, self.frame_ids, self.dt)
        self._sim_models.arm(self.x, self.x[:m.nq], self._plant, self._friction, self._actuators, self._sensors, self._foot_sensors, self._estimator,
                             None if self._disturbances is None else (self._disturbances, self.device_contacts), tipping=self._tipping,
                             joint_stops=self._joint_stops)

    def _build_native(self):
        """the handle (opened once) with the model, the terminal stage and the contact-mask stages at the anchors ``_contact_pose`` as they stand"""
        frames = self.model.frames
        contacts = [(name, frames[fid].parentJoint, frames[fid].placement, pose)
                    for name, fid, pose in zip(self.contact_frames, self.frame_ids, self._contact_pose)]
        self._native, self._stage_tables = _tsim.build_simulator(self._lib, self.model, contacts, 1, self.dt, 0, sim=self._native)
        self._mask_uploaded = None

    def _upload_mask(self):
        mask = tuple(bool(c) for c in self.in_contact)
        if mask == (False, False):
            raise RuntimeError("headless BulletRobot: both feet off the ground (flight phases are not simulated)")
        self._mask_uploaded = _tsim.upload_stage0(self._native, self._stage_tables, mask, self._mask_uploaded)

    # -- simulation -------------------------------------------------------------------------------------------------------------
    def execute(self, torques):
        if self.max_steps is not None and self.steps >= self.max_steps:
            raise StopIteration("headless BulletRobot: step budget of %d reached" % self.max_steps)
        tau = np.asarray(torques, dtype=float).reshape(-1)
        m = self.model
        if tau.size != m.nv - 6:
            raise ValueError("expected %d joint torques, got %d" % (m.nv - 6, tau.size))
        if not self.device_contacts:
            self._upload_mask()
        push = self._pending_force
        if push is not None:  # (apply_force: the push of the scripts, e.g. kinodynamic_talos.py:459-461 — a world force at a world point, this step only)
            if not hasattr(self._native.lib, "mpc_sim_set_push"):
                raise NotImplementedError("apply_force needs the HIP library (libmpc_hip.so, mpc_sim_set_push of include/mpc_sim_ext.h): %s does not "
                                          "export it; mpc_simulate_push through EnsembleMPC pushes the full-dynamics loop on either library" % self._native.backend)
            self._native.set_push(np.concatenate([push[0], push[1]]))
        try:
            x, wr = self._native.simulate_torque(self.x, tau, 1, self.dt, wrenches=True)
        finally:
            if push is not None:
                self._pending_force = None
                self._native.set_push(None)
        self.x = x[0]
        self.steps += 1
        if self.trace_from is not None and self.steps >= self.trace_from:
            import sys
            sys.stderr.write("   [sim] step %d in_contact %s fz L %.2f R %.2f z %s\n" % (self.steps, self.in_contact, wr[0][0][2], wr[0][1][2], ["%.4f" % v for v in self._z_prev]))
        if self.device_contacts:
            self._read_device_contacts()
        else:
            self._update_contacts(wr[0])
        if self.record:
            self.history.append((self.x.copy(), tuple(self.in_contact), tuple(self._z_prev)))

    def _update_contacts(self, wrenches):
        """Unilateral contact by rule: an active contact whose normal force turned negative is released (the ground cannot pull); a free
        foot that is moving down and reaches the ground plane is caught at the pose it lands with (flattened onto the ground)."""
        m = self.model
        pin.framesForwardKinematics(m, self.data, self.x[:m.nq])
        relanded = False
        for i, fid in enumerate(self.frame_ids):
            z = float(self.data.oMf[fid].translation[2])
            ground_z = self._ground_under(self.data.oMf[fid].translation)
            if self.in_contact[i]:
                self._pulling[i] = self._pulling[i] + 1 if wrenches[i][2] < -self.release_force else 0  # (an unloaded sole, 0 +- round-off, rests on the ground)
                if self._pulling[i] >= self.release_steps and sum(self.in_contact) > 1:
                    self.in_contact[i] = False
                    self._lifted[i] = False
                    self._pulling[i] = 0
            elif z > ground_z + 2.0 * self.ground_tol:
                self._lifted[i] = True  # (a released foot is caught again only after it has really left the ground ...)
            elif (z <= ground_z + self.ground_tol and self._lifted[i]) or (z < ground_z and z < self._z_prev[i]):  # (... or sinks into it)
                pose = self.data.oMf[fid].copy()
                pose.translation[2] = ground_z
                yaw = np.arctan2(pose.rotation[1, 0], pose.rotation[0, 0])
                c, s = np.cos(yaw), np.sin(yaw)
                pose.rotation = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
                self._contact_pose[i] = pose
                self.in_contact[i] = True
                relanded = True
            self._z_prev[i] = z
        if relanded:
            self._build_native()

    def _ground_under(self, p):
        """height of the ground under the point p: the plane, or the terrain at (x, y) (the origin of a sole frame decides, nothing else of the sole)"""
        if self.terrain is None:
            return self.ground_z
        return float(_contact_rule.terrain_height(self.terrain, np.asarray(p, dtype=float)[:2], self.ground_z))

    def _read_device_contacts(self):
        """``in_contact`` and the rule's per-foot state after a step, from the device rows (mpc_sim_contacts_read)."""
        r = self._native.read_contacts()
        self.in_contact = [bool(v) for v in r["in_contact"][0]]
        self._lifted = [bool(v) for v in r["lifted"][0]]
        self._pulling = [int(v) for v in r["pulling"][0]]
        self._z_prev = [float(v) for v in r["z_prev"][0]]

    def measureState(self):
        """-> (q, v) of the COMPLETE model (bullet_robot.py:172-196): locked joints at their initial positions, zero velocity."""
        m = self.model
        x = self.x if self._sim_models is None else np.reshape(self._sim_models.x_est(self.x), -1)   # (the estimate, the measurement or the true state)
        q, v = self.q_complete.copy(), self.v_complete.copy()
        q[:7] = x[:7]
        v[:6] = x[m.nq:m.nq + 6]
        for src, dst in self._qmap:
            q[src] = x[dst]
        for src, dst in self._vmap:
            v[src] = x[m.nq + dst]
        return q, v

    def resetState(self, q0Start):
        m = self.model
        self.x[:m.nq] = np.asarray(q0Start, dtype=float)[:m.nq]
        self.x[m.nq:] = 0.0
        if self._sim_models is not None:
            if self._sensors is not None:  # (an imposed state: the sensor model is armed again, on it, and the estimator after the sensors)
                self._sim_models.set_sensors(self._sensors, self.x)
            elif self._estimator is not None:
                self._sim_models.set_estimator(self._estimator, self.x)

    def apply_force(self, force, position):
        """PyBullet's applyExternalForce(robot, -1, force, position, WORLD_FRAME): a world-frame force on the base link at a world point, acting
        during the NEXT ``execute`` only (the scripts call it after every execute of their push window).  HIP library only (mpc_sim_set_push)."""
        f = np.asarray(force, dtype=float).reshape(-1)
        p = np.asarray(position, dtype=float).reshape(-1)
        if f.size != 3 or p.size != 3:
            raise ValueError("apply_force: a 3-vector force and a 3-vector world position expected")
        if self._disturbances is not None:
            raise ValueError("apply_force: a push schedule is armed on this robot (setDisturbances): its events are the pushes; setDisturbances(None) "
                             "turns it off")
        self._pending_force = (f, p)

    # -- GUI calls of the scripts: recorded, nothing to draw ------------------------------------------------------------------------
    def changeCamera(self, cameraDistance, cameraYaw, cameraPitch, cameraTargetPos):
        self.camera = (cameraDistance, cameraYaw, cameraPitch, tuple(cameraTargetPos))

    def showTargetToTrack(self, LF_pose, RF_pose):
        self.markers = (np.array(LF_pose.translation), np.array(RF_pose.translation))

    def moveMarkers(self, LF_trans, RF_trans):
        self.markers = (np.array(LF_trans), np.array(RF_trans))

    def showQuadrupedFeet(self, *poses):
        self.markers = tuple(np.array(p.translation) for p in poses)

    def moveQuadrupedFeet(self, *trans):
        self.markers = tuple(np.array(t) for t in trans)

    def setFrictionCoefficients(self, link_id, lateral_friction, spinning_friction):
        """bullet_robot.py of the reference: ``changeDynamics(robot, link_id, lateralFriction=..., spinningFriction=...)``.  Here ``mu`` and
        ``mu_spin`` of one sole of the friction model (``setFriction``; it is turned on with the other sole at the identity if it was off):
        ``link_id`` 0 / 1 (left, right), or the frame id or the joint id of a sole in ``model`` once ``initializeJoints`` has built it.  Any other
        link has no contact model here: a no-op, as before."""
        sole = self._sole_of(link_id)
        if sole is None:
            return
        rows = dict(self._friction) if isinstance(self._friction, dict) else \
            ({} if self._friction is None else dict(zip(_friction_model.FIELDS, _friction_model.rows(self._friction, 1)[0])))
        for short in _friction_model.BOTH:   # (a dict given with the shorthands: spelled out per sole before one sole is changed)
            if short in rows:
                v = rows.pop(short)
                rows.setdefault(short + "_left", v), rows.setdefault(short + "_right", v)
        side = ("left", "right")[sole]
        rows["mu_" + side], rows["mu_spin_" + side] = float(lateral_friction), float(spinning_friction)
        self.setFriction(rows)

    def _sole_of(self, link_id):
        """0 / 1 for the ids ``setFrictionCoefficients`` takes for the left / right sole, None for any other"""
        link_id = int(link_id)
        if link_id in (0, 1):
            return link_id
        if self._native is not None:
            for i, fid in enumerate(self.frame_ids):
                if link_id in (fid, self.model.frames[fid].parentJoint):
                    return i
        return None

    def setFriction(self, rows):
        """The ground friction under the soles (``friction_model``; HIP library only, needs ``device_contacts=True``): ``rows`` one row of 8, (1, 8),
        or a dict by field name (``mu`` / ``mu_spin``: both soles; missing fields as in ``friction_model.defaults`` of this robot: coefficients
        +inf, slider masses from its mass and posture); None: off.  Arms the model with every sole at rest; before ``initializeJoints`` it is kept
        for then."""
        self._refuse_friction_without_rule(rows)
        self._friction = rows
        if self._sim_models is not None:
            self._sim_models.set_friction(rows, self.x[:self.model.nq])

    def setDisturbances(self, events):
        """The push schedule of the robot (``disturbance_model``; HIP library only): ``events`` an (n, 16) table, (1, n, 16), or a list holding one
        list of events; contact triggers need ``device_contacts=True``.  Arms the schedule and resets its clock; None turns it off."""
        if events is not None and self._pending_force is not None:
            raise ValueError("setDisturbances: a force of apply_force is pending for the next execute; execute it first")
        if self._sim_models is not None:
            self._sim_models.set_disturbances(events, self.device_contacts)
        self._disturbances = events

    def disturbanceState(self):
        """the state rows of the push schedule by ``disturbance_model.unpack`` (``step``, ``acting``, ``impulse`` ...); None without one"""
        return None if self._sim_models is None else self._sim_models.disturbance_state()

    def _refuse_friction_without_rule(self, rows):
        if rows is not None and not self.device_contacts:
            raise ValueError("setFriction: the friction model needs device_contacts=True (it slides the soles the device contact rule holds)")

    def frictionState(self):
        """the state rows of the friction model by ``friction_model.unpack`` (``v``, ``sliding``, ``slip_dist`` ...); None without one"""
        return None if self._sim_models is None else self._sim_models.friction_state()

    def setTipping(self, rows):
        """The sole tipping (``tipping_model``; HIP library only, needs ``device_contacts=True``): ``rows`` one row of 8, (1, 8), or a dict by field
        name (``half_length`` / ``half_width``: both soles; missing fields as in ``tipping_model.defaults`` of this robot: extents +inf, slider
        inertia from its mass and posture); None: off.  Arms the model with every sole flat and at rest; before ``initializeJoints`` it is kept for
        then."""
        self._refuse_tipping_without_rule(rows)
        self._tipping = rows
        if self._sim_models is not None:
            self._sim_models.set_tipping(rows, self.x[:self.model.nq])

    def _refuse_tipping_without_rule(self, rows):
        if rows is not None and not self.device_contacts:
            raise ValueError("setTipping: the tipping model needs device_contacts=True (it tips the soles the device contact rule holds)")

    def tippingState(self):
        """the state rows of the tipping model by ``tipping_model.unpack`` (``v``, ``th``, ``tipping``, ``peak_angle`` ...); None without one"""
        return None if self._sim_models is None else self._sim_models.tipping_state()

    def addStairs(self, path, position, orientation):
        raise NotImplementedError("headless BulletRobot: flat ground only")  # (a URDF staircase; createStairs / setTerrain lay boxes under the contact rule)

    def setTerrain(self, boxes):
        """The ground under the contact rule: boxes (n, 5) ``(x_lo, x_hi, y_lo, y_hi, z_top)``, n <= 16, over the plane z = ``ground_z``
        (``contact_rule.terrain_height``); None: the plane again.  The host rule takes it at once, ``device_contacts=True`` passes it to the device.
        What stands is not moved: a sole in contact keeps its anchor.  Only the height under the ORIGIN of a sole frame counts: no risers, no sole
        edges hanging over a step, no slopes."""
        if boxes is None:
            self.terrain = None
        else:
            b = _contact_rule.terrain_boxes(boxes)
            if b.ndim != 2:
                raise ValueError("setTerrain: boxes of shape (n, 5) expected (one robot)")
            self.terrain = b
        if self.device_contacts and self._native is not None:  # (the rule is on since initializeJoints)
            self._native.terrain(self.terrain)

    def setActuators(self, params, limit=None, friction_shape=None):
        """The actuator model between ``execute(torques)`` and the dynamics (``actuator_model``; HIP library only): ``params`` one row of 8, (1, 8), or a
        dict by field name (missing fields: the identity value); ``limit``: the effort limits of the controlled joints (default: the model's);
        None: off.  Arms and resets the model; before ``initializeJoints`` it is kept for then."""
        self._actuators = None if params is None else (params, limit, friction_shape)
        if self._sim_models is not None:
            self._sim_models.set_actuators(params, limit, friction_shape)

    def setJointStops(self, params, lo=None, hi=None, scale=None):
        """The joint end-stops between the actuators and the dynamics (``joint_stops``; HIP library only): ``params`` one row of 8, (1, 8), or a dict
        by field name (``k``, ``d``, ``cap``; missing fields: ``joint_stops.DEFAULTS``), which may also carry ``lo``, ``hi``, ``scale``,
        ``range_scale``, ``margin`` and ``lock``; the range defaults to the model's position limits, ``scale`` to its effort limits; None: off.
        Arms and resets the model; before ``initializeJoints`` it is kept for then."""
        self._joint_stops = None if params is None else (params, lo, hi, scale)
        if self._sim_models is not None:
            self._sim_models.set_joint_stops(params, lo, hi, scale)

    def jointStopState(self):
        """the state rows of the joint stops by ``joint_stops.unpack`` (``tau_stop``, ``pen``, ``peak_pen``, ``hits`` ...); None without them"""
        return None if self._sim_models is None else self._sim_models.joint_stop_state()

    def setPlant(self, rows, link_scale=None):
        """The plant's own link inertias (``plant_model``; HIP library only): ``rows`` one row of 16, (1, 16), or a dict by field name (missing fields:
        the identity value); ``link_scale``: None or (1, nj) / (nj,), every link's own mass factor; None: off.  Body indices are table joint indices
        of the REDUCED model (``model.names[j + 1]``).  Checked here before any library call; before ``initializeJoints`` it is kept for then."""
        if link_scale is not None:
            link_scale = np.asarray(link_scale, dtype=float).reshape(1, -1)
        self._plant = None if rows is None else (rows, link_scale)
        if self._sim_models is not None:
            self._sim_models.set_plant(rows, link_scale)

    def plantModel(self):
        """the ``minipin.Model`` the simulator integrates: ``model`` with the inertias of ``setPlant`` (``model`` itself without one)"""
        if self._plant is None:
            return self.model
        return _plant_model.models(self.model, *_tsim.checked_plant(*self._plant, 1, self.model.njoints - 1))[0]

    def setSensors(self, params):
        """The sensor model between the dynamics and ``measureState()`` (``sensor_model``; HIP library only): ``params`` one row of 16, (1, 16), or a
        dict by field name (missing fields 0: the identity); None: off.  Arms and resets the model at the current true state; before
        ``initializeJoints`` it is kept for then."""
        self._sensors = params
        if self._sim_models is not None:
            self._sim_models.set_sensors(params, self.x)

    def setEstimator(self, params):
        """The base-state estimator between the sensors and ``measureState()`` (``state_estimator``; HIP library only, needs
        ``device_contacts=True``): ``params`` one row of 16, (1, 16), or a dict by field name (``w_p``, ``w_v``; missing fields 0: the identity); None:
        off.  Arms and resets the estimator at the current measurement; before ``initializeJoints`` it is kept for then."""
        self._estimator = params
        if self._sim_models is not None:
            self._sim_models.set_estimator(params, self.x)

    def setFootSensors(self, params, detected_contacts=()):
        """The foot force sensors and the contact detector after every step (``foot_sensors``; HIP library only, needs ``device_contacts=True``):
        ``params`` one row of 16, (1, 16), or a dict by field name (missing fields as in ``foot_sensors.EXACT``); None: off.  ``detected_contacts``:
        () or ("estimator",): the estimator works from the detected pair.  Arms the detector on the rule's ``in_contact`` pair; before
        ``initializeJoints`` it is kept for then."""
        self._foot_sensors = None if params is None else (params, tuple(detected_contacts))
        if self._sim_models is not None:
            self._sim_models.set_foot_sensors(params, tuple(detected_contacts))

    def detectedContacts(self):
        """[left, right] the contacts the detector of ``setFootSensors`` reports; ``in_contact`` without one"""
        if self._sim_models is None or self._sim_models.rows["foot_sensors"] is None:
            return list(self.in_contact)
        return [bool(v) for v in self._sim_models.detected[0]]

    def createStairs(self, pose_stairs, height_step):
        """bullet_robot.py:275-340 of the reference: three steps of half extents 0.2 x 0.5 x height_step / 2, each 0.3 m further and height_step higher,
        the first centred at ``pose_stairs`` (``contact_rule.stairs``)."""
        self.setTerrain(_contact_rule.stairs(pose_stairs, height_step))

    def close(self):
        if self._native is not None:
            self._native.close()
            self._native = self._sim_models = None
