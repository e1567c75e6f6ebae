"""Every refusal of the simulator's entry points (csrc/sim_host.h; include/mpc_sim_*.h), word for word: the arming calls, ``_set``, and ``_read`` /
``_set`` / ``_feed`` of a model that is off, for the actuators, sensors, estimator, foot sensors, plant model, friction, disturbances, contact rule and
terrain; which of two refusals comes first; and that a refused arming call leaves the configuration in force.  The calls go to the bound functions
themselves (``NativeSolver._hip``), since the Python wrappers refuse most of these rows before the library sees them, and ``mpc_last_error`` is
compared for equality.  The bad entry is always in row 1 of a batch of 2, never in row 0.

Not here: the ``*_width`` calls on a handle that is no simulator handle (no such handle is cheap to build next to these two; the wrappers' tests
reach them), and the refusals that need another robot model (a model without the two sole contacts, more joints or a longer state than the kernels
hold, a handle without a model)."""
import ctypes as C

import numpy as np
import pytest

from mpc_benchmark_amd import _capi
from mpc_benchmark_amd import contact_rule as cr
from tests.test_gpu_sim_friction import _sim

pytestmark = pytest.mark.gpu

B = 2
NAN = float("nan")
OFF_RULE = "the contact rule is off on this handle (turn it on with mpc_sim_contacts first)"
OFF = {"actuators": "the actuator model is off on this handle (turn it on with mpc_sim_actuators)",
       "sensors": "the sensor model is off on this handle (turn it on with mpc_sim_sensors)",
       "estimator": "the estimator is off on this handle (turn it on with mpc_sim_estimator)",
       "foot_sensors": "the foot sensors are off on this handle (turn them on with mpc_sim_foot_sensors)",
       "plant": "the plant model is off on this handle (turn it on with mpc_sim_plant)",
       "friction": "the friction model is off on this handle (turn it on with mpc_sim_friction)",
       "disturbances": "the disturbance schedule is off on this handle (turn it on with mpc_sim_disturbances)"}


def _call(sim, name, *args):
    """the bound function on the handle -> (return code, mpc_last_error)"""
    rc = sim._hip(name)(sim._h, *[_capi._dp(a) if isinstance(a, np.ndarray) else a for a in args])
    return rc, sim.lib.mpc_last_error(sim._h).decode()


def _rows(row):
    return np.tile(np.asarray(row, dtype=np.float64), (B, 1))


def _bad(a, where, value):
    """a copy of ``a`` with ``value`` at index ``where`` of row 1"""
    a = np.array(a, dtype=np.float64)
    a[1][where] = value
    return a


class Ctx:
    """The two handles and valid arguments of every call: ``on`` has the contact rule and every model on (no push schedule: ``on`` keeps a push
    armed instead), ``off`` has the rule and every model off and a push armed."""

    def __init__(self, lib):
        rb, self.on = _sim(lib, B)
        _, self.off = _sim(lib, B, rule=False)
        d = self.on.dims
        self.nx, self.nu, self.nj = d.nx, d.nu, self.on._model_nj
        self.x0 = np.tile(np.asarray(rb.x0, dtype=np.float64), (B, 1))
        self.act = _rows([0, 1, 0, 0, 0, 0, 0, 0])
        self.limit = np.full(self.nu, 10.0)
        self.sen = _rows([0.0] * 16)
        self.est = _rows([0.0] * 16)
        self.fs = _rows([0, 0, 0, 0, 0, 0, 50, 20, 1, 1, 0, 0, 0, 0, 0, 0])
        self.plant = _rows([1, 1] + [0.0] * 14)
        self.link_scale = np.ones((B, self.nj))
        self.fr = _rows([1.0] * 8)
        self.event = [1, 0, 0, 1, 0, 0, 0, 0, 0, 5.0, 0, 0, 0, 0, 0, 0]
        self.dis = _rows(self.event)
        self.cfg = cr.config({}, ground_z=0.0)
        self.push = np.zeros((B, 3))
        for h in (self.on, self.off):
            assert _call(h, "mpc_sim_set_push", self.push, 3)[0] == 0
        self.act_on = _rows([2, 1.5, 0.01, 0, 0, 0, 0, 0])
        self.sen_on = _rows([3, 0.01] + [0.0] * 14)
        self.fr_on = _rows([0.5] * 4 + [2.0] * 4)
        for name, args in (("mpc_sim_actuators", (self.act_on, None, None)), ("mpc_sim_sensors", (self.sen_on, self.x0)),
                           ("mpc_sim_estimator", (self.est, self.x0)), ("mpc_sim_foot_sensors", (self.fs,)), ("mpc_sim_plant", (self.plant, None)),
                           ("mpc_sim_friction", (self.fr_on,))):
            rc, err = _call(self.on, name, *args)
            assert rc == 0, (name, err)
        self.state = {}
        for noun, extra in (("actuators", 0), ("sensors", 1), ("estimator", 1), ("foot_sensors", 0), ("friction", 0)):
            st = np.zeros((B, self.on._width("mpc_sim_%s_width" % noun)))
            assert _call(self.on, "mpc_sim_%s_read" % noun, None, st, *([None] * extra))[0] == 0, noun
            self.state[noun] = st
        self.con = np.zeros((B, cr.WIDTH))
        assert _call(self.on, "mpc_sim_contacts_read", self.con)[0] == 0

    def contacts_cfg(self, **kw):
        c = dict(self.cfg, **kw)
        return C.byref(_capi.MpcSimContactsConfig(c["ground_z"], c["ground_tol"], c["release_force"], c["release_steps"], 0))

    def events(self, robot1):
        """one event per robot, robot 1's changed by ``robot1`` {index: value}"""
        ev = np.array(self.dis)
        for i, v in robot1.items():
            ev[1][i] = v
        return ev


CTX = []


@pytest.fixture(scope="module")
def ctx(hip_lib):
    if not CTX:
        CTX.append(Ctx(hip_lib))
    return CTX[0]


def terrain_cfg(n, per_robot):
    return C.byref(_capi.MpcSimTerrainConfig(n, per_robot))


W_ACT = lambda c: c.state["actuators"].shape[1]
W_SEN = lambda c: c.state["sensors"].shape[1]
W_EST = lambda c: c.state["estimator"].shape[1]
W_FS = 232
BOXES = np.array([[[0, 1, 0, 1, 0.1]], [[0, 1, 0, 1, 0.1]]], dtype=np.float64)

# (handle, entry point, arguments from the context, the message).  The messages are those of csrc/sim_host.h before its refusals were gathered into
# helpers, copied from that source.
CASES = [
    # ---- actuators
    ("on", "mpc_sim_actuators", lambda c: (_bad(c.act, 3, NAN), None, None), "sim_actuators: row 1 holds a non-finite entry (3)"),
    ("on", "mpc_sim_actuators", lambda c: (_bad(c.act, 0, 16), None, None), "sim_actuators: row 1: delay must be an integer value in [0, 15]"),
    ("on", "mpc_sim_actuators", lambda c: (_bad(c.act, 0, 0.5), None, None), "sim_actuators: row 1: delay must be an integer value in [0, 15]"),
    ("on", "mpc_sim_actuators", lambda c: (_bad(c.act, 1, 0), None, None), "sim_actuators: row 1: scale must be > 0"),
    ("on", "mpc_sim_actuators", lambda c: (_bad(c.act, 3, -1), None, None),
     "sim_actuators: row 1: time_constant, damping, coulomb, v_eps and sat must be >= 0"),
    ("on", "mpc_sim_actuators", lambda c: (_bad(c.act, 4, 1), None, None), "sim_actuators: row 1: coulomb > 0 needs v_eps > 0"),
    ("on", "mpc_sim_actuators", lambda c: (_bad(c.act, 6, 1), None, None),
     "sim_actuators: a row with sat > 0 needs the effort limits (limit must not be null)"),
    ("on", "mpc_sim_actuators", lambda c: (c.act, -c.limit, None), "sim_actuators: limit and friction_shape must be finite and >= 0"),
    ("on", "mpc_sim_actuators", lambda c: (c.act, c.limit, c.limit * NAN), "sim_actuators: limit and friction_shape must be finite and >= 0"),
    ("on", "mpc_sim_actuators_set", lambda c: (None,), "sim_actuators_set: state must not be null"),
    ("on", "mpc_sim_actuators_set", lambda c: (_bad(c.state["actuators"], 0, NAN),), "sim_actuators_set: row 1 holds a non-finite entry (0)"),
    ("on", "mpc_sim_actuators_set", lambda c: (_bad(c.state["actuators"], W_ACT(c) - 2, 16),),
     "sim_actuators_set: row 1: head must be an integer value in [0, 16)"),
    ("on", "mpc_sim_actuators_set", lambda c: (_bad(c.state["actuators"], W_ACT(c) - 1, -1),), "sim_actuators_set: row 1: count must be >= 0"),
    ("off", "mpc_sim_actuators_read", lambda c: (None, None), "sim_actuators_read: " + OFF["actuators"]),
    ("off", "mpc_sim_actuators_set", lambda c: (c.state["actuators"],), "sim_actuators_set: " + OFF["actuators"]),
    # ---- sensors
    ("on", "mpc_sim_sensors", lambda c: (_bad(c.sen, 15, NAN), c.x0), "sim_sensors: row 1 holds a non-finite entry (15)"),
    ("on", "mpc_sim_sensors", lambda c: (_bad(c.sen, 0, 16), c.x0), "sim_sensors: row 1: delay must be an integer value in [0, 15]"),
    ("on", "mpc_sim_sensors", lambda c: (_bad(c.sen, 10, -1), c.x0),
     "sim_sensors: row 1: the noise levels (sigma_*), quantum, q_bias and v_time_constant must be >= 0"),
    ("on", "mpc_sim_sensors", lambda c: (_bad(c.sen, 9, 2), c.x0), "sim_sensors: row 1: v_from_q must be 0 or 1"),
    ("on", "mpc_sim_sensors", lambda c: (_bad(c.sen, 11, 4294967296.0), c.x0), "sim_sensors: row 1: seed must be an integer value in [0, 2^32)"),
    ("on", "mpc_sim_sensors", lambda c: (_bad(c.sen, 12, 1), c.x0), "sim_sensors: row 1: the reserved entries must be 0"),
    ("on", "mpc_sim_sensors", lambda c: (c.sen, None), "sim_sensors: x0 must not be null (the first measurement is taken of it)"),
    ("on", "mpc_sim_sensors", lambda c: (c.sen, _bad(c.x0, 4, NAN)), "sim_sensors: x0 holds a non-finite entry"),
    ("on", "mpc_sim_sensors_set", lambda c: (None,), "sim_sensors_set: state must not be null"),
    ("on", "mpc_sim_sensors_set", lambda c: (_bad(c.state["sensors"], 7, NAN),), "sim_sensors_set: row 1 holds a non-finite entry (7)"),
    ("on", "mpc_sim_sensors_set", lambda c: (_bad(c.state["sensors"], W_SEN(c) - 2, -1),),
     "sim_sensors_set: row 1: head must be an integer value in [0, 16)"),
    ("on", "mpc_sim_sensors_set", lambda c: (_bad(c.state["sensors"], W_SEN(c) - 1, 0),),
     "sim_sensors_set: row 1: count must be >= 1 (a measurement is always held)"),
    ("off", "mpc_sim_sensors_read", lambda c: (None, None, None), "sim_sensors_read: " + OFF["sensors"]),
    ("off", "mpc_sim_sensors_set", lambda c: (c.state["sensors"],), "sim_sensors_set: " + OFF["sensors"]),
    # ---- estimator
    ("on", "mpc_sim_estimator", lambda c: (_bad(c.est, 1, NAN), c.x0), "sim_estimator: row 1 holds a non-finite entry (1)"),
    ("on", "mpc_sim_estimator", lambda c: (_bad(c.est, 1, 1.5), c.x0), "sim_estimator: row 1: the weights w_p and w_v must be in [0, 1]"),
    ("on", "mpc_sim_estimator", lambda c: (_bad(c.est, 2, 1), c.x0), "sim_estimator: row 1: the reserved entries must be 0"),
    ("on", "mpc_sim_estimator", lambda c: (c.est, None), "sim_estimator: x0 must not be null (the arming event is run on it)"),
    ("on", "mpc_sim_estimator", lambda c: (c.est, _bad(c.x0, 0, NAN)), "sim_estimator: x0 holds a non-finite entry"),
    ("off", "mpc_sim_estimator", lambda c: (c.est, c.x0), "sim_estimator: " + OFF_RULE),
    ("on", "mpc_sim_estimator_set", lambda c: (None,), "sim_estimator_set: state must not be null"),
    ("on", "mpc_sim_estimator_set", lambda c: (_bad(c.state["estimator"], 2, NAN),), "sim_estimator_set: row 1 holds a non-finite entry (2)"),
    ("on", "mpc_sim_estimator_set", lambda c: (_bad(c.state["estimator"], c.nx + 1, 2),), "sim_estimator_set: row 1: held must be 0 or 1"),
    ("on", "mpc_sim_estimator_set", lambda c: (_bad(c.state["estimator"], W_EST(c) - 1, 0),),
     "sim_estimator_set: row 1: count must be >= 1 (an estimate is always held)"),
    ("off", "mpc_sim_estimator_read", lambda c: (None, None, None), "sim_estimator_read: " + OFF["estimator"]),
    ("off", "mpc_sim_estimator_set", lambda c: (c.state["estimator"],), "sim_estimator_set: " + OFF["estimator"]),
    # ---- foot sensors
    ("on", "mpc_sim_foot_sensors", lambda c: (_bad(c.fs, 6, NAN),), "sim_foot_sensors: row 1 holds a non-finite entry (6)"),
    ("on", "mpc_sim_foot_sensors", lambda c: (_bad(c.fs, 0, -1),), "sim_foot_sensors: row 1: delay must be an integer value in [0, 15]"),
    ("on", "mpc_sim_foot_sensors", lambda c: (_bad(c.fs, 5, -1),),
     "sim_foot_sensors: row 1: sigma_f, sigma_m, bias_f, bias_m and time_constant must be >= 0"),
    ("on", "mpc_sim_foot_sensors", lambda c: (_bad(c.fs, 7, 60),), "sim_foot_sensors: row 1: f_off must be <= f_on"),
    ("on", "mpc_sim_foot_sensors", lambda c: (_bad(c.fs, 9, 0),), "sim_foot_sensors: row 1: on_steps and off_steps must be integer values >= 1"),
    ("on", "mpc_sim_foot_sensors", lambda c: (_bad(c.fs, 10, 0.5),), "sim_foot_sensors: row 1: seed must be an integer value in [0, 2^32)"),
    ("on", "mpc_sim_foot_sensors", lambda c: (_bad(c.fs, 11, 1),), "sim_foot_sensors: row 1: the reserved entries must be 0"),
    ("off", "mpc_sim_foot_sensors", lambda c: (c.fs,), "sim_foot_sensors: " + OFF_RULE),
    ("on", "mpc_sim_foot_sensors_set", lambda c: (None,), "sim_foot_sensors_set: state must not be null"),
    ("on", "mpc_sim_foot_sensors_set", lambda c: (_bad(c.state["foot_sensors"], 231, NAN),), "sim_foot_sensors_set: row 1 holds a non-finite entry (231)"),
    ("on", "mpc_sim_foot_sensors_set", lambda c: (_bad(c.state["foot_sensors"], 1, 2),), "sim_foot_sensors_set: row 1: det must be 0 or 1"),
    ("on", "mpc_sim_foot_sensors_set", lambda c: (_bad(c.state["foot_sensors"], slice(0, 2), 0),),
     "sim_foot_sensors_set: row 1 has no sole detected (the detector never reports an empty set)"),
    ("on", "mpc_sim_foot_sensors_set", lambda c: (_bad(c.state["foot_sensors"], 5, -1),),
     "sim_foot_sensors_set: row 1: the counters above and below must be >= 0"),
    ("on", "mpc_sim_foot_sensors_set", lambda c: (_bad(c.state["foot_sensors"], 37, -1),), "sim_foot_sensors_set: row 1: the confusion counts must be >= 0"),
    ("on", "mpc_sim_foot_sensors_set", lambda c: (_bad(c.state["foot_sensors"], W_FS - 2, 16),),
     "sim_foot_sensors_set: row 1: head must be an integer value in [0, 16)"),
    ("on", "mpc_sim_foot_sensors_set", lambda c: (_bad(c.state["foot_sensors"], W_FS - 1, -1),), "sim_foot_sensors_set: row 1: count must be >= 0"),
    ("on", "mpc_sim_foot_sensors_feed", lambda c: (4,), "sim_foot_sensors_feed: unknown consumer bit in 4 (1: the estimator, 2: the low-level QPs)"),
    ("off", "mpc_sim_foot_sensors_read", lambda c: (None, None), "sim_foot_sensors_read: " + OFF["foot_sensors"]),
    ("off", "mpc_sim_foot_sensors_set", lambda c: (c.state["foot_sensors"],), "sim_foot_sensors_set: " + OFF["foot_sensors"]),
    ("off", "mpc_sim_foot_sensors_feed", lambda c: (1,), "sim_foot_sensors_feed: " + OFF["foot_sensors"]),
    # ---- plant model
    ("on", "mpc_sim_plant", lambda c: (_bad(c.plant, 8, NAN), None), "sim_plant: row 1 holds a non-finite entry (8)"),
    ("on", "mpc_sim_plant", lambda c: (_bad(c.plant, 1, 0), None), "sim_plant: row 1: mass_scale and inertia_scale must be > 0"),
    ("on", "mpc_sim_plant", lambda c: (_bad(c.plant, 7, -1), None), "sim_plant: row 1: payload_mass must be >= 0"),
    ("on", "mpc_sim_plant", lambda c: (_bad(c.plant, 6, c.nj), None),
     lambda c: "sim_plant: row 1: shift_body and payload_body must be integer values in [0, %d] (table joint indices)" % (c.nj - 1)),
    ("on", "mpc_sim_plant", lambda c: (_bad(c.plant, 11, 1), None), "sim_plant: row 1: the reserved entries must be 0"),
    ("on", "mpc_sim_plant", lambda c: (c.plant, _bad(c.link_scale, 2, 0)), "sim_plant: link_scale must be finite and > 0 (robot 1, joint 2)"),
    ("off", "mpc_sim_plant_read", lambda c: (None, None, None), "sim_plant_read: " + OFF["plant"]),
    # ---- friction
    ("on", "mpc_sim_friction", lambda c: (_bad(c.fr, 1, NAN),), "sim_friction: row 1: mu and mu_spin must be >= 0 (+inf: the sole never slides), entry 1"),
    ("on", "mpc_sim_friction", lambda c: (_bad(c.fr, 3, -1),), "sim_friction: row 1: mu and mu_spin must be >= 0 (+inf: the sole never slides), entry 3"),
    ("on", "mpc_sim_friction", lambda c: (_bad(c.fr, 5, float("inf")),),
     "sim_friction: row 1: m_slip, I_slip, v_max and w_max must be finite and > 0, entry 5"),
    ("off", "mpc_sim_friction", lambda c: (c.fr,), "sim_friction: " + OFF_RULE),
    ("on", "mpc_sim_friction_set", lambda c: (None,), "sim_friction_set: state must not be null"),
    ("on", "mpc_sim_friction_set", lambda c: (_bad(c.state["friction"], 16, NAN),), "sim_friction_set: row 1 holds a non-finite entry (16)"),
    ("on", "mpc_sim_friction_set", lambda c: (_bad(c.state["friction"], 7, 2),), "sim_friction_set: row 1: sliding must be 0 or 1"),
    ("on", "mpc_sim_friction_set", lambda c: (_bad(c.state["friction"], 4, 0.1),),
     "sim_friction_set: row 1: sole 1 holds a velocity but its sliding flag is 0"),
    ("on", "mpc_sim_friction_set", lambda c: (_bad(c.state["friction"], 12, -1),),
     "sim_friction_set: row 1: slip_steps, slip_dist, slip_yaw, peak_excess and steps must be >= 0"),
    ("off", "mpc_sim_friction_read", lambda c: (None, None), "sim_friction_read: " + OFF["friction"]),
    ("off", "mpc_sim_friction_set", lambda c: (c.state["friction"],), "sim_friction_set: " + OFF["friction"]),
    # ---- disturbances (both handles keep a push armed: every refusal here comes before that one)
    ("on", "mpc_sim_disturbances", lambda c: (c.dis, 0), "sim_disturbances: n_events must be 1 .. 8"),
    ("on", "mpc_sim_disturbances", lambda c: (c.dis, 9), "sim_disturbances: n_events must be 1 .. 8"),
    ("on", "mpc_sim_disturbances", lambda c: (c.events({1: NAN}), 1), "sim_disturbances: robot 1, event 0: start is not finite"),
    ("on", "mpc_sim_disturbances", lambda c: (c.events({3: 1.5}), 1), "sim_disturbances: robot 1, event 0: steps must be an integer value"),
    ("on", "mpc_sim_disturbances", lambda c: (c.events({0: 6}), 1), "sim_disturbances: robot 1, event 0: trigger must be 0 .. 5"),
    ("on", "mpc_sim_disturbances", lambda c: (c.events({15: 1}), 1), "sim_disturbances: robot 1, event 0: reserved must be 0"),
    ("on", "mpc_sim_disturbances", lambda c: (c.events({1: -1}), 1), "sim_disturbances: robot 1, event 0: start must be >= 0 (a step of the clock)"),
    ("on", "mpc_sim_disturbances", lambda c: (c.events({0: 2, 1: 0}), 1),
     "sim_disturbances: robot 1, event 0: start must be >= 1 (an occurrence of the transition)"),
    ("on", "mpc_sim_disturbances", lambda c: (c.events({2: -1}), 1), "sim_disturbances: robot 1, event 0: delay must be >= 0"),
    ("on", "mpc_sim_disturbances", lambda c: (c.events({3: 0}), 1), "sim_disturbances: robot 1, event 0: steps must be >= 1"),
    ("on", "mpc_sim_disturbances", lambda c: (c.events({3: 4, 4: 2}), 1),
     "sim_disturbances: robot 1, event 0: period must be 0 (once) or, on an absolute trigger, >= steps"),
    ("on", "mpc_sim_disturbances", lambda c: (c.events({7: 2}), 1), "sim_disturbances: robot 1, event 0: force_frame must be 0 or 1"),
    ("on", "mpc_sim_disturbances", lambda c: (c.events({6: c.nj}), 1),
     lambda c: "sim_disturbances: robot 1, event 0: link must be in [0, %d] (table joint indices)" % (c.nj - 1)),
    ("on", "mpc_sim_disturbances", lambda c: (c.dis, 1),
     "sim_disturbances: a push is armed on this handle (mpc_sim_set_push): disarm it with mpc_sim_set_push(sim, NULL, 0) before arming a schedule"),
    ("off", "mpc_sim_disturbances_read", lambda c: (None, None, None), "sim_disturbances_read: " + OFF["disturbances"]),
    ("off", "mpc_sim_disturbances_reset", lambda c: (), "sim_disturbances_reset: " + OFF["disturbances"]),
    ("on", "mpc_sim_set_push", lambda c: (c.push, 4), "sim_set_push: width must be 3 (force at the base origin) or 6 (force, world point)"),
    # ---- the contact rule
    ("on", "mpc_sim_contacts", lambda c: (c.contacts_cfg(ground_z=NAN),), "sim_contacts: ground_z, ground_tol and release_force must be finite"),
    ("on", "mpc_sim_contacts", lambda c: (c.contacts_cfg(ground_tol=-1.0),), "sim_contacts: ground_tol and release_force must be >= 0"),
    ("on", "mpc_sim_contacts", lambda c: (c.contacts_cfg(release_steps=0),), "sim_contacts: release_steps must be >= 1"),
    ("on", "mpc_sim_contacts_set", lambda c: (None,), "sim_contacts_set: rows must not be null"),
    ("on", "mpc_sim_contacts_set", lambda c: (_bad(c.con, 40, NAN),), "sim_contacts_set: row 1 holds a non-finite entry (40)"),
    ("on", "mpc_sim_contacts_set", lambda c: (_bad(c.con, 3, 2),), "sim_contacts_set: row 1: in_contact and lifted must be 0 or 1"),
    ("on", "mpc_sim_contacts_set", lambda c: (_bad(c.con, slice(0, 2), 0),), "sim_contacts_set: row 1 has no sole in contact (flight phases are not simulated)"),
    ("on", "mpc_sim_contacts_set", lambda c: (_bad(c.con, 33, -1),), "sim_contacts_set: row 1: pulling, the counts and steps must be >= 0"),
    ("on", "mpc_sim_contacts_set", lambda c: (_bad(c.con, slice(20, 29), 2 * c.con[1, 20:29]),), "sim_contacts_set: row 1: the anchor of sole 1 is not a rotation"),
    ("off", "mpc_sim_contacts_set", lambda c: (c.con,), "sim_contacts_set: the contact rule is off on this handle (turn it on with mpc_sim_contacts)"),
    ("off", "mpc_sim_contacts_read", lambda c: (c.con,), "sim_contacts_read: the contact rule is off on this handle (turn it on with mpc_sim_contacts)"),
    ("off", "mpc_sim_contacts_read", lambda c: (None,), "sim_contacts_read: rows must not be null"),
    # ---- the terrain
    ("off", "mpc_sim_terrain", lambda c: (terrain_cfg(1, 1), BOXES), "sim_terrain: " + OFF_RULE),
    ("off", "mpc_sim_terrain_read", lambda c: (terrain_cfg(0, 0), None), "sim_terrain_read: " + OFF_RULE),
    ("off", "mpc_sim_terrain_height", lambda c: (np.zeros((B, 1, 2)), 1, np.zeros((B, 1))), "sim_terrain_height: " + OFF_RULE),
    ("on", "mpc_sim_terrain", lambda c: (terrain_cfg(17, 1), BOXES), "sim_terrain: n_boxes must be 0 .. 16"),
    ("on", "mpc_sim_terrain", lambda c: (terrain_cfg(1, 2), BOXES), "sim_terrain: per_robot must be 0 or 1"),
    ("on", "mpc_sim_terrain", lambda c: (terrain_cfg(1, 1), None), "sim_terrain: boxes must not be null with n_boxes > 0"),
    ("on", "mpc_sim_terrain", lambda c: (terrain_cfg(1, 1), _bad(BOXES, (0, 4), NAN)), "sim_terrain: box 1 holds a non-finite number"),
    ("on", "mpc_sim_terrain", lambda c: (terrain_cfg(1, 1), _bad(BOXES, (0, 2), 2)), "sim_terrain: box 1 has x_lo > x_hi or y_lo > y_hi"),
    ("on", "mpc_sim_terrain_read", lambda c: (None, None), "sim_terrain_read: cfg must not be null"),
    ("on", "mpc_sim_terrain_height", lambda c: (None, -1, None), "sim_terrain_height: n must be >= 0"),
    ("on", "mpc_sim_terrain_height", lambda c: (None, 1, np.zeros((B, 1))), "sim_terrain_height: xy and h must not be null"),
    ("on", "mpc_sim_terrain_height", lambda c: (_bad(np.zeros((B, 1, 2)), (0, 1), NAN), 1, np.zeros((B, 1))), "sim_terrain_height: xy holds a non-finite number"),
    # ---- two wrong things at once: the first refusal of the entry point is the one reported
    ("off", "mpc_sim_estimator", lambda c: (_bad(c.est, 0, -1), c.x0), "sim_estimator: row 1: the weights w_p and w_v must be in [0, 1]"),
    ("off", "mpc_sim_foot_sensors", lambda c: (_bad(c.fs, 7, 60),), "sim_foot_sensors: row 1: f_off must be <= f_on"),
    ("off", "mpc_sim_friction", lambda c: (_bad(c.fr, 4, 0),), "sim_friction: row 1: m_slip, I_slip, v_max and w_max must be finite and > 0, entry 4"),
    ("on", "mpc_sim_sensors", lambda c: (_bad(c.sen, 9, 0.5), None), "sim_sensors: row 1: v_from_q must be 0 or 1"),
    ("off", "mpc_sim_disturbances", lambda c: (c.events({0: 2, 1: 1}), 1),
     "sim_disturbances: a contact trigger (2 to 5) needs the contact rule, which is off on this handle (turn it on with mpc_sim_contacts first)"),
]


@pytest.mark.parametrize("case", range(len(CASES)), ids=["%03d-%s-%s" % (i, c[1][8:], c[0]) for i, c in enumerate(CASES)])
def test_refusal_is_worded_as_before(ctx, case):
    handle, name, args, message = CASES[case]
    rc, err = _call(getattr(ctx, handle), name, *args(ctx))
    assert rc == -1
    assert err == (message(ctx) if callable(message) else message)


def test_push_and_schedule_exclude_each_other(ctx):
    """a push armed refuses a schedule (in CASES); a schedule armed refuses a push, and disarming either lets the other in"""
    sim = ctx.off
    assert _call(sim, "mpc_sim_set_push", None, 0)[0] == 0
    assert _call(sim, "mpc_sim_disturbances", ctx.dis, 1)[0] == 0
    assert _call(sim, "mpc_sim_set_push", ctx.push, 3) == (-1, "sim_set_push: the disturbance schedule is on (mpc_sim_disturbances): its events are the "
                                                          "pushes of this handle; turn it off with mpc_sim_disturbances(sim, NULL, 0) before arming a push")
    assert _call(sim, "mpc_sim_disturbances", None, 0)[0] == 0
    assert _call(sim, "mpc_sim_set_push", ctx.push, 3)[0] == 0


@pytest.mark.parametrize("noun", ["actuators", "sensors", "friction"])
def test_refused_arming_leaves_the_rows_in_force(ctx, noun):
    """a refused arming call on an armed model: _read gives the params of the earlier call, unchanged"""
    armed = {"actuators": ctx.act_on, "sensors": ctx.sen_on, "friction": ctx.fr_on}[noun]
    bad = {"actuators": (_bad(ctx.act, 1, -1), None, None), "sensors": (_bad(ctx.sen, 0, 99), ctx.x0), "friction": (_bad(ctx.fr, 6, 0),)}[noun]
    assert _call(ctx.on, "mpc_sim_" + noun, *bad)[0] == -1
    params = np.zeros_like(armed)
    state = np.zeros_like(ctx.state[noun])
    assert _call(ctx.on, "mpc_sim_%s_read" % noun, params, state, *([None] if noun == "sensors" else []))[0] == 0
    assert np.array_equal(params, armed)
    assert np.array_equal(state, ctx.state[noun])
