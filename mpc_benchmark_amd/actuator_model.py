"""The per-robot actuator model of the torque-driven simulator, in numpy: one step for B robots.  It is the definition the device kernel
(``mpc_sim_actuators``, include/mpc_sim_actuators.h, csrc/sim_actuators.h; ``NativeSolver.actuators`` / ``read_actuators`` / ``set_actuators``) is
held to.  The model sits between "the controller wrote the torque of the step" and "the dynamics integrate it": transport delay, gain error,
first-order lag, saturation, joint friction.  What it returns is the APPLIED torque: what the step integrates, what the record stores and what the
metrics' power and energy are taken from.

Every robot has one parameter row of ``PARAMS`` doubles (``FIELDS``):

  0 ``delay``          transport delay in steps, an integer value in [0, RING - 1]
  1 ``scale``          torque gain error, finite and > 0
  2 ``time_constant``  first-order lag in seconds, >= 0 (0: none)
  3 ``damping``        viscous joint friction in N m s / rad, >= 0
  4 ``coulomb``        Coulomb friction in N m, >= 0
  5 ``v_eps``          smoothing velocity of the Coulomb term in rad / s, > 0 when ``coulomb`` > 0
  6 ``sat``            saturation as a fraction of ``limit[j]``, >= 0 (0: none)
  7 reserved, 0

and two vectors of length nu = nv - 6 are shared by all robots: ``limit`` (the effort limits; needed when any row has ``sat`` > 0) and
``friction_shape`` (multiplies ``damping`` and ``coulomb`` joint by joint; None: ones).

Every robot has one state row of ``width(nu)`` = 18 nu + 2 doubles: a ring of the latest ``RING`` commanded torque vectors ``ring[RING][nu]``, the
lag state ``y[nu]``, ``applied[nu]`` (the torque the latest step integrated), ``head`` (the ring slot of the newest command) and ``count`` (commands
since the reset).  After a reset everything is 0.

One step of length ``dt`` (a device loop's dt; ``substeps * dt`` of one ``mpc_simulate_torque`` call, which holds the applied torque over its
substeps), from the commanded torque ``u`` and the joint velocities ``v = x[nq + 6:]`` of the state the step STARTS from, joint by joint:

  1. ``u`` is pushed into the ring (``head`` advances, ``count`` + 1);
  2. ``ud``: the command pushed ``delay`` steps ago; while fewer than ``delay + 1`` commands are held, the oldest one (the line is primed with the
     first command: a robot does not drop to zero torque at a reset);
  3. ``w = scale ud`` (``scale`` == 1: ``ud`` itself);
  4. lag: ``time_constant`` == 0: ``y = w``; else at ``count`` == 1: ``y = w`` (primed); else ``y += -expm1(-dt / time_constant) (w - y)``;
  5. saturation: ``sat`` > 0: ``y_out = clamp(y, +- sat limit[j])``, the lag state keeps the unclamped ``y``; else ``y_out = y``;
  6. friction: ``damping`` > 0 or ``coulomb`` > 0: ``tau = y_out - s_j (damping v_j + coulomb tanh(v_j / v_eps))`` (the Coulomb term only with
     ``coulomb`` > 0); else ``tau = y_out``;
  7. ``applied = tau``.

The identity row ``IDENTITY`` = (0, 1, 0, 0, 0, 0, 0, 0) takes none of the arithmetic branches: the applied torque is the command bit for bit.

The viscous term is explicit: it uses the velocity at the start of the step.  It is stable only while ``damping * dt`` is small against the joint's
reflected inertia; choosing ``damping`` so is the caller's business, nothing here checks it."""
from __future__ import annotations

import numpy as np

FIELDS = ("delay", "scale", "time_constant", "damping", "coulomb", "v_eps", "sat", "reserved")
PARAMS = len(FIELDS)         # MPC_SIM_ACTUATORS_PARAMS
RING = 16                    # MPC_SIM_ACTUATORS_RING
IDENTITY = (0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
P_DELAY, P_SCALE, P_TC, P_DAMPING, P_COULOMB, P_VEPS, P_SAT = range(7)


def width(nu):
    """doubles of one robot's state row"""
    return (RING + 2) * int(nu) + 2


def reset(B, nu):
    """the state rows after ``mpc_sim_actuators(params, ...)``: (B, width(nu)) zeros"""
    return np.zeros((int(B), width(nu)))


def rows(params, batch):
    """The forms the Python interfaces take -> (B, PARAMS) float64: ``(B, 8)`` rows, one row of 8 (for every robot), or a dict by ``FIELDS`` name of
    scalars or (B,) arrays, missing fields at their identity value."""
    B = int(batch)
    if isinstance(params, dict):
        bad = sorted(set(params) - set(FIELDS[:-1]))
        if bad:
            raise ValueError("actuators: unknown fields %s (known: %s)" % (bad, ", ".join(FIELDS[:-1])))
        out = np.tile(np.array(IDENTITY), (B, 1))
        for k, val in params.items():
            a = np.asarray(val, dtype=float)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
                raise ValueError("actuators: field %r is a scalar or a (B,) array with B = %d, got shape %s" % (k, B, a.shape))
            out[:, FIELDS.index(k)] = a
        return out
    p = np.asarray(params, dtype=float)
    if p.shape == (PARAMS,):
        return np.tile(p, (B, 1))
    if p.shape != (B, PARAMS):
        raise ValueError("actuators: params of shape (%d, %d), (%d,) or a dict by field name expected, got %s" % (B, PARAMS, PARAMS, p.shape))
    return np.ascontiguousarray(p)


def validate(params, limit=None, shape=None):
    """The checks of ``mpc_sim_actuators`` (ValueError): rows (B, PARAMS) by the table of the module docstring; ``limit`` finite and >= 0, needed when
    any row has ``sat`` > 0; ``shape`` finite and >= 0.  -> (params, limit, shape) as float64 arrays (None stays None)."""
    p = np.asarray(params, dtype=float)
    if p.ndim != 2 or p.shape[1] != PARAMS:
        raise ValueError("actuators: params of shape (B, %d) expected, got %s" % (PARAMS, p.shape))
    if not np.all(np.isfinite(p)):
        raise ValueError("actuators: non-finite parameters")
    for b, r in enumerate(p):
        if r[P_DELAY] != np.floor(r[P_DELAY]) or not 0 <= r[P_DELAY] <= RING - 1:
            raise ValueError("actuators: row %d: delay must be an integer value in [0, %d], got %r" % (b, RING - 1, r[P_DELAY]))
        if not r[P_SCALE] > 0.0:
            raise ValueError("actuators: row %d: scale must be > 0, got %r" % (b, r[P_SCALE]))
        for k in (P_TC, P_DAMPING, P_COULOMB, P_VEPS, P_SAT):
            if r[k] < 0.0:
                raise ValueError("actuators: row %d: %s must be >= 0, got %r" % (b, FIELDS[k], r[k]))
        if r[P_COULOMB] > 0.0 and not r[P_VEPS] > 0.0:
            raise ValueError("actuators: row %d: coulomb > 0 needs v_eps > 0" % b)
        if r[P_SAT] > 0.0 and limit is None:
            raise ValueError("actuators: row %d: sat > 0 needs the effort limits (limit)" % b)
    out = [p]
    for name, a in (("limit", limit), ("friction_shape", shape)):
        if a is not None:
            a = np.asarray(a, dtype=float)
            if a.ndim != 1 or not np.all(np.isfinite(a)) or np.any(a < 0.0):
                raise ValueError("actuators: %s must be a finite vector of nu entries >= 0" % name)
        out.append(a)
    if out[1] is not None and out[2] is not None and out[1].shape != out[2].shape:
        raise ValueError("actuators: limit and friction_shape must both have nu entries")
    return tuple(out)


def unpack(state, nu):
    """(B, width(nu)) rows -> dict: ``ring`` (B, RING, nu), ``y`` (B, nu), ``applied`` (B, nu), ``head`` (B,), ``count`` (B,) (views of ``state``)"""
    nu = int(nu)
    s = np.asarray(state, dtype=float)
    if s.ndim != 2 or s.shape[1] != width(nu):
        raise ValueError("actuators: state rows of shape (B, %d) expected, got %s" % (width(nu), s.shape))
    o = RING * nu
    return {"ring": s[:, :o].reshape(-1, RING, nu), "y": s[:, o:o + nu], "applied": s[:, o + nu:o + 2 * nu], "head": s[:, o + 2 * nu],
            "count": s[:, o + 2 * nu + 1]}


def commands(state, nu, n):
    """the latest ``n`` <= RING commands held by the rings, oldest first -> (n, B, nu)"""
    s = unpack(state, nu)
    n = int(n)
    if not 0 <= n <= RING or np.any(s["count"] < n):
        raise ValueError("actuators: the rings do not hold %d commands" % n)
    b = np.arange(s["ring"].shape[0])
    return np.array([s["ring"][b, (s["head"].astype(int) - (n - 1 - i)) % RING] for i in range(n)])


def step(state, params, u, v, dt, limit=None, shape=None):
    """One step of the model for B robots (module docstring) -> the applied torques (B, nu); ``state`` (B, width(nu)) is updated in place.
    params (B, PARAMS); u (B, nu) the commanded torques; v (B, nu) the joint velocities of the states the step starts from; ``dt`` its length."""
    u, v = np.asarray(u, dtype=float), np.asarray(v, dtype=float)
    B, nu = u.shape
    p, limit, shape = validate(np.asarray(params, dtype=float).reshape(B, PARAMS), limit, shape)
    if not isinstance(state, np.ndarray) or state.dtype != np.float64 or state.shape != (B, width(nu)):
        raise ValueError("actuators: state must be a float64 array of shape (%d, %d)" % (B, width(nu)))
    dt = float(dt)
    s = unpack(state, nu)
    out = np.zeros((B, nu))
    for b in range(B):
        delay, scale, tc, damping, coulomb, v_eps, sat = p[b, :7]
        head = (int(s["head"][b]) + 1) % RING
        count = s["count"][b] + 1.0
        s["ring"][b, head] = u[b]
        back = int(min(delay, count - 1.0))
        ud = s["ring"][b, (head - back) % RING]
        w = scale * ud if scale != 1.0 else ud.copy()
        if tc == 0.0 or count == 1.0:
            y = w
        else:
            y = s["y"][b] + -np.expm1(-dt / tc) * (w - s["y"][b])
        s["y"][b] = y
        if sat > 0.0:
            lim = sat * limit
            y = np.minimum(np.maximum(y, -lim), lim)
        if damping > 0.0 or coulomb > 0.0:
            f = damping * v[b]
            if coulomb > 0.0:
                f = f + coulomb * np.tanh(v[b] / v_eps)
            y = y - (f if shape is None else shape * f)
        s["applied"][b] = y
        s["head"][b], s["count"][b] = float(head), count
        out[b] = y
    return out
