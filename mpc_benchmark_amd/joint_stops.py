"""The per-robot joint end-stops of the torque-driven simulator, in numpy: one step for B robots.  It is the definition the device kernel
(``mpc_sim_joint_stops``, include/mpc_sim_joint_stops.h, csrc/sim_joint_stops.h; ``NativeSolver.joint_stops`` / ``read_joint_stops`` /
``set_joint_stops``) is held to.  The model sits between "the actuators applied the torque of the step" and "the dynamics integrate it": an actuated
joint that stands beyond its range gets the torque of a one-sided spring and damper that pushes it back.  What ``step`` returns is the STOP torque
alone; the dynamics integrate the applied torque plus it (``integrated``).  A stop is not a motor: the ``tau`` of the loops, the record's torque
columns and the metrics' joint power and energy stay the actuators' torque.

Every robot has one parameter row of ``PARAMS`` doubles (``FIELDS``):

  0 ``k``    stiffness in ``scale[j]`` per rad, finite and >= 0
  1 ``d``    damping in ``scale[j]`` s per rad, finite and >= 0
  2 ``cap``  bound on ``|tau_stop_j|`` as a multiple of ``scale[j]``, > 0 (+inf: none)
  3 .. 7     reserved, 0

two tables ``lo`` and ``hi`` of shape (B, nu), nu = nv - 6, in rad: every robot's own range of every actuated joint (-inf / +inf: no stop on that
side; ``lo == hi``: a seized joint; ``lo > hi`` or NaN is refused), and one vector ``scale`` of nu entries in N m that all robots share (None: ones;
finite and > 0; the Python interfaces default it to the model's effort limits).

Every robot has one state row of ``width(nu)`` = 5 nu + 2 doubles: ``tau_stop[nu]`` (the stop torque the latest step integrated), ``pen[nu]`` (the
signed penetration of the state that step started from: ``q - hi`` > 0 above the range, ``q - lo`` < 0 below it, 0 inside or exactly on a limit),
``peak_pen[nu]`` (the largest ``|pen|`` so far), ``stop_steps[nu]`` (the steps in which the joint's stop acted: ``tau_stop != 0``), ``hits[nu]``
(the steps whose ``pen != 0`` followed a step with ``pen == 0``), ``any_steps`` (the steps in which any stop of the robot acted) and ``steps``.
After a reset everything is 0.

One step (a device loop's dt; the ``substeps * dt`` of one ``mpc_simulate_torque`` call, which holds the stop torque over its substeps), from
``q_j = x[7 + j]`` and ``v_j = x[nq + 6 + j]`` of the TRUE state the step STARTS from (never a sensor model's measurement), joint by joint:

  inside the range, ``lo <= q <= hi`` (always, with infinite limits):  ``tau_stop = 0``
  above ``hi``:  ``p = q - hi``,  ``t = max(0, k p + d v)``,  ``tau_stop = -scale_j min(t, cap)``
  below ``lo``:  ``p = lo - q``,  ``t = max(0, k p - d v)``,  ``tau_stop = +scale_j min(t, cap)``

(``t == 0``: ``tau_stop = +0``).  A stop only pushes back into the range and never pulls: the damper is cut off where it would hold a joint that is
already leaving.  With ``lo == hi`` the two branches together are a two-sided spring.  The dynamics integrate ``applied_j + tau_stop_j`` where
``tau_stop_j != 0`` and the applied torque itself elsewhere, so a robot none of whose stops acts keeps every bit.

The rule is explicit: it uses the state at the start of the step and holds the stop torque over the step.  It is stable only while
``scale_j k dt_step**2`` and ``scale_j d dt_step`` are small against the joint's reflected inertia; choosing ``k`` and ``d`` so is the caller's
business, nothing here checks it."""
from __future__ import annotations

import numpy as np

FIELDS = ("k", "d", "cap", "reserved3", "reserved4", "reserved5", "reserved6", "reserved7")
PARAMS = len(FIELDS)         # MPC_SIM_JOINT_STOPS_PARAMS
P_K, P_D, P_CAP = range(3)
IDENTITY = (0.0, 0.0, np.inf, 0.0, 0.0, 0.0, 0.0, 0.0)      # no spring, no damper: no stop ever acts, whatever the limits
# what a dict leaves out.  With scale = the effort limit: the full effort limit at 0.05 rad beyond a stop, twice that at the most.  Not measured yet
# on the light wrist and head joints (README)
DEFAULTS = (20.0, 0.02, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0)
PARTS = ("tau_stop", "pen", "peak_pen", "stop_steps", "hits")


def width(nu):
    """doubles of one robot's state row"""
    return 5 * int(nu) + 2


def reset(B, nu):
    """the state rows after ``mpc_sim_joint_stops(params, ...)``: (B, width(nu)) zeros"""
    return np.zeros((int(B), width(nu)))


def rows(params, batch):
    """The forms the Python interfaces take -> (B, PARAMS) float64: ``(B, 8)`` rows, one row of 8 (for every robot), or a dict by ``FIELDS`` name
    (``k``, ``d``, ``cap``) of scalars or (B,) arrays, missing fields as in ``DEFAULTS``."""
    B = int(batch)
    if isinstance(params, dict):
        bad = sorted(set(params) - set(FIELDS[:3]))
        if bad:
            raise ValueError("joint_stops: unknown fields %s (known: %s)" % (bad, ", ".join(FIELDS[:3])))
        out = np.tile(np.array(DEFAULTS), (B, 1))
        for k, val in params.items():
            a = np.asarray(val, dtype=float)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
                raise ValueError("joint_stops: field %r is a scalar or a (B,) array with B = %d, got shape %s" % (k, B, a.shape))
            out[:, FIELDS.index(k)] = a
        return out
    p = np.asarray(params, dtype=float)
    if p.shape == (PARAMS,):
        return np.tile(p, (B, 1))
    if p.shape != (B, PARAMS):
        raise ValueError("joint_stops: params of shape (%d, %d), (%d,) or a dict by field name expected, got %s" % (B, PARAMS, PARAMS, p.shape))
    return np.ascontiguousarray(p)


def validate(params, lo, hi, scale=None):
    """The checks of ``mpc_sim_joint_stops`` (ValueError): rows (B, PARAMS) by the table of the module docstring; ``lo`` and ``hi`` (B, nu) without
    NaN, ``lo <= hi``, ``lo`` < +inf and ``hi`` > -inf; ``scale`` (nu,) finite and > 0.  -> (params, lo, hi, scale) as float64 arrays (a ``scale`` of
    None stays None)."""
    p = np.asarray(params, dtype=float)
    if p.ndim != 2 or p.shape[1] != PARAMS:
        raise ValueError("joint_stops: params of shape (B, %d) expected, got %s" % (PARAMS, p.shape))
    B = p.shape[0]
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    if lo.ndim != 2 or lo.shape[0] != B or hi.shape != lo.shape:
        raise ValueError("joint_stops: lo and hi of shape (B, nu) with B = %d expected, got %s and %s" % (B, lo.shape, hi.shape))
    for b, r in enumerate(p):
        if not np.all(np.isfinite(r[:2])) or np.any(r[:2] < 0.0):
            raise ValueError("joint_stops: row %d: k and d must be finite and >= 0, got %r" % (b, tuple(r[:2])))
        if not r[P_CAP] > 0.0:
            raise ValueError("joint_stops: row %d: cap must be > 0 (+inf: none), got %r" % (b, r[P_CAP]))
        if np.any(r[3:] != 0.0):
            raise ValueError("joint_stops: row %d: the reserved entries must be 0" % b)
        if np.any(np.isnan(lo[b])) or np.any(np.isnan(hi[b])):
            raise ValueError("joint_stops: row %d: a limit is NaN" % b)
        if np.any(lo[b] > hi[b]):
            raise ValueError("joint_stops: row %d: lo > hi (joint %d)" % (b, int(np.argmax(lo[b] > hi[b]))))
        if np.any(lo[b] == np.inf) or np.any(hi[b] == -np.inf):
            raise ValueError("joint_stops: row %d: lo must be < +inf and hi > -inf" % b)
    if scale is not None:
        scale = np.asarray(scale, dtype=float)
        if scale.shape != (lo.shape[1],) or not np.all(np.isfinite(scale)) or np.any(scale <= 0.0):
            raise ValueError("joint_stops: scale must be a finite vector of nu = %d entries > 0" % lo.shape[1])
    return p, np.ascontiguousarray(lo), np.ascontiguousarray(hi), scale


def unpack(state, nu):
    """(B, width(nu)) rows -> dict: ``tau_stop``, ``pen``, ``peak_pen``, ``stop_steps``, ``hits`` (B, nu), ``any_steps``, ``steps`` (B,) (views of
    ``state``)"""
    nu = int(nu)
    s = np.asarray(state, dtype=float)
    if s.ndim != 2 or s.shape[1] != width(nu):
        raise ValueError("joint_stops: state rows of shape (B, %d) expected, got %s" % (width(nu), s.shape))
    out = {name: s[:, i * nu:(i + 1) * nu] for i, name in enumerate(PARTS)}
    out["any_steps"], out["steps"] = s[:, 5 * nu], s[:, 5 * nu + 1]
    return out


def step(state, rows, lo, hi, q, v, scale=None):
    """One step of the model for B robots (module docstring) -> the stop torques (B, nu); ``state`` (B, width(nu)) is updated in place.  rows
    (B, PARAMS); lo, hi (B, nu); q, v (B, nu) the joint positions ``x[7:nq]`` and velocities ``x[nq + 6:]`` of the true states the step starts from."""
    q, v = np.asarray(q, dtype=float), np.asarray(v, dtype=float)
    B, nu = q.shape
    p, lo, hi, scale = validate(np.asarray(rows, dtype=float).reshape(B, PARAMS), lo, hi, scale)
    if not isinstance(state, np.ndarray) or state.dtype != np.float64 or state.shape != (B, width(nu)):
        raise ValueError("joint_stops: state must be a float64 array of shape (%d, %d)" % (B, width(nu)))
    sc = np.ones(nu) if scale is None else scale
    s = unpack(state, nu)
    out = np.zeros((B, nu))
    for b in range(B):
        k, d, cap = p[b, :3]
        above, below = q[b] > hi[b], q[b] < lo[b]
        pen = np.zeros(nu)
        pen[above] = (q[b] - hi[b])[above]
        pen[below] = (q[b] - lo[b])[below]
        with np.errstate(invalid="ignore"):   # (inf - inf of the lanes np.where drops)
            t_hi = np.maximum(0.0, k * (q[b] - hi[b]) + d * v[b])
            t_lo = np.maximum(0.0, k * (lo[b] - q[b]) - d * v[b])
            tau = np.where(above & (t_hi > 0.0), -(sc * np.minimum(t_hi, cap)), np.where(below & (t_lo > 0.0), sc * np.minimum(t_lo, cap), 0.0))
        s["hits"][b] += (pen != 0.0) & (s["pen"][b] == 0.0)
        s["stop_steps"][b] += tau != 0.0
        s["tau_stop"][b], s["pen"][b] = tau, pen
        s["peak_pen"][b] = np.maximum(s["peak_pen"][b], np.abs(pen))
        s["any_steps"][b] += float(np.any(tau != 0.0))
        s["steps"][b] += 1.0
        out[b] = tau
    return out


def integrated(applied, tau_stop):
    """what the dynamics integrate: ``applied + tau_stop`` where a stop acts, the applied torque itself (an assignment, no add) elsewhere"""
    applied, tau_stop = np.asarray(applied, dtype=float), np.asarray(tau_stop, dtype=float)
    out = applied.copy()
    acts = tau_stop != 0.0
    out[acts] = applied[acts] + tau_stop[acts]
    return out


def limits(model, batch, range_scale=1.0, margin=0.0, lock=None):
    """``lo`` / ``hi`` tables (B, nu) from the model's ``lowerPositionLimit`` / ``upperPositionLimit`` of the actuated joints: every robot's range scaled
    about its middle by ``range_scale`` (a scalar, (B,) or (B, nu); a side without a limit stays without one, and the other side then stays where it
    is) and then shrunk on every finite side by ``margin`` rad (the same forms).  ``lock``: {robot: {joint: angle}} sets ``lo == hi == angle``, a
    seized joint; ``joint`` is the index among the actuated joints or a joint name of the model."""
    B = int(batch)
    lo0, hi0 = (np.asarray(a, dtype=float)[7:] for a in (model.lowerPositionLimit, model.upperPositionLimit))
    nu = lo0.shape[0]

    def table(a, name):
        a = np.asarray(a, dtype=float)
        if a.ndim == 1 and a.shape == (B,):
            a = a[:, None]
        try:
            return np.broadcast_to(a, (B, nu))
        except ValueError:
            raise ValueError("joint_stops: %s is a scalar, (B,) or (B, nu) with B = %d, nu = %d, got shape %s" % (name, B, nu, a.shape)) from None

    rs, mg = table(range_scale, "range_scale"), table(margin, "margin")
    if not np.all(np.isfinite(rs)) or np.any(rs < 0.0) or not np.all(np.isfinite(mg)):
        raise ValueError("joint_stops: range_scale must be finite and >= 0, margin finite")
    lo, hi = np.tile(lo0, (B, 1)), np.tile(hi0, (B, 1))
    both = np.isfinite(lo) & np.isfinite(hi) & (rs != 1.0)   # (a range scaled by 1 keeps the model's limits bit for bit)
    mid, half = 0.5 * (lo0 + hi0), 0.5 * (hi0 - lo0)
    lo[both] = (mid - half * rs)[both]
    hi[both] = (mid + half * rs)[both]
    lo = np.where(np.isfinite(lo), lo + mg, lo)
    hi = np.where(np.isfinite(hi), hi - mg, hi)
    if np.any(lo > hi):
        b, j = np.argwhere(lo > hi)[0]
        raise ValueError("joint_stops: the margin leaves no range (robot %d, joint %d)" % (b, j))
    for b, joints in (lock or {}).items():
        if not 0 <= int(b) < B:
            raise ValueError("joint_stops: lock names robot %r of %d" % (b, B))
        for j, angle in joints.items():
            if isinstance(j, str):
                jid = model.getJointId(j)
                if jid >= len(model.names):
                    raise ValueError("joint_stops: lock names the unknown joint %r" % j)
                j = model.joints[jid].idx_q - 7
            if not 0 <= int(j) < nu or not np.isfinite(angle):
                raise ValueError("joint_stops: lock takes a finite angle of an actuated joint 0 .. %d, got joint %r, angle %r" % (nu - 1, j, angle))
            lo[int(b), int(j)] = hi[int(b), int(j)] = float(angle)
    return lo, hi
