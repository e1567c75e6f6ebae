"""The per-robot base-state estimator of the torque-driven simulator, in numpy: one estimation event for B robots.  It is the definition the device
kernel (``mpc_sim_estimator``, include/mpc_sim_estimator.h, csrc/sim_estimator.h; ``NativeSolver.estimator`` / ``read_estimator`` /
``set_estimator``) is held to.  The estimator sits between "the sensors measured the state" and "the controllers read it": no robot measures its
floating base directly, it estimates the base from the joint encoders through the feet that stand (leg odometry) and lets an absolute measurement
correct the result slowly (a complementary filter).  What it returns is the ESTIMATE: the measured state with the base position and the base linear
velocity replaced.  The plant, its record, its metrics and its contact rule keep the true state; the sensor model keeps its measurement.

State layout: ``x = [q (nq = nv + 1: base position 3, base quaternion xyzw 4, joints nu) ; v (nv: base linear 3, base angular 3, joints nu)]``,
nu = nv - 6, nx = nq + nv.  The base linear velocity is expressed in the base frame.

Every robot has one parameter row of ``PARAMS`` = 16 doubles (``FIELDS``):

   0 ``w_p``   weight of the leg odometry in the base position, in [0, 1]; per event
   1 ``w_v``   weight of the leg odometry in the base linear velocity, in [0, 1]; per event
   2 - 15 reserved, 0

Every robot has one state row of ``width(nv)`` = nx + 17 doubles: ``est[nx]`` the latest estimate, ``held[2]`` the ``in_contact`` pair of the event
before, ``anchor[2][3]`` the world points the two soles' origins are taken to stand on, ``stats[8]`` and ``count`` (events since the reset).  Arming
is one event on the first measured states: ``count`` is 1 after it and an estimate is always held.

One event, from the measured state ``xm`` (the sensor model's measurement, or the true state without one), the robot's ``in_contact`` pair ``c`` of
the contact rule as the rule left it after this step, and the true state ``xt`` (for the statistics only):

  1. kinematics at ``xk`` = ``xm`` with the base position and the base linear velocity set to 0 (orientation, angular velocity, joints and joint
     velocities are the measured ones): for each sole i (the two contact frames of the model) ``r_i`` is the world position of the sole's origin and
     ``u_i`` the world velocity of that point (``sole_kinematics``).
  2. ``count`` + 1.  kept: the soles with ``c_i`` = 1 and ``held_i`` = 1 and ``count`` > 1; new: the soles with ``c_i`` = 1 that are not kept.
  3. position odometry: ``p_odo`` = the mean over the kept soles of ``anchor_i - r_i`` (two: ``0.5 (a + b)``); no sole kept: ``p_odo = p_m``.
  4. velocity odometry, over all soles with ``c_i`` = 1: ``v_odo = - R_b^T mean(u_i)``, ``R_b`` the measured base rotation; none: ``v_odo = v_m``.
  5. ``p_hat = p_m`` if ``w_p`` == 0, else ``p_m + w_p (p_odo - p_m)``.
  6. ``v_hat`` likewise with ``w_v``.
  7. drift correction: every kept anchor ``+= p_hat - p_odo``; nothing is added when ``w_p`` == 1 (pure odometry never moves an anchor); with
     ``w_p`` == 0 the anchors follow the measurement entirely.
  8. new soles: ``anchor_i = p_hat + r_i``.
  9. ``held = c``.
 10. ``est`` = ``xm`` with ``p_hat`` and ``v_hat`` in place of the base position and the base linear velocity.
 11. statistics, skipped on the arming event (``count`` == 1), of the errors against ``xt``: ``stats[0:4]`` for ``est`` the sum of |p error|^2, the
     sum of |v_lin error|^2, the largest |p error| and the largest |v_lin error| (Euclidean norms of the 3-vectors); ``stats[4:8]`` the same four
     for ``xm``: what the estimator gains over the raw measurement, read without a record.

The identity row ``IDENTITY`` (sixteen zeros) takes none of the arithmetic branches of 5 and 6: the estimate is the measurement bit for bit."""
from __future__ import annotations

import numpy as np

from .robot import minipin as pin

FIELDS = ("w_p", "w_v") + tuple("reserved%d" % i for i in range(14))
NAMED = FIELDS[:2]
PARAMS = len(FIELDS)         # MPC_SIM_ESTIMATOR_PARAMS
IDENTITY = (0.0,) * PARAMS
P_W_P, P_W_V = 0, 1
TAIL = 17                    # held 2, anchor 6, stats 8, count 1
STATS = ("est_sum_p2", "est_sum_v2", "est_max_p", "est_max_v", "meas_sum_p2", "meas_sum_v2", "meas_max_p", "meas_max_v")


def width(nv):
    """doubles of one robot's state row"""
    return 2 * int(nv) + 1 + TAIL


def rows(params, batch):
    """The forms the Python interfaces take -> (B, PARAMS) float64: ``(B, 16)`` rows, one row of 16 (for every robot), or a dict by ``FIELDS`` name
    of scalars or (B,) arrays, missing fields 0 (the identity)."""
    B = int(batch)
    if isinstance(params, dict):
        bad = sorted(set(params) - set(NAMED))
        if bad:
            raise ValueError("estimator: unknown fields %s (known: %s)" % (bad, ", ".join(NAMED)))
        out = np.tile(np.array(IDENTITY), (B, 1))
        for k, val in params.items():
            a = np.asarray(val, dtype=float)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
                raise ValueError("estimator: field %r is a scalar or a (B,) array with B = %d, got shape %s" % (k, B, a.shape))
            out[:, FIELDS.index(k)] = a
        return out
    p = np.asarray(params, dtype=float)
    if p.shape == (PARAMS,):
        return np.tile(p, (B, 1))
    if p.shape != (B, PARAMS):
        raise ValueError("estimator: params of shape (%d, %d), (%d,) or a dict by field name expected, got %s" % (B, PARAMS, PARAMS, p.shape))
    return np.ascontiguousarray(p)


def check(params):
    """The checks of ``mpc_sim_estimator`` (ValueError): rows (B, PARAMS) by the table of the module docstring -> params as a float64 array."""
    p = np.asarray(params, dtype=float)
    if p.ndim != 2 or p.shape[1] != PARAMS:
        raise ValueError("estimator: params of shape (B, %d) expected, got %s" % (PARAMS, p.shape))
    if not np.all(np.isfinite(p)):
        raise ValueError("estimator: non-finite parameters")
    for b, r in enumerate(p):
        for k in (P_W_P, P_W_V):
            if not 0.0 <= r[k] <= 1.0:
                raise ValueError("estimator: row %d: %s must be in [0, 1], got %r" % (b, FIELDS[k], r[k]))
        if np.any(r[2:] != 0.0):
            raise ValueError("estimator: row %d: the reserved entries must be 0" % b)
    return p


def unpack(state, nv):
    """(B, width(nv)) rows -> dict: ``est`` (B, nx), ``held`` (B, 2), ``anchor`` (B, 2, 3), ``stats`` (B, 8) (``STATS``), ``count`` (B,) (views of
    ``state``)"""
    nx = 2 * int(nv) + 1
    s = np.asarray(state, dtype=float)
    if s.ndim != 2 or s.shape[1] != width(nv):
        raise ValueError("estimator: state rows of shape (B, %d) expected, got %s" % (width(nv), s.shape))
    return {"est": s[:, :nx], "held": s[:, nx:nx + 2], "anchor": s[:, nx + 2:nx + 8].reshape(-1, 2, 3), "stats": s[:, nx + 8:nx + 16],
            "count": s[:, nx + 16]}


def sole_kinematics(model, frame_ids, x):
    """The soles of one robot at the state ``x`` (nx,): ``r`` (2, 3) the world positions of the origins of the frames ``frame_ids`` (left, right) and
    ``u`` (2, 3) the world velocities of those points.  Every joint on the way from the sole to the root adds its spatial velocity at the world
    origin, ``(p_j x w_j, w_j) v_j`` for a rotation about the world axis ``w_j`` through ``p_j`` and the body axes for the translations of the
    floating base; the point velocity is ``v_O + omega x r`` (csrc/body_kinematics.h cg_kinematics, in its order)."""
    nq = model.nq
    q, v = np.asarray(x[:nq], dtype=float), np.asarray(x[nq:], dtype=float)
    data = model.createData()
    pin.forwardKinematics(model, data, q)
    r, u = np.zeros((2, 3)), np.zeros((2, 3))
    for i, fid in enumerate(frame_ids):
        f = model.frames[fid]
        r[i] = data.oMi[f.parentJoint].rotation @ f.placement.translation + data.oMi[f.parentJoint].translation
        lin, ang = np.zeros(3), np.zeros(3)
        j = f.parentJoint
        while j > 0:
            jm, R, p = model.joints[j], data.oMi[j].rotation, data.oMi[j].translation
            k = jm.shortname()
            if k == "JointModelFreeFlyer":
                for d in range(3):
                    lin = lin + v[jm.idx_v + d] * R[:, d]
                for d in range(3):
                    lin = lin + v[jm.idx_v + 3 + d] * np.cross(p, R[:, d])
                    ang = ang + v[jm.idx_v + 3 + d] * R[:, d]
            else:
                w = R[:, pin._AXIS[k]]
                lin = lin + v[jm.idx_v] * np.cross(p, w)
                ang = ang + v[jm.idx_v] * w
            j = model.parents[j]
        u[i] = lin + np.cross(ang, r[i])
    return r, u


def _norm2(d):
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2]


def estimate(state, params, xm, in_contact, xt, model, frame_ids):
    """One event for B robots (module docstring) -> the estimates (B, nx); ``state`` (B, width(nv)) is advanced in place.  params (B, PARAMS); xm
    (B, nx) the measured states; in_contact (B, 2) the pair of the contact rule's rows after the step; xt (B, nx) the true states (statistics only);
    ``model``, ``frame_ids``: the robot model (minipin) and its two sole frames (left, right)."""
    nv = int(model.nv)
    nq, nx = nv + 1, 2 * nv + 1
    xm, xt = np.asarray(xm, dtype=float), np.asarray(xt, dtype=float)
    if xm.ndim != 2 or xm.shape[1] != nx or xt.shape != xm.shape:
        raise ValueError("estimator: measured and true states of shape (B, %d) expected, got %s and %s" % (nx, xm.shape, xt.shape))
    B = xm.shape[0]
    p = check(np.asarray(params, dtype=float).reshape(B, PARAMS))
    if not isinstance(state, np.ndarray) or state.dtype != np.float64 or state.shape != (B, width(nv)):
        raise ValueError("estimator: state must be a float64 array of shape (%d, %d)" % (B, width(nv)))
    c = np.asarray(in_contact, dtype=float)
    if c.shape != (B, 2) or np.any((c != 0.0) & (c != 1.0)):
        raise ValueError("estimator: in_contact of shape (%d, 2) with entries 0 or 1 expected" % B)
    s = unpack(state, nv)
    out = np.zeros((B, nx))
    for b in range(B):
        w_p, w_v = p[b, P_W_P], p[b, P_W_V]
        xk = xm[b].copy()
        xk[0:3] = 0.0
        xk[nq:nq + 3] = 0.0
        r, u = sole_kinematics(model, frame_ids, xk)
        Rb = pin.quat_to_rot(xk[3:7])
        count = s["count"][b] + 1.0
        anchor, held = s["anchor"][b], s["held"][b]
        on = [i for i in range(2) if c[b, i] != 0.0]
        kept = [i for i in on if held[i] != 0.0 and count > 1.0]
        new = [i for i in on if i not in kept]
        p_m, v_m = xm[b, 0:3].copy(), xm[b, nq:nq + 3].copy()
        if len(kept) == 2:
            p_odo = 0.5 * ((anchor[0] - r[0]) + (anchor[1] - r[1]))
        elif len(kept) == 1:
            p_odo = anchor[kept[0]] - r[kept[0]]
        else:
            p_odo = p_m
        if on:
            um = 0.5 * (u[0] + u[1]) if len(on) == 2 else u[on[0]]
            v_odo = -np.array([Rb[0, k] * um[0] + Rb[1, k] * um[1] + Rb[2, k] * um[2] for k in range(3)])
        else:
            v_odo = v_m
        p_hat = p_m if w_p == 0.0 else p_m + w_p * (p_odo - p_m)
        v_hat = v_m if w_v == 0.0 else v_m + w_v * (v_odo - v_m)
        if w_p != 1.0:
            for i in kept:
                anchor[i] = anchor[i] + (p_hat - p_odo)
        for i in new:
            anchor[i] = p_hat + r[i]
        held[:] = c[b]
        e = xm[b].copy()
        e[0:3] = p_hat
        e[nq:nq + 3] = v_hat
        s["est"][b] = e
        if count > 1.0:
            st = s["stats"][b]
            for o, z in ((0, e), (4, xm[b])):
                ep, ev = _norm2(z[0:3] - xt[b, 0:3]), _norm2(z[nq:nq + 3] - xt[b, nq:nq + 3])
                st[o] += ep
                st[o + 1] += ev
                st[o + 2] = max(st[o + 2], np.sqrt(ep))
                st[o + 3] = max(st[o + 3], np.sqrt(ev))
        s["count"][b] = count
        out[b] = e
    return out


def reset(params, x0, in_contact, model, frame_ids):
    """the state rows after ``mpc_sim_estimator(params, x0)``: zero rows, then the arming event on the measured states ``x0`` (B, nx) with the
    ``in_contact`` (B, 2) pair of the contact rule's rows -> (B, width(nv)); ``count`` is 1, every sole in contact is anchored at ``p_m + r_i``"""
    x0 = np.asarray(x0, dtype=float)
    nx = 2 * int(model.nv) + 1
    if x0.ndim != 2 or x0.shape[1] != nx:
        raise ValueError("estimator: initial states of shape (B, %d) expected, got %s" % (nx, x0.shape))
    state = np.zeros((x0.shape[0], width(model.nv)))
    estimate(state, rows(params, x0.shape[0]), x0, in_contact, x0, model, frame_ids)
    return state
