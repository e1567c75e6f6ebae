"""Per-robot ground friction under the soles of the torque-driven simulator, in numpy: one update for B robots.  It is the definition the device
kernel (``mpc_sim_friction``, include/mpc_sim_friction.h, csrc/sim_friction.h; ``NativeSolver.friction`` / ``read_friction`` / ``set_friction``) is
held to.

Why slip is a velocity.  The contacts of the simulator carry ``Kp = (0, 0, 10, 0, 0, 0)`` and ``Kd = 50`` on all six rows, and the contact row of
the dynamics is ``gamma = acb + Kd vcb - Kp e``: tangentially and in yaw a sole is held by VELOCITY only, and where its anchor lies in x, y and yaw
does not enter the dynamics.  Moving the anchor is therefore not slip.  With this model on the row becomes ``acb + Kd (vcb - vs) - Kp e`` with
``vs = (v_x, v_y, 0, 0, 0, w_z)`` in the contact's LOCAL frame: the velocity the sole is allowed to have.

Every robot has one parameter row of ``PARAMS`` = 8 doubles (``FIELDS``): ``mu`` of the left and the right sole, ``mu_spin`` (m) of each, ``m_slip``
(kg), ``I_slip`` (kg m^2), ``v_max`` (m/s), ``w_max`` (rad/s).  ``mu = +inf`` or ``mu_spin = +inf`` is the identity of that direction (and the default
of each field): it never slides, by an explicit ``isinf`` test.

Every robot has one state row of ``WIDTH`` = 17 doubles: ``(v_x, v_y, w_z)`` of sole 0 and of sole 1, ``sliding[2]``, ``slip_steps[2]``,
``slip_dist[2]``, ``slip_yaw[2]``, ``peak_excess[2]``, ``steps``.

One update, after the contact rule of a step of length ``dt``, per sole i with the step's LOCAL wrench ``w`` (ground on robot):

  1. The step just integrated is accounted with the velocities it was integrated with.  If any of them is not 0: ``slip_steps + 1``,
     ``slip_dist += |v| dt``, ``slip_yaw += |w_z| dt``, and the sole's anchor (R2, p) in the contact rule's row follows: ``p += R2 (v_x, v_y, 0) dt``,
     then ``R2 <- Rz(w_z dt) R2``.  A sole at rest touches nothing.
  2. The velocities of the next step.  A sole that is not in contact after the contact rule: ``v = 0``, ``w_z = 0``.  Otherwise, with
     ``n = max(f_z, 0)``, ``f = (f_x, f_y)``, ``|f| = sqrt(f_x f_x + f_y f_y)``, ``lim = mu n``:
       ``mu = +inf``: ``v = 0``.  Else ``peak_excess = max(peak_excess, |f| - lim)`` and
       sticking (``v == 0``): if ``|f| > lim``: ``v = -(dt / m_slip) (|f| - lim) f / |f|``;
       sliding: ``v_new = v - (dt / m_slip) (f + lim v / |v|)``; if ``dot(v_new, v) <= 0`` the sole sticks again (``v = 0``), else ``v = v_new``;
       then ``|v|`` is clamped to ``v_max``.
     Yaw: the same scalar law on ``w_z`` with ``tau_z``, ``lim_s = mu_spin n``, ``I_slip`` and ``w_max`` (no peak is kept).
  3. ``sliding = 1`` if a velocity of the sole is not 0, else 0; ``steps + 1``.

Properties.  In steady sliding the ground force is ``-(mu n) v / |v|``, kinetic Coulomb friction, plus ``m_slip dv/dt``: ``m_slip`` acts as added
mass at the sole, and that is the whole regularisation error.  (A block of mass M pushed by F whose constraint is ``a = -Kd (v_c - v)`` settles at
``a = (F - mu M g) / (M + m_slip)``.)  Let G be the sole's effective mass times ``Kd``: the update is stable while ``G dt / m_slip < 2``.
``defaults`` gives ``m_slip = 2 Kd_x dt (total mass)``, so ``G dt / m_slip <= 0.5`` for any effective mass up to the robot's, and ``I_slip``
likewise from a bound on the robot's yaw inertia about a sole origin at the nominal posture: the sum over the links of ``m_i r_i^2`` plus the
link's largest principal inertia (``r_i``: horizontal distance of the link's centre of mass from the sole's origin; the larger of the two soles).
The C-ABI takes explicit values and checks only that they are finite and > 0."""
from __future__ import annotations

import numpy as np

FIELDS = ("mu_left", "mu_right", "mu_spin_left", "mu_spin_right", "m_slip", "I_slip", "v_max", "w_max")
BOTH = {"mu": (0, 1), "mu_spin": (2, 3)}   # dict shorthands: both soles
PARAMS = len(FIELDS)         # MPC_SIM_FRICTION_PARAMS
WIDTH = 17                   # MPC_SIM_FRICTION_WIDTH
P_MU, P_MU_SPIN, P_M_SLIP, P_I_SLIP, P_V_MAX, P_W_MAX = 0, 2, 4, 5, 6, 7
O_V, O_SLIDING, O_SLIP_STEPS, O_SLIP_DIST, O_SLIP_YAW, O_PEAK, O_STEPS = 0, 6, 8, 10, 12, 14, 16
V_MAX, W_MAX = 2.0, 5.0      # default bounds on the slip speed (m/s) and the yaw slip rate (rad/s)
IDENTITY = (np.inf,) * 4 + (1.0, 1.0, V_MAX, W_MAX)   # (no direction ever slides: the slider's masses are never read)
KD = 50.0                    # the derivative gain of the simulator's contacts (fulldynamic_talos.py:94)


def defaults(model, q, sole_frames, dt, kd=KD):
    """The identity row of a robot with the slider masses of the module docstring -> (PARAMS,): ``m_slip = 2 kd dt (total mass)``, ``I_slip`` from
    the yaw-inertia bound at the posture ``q`` about the origins of ``sole_frames`` (frame ids or names), ``v_max``, ``w_max`` the module's."""
    from .robot import minipin as pin
    data = model.createData()
    pin.framesForwardKinematics(model, data, np.asarray(q, dtype=float))
    ids = [model.getFrameId(f) if isinstance(f, str) else int(f) for f in sole_frames]
    mass, bound = 0.0, 0.0
    for fid in ids:
        o = np.asarray(data.oMf[fid].translation, dtype=float)
        mass, yaw = 0.0, 0.0
        for j in range(1, model.njoints):
            Y = model.inertias[j]
            c = np.asarray(data.oMi[j].rotation) @ np.asarray(Y.lever, dtype=float) + np.asarray(data.oMi[j].translation)
            r2 = float((c[0] - o[0]) ** 2 + (c[1] - o[1]) ** 2)
            yaw += Y.mass * r2 + float(np.max(np.linalg.eigvalsh(np.asarray(Y.inertia, dtype=float))))
            mass += Y.mass
        bound = max(bound, yaw)
    row = np.array(IDENTITY)
    row[P_M_SLIP] = 2.0 * kd * dt * mass
    row[P_I_SLIP] = 2.0 * kd * dt * bound
    return row


def rows(params, batch, base=None):
    """The forms the Python interfaces take -> (B, PARAMS) float64: ``(B, 8)`` rows, one row of 8 (for every robot), or a dict by ``FIELDS`` name
    (and ``mu`` / ``mu_spin`` for both soles) of scalars or (B,) arrays, missing fields as in ``base`` (a row of 8, e.g. ``defaults``; None:
    ``IDENTITY``, and then a dict with a finite coefficient must name ``m_slip`` and ``I_slip``: they depend on the robot)."""
    B = int(batch)
    if isinstance(params, dict):
        bad = sorted(set(params) - set(FIELDS) - set(BOTH))
        if bad:
            raise ValueError("friction: unknown fields %s (known: %s)" % (bad, ", ".join(tuple(BOTH) + FIELDS)))
        out = np.tile(np.array(IDENTITY if base is None else base, dtype=float).reshape(PARAMS), (B, 1))
        for k, val in sorted(params.items(), key=lambda kv: kv[0] not in BOTH):   # (the shorthands first: a named sole overrides them)
            a = np.asarray(val, dtype=float)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
                raise ValueError("friction: field %r is a scalar or a (B,) array with B = %d, got shape %s" % (k, B, a.shape))
            for col in BOTH.get(k, ()) or (FIELDS.index(k),):
                out[:, col] = a
        if base is None and np.any(np.isfinite(out[:, :4])) and not ("m_slip" in params and "I_slip" in params):
            raise ValueError("friction: a finite mu or mu_spin needs m_slip and I_slip (friction_model.defaults(model, q, sole_frames, dt) "
                             "computes them for a robot)")
        return out
    p = np.asarray(params, dtype=float)
    if p.shape == (PARAMS,):
        return np.tile(p, (B, 1))
    if p.shape != (B, PARAMS):
        raise ValueError("friction: params of shape (%d, %d), (%d,) or a dict by field name expected, got %s" % (B, PARAMS, PARAMS, p.shape))
    return np.ascontiguousarray(p)


def validate(params):
    """The checks of ``mpc_sim_friction`` (ValueError): rows (B, PARAMS) -> params as a float64 array."""
    p = np.asarray(params, dtype=float)
    if p.ndim != 2 or p.shape[1] != PARAMS:
        raise ValueError("friction: params of shape (B, %d) expected, got %s" % (PARAMS, p.shape))
    for b, r in enumerate(p):
        for k in range(4):
            if np.isnan(r[k]) or r[k] < 0.0:
                raise ValueError("friction: row %d: %s must be >= 0 (+inf: never slides), got %r" % (b, FIELDS[k], r[k]))
        for k in range(4, PARAMS):
            if not np.isfinite(r[k]) or not r[k] > 0.0:
                raise ValueError("friction: row %d: %s must be finite and > 0, got %r" % (b, FIELDS[k], r[k]))
    return p


def unpack(state):
    """(B, WIDTH) rows -> dict: ``v`` (B, 2, 3) the (v_x, v_y, w_z) of each sole, ``sliding``, ``slip_steps``, ``slip_dist``, ``slip_yaw``,
    ``peak_excess`` (B, 2), ``steps`` (B,) (views of ``state``)"""
    s = np.asarray(state, dtype=float)
    if s.ndim != 2 or s.shape[1] != WIDTH:
        raise ValueError("friction: state rows of shape (B, %d) expected, got %s" % (WIDTH, s.shape))
    return {"v": s[:, O_V:O_SLIDING].reshape(-1, 2, 3), "sliding": s[:, O_SLIDING:O_SLIP_STEPS], "slip_steps": s[:, O_SLIP_STEPS:O_SLIP_DIST],
            "slip_dist": s[:, O_SLIP_DIST:O_SLIP_YAW], "slip_yaw": s[:, O_SLIP_YAW:O_PEAK], "peak_excess": s[:, O_PEAK:O_STEPS], "steps": s[:, O_STEPS]}


def reset(batch):
    """the state rows after arming -> (B, WIDTH): all 0"""
    return np.zeros((int(batch), WIDTH))


def _slide(vx, vy, fx, fy, lim, k, vmax):
    """the law of one direction pair -> (vx, vy, |f| - lim); ``k = dt / m_slip``"""
    fn = np.sqrt(fx * fx + fy * fy)
    if vx == 0.0 and vy == 0.0:
        if fn > lim:
            s = -k * (fn - lim)
            vx, vy = s * fx / fn, s * fy / fn
    else:
        vn = np.sqrt(vx * vx + vy * vy)
        nx, ny = vx - k * (fx + lim * vx / vn), vy - k * (fy + lim * vy / vn)
        vx, vy = (0.0, 0.0) if nx * vx + ny * vy <= 0.0 else (nx, ny)
    vn = np.sqrt(vx * vx + vy * vy)
    if vn > vmax:
        vx, vy = vx * vmax / vn, vy * vmax / vn
    return vx, vy, fn - lim


def step(rows, params, in_contact, wrenches, dt, anchors=None):
    """One update for B robots (module docstring); ``rows`` (B, WIDTH) is advanced in place and returned.  params (B, PARAMS); in_contact (B, 2) the
    pair of the contact rule's rows after the step; wrenches (B, 12) or (B, 2, 6) of the step; ``dt`` its length.  ``anchors``: None, or the
    (B, 2, 12) anchors of the contact rule's rows (R2 row-major 9, p 3; e.g. ``read_contacts()["anchor"]``), advanced in place."""
    if not isinstance(rows, np.ndarray) or rows.dtype != np.float64 or rows.ndim != 2 or rows.shape[1] != WIDTH:
        raise ValueError("friction: rows must be a float64 array of shape (B, %d)" % WIDTH)
    B = rows.shape[0]
    p = validate(np.asarray(params, dtype=float).reshape(B, PARAMS))
    w = np.asarray(wrenches, dtype=float).reshape(B, 2, 6)
    t = np.asarray(in_contact, dtype=float)
    if t.shape != (B, 2):
        raise ValueError("friction: in_contact of shape (%d, 2) expected" % B)
    if anchors is not None and (not isinstance(anchors, np.ndarray) or anchors.shape != (B, 2, 12)):
        raise ValueError("friction: anchors must be an array of shape (%d, 2, 12)" % B)
    dt = float(dt)
    for b in range(B):
        r = rows[b]
        for i in range(2):
            vx, vy, wz = (float(x) for x in r[3 * i:3 * i + 3])
            if vx != 0.0 or vy != 0.0 or wz != 0.0:
                r[O_SLIP_STEPS + i] += 1.0
                r[O_SLIP_DIST + i] += np.sqrt(vx * vx + vy * vy) * dt
                r[O_SLIP_YAW + i] += abs(wz) * dt
                if anchors is not None:
                    an = anchors[b, i]
                    R = an[:9].reshape(3, 3).copy()
                    an[9:] += (R[:, 0] * vx + R[:, 1] * vy) * dt
                    if wz != 0.0:
                        c, s = np.cos(wz * dt), np.sin(wz * dt)
                        an[0:3], an[3:6] = c * R[0] - s * R[1], s * R[0] + c * R[1]
            if t[b, i] == 0.0:
                vx = vy = wz = 0.0
            else:
                n = max(float(w[b, i, 2]), 0.0)
                mu, mu_spin = p[b, P_MU + i], p[b, P_MU_SPIN + i]
                if np.isinf(mu):
                    vx = vy = 0.0
                else:
                    vx, vy, excess = _slide(vx, vy, float(w[b, i, 0]), float(w[b, i, 1]), mu * n, dt / p[b, P_M_SLIP], p[b, P_V_MAX])
                    r[O_PEAK + i] = max(r[O_PEAK + i], excess)
                if np.isinf(mu_spin):
                    wz = 0.0
                else:
                    wz = _slide(wz, 0.0, float(w[b, i, 5]), 0.0, mu_spin * n, dt / p[b, P_I_SLIP], p[b, P_W_MAX])[0]
            r[3 * i:3 * i + 3] = vx, vy, wz
            r[O_SLIDING + i] = 1.0 if (vx != 0.0 or vy != 0.0 or wz != 0.0) else 0.0
        r[O_STEPS] += 1.0
    return rows
