"""Per-robot sole tipping in the torque-driven simulator, in numpy: one update for B robots.  It is the definition the device kernel
(``mpc_sim_tipping``, include/mpc_sim_tipping.h, csrc/sim_tipping.h; ``NativeSolver.tipping`` / ``read_tipping`` / ``set_tipping``) is held to.

Why tipping is a velocity.  The contacts of the simulator carry ``Kp = (0, 0, 10, 0, 0, 0)`` and ``Kd = 50``: in roll and pitch a sole held by the
contact rule is held by VELOCITY alone and transmits any moment, so the plant never tests the bound the controllers plan with, the centre of pressure
inside the sole.  With this model on the contact row of the dynamics becomes ``acb + Kd (vcb - vs) - Kp e`` with
``vs = friction's (v_x, v_y, 0, 0, 0, w_z) + (0, 0, v_z, w_x, w_y, 0)`` in the contact's LOCAL frame: the two models fill disjoint components.

Frame and signs.  The sole is the rectangle ``|x| <= L``, ``|y| <= W`` about the origin of the contact's LOCAL frame; ``w = (f, tau)`` is the
step's LOCAL wrench, ground on robot, ``n = max(f_z, 0)``.  The ground can supply ``|tau_x| <= W n`` and ``|tau_y| <= L n``.  Each axis a (roll about
x with the extent ``h = W`` and the moment ``tau_x``, pitch about y with ``h = L`` and ``tau_y``) has a rate ``w_a`` and an accumulated angle
``th_a`` whose sign says which edge carries the sole: ``th_x > 0`` the edge ``y = -W``, ``th_x < 0`` the edge ``y = +W``, ``th_y > 0`` the edge
``x = +L``, ``th_y < 0`` the edge ``x = -L``.

Every robot has one parameter row of ``PARAMS`` = 8 doubles (``FIELDS``): ``half_length`` (L) of the left and the right sole, ``half_width`` (W) of
each (``+inf`` is the identity of that axis, by an explicit ``isinf`` test, and the default), ``I_tip`` (kg m^2), ``w_max`` (rad/s), ``th_max``
(rad), all finite and > 0, and one reserved entry that must be 0.

Every robot has one state row of ``WIDTH`` = 21 doubles: ``(v_z, w_x, w_y)`` of sole 0 and of sole 1 (the velocities the NEXT step is integrated
with), ``(th_x, th_y)`` of each sole, ``tipping[2]``, ``tip_steps[2]``, ``peak_angle[2]``, ``peak_excess[2]`` (N m), ``landings[2]``, ``steps``.

One update, after the contact rule and after friction of a step of length ``dt``, per sole:

  1. The step just integrated is accounted, if ``w_x`` or ``w_y`` is not 0 (a sole at rest touches nothing): ``tip_steps + 1``; per axis
     ``th_a += w_a dt``, and if ``th_a`` was not 0 before and ``th_a_new th_a_old <= 0`` the sole has landed on that axis: ``th_a = 0``,
     ``w_a = 0``, ``landings + 1``; ``peak_angle = max(peak_angle, |th_x|, |th_y|)``.  The sole's anchor (R2, p) in the contact rule's row follows
     the LOCAL twist the step was integrated with: ``p += R2[:, 2] v_z dt``, then ``R2 <- R2 Exp((w_x, w_y, 0) dt)`` (Rodrigues).  The anchor must
     move, not only for reporting: ``Kp_z = 10`` acts on the anchor's height, and a sole rotating about an edge raises its origin.  A landing snaps
     the angle and the rate but NOT the anchor: the anchor keeps the rotation of the last, partial step, a leftover of second order in the angle
     and first order in ``dt``, on rows that carry ``Kp = 0`` (rotation) and so do not enter the dynamics.
  2. The rates of the next step.  A sole that is free after the contact rule: rates, angles and ``v_z`` all 0.  Otherwise per axis, with
     ``lim = h n``:
       ``h = +inf``: ``w_a = 0``.  Else
       flat at rest (``th_a == 0`` and ``w_a == 0``): ``excess = |tau_a| - lim``, ``peak_excess = max(peak_excess, excess)``, and if ``excess > 0``:
       ``w_a = -(dt / I_tip) excess sign(tau_a)``;
       otherwise, with ``s = sign(th_a)`` if ``th_a != 0`` else ``sign(w_a)``: ``w_a <- w_a - (dt / I_tip) (tau_a + s lim)``: an edge transmits
       exactly ``-s lim`` about the origin and the rate changes by what the constraint transmitted beyond that.  Tipping on and tipping back obey
       the same line; only the angle ends a tip.
       Then ``|w_a|`` is clamped to ``w_max``, and if ``|th_a| >= th_max`` and ``w_a th_a > 0``: ``w_a = 0``.
     ``v_z = s_x W w_x + s_y L w_y`` (an axis whose rate is 0 adds nothing): the velocity of the origin when the sole turns about the carrying
     edge, ``-w x r_edge``, which has only a z component.
  3. ``tipping = 1`` if a rate or an angle of the sole is not 0, else 0; ``steps + 1``.

Properties.  In a steady tip the ground moment about the origin is ``-s h n``: the CoP on the edge.  ``I_tip`` acts as added inertia at the sole and
is the whole regularisation error, as ``m_slip`` is friction's (``friction_model``).  Let G be the sole's effective rotational inertia times ``Kd``:
the update is stable while ``G dt / I_tip < 2``.  ``defaults`` gives ``I_tip = 2 Kd dt (bound)`` with ``bound`` the robot's inertia about the
horizontal axes through a sole origin at the nominal posture: the sum over the links of ``m_i r_i^2`` plus the link's largest principal inertia
(``r_i``: distance of the link's centre of mass from the axis; the larger of roll and pitch over both soles), so ``G dt / I_tip <= 0.5``.  The C-ABI
takes explicit values and checks only that they are finite and > 0."""
from __future__ import annotations

import numpy as np

FIELDS = ("half_length_left", "half_length_right", "half_width_left", "half_width_right", "I_tip", "w_max", "th_max", "reserved")
BOTH = {"half_length": (0, 1), "half_width": (2, 3)}   # dict shorthands: both soles
PARAMS = len(FIELDS)         # MPC_SIM_TIPPING_PARAMS
WIDTH = 21                   # MPC_SIM_TIPPING_WIDTH
P_LENGTH, P_WIDTH, P_I_TIP, P_W_MAX, P_TH_MAX, P_RESERVED = 0, 2, 4, 5, 6, 7
O_V, O_TH, O_TIPPING, O_TIP_STEPS, O_PEAK_ANGLE, O_PEAK_EXCESS, O_LANDINGS, O_STEPS = 0, 6, 10, 12, 14, 16, 18, 20
W_MAX, TH_MAX = 5.0, 0.5     # default bounds on the rate (rad/s) and the angle (rad)
IDENTITY = (np.inf,) * 4 + (1.0, W_MAX, TH_MAX, 0.0)   # (no axis ever tips: the slider's inertia is never read)
KD = 50.0                    # the derivative gain of the simulator's contacts (fulldynamic_talos.py:94)


def defaults(model, q, sole_frames, dt, kd=KD):
    """The identity row of a robot with the slider inertia of the module docstring -> (PARAMS,): ``I_tip = 2 kd dt (bound)``, ``bound`` the
    inertia about the horizontal axes through the origins of ``sole_frames`` (frame ids or names) at the posture ``q``; ``w_max``, ``th_max`` the
    module's."""
    from .robot import minipin as pin
    data = model.createData()
    pin.framesForwardKinematics(model, data, np.asarray(q, dtype=float))
    ids = [model.getFrameId(f) if isinstance(f, str) else int(f) for f in sole_frames]
    bound = 0.0
    for fid in ids:
        o = np.asarray(data.oMf[fid].translation, dtype=float)
        roll, pitch = 0.0, 0.0
        for j in range(1, model.njoints):
            Y = model.inertias[j]
            c = np.asarray(data.oMi[j].rotation) @ np.asarray(Y.lever, dtype=float) + np.asarray(data.oMi[j].translation) - o
            principal = float(np.max(np.linalg.eigvalsh(np.asarray(Y.inertia, dtype=float))))
            roll += Y.mass * float(c[1] ** 2 + c[2] ** 2) + principal
            pitch += Y.mass * float(c[0] ** 2 + c[2] ** 2) + principal
        bound = max(bound, roll, pitch)
    row = np.array(IDENTITY)
    row[P_I_TIP] = 2.0 * kd * dt * bound
    return row


def rows(params, batch, base=None):
    """The forms the Python interfaces take -> (B, PARAMS) float64: ``(B, 8)`` rows, one row of 8 (for every robot), or a dict by ``FIELDS`` name
    (and ``half_length`` / ``half_width`` for both soles) of scalars or (B,) arrays, missing fields as in ``base`` (a row of 8, e.g. ``defaults``;
    None: ``IDENTITY``, and then a dict with a finite extent must name ``I_tip``: it depends on the robot)."""
    B = int(batch)
    if isinstance(params, dict):
        bad = sorted(set(params) - set(FIELDS) - set(BOTH))
        if bad:
            raise ValueError("tipping: unknown fields %s (known: %s)" % (bad, ", ".join(tuple(BOTH) + FIELDS)))
        out = np.tile(np.array(IDENTITY if base is None else base, dtype=float).reshape(PARAMS), (B, 1))
        for k, val in sorted(params.items(), key=lambda kv: kv[0] not in BOTH):   # (the shorthands first: a named sole overrides them)
            a = np.asarray(val, dtype=float)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
                raise ValueError("tipping: field %r is a scalar or a (B,) array with B = %d, got shape %s" % (k, B, a.shape))
            for col in BOTH.get(k, ()) or (FIELDS.index(k),):
                out[:, col] = a
        if base is None and np.any(np.isfinite(out[:, :4])) and "I_tip" not in params:
            raise ValueError("tipping: a finite half_length or half_width needs I_tip (tipping_model.defaults(model, q, sole_frames, dt) computes it "
                             "for a robot)")
        return out
    p = np.asarray(params, dtype=float)
    if p.shape == (PARAMS,):
        return np.tile(p, (B, 1))
    if p.shape != (B, PARAMS):
        raise ValueError("tipping: params of shape (%d, %d), (%d,) or a dict by field name expected, got %s" % (B, PARAMS, PARAMS, p.shape))
    return np.ascontiguousarray(p)


def validate(params):
    """The checks of ``mpc_sim_tipping`` (ValueError): rows (B, PARAMS) -> params as a float64 array."""
    p = np.asarray(params, dtype=float)
    if p.ndim != 2 or p.shape[1] != PARAMS:
        raise ValueError("tipping: params of shape (B, %d) expected, got %s" % (PARAMS, p.shape))
    for b, r in enumerate(p):
        for k in range(4):
            if np.isnan(r[k]) or r[k] < 0.0:
                raise ValueError("tipping: row %d: %s must be >= 0 (+inf: never tips), got %r" % (b, FIELDS[k], r[k]))
        for k in (P_I_TIP, P_W_MAX, P_TH_MAX):
            if not np.isfinite(r[k]) or not r[k] > 0.0:
                raise ValueError("tipping: row %d: %s must be finite and > 0, got %r" % (b, FIELDS[k], r[k]))
        if r[P_RESERVED] != 0.0:
            raise ValueError("tipping: row %d: the reserved entry must be 0, got %r" % (b, r[P_RESERVED]))
    return p


def unpack(state):
    """(B, WIDTH) rows -> dict: ``v`` (B, 2, 3) the (v_z, w_x, w_y) of each sole, ``th`` (B, 2, 2) the (th_x, th_y) of each, ``tipping``,
    ``tip_steps``, ``peak_angle``, ``peak_excess``, ``landings`` (B, 2), ``steps`` (B,) (views of ``state``)"""
    s = np.asarray(state, dtype=float)
    if s.ndim != 2 or s.shape[1] != WIDTH:
        raise ValueError("tipping: state rows of shape (B, %d) expected, got %s" % (WIDTH, s.shape))
    return {"v": s[:, O_V:O_TH].reshape(-1, 2, 3), "th": s[:, O_TH:O_TIPPING].reshape(-1, 2, 2), "tipping": s[:, O_TIPPING:O_TIP_STEPS],
            "tip_steps": s[:, O_TIP_STEPS:O_PEAK_ANGLE], "peak_angle": s[:, O_PEAK_ANGLE:O_PEAK_EXCESS],
            "peak_excess": s[:, O_PEAK_EXCESS:O_LANDINGS], "landings": s[:, O_LANDINGS:O_STEPS], "steps": s[:, O_STEPS]}


def reset(batch):
    """the state rows after arming -> (B, WIDTH): all 0"""
    return np.zeros((int(batch), WIDTH))


def _sign(x):
    return 1.0 if x > 0.0 else (-1.0 if x < 0.0 else 0.0)


def exp_rotation(wx, wy):
    """Rodrigues: Exp((wx, wy, 0)) -> (3, 3), the identity where both are 0"""
    t2 = wx * wx + wy * wy
    if t2 == 0.0:
        return np.eye(3)
    t = np.sqrt(t2)
    a, c = np.sin(t) / t, (1.0 - np.cos(t)) / t2
    # I + a K + c K K with K the cross-product matrix of (wx, wy, 0)
    return np.array([[1.0 - c * wy * wy, c * wx * wy, a * wy],
                     [c * wx * wy, 1.0 - c * wx * wx, -a * wx],
                     [-a * wy, a * wx, 1.0 - c * t2]])


def _axis(w, th, tau, h, n, k, wmax, thmax):
    """the law of one axis of a held sole -> (w, excess or None); ``k = dt / I_tip``"""
    if np.isinf(h):
        return 0.0, None
    lim, excess = h * n, None
    if th == 0.0 and w == 0.0:
        excess = abs(tau) - lim
        if excess > 0.0:
            w = -k * excess * _sign(tau)
    else:
        s = _sign(th) if th != 0.0 else _sign(w)
        w = w - k * (tau + s * lim)
    if abs(w) > wmax:
        w = wmax * _sign(w)
    if abs(th) >= thmax and w * th > 0.0:
        w = 0.0
    return w, excess


def step(rows, params, in_contact, wrenches, dt, anchors=None):
    """One update for B robots (module docstring); ``rows`` (B, WIDTH) is advanced in place and returned.  params (B, PARAMS); in_contact (B, 2) the
    pair of the contact rule's rows after the step; wrenches (B, 12) or (B, 2, 6) of the step; ``dt`` its length.  ``anchors``: None, or the
    (B, 2, 12) anchors of the contact rule's rows (R2 row-major 9, p 3; e.g. ``read_contacts()["anchor"]``), advanced in place."""
    if not isinstance(rows, np.ndarray) or rows.dtype != np.float64 or rows.ndim != 2 or rows.shape[1] != WIDTH:
        raise ValueError("tipping: rows must be a float64 array of shape (B, %d)" % WIDTH)
    B = rows.shape[0]
    p = validate(np.asarray(params, dtype=float).reshape(B, PARAMS))
    w = np.asarray(wrenches, dtype=float).reshape(B, 2, 6)
    t = np.asarray(in_contact, dtype=float)
    if t.shape != (B, 2):
        raise ValueError("tipping: in_contact of shape (%d, 2) expected" % B)
    if anchors is not None and (not isinstance(anchors, np.ndarray) or anchors.shape != (B, 2, 12)):
        raise ValueError("tipping: anchors must be an array of shape (%d, 2, 12)" % B)
    dt = float(dt)
    for b in range(B):
        r = rows[b]
        k, wmax, thmax = dt / p[b, P_I_TIP], p[b, P_W_MAX], p[b, P_TH_MAX]
        for i in range(2):
            vz, wx, wy = (float(x) for x in r[3 * i:3 * i + 3])
            th = [float(r[O_TH + 2 * i]), float(r[O_TH + 2 * i + 1])]
            if wx != 0.0 or wy != 0.0:
                r[O_TIP_STEPS + i] += 1.0
                rate = [wx, wy]
                for a in range(2):
                    old = th[a]
                    th[a] = old + rate[a] * dt
                    if old != 0.0 and th[a] * old <= 0.0:
                        th[a], rate[a] = 0.0, 0.0
                        r[O_LANDINGS + i] += 1.0
                r[O_PEAK_ANGLE + i] = max(r[O_PEAK_ANGLE + i], abs(th[0]), abs(th[1]))
                if anchors is not None:   # (with the twist the step was integrated with: a landing does not snap the anchor)
                    an = anchors[b, i]
                    R = an[:9].reshape(3, 3).copy()
                    an[9:] += R[:, 2] * (vz * dt)
                    an[:9] = (R @ exp_rotation(wx * dt, wy * dt)).reshape(9)
                wx, wy = rate
            if t[b, i] == 0.0:
                vz = wx = wy = 0.0
                th = [0.0, 0.0]
            else:
                n = max(float(w[b, i, 2]), 0.0)
                L, W = p[b, P_LENGTH + i], p[b, P_WIDTH + i]
                wx, ex = _axis(wx, th[0], float(w[b, i, 3]), W, n, k, wmax, thmax)
                wy, ey = _axis(wy, th[1], float(w[b, i, 4]), L, n, k, wmax, thmax)
                for e in (ex, ey):
                    if e is not None:
                        r[O_PEAK_EXCESS + i] = max(r[O_PEAK_EXCESS + i], e)
                vz = 0.0
                if wx != 0.0:
                    vz += (_sign(th[0]) if th[0] != 0.0 else _sign(wx)) * W * wx
                if wy != 0.0:
                    vz += (_sign(th[1]) if th[1] != 0.0 else _sign(wy)) * L * wy
            r[3 * i:3 * i + 3] = vz, wx, wy
            r[O_TH + 2 * i:O_TH + 2 * i + 2] = th
            r[O_TIPPING + i] = 1.0 if (wx != 0.0 or wy != 0.0 or th[0] != 0.0 or th[1] != 0.0) else 0.0
        r[O_STEPS] += 1.0
    return rows
