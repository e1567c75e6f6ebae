"""The unilateral foot-contact rule of the torque-driven simulator, in numpy: one step for B robots.  It is the definition the device rule
(``mpc_sim_contacts``, include/mpc_sim_contacts.h; ``NativeSolver.contacts`` / ``read_contacts`` / ``set_contacts``) is held to, and it is
``BulletRobot._update_contacts`` applied to a batch, in the same order:

  feet 0 (left), then 1 (right); foot 0's release already counts for foot 1's "other foot in contact" test of the same step;
  - a foot in contact: ``pulling`` counts the consecutive steps whose LOCAL-frame normal force is below ``-release_force``; at
    ``release_steps`` the foot is released if the other foot is in contact (the last contact is never released), and ``lifted`` clears;
  - a free foot: above ``ground_z + 2 ground_tol`` it has ``lifted``; it is caught when it is back within ``ground_tol`` of the ground after
    lifting, or when it sinks below the ground plane (``z < ground_z`` and lower than the step before); the ground side of the caught contact
    is its landing pose flattened onto the plane: ``p = (x, y, ground_z)``, ``R = Rz(yaw)``;
  - ``z_prev`` of both feet becomes this step's sole height.

A robot's state is one row of ``WIDTH`` doubles (the layout of include/mpc_sim_contacts.h, ``FIELDS``).

Terrain (``mpc_sim_terrain``, include/mpc_sim_terrain.h; ``NativeSolver.terrain``): up to ``TERRAIN_MAX_BOXES`` axis-aligned boxes
``(x_lo, x_hi, y_lo, y_hi, z_top)`` per robot, one set for all robots ``(n, 5)`` or one per robot ``(B, n, 5)``.  The ground height is

    h(x, y) = max(ground_z, max{z_top of the boxes with x_lo <= x <= x_hi and y_lo <= y <= y_hi})

(closed intervals; boxes may overlap, the higher wins; a box below ``ground_z`` has no effect; comparisons and ``max`` only, so the device agrees
bit for bit).  The ground under sole i is ``g_i = h`` at the ORIGIN of the sole frame, and the rule is the one above with ``g_i`` in place of
``ground_z`` in the free-foot branch: lifted above ``g_i + 2 ground_tol``, caught within ``ground_tol`` of ``g_i`` after lifting or when sinking
below ``g_i``, the anchor at ``(x, y, g_i)``.  Without a terrain ``g_i`` is ``ground_z`` itself.  Deliberately not modelled, in keeping with a rule
that is not a physics engine: risers (nothing stops a foot horizontally), a sole that hangs over an edge, a toe inside the next step (only the
origin decides, so a toe that has crossed the next riser does not catch a descending foot on the step above), slopes.

The contact set of the low-level QPs (``mpc_qp_contact_source``, include/mpc_qp_contacts.h; ``BatchedQP.contact_source``, the pipelines'
``contact_source=``): ``qp_contact_states`` and ``qp_contact_counts`` below are the definition the device loops are held to.  Per robot, with ``s`` the
schedule's pair (what the plan's stage says) and ``p`` the rule's ``in_contact`` pair: ``"schedule"``: ``used = s``; ``"plant"``: ``used = p``;
``"both"``: ``used = s & p``, and a robot for which that is empty takes ``p`` (the rule never releases the last contact, so ``p`` holds one).  The QP of
step k reads the rows as they stand before step k: the state the rule left after step k - 1, which is the state the QP is solved at."""
from __future__ import annotations

import numpy as np

# (name, doubles) in the order of a row; MPC_SIM_CONTACTS_WIDTH = 41
FIELDS = (("in_contact", 2), ("lifted", 2), ("pulling", 2), ("z_prev", 2), ("anchor", 24), ("touchdowns", 2), ("liftoffs", 2),
          ("last_touchdown", 2), ("last_liftoff", 2), ("steps", 1))
WIDTH = sum(w for _, w in FIELDS)
O_IN, O_LIFTED, O_PULLING, O_ZPREV, O_ANCHOR, O_TD, O_LO, O_LAST_TD, O_LAST_LO, O_STEPS = 0, 2, 4, 6, 8, 32, 34, 36, 38, 40

# mpc_sim_contacts_config, in the order of its fields (``reserved`` is not a setting)
DEFAULTS = {
    "ground_z": 0.0,        # m: the ground plane (BulletRobot: the lower sole at initializeJoints; the pipelines: the lower initial foothold)
    "ground_tol": 5e-3,     # m: BulletRobot's ground_tol
    "release_force": 1.0,   # N: a contact pulls when its LOCAL-frame f_z < -release_force
    "release_steps": 5,     # consecutive pulling steps before the release (>= 1)
}


TERRAIN_MAX_BOXES = 16   # MPC_SIM_TERRAIN_MAX_BOXES
TERRAIN_BOX_WIDTH = 5    # MPC_SIM_TERRAIN_BOX_WIDTH: x_lo, x_hi, y_lo, y_hi, z_top


QP_SOURCES = {"schedule": 0, "plant": 1, "both": 2}   # MPC_QP_CONTACTS_SCHEDULE, _PLANT, _BOTH


def qp_source(source):
    """the name of a contact source, checked -> its value in ``QP_SOURCES``"""
    if not isinstance(source, str) or source not in QP_SOURCES:
        raise ValueError("contact_source: one of %s expected, got %r" % (", ".join(repr(k) for k in QP_SOURCES), source))
    return QP_SOURCES[source]


def _pairs(schedule, in_contact):
    p = (np.asarray(in_contact).reshape(-1, 2) != 0).astype(np.int32)
    s = (np.broadcast_to(np.asarray(schedule), p.shape) != 0).astype(np.int32)
    return s, p


def qp_contact_states(source, schedule, in_contact):
    """The contact set of every robot's low-level QP -> ``used`` (B, 2) int32.  ``source``: a name of ``QP_SOURCES``; ``schedule`` (2,) or (B, 2): the
    plan's contact state; ``in_contact`` (B, 2): columns 0 and 1 of the rule's rows (module docstring)."""
    k = qp_source(source)
    s, p = _pairs(schedule, in_contact)
    if k == QP_SOURCES["schedule"]:
        return s.copy()
    if k == QP_SOURCES["plant"]:
        return p.copy()
    both = s & p
    return np.where(both.any(axis=1, keepdims=True), both, p).astype(np.int32)


def qp_contact_counts(counts, schedule, in_contact):
    """One step of the count of plan against plant -> a copy of ``counts`` (B, 2, 4) int32 (None: zeros) with ``counts[b, c, 2 s + p] += 1``:
    index 0 both have the foot in the air, 3 both on the ground, 1 the plant holds a foot the plan has in the air, 2 the plan stands on a foot the
    plant has released."""
    s, p = _pairs(schedule, in_contact)
    out = np.zeros(p.shape + (4,), dtype=np.int32) if counts is None else np.array(counts, dtype=np.int32, copy=True).reshape(p.shape + (4,))
    b, c = np.indices(p.shape)
    out[b, c, 2 * s + p] += 1
    return out


def qp_zero_unused(forces, used):
    """``forces`` (B, 12) of a QP that worked with ``used`` (B, 2): the six components of a contact it did not use are 0 (a copy)."""
    f = np.array(forces, dtype=float, copy=True).reshape(-1, 2, 6)
    f[np.asarray(used).reshape(-1, 2) == 0] = 0.0
    return f.reshape(-1, 12)


def config(cfg=None, ground_z=None):
    """``cfg`` (dict or None) over ``DEFAULTS``; unknown keys are an error.  ``ground_z``: the default of the ground height when ``cfg`` names none."""
    out = dict(DEFAULTS)
    if ground_z is not None:
        out["ground_z"] = float(ground_z)
    if cfg:
        bad = sorted(set(cfg) - set(DEFAULTS))
        if bad:
            raise ValueError("contact rule: unknown configuration keys %s (known: %s)" % (bad, ", ".join(DEFAULTS)))
        out.update(cfg)
    for k in out:
        out[k] = int(out[k]) if k == "release_steps" else float(out[k])
    return out


def unpack(rows):
    """(B, WIDTH) rows -> dict of arrays by ``FIELDS`` name: flags and counters (B, 2) (``steps`` (B,)), ``anchor_R`` (B, 2, 3, 3), ``anchor_p`` (B, 2, 3)."""
    rows = np.asarray(rows, dtype=float)
    out, o = {}, 0
    for name, w in FIELDS:
        out[name] = rows[:, o] if w == 1 else rows[:, o:o + w]
        o += w
    a = out.pop("anchor").reshape(-1, 2, 12)
    out["anchor_R"], out["anchor_p"] = a[..., :9].reshape(-1, 2, 3, 3), a[..., 9:]
    return out


def reset_rows(anchor_R, anchor_p):
    """The rows after ``mpc_sim_contacts(cfg)``: both soles in contact at the anchors (R (B, 2, 3, 3) or (2, 3, 3), p (B, 2, 3) or (2, 3): the model's
    ground-side contact placements), nothing counted, ``z_prev`` the anchors' heights, no touchdown or lift-off yet (step index -1)."""
    R = np.asarray(anchor_R, dtype=float).reshape(-1, 2, 9)
    p = np.asarray(anchor_p, dtype=float).reshape(-1, 2, 3)
    B = max(R.shape[0], p.shape[0])
    R, p = np.broadcast_to(R, (B, 2, 9)), np.broadcast_to(p, (B, 2, 3))
    r = np.zeros((B, WIDTH))
    r[:, O_IN:O_IN + 2] = 1.0
    r[:, O_ZPREV:O_ZPREV + 2] = p[..., 2]
    r[:, O_ANCHOR:O_ANCHOR + 24] = np.concatenate([R, p], axis=-1).reshape(-1, 24)
    r[:, O_LAST_TD:O_LAST_LO + 2] = -1.0
    return r


def flatten(R, p, ground_z):
    """The landing pose of a sole flattened onto the ground plane: (Rz(yaw), (x, y, ground_z)), yaw = atan2(R[1, 0], R[0, 0])."""
    yaw = np.arctan2(R[1, 0], R[0, 0])
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]), np.array([p[0], p[1], ground_z])


def terrain_boxes(boxes, batch=None):
    """Checked boxes as float64: ``(n, 5)`` (shared) or ``(B, n, 5)`` (per robot; ``batch`` checks B), 0 <= n <= ``TERRAIN_MAX_BOXES``, finite,
    ``x_lo <= x_hi`` and ``y_lo <= y_hi``.  An empty sequence is zero shared boxes."""
    b = np.asarray(boxes, dtype=float)
    if b.size == 0 and b.ndim < 3:
        b = b.reshape(0, TERRAIN_BOX_WIDTH)
    if b.ndim not in (2, 3) or b.shape[-1] != TERRAIN_BOX_WIDTH:
        raise ValueError("terrain: boxes of shape (n, 5) or (B, n, 5) expected (x_lo, x_hi, y_lo, y_hi, z_top), got %s" % (b.shape,))
    if b.shape[-2] > TERRAIN_MAX_BOXES:
        raise ValueError("terrain: at most %d boxes per robot, got %d" % (TERRAIN_MAX_BOXES, b.shape[-2]))
    if b.ndim == 3 and batch is not None and b.shape[0] != batch:
        raise ValueError("terrain: per-robot boxes for %d robots expected, got %d" % (batch, b.shape[0]))
    if not np.all(np.isfinite(b)):
        raise ValueError("terrain: the boxes must be finite")
    if np.any(b[..., 0] > b[..., 1]) or np.any(b[..., 2] > b[..., 3]):
        raise ValueError("terrain: x_lo <= x_hi and y_lo <= y_hi expected")
    return np.ascontiguousarray(b)


def terrain_height(boxes, xy, ground_z):
    """h at the points ``xy`` (..., 2) of shared boxes ``(n, 5)``, or (B, ..., 2) of per-robot boxes ``(B, n, 5)`` (robot b's points on robot b's
    terrain) -> heights of shape ``xy.shape[:-1]``."""
    b = terrain_boxes(boxes)
    xy = np.asarray(xy, dtype=float)
    h = np.full(xy.shape[:-1], float(ground_z))
    if b.ndim == 3 and (xy.ndim < 2 or xy.shape[0] != b.shape[0]):
        raise ValueError("terrain_height: per-robot boxes need points of shape (B, ..., 2) with B = %d, got %s" % (b.shape[0], xy.shape))
    x, y = xy[..., 0], xy[..., 1]
    for k in range(b.shape[-2]):
        # (+ 0.0: a top of -0 counts as +0, on the device too, so that equal tops are equal bits whatever the order of the max)
        bk = b[k] if b.ndim == 2 else b[:, k].reshape((b.shape[0],) + (1,) * (xy.ndim - 2) + (TERRAIN_BOX_WIDTH,))
        inside = (bk[..., 0] <= x) & (x <= bk[..., 1]) & (bk[..., 2] <= y) & (y <= bk[..., 3])
        top = bk[..., 4] + 0.0
        h = np.where(inside & (top > h), top, h)
    return h


def stairs(pose_stairs, height_step, n_steps=3, pitch=0.3, half_extents=(0.2, 0.5)):
    """The boxes of the reference's ``createStairs(pose_stairs, height_step)`` (bullet_robot.py:275-340): step k is a box of half extents
    (0.2, 0.5, height_step / 2) centred at ``pose_stairs + (k pitch, 0, k height_step)``, so its top is at the centre's z + height_step / 2 and
    consecutive steps overlap by 0.1 m (the visible tread is ``pitch``).  -> (n_steps, 5), ``n_steps <= TERRAIN_MAX_BOXES``."""
    n_steps = int(n_steps)
    if not 0 <= n_steps <= TERRAIN_MAX_BOXES:
        raise ValueError("stairs: 0 .. %d steps, got %d" % (TERRAIN_MAX_BOXES, n_steps))
    p = np.asarray(pose_stairs, dtype=float).reshape(-1)
    if p.size != 3:
        raise ValueError("stairs: pose_stairs is a 3-vector")
    h, hx, hy = float(height_step), float(half_extents[0]), float(half_extents[1])
    out = np.zeros((n_steps, TERRAIN_BOX_WIDTH))
    for k in range(n_steps):
        cx, cz = p[0] + k * pitch, p[2] + k * h
        out[k] = (cx - hx, cx + hx, p[1] - hy, p[1] + hy, cz + h / 2)
    return out


def step(rows, sole_z, fz, sole_R, sole_p, cfg=None, terrain=None):
    """One step of the rule for B robots -> the new rows (a copy).  rows (B, WIDTH); sole_z (B, 2) the sole heights of the state AFTER the step;
    fz (B, 2) the step's LOCAL-frame normal forces (0 for a free foot); sole_R (B, 2, 3, 3), sole_p (B, 2, 3) the sole placements after the step
    (a catch reads them, and the terrain the origins' x, y); ``cfg`` over ``DEFAULTS``; ``terrain``: None, or boxes (n, 5) / (B, n, 5): the ground
    under sole i is ``terrain_height`` at ``sole_p[b, i, :2]`` instead of ``ground_z`` (module docstring)."""
    c = config(cfg)
    gz, tol, rf, rs = c["ground_z"], c["ground_tol"], c["release_force"], c["release_steps"]
    r = np.array(rows, dtype=float, copy=True).reshape(-1, WIDTH)
    sole_z, fz = np.asarray(sole_z, dtype=float).reshape(-1, 2), np.asarray(fz, dtype=float).reshape(-1, 2)
    sole_R, sole_p = np.asarray(sole_R, dtype=float).reshape(-1, 2, 3, 3), np.asarray(sole_p, dtype=float).reshape(-1, 2, 3)
    ground = None
    if terrain is not None:
        boxes = terrain_boxes(terrain, r.shape[0])
        ground = terrain_height(boxes, sole_p[..., :2], gz)
    plane = gz
    for b in range(r.shape[0]):
        row = r[b]
        n = row[O_STEPS]
        for i in range(2):
            z = sole_z[b, i]
            gz = plane if ground is None else ground[b, i]
            if row[O_IN + i] != 0.0:
                row[O_PULLING + i] = row[O_PULLING + i] + 1.0 if fz[b, i] < -rf else 0.0
                if row[O_PULLING + i] >= rs and row[O_IN] + row[O_IN + 1] > 1.0:
                    row[O_IN + i] = row[O_LIFTED + i] = row[O_PULLING + i] = 0.0
                    row[O_LO + i] += 1.0
                    row[O_LAST_LO + i] = n
            elif z > gz + 2.0 * tol:
                row[O_LIFTED + i] = 1.0
            elif (z <= gz + tol and row[O_LIFTED + i] != 0.0) or (z < gz and z < row[O_ZPREV + i]):
                R, p = flatten(sole_R[b, i], sole_p[b, i], gz)
                row[O_ANCHOR + 12 * i:O_ANCHOR + 12 * i + 9] = R.reshape(-1)
                row[O_ANCHOR + 12 * i + 9:O_ANCHOR + 12 * i + 12] = p
                row[O_IN + i] = 1.0
                row[O_TD + i] += 1.0
                row[O_LAST_TD + i] = n
            row[O_ZPREV + i] = z
        row[O_STEPS] = n + 1.0
    return r
