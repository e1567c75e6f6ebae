"""Locomotion metrics of a simulated run, in numpy: the definitions the device accumulates per robot after every torque-driven simulator step
(``mpc_sim_metrics``, include/mpc_sim_metrics.h; ``NativeSolver.metrics`` / ``read_metrics``), and what its tests compare against.

They are plot.py's evaluation of a recorded run of the scripts, reduced to one row per robot:
  - the centre of pressure of the two sole wrenches (talos_utils.computeCoP, ``trajectory_log.compute_cop``) against plot.py's support box
    of the loaded feet (plot.py:123-164): how many steps it left the box, and the signed margin to the box's edges;
  - the centroidal momentum, and the angular momentum about z that plot.py:348-355 plots;
  - joint power ``sum |u * v_joints|`` and dissipated energy ``sum(power) * dt`` (plot.py:488-520), with ``u[i]`` paired with the state
    ``x[i]`` it was computed from: the state the step STARTED from;
  - the fall verdict of tools/push_recovery.py (base more than 0.2 m below, or both soles more than 2 cm above, their heights after the first
    step; or a non-finite state).

On a handle with a terrain (``NativeSolver.terrain``, include/mpc_sim_terrain.h) the fall verdict is taken above the ground, so that a robot that
has climbed a step is not "fallen": sole i by ``z_i - g_i`` (``g_i`` the terrain height under the origin of the sole frame after the step, as the
contact rule takes it), the base by ``z_base - a``, ``a`` the mean anchor height of the soles in contact in the contact row the step was integrated
with; ``base_z0`` and ``sole_z0`` are latched in the same terms.  Nothing else in a row changes.

``from_record`` computes the row of every robot from the per-step record (``NativeSolver.read_record``) of the same steps."""
from __future__ import annotations

import numpy as np

from . import contact_rule as _contact_rule

# (name, doubles) in the order of a row; MPC_SIM_METRICS_WIDTH = 21
FIELDS = (("steps", 1), ("time", 1), ("energy", 1), ("peak_power", 1), ("cop_steps", 1), ("cop_outside", 1), ("margin_min", 1), ("margin_sum", 1),
          ("peak_h_lin", 1), ("peak_h_ang", 1), ("h_ang_z_sq", 1), ("fall_step", 1), ("base_z0", 1), ("sole_z0", 2), ("com_first", 3), ("com_last", 3))
WIDTH = sum(w for _, w in FIELDS)

# mpc_sim_metrics_config, in the order of its fields
DEFAULTS = {
    "min_force": 1.0,     # N: a sole is loaded when its LOCAL f_z exceeds this (talos_utils.computeCoP, plot.py:32, 40)
    "half_length": 0.1,   # m: FOOT_LENGTH of plot.py:123
    "half_width": 0.05,   # m: FOOT_WIDTH of plot.py:124
    "fall_drop": 0.2,     # m: fallen when the base is this far below its latched height (tools/push_recovery.py)
    "sole_lift": 0.02,    # m: fallen when BOTH soles are this far above their latched heights
}


def config(cfg=None):
    """``cfg`` (dict or None) over ``DEFAULTS``; unknown keys are an error."""
    out = dict(DEFAULTS)
    if cfg:
        bad = sorted(set(cfg) - set(DEFAULTS))
        if bad:
            raise ValueError("metrics: unknown configuration keys %s (known: %s)" % (bad, ", ".join(DEFAULTS)))
        out.update({k: float(v) for k, v in cfg.items()})
    return out


def unpack(rows):
    """(B, WIDTH) rows -> dict of (B,) arrays by ``FIELDS`` name; ``sole_z0`` (B, 2), ``com_first`` / ``com_last`` (B, 3)."""
    rows = np.asarray(rows, dtype=float)
    out, o = {}, 0
    for name, w in FIELDS:
        out[name] = rows[:, o] if w == 1 else rows[:, o:o + w]
        o += w
    return out


def reset_rows(batch):
    """The rows after a reset: nothing accumulated, no fall, nothing latched (NaN)."""
    r = np.zeros((batch, WIDTH))
    r[:, 6] = np.nan
    r[:, 11] = -1.0
    r[:, 12:] = np.nan
    return r


def cop(sole_R, sole_p, wrenches, min_force=DEFAULTS["min_force"]):
    """``trajectory_log.compute_cop`` over leading axes: sole_R (..., 2, 3, 3), sole_p (..., 2, 3), wrenches (..., 2, 6) in the sole frames (force,
    torque), [left, right].  -> (CoP (..., 3), NaN where no sole is loaded ; loaded (..., 2): f_z > min_force)."""
    sole_R, sole_p, wrenches = (np.asarray(a, dtype=float) for a in (sole_R, sole_p, wrenches))
    fz = wrenches[..., 2]
    loaded = fz > min_force
    with np.errstate(divide="ignore", invalid="ignore"):
        local = np.stack([-wrenches[..., 4] / fz, wrenches[..., 3] / fz, np.zeros_like(fz)], axis=-1)
        world = np.einsum("...ij,...j->...i", sole_R, local) + sole_p
        total = np.where(loaded[..., None], world * fz[..., None], 0.0)
        total = total[..., 0, :] + total[..., 1, :]
        fs = np.where(loaded[..., 0], fz[..., 0], 0.0) + np.where(loaded[..., 1], fz[..., 1], 0.0)
        c = np.where((fs > 0.0)[..., None], total / fs[..., None], np.nan)
    return c, loaded


def support_box(sole_p, loaded, half_length=DEFAULTS["half_length"], half_width=DEFAULTS["half_width"]):
    """plot.py:145-164 over leading axes: sole_p (..., 2, 3) [left, right], loaded (..., 2).  -> (x_lo, x_hi, y_lo, y_hi), each (...).
    Both soles loaded (and, as in plot.py's last branch, neither): x from the rearmost sole - L to the foremost + L, y from the right sole - W to the
    left sole + W; one sole loaded: that sole +- L, +- W."""
    sole_p, loaded = np.asarray(sole_p, dtype=float), np.asarray(loaded, dtype=bool)
    pl, pr = sole_p[..., 0, :], sole_p[..., 1, :]
    lf, rf = loaded[..., 0], loaded[..., 1]
    one = lf != rf
    q = np.where(lf[..., None], pl, pr)  # the loaded sole where only one is
    x_lo = np.where(one, q[..., 0] - half_length, np.minimum(pl[..., 0], pr[..., 0]) - half_length)
    x_hi = np.where(one, q[..., 0] + half_length, np.maximum(pl[..., 0], pr[..., 0]) + half_length)
    y_lo = np.where(one, q[..., 1] - half_width, pr[..., 1] - half_width)
    y_hi = np.where(one, q[..., 1] + half_width, pl[..., 1] + half_width)
    return x_lo, x_hi, y_lo, y_hi


def margin(c, box):
    """signed distance of the point c (..., >= 2) to the edges of the box (x_lo, x_hi, y_lo, y_hi): positive inside"""
    x_lo, x_hi, y_lo, y_hi = box
    x, y = c[..., 0], c[..., 1]
    return np.minimum(np.minimum(x - x_lo, x_hi - x), np.minimum(y - y_lo, y_hi - y))


def joint_power(tau, x_before, nq):
    """plot.py:494-504: sum_j |u_j * v_j| with v = x_before[nq + 6:], x_before the state u was computed from.  tau (..., nu), x_before (..., nx)."""
    return np.sum(np.abs(np.asarray(tau) * np.asarray(x_before)[..., nq + 6:]), axis=-1)


def from_record(rec, x_start, dt, cfg=None, terrain=None, contact_rows=None, ground_z=0.0):
    """The metric rows of every robot over the recorded steps, as ``NativeSolver.read_metrics`` returns them after the same steps from a reset.
    ``rec``: the dict of ``NativeSolver.read_record`` (steps, B, ...); ``x_start`` (B, nx): the states the first recorded step started from;
    ``dt``: the length of each step, a scalar or (steps,) (substeps * dt of the call).  ``terrain``: None, or the boxes (n, 5) / (B, n, 5) of the
    handle's terrain over the plane ``ground_z`` (the contact rule's): the fall verdict above the ground (module docstring); it needs
    ``contact_rows`` (steps, B, ``contact_rule.WIDTH``), the rows of the contact rule each step was integrated with (before that step's update).
    Zero boxes are no terrain, as on the device."""
    c = config(cfg)
    if terrain is not None:
        terrain = _contact_rule.terrain_boxes(terrain, np.asarray(rec["x"]).shape[1])
        if terrain.shape[-2] == 0:
            terrain = None
    if terrain is not None:
        if contact_rows is None:
            raise ValueError("from_record: terrain needs contact_rows (the anchors the steps were integrated with)")
        contact_rows = np.asarray(contact_rows, dtype=float)
    x, tau = np.asarray(rec["x"], dtype=float), np.asarray(rec["tau"], dtype=float)
    S, B, nx = x.shape
    nq = nx - (tau.shape[2] + 6)
    dts = np.broadcast_to(np.asarray(dt, dtype=float), (S,))
    r = reset_rows(B)
    frozen = np.zeros(B, dtype=bool)
    x_before = np.asarray(x_start, dtype=float).reshape(B, nx)
    for k in range(S):
        xk = x[k]
        bad = ~np.all(np.isfinite(xk), axis=1) & ~frozen
        first_fall = bad & (r[:, 11] < 0)
        r[first_fall, 11] = r[first_fall, 0]
        frozen |= bad
        a = ~frozen   # the rows this step is folded into
        n = r[:, 0].copy()
        with np.errstate(invalid="ignore", over="ignore"):
            p = joint_power(tau[k], x_before, nq)
            sole_p = np.asarray(rec["sole_p"][k], dtype=float)
            zb, zs = xk[:, 2], sole_p[:, :, 2]
            if terrain is not None:   # heights above the ground
                cr = contact_rows[k]
                on = cr[:, _contact_rule.O_IN:_contact_rule.O_IN + 2] != 0.0
                az = cr[:, [_contact_rule.O_ANCHOR + 11, _contact_rule.O_ANCHOR + 23]]
                zb = zb - np.where(on[:, 0] & on[:, 1], 0.5 * (az[:, 0] + az[:, 1]), np.where(on[:, 0], az[:, 0], az[:, 1]))
                zs = zs - _contact_rule.terrain_height(terrain, sole_p[:, :, :2], ground_z)
            first = a & (n == 0)
            r[first, 12] = zb[first]
            r[first, 13:15] = zs[first]
            r[first, 15:18] = rec["com"][k][first]
            r[a, 0] = n[a] + 1.0
            r[a, 1] += dts[k]
            r[a, 2] += dts[k] * p[a]
            r[a, 3] = np.where(p[a] > r[a, 3], p[a], r[a, 3])
            cp, loaded = cop(rec["sole_R"][k], sole_p, rec["wrenches"][k], c["min_force"])
            has = a & loaded.any(axis=1)
            mg = margin(cp, support_box(sole_p, loaded, c["half_length"], c["half_width"]))
            new_min = has & ((r[:, 4] == 0) | (mg < r[:, 6]))
            r[new_min, 6] = mg[new_min]
            r[has, 4] += 1.0
            r[has & (mg < 0.0), 5] += 1.0
            r[has, 7] += mg[has]
            h = np.asarray(rec["momentum"][k], dtype=float)
            hl, ha = np.linalg.norm(h[:, :3], axis=1), np.linalg.norm(h[:, 3:], axis=1)
            r[a, 8] = np.where(hl[a] > r[a, 8], hl[a], r[a, 8])
            r[a, 9] = np.where(ha[a] > r[a, 9], ha[a], r[a, 9])
            r[a, 10] += h[a, 5] ** 2
            fell = a & (r[:, 11] < 0) & ((zb < r[:, 12] - c["fall_drop"]) |
                                          ((zs[:, 0] > r[:, 13] + c["sole_lift"]) & (zs[:, 1] > r[:, 14] + c["sole_lift"])))
            r[fell, 11] = n[fell]
            r[a, 18:21] = rec["com"][k][a]
        x_before = xk
    return unpack(r)
