"""The per-robot hand-over latency of the plan (include/mpc_plan_latency.h, csrc/plan_latency.h): the numpy mirror that defines the model.

A control pipeline publishes a new plan once per MPC period.  Without this model every robot follows knot 0 of the new plan from the first low-level
step of the next period: the plan arrives instantly.  With it robot b keeps running the plan it already has for its first ``L_b`` low-level steps
after a publication.  The plan it already has is knot 1 of the outgoing plan, which covers the same period as knot 0 of the new one: the HELD record
(``xs[1]``, ``us[1]``, ``K_1`` and the part of knot 1's ``xdot`` the loops read), taken by value at the publication.  After those steps the robot
follows knot 0 of the new plan as without the model.

One row of ``PARAMS`` = 4 doubles per robot: ``steps``, ``jitter`` (integer-valued, 0 .. ``MAX_STEPS``), ``seed`` (integer-valued, 0 .. 2^32 - 1) and
a reserved 0.  One state row of ``STATE`` = 8 doubles per robot (``STATE_FIELDS``), every entry integer-valued:

  ``remaining``    low-level steps the robot still runs the held record for
  ``drawn``        ``L_b`` of the last publication
  ``plans``        publications so far
  ``late_steps``   low-level steps run on a held record so far
  ``steps_total``  low-level steps so far
  ``max_drawn``    the largest ``L_b`` so far
  ``held_valid``   1 once a publication took a held record (0 after arming and after a restored checkpoint)

The events, as the kernels run them:

  publication (``publish``)   ``plans += 1`` ; ``L_b = steps + min(floor(u (jitter + 1)), jitter)`` (``draw``) with ``u`` the first uniform of the
                              Philox4x32-10 block of counter ``(plans mod 2^32, plans // 2^32, 0, 0)`` and key ``(seed, 0)``
                              (``sensor_model.philox4x32`` / ``uniforms``) ; ``remaining = drawn = L_b`` ; ``held_valid = 1``.  A robot's draws
                              depend on its row and its own count only, never on its place in the batch.
  low-level step (``step``)   the robot uses the held record when ``remaining > 0`` and ``held_valid`` ; then ``remaining -= 1`` and
                              ``late_steps += 1`` ; ``steps_total += 1`` either way.

A latency longer than a period acts as one period: the next publication replaces the held record and the countdown of every robot, whether or not
it had handed over.  ``steps = jitter = 0`` is the pipeline without the model, bit for bit."""
from __future__ import annotations

import math

import numpy as np

from . import sensor_model as _sensor_model

PARAMS = 4
FIELDS = ("steps", "jitter", "seed", "reserved")
NAMED = FIELDS[:3]
STATE = 8
STATE_FIELDS = ("remaining", "drawn", "plans", "late_steps", "steps_total", "max_drawn", "held_valid", "reserved")
MAX_STEPS = 1000
MAX_SEED = 2 ** 32 - 1
XDOT_PART = 6   # doubles of knot 1's xdot a held record keeps


def held_width(nx, ndx, nu):
    """doubles of one robot's held record: ``xs[1]`` (nx) | ``us[1]`` (nu) | ``K_1`` (nu x ndx, row-major) | the xdot part (6)"""
    return int(nx) + int(nu) + int(nu) * int(ndx) + XDOT_PART


def xdot_offset(multibody, ndx):
    """first entry of the xdot part: the base acceleration ``xdot[nv : nv + 6]`` of a multibody plan (k_pipe_feedback), ``xdot[3 : 9]`` of a centroidal
    one (the rate of the centroidal momentum, k_ikid_task_errors)"""
    return int(ndx) // 2 if multibody else 3


def rows(params, batch):
    """The forms the Python interfaces take -> (B, 4) float64, or None (off): ``None``, an int (``steps`` of every robot), a ``(B,)`` array of ints
    (``steps`` per robot), a ``(B, 4)`` table, or a dict of ``steps`` / ``jitter`` / ``seed`` (scalars or (B,) arrays, missing fields 0).  The rows are
    checked (``validate``)."""
    B = int(batch)
    if params is None:
        return None
    out = np.zeros((B, PARAMS))
    if isinstance(params, dict):
        bad = sorted(set(params) - set(NAMED))
        if bad:
            raise ValueError("latency: unknown fields %s (known: %s)" % (bad, ", ".join(NAMED)))
        for k, val in params.items():
            a = np.asarray(val, dtype=float)
            if a.shape not in ((), (B,)):
                raise ValueError("latency: field %r must be a scalar or of shape (%d,), got %s" % (k, B, a.shape))
            out[:, NAMED.index(k)] = a
    else:
        a = np.asarray(params, dtype=float)
        if a.shape == () or a.shape == (B,):
            out[:, 0] = a
        elif a.shape == (B, PARAMS):
            out[:] = a
        else:
            raise ValueError("latency: an int, (%d,) steps, (%d, %d) rows or a dict expected, got shape %s" % (B, B, PARAMS, a.shape))
    return validate(out, B)


def validate(params, batch):
    """(B, 4) rows checked as mpc_plan_latency checks them: finite, integer-valued, ``steps`` and ``jitter`` in 0 .. 1000, ``seed`` in
    0 .. 2^32 - 1, the reserved entry 0 -> the rows as float64"""
    p = np.asarray(params, dtype=float)
    if p.shape != (int(batch), PARAMS):
        raise ValueError("latency: rows of shape (%d, %d) expected, got %s" % (int(batch), PARAMS, p.shape))
    for b, row in enumerate(p):
        if not np.all(np.isfinite(row)):
            raise ValueError("latency: non-finite value in the row of robot %d" % b)
        if np.any(row != np.floor(row)):
            raise ValueError("latency: the row of robot %d holds a value that is not an integer" % b)
        for i, hi in ((0, MAX_STEPS), (1, MAX_STEPS), (2, MAX_SEED), (3, 0)):
            if not 0 <= row[i] <= hi:
                raise ValueError("latency: %s of robot %d out of range (0 .. %d)" % (FIELDS[i], b, hi))
    return np.ascontiguousarray(p)


def draw(row, plans):
    """``L_b`` of the publication that makes the robot's count ``plans`` (1 for the first) with the parameter row ``row`` -> int"""
    steps, jitter, seed = int(row[0]), int(row[1]), int(row[2])
    plans = int(plans)
    u = _sensor_model.uniforms(_sensor_model.philox4x32((plans & MAX_SEED, plans >> 32, 0, 0), (seed, 0)))[0]
    return steps + min(int(math.floor(u * float(jitter + 1))), jitter)


def initial_state(batch):
    """the state rows after arming: (B, 8) zeros"""
    return np.zeros((int(batch), STATE))


def publish(state, params):
    """a publication for every robot -> the new state rows"""
    s = np.array(state, dtype=float)
    for b in range(s.shape[0]):
        s[b, 2] += 1.0
        L = float(draw(params[b], s[b, 2]))
        s[b, 0] = s[b, 1] = L
        s[b, 5] = max(s[b, 5], L)
        s[b, 6] = 1.0
    return s


def step(state):
    """one low-level step for every robot -> (use_held (B,) bool: the record each robot's controller reads on this step, the new state rows)"""
    s = np.array(state, dtype=float)
    use = (s[:, 0] > 0.0) & (s[:, 6] != 0.0)
    s[use, 0] -= 1.0
    s[use, 3] += 1.0
    s[:, 4] += 1.0
    return use, s


def invalidate(state):
    """what a restored checkpoint does (mpc_set_state on an armed handle): ``remaining = 0``, no held record -> the new state rows"""
    s = np.array(state, dtype=float)
    s[:, 0] = 0.0
    s[:, 6] = 0.0
    return s


def unpack(state):
    """(B, 8) state rows -> dict by ``STATE_FIELDS`` name of (B,) int64 arrays (without the reserved entry)"""
    s = np.asarray(state, dtype=float)
    return {name: s[:, i].astype(np.int64) for i, name in enumerate(STATE_FIELDS[:7])}


def unpack_held(held, nx, ndx, nu):
    """(B, held_width) held records -> dict(xs (B, nx), us (B, nu), K (B, nu, ndx), xdot (B, 6))"""
    h = np.asarray(held, dtype=float)
    nx, ndx, nu = int(nx), int(ndx), int(nu)
    o = nx + nu + nu * ndx
    return dict(xs=h[:, :nx].copy(), us=h[:, nx:nx + nu].copy(), K=h[:, nx + nu:o].reshape(-1, nu, ndx).copy(), xdot=h[:, o:o + XDOT_PART].copy())


def from_solve_ms(ms, sim_dt):
    """a measured solve time in milliseconds -> the low-level steps of ``sim_dt`` seconds it covers: ``ceil(ms / (1000 sim_dt))`` (a quotient
    within 1e-12 above an integer is that integer: 0.3 ms at 0.1 ms steps is 3 steps, not 4)"""
    ms, sim_dt = float(ms), float(sim_dt)
    if not (ms >= 0.0 and math.isfinite(ms)) or not sim_dt > 0.0:
        raise ValueError("from_solve_ms: ms >= 0 and sim_dt > 0 expected")
    return int(math.ceil(ms / (1000.0 * sim_dt) - 1e-12))
