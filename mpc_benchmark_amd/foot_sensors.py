"""The per-robot foot force/torque sensors and contact detector of the torque-driven simulator, in numpy: one detection event for B robots.  It is
the definition the device kernel (``mpc_sim_foot_sensors``, include/mpc_sim_foot_sensors.h, csrc/sim_foot_sensors.h; ``NativeSolver.foot_sensors`` /
``read_foot_sensors`` / ``set_foot_sensors`` / ``foot_sensors_feed``) is held to.  The model closes the last leak of ground truth between the plant and
the controllers: which feet stand.  A robot has force/torque sensors in its ankles, a threshold and a debounce counter; it learns of a touchdown late
and of a noisy swing foot wrongly.  What the model returns is the DETECTED pair; the plant, its record, its metrics and its contact rule keep the
true contacts and wrenches.

A wrench is ``w[12]``: sole 0's force 3 and moment 3, then sole 1's, in the LOCAL frame of the sole (what ``simulate_torque(..., wrenches=True)``
returns, 0 for a contact the step did not hold).

Every robot has one parameter row of ``PARAMS`` = 16 doubles (``FIELDS``):

   0 ``delay``          latency in steps, an integer value in [0, RING - 1]
   1 ``sigma_f``        force noise (N), >= 0
   2 ``sigma_m``        moment noise (N m), >= 0
   3 ``bias_f``         scale of a constant per-component force offset (N), >= 0
   4 ``bias_m``         likewise for the moments (N m), >= 0
   5 ``time_constant``  first-order low-pass on the measured wrench (s), >= 0 (0: none)
   6 ``f_on``           a free sole is a candidate while the filtered ``f_z > f_on``
   7 ``f_off``          a standing sole is a candidate for release while the filtered ``f_z <= f_off``; ``f_off <= f_on``, both finite
   8 ``on_steps``       consecutive candidate steps before the sole is detected, an integer value >= 1
   9 ``off_steps``      likewise before it is released, an integer value >= 1
  10 ``seed``           an integer value in [0, 2^32)
  11 - 15 reserved, 0

Every robot has one state row of ``WIDTH`` = 232 doubles: ``det[2]`` the detected pair (entries 0 and 1, where the rows of the contact rule hold
``in_contact``), ``above[2]``, ``below[2]`` the debounce counters, ``wf[12]`` the filtered wrench, ``wm[12]`` the latest measured wrench,
``counts[2][4]`` the confusion counts, ``ring[RING][12]`` the latest true wrenches, ``head`` (the ring slot of the newest) and ``count`` (events since
arming).  Arming (``reset``): ``det`` = the ``in_contact`` pair of the contact rule, everything else 0.

One detection event, from the wrenches ``w`` of the step, its length ``dt_step`` and the ``in_contact`` pair ``t`` of the contact rule after the step:

  1. ``w`` is pushed into the ring (``head`` advances, ``count`` + 1); ``wd``: the wrench pushed ``delay`` events ago, the oldest one held while
     fewer than ``delay + 1`` are.
  2. Random numbers are the sensor model's (``sensor_model.normals``: Philox4x32-10, key ``(seed, 0)``), on streams that model does not use, so a
     robot whose two rows share a seed still draws independent numbers.  Stream 2 at this event's ``count`` is the noise ``n0[12]``; stream 3 at
     count 0 holds the constant offsets ``n1[12]``.  ``wm_c = wd_c + bias n1_c + sigma n0_c``, each term only when its parameter is non-zero:
     ``bias_f`` / ``sigma_f`` on components 0 - 2 of a sole, ``bias_m`` / ``sigma_m`` on 3 - 5.  A free sole's sensor therefore reads its offset and
     its noise: that is what the thresholds are for.
  3. ``wf = wm`` at ``count`` == 1 or ``time_constant`` == 0, else ``wf += -expm1(-dt_step / time_constant) (wm - wf)``.
  4. For each sole i, ``z_i = wf[6 i + 2]``; both decisions are taken from the state before the event.  Free: ``above_i + 1`` if ``z_i > f_on``, else
     0; at ``above_i >= on_steps`` the sole is detected (``det_i`` = 1, both its counters 0).  Detected: ``below_i + 1`` if ``z_i <= f_off``, else 0; at
     ``below_i >= off_steps`` it is released (``det_i`` = 0, both its counters 0).  The detector never reports an empty set, as the contact rule never
     releases the last contact and the QPs need one: if both soles would be free, the one with the larger ``z`` is detected (tie: sole 0), its
     counters 0.
  5. ``counts[i][2 t_i + det_i] += 1``: index 0 and 3 agreement, 1 detected but the plant has released it, 2 the plant holds it but it is not
     detected.

The row ``EXACT`` (no latency, noise, offset or filter, both thresholds at ``F_DEFAULT`` = 10 N, one step each way) detects a sole exactly while
the true normal force of the step is above 10 N: what a dict passed to ``rows`` starts from."""
from __future__ import annotations

import numpy as np

from . import sensor_model as _sensor_model

FIELDS = ("delay", "sigma_f", "sigma_m", "bias_f", "bias_m", "time_constant", "f_on", "f_off", "on_steps", "off_steps", "seed", "reserved0",
          "reserved1", "reserved2", "reserved3", "reserved4")
NAMED = FIELDS[:11]
PARAMS = len(FIELDS)         # MPC_SIM_FOOT_SENSORS_PARAMS
RING = 16                    # MPC_SIM_FOOT_SENSORS_RING
WIDTH = 232                  # MPC_SIM_FOOT_SENSORS_WIDTH
(P_DELAY, P_SIGMA_F, P_SIGMA_M, P_BIAS_F, P_BIAS_M, P_TC, P_F_ON, P_F_OFF, P_ON_STEPS, P_OFF_STEPS, P_SEED) = range(11)
F_DEFAULT = 10.0
EXACT = (0.0,) * 6 + (F_DEFAULT, F_DEFAULT, 1.0, 1.0) + (0.0,) * 6
STREAM_NOISE, STREAM_BIAS = 2, 3
O_DET, O_ABOVE, O_BELOW, O_WF, O_WM, O_COUNTS, O_RING, O_HEAD, O_COUNT = 0, 2, 4, 6, 18, 30, 38, 230, 231
CONSUMERS = ("estimator", "qp")   # bits 0 and 1 of mpc_sim_foot_sensors_feed


def feed_mask(consumers):
    """a subset of ``CONSUMERS`` (or None) -> the bit mask of ``mpc_sim_foot_sensors_feed``"""
    names = () if consumers is None else ((consumers,) if isinstance(consumers, str) else tuple(consumers))
    bad = sorted(set(names) - set(CONSUMERS))
    if bad:
        raise ValueError("foot_sensors: unknown consumers %s (known: %s)" % (bad, ", ".join(CONSUMERS)))
    return sum(1 << CONSUMERS.index(n) for n in set(names))


def rows(params, batch):
    """The forms the Python interfaces take -> (B, PARAMS) float64: ``(B, 16)`` rows, one row of 16 (for every robot), or a dict by ``FIELDS`` name
    of scalars or (B,) arrays, missing fields as in ``EXACT``."""
    B = int(batch)
    if isinstance(params, dict):
        bad = sorted(set(params) - set(NAMED))
        if bad:
            raise ValueError("foot_sensors: unknown fields %s (known: %s)" % (bad, ", ".join(NAMED)))
        out = np.tile(np.array(EXACT), (B, 1))
        for k, val in params.items():
            a = np.asarray(val, dtype=float)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
                raise ValueError("foot_sensors: field %r is a scalar or a (B,) array with B = %d, got shape %s" % (k, B, a.shape))
            out[:, FIELDS.index(k)] = a
        return out
    p = np.asarray(params, dtype=float)
    if p.shape == (PARAMS,):
        return np.tile(p, (B, 1))
    if p.shape != (B, PARAMS):
        raise ValueError("foot_sensors: params of shape (%d, %d), (%d,) or a dict by field name expected, got %s" % (B, PARAMS, PARAMS, p.shape))
    return np.ascontiguousarray(p)


def validate(params):
    """The checks of ``mpc_sim_foot_sensors`` (ValueError): rows (B, PARAMS) by the table of the module docstring -> params as a float64 array."""
    p = np.asarray(params, dtype=float)
    if p.ndim != 2 or p.shape[1] != PARAMS:
        raise ValueError("foot_sensors: params of shape (B, %d) expected, got %s" % (PARAMS, p.shape))
    if not np.all(np.isfinite(p)):
        raise ValueError("foot_sensors: non-finite parameters")
    for b, r in enumerate(p):
        if r[P_DELAY] != np.floor(r[P_DELAY]) or not 0 <= r[P_DELAY] <= RING - 1:
            raise ValueError("foot_sensors: row %d: delay must be an integer value in [0, %d], got %r" % (b, RING - 1, r[P_DELAY]))
        for k in (P_SIGMA_F, P_SIGMA_M, P_BIAS_F, P_BIAS_M, P_TC):
            if r[k] < 0.0:
                raise ValueError("foot_sensors: row %d: %s must be >= 0, got %r" % (b, FIELDS[k], r[k]))
        if r[P_F_OFF] > r[P_F_ON]:
            raise ValueError("foot_sensors: row %d: f_off must be <= f_on, got %r > %r" % (b, r[P_F_OFF], r[P_F_ON]))
        for k in (P_ON_STEPS, P_OFF_STEPS):
            if r[k] != np.floor(r[k]) or r[k] < 1.0:
                raise ValueError("foot_sensors: row %d: %s must be an integer value >= 1, got %r" % (b, FIELDS[k], r[k]))
        if r[P_SEED] != np.floor(r[P_SEED]) or not 0 <= r[P_SEED] < 2.0 ** 32:
            raise ValueError("foot_sensors: row %d: seed must be an integer value in [0, 2^32), got %r" % (b, r[P_SEED]))
        if np.any(r[11:] != 0.0):
            raise ValueError("foot_sensors: row %d: the reserved entries must be 0" % b)
    return p


def unpack(state):
    """(B, WIDTH) rows -> dict: ``det`` (B, 2), ``above`` (B, 2), ``below`` (B, 2), ``wf`` (B, 12), ``wm`` (B, 12), ``counts`` (B, 2, 4), ``ring``
    (B, RING, 12), ``head`` (B,), ``count`` (B,) (views of ``state``)"""
    s = np.asarray(state, dtype=float)
    if s.ndim != 2 or s.shape[1] != WIDTH:
        raise ValueError("foot_sensors: state rows of shape (B, %d) expected, got %s" % (WIDTH, s.shape))
    return {"det": s[:, O_DET:O_ABOVE], "above": s[:, O_ABOVE:O_BELOW], "below": s[:, O_BELOW:O_WF], "wf": s[:, O_WF:O_WM], "wm": s[:, O_WM:O_COUNTS],
            "counts": s[:, O_COUNTS:O_RING].reshape(-1, 2, 4), "ring": s[:, O_RING:O_HEAD].reshape(-1, RING, 12), "head": s[:, O_HEAD],
            "count": s[:, O_COUNT]}


def reset(in_contact):
    """the state rows after arming on the ``in_contact`` (B, 2) pair of the contact rule's rows -> (B, WIDTH): ``det`` = the pair, the rest 0"""
    c = np.asarray(in_contact, dtype=float)
    if c.ndim != 2 or c.shape[1] != 2 or np.any((c != 0.0) & (c != 1.0)):
        raise ValueError("foot_sensors: in_contact of shape (B, 2) with entries 0 or 1 expected")
    state = np.zeros((c.shape[0], WIDTH))
    state[:, O_DET:O_ABOVE] = c
    return state


def detect(state, params, wrenches, dt_step, in_contact):
    """One detection event for B robots (module docstring) -> the detected pairs (B, 2); ``state`` (B, WIDTH) is advanced in place.  params
    (B, PARAMS); wrenches (B, 12) or (B, 2, 6) of the step; ``dt_step`` its length; in_contact (B, 2) the pair of the contact rule's rows after the
    step (the confusion counts only).  Vectorised over the robots but for the counter-based normals."""
    if not isinstance(state, np.ndarray) or state.dtype != np.float64 or state.ndim != 2 or state.shape[1] != WIDTH:
        raise ValueError("foot_sensors: state must be a float64 array of shape (B, %d)" % WIDTH)
    B = state.shape[0]
    p = validate(np.asarray(params, dtype=float).reshape(B, PARAMS))
    w = np.asarray(wrenches, dtype=float).reshape(B, 12)
    t = np.asarray(in_contact, dtype=float)
    if t.shape != (B, 2) or np.any((t != 0.0) & (t != 1.0)):
        raise ValueError("foot_sensors: in_contact of shape (%d, 2) with entries 0 or 1 expected" % B)
    dt_step = float(dt_step)
    s = unpack(state)
    rb = np.arange(B)
    # 1. the delay line
    head = (s["head"].astype(int) + 1) % RING
    count = s["count"] + 1.0
    s["ring"][rb, head] = w
    back = np.minimum(p[:, P_DELAY], count - 1.0).astype(int)
    wd = s["ring"][rb, (head - back) % RING]
    # 2. offsets and noise
    force = (np.arange(12) % 6) < 3
    bias = np.where(force[None, :], p[:, P_BIAS_F, None], p[:, P_BIAS_M, None])
    sigma = np.where(force[None, :], p[:, P_SIGMA_F, None], p[:, P_SIGMA_M, None])
    n0, n1 = np.zeros((B, 12)), np.zeros((B, 12))
    for b in range(B):
        if p[b, P_SIGMA_F] != 0.0 or p[b, P_SIGMA_M] != 0.0:
            n0[b] = _sensor_model.normals(p[b, P_SEED], count[b], STREAM_NOISE, 12)
        if p[b, P_BIAS_F] != 0.0 or p[b, P_BIAS_M] != 0.0:
            n1[b] = _sensor_model.normals(p[b, P_SEED], 0, STREAM_BIAS, 12)
    wm = wd.copy()
    wm = np.where(bias != 0.0, wm + bias * n1, wm)
    wm = np.where(sigma != 0.0, wm + sigma * n0, wm)
    # 3. the low-pass
    tc = p[:, P_TC]
    lagged = (tc != 0.0) & (count != 1.0)
    alpha = np.where(lagged, -np.expm1(-dt_step / np.where(lagged, tc, 1.0)), 0.0)
    wf0 = s["wf"].copy()
    wf = np.where(lagged[:, None], wf0 + alpha[:, None] * (wm - wf0), wm)
    # 4. the detector, both soles from the state before the event
    z = wf[:, [2, 8]]
    det0 = s["det"] != 0.0
    above = np.where(~det0, np.where(z > p[:, P_F_ON, None], s["above"] + 1.0, 0.0), s["above"])
    below = np.where(det0, np.where(z <= p[:, P_F_OFF, None], s["below"] + 1.0, 0.0), s["below"])
    caught = ~det0 & (above >= p[:, P_ON_STEPS, None])
    freed = det0 & (below >= p[:, P_OFF_STEPS, None])
    det = (det0 | caught) & ~freed
    empty = ~det[:, 0] & ~det[:, 1]
    pick = np.where(z[:, 1] > z[:, 0], 1, 0)
    kept = np.zeros((B, 2), dtype=bool)
    kept[rb[empty], pick[empty]] = True
    det = det | kept
    zeroed = caught | freed | kept
    above, below = np.where(zeroed, 0.0, above), np.where(zeroed, 0.0, below)
    # 5. the confusion counts
    idx = (2 * (t != 0.0) + det).astype(int)
    for i in range(2):
        s["counts"][rb, i, idx[:, i]] += 1.0
    s["det"][:], s["above"][:], s["below"][:] = det.astype(float), above, below
    s["wf"][:], s["wm"][:] = wf, wm
    s["head"][:], s["count"][:] = head.astype(float), count
    return det.astype(float)
