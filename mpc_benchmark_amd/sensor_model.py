"""The per-robot sensor model of the torque-driven simulator, in numpy: one measurement event for B robots.  It is the definition the device kernel
(``mpc_sim_sensors``, include/mpc_sim_sensors.h, csrc/sim_sensors.h; ``NativeSolver.sensors`` / ``read_sensors`` / ``set_sensors``) is held to.  The
model sits between "the simulator produced the true state" and "the controllers read it": latency, encoder resolution, calibration offsets, noise on
the joints and on the floating base, joint velocities obtained by differencing positions, a low-pass on them.  What it returns is the MEASUREMENT:
what the feedback laws, the low-level QPs, the task errors, the next solve's initial condition and the walk generators see.  The plant, its record,
its metrics and its contact rule keep the true state.

State layout: ``x = [q (nq = nv + 1: base position 3, base quaternion xyzw 4, joints nu) ; v (nv: base linear 3, base angular 3, joints nu)]``,
nu = nv - 6, nx = nq + nv.

Every robot has one parameter row of ``PARAMS`` = 16 doubles (``FIELDS``):

   0 ``delay``            latency in steps, an integer value in [0, RING - 1]
   1 ``sigma_q``          joint position noise (rad), >= 0
   2 ``sigma_v``          joint velocity noise (rad / s), >= 0
   3 ``sigma_base_p``     base position noise (m), >= 0
   4 ``sigma_base_r``     base orientation noise (rad: a rotation vector in the base frame), >= 0
   5 ``sigma_base_v``     base linear velocity noise, >= 0
   6 ``sigma_base_w``     base angular velocity noise, >= 0
   7 ``quantum``          encoder resolution (rad), >= 0 (0: none)
   8 ``q_bias``           scale of a constant per-joint calibration offset (rad), >= 0
   9 ``v_from_q``         0 or 1: joint velocities by finite differences of the measured joint positions
  10 ``v_time_constant``  first-order low-pass on the joint velocities (s), >= 0 (0: none)
  11 ``seed``             an integer value in [0, 2^32)
  12 - 15 reserved, 0

Every robot has one state row of ``width(nv)`` = 17 nx + 2 nu + 2 doubles: ``ring[RING][nx]`` the latest true states, ``meas[nx]`` the latest
measurement, ``vf[nu]`` the low-pass state, ``qm_prev[nu]`` the joint positions of the measurement before, ``head`` (the ring slot of the newest
state) and ``count`` (events since the reset).  Arming is one event on the initial state: ``count`` is 1 after it and a measurement is always held.

One measurement event, from the true state ``x`` and the length ``dt_step`` of the step that produced it:

  1. ``x`` is pushed into the ring (``head`` advances, ``count`` + 1); ``xd``: the state pushed ``delay`` events ago, the oldest one held while
     fewer than ``delay + 1`` are (the line is primed with the first state).
  2. Random numbers are counter based: Philox4x32-10 (``philox4x32``), key ``(seed, 0)``, counter ``(count mod 2^32, count // 2^32, block, stream)``
     with the ``count`` of this event (1 at arming).  The four words of a block give two uniforms in (0, 1), exact in fp64,
     ``u1 = ((w1 << 20 | w0 >> 12) + 0.5) 2^-52`` and ``u2`` likewise from ``w3, w2``, and those two normals, ``z0 = sqrt(-2 log u1) cos(2 pi u2)``
     and ``z1 = sqrt(-2 log u1) sin(2 pi u2)``; normal k of a stream is ``z_(k mod 2)`` of block ``k // 2`` (``normals``).  Stream 0 is the noise of
     this event, n0, indexed in tangent order: 0 .. nv - 1 the configuration tangent, nv .. 2 nv - 1 the velocity.  Stream 1 with counter words 0
     and 1 set to 0 holds the calibration offsets, n1: index k = joint k.  So a robot's stream depends on its row and its own event count, not
     on its place in the batch, the batch size or the launch shape.
  3. joint positions: ``a_j = xd.q_j + q_bias n1_j + sigma_q n0_(6 + j)``, each term only when its parameter is non-zero;
     ``qm_j = rint(a_j / quantum) quantum`` when ``quantum`` > 0, else ``a_j``.
  4. base position: ``xd.p + sigma_base_p n0_(0..2)``.
  5. base orientation: ``quat(xd) (x) exp(delta)``, ``delta = sigma_base_r n0_(3..5)``, ``exp(delta) = (sin(|delta| / 2) delta / |delta|,
     cos(|delta| / 2))`` (below |delta| = 1e-8 the two-term series ``(delta (1/2 - |delta|^2 / 48), 1 - |delta|^2 / 8)``), a Hamilton product,
     normalised afterwards; skipped entirely when ``sigma_base_r`` == 0.
  6. base velocity: linear and angular plus ``sigma_base_v n0_(nv..nv+2)`` and ``sigma_base_w n0_(nv+3..nv+5)``.
  7. joint velocities: ``w_j = (qm_j - qm_prev_j) / dt_step`` when ``v_from_q`` and ``count`` > 1, else ``xd.v_j``; plus ``sigma_v n0_(nv+6+j)``;
     low-pass: ``vf = w`` at ``count`` == 1 or ``v_time_constant`` == 0, else ``vf += -expm1(-dt_step / v_time_constant) (w - vf)``; the measured
     joint velocity is ``vf``.
  8. ``meas``, ``qm_prev = qm``, ``head`` and ``count`` are stored.

The identity row ``IDENTITY`` (sixteen zeros) takes none of the arithmetic branches: the measurement is the state bit for bit."""
from __future__ import annotations

import numpy as np

FIELDS = ("delay", "sigma_q", "sigma_v", "sigma_base_p", "sigma_base_r", "sigma_base_v", "sigma_base_w", "quantum", "q_bias", "v_from_q",
          "v_time_constant", "seed", "reserved0", "reserved1", "reserved2", "reserved3")
NAMED = FIELDS[:12]
PARAMS = len(FIELDS)         # MPC_SIM_SENSORS_PARAMS
RING = 16                    # MPC_SIM_SENSORS_RING
IDENTITY = (0.0,) * PARAMS
(P_DELAY, P_SIGMA_Q, P_SIGMA_V, P_SIGMA_BASE_P, P_SIGMA_BASE_R, P_SIGMA_BASE_V, P_SIGMA_BASE_W, P_QUANTUM, P_Q_BIAS, P_V_FROM_Q, P_V_TC,
 P_SEED) = range(12)

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF
TWO_PI = 6.283185307179586


def philox4x32(counter, key):
    """Philox4x32-10: counter (4 words), key (2 words) -> the block's 4 words (Python ints)"""
    c0, c1, c2, c3 = (int(c) & _MASK for c in counter)
    k0, k1 = (int(k) & _MASK for k in key)
    for r in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def uniforms(words):
    """the 4 words of a block -> (u1, u2), both strictly inside (0, 1) and exact in fp64"""
    w0, w1, w2, w3 = (int(w) for w in words)
    return (float((w1 << 20) | (w0 >> 12)) + 0.5) * 2.0 ** -52, (float((w3 << 20) | (w2 >> 12)) + 0.5) * 2.0 ** -52


def normals(seed, count, stream, n):
    """the first ``n`` normals of stream ``stream`` of the robot with ``seed`` at event ``count`` -> (n,)"""
    count = int(count)
    out = np.zeros(2 * ((int(n) + 1) // 2))
    for blk in range(out.size // 2):
        u1, u2 = uniforms(philox4x32((count & _MASK, count >> 32, blk, int(stream)), (int(seed), 0)))
        r, a = np.sqrt(-2.0 * np.log(u1)), TWO_PI * u2
        out[2 * blk], out[2 * blk + 1] = r * np.cos(a), r * np.sin(a)
    return out[:int(n)]


def width(nv):
    """doubles of one robot's state row"""
    nv = int(nv)
    return (RING + 1) * (2 * nv + 1) + 2 * (nv - 6) + 2


def rows(params, batch):
    """The forms the Python interfaces take -> (B, PARAMS) float64: ``(B, 16)`` rows, one row of 16 (for every robot), or a dict by ``FIELDS`` name
    of scalars or (B,) arrays, missing fields 0 (the identity)."""
    B = int(batch)
    if isinstance(params, dict):
        bad = sorted(set(params) - set(NAMED))
        if bad:
            raise ValueError("sensors: unknown fields %s (known: %s)" % (bad, ", ".join(NAMED)))
        out = np.tile(np.array(IDENTITY), (B, 1))
        for k, val in params.items():
            a = np.asarray(val, dtype=float)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
                raise ValueError("sensors: field %r is a scalar or a (B,) array with B = %d, got shape %s" % (k, B, a.shape))
            out[:, FIELDS.index(k)] = a
        return out
    p = np.asarray(params, dtype=float)
    if p.shape == (PARAMS,):
        return np.tile(p, (B, 1))
    if p.shape != (B, PARAMS):
        raise ValueError("sensors: params of shape (%d, %d), (%d,) or a dict by field name expected, got %s" % (B, PARAMS, PARAMS, p.shape))
    return np.ascontiguousarray(p)


def validate(params):
    """The checks of ``mpc_sim_sensors`` (ValueError): rows (B, PARAMS) by the table of the module docstring -> params as a float64 array."""
    p = np.asarray(params, dtype=float)
    if p.ndim != 2 or p.shape[1] != PARAMS:
        raise ValueError("sensors: params of shape (B, %d) expected, got %s" % (PARAMS, p.shape))
    if not np.all(np.isfinite(p)):
        raise ValueError("sensors: non-finite parameters")
    for b, r in enumerate(p):
        if r[P_DELAY] != np.floor(r[P_DELAY]) or not 0 <= r[P_DELAY] <= RING - 1:
            raise ValueError("sensors: row %d: delay must be an integer value in [0, %d], got %r" % (b, RING - 1, r[P_DELAY]))
        for k in (P_SIGMA_Q, P_SIGMA_V, P_SIGMA_BASE_P, P_SIGMA_BASE_R, P_SIGMA_BASE_V, P_SIGMA_BASE_W, P_QUANTUM, P_Q_BIAS, P_V_TC):
            if r[k] < 0.0:
                raise ValueError("sensors: row %d: %s must be >= 0, got %r" % (b, FIELDS[k], r[k]))
        if r[P_V_FROM_Q] not in (0.0, 1.0):
            raise ValueError("sensors: row %d: v_from_q must be 0 or 1, got %r" % (b, r[P_V_FROM_Q]))
        if r[P_SEED] != np.floor(r[P_SEED]) or not 0 <= r[P_SEED] < 2.0 ** 32:
            raise ValueError("sensors: row %d: seed must be an integer value in [0, 2^32), got %r" % (b, r[P_SEED]))
        if np.any(r[12:] != 0.0):
            raise ValueError("sensors: row %d: the reserved entries must be 0" % b)
    return p


def unpack(state, nv):
    """(B, width(nv)) rows -> dict: ``ring`` (B, RING, nx), ``meas`` (B, nx), ``vf`` (B, nu), ``qm_prev`` (B, nu), ``head`` (B,), ``count`` (B,)
    (views of ``state``)"""
    nv = int(nv)
    nx, nu = 2 * nv + 1, nv - 6
    s = np.asarray(state, dtype=float)
    if s.ndim != 2 or s.shape[1] != width(nv):
        raise ValueError("sensors: state rows of shape (B, %d) expected, got %s" % (width(nv), s.shape))
    o = RING * nx
    return {"ring": s[:, :o].reshape(-1, RING, nx), "meas": s[:, o:o + nx], "vf": s[:, o + nx:o + nx + nu],
            "qm_prev": s[:, o + nx + nu:o + nx + 2 * nu], "head": s[:, o + nx + 2 * nu], "count": s[:, o + nx + 2 * nu + 1]}


def _exp_quat(d):
    """exp of a rotation vector -> unit quaternion xyzw"""
    a2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    a = np.sqrt(a2)
    if a < 1e-8:
        return np.array([*(d * (0.5 - a2 / 48.0)), 1.0 - a2 / 8.0])
    return np.array([*(d * (np.sin(0.5 * a) / a)), np.cos(0.5 * a)])


def _quat_mul(a, b):
    """Hamilton product of quaternions xyzw"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def measure(state, params, x, dt_step, nv):
    """One measurement event for B robots (module docstring) -> the measurements (B, nx); ``state`` (B, width(nv)) is advanced in place.
    params (B, PARAMS); x (B, nx) the true states; ``dt_step`` the length of the step that produced them."""
    nv = int(nv)
    nq, nu, nx = nv + 1, nv - 6, 2 * nv + 1
    x = np.asarray(x, dtype=float)
    if x.ndim != 2 or x.shape[1] != nx:
        raise ValueError("sensors: states of shape (B, %d) expected, got %s" % (nx, x.shape))
    B = x.shape[0]
    p = validate(np.asarray(params, dtype=float).reshape(B, PARAMS))
    if not isinstance(state, np.ndarray) or state.dtype != np.float64 or state.shape != (B, width(nv)):
        raise ValueError("sensors: state must be a float64 array of shape (%d, %d)" % (B, width(nv)))
    dt_step = float(dt_step)
    s = unpack(state, nv)
    out = np.zeros((B, nx))
    for b in range(B):
        delay, sq, sv, sbp, sbr, sbv, sbw, quantum, q_bias, v_from_q, tc, seed = p[b, :12]
        head = (int(s["head"][b]) + 1) % RING
        count = s["count"][b] + 1.0
        s["ring"][b, head] = x[b]
        back = int(min(delay, count - 1.0))
        xd = s["ring"][b, (head - back) % RING]
        m = xd.copy()
        noisy = sq != 0.0 or sv != 0.0 or sbp != 0.0 or sbr != 0.0 or sbv != 0.0 or sbw != 0.0
        n0 = normals(seed, count, 0, 2 * nv) if noisy else None
        # joint positions
        a = xd[7:nq].copy()
        if q_bias != 0.0:
            a = a + q_bias * normals(seed, 0, 1, nu)
        if sq != 0.0:
            a = a + sq * n0[6:nv]
        qm = np.rint(a / quantum) * quantum if quantum > 0.0 else a
        m[7:nq] = qm
        # the base
        if sbp != 0.0:
            m[0:3] = xd[0:3] + sbp * n0[0:3]
        if sbr != 0.0:
            q = _quat_mul(xd[3:7], _exp_quat(sbr * n0[3:6]))
            m[3:7] = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
        if sbv != 0.0:
            m[nq:nq + 3] = xd[nq:nq + 3] + sbv * n0[nv:nv + 3]
        if sbw != 0.0:
            m[nq + 3:nq + 6] = xd[nq + 3:nq + 6] + sbw * n0[nv + 3:nv + 6]
        # joint velocities
        w = (qm - s["qm_prev"][b]) / dt_step if (v_from_q != 0.0 and count > 1.0) else xd[nq + 6:].copy()
        if sv != 0.0:
            w = w + sv * n0[nv + 6:]
        if tc == 0.0 or count == 1.0:
            vf = w
        else:
            vf = s["vf"][b] + -np.expm1(-dt_step / tc) * (w - s["vf"][b])
        m[nq + 6:] = vf
        s["meas"][b], s["vf"][b], s["qm_prev"][b] = m, vf, qm
        s["head"][b], s["count"][b] = float(head), count
        out[b] = m
    return out


def reset(params, x0):
    """the state rows after ``mpc_sim_sensors(params, x0)``: zero rows, then one event on ``x0`` (B, nx) -> (B, width(nv)); ``count`` is 1"""
    x0 = np.asarray(x0, dtype=float)
    if x0.ndim != 2 or x0.shape[1] % 2 != 1 or x0.shape[1] < 15:
        raise ValueError("sensors: initial states of shape (B, nx = 2 nv + 1) expected, got %s" % (x0.shape,))
    nv = (x0.shape[1] - 1) // 2
    state = np.zeros((x0.shape[0], width(nv)))
    measure(state, rows(params, x0.shape[0]), x0, 0.0, nv)
    return state
