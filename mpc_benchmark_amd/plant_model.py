"""The per-robot plant inertias of the torque-driven simulator, in numpy: the model tables of B robots.  It is the definition the device kernel
(``mpc_sim_plant``, include/mpc_sim_plant.h, csrc/sim_plant.h; ``NativeSolver.plant`` / ``read_plant``) is held to.

With the model on, every robot of the simulator handle is integrated with its OWN link masses, centres of mass and rotational inertias: a payload, a
mass error, a displaced centre of mass.  The controllers keep the nominal model: the plant differs from what they believe.

One parameter row of ``PARAMS`` = 16 doubles per robot (``FIELDS``):

    0      mass_scale      every link's mass and ``I_com`` multiplied by it (> 0; 1 is nominal)
    1      inertia_scale   every link's ``I_com`` multiplied by it once more (> 0; 1 is nominal)
    2      shift_body      table joint index (0 is the base) whose centre of mass is displaced
    3-5    com_shift       added to that link's ``lever``, in the joint frame, in metres
    6      payload_body    table joint index carrying a point mass
    7      payload_mass    kg, >= 0; 0: none
    8-10   payload_point   where the point mass sits, in the joint frame
    11-15  reserved        0

and an optional ``link_scale`` (B, nj): link j's mass and ``I_com`` multiplied by its entry (> 0), the "every link off by a few percent" case.  The
table joint index is the one of the model tables (``LoweringContext.model_tables``): joint j of the table is joint j + 1 of the ``minipin.Model``.

Per link j of robot b, from the nominal (m, c, I) = (mass, lever, I_com), in this order, every step a branch on its parameter:

    mass_scale != 1:                         m *= mass_scale, I *= mass_scale
    inertia_scale != 1:                      I *= inertia_scale
    link_scale given and link_scale[j] != 1: m *= link_scale[j], I *= link_scale[j]
    j == shift_body and com_shift != 0:      c += com_shift
    j == payload_body and payload_mass > 0:  the point mass m_p at r is composed by the parallel-axis rule (``minipin.Inertia.__add__``):
        m' = m + m_p,  c' = (m c + m_p r) / m',  I' = I + m (|d|^2 1 - d d^T) + m_p (|e|^2 1 - e e^T),  d = c - c',  e = r - c'

A robot on the ``IDENTITY`` row, without ``link_scale`` or with ones, keeps the nominal entries bit for bit.  Joint placements, frames, contact
placements and gains, gravity and ``prox_mu`` are never touched."""
from __future__ import annotations

import numpy as np

from .robot import minipin as pin

FIELDS = ("mass_scale", "inertia_scale", "shift_body", "com_shift_x", "com_shift_y", "com_shift_z", "payload_body", "payload_mass",
          "payload_x", "payload_y", "payload_z")
PARAMS = 16                  # MPC_SIM_PLANT_PARAMS
IDENTITY = (1.0, 1.0) + (0.0,) * 14
P_MASS, P_INERTIA, P_SHIFT_BODY, P_SHIFT, P_PAYLOAD_BODY, P_PAYLOAD_MASS, P_PAYLOAD_POINT = 0, 1, 2, 3, 6, 7, 8
# the model tables (include/mpc_abi.h): 4 header doubles, then 25 per joint: R[9] p[3] mass lever[3] I_com[9]
HEADER_DOUBLES, JOINT_DOUBLES, INERTIA_OFFSET, INERTIA_DOUBLES = 4, 25, 12, 13


def rows(params, batch):
    """The forms the Python interfaces take -> (B, PARAMS) float64: ``(B, 16)`` rows, one row of 16 (for every robot), or a dict by ``FIELDS`` name
    of scalars or (B,) arrays, missing fields at their identity value."""
    B = int(batch)
    if isinstance(params, dict):
        bad = sorted(set(params) - set(FIELDS))
        if bad:
            raise ValueError("plant: unknown fields %s (known: %s)" % (bad, ", ".join(FIELDS)))
        out = np.tile(np.array(IDENTITY), (B, 1))
        for k, val in params.items():
            a = np.asarray(val, dtype=float)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
                raise ValueError("plant: field %r is a scalar or a (B,) array with B = %d, got shape %s" % (k, B, a.shape))
            out[:, FIELDS.index(k)] = a
        return out
    p = np.asarray(params, dtype=float)
    if p.shape == (PARAMS,):
        return np.tile(p, (B, 1))
    if p.shape != (B, PARAMS):
        raise ValueError("plant: params of shape (%d, %d), (%d,) or a dict by field name expected, got %s" % (B, PARAMS, PARAMS, p.shape))
    return np.ascontiguousarray(p)


def validate(params, nj, link_scale=None):
    """The checks of ``mpc_sim_plant`` (ValueError): rows (B, PARAMS) by the table of the module docstring for a model of ``nj`` table joints;
    ``link_scale`` None or (B, nj), finite and > 0.  -> (params, link_scale) as float64 arrays (None stays None)."""
    p = np.asarray(params, dtype=float)
    nj = int(nj)
    if p.ndim != 2 or p.shape[1] != PARAMS:
        raise ValueError("plant: params of shape (B, %d) expected, got %s" % (PARAMS, p.shape))
    if not np.all(np.isfinite(p)):
        raise ValueError("plant: non-finite parameters")
    for b, r in enumerate(p):
        for k in (P_MASS, P_INERTIA):
            if not r[k] > 0.0:
                raise ValueError("plant: row %d: %s must be > 0, got %r" % (b, FIELDS[k], r[k]))
        if r[P_PAYLOAD_MASS] < 0.0:
            raise ValueError("plant: row %d: payload_mass must be >= 0, got %r" % (b, r[P_PAYLOAD_MASS]))
        for k in (P_SHIFT_BODY, P_PAYLOAD_BODY):
            if r[k] != np.floor(r[k]) or not 0 <= r[k] <= nj - 1:
                raise ValueError("plant: row %d: %s must be an integer value in [0, %d], got %r" % (b, FIELDS[k], nj - 1, r[k]))
        if np.any(r[11:] != 0.0):
            raise ValueError("plant: row %d: the reserved entries must be 0" % b)
    ls = None
    if link_scale is not None:
        ls = np.asarray(link_scale, dtype=float)
        if ls.shape != (p.shape[0], nj):
            raise ValueError("plant: link_scale of shape (%d, %d) expected, got %s" % (p.shape[0], nj, ls.shape))
        if not np.all(np.isfinite(ls)) or np.any(ls <= 0.0):
            raise ValueError("plant: link_scale must be finite and > 0")
        ls = np.ascontiguousarray(ls)
    return np.ascontiguousarray(p), ls


def perturb(mass, lever, inertia, row, j, scale=None):
    """The rule of the module docstring for link ``j`` (table joint index): nominal (mass, lever (3,), I_com (3, 3)), one parameter row, this
    link's ``link_scale`` entry or None -> (mass, lever, I_com) of the plant"""
    m, c, I = float(mass), np.array(lever, dtype=float).reshape(3), np.array(inertia, dtype=float).reshape(3, 3)
    if row[P_MASS] != 1.0:
        m, I = m * row[P_MASS], I * row[P_MASS]
    if row[P_INERTIA] != 1.0:
        I = I * row[P_INERTIA]
    if scale is not None and scale != 1.0:
        m, I = m * scale, I * scale
    shift = np.asarray(row[P_SHIFT:P_SHIFT + 3], dtype=float)
    if j == int(row[P_SHIFT_BODY]) and np.any(shift != 0.0):
        c = c + shift
    mp = float(row[P_PAYLOAD_MASS])
    if j == int(row[P_PAYLOAD_BODY]) and mp > 0.0:
        r = np.asarray(row[P_PAYLOAD_POINT:P_PAYLOAD_POINT + 3], dtype=float)
        mt = m + mp
        ct = (m * c + mp * r) / mt
        d, e = c - ct, r - ct
        I = I + m * (d @ d * np.eye(3) - np.outer(d, d)) + mp * (e @ e * np.eye(3) - np.outer(e, e))
        m, c = mt, ct
    return m, c, I


def tables(dtab, itab, params, link_scale=None):
    """The model tables of B robots: the nominal double table ``dtab`` (``LoweringContext.model_tables``) with every joint's 13 inertia doubles
    rewritten by the rule, everything else copied -> (B, nd) float64"""
    dtab = np.asarray(dtab, dtype=float).reshape(-1)
    nj = int(np.asarray(itab).reshape(-1)[0])
    p, ls = validate(params, nj, link_scale)
    out = np.tile(dtab, (p.shape[0], 1))
    for b, row in enumerate(p):
        for j in range(nj):
            o = HEADER_DOUBLES + JOINT_DOUBLES * j + INERTIA_OFFSET
            m, c, I = perturb(dtab[o], dtab[o + 1:o + 4], dtab[o + 4:o + 13], row, j, None if ls is None else ls[b, j])
            out[b, o], out[b, o + 1:o + 4], out[b, o + 4:o + 13] = m, c, I.reshape(9)
    return out


def models(model, params, link_scale=None):
    """One perturbed ``minipin.Model`` per robot (copies of ``model``; only ``inertias`` differ): what the plant of robot b is, for reference dynamics
    and for inspection (``pin.computeTotalMass``, ``pin.centerOfMass``)."""
    nj = model.njoints - 1
    p, ls = validate(params, nj, link_scale)
    out = []
    for b, row in enumerate(p):
        mb = model.copy()
        for j in range(nj):
            Y = model.inertias[j + 1]
            mb.inertias[j + 1] = pin.Inertia(*perturb(Y.mass, Y.lever, Y.inertia, row, j, None if ls is None else ls[b, j]))
        out.append(mb)
    return out
