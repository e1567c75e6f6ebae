"""Per-robot push schedules of the torque-driven simulator, in numpy: one event of the kernel for B robots.  It is the definition the device kernel
(``mpc_sim_disturbances``, include/mpc_sim_disturbances.h, csrc/sim_disturbances.h; ``NativeSolver.disturbances`` / ``read_disturbances`` /
``reset_disturbances``) is held to.

Every robot carries a table of up to ``MAX_EVENTS`` events of ``EVENT`` doubles (``FIELDS``; integers held as doubles):

  0 ``trigger``      0 empty slot; 1 absolute step; 2 left touchdown; 3 left lift-off; 4 right touchdown; 5 right lift-off (``TRIGGERS``)
  1 ``start``        trigger 1: the step of the disturbance clock at which the event begins (>= 0; the clock is 0 at arming or reset and advances by
                     one per simulator step); triggers 2 - 5: which occurrence of that transition since arming or reset (>= 1)
  2 ``delay``        steps between the trigger and the first pushed step (>= 0)
  3 ``steps``        duration in simulator steps (>= 1)
  4 ``period``       0: once.  Trigger 1: repeat every ``period`` steps (>= ``steps``).  Triggers 2 - 5: fire again at every ``period``-th further
                     occurrence
  5 ``shape``        0 rectangular; 1 half sine: step k of n carries ``sin(pi (k + 1/2) / n)`` times the force
  6 ``link``         the moving joint the force acts on, a table joint index as in ``plant_model`` (0 is the floating base; joint j of the table is
                     joint j + 1 of the ``minipin.Model``)
  7 ``force_frame``  0 world axes; 1 the link's own axes
  8 ``point_frame``  0 a fixed world point; 1 a point of the link in the link's frame, carried with it
  9 - 11 ``force``   N
  12 - 14 ``point``  m
  15 reserved        0

The rule (``step``), once per simulator step BEFORE the step's dynamics, on the state ``x`` the step starts from and the ``in_contact`` pair the
contact rule's rows hold then (what the step before left), t the clock:

  1. transitions: a robot whose ``seen`` pair is the sentinel -1 takes the pair without counting; else sole i going 0 -> 1 is a touchdown, 1 -> 0 a
     lift-off: its occurrence counter advances to n, and every event e of that trigger with ``n >= start`` and (``n == start``, or ``period > 0``
     and ``(n - start) % period == 0``) gets ``fire_step[e] = t + delay``.  Without the contact rule (``in_contact`` None) nothing is compared.
  2. event e is active with step index k of ``n = steps``: trigger 1: ``u = t - start - delay >= 0``, ``k = u`` (period 0) or ``u % period``, ``k < n``;
     triggers 2 - 5: ``fire_step[e] >= 0``, ``k = t - fire_step[e]``, ``0 <= k < n``.
  3. the active event of lowest index acts; every other active one adds 1 to ``shadowed_steps`` (one (force, point) cannot carry a sum of wrenches).
  4. frames 1 are evaluated by the forward kinematics of ``x`` (link placement R, p) and held for the step: ``f = w force`` or ``w R force``,
     ``point`` or ``R point + p``; ``applied = (f, point, link)``; ``impulse += f dt``; ``pushed_steps += 1``; ``peak_force = max(., |f|)``.
     Nothing active: ``applied = 0``, ``link = acting = -1`` and the step's dynamics skip the term.
  5. ``step = t + 1``.

The state row (``WIDTH`` doubles; ``unpack``): ``step``, ``acting``, ``occurrences`` (4: triggers 2, 3, 4, 5), ``fire_step`` (8), ``impulse`` (3),
``pushed_steps``, ``shadowed_steps``, ``peak_force``, ``applied`` (6: world force, world point), ``link``, ``seen`` (2)."""
from __future__ import annotations

import numpy as np

FIELDS = ("trigger", "start", "delay", "steps", "period", "shape", "link", "force_frame", "point_frame")
EVENT = 16                   # MPC_SIM_DISTURBANCES_EVENT
MAX_EVENTS = 8               # MPC_SIM_DISTURBANCES_MAX_EVENTS
WIDTH = 32                   # MPC_SIM_DISTURBANCES_WIDTH
PARAMS = EVENT               # (the parameter rows of this model are its events)
TRIGGERS = {"empty": 0, "step": 1, "left_touchdown": 2, "left_liftoff": 3, "right_touchdown": 4, "right_liftoff": 5}
E_TRIGGER, E_START, E_DELAY, E_STEPS, E_PERIOD, E_SHAPE, E_LINK, E_FORCE_FRAME, E_POINT_FRAME, E_FORCE, E_POINT, E_RESERVED = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15
O_STEP, O_ACTING, O_OCC, O_FIRE, O_IMPULSE, O_PUSHED, O_SHADOWED, O_PEAK, O_APPLIED, O_LINK, O_SEEN = 0, 1, 2, 6, 14, 17, 18, 19, 20, 26, 27
_NAMES = FIELDS + ("force[0]", "force[1]", "force[2]", "point[0]", "point[1]", "point[2]", "reserved")


def event(trigger=1, start=0, delay=0, steps=1, period=0, shape=0, link=0, force_frame=0, point_frame=0, force=(0.0, 0.0, 0.0), point=(0.0, 0.0, 0.0)):
    """one event -> (EVENT,); ``trigger`` a number or a name of ``TRIGGERS``"""
    e = np.zeros(EVENT)
    e[:9] = (TRIGGERS.get(trigger, trigger), start, delay, steps, period, shape, link, force_frame, point_frame)
    e[E_FORCE:E_FORCE + 3], e[E_POINT:E_POINT + 3] = force, point
    return e


def rows(events, batch):
    """The forms the Python interfaces take -> (B, n_events, EVENT) float64: ``(B, n, 16)`` tables, one ``(n, 16)`` table or one ``(16,)`` event for
    every robot, or a list with one entry per robot, each a list of events (``event(...)`` vectors or dicts of its arguments), padded with empty
    slots to the longest."""
    B = int(batch)
    if isinstance(events, (list, tuple)) and len(events) == B and all(isinstance(r, (list, tuple)) for r in events):
        n = max(1, max(len(r) for r in events))
        out = np.zeros((B, n, EVENT))
        for b, r in enumerate(events):
            for i, e in enumerate(r):
                out[b, i] = event(**e) if isinstance(e, dict) else np.asarray(e, dtype=float).reshape(EVENT)
        return out
    a = np.asarray(events, dtype=float)
    if a.shape == (EVENT,):
        a = a.reshape(1, EVENT)
    if a.ndim == 2 and a.shape[1] == EVENT:
        a = np.tile(a, (B, 1, 1))
    if a.ndim != 3 or a.shape[0] != B or a.shape[2] != EVENT:
        raise ValueError("disturbances: events of shape (%d, n, %d), (n, %d), (%d,) or one list of events per robot expected, got %s"
                         % (B, EVENT, EVENT, EVENT, a.shape))
    return np.ascontiguousarray(a)


def validate(events, nj, contact_rule=True):
    """The checks of ``mpc_sim_disturbances`` (ValueError naming robot, event and field): tables (B, n, EVENT) of a model with ``nj`` table joints;
    ``contact_rule`` False refuses contact triggers.  -> the tables as a float64 array."""
    ev = np.asarray(events, dtype=float)
    if ev.ndim != 3 or ev.shape[2] != EVENT or not 1 <= ev.shape[1] <= MAX_EVENTS:
        raise ValueError("disturbances: events of shape (B, n, %d) with 1 <= n <= %d expected, got %s" % (EVENT, MAX_EVENTS, ev.shape))
    for b in range(ev.shape[0]):
        for e in range(ev.shape[1]):
            v, who = ev[b, e], "disturbances: robot %d, event %d: " % (b, e)
            for i in range(EVENT):
                if not np.isfinite(v[i]):
                    raise ValueError(who + "%s is not finite" % _NAMES[i])
            for i in range(9):
                if v[i] != np.floor(v[i]):
                    raise ValueError(who + "%s must be an integer value, got %r" % (_NAMES[i], v[i]))
            if not 0 <= v[E_TRIGGER] <= 5:
                raise ValueError(who + "trigger must be 0 .. 5, got %r" % v[E_TRIGGER])
            if v[E_RESERVED] != 0.0:
                raise ValueError(who + "reserved must be 0")
            if v[E_TRIGGER] == 0:
                continue
            if v[E_TRIGGER] == 1 and v[E_START] < 0:
                raise ValueError(who + "start must be >= 0 (a step of the clock)")
            if v[E_TRIGGER] >= 2 and v[E_START] < 1:
                raise ValueError(who + "start must be >= 1 (an occurrence of the transition)")
            if v[E_DELAY] < 0:
                raise ValueError(who + "delay must be >= 0")
            if v[E_STEPS] < 1:
                raise ValueError(who + "steps must be >= 1")
            if v[E_PERIOD] < 0 or (v[E_TRIGGER] == 1 and 0 < v[E_PERIOD] < v[E_STEPS]):
                raise ValueError(who + "period must be 0 (once) or, on an absolute trigger, >= steps")
            for i in (E_SHAPE, E_FORCE_FRAME, E_POINT_FRAME):
                if v[i] not in (0.0, 1.0):
                    raise ValueError(who + "%s must be 0 or 1" % _NAMES[i])
            if not 0 <= v[E_LINK] <= nj - 1:
                raise ValueError(who + "link must be in [0, %d] (table joint indices)" % (nj - 1))
            if v[E_TRIGGER] >= 2 and not contact_rule:
                raise ValueError(who + "trigger %d is a contact trigger and needs the contact rule (contact_rule={} turns it on)" % v[E_TRIGGER])
    return ev


def uses_contacts(events):
    """does a table hold a contact trigger (2 - 5)?"""
    return bool(np.any(np.asarray(events, dtype=float)[..., E_TRIGGER] >= 2))


def reset(batch):
    """the state rows after arming or a reset -> (B, WIDTH)"""
    s = np.zeros((int(batch), WIDTH))
    s[:, O_ACTING] = s[:, O_LINK] = -1.0
    s[:, O_FIRE:O_FIRE + MAX_EVENTS] = -1.0
    s[:, O_SEEN:O_SEEN + 2] = -1.0
    return s


def unpack(state):
    """(B, WIDTH) rows -> dict (views of ``state``): ``step``, ``acting`` (B,), ``occurrences`` (B, 4), ``fire_step`` (B, 8), ``impulse`` (B, 3),
    ``pushed_steps``, ``shadowed_steps``, ``peak_force`` (B,), ``applied`` (B, 6) (world force, world point), ``link`` (B,), ``seen`` (B, 2)"""
    s = np.asarray(state, dtype=float)
    if s.ndim != 2 or s.shape[1] != WIDTH:
        raise ValueError("disturbances: state rows of shape (B, %d) expected, got %s" % (WIDTH, s.shape))
    return {"step": s[:, O_STEP], "acting": s[:, O_ACTING], "occurrences": s[:, O_OCC:O_FIRE], "fire_step": s[:, O_FIRE:O_IMPULSE],
            "impulse": s[:, O_IMPULSE:O_PUSHED], "pushed_steps": s[:, O_PUSHED], "shadowed_steps": s[:, O_SHADOWED], "peak_force": s[:, O_PEAK],
            "applied": s[:, O_APPLIED:O_LINK], "link": s[:, O_LINK], "seen": s[:, O_SEEN:O_SEEN + 2]}


def weight(shape, k, n):
    """the factor step ``k`` of ``n`` carries"""
    return float(np.sin(np.pi * (k + 0.5) / n)) if shape else 1.0


def step(events, state, in_contact, x, model, dt):
    """One event of the kernel for B robots (module docstring); ``state`` (B, WIDTH) is advanced in place.  events (B, n, EVENT); in_contact (B, 2) the
    pair of the contact rule's rows before the step, or None without the rule; x (B, nx) the states the step starts from and ``model`` the
    ``minipin.Model`` (both read only when the acting event has a body-fixed frame; may be None otherwise); ``dt`` the step's length.
    -> applied (B, 7): world force, world point, link (-1: nothing acts), what the step's dynamics get."""
    if not isinstance(state, np.ndarray) or state.dtype != np.float64 or state.ndim != 2 or state.shape[1] != WIDTH:
        raise ValueError("disturbances: state must be a float64 array of shape (B, %d)" % WIDTH)
    B = state.shape[0]
    ev = np.asarray(events, dtype=float)
    if ev.ndim != 3 or ev.shape[0] != B or ev.shape[2] != EVENT:
        raise ValueError("disturbances: events of shape (%d, n, %d) expected, got %s" % (B, EVENT, ev.shape))
    applied = np.zeros((B, 7))
    for b in range(B):
        r, t = state[b], state[b, O_STEP]
        if in_contact is not None:
            for i in range(2):
                now, was = (1.0 if in_contact[b][i] != 0.0 else 0.0), r[O_SEEN + i]
                r[O_SEEN + i] = now
                if was < 0.0 or now == was:
                    continue
                which = 2 * i + (0 if now > was else 1)
                n = r[O_OCC + which] + 1.0
                r[O_OCC + which] = n
                for e, v in enumerate(ev[b]):
                    if int(v[E_TRIGGER]) != which + 2 or n < v[E_START]:
                        continue
                    if n == v[E_START] or (v[E_PERIOD] > 0 and (n - v[E_START]) % v[E_PERIOD] == 0):
                        r[O_FIRE + e] = t + v[E_DELAY]
        acting, kstep = -1, 0
        for e, v in enumerate(ev[b]):
            k = -1.0
            if v[E_TRIGGER] == 1:
                u = t - v[E_START] - v[E_DELAY]
                if u >= 0:
                    k = u % v[E_PERIOD] if v[E_PERIOD] > 0 else u
            elif v[E_TRIGGER] >= 2 and r[O_FIRE + e] >= 0:
                k = t - r[O_FIRE + e]
            if k < 0 or k >= v[E_STEPS]:
                continue
            if acting < 0:
                acting, kstep = e, int(k)
            else:
                r[O_SHADOWED] += 1.0
        f, p, link = np.zeros(3), np.zeros(3), -1
        if acting >= 0:
            v = ev[b, acting]
            link = int(v[E_LINK])
            f = weight(v[E_SHAPE], kstep, v[E_STEPS]) * v[E_FORCE:E_FORCE + 3]
            p = v[E_POINT:E_POINT + 3].copy()
            if v[E_FORCE_FRAME] or v[E_POINT_FRAME]:
                from .robot import minipin as pin
                data = model.createData()
                pin.forwardKinematics(model, data, np.asarray(x, dtype=float).reshape(B, -1)[b, :model.nq])
                M = data.oMi[link + 1]
                R = np.asarray(M.rotation, dtype=float)
                if v[E_FORCE_FRAME]:
                    f = R @ f
                if v[E_POINT_FRAME]:
                    p = R @ p + np.asarray(M.translation, dtype=float)
            r[O_IMPULSE:O_IMPULSE + 3] += f * dt
            r[O_PUSHED] += 1.0
            r[O_PEAK] = max(r[O_PEAK], float(np.sqrt(f @ f)))
        r[O_APPLIED:O_APPLIED + 3], r[O_APPLIED + 3:O_APPLIED + 6] = f, p
        r[O_LINK], r[O_ACTING] = link, acting
        r[O_STEP] = t + 1.0
        applied[b, :3], applied[b, 3:6], applied[b, 6] = f, p, link
    return applied


# -- helpers that fill tables on the host (there is no device random generator) ---------------------------------------------------------------------
def from_push_schedule(fd, theta, ticks, substeps):
    """The events that reproduce ``pipeline.push_schedule`` passed as ``tick(push=...)`` on a pipeline armed at MPC tick 0: the world force
    ``[cos theta, sin theta, 0] fd`` at the world origin on the base, on every simulator step of the periods ``ticks[0] <= t < ticks[1]``
    (``substeps`` simulator steps per period).  -> (1, EVENT)"""
    f = np.array([np.cos(theta), np.sin(theta), 0.0]) * float(fd)
    return event("step", start=int(ticks[0]) * int(substeps), steps=(int(ticks[1]) - int(ticks[0])) * int(substeps), force=f).reshape(1, EVENT)


def sweep(magnitudes, thetas=(0.0,), delays=(0,), steps=10, trigger="step", start=0, link=0, point=(0.0, 0.0, 0.0), point_frame=0, shape=0):
    """One robot per (magnitude, direction, delay): a horizontal world force ``m [cos theta, sin theta, 0]`` of ``steps`` steps.
    -> (tables (B, 1, EVENT), grid (B, 3) the (magnitude, theta, delay) of each robot), B = len(magnitudes) len(thetas) len(delays)"""
    grid = np.array([(m, th, d) for m in magnitudes for th in thetas for d in delays], dtype=float)
    out = np.zeros((len(grid), 1, EVENT))
    for b, (m, th, d) in enumerate(grid):
        out[b, 0] = event(trigger, start=start, delay=int(d), steps=steps, shape=shape, link=link, point_frame=point_frame,
                          force=m * np.array([np.cos(th), np.sin(th), 0.0]), point=point)
    return out, grid


def random_pushes(rng, batch, n_events=4, window=(0, 1000), steps=(5, 50), magnitude=(50.0, 300.0), links=(0,), shape=1):
    """A train of ``n_events`` random pushes per robot, filled on the host from ``rng`` (``numpy.random.Generator``): absolute triggers at uniform
    starts in ``window``, uniform durations in ``steps`` (inclusive), horizontal world forces of uniform magnitude and direction at the origin
    of a link drawn from ``links`` (carried with it).  -> (batch, n_events, EVENT)"""
    out = np.zeros((int(batch), int(n_events), EVENT))
    for b in range(int(batch)):
        starts = np.sort(rng.integers(window[0], window[1], size=n_events))
        for i, s0 in enumerate(starts):
            m, th = rng.uniform(*magnitude), rng.uniform(0.0, 2.0 * np.pi)
            out[b, i] = event("step", start=int(s0), steps=int(rng.integers(steps[0], steps[1] + 1)), shape=shape, link=int(rng.choice(links)),
                              point_frame=1, force=m * np.array([np.cos(th), np.sin(th), 0.0]))
    return out
