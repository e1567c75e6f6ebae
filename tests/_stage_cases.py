"""The cases of tests/test_stage_reference.py and tests/test_gpu_stage_reference.py: problems whose stages cover every contact pattern,
the state classes (today's regime, far states, the negated base quaternion, the base near a half turn from x0), and the block-wise
comparison of a library's value dumps with the numpy reference (tests/_stage_reference.py)."""
import numpy as np

from mpc_benchmark_amd import aligator
from tests import _stage_reference as ref
from tests._metrics import rel_rows

VALUES = ("xdot", "wrench", "xnext", "f", "cost", "cval")
STATE_CLASSES = ("small", "far", "negated", "half_turn", "half_turn_negated")
FLOOR = 1e-9   # absolute floor of a block's magnitude, as in tests/_phase_parity.py

# Directional derivatives of a library against Richardson-extrapolated central differences of the numpy reference: the agreement is
# set by the finite differences, not by the library.  The step is where the two error terms meet at far states (accelerations of 1e4):
# the h^4 truncation term (x 81 from h = 1e-2 to 3e-2, measured) and the rounding of the reference / h (1e-9 at h = 1e-3, 4e-8 at 1e-4).
# Worst values measured with the oracle at the cases of tests/test_stage_reference.py and at two more sets of directions are recorded
# in profiles/stage_reference.txt; the bound is 10 x those (seed-to-seed spread of the truncation error).
FD_STEP = 1e-2
FD_MEASURED = {"AB": 4.6e-10, "CD": 9.2e-11, "grad": 5.8e-11}
FD_BOUND = {q: 10.0 * e for q, e in FD_MEASURED.items()}


# ---- stages -----------------------------------------------------------------------------------------------------------------------
def wholebody_stage(fp, pattern):
    """'double' / 'left' / 'right': the stages of fulldynamic_talos.py:100-232; 'flight': create_stage([False, False]) — no force
    cost, no cone, no foot tracked, and (the script's own else-branch, :103-106) BOTH contact models in the dynamics; 'unconstrained':
    the double-support cost and dynamics with an empty constraint stack (tests/test_gpu_edge_cases.py); 'no_contact_models': the flight
    cost stack on dynamics without any contact model (no KKT block: a = M^-1 (S u - nle))."""
    lf, rf = fp.robot.foot_placements
    cs = {"double": [True, True], "left": [True, False], "right": [False, True], "flight": [False, False],
          "unconstrained": [True, True], "no_contact_models": [False, False]}[pattern]
    st = fp.create_stage(cs, lf.copy(), rf.copy())
    if pattern == "unconstrained":
        return aligator.StageModel(st.cost, st.dynamics)
    if pattern == "no_contact_models":
        from mpc_benchmark_amd.aligator import dynamics
        ode = dynamics.MultibodyConstraintFwdDynamics(st.xspace, fp.act_matrix, [], fp.prox_settings)
        free = aligator.StageModel(st.cost, dynamics.IntegratorSemiImplEuler(ode, fp.dt))
        for f, s in zip(st.constraints.funcs, st.constraints.sets):
            free.addConstraint(f, s)
        return free
    return st


def wholebody_problem(fp, patterns, terminal_constraint=True):
    prob = aligator.TrajOptProblem(fp.x0, [wholebody_stage(fp, p) for p in patterns], fp.terminal_cost())
    if terminal_constraint:
        prob.addTerminalConstraint(fp.terminal_com_constraint(fp.robot.com0 + np.array([0.01, -0.005, 0.0])))
    return prob


def kinodynamic_problem(kp, patterns):
    lf, rf = kp.robot.foot_placements
    stages = [kp.create_stage(list(cs), lf.copy(), rf.copy(), kp.urefs[10 * i]) for i, cs in enumerate(patterns)]
    prob = aligator.TrajOptProblem(kp.x0, stages, aligator.CostStack(kp.space, kp.nu))
    prob.addTerminalConstraint(kp.terminal_com_constraint(kp.robot.com0 + np.array([0.01, -0.005, 0.0])))
    return prob


def centroidal_problem(cp, patterns):
    lf, rf = cp.robot.foot_placements
    stages = [cp.create_stage(list(cs), lf, rf, cp.urefs[10 * i]) for i, cs in enumerate(patterns)]
    return aligator.TrajOptProblem(cp.x0, stages, aligator.CostStack(cp.space, cp.nu))


# ---- states and controls ------------------------------------------------------------------------------------------------------------
def make_state(pd, rng, cls):
    if cls == "small":
        return ref.far_state(pd, rng, 0.03)
    if cls == "far":
        return ref.far_state(pd, rng, 1.0)
    if cls == "negated":
        return ref.far_state(pd, rng, 1.0, negate_quaternion=True)
    if cls == "half_turn":
        return ref.near_half_turn_state(pd, rng, 1.0)
    if cls == "half_turn_negated":
        return ref.near_half_turn_state(pd, rng, 0.03, negate_quaternion=True)
    raise KeyError(cls)


def make_control(pd, rng):
    """whole body: torques 30 randn; kinodynamic: the initial wrenches + 30 randn, joint accelerations 3 randn; centroidal: u0 + 30 randn"""
    if hasattr(pd, "u_init"):
        return pd.u_init + np.concatenate((30.0 * rng.standard_normal(12), 3.0 * rng.standard_normal(pd.nv - 6)))
    return np.asarray(pd.u0, dtype=float) + 30.0 * rng.standard_normal(pd.nu)


def trajectory(pd, classes, seed):
    """one state per entry of ``classes`` (N + 1 knots, all different) and N controls (all different)"""
    rng = np.random.default_rng(seed)
    xs = np.array([make_state(pd, rng, c) for c in classes])
    us = np.array([make_control(pd, rng) for _ in range(len(classes) - 1)])
    return xs, us


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
def value_blocks(problem, k, q):
    """the blocks a value vector is cut in, each held against its own magnitude: [v | a], [q | v], the base and joint parts of the
    gap, one wrench per slot, one block per constraint function"""
    N = len(problem.stages)
    space = problem.stages[0].xspace
    if q in ("cost",):
        return [slice(0, 1)]
    if q == "cval":
        funcs = (problem.stages[k].constraints if k < N else problem.term_constraints).funcs
        out, o = [], 0
        for f in funcs:
            out.append(slice(o, o + f.nr))
            o += f.nr
        return out
    if q == "wrench":
        return [slice(0, 6), slice(6, 12)]
    if not hasattr(space, "model"):
        return [slice(0, 3), slice(3, 6), slice(6, 9)]
    nq, nv = space.model.nq, space.model.nv
    if q == "xnext":
        return [slice(0, 3), slice(3, 7), slice(7, nq), slice(nq, nq + 6), slice(nq + 6, nq + nv)]
    return [slice(0, 3), slice(3, 6), slice(6, nv), slice(nv, nv + 3), slice(nv + 3, nv + 6), slice(nv + 6, 2 * nv)]


def blockwise(problem, k, q, a, b):
    a, b = np.asarray(a, dtype=float).ravel(), np.asarray(b, dtype=float).ravel()
    assert a.shape == b.shape, (q, k, a.shape, b.shape)
    return max([rel_rows(a[s], b[s], FLOOR) for s in value_blocks(problem, k, q) if s.stop > s.start] or [0.0])


def compare_values(native, problem, reference, b=0, knots=None, skip=()):
    """{(q, k): block-wise error of the library's dump of instance b against reference[k][q]}.  The base quaternion of xnext is
    determined up to its sign (q and -q are one placement): the dump's sign is aligned with the reference's before comparing.
    The wrench record of a kinodynamic stage is held to zero (tests/_stage_reference.py); ``skip``: quantities a problem has no
    record of (the wrench of the vector-space stages, which eval_vector.h never writes)."""
    N = len(problem.stages)
    out = {}
    for k in (range(N + 1) if knots is None else knots):
        for q in (VALUES if k < N else ("cost", "cval")):
            if q in skip:
                continue
            a = native.debug_get(q, k, b)
            r = reference[k][q]
            if q == "xnext":
                a = ref.align_quaternion(a, r)
            out[(q, k)] = blockwise(problem, k, q, a, r)
    return out


def worst_per_quantity(errs):
    w = {}
    for (q, k), e in errs.items():
        w[q] = max(w.get(q, 0.0), e)
    return w


def directional_errors(native, problem, k, xs, us, directions, b=0, step=FD_STEP):
    """worst block-wise error of [A B] d, [C D] d and grad . d of the library (knot k of the evaluation it holds) against the
    extrapolated central differences of the numpy reference"""
    st = problem.stages[k]
    n, m = st.xspace.ndx, st.nu
    nz = n + m
    slots = ref.contact_slots(problem)
    AB = native.debug_get("AB", k, b).reshape(n, nz)
    CD = native.debug_get("CD", k, b).reshape(-1, nz)
    g = native.debug_get("grad", k, b)
    worst = {"AB": 0.0, "CD": 0.0, "grad": 0.0}
    for d in directions:
        fd = ref.directional_derivatives(st, xs[k], us[k], xs[k + 1], d, slots, h=step)
        worst["AB"] = max(worst["AB"], blockwise(problem, k, "f", AB @ d, fd["AB"]))
        worst["CD"] = max(worst["CD"], blockwise(problem, k, "cval", CD @ d, fd["CD"]))
        worst["grad"] = max(worst["grad"], blockwise(problem, k, "cost", np.array([g @ d]), fd["grad"]))
    return worst


def unit_directions(nz, count, seed):
    rng = np.random.default_rng(seed)
    ds = rng.standard_normal((count, nz))
    return ds / np.linalg.norm(ds, axis=1, keepdims=True)
