"""The HIP stage kernels against the numpy reference of the stage (tests/_stage_reference.py), far from the nominal posture.

tests/test_stage_reference.py shows that the reference and the oracle agree to <= 1e-11 at these state classes; here the VALUES of
the HIP library — xdot, wrench, xnext, f, cost, cval — are held to the reference at the 1e-9 of the phase dumps, every dump of PHASES
(derivative blocks and H included) to the oracle at the same far states, and [A B] d, [C D] d, grad . d to central differences of the
reference.  Small shapes chosen so that an indexing mistake cannot hide: batch 2, every one of the 2 x (N + 1) states and 2 x N
controls different, mixed contact patterns with a flight and a constraint-free stage, a terminal CoM constraint.  Instance 0 sits at
scale 1; instance 1 mixes today's regime (scale 0.03), negated base quaternions and the base near a half turn from x0.  One
evaluation launch per handle, no solve.  The wrench record of the kinodynamic stages is held to zero (the kernel clears it).

Worst errors per quantity are printed; profiles/stage_reference.txt has the CPU figures of the same comparison and takes the device's.

Models: reduced (nv 28) and complete (nv 38: other partial MFMA tiles, other LDS plans) for the whole-body and the kinodynamic problem,
and the centroidal problem (eval_vector.h)."""
import numpy as np
import pytest

from mpc_benchmark_amd import aligator
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem
from tests import _stage_cases as cases
from tests import _stage_reference as ref
from tests._phase_parity import compare
from tests.test_gpu_fulldynamic import PHASES

pytestmark = pytest.mark.gpu

TOL = 1e-9
# tests/test_gpu_fulldynamic.PATTERN with a flight stage and a constraint-free stage in place of two of the double-support ones
WB_PATTERN = ("double", "flight", "left", "left", "right", "right", "unconstrained", "double")
KINO_PATTERN = ((True, True), (True, False), (True, False), (False, True), (False, True), (True, True))  # tests/test_gpu_kinodynamic.PATTERN
CENT_PATTERN = ((True, True), (True, False), (False, True), (False, False), (True, True))
MIXED = ("small", "negated", "half_turn", "half_turn_negated")
FD_KNOTS = (0, 2)  # a double-support and a single-support stage of instance 0


class _Instance:
    """instance b of a batched handle, with the debug_get(name, k) of tests/_phase_parity.compare"""

    def __init__(self, native, b):
        self._native, self._b = native, b

    def debug_get(self, name, k):
        return self._native.debug_get(name, k, self._b)


def _problem(kind, complete):
    if kind == "wholebody":
        pd = FullDynamicsProblem(horizon=len(WB_PATTERN), complete_model=complete)
        return pd, cases.wholebody_problem(pd, WB_PATTERN)
    if kind == "kinodynamic":
        pd = KinodynamicProblem(horizon=len(KINO_PATTERN), complete_model=complete)
        return pd, cases.kinodynamic_problem(pd, KINO_PATTERN)
    pd = CentroidalProblem(horizon=len(CENT_PATTERN))
    return pd, cases.centroidal_problem(pd, CENT_PATTERN)


def _handle(pd, prob, lib, xs, us):
    solver = pd.make_solver(_native_library=lib)
    solver.batch = 2
    solver.linear_solver_choice = aligator.LQ_SOLVER_SERIAL  # (no sweep runs here)
    solver.setup(prob)
    solver._native.debug_evaluate(xs, us)  # the one launch
    return solver


def evaluate_both(kind, complete, hip_lib, oracle_lib, seed):
    """-> (problem, xs, us [2, ...], numpy reference per instance, HIP handle, oracle handle)"""
    pd, prob = _problem(kind, complete)
    N = len(prob.stages)
    multibody = kind != "centroidal"
    x0cls = ["far"] * (N + 1)
    x1cls = [MIXED[k % len(MIXED)] for k in range(N + 1)] if multibody else ["small"] * (N + 1)
    xa, ua = cases.trajectory(pd, x0cls, seed)
    xb, ub = cases.trajectory(pd, x1cls, seed + 1)
    xs, us = np.stack((xa, xb)), np.stack((ua, ub))
    reference = [ref.evaluate_problem(prob, xs[b], us[b]) for b in range(2)]
    return prob, xs, us, reference, _handle(pd, prob, hip_lib, xs, us), _handle(pd, prob, oracle_lib, xs, us)


def check(kind, complete, hip_lib, oracle_lib, seed):
    prob, xs, us, reference, sh, so = evaluate_both(kind, complete, hip_lib, oracle_lib, seed)
    N = len(prob.stages)
    n, nu = prob.stages[0].xspace.ndx, prob.stages[0].nu
    report = {}
    for b in range(2):
        # 1. values against the numpy reference
        worst = cases.worst_per_quantity(cases.compare_values(sh._native, prob, reference[b], b=b, skip=("wrench",) if kind == "centroidal" else ()))
        report["values[%d]" % b] = worst
        bad = {q: e for q, e in worst.items() if not e <= TOL}
        assert not bad, "instance %d: HIP values deviate from the numpy reference: %s (all: %s)" % (b, bad, worst)
        # 2. every phase dump against the oracle at the same far states
        names = [q for q in PHASES if not (kind == "centroidal" and q == "wrench")]  # (eval_vector.h keeps no wrench record)
        phases = compare(_Instance(sh._native, b), _Instance(so._native, b), names, range(N + 1), n, nu, N,
                         skip_terminal=("AB", "f", "E6", "xdot", "wrench", "xnext"))
        report["phases[%d]" % b] = phases
        bad = {q: e for q, e in phases.items() if not e <= TOL}
        assert not bad, "instance %d: HIP phase dumps deviate from the oracle: %s (all: %s)" % (b, bad, phases)
    # 3. first-order blocks against differences of the reference (whole-body stages of instance 0)
    if kind == "wholebody":
        for k in FD_KNOTS:
            ds = cases.unit_directions(n + nu, 3, seed=60 + k)
            w = cases.directional_errors(sh._native, prob, k, xs[0], us[0], ds, b=0)
            report["directional[knot %d]" % k] = w
            bad = {q: e for q, e in w.items() if not e <= cases.FD_BOUND[q]}
            assert not bad, "knot %d: first-order blocks deviate from the differences of the reference: %s (bounds %s)" % (k, bad, cases.FD_BOUND)
    for name, w in report.items():
        print("%s %s %s: %s" % (kind, "complete" if complete else "reduced", name, {q: "%.1e" % e for q, e in w.items()}))
    return report


@pytest.mark.parametrize("complete", [False, True], ids=["reduced", "complete"])
def test_wholebody_stage_against_reference(hip_lib, oracle_lib, complete):
    check("wholebody", complete, hip_lib, oracle_lib, seed=300)


@pytest.mark.parametrize("complete", [False, True], ids=["reduced", "complete"])
def test_kinodynamic_stage_against_reference(hip_lib, oracle_lib, complete):
    check("kinodynamic", complete, hip_lib, oracle_lib, seed=400)


def test_centroidal_stage_against_reference(hip_lib, oracle_lib):
    check("centroidal", False, hip_lib, oracle_lib, seed=500)
