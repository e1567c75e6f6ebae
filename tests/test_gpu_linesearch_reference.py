"""What decides whether a step is TAKEN, on the device: the primal-dual merit per knot (k_eval_multibody / k_eval_vector, knot_merit),
its slope (k_duals: MISC_DMERIT per knot, in the [A B] dz + E dx' form that k_forward_prefetch leaves behind and in the substituted form
mu_d (lambda' - lambda_e) - f of the legs and of k_forward_phi), the candidates alpha_i = 2^-i written by the values-only instantiations
k_eval_multibody<1> / k_eval_vector<1> (the manifold step x (+) alpha dx, the trial multipliers, the projections at the trial point),
the Armijo choice of k_linesearch, the iterate k_accept leaves and the reductions of k_decide (stats.merit, traj_cost, prim_infeas,
dual_infeas) — against the numpy statement of tests/_linesearch_reference.py, one pass at a time.  tests/_linesearch_cases.py holds the
cases, the isolation of a pass, the tolerances and the check ; tests/test_linesearch_reference.py runs the same check on the CPU oracle,
pins the case set and measures the slope floors the handle forms here are held to.

Handle forms, each on every case it applies to: the serial sweep with the default forward sweep, with forward_mode = 1, four legs, and
(reduced whole-body case) the generic kernels.  One MPC tick on the shim route, where k_eval_multibody<3> writes candidate 0.

Worst errors per quantity are printed ; profiles/linesearch_reference.txt has the figures of the CPU and of the device.

Not shown here: the stall branch (MPC_STALL_TOL), the BCL updates of k_decide, passes after a multiplier refresh (al_iters > 0), the
inner criterion ``crit`` ; candidates > 0 of a pass whose full step was accepted are never evaluated and so never read."""
import pytest

from tests import _linesearch_cases as lc

pytestmark = pytest.mark.gpu

PAIRS = [(name, form) for name in lc.CASES for form in lc.applicable_forms(name, lc.HIP_FORMS)]


@pytest.mark.parametrize("name,form", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_pass_against_reference(hip_lib, oracle_lib, name, form):
    report, _ = lc.check_case(name, hip_lib, form, oracle_lib, lc.HIP_FORMS)
    worst = {}
    for r in report.values():
        for q, e in r.items():
            worst[q] = max(worst.get(q, 0.0), e)
    print("%s %s worst: %s" % (name, form, {q: "%.1e" % e for q, e in worst.items()}))


@pytest.mark.parametrize("form", ["serial", "legs4"])
def test_tick_against_reference(hip_lib, form):
    lc.check_ticks(hip_lib, form, lc.HIP_FORMS)
