"""What decides whether a step is TAKEN — the primal-dual merit, its slope along the step, the candidates alpha_i = 2^-i, the Armijo
choice and the accepted iterate — of the CPU oracle against the numpy statement of tests/_linesearch_reference.py, one pass at a time
(tests/_linesearch_cases.py says how a pass is isolated and what is held to which tolerance).

This file is how the numpy statement earns trust and where the case set is pinned: the oracle agrees with it to 1e-13 on every value
(profiles/linesearch_reference.txt), the conditions on the case set are asserted on the reference's own numbers, and the slope floors
the HIP forms are held to (tests/test_gpu_linesearch_reference.py) are the oracle's deviations measured here.

Not shown here, nor by the GPU file: the stall branch (MPC_STALL_TOL: no step when |dphi0| is at the round-off floor), the BCL updates
of k_decide / run_instance, passes after a multiplier refresh (al_iters > 0: nonzero estimates v_e, lambda_e enter the reference's
formulas but no case reaches them), and the inner criterion ``crit``."""
import numpy as np
import pytest

from tests import _linesearch_cases as lc

_results = {}


def _checked(name, form, oracle_lib):
    key = (name, form)
    if key not in _results:
        _results[key] = lc.check_case(name, oracle_lib, form, oracle_lib, lc.ORACLE_FORMS)
    return _results[key]


@pytest.mark.parametrize("form", list(lc.ORACLE_FORMS))
@pytest.mark.parametrize("name", list(lc.CASES))
def test_pass_against_reference(oracle_lib, name, form):
    report, _ = _checked(name, form, oracle_lib)
    worst = {}
    for r in report.values():
        for q, e in r.items():
            worst[q] = max(worst.get(q, 0.0), e)
    print("%s %s worst: %s" % (name, form, {q: "%.1e" % e for q, e in worst.items()}))


def test_case_set_conditions(oracle_lib):
    """On the reference's own numbers: among the whole-body passes an instance accepts alpha = 1 and one stops at candidate >= 2, and on
    every pass used no candidate up to the accepted one lies within 1e-6 |phi0| of its Armijo bound (round-off cannot flip a decision)."""
    full = deep = False
    for name in lc.CASES:
        _, choices = _checked(name, "serial", oracle_lib)
        for (j, b), c in choices.items():
            assert c["clearance"] > lc.ARMIJO_CLEARANCE, "%s pass %d instance %d: a candidate lies %.1e |phi0| from its Armijo bound" % (name, j, b, c["clearance"])
            if lc.CASES[name][0] == "wholebody":
                full, deep = full or c["alpha"] == 1.0, deep or c["ls_step"] >= 2
        print(name, {k: (c["alpha"], c["ls_step"], "%.1e" % c["clearance"]) for k, c in choices.items()})
    assert full and deep


def test_checkpointed_pass_is_the_pass_of_a_straight_run(oracle_lib):
    """the isolation of tests/_linesearch_cases.py: j - 1 iterations, checkpoint, one iteration == j iterations, bit for bit"""
    name, j = "wholebody-reduced", 3
    pd, prob, xs, us = lc.build(name, oracle_lib)
    st = lc.canonical(name, oracle_lib)[j]
    one = lc.make_handle(pd, prob, oracle_lib, "serial")
    one._native.set_state(st["state"])
    one._native.run(st["xs"], st["us"])
    straight = lc.make_handle(pd, prob, oracle_lib, "serial")
    lc.set_options(straight, max_iters=j)
    straight._native.set_x0(xs[:, 0])
    stats = straight._native.run(xs, us)
    assert all(s.num_iters == j and s.al_iters == 0 for s in stats)
    a, b = one._native.get_results(gains=False, multipliers=True), straight._native.get_results(gains=False, multipliers=True)
    for q in ("xs", "us", "vs", "lams"):
        assert np.array_equal(a[q], b[q]), q
    for k in range(len(prob.stages) + 1):
        for q in ("ls_knot", "dmerit"):
            assert np.array_equal(one._native.debug_get(q, k, 1), straight._native.debug_get(q, k, 1), equal_nan=True), (q, k)


@pytest.mark.parametrize("form", list(lc.ORACLE_FORMS))
def test_tick_against_reference(oracle_lib, form):
    lc.check_ticks(oracle_lib, form, lc.ORACLE_FORMS)


def test_reference_projections_and_choice():
    """the pieces of the numpy statement that no library run pins on their own: the three projections, and the end of the backtracking"""
    from tests import _linesearch_reference as lsr
    rows = (np.array([lsr.EQUALITY, lsr.NEG_ORTHANT, lsr.NEG_ORTHANT, lsr.BOX, lsr.BOX, lsr.BOX]), np.array([0, 0, 0, -1.0, -1.0, -1.0]), np.array([0, 0, 0, 2.0, 2.0, 2.0]))
    p, act = lsr.project(rows, np.array([-3.0, -3.0, 3.0, -1.5, 0.5, 2.5]))
    assert np.array_equal(p, [-3.0, 0.0, 3.0, -0.5, 0.0, 0.5]) and list(act) == [True, False, True, True, False, True]
    phis = [5.0, 3.0, 0.5, 0.1]
    assert lsr.armijo_choice(1.0, -1.0, lambda i: phis[i], 1e-4, 8, 1e-7)[:2] == (2, 0.25)
    assert lsr.armijo_choice(1.0, -1.0, lambda i: 9.0, 1e-4, 3, 1e-7)[:2] == (2, 0.25)   # out of candidates: the one in hand
    assert lsr.armijo_choice(1.0, -1.0, lambda i: 9.0, 1e-4, 8, 0.2)[:2] == (2, 0.25)    # the next alpha would fall below alpha_min
