"""The CPU side of the mfma_blocks.h tests: what the case generators promise, and what the float64 restatements of the algorithms
(tests/_mfma_reference.py) deliver against longdouble — the yardstick the device is held to in tests/test_gpu_mfma_blocks.py."""
import numpy as np
import pytest

from tests import _mfma_accuracy as acc
from tests import _mfma_cases as cases
from tests import _mfma_reference as ref


def test_residuals_are_evaluated_above_double_precision():
    # (where longdouble is no wider than double the metrics fall back to exact Fractions: _mfma_reference._hp)
    assert ref.LONGDOUBLE_OK == bool(np.finfo(np.longdouble).eps < 1e-18)
    one_plus = np.asarray([1.0, 2.0 ** -60], dtype=np.float64)
    assert ref._hp(one_plus).sum() != 1 or not ref.LONGDOUBLE_OK


def test_sentinel_is_a_nan_with_a_payload_and_images_start_full_of_it():
    img = cases.sentinel_images(2, 7)
    assert np.isnan(img).all() and (img.view(np.uint64) == cases.SENTINEL_BITS).all()
    assert cases.SENTINEL_BITS != np.array([np.nan]).view(np.uint64)[0]


@pytest.mark.parametrize("nb,n_real", cases.BLOCKED_SHAPES + tuple((nb, 16 * (nb - 1) + nl) for nb, nl in cases.NLAST_SHAPES))
def test_planted_cases_are_exact(nb, n_real):
    case = cases.planted_factor(nb, seed=3, n_real=n_real)
    L0 = case["L0"]
    n = 16 * nb
    assert np.array_equal(np.diag(L0), np.ones(n)) and np.array_equal(L0, np.tril(L0)) and set(np.unique(L0)) <= {-1.0, 0.0, 1.0}
    if n_real is not None:
        assert np.array_equal(case["A"][n_real:], np.eye(n)[n_real:])
    assert case["bound"] < cases.EXACT_LIMIT and case["solve_bound"] * 2.0 ** 12 < cases.EXACT_LIMIT
    assert np.count_nonzero(np.tril(L0, -1)) > 0 or nb == 1
    assert cases.planted_exact_in_fractions(case)


def test_planted_factors_are_not_trivial():
    # every block row of an 80 x 80 factor still couples to the block rows before it after thinning
    L0 = cases.planted_factor(5, seed=3)["L0"]
    for bi in range(1, 5):
        for bj in range(bi):
            assert np.count_nonzero(L0[16 * bi:16 * bi + 16, 16 * bj:16 * bj + 16]) > 0, (bi, bj)


def test_tile_product_operands_are_distinct_integers_and_exact():
    for la in cases.tile_product_launches(cases.distinct_integers):
        As, B, C0s, neg, K = la.operands
        for A in As:
            assert all(len(np.unique(np.abs(a))) == a.size for a in A)
        assert all(len(np.unique(np.abs(b))) == b.size for b in B)
        assert all(np.abs(C0).min() > 0 for C0 in C0s)
        for A, C0 in zip(As, C0s):
            assert (np.abs(C0) + np.abs(A) @ np.abs(B)).max() < cases.EXACT_LIMIT
        assert not la.may_write.all() and np.isnan(la.images[:, ~la.may_write]).any()   # (some padding is there to be watched)
    ks = {la.operands[4] for la in cases.tile_product_launches(cases.distinct_integers) if la.name.startswith("mma_tile<")}
    assert ks == set(cases.TILE_KS)


def test_metrics_see_a_wrong_entry_and_a_lost_digit():
    rng = np.random.default_rng(0)
    A = cases.spd(32, 1e3, True, rng)
    L, LI = ref.chol_blocked(A, 2)
    good, _ = ref.factor_metric(A, L)
    assert good < 40
    Lbad = L.copy()
    Lbad[20, 3] *= 1 + 2.0 ** -30
    bad, where = ref.factor_metric(A, Lbad)
    assert bad > 1e5 and where[0] == 20
    gi, _ = ref.inverse_metric(LI[1], L[16:, 16:])
    Xbad = LI[1].copy()
    Xbad[9, 2] *= 1 + 2.0 ** -30
    bi, where = ref.inverse_metric(Xbad, L[16:, 16:])
    assert gi < 40 and bi > 1e5 and where[0] == 9
    C0, Am, Bm = (rng.standard_normal(s) for s in ((16, 16), (16, 20), (20, 16)))
    assert ref.tile_metric(ref.tile_product(C0, Am, Bm, True), C0, Am, Bm, True)[0] <= 21
    assert ref.tile_metric(C0 - Am[:, :16] @ Bm[:16], C0, Am, Bm, True)[0] > 1e10   # a k-step left out


def test_float64_restatements_against_longdouble():
    """The numbers of (d): worst componentwise backward error of the float64 restatements per routine, size and condition class, in u.
    The figures themselves are kept in profiles/mfma_blocks_reference.txt; here only: none is zero (the metric sees rounding at all) and
    none is beyond 2^26 u — a restatement that lost half its digits is wrong, whatever the condition number."""
    table = acc.reference_table()
    for (routine, size, metric), per_class in sorted(table.items()):
        print("%-22s n=%-3d %-8s " % (routine, size, metric) + "  ".join("%6.2f" % v for v in per_class))
        assert np.isfinite(per_class).all() and max(per_class) <= 2.0 ** 26, (routine, size, metric, per_class)
        assert max(per_class) > 0


@pytest.mark.parametrize("ncols", [16, 12, 6, 3])
def test_pivot_margins_of_single_blocks(ncols):
    for label, a, flag, at in cases.refusal_blocks(ncols):
        if flag:
            piv = cases.pivots_longdouble(a, 15) / np.abs(np.diag(a)).max()
            assert piv.min() >= 1e-6, (label, piv.min())
        elif at is not None:
            deciding, before = cases.pivot_margin(a, at)
            assert deciding <= -1e-6 and before >= 1e-6, (label, deciding, before)
        else:
            assert not np.isfinite(np.tril(a)).all(), label
            assert np.array_equal(a[ncols:], np.eye(16)[ncols:]), label


@pytest.mark.parametrize("nb", [3, 5])
def test_pivot_margins_of_blocked_matrices(nb):
    seen = set()
    for label, a, flag, at in cases.refusal_blocked(nb):
        if flag:
            piv = cases.pivots_longdouble(a, 16 * nb - 1) / np.abs(np.diag(a)).max()
            assert piv.min() >= 1e-6, (label, piv.min())
        elif at is not None:
            deciding, before = cases.pivot_margin(a, at)
            assert deciding <= -1e-6 and before >= 1e-6, (label, deciding, before)
            seen.add(at)
        else:
            assert not np.isfinite(np.tril(a)).all(), label
    assert seen == set(range(16 * nb))
