"""The LDS plan of the batched QP kernel (mpc_benchmark_amd/csrc/qp_layout.h: which of the five forms of k_qp_solve a shape runs, and where P, Y, S,
ZD, the vectors and the staged H, A, C lie in the 160 KB of a workgroup) checked on the host, as tests/test_ric_layout.py does for the Riccati sweep:
the header is plain C++, compiled here with g++ into a dump of every plan of the planted-solution grid (tests/_qp_cases.py PLANTED_GRID), at batch 6 and
300, with the matrix cores allowed and not.  The GPU test reads the same table, so a retuned plan cannot silently take a kernel out of the grid."""
import pytest

from tests import _qp_cases as cases, _qp_layout as lay


@pytest.fixture(scope="module")
def table():
    return lay.layout_table(cases.PLANTED_GRID)


def test_regions_do_not_overlap_and_fit_the_lds(table):
    assert len(table) == 4 * len(set(s[:4] for s in cases.PLANTED_GRID))
    for key, p in table.items():
        regs = sorted((v for v in p["regions"].values() if v[1] > 0), key=lambda v: v[0])
        for a, b in zip(regs, regs[1:]):
            assert a[0] + a[1] <= b[0], "%s: regions overlap: %s" % (key, p["regions"])
        assert regs[0][0] == 0 and 8 * (regs[-1][0] + regs[-1][1]) <= p["total_bytes"], key
        assert all(start % 2 == 0 for start, _ in p["regions"].values()), key   # 16-byte alignment of every carve-out
        # everything the GPU test creates fits (64 bytes are kept for the kernel's static LDS)
        assert p["total_bytes"] + 64 <= lay.LDS_LIMIT, (key, p["total_bytes"])
        # the form only follows what the shape allows
        n, neq = p["n"], p["neq"]
        assert p["mf"] == 0 or (p["allow_mf"] and n >= 16 and neq > 0), key
        assert p["mats"] == 0 or p["batch"] <= 256, key
        assert (p["mats"], p["mf"]) in lay.FORMS, key


def test_vec_region_holds_what_the_kernel_carves_from_it(table):
    """k_qp_solve (csrc/qp_kernel.h, the pointer chain behind `double *x = v`): x, xk, grad, r1, dx, w, hx, hd, tmpn (9 n) ; y, ye, yplus, Ax, Ad, tmpe
    (6 neq) ; z, zp, s, ds (4 m) ; red (16) ; hx0, hdx (2 n) doubles, then actl (nin ints) = 11 n + 6 neq + 4 m + 16 doubles + nin ints.  The plan reserves
    11 n + 6 neq + 4 m + nin + 64 doubles; the next region (or the end of the plan) must not begin before the carve-out ends."""
    for key, p in table.items():
        n, neq, nin, m = p["n"], p["neq"], p["nin"], p["nin"] + (p["n"] if p["box"] else 0)
        start, length = p["regions"]["vec"]
        need_bytes = 8 * (11 * n + 6 * neq + 4 * m + 16) + 4 * nin
        assert 8 * length >= need_bytes, key
        later = [v[0] for v in p["regions"].values() if v[1] > 0 and v[0] > start]
        end = min(later) if later else p["total_bytes"] // 8
        assert 8 * (end - start) >= need_bytes, key
        assert end - start >= 11 * n + 6 * neq + 4 * m + nin + 64, key   # (what make_qp_lds takes)


def test_the_grid_reaches_all_five_kernels_boxed_and_unboxed(table):
    reached = {}
    for shape in cases.PLANTED_GRID:
        for batch, no_mfma, form in lay.creations(table, shape):
            reached.setdefault(form, set()).add(bool(shape[3]))
    assert set(reached) == set(lay.FORMS), reached
    for form in lay.FORMS:
        assert reached[form] == {False, True}, (form, reached[form])


def test_shapes_the_library_refuses_do_not_fit_in_any_form():
    t = lay.layout_table(cases.PLANTED_TOO_LARGE)
    for p in t.values():
        assert p["total_bytes"] > lay.LDS_LIMIT, p   # mpc_qp_create: "QP too large for the LDS of one workgroup"


def test_reference_problem_sizes_keep_their_kernels(table):
    """The 28-dof inverse-dynamics QP (n = 62, neq = 40, nin = 18) runs on the matrix cores with everything in LDS while every QP has a CU to itself,
    the complete model's (n = 82, neq = 50) on the matrix cores from global memory; H alone leaves the LDS at n = 66, neq = 44."""
    form = lambda s, batch, no: (table[s + (batch, no)]["mats"], table[s + (batch, no)]["mf"])
    for box in (False, True):
        assert form((62, 40, 18, box), 6, False) == (1, 1) and form((62, 40, 18, box), 300, False) == (0, 1)
        assert form((62, 40, 18, box), 6, True) == (1, 0) and form((62, 40, 18, box), 300, True) == (0, 0)
        assert form((82, 50, 18, box), 6, False) == (0, 1)
        assert form((66, 44, 18, box), 6, False) == (2, 1)
