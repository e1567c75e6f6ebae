"""Every form of the batched QP kernel (csrc/qp_kernel.h k_qp_solve<MATS, MF>: matrix-core or column-by-column linear algebra; H, A, C in LDS, A and C
only, or all from global memory) against PLANTED solutions: QPs built from their solution (tests/_qp_cases.py planted_qp), so that the reference is exact
and owes nothing to any solver — neither to the oracle, which is the same algorithm on the same path.  The shapes sit where the kernel has its edges
(n < 16, n and neq multiples of 16, neq + 1 = 16, neq = 0, nin = 0 with and without a box, n = 128 on the column-by-column form, n odd at the LDS limit),
with active lower AND upper bounds of C x, active lower and upper box bounds and two-sided rows.

Which kernel a creation launches is read from the LDS plan itself (tests/_qp_layout.py: csrc/qp_layout.h compiled on the host; tests/test_qp_layout.py
proves there that the grid reaches all five forms).  A shape is created up to four ways — batch 6 or 300 (more than 256 QPs: nothing is staged in LDS),
with or without MPC_QP_NO_MFMA (read by mpc_qp_create) — and creations that give a form the shape already ran are dropped.

TOL: the distance to the planted point is bounded by TOL kappa eps_abs, kappa = || K^-1 ||_inf of the planted active set's KKT matrix.  TOL is measured on the
CPU oracle, never on these kernels (tests/test_oracle_qp.py::test_planted_solution, the same grid and seeds): worst error / (kappa eps_abs) = 5.74, TOL = 10 x
that = 57.4; the shape (16, 1, 1, box) has its own measured 13.3, bound 133 ("What the stop rule of the QP bounds").  The complementarity bound
is 10 x the oracle's worst (1.43e-5).  profiles/qp_planted.txt has the figures of every shape and form, oracle beside GPU.

Run the whole file: the last test requires that every parameter of test_planted_solution ran, so that a deselected parameter cannot hide a kernel."""
import numpy as np
import pytest

from tests import _qp_cases as cases, _qp_layout as lay
from mpc_benchmark_amd import _capi
from mpc_benchmark_amd._qp_capi import BatchedQP

pytestmark = pytest.mark.gpu

TABLE = lay.layout_table(cases.PLANTED_GRID)
_name = lambda s: "-".join(str(int(v)) for v in s)
# (shape, batch, no_mfma, (mats, mf)) of every creation that reaches a form the shape has not run yet
PARAMS = [(shape, batch, no_mfma, form) for shape in cases.PLANTED_GRID for batch, no_mfma, form in lay.creations(TABLE, shape)]
_pid = lambda p: "%s-b%d%s" % (_name(p[0]), p[1], "-valu" if p[2] else "")
COPIES = 50  # batch 300 = the 6 problems 50 times

_solutions = {}  # (shape, batch, no_mfma) -> (x, y, z, zb, info) of the 6 problems, from test_planted_solution
_ran = {}        # ... -> (mats, mf) it ran


def _lib():
    return _capi.load_hip_library()


def _create(shape, batch, no_mfma, monkeypatch):
    """A handle of `batch` QPs of this shape with the planted settings; MPC_QP_NO_MFMA is read by mpc_qp_create (getenv)."""
    if no_mfma:
        monkeypatch.setenv("MPC_QP_NO_MFMA", "1")
    else:
        monkeypatch.delenv("MPC_QP_NO_MFMA", raising=False)
    n, neq, nin, box = shape[:4]
    qp = BatchedQP(batch, n, neq, nin, box=box, library=_lib())
    for k, v in cases.PLANTED_SETTINGS.items():
        setattr(qp.settings, k, v)
    return qp


def _args(qs, box, copies=1):
    st = lambda k: np.concatenate([np.stack([q[k] for q in qs])] * copies)
    return [st(k) for k in ("H", "g", "A", "b", "C", "l", "u")] + ([st("l_box"), st("u_box")] if box else [])


def _info_tuple(i):
    return (i.prim_res, i.dual_res, i.mu_eq, i.mu_in, i.iters, i.iters_in, i.status, i.n_active)


def _solve(shape, batch, no_mfma, monkeypatch):
    """-> (x, y, z, zb, info) of the shape's 6 problems; at batch 300 the 50 copies of each must be bitwise equal (instances never interact)."""
    key = (tuple(shape), batch, no_mfma)
    if key not in _solutions:
        qs = cases.planted_problems(shape)
        P = len(qs)
        assert batch % P == 0
        x, y, z, zb, info = _create(shape, batch, no_mfma, monkeypatch).solve(*_args(qs, shape[3], batch // P))
        for a in (x, y, z, zb):
            blocks = a.reshape(batch // P, P, -1)
            assert all(np.array_equal(blocks[0].view(np.uint64), b.view(np.uint64)) for b in blocks[1:]), "copies of one problem differ: workgroups interact"
        assert all(_info_tuple(info[i]) == _info_tuple(info[i % P]) for i in range(batch))
        _solutions[key] = (x[:P], y[:P], z[:P], zb[:P], info[:P])
    return _solutions[key]


@pytest.mark.parametrize("param", PARAMS, ids=_pid)
def test_planted_solution(param, monkeypatch):
    """Per problem: status 0; prim_res, dual_res <= eps_abs and equal to the residuals of the returned point; the active set is the planted one, sign by sign,
    and n_active its size; stationarity, feasibility AND complementarity; distance to the planted point <= TOL kappa eps_abs (module docstring)."""
    shape, batch, no_mfma, form = param
    plan = TABLE[tuple(shape[:4]) + (batch, no_mfma)]
    assert (plan["mats"], plan["mf"]) == form and plan["total_bytes"] + 64 <= lay.LDS_LIMIT
    qs = cases.planted_problems(shape)
    x, y, z, zb, info = _solve(shape, batch, no_mfma, monkeypatch)
    box = shape[3]
    figs = [cases.check_planted(shape, q, x[i], y[i], z[i], zb[i] if box else None, info[i], tag="mats=%d mf=%d batch=%d problem %d" % (form + (batch, i)))
            for i, q in enumerate(qs)]
    print("planted %-24s mats=%d mf=%d batch=%-3d ratio %.3g err %.2e kappa %.2e comp %.2e outer %d newton %d" % (
        _name(shape), form[0], form[1], batch, max(f["ratio"] for f in figs), max(f["err"] for f in figs), max(q["kappa"] for q in qs),
        max(f["comp"] for f in figs), max(f["iters"] for f in figs), max(f["iters_in"] for f in figs)))
    _ran[(tuple(shape), batch, no_mfma)] = form


@pytest.mark.parametrize("shape", cases.PLANTED_GRID, ids=_name)
def test_variants_agree(shape, monkeypatch):
    """Between the creations of one shape: the same status, n_active and active set.  The spread of x is printed, not asserted: the forms sum in different
    orders and a Newton pass may end one step apart; each is already held to the planted point."""
    sols = [(form, _solve(shape, batch, no_mfma, monkeypatch)) for batch, no_mfma, form in lay.creations(TABLE, shape)]
    f0, (x0, y0, z0, zb0, i0) = sols[0]
    spread = 0.0
    for form, (x, y, z, zb, info) in sols[1:]:
        for i in range(len(i0)):
            assert info[i].status == i0[i].status and info[i].n_active == i0[i].n_active, (shape, f0, form, i)
            assert np.array_equal(np.sign(z[i]), np.sign(z0[i])) and np.array_equal(np.sign(zb[i]), np.sign(zb0[i])), (shape, f0, form, i)
    for a in range(len(sols)):
        for b in range(a + 1, len(sols)):
            spread = max(spread, float(np.max(np.abs(sols[a][1][0] - sols[b][1][0]))))
    print("spread %-24s forms %s max |x_a - x_b| %.2e" % (_name(shape), " ".join("%d%s" % (f[0], "T" if f[1] else "F") for f, _ in sols), spread))


# one matrix-core and one column-by-column shape for the paths a cold solve from zero never takes
MF_SHAPE, VALU_SHAPE = (62, 40, 18, True, 5, 6), (15, 4, 6, True, 3, 3)


@pytest.mark.parametrize("shape", [MF_SHAPE, VALU_SHAPE], ids=_name)
def test_warm_start_on_the_device(shape, monkeypatch):
    """warm_start = 1 starts from the handle's previous (x, y, z): on the same data no more than one Newton step and still the planted point; after a small
    change of g the warm and the cold solve find the same active set and the warm one takes no more Newton steps."""
    assert (TABLE[shape[:4] + (6, False)]["mf"] == 1) == (shape == MF_SHAPE)
    box = shape[3]
    qs = cases.planted_problems(shape)
    args = _args(qs, box)
    qp = _create(shape, len(qs), False, monkeypatch)
    cold = qp.solve(*args)
    qp.settings.warm_start = 1
    x, y, z, zb, info = qp.solve(*args)
    for i, q in enumerate(qs):
        assert cold[4][i].iters_in > 1 and info[i].iters_in <= 1, (shape, i, cold[4][i].iters_in, info[i].iters_in)
        cases.check_planted(shape, q, x[i], y[i], z[i], zb[i] if box else None, info[i], tag="warm problem %d" % i)
    args[1] = args[1] + 1e-3 * np.random.default_rng(5).normal(size=args[1].shape)
    xw, yw, zw, zbw, iw = qp.solve(*args)          # warm: from the solution of the unperturbed problems
    qp.settings.warm_start = 0
    xc, yc, zc, zbc, ic = qp.solve(*args)
    for i in range(len(qs)):
        assert iw[i].status == 0 and ic[i].status == 0
        assert np.array_equal(np.sign(zw[i]), np.sign(zc[i])) and np.array_equal(np.sign(zbw[i]), np.sign(zbc[i])) and iw[i].n_active == ic[i].n_active
        assert iw[i].iters_in <= ic[i].iters_in, (shape, i, iw[i].iters_in, ic[i].iters_in)
    print("warm %-24s Newton steps warm %s cold %s" % (_name(shape), [i.iters_in for i in iw], [i.iters_in for i in ic]))


@pytest.mark.parametrize("shape", [MF_SHAPE, VALU_SHAPE], ids=_name)
def test_iteration_limit_and_failed_factorisation_are_reported(shape, monkeypatch):
    """status 1 and 2 are ordinary return codes.  max_iter = max_iter_in = 1: status 1, one outer iteration, finite outputs.  One problem of six with
    H = -I (the primal block is not positive definite): status 2 for it — the kernel's `goto done` between its barriers — and the other five
    solved to the planted point."""
    box = shape[3]
    qs = cases.planted_problems(shape)
    qp = _create(shape, len(qs), False, monkeypatch)
    qp.settings.max_iter, qp.settings.max_iter_in = 1, 1
    x, y, z, zb, info = qp.solve(*_args(qs, box))
    for i in range(len(qs)):
        assert info[i].status == 1 and info[i].iters == 1 and info[i].iters_in == 1, (shape, i, _info_tuple(info[i]))
        assert all(np.all(np.isfinite(a[i])) for a in (x, y, z, zb)) and np.isfinite(info[i].prim_res) and np.isfinite(info[i].dual_res)
    qp = _create(shape, len(qs), False, monkeypatch)
    args = _args(qs, box)
    bad = 2
    args[0][bad] = -np.eye(shape[0])
    x, y, z, zb, info = qp.solve(*args)
    for i, q in enumerate(qs):
        if i == bad:
            assert info[i].status == 2, (shape, _info_tuple(info[i]))
        else:
            cases.check_planted(shape, q, x[i], y[i], z[i], zb[i] if box else None, info[i], tag="beside a failed factorisation, problem %d" % i)


@pytest.mark.parametrize("dims", cases.PLANTED_TOO_LARGE, ids=_name)
def test_shapes_beyond_the_lds_are_refused(dims, monkeypatch):
    monkeypatch.delenv("MPC_QP_NO_MFMA", raising=False)
    with pytest.raises(RuntimeError, match="mpc_qp_create failed"):
        BatchedQP(6, dims[0], dims[1], dims[2], box=dims[3], library=_lib())


def test_all_five_kernels_ran():
    """Over the parameters of test_planted_solution that ran and passed: every one of them, and with them all five forms of k_qp_solve, each on a boxed and
    on an unboxed shape."""
    assert len(_ran) == len(PARAMS), "parameters of test_planted_solution that did not run or did not pass: %s" % sorted(
        _pid(p) for p in PARAMS if (tuple(p[0]), p[1], p[2]) not in _ran)
    for form in lay.FORMS:
        boxes = {bool(k[0][3]) for k, f in _ran.items() if f == form}
        assert boxes == {False, True}, (form, boxes)
