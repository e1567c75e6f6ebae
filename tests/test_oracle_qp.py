"""N3 on the CPU: the QP restatement (oracle/qp.hpp) is pinned by the KKT conditions of the convex QP on problems with the
structure of QP_utils.py's inverse-dynamics QPs, by a brute-force active-set enumeration on small problems, and by QPs built from their
solution (planted) on the grid of shapes the HIP kernel's five forms are tested on."""
import itertools

import numpy as np
import pytest

from tests import _oracle, _qp_cases as cases
from mpc_benchmark_amd._qp_capi import BatchedQP


def _solve(qs, box=False, eps=1e-6, **kw):
    n, neq, nin = qs[0]["H"].shape[0], qs[0]["A"].shape[0], qs[0]["C"].shape[0]
    qp = BatchedQP(len(qs), n, neq, nin, box=box, library=_oracle.load())
    qp.settings.eps_abs = eps
    qp.settings.max_iter, qp.settings.max_iter_in = 60, 40
    for k, v in kw.items():
        setattr(qp.settings, k, v)
    st = lambda k: np.stack([q[k] for q in qs])
    args = [st(k) for k in ("H", "g", "A", "b", "C", "l", "u")]
    if box:
        args += [st("l_box"), st("u_box")]
    return qp.solve(*args)


def test_id_qp_satisfies_kkt():
    rng = np.random.default_rng(3)
    qs = [cases.id_qp(rng, contact=c) for c in ((True, True), (True, False), (False, True), (True, True))]
    x, y, z, zb, info = _solve(qs)
    for i, q in enumerate(qs):
        assert info[i].status == 0
        stat, prim, comp = cases.kkt_residuals(q, x[i], y[i], z[i])
        assert stat < 2e-6 and prim < 2e-6 and comp < 1e-3
    assert any(i.n_active > 0 for i in info)  # the cone binds somewhere: the active-set logic is exercised


def test_torque_box_binds_and_kkt_holds():
    rng = np.random.default_rng(5)
    qs = [cases.id_qp(rng, torque_limit=45.0) for _ in range(3)]
    x, y, z, zb, info = _solve(qs, box=True)
    nbind = 0
    for i, q in enumerate(qs):
        assert info[i].status == 0
        stat, prim, comp = cases.kkt_residuals(q, x[i], y[i], z[i], zb[i])
        assert stat < 2e-6 and prim < 2e-6 and comp < 1e-2
        nbind += int(np.sum(np.abs(zb[i]) > 0))
    assert nbind > 0


def test_small_qp_against_active_set_enumeration():
    """Brute force: for every subset of inequality rows treated as equalities, solve the equality-constrained QP; the
    feasible candidate with correctly signed multipliers and the lowest cost is the solution."""
    rng = np.random.default_rng(11)
    n, neq, nin = 6, 2, 4
    R = rng.normal(size=(n, n)); H = R @ R.T + 0.1 * np.eye(n); g = rng.normal(size=n)
    A = rng.normal(size=(neq, n)); b = rng.normal(size=neq)
    C = rng.normal(size=(nin, n)); l = -np.abs(rng.normal(size=nin)) * 0.3; u = np.abs(rng.normal(size=nin)) * 0.3
    q = dict(H=H, g=g, A=A, b=b, C=C, l=l, u=u)
    best = None
    for pattern in itertools.product((0, 1, 2), repeat=nin):  # 0 free, 1 at lower, 2 at upper
        rows = [i for i, p in enumerate(pattern) if p]
        E = np.vstack([A] + [C[i:i + 1] for i in rows]); e = np.concatenate([b] + [[l[i] if pattern[i] == 1 else u[i]] for i in rows])
        KKT = np.block([[H, E.T], [E, np.zeros((E.shape[0],) * 2)]])
        try:
            sol = np.linalg.solve(KKT, np.concatenate([-g, e]))
        except np.linalg.LinAlgError:
            continue
        xc, lam = sol[:n], sol[n + neq:]
        s = C @ xc
        if np.any(s > u + 1e-9) or np.any(s < l - 1e-9):
            continue
        if any((pattern[i] == 1 and lam[j] > 1e-9) or (pattern[i] == 2 and lam[j] < -1e-9) for j, i in enumerate(rows)):
            continue
        cost = 0.5 * xc @ H @ xc + g @ xc
        if best is None or cost < best[0]:
            best = (cost, xc)
    x, y, z, zb, info = _solve([q])
    assert info[0].status == 0
    assert np.allclose(x[0], best[1], atol=1e-5)


def test_reference_settings_reach_their_tolerance():
    """eps_abs = 1e-3, max_iter = 10, max_iter_in = 10 as IDSolver_ulim sets them (QP_utils.py:502-507)."""
    rng = np.random.default_rng(8)
    qs = [cases.id_qp(rng) for _ in range(4)]
    x, y, z, zb, info = _solve(qs, eps=1e-3, max_iter=10, max_iter_in=10)
    for i, q in enumerate(qs):
        assert info[i].status == 0 and info[i].iters <= 10
        stat, prim, comp = cases.kkt_residuals(q, x[i], y[i], z[i])
        assert stat < 2e-3 and prim < 2e-3


@pytest.mark.parametrize("shape", cases.PLANTED_GRID, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_planted_solution(shape):
    """The oracle on the planted-solution grid (tests/_qp_cases.py planted_qp: the reference is the point the QP was built from, not a solver),
    6 problems per shape, eps_abs = 1e-7: solved, the reported residuals are those of the returned point, the active set is the planted one sign by
    sign, stationarity / feasibility / complementarity hold, and the distance to the planted point is within TOL kappa eps_abs.  This is the home of
    TOL: the worst error / (kappa eps_abs) measured HERE is 5.74 (shape (33, 16, 9)), 13.3 on (16, 1, 1, box); the bound is 10 x that, and the same
    bound is what tests/test_gpu_qp_planted.py holds the HIP kernels to."""
    n, neq, nin, box = shape[:4]
    qs = cases.planted_problems(shape)
    regular = neq + shape[4] + shape[5] <= n - 2
    assert all(q["kappa"] <= 2e3 for q in qs) or not regular
    x, y, z, zb, info = _solve(qs, box=box, **cases.PLANTED_SETTINGS)
    for i, q in enumerate(qs):
        cases.check_planted(shape, q, x[i], y[i], z[i], zb[i] if box else None, info[i], tag="oracle problem %d" % i)
