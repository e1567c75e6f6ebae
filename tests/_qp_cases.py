"""QPs with the structure of the reference's whole-body inverse-dynamics problems (QP_utils.py:437-575): variables
(da, df, tau), dynamics + contact-acceleration equalities, wrench-cone inequalities, optional torque box — and QPs built FROM their
solution (planted_qp), whose reference owes nothing to any solver."""
import numpy as np

CMIN = lambda mu, L, W: np.array([[-1, 0, mu, 0, 0, 0], [1, 0, mu, 0, 0, 0], [-1, 0, mu, 0, 0, 0], [1, 0, mu, 0, 0, 0], [0, 0, 1, 0, 0, 0],
                                  [0, 0, W, -1, 0, 0], [0, 0, W, 1, 0, 0], [0, 0, L, 0, -1, 0], [0, 0, L, 0, 1, 0]], dtype=float)


def id_qp(rng, nv=28, nk=2, weights=(1.0, 1e-3), mu=0.8, L=0.1, W=0.075, torque_limit=None, contact=(True, True)):
    """-> dict(H, g, A, b, C, l, u[, l_box, u_box]) of one IDSolver_ulim-like problem with random (physically scaled) data."""
    fs = 6
    n, neq, nin = 2 * nv - 6 + fs * nk, nv + fs * nk, 9 * nk
    R = rng.normal(size=(nv, nv))
    M = R @ R.T / nv + np.diag(rng.uniform(0.5, 30.0, nv))   # mass-matrix like: SPD, mixed scales
    Jc = np.zeros((fs * nk, nv))
    for i in range(nk):
        if contact[i]:
            Jc[fs * i:fs * (i + 1)] = rng.normal(size=(fs, nv)) * 0.5
    a = rng.normal(size=nv) * 0.5
    forces = np.zeros(fs * nk)
    for i in range(nk):
        if contact[i]:
            forces[fs * i:fs * (i + 1)] = np.array([rng.normal() * 20, rng.normal() * 20, 450 + rng.normal() * 50, rng.normal() * 5, rng.normal() * 5, rng.normal()])
    nle = rng.normal(size=nv) * 30
    gamma = rng.normal(size=fs * nk) * 0.3
    for i in range(nk):
        if not contact[i]:
            gamma[fs * i:fs * (i + 1)] = 0.0  # a foot in the air contributes empty rows (0 = 0), as in QP_utils.py:520-530
    S = np.zeros((nv, nv - 6)); S[6:] = np.eye(nv - 6)
    A = np.zeros((neq, n)); b = np.zeros(neq)
    A[:nv, :nv] = M; A[:nv, nv:nv + fs * nk] = -Jc.T; A[:nv, nv + fs * nk:] = -S; A[nv:, :nv] = Jc
    b[:nv] = -nle - M @ a + Jc.T @ forces
    b[nv:] = -gamma - Jc @ a
    C = np.zeros((nin, n)); l = np.zeros(nin)
    cm = CMIN(mu, L, W)
    for i in range(nk):
        if contact[i]:
            f = forces[fs * i:fs * (i + 1)]
            l[9 * i:9 * (i + 1)] = -cm @ f          # C (f + df) >= 0  <=>  C df >= -C f
            C[9 * i:9 * (i + 1), nv + fs * i:nv + fs * (i + 1)] = cm
    H = np.zeros((n, n)); H[:nv, :nv] = np.eye(nv) * weights[0]; H[nv:nv + fs * nk, nv:nv + fs * nk] = np.eye(fs * nk) * weights[1]
    out = dict(H=H, g=np.zeros(n), A=A, b=b, C=C, l=l, u=np.full(nin, 1e5))
    if torque_limit is not None:
        lb = np.full(n, -1e5); ub = np.full(n, 1e5)
        lb[nv + fs * nk:] = -torque_limit; ub[nv + fs * nk:] = torque_limit
        out["l_box"], out["u_box"] = lb, ub
    return out


def kkt_residuals(q, x, y, z, zb=None):
    """Optimality of a convex QP, independent of how it was solved: stationarity, primal feasibility, sign and
    complementarity of the inequality multipliers (z > 0 on an upper bound, < 0 on a lower bound).  (Empty blocks, neq = 0 or nin = 0, count as 0.)"""
    H, g, A, b, C, l, u = (q[k] for k in ("H", "g", "A", "b", "C", "l", "u"))
    mx = lambda a: float(np.max(a, initial=0.0))
    stat = H @ x + g + A.T @ y + C.T @ z + (zb if zb is not None else 0.0)
    s = C @ x
    prim = max(mx(np.abs(A @ x - b)), mx(np.maximum(s - u, 0)), mx(np.maximum(l - s, 0)))
    comp = max(mx(np.abs(np.maximum(z, 0) * (u - s))), mx(np.abs(np.minimum(z, 0) * (s - l))))
    if zb is not None:
        prim = max(prim, mx(np.maximum(x - q["u_box"], 0)), mx(np.maximum(q["l_box"] - x, 0)))
        comp = max(comp, mx(np.abs(np.maximum(zb, 0) * (q["u_box"] - x))), mx(np.abs(np.minimum(zb, 0) * (x - q["l_box"]))))
    return mx(np.abs(stat)), float(prim), float(comp)


# ---- planted-solution QPs -----------------------------------------------------------------------------------------------------------
# (n, neq, nin, box, n_act_in, n_act_box): the shapes at which the five forms of the HIP kernel (csrc/qp_layout.h) meet their edges.
# Every shape fits the 160 KB of a workgroup in every form it is created in (tests/test_qp_layout.py).
PLANTED_GRID = (
    (62, 40, 18, False, 6, 0), (62, 40, 18, True, 5, 6),      # the inverse-dynamics QP of the 28-dof model
    (82, 50, 18, True, 6, 8), (82, 50, 18, False, 6, 0),      # ... of the complete model: matrix cores, matrices from global memory
    (66, 44, 18, False, 6, 0), (66, 44, 18, True, 5, 6),      # H no longer fits beside the tiles: A and C only in LDS
    (17, 5, 7, True, 3, 3),                                   # one real row in the second 16-block
    (33, 16, 9, False, 4, 0),                                 # neq = 16: row neq of the Gram matrix opens a tile of its own
    (48, 32, 16, True, 5, 5),                                 # all multiples of 16: no identity padding at all
    (47, 15, 31, True, 10, 8),                                # neq + 1 = 16, nin > neq
    (15, 4, 6, True, 3, 3),                                   # n < 16: column-by-column form
    (24, 0, 10, True, 5, 5),                                  # neq = 0: column-by-column form, empty Schur complement
    (40, 12, 0, False, 0, 0), (40, 12, 0, True, 0, 9),        # nin = 0, without and with a box
    (128, 0, 12, True, 5, 10),                                # n = 128 on the column-by-column form: h_times with its second column per lane
    (128, 8, 12, False, 5, 0), (128, 8, 12, True, 4, 12),
    (123, 20, 12, True, 5, 10), (125, 20, 12, False, 5, 0),   # n odd, the largest plans
    (1, 0, 1, False, 1, 0), (6, 6, 3, False, 0, 0), (16, 1, 1, True, 1, 2),  # degenerate: n = 1, neq = n, one row of each kind
)
PLANTED_PROBLEMS = 6
PLANTED_SETTINGS = dict(eps_abs=1e-7, max_iter=60, max_iter_in=40)
# shapes that do not fit the LDS of a workgroup in any form: mpc_qp_create refuses them
PLANTED_TOO_LARGE = ((128, 40, 30, True), (100, 80, 20, False), (128, 100, 18, False), (96, 64, 48, True))


def planted_rng(n, neq):
    return np.random.default_rng(1000 + 7 * n + neq)


def planted_qp(rng, n, neq, nin, box, n_act_in, n_act_box):
    """One QP built from its solution: -> dict(H, g, A, b, C, l, u[, l_box, u_box], x, y, z, z_box, kappa).

    H = R R^T / n + diag(U(0.5, 2)) (SPD: x* unique); A, C, x*, y* standard normal; s* = C x*.  Every inequality row has a slack of U(0.5, 2)
    on both sides, about 40 % of the rows are one-sided (u = 1e5, as the project's cones); n_act_in rows are active, alternately at the lower bound
    (l = s*, z* = -U(0.5, 2)) and at the upper bound (u = s*, z* = +U(0.5, 2)): the sign convention of include/mpc_qp_abi.h.  Box: about half of the
    coordinates with finite bounds at distance U(0.5, 2), the rest +-1e5; n_act_box coordinates active, alternately lower and upper.  Then
    g = -(H x* + A^T y* + C^T z* + z_box*), b = A x*.  Strict complementarity holds by construction (active multipliers and inactive slacks >= 0.5);
    with neq + n_act_in + n_act_box <= n - 2 (the regular shapes) the active rows are independent, so (y*, z*, z_box*) are unique too.
    kappa = || K^-1 ||_inf of the KKT matrix of the planted active set, K = [[H, E^T], [E, 0]], E = [A ; C_active ; I_active]: what turns a KKT
    residual into a distance to the planted point.  Regular shapes must have kappa <= 2e3."""
    assert 0 <= n_act_in <= nin and 0 <= n_act_box <= (n if box else 0)
    R = rng.normal(size=(n, n))
    H = R @ R.T / n + np.diag(rng.uniform(0.5, 2.0, n))
    A = rng.normal(size=(neq, n)); C = rng.normal(size=(nin, n))
    xs = rng.normal(size=n); ys = rng.normal(size=neq)
    s = C @ xs
    l = s - rng.uniform(0.5, 2.0, nin); u = s + rng.uniform(0.5, 2.0, nin)
    u[rng.random(nin) < 0.4] = 1e5
    zs = np.zeros(nin)
    act_in = rng.permutation(nin)[:n_act_in]
    for k, r in enumerate(act_in):
        mag = rng.uniform(0.5, 2.0)
        if k % 2 == 0:
            l[r], zs[r] = s[r], -mag
        else:
            u[r], zs[r] = s[r], mag
    q = dict(H=H, A=A, C=C, l=l, u=u)
    zb = np.zeros(n)
    act_box = np.zeros(0, dtype=int)
    if box:
        finite = rng.random(n) < 0.5
        lb = np.where(finite, xs - rng.uniform(0.5, 2.0, n), -1e5); ub = np.where(finite, xs + rng.uniform(0.5, 2.0, n), 1e5)
        act_box = rng.permutation(n)[:n_act_box]
        for k, j in enumerate(act_box):
            mag = rng.uniform(0.5, 2.0)
            if k % 2 == 0:
                lb[j], zb[j] = xs[j], -mag
            else:
                ub[j], zb[j] = xs[j], mag
        q["l_box"], q["u_box"] = lb, ub
    q["g"] = -(H @ xs + A.T @ ys + C.T @ zs + zb)
    q["b"] = A @ xs
    E = np.vstack([A, C[np.sort(act_in)], np.eye(n)[np.sort(act_box)]])
    K = np.block([[H, E.T], [E, np.zeros((E.shape[0],) * 2)]])
    kappa = float(np.max(np.sum(np.abs(np.linalg.inv(K)), axis=1)))
    if neq + n_act_in + n_act_box <= n - 2:
        assert kappa <= 2e3, (n, neq, nin, box, kappa)
    q.update(x=xs, y=ys, z=zs, z_box=zb, kappa=kappa)
    return q


def planted_problems(shape):
    """The PLANTED_PROBLEMS problems of one shape of the grid, as every planted test draws them."""
    rng = planted_rng(shape[0], shape[1])
    return [planted_qp(rng, *shape) for _ in range(PLANTED_PROBLEMS)]


def qp_residuals(q, x, y, z, zb=None):
    """prim_res, dual_res as include/mpc_qp_abi.h defines them (inf-norms at the returned point), and the largest term that enters either sum."""
    mx = lambda a: float(np.max(a, initial=0.0))
    s = q["C"] @ x
    prim = max(mx(np.abs(q["A"] @ x - q["b"])), mx(s - q["u"]), mx(q["l"] - s), 0.0)
    terms = [q["H"] * x, q["g"], q["A"].T * y, q["C"].T * z, q["A"] * x, q["b"], q["C"] * x]
    dual = q["H"] @ x + q["g"] + q["A"].T @ y + q["C"].T @ z
    if zb is not None:
        prim = max(prim, mx(x - q["u_box"]), mx(q["l_box"] - x))
        dual = dual + zb
        terms.append(zb)
    return prim, mx(np.abs(dual)), max(mx(np.abs(t)) for t in terms)


# Tolerances of the planted comparison, measured on the CPU oracle (never on the HIP kernel) on exactly PLANTED_GRID with planted_problems and
# PLANTED_SETTINGS (tests/test_oracle_qp.py::test_planted_solution holds them; profiles/qp_planted.txt has every shape's figures):
#   worst error / (kappa eps_abs) over the grid without (16, 1, 1, box): 5.74, at (33, 16, 9); on (16, 1, 1, box): 13.3.
# Both come from the stop rule ("What the stop rule of the QP bounds"): it bounds the violation of a bound by eps_abs, not the distance to it
# on the feasible side, so a point may carry a multiplier on a row and rest inside it by a few eps_abs / (mu_in |z|)-sized steps.
# TOL = 10 x the oracle's worst: the five kernels sum in other orders than the oracle, and a Newton pass that ends at the tolerance may end one step apart.
PLANTED_ORACLE_WORST_RATIO = 5.74
PLANTED_TOL = 10 * PLANTED_ORACLE_WORST_RATIO
PLANTED_TOL_OF_SHAPE = {(16, 1, 1, True, 1, 2): 10 * 13.3}
# complementarity (kkt_residuals' third result): the oracle's worst over the grid is 1.43e-5, at (33, 16, 9); bound = 10 x
PLANTED_COMP_BOUND = 10 * 1.43e-5


def planted_tol(shape):
    return PLANTED_TOL_OF_SHAPE.get(tuple(shape), PLANTED_TOL)


def planted_error(q, x, y, z, zb=None):
    mx = lambda a: float(np.max(np.abs(a), initial=0.0))
    return max(mx(x - q["x"]), mx(y - q["y"]), mx(z - q["z"]), mx(zb - q["z_box"]) if zb is not None else 0.0)


def check_planted(shape, q, x, y, z, zb, info, eps_abs=PLANTED_SETTINGS["eps_abs"], tag=""):
    """Everything the planted tests require of ONE returned solution (zb: None without a box).  -> dict of the measured figures."""
    tag = "%s %s" % (tuple(shape), tag)
    assert info.status == 0, (tag, info.status, info.prim_res, info.dual_res, info.iters, info.iters_in)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.all(np.isfinite(z)), tag
    # the residuals the solver reports are those of the point it returns
    prim, dual, term = qp_residuals(q, x, y, z, zb)
    assert info.prim_res <= eps_abs and info.dual_res <= eps_abs, (tag, info.prim_res, info.dual_res)
    assert abs(info.prim_res - prim) <= 1e-12 * (1 + term) and abs(info.dual_res - dual) <= 1e-12 * (1 + term), (tag, info.prim_res, prim, info.dual_res, dual)
    # the active set is the planted one, multiplier signs included
    assert np.array_equal(np.sign(z), np.sign(q["z"])), (tag, np.sign(z), np.sign(q["z"]))
    n_act = int(np.count_nonzero(q["z"]))
    if zb is not None:
        assert np.array_equal(np.sign(zb), np.sign(q["z_box"])), (tag, np.sign(zb), np.sign(q["z_box"]))
        n_act += int(np.count_nonzero(q["z_box"]))
    assert info.n_active == n_act, (tag, info.n_active, n_act)
    stat, prim_kkt, comp = kkt_residuals(q, x, y, z, zb)
    assert stat < 2 * eps_abs and prim_kkt < 2 * eps_abs and comp <= PLANTED_COMP_BOUND, (tag, stat, prim_kkt, comp)
    err = planted_error(q, x, y, z, zb)
    ratio = err / (q["kappa"] * eps_abs)
    assert ratio <= planted_tol(shape), (tag, err, q["kappa"], ratio)
    return dict(err=err, ratio=ratio, comp=comp, stat=stat, prim=prim_kkt, iters=info.iters, iters_in=info.iters_in)
