"""The back-substitution kernels between the consensus over the cuts and the trial evaluation: k_leg_apply with chunks of consecutive
knots per workgroup (csrc/legs.h: every Lm read once per chunk) and k_duals with the per-row scalars staged in LDS (csrc/solver_kernels.h:
a row that contributes nothing costs neither a load nor a reduction).  Which workgroup forms which sum changes, the sums do not: a handle
with the earlier forms (MPC_LEG_APPLY_CHUNK=1, MPC_DUALS_PLAIN=1) and a handle with the new ones give the same bits — trajectories, the
gains and affine terms of every knot, the multiplier steps and the per-instance statistics, after a cold solve and after every MPC tick."""
import numpy as np
import pytest

from mpc_benchmark_amd.ensemble import EnsembleMPC
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem

pytestmark = pytest.mark.gpu

COLD_ITERS = 1   # one cold pass, then three MPC ticks
TICKS = 3
KNOBS = ("MPC_LEG_APPLY_CHUNK", "MPC_DUALS_PLAIN", "MPC_LEG_TAIL_CUS")
_PROBLEMS = {}
_OLD = {}        # traces of the handles with the earlier forms: computed once per problem, shared by the cases, never modified


def _problem(kind, N):
    key = (kind, N)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = (CentroidalProblem(horizon=N) if kind == "centroidal" else
                          KinodynamicProblem(horizon=N, complete_model=False) if kind == "kinodynamic" else
                          FullDynamicsProblem(horizon=N, complete_model=False))
    return _PROBLEMS[key]


def _at_joint_limit(pd, x):
    """The joint whose position is nearest to one of its limits (the box of the stage's joint-limit rows, problems/fulldynamic.py
    create_stage) moved 0.02 rad past that limit: the row is violated at knot 0, where the state is fixed, and is active there."""
    m = pd.robot.model
    nj = m.nv - 6
    lo, hi = np.asarray(m.lowerPositionLimit[7:7 + nj], dtype=float), np.asarray(m.upperPositionLimit[7:7 + nj], dtype=float)
    q = x[7:7 + nj]
    d_lo = np.where(np.isfinite(lo), np.abs(q - lo), np.inf)
    d_hi = np.where(np.isfinite(hi), np.abs(hi - q), np.inf)
    j = int(np.argmin(np.minimum(d_lo, d_hi)))
    x[7 + j] = hi[j] + 0.02 if d_hi[j] <= d_lo[j] else lo[j] - 0.02


def _handle(monkeypatch, lib, kind, N, legs, batch, chunk, plain, cus=None):
    """A handle whose developer knobs (read once, when the handle is created) are `chunk` (None: unset, the automatic choice), `plain`, `cus`."""
    for name, val in zip(KNOBS, (chunk, 1 if plain else None, cus)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    pd = _problem(kind, N)
    ens = EnsembleMPC(pd, batch=batch, library=lib, seed=11, sigma_q=0.005, sigma_v=0.01)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    if kind == "centroidal":
        rng = np.random.default_rng(11)
        ens.x0[1:] += 1e-2 * rng.standard_normal(ens.x0[1:].shape)
    elif kind == "fulldynamic":
        _at_joint_limit(pd, ens.x0[batch - 1])
    ens.options.riccati_legs = legs
    ens.options.tol = 0.0  # a fixed number of iterations
    ens.native.set_options(ens.options)
    ens.prepare_schedule(TICKS + 2)
    return ens


PER_KNOT = ("p", "phi", "kff", "knu", "dvs", "dlams", "dx")


def _snapshot(ens, stats):
    """Everything the two kernels write or feed, as bytes: the iterate, the feedback gains, the affine terms of every gain record
    (p, phi, k, knu), the multiplier steps (dvs, dlams) and the primal step of every knot, and the per-instance status."""
    r = ens.results(gains=True)
    out = {"xs": r["xs"], "us": r["us"], "K": r["K"], "kff_all": r["kff"],
           "status": np.array([[s.num_iters, s.alpha, s.converged, s.traj_cost] for s in stats], dtype=float)}
    N, B = ens.dims.horizon, ens.batch
    for name in PER_KNOT:
        out[name] = np.concatenate([ens.native.debug_get(name, k, b).ravel() for b in range(B) for k in range(N + (0 if name == "kff" else 1))])
    return {k: np.ascontiguousarray(v).tobytes() for k, v in out.items()}, r


def _trace(ens):
    """One cold pass, then TICKS MPC ticks: a snapshot after each ; ens.active_rows: the active rows of every knot at each snapshot."""
    out, ens.active_rows = [], []
    for t in range(TICKS + 1):
        stats = ens.cold_solve(max_iters=COLD_ITERS) if t == 0 else ens.step()
        snap, r = _snapshot(ens, stats)
        assert np.all(np.isfinite(r["xs"])) and np.all(np.isfinite(r["us"])), t
        out.append(snap)
        ens.active_rows.append(_active_rows(ens))
    return out


def _probe(ens):
    v = ens.native.debug_get("backsubst", 0)
    return {"chunk": int(v[0]), "chunked": int(v[1]), "single": int(v[2]), "staged": int(v[3]), "plain": int(v[4]), "grid": int(v[5])}


def _active_rows(ens):
    """Active constraint rows of every knot of every instance (from the knot records)."""
    return np.array([[int(np.count_nonzero(ens.native.debug_get("act", k, b))) for k in range(ens.dims.horizon + 1)] for b in range(ens.batch)])


def _assert_same(a, b):
    assert len(a) == len(b) == TICKS + 1
    for t, (sa, sb) in enumerate(zip(a, b)):
        assert sa.keys() == sb.keys()
        for name in sa:
            assert len(sa[name]) > 0 and sa[name] == sb[name], (t, name)


def _chunks(N, J, C):
    return sum(-(-((j + 1) * N // J - j * N // J) // C) for j in range(J - 1))


def _old(monkeypatch, lib, kind, N, legs, batch):
    key = (kind, N, legs, batch)
    if key not in _OLD:
        ens = _handle(monkeypatch, lib, kind, N, legs, batch, 1, True)
        tr = _trace(ens)
        p = _probe(ens)
        assert p["staged"] == 0 and p["plain"] > 0 and p["chunked"] == 0, p
        assert (p["single"] > 0 and p["chunk"] == 1) if legs > 1 else p["single"] == 0, p
        _OLD[key] = tr
    return _OLD[key]


def _compare(monkeypatch, lib, kind, N, legs, batch, chunk, cus=None, want_chunk=None):
    old = _old(monkeypatch, lib, kind, N, legs, batch)
    ens = _handle(monkeypatch, lib, kind, N, legs, batch, chunk, False, cus=cus)
    new = _trace(ens)
    p = _probe(ens)
    want = (chunk if want_chunk is None else want_chunk)
    assert p["plain"] == 0 and p["staged"] >= COLD_ITERS + TICKS, p
    if legs > 1:
        assert p["chunk"] == min(want, 32) and p["grid"] == _chunks(N, legs, p["chunk"]), p
        assert (p["chunked"] == 0 and p["single"] > 0) if want == 1 else (p["single"] == 0 and p["chunked"] > 0), p
    else:
        assert p["chunked"] == 0 and p["single"] == 0, p   # one leg: k_leg_apply does not run, k_duals takes [A B][dx; du] from the serial sweep
    _assert_same(old, new)
    return ens


@pytest.mark.parametrize("chunk", [1, 2, 3, 8])
def test_reduced_model_four_legs(hip_lib, monkeypatch, chunk):
    """N = 10 with 4 legs: the parametric legs have 2, 3 and 2 knots.  C = 2: a short chunk and chunks that end at a cut ; C = 3: one chunk per
    leg, two of them short ; C = 8: larger than every leg ; C = 1: only k_duals differs.  Instance 2 starts past a joint limit: knots with
    active rows and knots without any, in the parametric legs."""
    ens = _compare(monkeypatch, hip_lib, "fulldynamic", 10, 4, 3, chunk)
    assert ens.dims.nu == 22
    act = np.array(ens.active_rows)   # [snapshot][instance][knot]
    assert act[0, 2, 0] >= 1, act     # the violated joint limit at the fixed initial state of the cold pass
    assert np.any(act[:, :, :7] >= 1) and np.any(act[:, :, :7] == 0), act   # (knots 0 .. 6: the parametric legs)


@pytest.mark.parametrize("N,legs,chunk", [(10, 4, 2), (7, 2, 2), (7, 2, 3)])
def test_kinodynamic_generic_dimensions(hip_lib, monkeypatch, N, legs, chunk):
    """m = 34: the generic-dimension paths.  N = 7 with 2 legs: one parametric leg of 3 knots, C = 2 cuts it into 2 + 1."""
    ens = _compare(monkeypatch, hip_lib, "kinodynamic", N, legs, 3, chunk)
    assert ens.dims.nu == 34


def test_one_leg(hip_lib, monkeypatch):
    """legs = 1: the serial sweep, no k_leg_apply ; k_duals with [A B][dx; du] left by the forward sweep."""
    ens = _compare(monkeypatch, hip_lib, "fulldynamic", 7, 1, 3, 2)
    act = np.array(ens.active_rows)
    assert np.any(act >= 1) and np.any(act == 0), act


def test_automatic_chunk(hip_lib, monkeypatch):
    """MPC_LEG_APPLY_CHUNK unset: N x B = 30 workgroups are one round of the real device, one knot per workgroup ; with 8 compute units
    (MPC_LEG_TAIL_CUS) the grid exceeds a round and the chunks are 5 knots (here: every parametric leg in one chunk)."""
    _compare(monkeypatch, hip_lib, "fulldynamic", 10, 4, 3, None, want_chunk=1)
    _compare(monkeypatch, hip_lib, "fulldynamic", 10, 4, 3, None, cus=8, want_chunk=5)


def test_finished_instance_is_left_alone(hip_lib, monkeypatch):
    """Batch 3, centroidal ensemble solved to convergence with instance 1 started AT the solution: it is done after its first iteration,
    the others still step, so its workgroups leave both kernels at once in the later passes and its records keep their bits."""
    kind, N, legs, batch = "centroidal", 20, 5, 3
    pd = _problem(kind, N)
    sol, out = None, {}
    for tag, chunk, plain in (("solution", 1, True), ("old", 1, True), ("new", 3, False)):
        ens = _handle(monkeypatch, hip_lib, kind, N, legs, batch, chunk, plain)
        ens.options.tol = 1e-5
        ens.options.max_iters = 60
        ens.native.set_options(ens.options)
        xs, us = pd.initial_guess()
        xs = np.tile(np.array(xs)[None], (batch, 1, 1))
        us = np.tile(np.array(us)[None], (batch, 1, 1))
        xs[:, 0, :] = ens.x0
        if sol is not None:
            xs[1], us[1] = sol
        ens.native.set_x0(ens.x0)
        ens.native.setup()
        stats = ens.native.run(xs, us)
        assert all(s.converged for s in stats)
        if sol is None:
            r = ens.results(gains=False)
            sol = (r["xs"][1].copy(), r["us"][1].copy())
            continue
        out[tag] = (_snapshot(ens, stats)[0], np.array([s.num_iters for s in stats]), _probe(ens))
    its = out["new"][1]
    assert its[1] < min(its[0], its[2]), its  # instance 1 was done while the others stepped
    assert np.array_equal(its, out["old"][1])
    assert out["new"][2]["chunk"] == 3 and out["new"][2]["plain"] == 0 and out["old"][2]["staged"] == 0 and out["old"][2]["chunked"] == 0
    for name in out["old"][0]:
        assert out["old"][0][name] == out["new"][0][name], name
