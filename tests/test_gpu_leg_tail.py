"""k_leg_condense_tail (csrc/legs.h): the last leg's per-knot pass walked beside the condensation of the parametric legs.  Which
workgroup runs which body changes, the bodies do not: a handle with the fused launch and a handle with the separate launches
(MPC_LEG_TAIL_KNOTS=0) give the same bits — trajectories, gains of knot 0 and per-instance statistics after a cold solve and after
every MPC tick."""
import numpy as np
import pytest

from mpc_benchmark_amd.ensemble import EnsembleMPC
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem

pytestmark = pytest.mark.gpu

COLD_ITERS = 3
TICKS = 3
_PROBLEMS = {}


def _problem(kind, N, complete):
    """(problem definitions are built once and shared by the handles of every case that uses them: they are never modified)"""
    key = (kind, N, complete)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = (CentroidalProblem(horizon=N) if kind == "centroidal" else
                          KinodynamicProblem(horizon=N, complete_model=complete) if kind == "kinodynamic" else
                          FullDynamicsProblem(horizon=N, complete_model=complete))
    return _PROBLEMS[key]


def _x0(pd, ens, batch, seed):
    """Seeded initial states of a vector-space ensemble (EnsembleMPC perturbs only multibody states): instance 0 nominal."""
    rng = np.random.default_rng(seed)
    x0 = np.tile(np.asarray(ens.problem.x0_init, dtype=float), (batch, 1))
    x0[1:] += 1e-2 * rng.standard_normal(x0[1:].shape)
    return x0


def _handle(monkeypatch, lib, kind, N, legs, batch, complete, knob, cus=None):
    """A handle whose developer knobs (read once, when the handle is created) are `knob` (None: unset, the automatic choice) and `cus`."""
    for name, val in (("MPC_LEG_TAIL_KNOTS", knob), ("MPC_LEG_TAIL_CUS", cus)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    pd = _problem(kind, N, complete)
    ens = EnsembleMPC(pd, batch=batch, library=lib, seed=7, sigma_q=0.005, sigma_v=0.01)
    if kind == "centroidal":
        ens.x0 = _x0(pd, ens, batch, 7)
    monkeypatch.delenv("MPC_LEG_TAIL_KNOTS", raising=False)
    monkeypatch.delenv("MPC_LEG_TAIL_CUS", raising=False)
    ens.options.riccati_legs = legs
    ens.options.tol = 0.0  # a fixed number of iterations
    ens.native.set_options(ens.options)
    ens.prepare_schedule(TICKS + 2)
    return ens


def _snapshot(ens, stats):
    r = ens.results(gains=True)
    return (r["xs"].copy(), r["us"].copy(), r["K"][:, 0].copy(), r["kff"][:, 0].copy(),
            np.array([s.num_iters for s in stats]), np.array([s.alpha for s in stats]))


def _trace(ens):
    """Cold solve of COLD_ITERS iterations, then TICKS MPC ticks: a snapshot after each."""
    out = [_snapshot(ens, ens.cold_solve(max_iters=COLD_ITERS))]
    for _ in range(TICKS):
        out.append(_snapshot(ens, ens.step()))
    return out


def _probe(ens):
    v = ens.native.debug_get("leg_tail", 0)
    return {"tail": int(v[0]), "fused": int(v[1]), "separate": int(v[2]), "legs": int(v[4]), "cus": int(v[5]), "multi": int(v[6]), "single": int(v[7])}


def _assert_same(a, b):
    assert len(a) == len(b) == TICKS + 1
    for t, (sa, sb) in enumerate(zip(a, b)):
        for name, x, y in zip(("xs", "us", "K0", "k0", "iterations", "alpha"), sa, sb):
            assert np.all(np.isfinite(x)), (t, name)
            assert np.array_equal(x, y), (t, name, float(np.max(np.abs(x - y))))


def _last_leg(N, J):
    return N - (J - 1) * N // J


WHOLE = 1000  # MPC_LEG_TAIL_KNOTS above any leg: the whole last leg in the fused launch (the automatic choice fuses only ensembles that fill the chip)


def _compare(monkeypatch, lib, kind, N, legs, batch, complete, knob=WHOLE, want_tail=None):
    sep = _handle(monkeypatch, lib, kind, N, legs, batch, complete, 0)
    fus = _handle(monkeypatch, lib, kind, N, legs, batch, complete, knob)
    a, b = _trace(sep), _trace(fus)
    ps, pf = _probe(sep), _probe(fus)
    J = pf["legs"]
    assert ps["legs"] == J
    # the code path: the handle with MPC_LEG_TAIL_KNOTS=0 never launched the fused kernel, the other one never the separate condensation ;
    # the first pass of either swept several times (no guess of the value function at the cuts yet), every later pass once, and the
    # fused kernel served both kinds of passes (every launch of the condensation is counted)
    assert ps["fused"] == 0 and ps["tail"] == 0
    if J > 1:
        assert ps["separate"] > 0 and pf["separate"] == 0
        assert pf["tail"] == (_last_leg(N, J) if want_tail is None else want_tail), pf
        assert pf["multi"] == ps["multi"] == 1 and pf["single"] == ps["single"] and pf["single"] >= COLD_ITERS - 1 + TICKS, (pf, ps)
        assert pf["fused"] == ps["separate"] >= 2 * pf["multi"] + pf["single"], (pf, ps)
    else:
        assert pf["fused"] == 0 and pf["separate"] == 0 and pf["tail"] == 0
    _assert_same(a, b)
    return sep, fus


@pytest.mark.parametrize("kind,N,legs,batch,complete,nu", [
    ("fulldynamic", 9, 3, 3, False, 22),   # fixed-dimension kernels of the reduced model
    ("fulldynamic", 8, 4, 2, True, 32),    # the benchmark's instantiation
    ("kinodynamic", 10, 3, 2, True, 44),   # m = 44: the MP = 48 plan
    ("centroidal", 20, 5, 3, False, None),  # generic small dimensions
    ("fulldynamic", 2, 2, 2, False, 22),   # last leg of one knot
    ("fulldynamic", 3, 2, 2, False, 22),   # first leg of one knot, last leg of two
])
def test_fused_launch_equals_separate_launches(hip_lib, monkeypatch, kind, N, legs, batch, complete, nu):
    sep, fus = _compare(monkeypatch, hip_lib, kind, N, legs, batch, complete)
    assert _probe(fus)["legs"] == legs
    if nu is not None:
        assert fus.dims.nu == nu
    fixed = int(fus.native.debug_get("fixed_dims", 0)[0])
    assert (fixed > 0) == (kind != "centroidal")


def test_more_legs_than_knots(hip_lib, monkeypatch):
    """Horizon 1 with 8 legs asked for: whatever number of legs the library settles on (as test_short_horizons_with_legs)."""
    _compare(monkeypatch, hip_lib, "fulldynamic", 1, 8, 2, False)


@pytest.mark.parametrize("t", [1, 2])
def test_partial_tails(hip_lib, monkeypatch, t):
    """MPC_LEG_TAIL_KNOTS=t: only the last t knots of the last leg (3 knots) in the fused launch, the others in k_leg_knot."""
    _compare(monkeypatch, hip_lib, "fulldynamic", 9, 3, 3, False, knob=t, want_tail=t)


def test_fallback_when_the_grid_exceeds_the_chip(hip_lib, monkeypatch):
    """Automatic choice (MPC_LEG_TAIL_KNOTS unset): nlegs x B = 9 workgroups in the fused grid, N x B = 27 in k_leg_knot.  With 8 compute
    units (MPC_LEG_TAIL_CUS) the fused grid exceeds one round of the chip and the separate launches stay ; with 9 it fits and the tail is
    4 / 5 of a parametric leg (2 of 3 knots) ; on the real device (27 workgroups: k_leg_knot is one round already) the separate launches
    stay again.  Same bits every time."""
    args = ("fulldynamic", 9, 3, 3, False)
    small = _handle(monkeypatch, hip_lib, *args, None, cus=8)
    fits = _handle(monkeypatch, hip_lib, *args, None, cus=9)
    real = _handle(monkeypatch, hip_lib, *args, None)
    a, b, c = _trace(small), _trace(fits), _trace(real)
    ps, pf, pr = _probe(small), _probe(fits), _probe(real)
    assert ps["cus"] == 8 and ps["tail"] == 0 and ps["fused"] == 0 and ps["separate"] > 0, ps
    assert pf["cus"] == 9 and pf["tail"] == 2 and pf["separate"] == 0 and pf["fused"] == ps["separate"], pf
    assert pr["cus"] >= 64 and pr["tail"] == 0 and pr["fused"] == 0 and pr["separate"] == ps["separate"], pr  # the device's own count
    _assert_same(a, b)
    _assert_same(a, c)


def test_converged_instance_leaves_both_roles_early(hip_lib, monkeypatch):
    """Centroidal ensemble solved to convergence, instance 0 started AT the solution: it is done after its first iteration while the
    others still step, so its workgroups (condensation role and tail role alike) leave at once in the later passes."""
    kind, N, legs, batch = "centroidal", 20, 5, 3
    pd = _problem(kind, N, False)
    sol = None
    out = {}
    for tag, knob in (("solution", 0), ("separate", 0), ("fused", WHOLE)):
        ens = _handle(monkeypatch, hip_lib, kind, N, legs, batch, False, knob)
        ens.options.tol = 1e-5
        ens.options.max_iters = 60
        ens.native.set_options(ens.options)
        xs, us = pd.initial_guess()
        xs = np.tile(np.array(xs)[None], (batch, 1, 1))
        us = np.tile(np.array(us)[None], (batch, 1, 1))
        xs[:, 0, :] = ens.x0
        if sol is not None:
            xs[0], us[0] = sol
        ens.native.set_x0(ens.x0)
        ens.native.setup()
        stats = ens.native.run(xs, us)
        if sol is None:
            assert all(s.converged for s in stats)
            r = ens.results(gains=False)
            sol = (r["xs"][0].copy(), r["us"][0].copy())
            continue
        ens.options.max_iters = 1
        ens.native.set_options(ens.options)
        ens.native.set_x0(None)
        tr = [_snapshot(ens, stats)]
        for _ in range(TICKS):
            tr.append(_snapshot(ens, ens.step()))
        out[tag] = (tr, [bool(s.converged) for s in stats], _probe(ens))
    its = out["fused"][0][0][4]
    assert all(out["fused"][1]) and all(out["separate"][1])
    assert its[0] < its[1:].min(), its  # instance 0 was done while the others stepped
    assert out["fused"][2]["separate"] == 0 and out["fused"][2]["tail"] == _last_leg(N, legs) and out["separate"][2]["fused"] == 0
    _assert_same(out["separate"][0], out["fused"][0])
