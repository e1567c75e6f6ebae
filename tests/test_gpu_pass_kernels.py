"""The kernels of a solver pass are chosen once per handle, in one table (csrc/pass_kernels.h): this test holds the table to what the
handle's dimensions call for.  For every configuration below, kernel_info() must name the instantiations listed here letter for
letter, with the threads per workgroup, the dynamic LDS bytes and the workgroups per launch worked out HERE from the dimensions: the
LDS bytes by the make_*_lds rules of riccati_layout.h and legs.h (re-stated below), the grids from N, B, the number of legs, the tail
and the chunk.  VGPR counts are printed, not pinned.  The stage kernel's entries (eval_multibody.hip has its own variant list, which
this test does not look into) are held to their names, threads, grids and the LDS bytes of make_mb_lds (eval_multibody_host.h).  Some
configurations also run one profiled tick: the profile slots and the probes of debug_get("leg_tail") / ("backsubst") must show the
launch form the report named.

What the report cannot show: the generic rows of a family share one name (k_leg_knot for <16>, <32> and <48> ; k_leg_consensus,
k_leg_compose and k_leg_tree_down for 16 .. 80 ; k_forward_phi for <4,10> and <6,10> ; "k_riccati_mfma (serial sweep)" for all five
serial forms), so name, threads, LDS bytes and grid do not pin the template argument of those rows: a wrong generic instantiation
would pass here.  The names are the report's own from before the table and stay as they were ; that the right instantiation runs was
checked once, bit for bit against the library before the table (profiles/pass_kernels_refactor.txt).

The report was corrected where it disagreed with the launches, so three expectations hold from the table on and fail on the library
before it: the k_leg_knot grid under MPC_LEG_KNOT_CHUNK (ceil(knots / chunk) x B, it was knots x B: the "chunk3" case), the grid of
the k_leg_tree_down entry, which is labelled "last level" (nodes of the last level + 1, it was the nodes of the FIRST level: the
"legs3" case ; with 4 legs both are 2), and the thread counts in the sweep's names in a build with -DRIC_THREADS=256 (`make variants`:
not built by this test).

Rows of the table that no problem of the repository reaches (a vector-space problem with 16 < n <= 80 or a state of 80 < n <= 96
would ; the developer knob MPC_HIP_DENSE_AB is not a supported configuration): k_riccati_mfma<512,96>, <512,96,true>, <512,80> and
<512,80,false,true> ; k_leg_consensus / k_leg_compose / k_leg_tree_down<32> and <48> (16 < n <= 48) ; k_forward, the serial forward
sweep of n > 80 or m > 48.  The serial forward sweeps are not entries of the report: test_serial_forward_sweeps launches
k_forward_phi<4,10> after k_closed_loop, k_forward_prefetch<4,10> (full dynamics, forward_mode = 1) and k_forward_prefetch<6,10>
(kinodynamic, m = 44), and sees their profile slot and finite results, no more.
Centroidal problems (n = 9, m = 12) reach the small-problem sweeps, <256,16> and <256,16,false,true>."""
import numpy as np
import pytest

from mpc_benchmark_amd import _capi as K
from mpc_benchmark_amd.ensemble import EnsembleMPC
from mpc_benchmark_amd.problems.centroidal import CentroidalProblem
from mpc_benchmark_amd.problems.fulldynamic import FullDynamicsProblem
from mpc_benchmark_amd.problems.kinodynamic import KinodynamicProblem

pytestmark = pytest.mark.gpu

N, B = 8, 2
WHOLE = 1000  # MPC_LEG_TAIL_KNOTS above any leg: the whole last leg in the fused launch
KNOBS = ("MPC_LEG_TAIL_KNOTS", "MPC_LEG_KNOT_CHUNK", "MPC_HIP_GENERIC_DIMS", "MPC_LEGS_CHAIN", "MPC_HIP_GENERIC_RICCATI", "MPC_DUALS_PLAIN")
_PROBLEMS = {}

# (n, m) -> (id, gfull, st_lds, NP, MP): the fixed-dimension models and the sweep's LDS plan for them (MPC_FIXED_MODELS)
FIXED = {(76, 32): (1, 1, 1, 80, 32), (76, 44): (2, 3, 0, 80, 48), (56, 22): (3, 3, 1, 64, 32), (56, 34): (4, 3, 1, 64, 48)}


def _problem(kind, complete):
    """(problem definitions are built once and shared by the handles of every case: they are never modified)"""
    key = (kind, complete)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = (CentroidalProblem(horizon=N) if kind == "centroidal" else
                          KinodynamicProblem(horizon=N, complete_model=complete) if kind == "kinodynamic" else
                          FullDynamicsProblem(horizon=N, complete_model=complete))
    return _PROBLEMS[key]


def _handle(monkeypatch, lib, kind, complete, legs, env):
    """A handle whose developer knobs (read once, when the handle is created) are `env` ; every other knob unset."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, str(val))
    ens = EnsembleMPC(_problem(kind, complete), batch=B, library=lib, seed=7, sigma_q=0.005, sigma_v=0.01)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    ens.options.riccati_legs = legs
    ens.options.tol = 0.0  # a fixed number of iterations
    ens.native.set_options(ens.options)
    ens.prepare_schedule(3)
    return ens


# ---- the LDS rules, from the dimensions --------------------------------------------------------------------------------------------
def _pad(x):
    return (x + 15) & ~15


def _even(x):
    return (x + 1) & ~1


def _ric_bytes(n, m, c, gfull, st):
    """total_bytes of make_ric_lds (riccati_layout.h): Pt, then the largest of the three phase views, the legs' solve, the vectors."""
    np_, mp = _pad(n), _pad(m)
    nzp, ldl, ldr, nb, nbm, lw = np_ + mp, np_ + 1, mp + 1, np_ // 16, mp // 16, np_ + 17
    g1 = gfull in (1, 3)
    skip = ((n // 2) & ~3) if gfull == 3 else 0
    r1 = _even(np_ * (np_ + 1))
    end1 = r1 + _even(np_ * ldl) + _even(nb * 272)
    gp = r1 + _even((np_ - skip) * nzp)
    end2 = gp + _even(np_ * mp if g1 else max(np_ * 16, 8 * nzp))
    rest = [mp * lw, mp * np_ if st else 0, 16 * lw, 16 * lw, mp * 17, 16 * 17, 272]  # W ST CT VX Y SC LIs
    end3 = r1 + _even(mp * ldr) + _even(nbm * 272) + sum(_even(x) for x in rest)
    cur = r1 + sum(_even(x) for x in rest)
    if gfull == 3 and nbm <= 3:
        end3 = max(cur, gp) + _even(mp * ldr) + _even(nbm * 272)
    if gfull == 1 and nbm <= 3:
        need = _even(mp * ldr) + _even(nbm * 272)
        if need <= np_ * mp and cur <= gp + ((np_ * mp - need) & ~1):
            end3 = gp + np_ * mp
    o = max(end1, end2, end3)
    if np_ * (np_ + 1) < (mp + 16) * (mp + 1):
        o += _even((mp + 16) * (mp + 1))
    o += _even(7 * nzp + 2 * c + 96 + 80)
    return o * 8 + (c + 72) * 4


def _lk_bytes(n, m):
    np_, mp = _pad(n), _pad(m)
    nzp, lda, ldp, ldm = np_ + mp, np_ + mp + 1, np_ + 1, mp + 1
    return 8 * (_even(np_ * lda) + _even(max(np_ * ldp, mp * np_ + mp * ldm)) + _even(6 * nzp + 6 * np_ + 40) + _even(16 * ldm) + _even(mp + 3 * np_ + 80 + 8))


def _lc_bytes(n):
    np_ = _pad(n)
    ld = np_
    while ld & 31 != 16:
        ld += 1
    return 8 * (3 * _even(np_ * ld) + _even(3 * np_ + 16))


def _lx_bytes(n, m):
    np_ = _pad(n)
    return 8 * (3 * _even(np_ * (np_ + 1)) + _even(8 * np_ + 16 + 128)) + (2 * np_ + 8) * 4


def _mb_bytes(nj, nv, nq, nu, nz, contact_dyn):
    """total_bytes of make_mb_lds (eval_multibody_host.h), the stage kernel's carve-out: body and dof arrays, vectors, the derivative
    blocks, then one region shared in time by the body-level blocks, the factor of M (only with contact-constrained dynamics) and the
    staged Jacobian rows of the terms ; the d lambda rows ; behind the doubles, the integer tables of the tree."""
    nvp = _pad(nv)
    nbm, ldl = nvp // 16, 16 * ((nz + 15) // 16) + 1
    ldj = ((nz - 16 + 31) // 32) * 32 + 16  # leading dimension of the staged Jacobian rows
    o = sum(_even(k * nj) for k in (9, 3, 6, 6, 6, 6)) + 3 * _even(6 * nv)                     # oR op ov oa Hc Fc | J U Psd
    o += _even(nq + nv) + _even(max(nu, 1)) + _even(nq + nv) + _even(nvp) + 16 + 16 + _even(nv)  # x u xn | a lam gam bias
    o += 2 * (12 + 36 + 6) + (6 * 36 + 64) + 6 * 48 + (112 + 24 * 4)                            # cfr small se3 (6 slots) red (4 wavefronts)
    o += _even(2 * nz + 36 + 24 + 2 + 16) + 7 * _even(6 * nv)                                   # early | Phi Bt Tv BcPsd YcPsd Psdd Tq
    yc = o
    o += _even(21 * nj)
    e1 = o + 2 * _even(36 * nj) + 2 * _even(6 * nj)                                             # stage 1: oY Bc oh of
    if contact_dyn:
        o += _even(nbm * (nbm + 1) // 2 * 272) + _even(nvp * 17) + 272 + 272                    # stage 2: Mt Y16 Sp LIs
    o = max(o, e1)
    if o < yc + 32 * ldj + 8:                                                                   # stage 3: 32 staged rows from Yc on
        o = _even(yc + 32 * ldj + 8)
    o += _even(max(12 * ldl, nvp * 16)) if contact_dyn else 2                                   # DL
    return o * 8 + 4 * nj * 8 + nv * 4 + nj * 4 * 3 + 64


def _tree_levels(J):
    """inner nodes created per level of the tree over the cuts: adjacent nodes paired, an odd one carried up"""
    out, cnt = [], J
    while cnt > 1:
        out.append(cnt // 2)
        cnt = cnt // 2 + cnt % 2
    return out


def _expected(d, legs, env, nj=0, contact_dyn=False):
    """[(name, threads, dynamic LDS, workgroups)] of kernel_info() for dimensions d (whole-body problems: nj bodies, and whether some
    stage has contact-constrained dynamics)"""
    n, m, c = d.ndx, d.nu, d.nc_max
    nz = n + m
    vector = d.space == K.SPACE_VECTOR
    knots = (N + 1) * B
    if vector:
        e = [("k_eval_vector<0> (stage kernel, value + derivatives)", 64, 0, knots), ("k_eval_vector<1> (linesearch candidate)", 64, 0, knots)]
    else:
        mb = _mb_bytes(nj, n // 2, d.nx - n // 2, m, nz, contact_dyn)
        e = [("k_eval_multibody<0> (stage kernel, value + derivatives)", 256, mb, knots), ("k_eval_multibody<3> (alpha = 1 candidate with derivatives)", 256, mb, knots),
             ("k_eval_multibody<1> (backtracking candidates, values only)", 256, mb, knots)]
    generic_riccati = "MPC_HIP_GENERIC_RICCATI" in env
    J = 1 if generic_riccati else min(legs, N)
    fx = None if (vector or "MPC_HIP_GENERIC_DIMS" in env) else FIXED[(n, m)]
    # the sweep's LDS plan: whole-body problems the one of their model's row of MPC_FIXED_MODELS (whatever kernels serve them),
    # the centroidal problem plan 1 ; small problems (np = mp = 16) run 256 threads
    ric = _ric_bytes(n, m, c, 1, 1) if vector else _ric_bytes(n, m, c, FIXED[(n, m)][1], FIXED[(n, m)][2])
    assert ric <= 160 * 1024
    rt = 256 if vector else 512
    if J > 1:
        tail = min(int(env.get("MPC_LEG_TAIL_KNOTS", 0)), N - (J - 1) * N // J)
        chunk = int(env.get("MPC_LEG_KNOT_CHUNK", 1))
        tree = J >= 3 and "MPC_LEGS_CHAIN" not in env
        lk, lc, lx = _lk_bytes(n, m), _lc_bytes(n), _lx_bytes(n, m)
        if fx:
            _, gf, st, NP, MP = fx
            dims3, dimsx = "%d,%d,%d" % (MP, n, m), "%d,%d,%d" % (NP, n, m)
            e.append(("k_riccati_mfma<512,80,true,true,%d,%d,%d,%d> (sweep, legs, fixed dimensions)" % (n, m, gf, st), 512, ric, B * J))
            names = {"knot": "k_leg_knot<%s> (fixed dimensions)" % dims3, "condense": "k_leg_condense<%d> (fixed dimensions)" % n,
                     "tail": "k_leg_condense_tail<%s> (fixed dimensions)" % dims3,
                     "compose": "k_leg_compose<%s> (first level of the tree over the cuts, fixed dimensions)" % dimsx,
                     "down": "k_leg_tree_down<%s> (last level, fixed dimensions)" % dimsx}
        else:
            e.append(("k_riccati_mfma<256,16,false,true> (sweep, legs)" if vector else "k_riccati_mfma<512,80,true,true> (sweep, legs)", rt, ric, B * J))
            names = {"knot": "k_leg_knot", "condense": "k_leg_condense", "tail": "k_leg_condense_tail (condensation + the last leg's knots)",
                     "compose": "k_leg_compose (first level of the tree over the cuts)", "down": "k_leg_tree_down (last level)"}
        e.append((names["knot"], 512, lk, -(-(N - tail) // chunk) * B))
        e.append((names["tail"], 512, max(lc, lk), J * B) if tail > 0 else (names["condense"], 512, lc, (J - 1) * B))
        if tree:
            lev = _tree_levels(J)
            e.append((names["compose"], 512, lx, (lev[0] + 1) * B * 2))
            e.append((names["down"], 512, lx, (lev[-1] + 1) * B))
        else:
            e.append(("k_leg_consensus", 512, lx, B))
        # (one knot per workgroup: N x B workgroups are less than one round of the chip) ; the knots of the parametric legs
        e.append(("k_leg_apply", 256, 3 * n * 8 + (4 * 8 + 2 * 4 + 256 * 2), ((J - 1) * N // J) * B))
        e.append(("k_forward_phi (forward sweeps of the legs)", 512, 2 * n * 8, B * J))
    elif generic_riccati:
        sc = min(c, 48)
        e.append(("k_riccati_backward (serial sweep, no matrix cores)", 256, (n * n + m * m + sc * sc) * 8 + (c + 4) * 4, B))
    else:
        e.append(("k_riccati_mfma (serial sweep)", rt, ric, B))
    # (the step, three vectors of n, the partial sums, then three per-row scalars of the constraint block — four in the staged form)
    if "MPC_DUALS_PLAIN" in env:
        e.append(("k_duals<true> (MPC_DUALS_PLAIN)", 256, (nz + 3 * n + 16 + 3 * c) * 8, knots))
    else:
        e.append(("k_duals", 256, (nz + 3 * n + 16 + 4 * c) * 8, knots))
    e.append(("k_lagrangian", 64, 0, knots))
    return e


FULL, KINO, CENT = "fulldynamic", "kinodynamic", "centroidal"
CASES = {
    # full dynamics, complete model: the fixed-dimension kernels of model 1
    "full-legs1": (FULL, True, 1, {}),
    "full-legs2-chain": (FULL, True, 2, {"MPC_LEG_TAIL_KNOTS": 0}),  # the tree needs three legs
    "full-legs4-separate": (FULL, True, 4, {"MPC_LEG_TAIL_KNOTS": 0}),
    "full-legs4-fused": (FULL, True, 4, {"MPC_LEG_TAIL_KNOTS": WHOLE}),
    "full-legs4-chain": (FULL, True, 4, {"MPC_LEGS_CHAIN": 1, "MPC_LEG_TAIL_KNOTS": 0}),
    # ... with the generic kernels (sq sweep, MP = 32, NP = 80 ; ric_fixed == 0)
    "generic-legs1": (FULL, True, 1, {"MPC_HIP_GENERIC_DIMS": 1}),
    "generic-legs2-chain": (FULL, True, 2, {"MPC_HIP_GENERIC_DIMS": 1, "MPC_LEG_TAIL_KNOTS": 0}),
    "generic-legs4-separate": (FULL, True, 4, {"MPC_HIP_GENERIC_DIMS": 1, "MPC_LEG_TAIL_KNOTS": 0}),
    "generic-legs4-fused": (FULL, True, 4, {"MPC_HIP_GENERIC_DIMS": 1, "MPC_LEG_TAIL_KNOTS": WHOLE}),
    # the other fixed-dimension models ; the generic rows only they reach (MP = 48, NP = 64)
    "kino-legs4": (KINO, True, 4, {"MPC_LEG_TAIL_KNOTS": WHOLE}),
    "reduced-full-legs4": (FULL, False, 4, {"MPC_LEG_TAIL_KNOTS": 0}),
    "reduced-kino-legs4": (KINO, False, 4, {"MPC_LEG_TAIL_KNOTS": WHOLE}),
    "generic-kino-legs4": (KINO, True, 4, {"MPC_HIP_GENERIC_DIMS": 1, "MPC_LEG_TAIL_KNOTS": WHOLE}),
    "generic-reduced-legs4": (FULL, False, 4, {"MPC_HIP_GENERIC_DIMS": 1, "MPC_LEG_TAIL_KNOTS": 0}),
    "generic-reduced-legs4-chain": (FULL, False, 4, {"MPC_HIP_GENERIC_DIMS": 1, "MPC_LEGS_CHAIN": 1, "MPC_LEG_TAIL_KNOTS": 0}),
    # vector space: the small-problem sweeps, MP = NP = 16
    "centroidal-legs1": (CENT, False, 1, {}),
    "centroidal-legs4": (CENT, False, 4, {"MPC_LEG_TAIL_KNOTS": WHOLE}),
    "centroidal-legs4-chain": (CENT, False, 4, {"MPC_LEGS_CHAIN": 1, "MPC_LEG_TAIL_KNOTS": 0}),
    "generic-riccati": (FULL, True, 4, {"MPC_HIP_GENERIC_RICCATI": 1}),  # no matrix cores: no legs either
    "kino-legs1": (KINO, True, 1, {}),
    "plain-duals": (FULL, True, 4, {"MPC_DUALS_PLAIN": 1, "MPC_LEG_TAIL_KNOTS": 0}),  # k_duals<true>: three per-row scalars, not four
    # where the report was corrected (module docstring)
    "chunk3": (FULL, True, 4, {"MPC_LEG_KNOT_CHUNK": 3, "MPC_LEG_TAIL_KNOTS": 0}),  # 3 + 3 + 2 knots
    "legs3": (FULL, True, 3, {"MPC_LEG_TAIL_KNOTS": 0}),  # levels of 1 and 1 nodes
}


def _check_report(ens, legs, env, tag):
    info = ens.native.kernel_info()
    nj, contact_dyn = 0, False
    if ens.dims.space == K.SPACE_MULTIBODY:
        nj = ens.ctx.model.njoints - 1
        contact_dyn = any(int(desc[0]) == K.DYN_MULTIBODY_CONSTRAINT_SEMIEULER for desc, _ in ens.tables)
    want = _expected(ens.dims, legs, env, nj, contact_dyn)
    for name, k in info:
        print("%-24s %-90s threads %4d vgprs %3d lds %6d workgroups %4d" % (tag, name, k["threads"], k["vgprs"], k["dynamic_lds"], k["workgroups_per_launch"]))
    assert [name for name, _ in info] == [w[0] for w in want]
    for (name, k), (_, threads, lds, grid) in zip(info, want):
        assert k["threads"] == threads, (name, k)
        assert k["dynamic_lds"] == lds, (name, k, lds)
        assert k["workgroups_per_launch"] == grid, (name, k, grid)
    return [name for name, _ in info]


@pytest.mark.parametrize("case", list(CASES))
def test_report_names_the_instantiations_the_dimensions_call_for(hip_lib, monkeypatch, case):
    kind, complete, legs, env = CASES[case]
    ens = _handle(monkeypatch, hip_lib, kind, complete, legs, env)
    fixed = int(ens.native.debug_get("fixed_dims", 0)[0])
    if kind == CENT or "MPC_HIP_GENERIC_DIMS" in env or "MPC_HIP_GENERIC_RICCATI" in env:
        assert fixed == 0
    else:
        assert fixed == FIXED[(ens.dims.ndx, ens.dims.nu)][0]
    _check_report(ens, legs, env, case)


def _profiled_tick(ens):
    ens.cold_solve(max_iters=3)
    ens.native.profile(2)
    ens.native.profile(1)
    ens.step()
    ens.native.profile(0)
    return set(ens.native.profile_read())


COMMON_SLOTS = {"k_eval_stage", "k_lagrangian", "k_decide", "k_riccati_backward", "k_forward", "k_duals", "k_eval_stage_trial_values", "k_linesearch",
                "k_eval_stage_backtrack", "k_linesearch_backtrack", "k_accept", "k_after_step"}
LEG_SLOTS = {"k_closed_loop", "k_leg_condense", "k_leg_consensus", "k_leg_tree_down", "k_leg_apply"}


@pytest.mark.parametrize("case", ["full-legs4-fused", "generic-legs4-separate"])
def test_a_tick_launches_the_form_the_report_named(hip_lib, monkeypatch, case):
    kind, complete, legs, env = CASES[case]
    ens = _handle(monkeypatch, hip_lib, kind, complete, legs, env)
    names = _check_report(ens, legs, env, case)
    assert _profiled_tick(ens) == COMMON_SLOTS | LEG_SLOTS
    tail = ens.native.debug_get("leg_tail", 0)  # tail knots of the last pass, fused / separate condensation launches so far, sweeps of the last pass, legs
    back = ens.native.debug_get("backsubst", 0)  # knots per workgroup of the last k_leg_apply, its launches chunked / single, k_duals staged / plain, its workgroups along x
    fused = any(n.startswith("k_leg_condense_tail") for n in names)
    assert fused == (env["MPC_LEG_TAIL_KNOTS"] > 0) and int(tail[4]) == legs
    # every pass launched the condensation in the form the report names and never in the other: the first pass of the handle once per
    # level of the tree and once more (no guess at the cuts yet: 3 sweeps with 4 legs), every later pass (cold solve and tick) once
    multi, single = int(tail[6]), int(tail[7])
    passes = multi + single
    assert multi == 1 and single >= 3
    assert (int(tail[1]), int(tail[2])) == ((3 + single, 0) if fused else (0, 3 + single)) and int(tail[0]) == (2 if fused else 0) and int(tail[3]) == 1
    assert "k_duals" in names and (int(back[3]), int(back[4])) == (passes, 0)  # the staged form, once per pass
    assert (int(back[0]), int(back[1]), int(back[2])) == (1, 0, passes) and int(back[5]) == (legs - 1) * N // legs  # k_leg_apply as reported: one knot per workgroup


def test_the_plain_form_of_k_duals(hip_lib, monkeypatch):
    """MPC_DUALS_PLAIN=1: the report names k_duals<true> with its smaller carve-out, and every pass launches that form."""
    kind, complete, legs, env = CASES["plain-duals"]
    ens = _handle(monkeypatch, hip_lib, kind, complete, legs, env)
    names = _check_report(ens, legs, env, "plain-duals")
    assert "k_duals<true> (MPC_DUALS_PLAIN)" in names and "k_duals" not in names
    assert _profiled_tick(ens) == COMMON_SLOTS | LEG_SLOTS
    tail, back = ens.native.debug_get("leg_tail", 0), ens.native.debug_get("backsubst", 0)
    passes = int(tail[6]) + int(tail[7])
    assert passes >= 4 and (int(back[3]), int(back[4])) == (0, passes)  # staged / plain launches so far


def test_serial_forward_sweeps(hip_lib, monkeypatch):
    """One leg.  Full dynamics (m = 32): the knot-parallel forward sweep (k_closed_loop, then k_forward_phi<4,10>) by default on a small
    ensemble, k_forward_prefetch<4,10> with forward_mode = 1.  Kinodynamic (m = 44 > 32): k_forward_prefetch<6,10> whatever the mode.
    None launches a leg kernel."""
    for case, mode, extra in (("full-legs1", 0, {"k_closed_loop"}), ("full-legs1", 1, set()), ("kino-legs1", 0, set())):
        kind, complete, legs, env = CASES[case]
        ens = _handle(monkeypatch, hip_lib, kind, complete, legs, env)
        ens.options.forward_mode = mode
        ens.native.set_options(ens.options)
        assert _profiled_tick(ens) == COMMON_SLOTS | extra
        r = ens.results(gains=False)
        assert np.all(np.isfinite(r["xs"])) and np.all(np.isfinite(r["us"]))
        assert tuple(int(v) for v in ens.native.debug_get("leg_tail", 0)[:3]) == (0, 0, 0)
