"""The building blocks of mpc_benchmark_amd/csrc/mfma_blocks.h, each called alone through the probe libraries of tests/kernels/ and held
to an exact or a high-precision reference (tests/_mfma_reference.py, tests/_mfma_cases.py):

  (a) planted exact cases (unit lower triangular integer factors, distinct integer tile operands): tolerance zero;
  (b) cells a routine must not write come back with the bits they went in with (checked on EVERY launch of this file as well);
  (c) the "same bits" sentences of the header, tolerance zero, on random SPD blocks;
  (d) componentwise backward errors against longdouble: tile products within (K + 1) u, factorisations / block inverses / solves within
      16 x the worst figure of the float64 restatement of the same algorithm, rsqrt_refined within what one Newton step leaves of a
      24-bit seed;
  (e) the refusal flag on blocks that are not positive definite.

One test per group and build of the probe; every test hands whole case lists to a few launches.  A failure names the routine, the
size, the case index and the (row, column) of the worst entry."""
import numpy as np
import pytest

from tests import _mfma_accuracy as acc
from tests import _mfma_cases as cases
from tests import _mfma_probe as P
from tests import _mfma_reference as ref

pytestmark = pytest.mark.gpu

BUILDS = ("left", "right", "fused")
SEEDS = (1, 2, 3)


@pytest.fixture(scope="module", params=BUILDS)
def probe(request):
    return P.load(request.param)


def _run(probe, la, fails):
    """run one launch; cells outside its may-write mask must come back bit for bit (group (b), on every launch)"""
    la.run(probe)
    bad = la.touched()
    if len(bad):
        case, cell = bad[0]
        fails.append("%s: %d cell(s) written that the routine must not write, first: case %d, LDS word %d (bits %#x, were %#x)"
                     % (la.name, len(bad), case, cell, la.out.view(np.uint64)[case, cell], la.images.view(np.uint64)[case, cell]))
    return la


def _same(fails, routine, what, got, want):
    """tolerance zero: every entry equal (NaN counts as different); names the first and the worst entry"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (routine, what, got.shape, want.shape)
    neq = ~(got == want)
    if neq.any():
        idx = np.argwhere(neq)
        with np.errstate(invalid="ignore"):
            d = np.where(neq, np.abs(got - want), 0.0)
        d = np.where(np.isnan(d), np.inf, d)
        worst = np.unravel_index(int(np.argmax(d)), d.shape)
        fails.append("%s: %s: %d of %d entries differ; first at case %d (row %d, col %d); worst at case %d (row %d, col %d): got %r, want %r"
                     % (routine, what, len(idx), got.size, idx[0][0], idx[0][-2], idx[0][-1], worst[0], worst[-2], worst[-1], got[worst], want[worst]))


def _report(fails):
    assert not fails, "%d finding(s):\n" % len(fails) + "\n".join(fails)


def _planted(nb, n_real=None):
    cs = [cases.planted_factor(nb, seed=s, n_real=n_real) for s in SEEDS]
    return np.stack([c["A"] for c in cs]), np.stack([c["L0"] for c in cs]), np.stack([c["LI"] for c in cs]), cs


def _offdiag(L, nb):
    L = L.copy()
    for b in range(nb):
        L[:, 16 * b:16 * b + 16, 16 * b:16 * b + 16] = 0.0
    return L


def _chol16_forms(ncols):
    """every 16 x 16 form that takes a block whose rows / columns from ncols on are identity padding: (name, op, launch keywords)"""
    forms = [("chol16_wave(ncols=16)", P.CHOL16, dict(ncols=16)), ("chol16_wave_mfma(ncols=16)", P.CHOL16_MFMA, dict(ncols=16, scratch=True))]
    if ncols < 16:
        forms += [("chol16_wave(ncols=%d)" % ncols, P.CHOL16, dict(ncols=ncols)), ("chol16_wave_nc(ncols=%d)" % ncols, P.CHOL16_NC, dict(ncols=ncols)),
                  ("chol16_wave_mfma(ncols=%d)" % ncols, P.CHOL16_MFMA, dict(ncols=ncols, scratch=True))]
    forms += [("chol16_wave_n<%d>" % nc, op, {}) for nc, op in sorted(P.CHOL16_N.items()) if ncols <= nc]
    return forms


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------
def test_a_planted_exact_cases(probe):
    fails = []
    for la in cases.tile_product_launches(cases.distinct_integers):
        _run(probe, la, fails)
        As, B, C0s, neg, K = la.operands
        for i, (A, C0, C) in enumerate(zip(As, C0s, la.get_C())):
            _same(fails, la.name, "result tile %d" % i, C, ref.tile_product(C0, A, B, neg))
    for ncols in (16, 12, 8, 6, 4, 3, 1):
        A, L0, LI, _ = _planted(1, ncols if ncols < 16 else None)
        for name, op, kw in _chol16_forms(ncols):
            la = _run(probe, cases.chol16_launch(name + " [%d real columns]" % ncols, op, A, **kw), fails)
            _same(fails, la.name, "L", la.get_L(), L0)
            _same(fails, la.name, "L^-1", la.get_X(), LI[:, 0])
            la = _run(probe, cases.chol16_launch(name + " in place [%d real columns]" % ncols, op, A, inplace=True, **kw), fails)
            _same(fails, la.name, "L^-1", la.get_X(), LI[:, 0])
    for nb, n_real in cases.BLOCKED_SHAPES:
        A, L0, LI, _ = _planted(nb, n_real)
        tag = " nb=%d%s" % (nb, " n_real=%d" % n_real if n_real else "")
        for ld in (16 * nb + 1, 16 * nb + 8):
            runs = [("chol_blocked", P.CHOL_BLOCKED, 512, 1 << 20)]
            if nb <= 4:
                runs.append(("chol_blocked_wave", P.CHOL_BLOCKED_WAVE, 64, n_real or 1 << 20))
            for name, op, threads, nr in runs:
                la = _run(probe, cases.blocked_launch("%s%s ld=%d" % (name, tag, ld), op, threads, A, nb, ld, nr), fails)
                _same(fails, la.name, "L", la.get_L(), L0)
                _same(fails, la.name, "block inverses", la.get_LI(), LI)
        runs = [("chol_tiles", P.CHOL_TILES, 512)] + ([("chol_tiles_wave", P.CHOL_TILES_WAVE, 64)] if nb <= 4 else [])
        for name, op, threads in runs:
            la = _run(probe, cases.tiles_launch(name + tag, op, threads, A, nb), fails)
            _same(fails, la.name, "off-diagonal tiles of L", la.get_L(), _offdiag(L0, nb))
            _same(fails, la.name, "block inverses", la.get_LI(), LI)
        for transpose in (False, True):
            ops = (P.TRSM_BWD_BLOCKED, P.TRSM_BWD_TILES, "trsm_bwd") if transpose else (P.TRSM_FWD_BLOCKED, P.TRSM_FWD_TILES, "trsm_fwd")
            for ncb in (1, 3, 9):
                B, X0 = zip(*[cases.planted_rhs(c, ncb, 100 + s, transpose) for s, c in zip(SEEDS, _planted(nb, n_real)[3])])
                # (a sentinel column block behind B where the LDS has room for it: nb = 5 with nine column blocks fills it)
                ldbs = (16 * ncb + 1, 16 * ncb + 24) if not (nb == 5 and ncb == 9) else (16 * ncb + 1,)
                for ldb in ldbs:
                    for threads in (512, 64) if ncb == 1 else (512,):
                        what = "%s nb=%d ncb=%d ldb=%d, %d wavefront(s)" % (tag, nb, ncb, ldb, threads // 64)
                        la = _run(probe, cases.trsm_launch(ops[2] + "_blocked" + what, ops[0], threads, L0, LI, nb, np.stack(B), ncb, ldb,
                                                           ld=16 * nb + (1 if ldb == 16 * ncb + 1 else 8)), fails)
                        _same(fails, la.name, "X", la.get_X(), np.stack(X0))
                        la = _run(probe, cases.trsm_launch(ops[2] + "_tiles" + what, ops[1], threads, L0, LI, nb, np.stack(B), ncb, ldb), fails)
                        _same(fails, la.name, "X", la.get_X(), np.stack(X0))
    for nb, nlast in cases.NLAST_SHAPES:
        A, L0, LI, _ = _planted(nb, 16 * (nb - 1) + nlast)
        la = _run(probe, cases.tiles_launch("chol_tiles_wave_last<%d> nb=%d" % (nlast, nb), P.CHOL_TILES_LAST[nlast], 64, A, nb), fails)
        _same(fails, la.name, "off-diagonal tiles of L", la.get_L(), _offdiag(L0, nb))
        _same(fails, la.name, "block inverses", la.get_LI(), LI)
    _report(fails)


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------
def test_b_cells_a_routine_must_not_write(probe):
    """Strict upper triangles that are not stored, leading-dimension padding, column blocks beyond ncb, D when D == LIb: SENTINEL in,
    SENTINEL out.  (Every other test of this file applies the same check to its own launches; here: random SPD data, wide leading
    dimensions, and a look at the masks themselves so that the check cannot pass by allowing everything.)"""
    fails = []
    blocks, _ = cases.spd_batch(1, per_class=1)
    for name, op, kw in _chol16_forms(16):
        for ld in (17, 33):
            la = _run(probe, cases.chol16_launch("%s ld=%d" % (name, ld), op, blocks, ld=ld, **kw), fails)
            assert la.may_write.sum() <= 136 + 256 + 7 and np.isnan(la.out[:, ~la.may_write]).all()
        la = _run(probe, cases.chol16_launch(name + " in place", op, blocks, inplace=True, **kw), fails)
        assert la.may_write.sum() <= 256 + 7 and not la.may_write[271]
    for nb in (3, 5):
        mats, _ = cases.spd_batch(nb, per_class=1)
        ld = 16 * nb + 8
        for name, op, threads in (("chol_blocked_wave", P.CHOL_BLOCKED_WAVE, 64), ("chol_blocked", P.CHOL_BLOCKED, 512)):
            la = _run(probe, cases.blocked_launch("%s nb=%d ld=%d" % (name, nb, ld), op, threads, mats, nb, ld), fails)
            assert (~la.may_write).sum() >= 16 * nb * 8 + 128 * nb * (nb - 1) + nb * 16
            L, LI = la.get_L(), la.get_LI()
        for name, op, threads in (("chol_tiles_wave", P.CHOL_TILES_WAVE, 64), ("chol_tiles", P.CHOL_TILES, 512)):
            la = _run(probe, cases.tiles_launch("%s nb=%d" % (name, nb), op, threads, mats, nb), fails)
            assert (~la.may_write).sum() == 16 * nb * (nb + 1) // 2
        B = cases.mixed_magnitudes(np.random.default_rng(4), (len(mats), 16 * nb, 32))
        for name, op, tl in (("trsm_fwd_blocked", P.TRSM_FWD_BLOCKED, False), ("trsm_bwd_blocked", P.TRSM_BWD_BLOCKED, False),
                             ("trsm_fwd_tiles", P.TRSM_FWD_TILES, True), ("trsm_bwd_tiles", P.TRSM_BWD_TILES, True)):
            la = _run(probe, cases.trsm_launch("%s nb=%d ncb=2 of 3" % (name, nb), op, 512, L, LI, nb, B, 2, 49, ld=None if tl else ld), fails)
            assert la.may_write.sum() == 16 * nb * 32 and np.isfinite(la.get_X()).all()
    _report(fails)


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------
def _spd_blocks(ncols=16):
    return cases.spd_batch(1, n_real=ncols if ncols < 16 else None, per_class=1, seed=23)[0]


def test_c_left_right_and_fused_inverse_are_the_same_bits():
    """header: "Each x[R] receives its terms in the order K = 0, 1, ...: the same bits" (right-looking) and "Same additions in the same
    order as InvCol / CholStep: the same bits" (fused) — three builds of the same source"""
    fails = []
    blocks = _spd_blocks()
    res = {}
    for build in BUILDS:
        la = _run(P.load(build), cases.chol16_launch("chol16_wave, %s build" % build, P.CHOL16, blocks), fails)
        res[build] = (la.get_L(), la.get_X())
    for build in ("right", "fused"):
        _same(fails, "chol16_wave", "L, %s-looking build against the left-looking one" % build, res[build][0], res["left"][0])
        _same(fails, "chol16_wave", "L^-1, %s build against the left-looking one" % build, res[build][1], res["left"][1])
    _report(fails)


def test_c_same_bits_claims_of_the_header(probe):
    fails = []
    eye = np.eye(16)
    for ncols in range(1, 17):
        blocks = _spd_blocks(ncols)
        full = _run(probe, cases.chol16_launch("chol16_wave(ncols=16) [%d real columns]" % ncols, P.CHOL16, blocks), fails)
        Lf, Xf = full.get_L(), full.get_X()
        forms = [("chol16_wave(ncols=%d)" % ncols, P.CHOL16, dict(ncols=ncols)), ("chol16_wave_nc(ncols=%d)" % ncols, P.CHOL16_NC, dict(ncols=ncols))]
        forms += [("chol16_wave_n<%d> [%d real columns]" % (nc, ncols), op, {}) for nc, op in sorted(P.CHOL16_N.items()) if ncols <= nc]
        for name, op, kw in forms:
            la = _run(probe, cases.chol16_launch(name, op, blocks, **kw), fails)
            _same(fails, name, "L on the leading %d rows and columns against the full form" % ncols, la.get_L()[:, :ncols, :ncols], Lf[:, :ncols, :ncols])
            _same(fails, name, "L^-1 on the leading %d rows and columns against the full form" % ncols, la.get_X()[:, :ncols, :ncols], Xf[:, :ncols, :ncols])
            _same(fails, name, "padding rows of L^-1 (unit rows)", la.get_X()[:, ncols:, :], np.broadcast_to(eye[ncols:], (len(blocks), 16 - ncols, 16)))
        mf16 = _run(probe, cases.chol16_launch("chol16_wave_mfma(ncols=16) [%d real columns]" % ncols, P.CHOL16_MFMA, blocks, ncols=16, scratch=True), fails)
        mf = _run(probe, cases.chol16_launch("chol16_wave_mfma(ncols=%d)" % ncols, P.CHOL16_MFMA, blocks, ncols=ncols, scratch=True), fails)
        _same(fails, mf.name, "L against ncols = 16 on the same padded block", mf.get_L(), mf16.get_L())
        _same(fails, mf.name, "L^-1 against ncols = 16 on the same padded block", mf.get_X(), mf16.get_X())
        _same(fails, mf.name, "padding rows of L^-1 (unit rows)", mf.get_X()[:, ncols:, :], np.broadcast_to(eye[ncols:], (len(blocks), 16 - ncols, 16)))
        mfi = _run(probe, cases.chol16_launch("chol16_wave_mfma(ncols=%d) in place" % ncols, P.CHOL16_MFMA, blocks, ncols=ncols, inplace=True, scratch=True), fails)
        _same(fails, mfi.name, "L^-1 in place (D == LIb, ld 17) against separate buffers (ld 33)", mfi.get_X(), mf.get_X())
    mats = cases.spd_batch(4, per_class=1, seed=29)[0]
    one = _run(probe, cases.tiles_launch("chol_tiles_wave nb=4", P.CHOL_TILES_WAVE, 64, mats, 4), fails)
    wg = _run(probe, cases.tiles_launch("chol_tiles nb=4 (512 threads)", P.CHOL_TILES, 512, mats, 4), fails)
    _same(fails, wg.name, "off-diagonal tiles against chol_tiles_wave", wg.get_L(), one.get_L())
    _same(fails, wg.name, "block inverses against chol_tiles_wave", wg.get_LI(), one.get_LI())
    one = _run(probe, cases.blocked_launch("chol_blocked_wave nb=4", P.CHOL_BLOCKED_WAVE, 64, mats, 4, 65), fails)
    wg = _run(probe, cases.blocked_launch("chol_blocked nb=4 (512 threads)", P.CHOL_BLOCKED, 512, mats, 4, 65), fails)
    _same(fails, wg.name, "L against chol_blocked_wave", wg.get_L(), one.get_L())
    _same(fails, wg.name, "block inverses against chol_blocked_wave", wg.get_LI(), one.get_LI())
    _report(fails)


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------
RSQRT_BOUND = 1.5 * 2.0 ** -48 / ref.U + 4.0   # = 52 u: one Newton step squares the seed's error (3/2 e^2, e <= 2^-24) and adds four roundings


def test_d_accuracy_against_longdouble(probe):
    """Device figures against FACTOR x the float64 restatement's (tests/_mfma_accuracy.py; the measured values: profiles/mfma_blocks_reference.txt)."""
    fails = []
    backend = acc.DeviceBackend(probe)
    records = acc.measure(backend)
    for la in backend.launches:
        if len(la.touched()):
            fails.append("%s: wrote cells it must not write (see test_b)" % la.name)
    bounds = acc.bounds()
    worst = {}
    for r in records:
        key = (r["routine"], r["size"], r["metric"])
        if key not in worst or r["value"] > worst[key]["value"]:
            worst[key] = r
    print(acc.format_table("device, %s build" % probe.form.decode(), acc.table(records, key="routine")))
    for key, r in sorted(worst.items()):
        bound = bounds[(r["family"], r["size"], r["metric"])]
        if not r["value"] <= bound:
            fails.append("%s n=%d %s: %.2f u > %.2f u (= %g x the float64 restatement '%s'); worst: %s, case %d, entry (row %d, col %d)"
                         % (key + (r["value"], bound, acc.FACTOR, r["family"], cases.class_name(*cases.spd_classes()[r["cls"]]), r["case"]) + tuple(r["where"])))
    for la in cases.tile_product_launches(cases.mixed_magnitudes):
        _run(probe, la, fails)
        As, B, C0s, neg, K = la.operands
        for i, (A, C0, C) in enumerate(zip(As, C0s, la.get_C())):
            vals = [ref.tile_metric(c, c0, a, b, neg) for c, c0, a, b in zip(C, C0, A, B)]
            case = int(np.argmax([v[0] for v in vals]))
            if not vals[case][0] <= K + 1:
                fails.append("%s, result tile %d: %.2f u > (K + 1) u = %d u; case %d, entry (row %d, col %d)" % ((la.name, i, vals[case][0], K + 1, case) + tuple(vals[case][1])))
    piv, ks = acc.rsqrt_pivots()
    err = ref.rsqrt_relative_error(piv, probe.rsqrt_refined(piv))
    print("rsqrt_refined: worst relative error %.3f u at %.17g" % (err.max(), piv[int(np.argmax(err))]))
    if not err.max() <= RSQRT_BOUND:
        fails.append("rsqrt_refined: relative error %.3f u > %.1f u at pivot %.17g" % (err.max(), RSQRT_BOUND, piv[int(np.argmax(err))]))
    p4 = probe.rsqrt_refined(4.0 ** ks)
    if not np.array_equal(p4, 2.0 ** -ks):
        k = ks[int(np.argmax(p4 != 2.0 ** -ks))]
        fails.append("rsqrt_refined(4^%d) = %r, not exactly 2^%d: the planted cases of (a) rest on this" % (k, p4[int(np.argmax(p4 != 2.0 ** -ks))], -k))
    _report(fails)


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------
def _flags(fails, la, listed):
    for i, (label, _, want, _) in enumerate(listed):
        if bool(la.flags[i]) != want:
            fails.append("%s: returned %s for case %d (%s), expected %s" % (la.name, bool(la.flags[i]), i, label, want))


def test_e_refusal_flag(probe):
    fails = []
    for ncols in (16, 12, 6, 3):
        listed = cases.refusal_blocks(ncols)
        blocks = np.stack([b for _, b, _, _ in listed])
        for name, op, kw in _chol16_forms(ncols):
            _flags(fails, _run(probe, cases.chol16_launch(name + " [%d real columns]" % ncols, op, blocks, **kw), fails), listed)
            _flags(fails, _run(probe, cases.chol16_launch(name + " in place [%d real columns]" % ncols, op, blocks, inplace=True, **kw), fails), listed)
    for nb in (3, 5):
        listed = cases.refusal_blocked(nb)
        mats = np.stack([m for _, m, _, _ in listed])
        ld = 16 * nb + 1
        path = "one-wavefront path" if nb <= 3 else "workgroup path"
        _flags(fails, _run(probe, cases.blocked_launch("chol_blocked nb=%d (%s)" % (nb, path), P.CHOL_BLOCKED, 512, mats, nb, ld), fails), listed)
        _flags(fails, _run(probe, cases.tiles_launch("chol_tiles nb=%d (%s)" % (nb, path), P.CHOL_TILES, 512, mats, nb), fails), listed)
        if nb <= 3:
            _flags(fails, _run(probe, cases.blocked_launch("chol_blocked_wave nb=%d" % nb, P.CHOL_BLOCKED_WAVE, 64, mats, nb, ld), fails), listed)
            _flags(fails, _run(probe, cases.tiles_launch("chol_tiles_wave nb=%d" % nb, P.CHOL_TILES_WAVE, 64, mats, nb), fails), listed)
    _report(fails)
