"""Case generators and LDS images for the tests of mfma_blocks.h (plain numpy; nothing here reads csrc/).

An LDS image is one flat float64 vector per case.  Cells no operand occupies hold SENTINEL, a NaN with a distinctive payload, and every
launch carries a mask of the cells its routine may write: everything else has to come back with the bits it went in with."""
import functools
from fractions import Fraction

import numpy as np

from tests import _mfma_probe as P
from tests import _mfma_reference as ref

SENTINEL_BITS = np.uint64(0x7FF8C0DEFACE5A5A)
EXACT_LIMIT = 2.0 ** 50
CONDITIONS = (1.0, 1e3, 1e6, 1e9, 1e12)
TILE_KS = (4, 12, 16, 20, 32, 36, 48, 80)


# ---- images -----------------------------------------------------------------------------------------------------------------------
def sentinel_images(ncases, words):
    img = np.empty((ncases, words), dtype=np.uint64)
    img[:] = SENTINEL_BITS
    return img.view(np.float64)


def cells(off, rows, cols, rs, cs=1):
    """flat indices of element (r, c) at off + r * rs + c * cs"""
    return off + np.arange(rows)[:, None] * rs + np.arange(cols)[None, :] * cs


TRIL16 = np.tril(np.ones((16, 16), dtype=bool))


class Launch:
    """one call of the probe: a routine, its launch shape and parameters, the images of all its cases and the cells it may write"""

    def __init__(self, name, op, threads, params, images, may_write):
        self.name, self.op, self.threads, self.params = name, op, threads, [int(v) for v in params]
        self.images, self.may_write = images, may_write
        self.out = self.flags = None
        assert images.shape[1] == may_write.size and images.shape[1] <= P.MAX_WORDS, (name, images.shape)

    def run(self, probe):
        self.out, self.flags = probe.run(self.op, self.threads, self.params, self.images)
        return self

    def touched(self):
        """(case, cell) of every cell outside may_write whose bits changed"""
        diff = (self.out.view(np.uint64) != self.images.view(np.uint64)) & ~self.may_write[None, :]
        return np.argwhere(diff)


def chol16_launch(name, op, blocks, ncols=16, ld=33, inplace=False, scratch=False):
    """16 x 16 forms: D (lower triangle, strict upper = SENTINEL) at 0 with leading dimension ld, LIb (ld 17) behind it — or on top of
    it (inplace: D == LIb, ld 17).  scratch: the routine may use the first 128 doubles of LIb (chol16_wave_mfma)."""
    blocks = np.asarray(blocks, dtype=np.float64)
    if inplace:
        ld, li, words = 17, 0, 272
    else:
        li, words = 16 * ld, 16 * ld + 272
    img = sentinel_images(len(blocks), words)
    d_idx, x_idx = cells(0, 16, 16, ld), cells(li, 16, 16, 17)
    img[:, d_idx[TRIL16]] = blocks[:, TRIL16]
    may = np.zeros(words, dtype=bool)
    may[x_idx] = True
    if not inplace:
        may[d_idx[TRIL16]] = True
    if scratch:
        may[li:li + 128] = True
    la = Launch(name, op, 64, [0, ld, li, ncols], img, may)
    la.get_L = lambda: np.where(TRIL16, la.out[:, d_idx], 0.0)
    la.get_X = lambda: la.out[:, x_idx]
    return la


def _block_lower_put(img, idx, mats, nb):
    """lower triangle of mats (elementwise) into the cells idx; the strict upper triangle keeps SENTINEL"""
    low = np.tril(np.ones((16 * nb, 16 * nb), dtype=bool))
    img[:, idx[low]] = mats[:, low]


def blocked_launch(name, op, threads, mats, nb, ld, n_real=1 << 20):
    """square layout: A (16 nb x 16 nb, leading dimension ld) at 0, LI (nb x 272) behind it"""
    mats = np.asarray(mats, dtype=np.float64)
    n = 16 * nb
    li, words = n * ld, n * ld + nb * 272
    img = sentinel_images(len(mats), words)
    a_idx = cells(0, n, n, ld)
    _block_lower_put(img, a_idx, mats, nb)
    may = np.zeros(words, dtype=bool)
    for bi in range(nb):
        for bj in range(bi + 1):
            t = a_idx[16 * bi:16 * bi + 16, 16 * bj:16 * bj + 16]
            may[t[TRIL16] if bi == 0 else t] = True   # (diagonal tiles after the first take a full-tile trailing update)
        may[cells(li + 272 * bi, 16, 16, 17)] = True
    la = Launch(name, op, threads, [0, ld, nb, li, n_real], img, may)
    la.get_L = lambda: np.tril(la.out[:, a_idx])
    la.get_LI = lambda: np.stack([la.out[:, cells(li + 272 * b, 16, 16, 17)] for b in range(nb)], axis=1)
    return la


def tile_off(bi, bj):
    return (bi * (bi + 1) // 2 + bj) * 272


def pack_tiles(img, t0, nb, offdiag=None, diag=None):
    """tile-packed lower block triangle at t0: off-diagonal tiles from the matrix offdiag, diagonal tiles from diag[:, bi] (16 x 16,
    or None: the lower triangle of offdiag's diagonal block, strict upper = SENTINEL)"""
    for bi in range(nb):
        for bj in range(bi + 1):
            idx = cells(t0 + tile_off(bi, bj), 16, 16, 17)
            blk = offdiag[:, 16 * bi:16 * bi + 16, 16 * bj:16 * bj + 16]
            if bi != bj:
                img[:, idx] = blk
            elif diag is not None:
                img[:, idx] = diag[:, bi]
            else:
                img[:, idx[TRIL16]] = blk[:, TRIL16]


def tiles_launch(name, op, threads, mats, nb):
    mats = np.asarray(mats, dtype=np.float64)
    words = tile_off(nb, 0)
    img = sentinel_images(len(mats), words)
    pack_tiles(img, 0, nb, offdiag=mats)
    may = np.zeros(words, dtype=bool)
    for bi in range(nb):
        for bj in range(bi + 1):
            may[cells(tile_off(bi, bj), 16, 16, 17)] = True
    la = Launch(name, op, threads, [0, nb], img, may)

    def get_L():  # off-diagonal blocks of L (the diagonal blocks are not kept: zero here)
        L = np.zeros((len(mats), 16 * nb, 16 * nb))
        for bi in range(nb):
            for bj in range(bi):
                L[:, 16 * bi:16 * bi + 16, 16 * bj:16 * bj + 16] = la.out[:, cells(tile_off(bi, bj), 16, 16, 17)]
        return L
    la.get_L = get_L
    la.get_LI = lambda: np.stack([la.out[:, cells(tile_off(b, b), 16, 16, 17)] for b in range(nb)], axis=1)
    return la


def trsm_launch(name, op, threads, L, LI, nb, B, ncb, ldb, ld=None):
    """solves: the factor (square layout with leading dimension ld, or tile-packed when ld is None), then B (16 nb rows, leading
    dimension ldb >= 16 ncb + 1).  The diagonal blocks of the square L stay SENTINEL (the solves use the block inverses only), and so
    does every column of B from 16 ncb on."""
    L, LI, B = (np.asarray(v, dtype=np.float64) for v in (L, LI, B))
    n = 16 * nb
    assert B.shape[1:] == (n, 16 * ncb) and ldb >= 16 * ncb + 1
    if ld is None:
        b0 = tile_off(nb, 0)
    else:
        li0 = n * ld
        b0 = li0 + nb * 272
    words = b0 + n * ldb
    img = sentinel_images(len(L), words)
    if ld is None:
        pack_tiles(img, 0, nb, offdiag=L, diag=LI)
        params = [0, nb, b0, ldb, ncb]
    else:
        l_idx = cells(0, n, n, ld)
        for bi in range(nb):
            for bj in range(bi):
                img[:, l_idx[16 * bi:16 * bi + 16, 16 * bj:16 * bj + 16]] = L[:, 16 * bi:16 * bi + 16, 16 * bj:16 * bj + 16]
            img[:, cells(li0 + 272 * bi, 16, 16, 17)] = LI[:, bi]
        params = [0, ld, li0, nb, b0, ldb, ncb]
    b_idx = cells(b0, n, 16 * ncb, ldb)
    img[:, b_idx] = B
    may = np.zeros(words, dtype=bool)
    may[b_idx] = True
    la = Launch(name, op, threads, params, img, may)
    la.get_X = lambda: la.out[:, b_idx]
    return la


class _Regions:
    def __init__(self):
        self.words = 0

    def add(self, size):
        off, self.words = self.words, self.words + size
        return off


def _operand(reg, rows, cols, transposed):
    """a rows x cols operand with one padding column: row-major, or stored transposed -> (offset, row stride, column stride, size)"""
    if transposed:
        return reg.add(cols * (rows + 1)), 1, rows + 1
    return reg.add(rows * (cols + 1)), cols + 1, 1


def mma_launch(name, op, As, a_t, B, b_t, C0s, neg=False, b_in_registers=False):
    """tile products: As = list of A operands (ncases, 16, K) with their orientation flags a_t, B (ncases, K, 16), C0s = the accumulators
    on entry, one per A.  -> Launch with get_C() -> list of results"""
    K = B.shape[1]
    reg = _Regions()
    a_loc = [_operand(reg, 16, K, t) for t in a_t]
    b_loc = _operand(reg, K, 16, b_t) if not b_in_registers else (reg.add(272), 17, 1)
    c_off = [reg.add(272) for _ in C0s]
    img = sentinel_images(len(B), reg.words)
    for A, (off, rs, cs) in zip(As, a_loc):
        img[:, cells(off, 16, K, rs, cs)] = A
    img[:, cells(b_loc[0], K, 16, b_loc[1], b_loc[2])] = B
    may = np.zeros(reg.words, dtype=bool)
    c_idx = [cells(off, 16, 16, 17) for off in c_off]
    for C0, idx in zip(C0s, c_idx):
        img[:, idx] = C0
        may[idx] = True
    (a0, a0_is, a0_ks), (b, b_ks, b_js) = a_loc[0], b_loc
    if op == P.MMA_TILE:
        params = [int(neg), a0, a0_is, a0_ks, b, b_ks, b_js, K, c_off[0], 17]
    elif op == P.MMA_TILE2:
        assert a_t[0] == a_t[1]
        params = [a0, a_loc[1][0], a0_is, a0_ks, b, b_ks, b_js, K, c_off[0], c_off[1], 17]
    elif op == P.MMA_TILE_2A:
        a1, a1_is, a1_ks = a_loc[1]
        params = [a0, a0_is, a0_ks, a1, a1_is, a1_ks, b, b_ks, b_js, K, c_off[0], c_off[1], 17]
    else:
        assert op == P.MMA_TILE_RB and K == 16
        params = [int(neg), a0, a0_is, a0_ks, b, 17, c_off[0], 17]
    la = Launch(name, op, 64, params, img, may)
    la.get_C = lambda: [la.out[:, idx] for idx in c_idx]
    la.operands = (As, B, C0s, neg, K)
    return la


def tile_product_launches(make, ncases=2):
    """Every tile-product configuration the tests cover.  make(rng, shape) draws one operand."""
    rng = np.random.default_rng(20240521)
    out = []

    def ops(K, n_a):
        return ([make(rng, (ncases, 16, K)) for _ in range(n_a)], make(rng, (ncases, K, 16)), [make(rng, (ncases, 16, 16)) for _ in range(n_a)])
    for K in TILE_KS:
        for neg in (False, True):
            for a_t in (False, True):
                for b_t in (False, True):
                    As, B, C0s = ops(K, 1)
                    out.append(mma_launch("mma_tile<%s> K=%d A%s B%s" % ("true" if neg else "false", K, "^T" if a_t else "", "^T" if b_t else ""),
                                          P.MMA_TILE, As, [a_t], B, b_t, C0s, neg=neg))
    for K in (8, 16, 80):
        for a_t in (False, True):
            As, B, C0s = ops(K, 2)
            out.append(mma_launch("mma_tile2 K=%d A%s" % (K, "^T" if a_t else ""), P.MMA_TILE2, As, [a_t, a_t], B, not a_t, C0s))
    for K in TILE_KS:
        for a_t in ((False, True), (True, False)):
            As, B, C0s = ops(K, 2)
            out.append(mma_launch("mma_tile_2a K=%d A0%s A1%s" % (K, "^T" if a_t[0] else "", "^T" if a_t[1] else ""),
                                  P.MMA_TILE_2A, As, list(a_t), B, K % 8 == 0, C0s))
    for neg in (False, True):
        for a_t in (False, True):   # (17, 1): trsm_fwd_tiles; (1, 17): trsm_bwd_tiles
            As, B, C0s = ops(16, 1)
            out.append(mma_launch("mma_tile_rb<%s> A%s" % ("true" if neg else "false", "^T" if a_t else ""),
                                  P.MMA_TILE_RB, As, [a_t], B, False, C0s, neg=neg, b_in_registers=True))
    return out


def distinct_integers(rng, shape):
    """integer operands, every entry of one operand different in magnitude, random signs (products stay far below 2^53)"""
    n = int(np.prod(shape[1:]))
    v = np.stack([rng.permutation(n) + 1 for _ in range(shape[0])]).reshape(shape).astype(np.float64)
    return v * rng.choice([-1.0, 1.0], size=shape)


def mixed_magnitudes(rng, shape):
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, size=shape)


# ---- (a) planted exact cases ------------------------------------------------------------------------------------------------------
def _comparison_inverse(Labs):
    """entrywise bound of every partial sum of the inverse of a unit lower triangular block: the inverse of its comparison matrix"""
    n = Labs.shape[0]
    N = np.eye(n)
    for r in range(n):
        N[r, :] += Labs[r, :r] @ N[:r, :]
    return N


@functools.lru_cache(maxsize=None)
def planted_factor(nb, seed, n_real=None):
    """L0 unit lower triangular with entries in {-1, 0, 1} (identity from n_real on), thinned until the factorisation of A = L0 L0^T,
    the 16 x 16 block inverses and the blocked solves are exact in float64 with every intermediate below 2^50.
    -> dict(A, L0, LI (nb, 16, 16), bound)"""
    rng = np.random.default_rng(seed)
    n = 16 * nb
    n_real = n if n_real is None else n_real
    density = 0.5
    while True:
        L0 = np.tril(rng.choice([-1.0, 0.0, 1.0], size=(n, n), p=[density / 2, 1 - density, density / 2]), -1) + np.eye(n)
        L0[n_real:, :] = np.eye(n)[n_real:, :]
        La = np.abs(L0)
        Ns = [_comparison_inverse(La[16 * b:16 * b + 16, 16 * b:16 * b + 16]) for b in range(nb)]
        # majorants: trailing updates |A| + |L| |L|^T, panel products with the block inverses, W = I - L X of the panel form
        gram = La @ La.T
        bound = 16.0 * (1.0 + 2.0 * gram.max()) * (1.0 + max(N.max() for N in Ns)) ** 2
        # forward / backward solves against a right-hand side of unit size, in absolute values
        Xf = np.ones((n, 1))
        for b in range(nb):
            r0 = 16 * b
            Xf[r0:r0 + 16] = Ns[b] @ (Xf[r0:r0 + 16] + La[r0:r0 + 16, :r0] @ Xf[:r0])
        Xb = np.ones((n, 1))
        for b in range(nb - 1, -1, -1):
            r0 = 16 * b
            Xb[r0:r0 + 16] = Ns[b].T @ (Xb[r0:r0 + 16] + La[r0 + 16:, r0:r0 + 16].T @ Xb[r0 + 16:])
        solve_bound = max(Xf.max(), Xb.max())
        if max(bound, solve_bound * 2.0 ** 12) < EXACT_LIMIT:   # (2^12: room for the planted right-hand sides, |B| <= 2^12)
            A = L0 @ L0.T
            LI = np.stack([np.linalg.inv(L0[16 * b:16 * b + 16, 16 * b:16 * b + 16]).round() for b in range(nb)])
            ok = all(np.array_equal(LI[b] @ L0[16 * b:16 * b + 16, 16 * b:16 * b + 16], np.eye(16)) for b in range(nb))
            for form in (ref.chol16_register, ref.chol16_panels):
                L, X = ref.chol_blocked(A, nb, n_real=n_real, chol16=form)
                ok = ok and np.array_equal(L, L0) and np.array_equal(np.stack(X), LI)
            if ok:
                return dict(A=A, L0=L0, LI=LI, nb=nb, n_real=n_real, bound=bound, solve_bound=solve_bound, density=density)
        density *= 0.8
        assert density > 1e-3, "no exact planted factor found"


def planted_rhs(case, ncb, seed, transpose):
    """B = L0 X0 (or L0^T X0) with planted integer X0, |X0| <= 3 -> (B, X0)"""
    rng = np.random.default_rng(seed)
    X0 = rng.integers(-3, 4, size=(16 * case["nb"], 16 * ncb)).astype(np.float64)
    B = (case["L0"].T if transpose else case["L0"]) @ X0
    assert np.abs(B).max() <= 2.0 ** 12
    return B, X0


def planted_exact_in_fractions(case):
    """the exact evaluation: factorisation, block inverses and both solves in Fraction agree with the float64 ones entry by entry"""
    A, nb = ref.to_fraction(case["A"]), case["nb"]
    for form in (ref.chol16_register, ref.chol16_panels):
        L, X = ref.chol_blocked(A, nb, n_real=case["n_real"], chol16=form)
        Lf, Xf = ref.chol_blocked(case["A"], nb, n_real=case["n_real"], chol16=form)
        assert all(L[i] == Fraction(float(Lf[i])) for i in np.ndindex(L.shape)), "factor"
        for b in range(nb):
            assert all(X[b][i] == Fraction(float(Xf[b][i])) for i in np.ndindex(16, 16)), "inverse"
    for transpose in (False, True):
        B, X0 = planted_rhs(case, 1, 7, transpose)
        solve = ref.trsm_bwd if transpose else ref.trsm_fwd
        Xq = solve(L, X, nb, ref.to_fraction(B))
        Xd = solve(case["L0"], list(case["LI"]), nb, B)
        assert all(Xq[i] == Fraction(float(Xd[i])) for i in np.ndindex(Xq.shape)) and np.array_equal(Xd, X0), "solve"
    return True


# blocked shapes of (a) and (d): (nb, n_real or None)
BLOCKED_SHAPES = ((1, None), (2, None), (3, None), (3, 38), (4, None), (5, None))
NLAST_SHAPES = ((3, 6), (3, 12), (1, 6), (2, 12))   # (nb, NLAST): chol16_wave_n<NLAST> on the last diagonal tile


# ---- (c), (d) random SPD matrices -------------------------------------------------------------------------------------------------
def spd(n, cond, scaled, rng, n_real=None):
    """symmetric positive definite with eigenvalues log-spaced over [1 / cond, 1]; scaled: D A D with D = 10^U(-3, 3); identity from n_real on"""
    m = n if n_real is None else n_real
    q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    lam = np.logspace(0.0, -np.log10(cond), m) if m > 1 else np.ones(1)
    a = (q * lam) @ q.T
    a = 0.5 * (a + a.T)
    if scaled:
        s = 10.0 ** rng.uniform(-3, 3, size=m)
        a = a * s[:, None] * s[None, :]
    out = np.eye(n)
    out[:m, :m] = a
    return out


def spd_classes():
    return [(cond, scaled) for cond in CONDITIONS for scaled in (False, True)]


def class_name(cond, scaled):
    return "cond %.0e%s" % (cond, " scaled" if scaled else "")


def spd_batch(nb, n_real=None, per_class=2, seed=11):
    """-> (matrices (ncases, 16 nb, 16 nb), class index per case)"""
    rng = np.random.default_rng(seed + 1000 * nb + (n_real or 0))
    mats, cls = [], []
    for ci, (cond, scaled) in enumerate(spd_classes()):
        for _ in range(per_class):
            mats.append(spd(16 * nb, cond, scaled, rng, n_real))
            cls.append(ci)
    return np.stack(mats), np.array(cls)


# ---- (e) blocks that are not positive definite -------------------------------------------------------------------------------------
def pivots_longdouble(A, upto):
    """the pivots 0 .. upto of the right-looking elimination of A (lower triangle), in longdouble"""
    a = np.asarray(ref.mirror_lower(A), dtype=np.longdouble).copy()
    piv = []
    for j in range(upto + 1):
        piv.append(a[j, j])
        if j < upto:
            a[j + 1:, j + 1:] -= np.outer(a[j + 1:, j], a[j + 1:, j]) / a[j, j]
    return np.array(piv)


def indefinite(n, at, rng, n_real=None):
    """L diag(s) L^T with L from a well-conditioned SPD matrix and s = -1 at `at`, +1 elsewhere: the pivots before `at` are those of
    L L^T, the pivot at `at` is -L[at][at]^2"""
    L = np.linalg.cholesky(spd(n, 10.0, False, rng, n_real))
    s = np.ones(n)
    s[at] = -1.0
    a = (L * s) @ L.T
    return 0.5 * (a + a.T)


def pivot_margin(A, at):
    """(deciding pivot, smallest earlier pivot) over the scale of A (its largest diagonal entry in magnitude), from the longdouble elimination"""
    piv = pivots_longdouble(A, at)
    scale = np.abs(np.diag(A)).max()
    return float(piv[at] / scale), float(piv[:at].min() / scale) if at else 1.0


def refusal_blocks(ncols=16, seed=5):
    """single 16 x 16 blocks with ncols real columns.  -> list of (label, block, expected flag, deciding position or None)"""
    rng = np.random.default_rng(seed + ncols)
    out = [("positive definite", spd(16, 100.0, False, rng, ncols), True, None), ("positive definite, condition 1e3", spd(16, 1e3, False, rng, ncols), True, None)]
    for j in range(ncols):
        out.append(("negative pivot at %d" % j, indefinite(16, j, rng, ncols), False, j))
    for j in range(ncols):
        for what, v in (("NaN", np.nan), ("+Inf", np.inf), ("-Inf", -np.inf)):
            a = spd(16, 100.0, False, rng, ncols)
            a[j, j] = v
            out.append(("%s on the diagonal at %d" % (what, j), a, False, None))
    for (r, c) in ((1, 0), (ncols - 1, 0), (ncols - 1, ncols - 2), ((ncols + 1) // 2, (ncols - 1) // 2)):
        if not 0 <= c < r < ncols:
            continue
        for what, v in (("NaN", np.nan), ("+Inf", np.inf), ("-Inf", -np.inf)):
            a = spd(16, 100.0, False, rng, ncols)
            a[r, c] = a[c, r] = v
            out.append(("%s off the diagonal at (%d, %d)" % (what, r, c), a, False, None))
    return out


def refusal_blocked(nb, seed=9):
    """(16 nb) x (16 nb) matrices whose diagonal block kb meets a negative pivot at each of its 16 positions, a NaN / Inf on its diagonal or
    below it, for every kb; and positive definite ones.  -> list of (label, matrix, expected flag, deciding global position or None)"""
    rng = np.random.default_rng(seed + nb)
    n = 16 * nb
    out = [("positive definite", spd(n, 100.0, False, rng), True, None), ("positive definite, condition 1e3", spd(n, 1e3, False, rng), True, None)]
    for kb in range(nb):
        for j in range(16):
            out.append(("negative pivot at %d of block %d" % (j, kb), indefinite(n, 16 * kb + j, rng), False, 16 * kb + j))
        for j in (0, 7, 14):
            for what, v in (("NaN", np.nan), ("+Inf", np.inf)):
                a = spd(n, 100.0, False, rng)
                a[16 * kb + j, 16 * kb + j] = v
                out.append(("%s on the diagonal at %d of block %d" % (what, j, kb), a, False, None))
        a = spd(n, 100.0, False, rng)
        a[16 * kb + 9, 16 * kb + 3] = a[16 * kb + 3, 16 * kb + 9] = np.nan
        out.append(("NaN off the diagonal in block %d" % kb, a, False, None))
        if kb + 1 < nb:
            a = spd(n, 100.0, False, rng)
            a[16 * kb + 20, 16 * kb + 2] = a[16 * kb + 2, 16 * kb + 20] = np.inf
            out.append(("Inf in the panel below block %d" % kb, a, False, None))
    return out
