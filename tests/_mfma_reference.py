"""Plain-numpy restatements of the algorithms of mfma_blocks.h and the high-precision metrics they are judged by.

Nothing here reads csrc/.  Every restatement follows the device's elimination order (right-looking 16 x 16 factorisation, the inverse of
each diagonal block formed once and then only multiplied with, blocked updates in the device's order) but takes sqrt and 1 / sqrt
correctly rounded, and works on whatever numpy dtype it is handed: float64 (the yardstick of the accuracy bounds) or object arrays of
fractions.Fraction (the exact evaluation behind the planted cases, where every pivot is 1).

The metrics are componentwise backward errors in units of u = 2^-53, evaluated in np.longdouble (64-bit significand) or, where the
platform's longdouble is no wider than a double, exactly in Fraction."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 1e-18)


# ---- scalar helpers that work for float64 and Fraction ----------------------------------------------------------------------------
def _sqrt(x):
    if isinstance(x, Fraction):
        assert x == 1, "exact cases are built so that every pivot is 1 (got %s)" % (x,)
        return Fraction(1)
    return np.sqrt(x)


def _zeros(shape, like):
    if like.dtype == object:
        z = np.empty(shape, dtype=object)
        z.fill(Fraction(0))
        return z
    return np.zeros(shape, dtype=like.dtype)


def _eye(n, like):
    e = _zeros((n, n), like)
    for i in range(n):
        e[i, i] = Fraction(1) if like.dtype == object else 1.0
    return e


def to_fraction(a):
    a = np.asarray(a)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = Fraction(float(a[idx]))
    return out


def mirror_lower(a):
    """the symmetric matrix whose lower triangle is a's"""
    lo = np.tril(a)
    return lo + np.tril(a, -1).T


# ---- 16 x 16 Cholesky + inverse ---------------------------------------------------------------------------------------------------
def chol16_register(D, ncols=16):
    """The register form (chol16_wave, chol16_wave_n<NC>): right-looking Cholesky column by column with the pivot's reciprocal square
    root, then L^-1 row by row (x[R] -= L[R][K] x[K] in the order K = 0, 1, ...).  Rows / columns from ncols on are identity padding.
    -> (L lower triangular, X = L^-1)"""
    n = D.shape[0]
    d = np.tril(D).copy()
    invd = [None] * n
    for j in range(ncols):
        piv = _sqrt(d[j, j])
        inv = 1 / piv
        invd[j] = inv
        d[j + 1:, j] = d[j + 1:, j] * inv
        d[j, j] = piv
        for c in range(j + 1, ncols):
            d[c:, c] = d[c:, c] - d[c:, j] * d[c, j]
    x = _eye(n, D)
    for k in range(ncols):
        x[k, :] = x[k, :] * invd[k]
        for r in range(k + 1, ncols):
            x[r, :] = x[r, :] - d[r, k] * x[k, :]
    return d, x


def chol16_panels(D, ncols=16):
    """The matrix-core form (chol16_wave_mfma): four panels of four columns; the 4 x 4 pivot block T T^T is factorised and inverted
    (M = T^-1) by every lane, the panel is L_p = A_p M^T, the rows of the inverse X_p = M W_p with W = I - L_done X_done, then
    A -= L_p L_p^T and W -= L_p X_p.  Panels that hold only identity padding are skipped.  -> (L, X)"""
    n = 16
    t = mirror_lower(D)
    w = _eye(n, D)
    L = np.tril(D).copy()
    X = _zeros((n, n), D)
    npan = (ncols + 3) >> 2
    for p in range(4):
        c0 = 4 * p
        if p >= npan:
            X[c0:c0 + 4, :] = w[c0:c0 + 4, :]
            continue
        a = t[c0:c0 + 4, c0:c0 + 4]
        t00 = _sqrt(a[0, 0]); i0 = 1 / t00
        t10, t20, t30 = a[1, 0] * i0, a[2, 0] * i0, a[3, 0] * i0
        t11 = _sqrt(a[1, 1] - t10 * t10); i1 = 1 / t11
        t21, t31 = (a[2, 1] - t20 * t10) * i1, (a[3, 1] - t30 * t10) * i1
        t22 = _sqrt(a[2, 2] - t20 * t20 - t21 * t21); i2 = 1 / t22
        t32 = (a[3, 2] - t30 * t20 - t31 * t21) * i2
        t33 = _sqrt(a[3, 3] - t30 * t30 - t31 * t31 - t32 * t32); i3 = 1 / t33
        m10 = -(t10 * i0) * i1
        m21 = -(t21 * i1) * i2
        m20 = -(t20 * i0 + t21 * m10) * i2
        m32 = -(t32 * i2) * i3
        m31 = -(t31 * i1 + t32 * m21) * i3
        m30 = -(t30 * i0 + t31 * m10 + t32 * m20) * i3
        z = i0 * 0
        T = np.array([[t00, z, z, z], [t10, t11, z, z], [t20, t21, t22, z], [t30, t31, t32, t33]], dtype=D.dtype)
        M = np.array([[i0, z, z, z], [m10, i1, z, z], [m20, m21, i2, z], [m30, m31, m32, i3]], dtype=D.dtype)
        lp = _zeros((n, 4), D)
        lp[c0:c0 + 4, :] = T
        lp[c0 + 4:, :] = t[c0 + 4:, c0:c0 + 4] @ M.T
        xp = M @ w[c0:c0 + 4, :]
        L[c0:, c0:c0 + 4] = lp[c0:, :]
        X[c0:c0 + 4, :] = xp
        if p + 1 < npan:
            t = t - lp @ lp.T
            w = w - lp @ xp
    return L, X


# ---- blocked factorisation and solves ---------------------------------------------------------------------------------------------
def chol_blocked(A, nb, n_real=None, chol16=chol16_register, last_ncols=None):
    """chol_blocked / chol_blocked_wave / chol_tiles / chol_tiles_wave: per diagonal block kb the 16 x 16 factorisation and its inverse,
    the panel L[ri][kb] = A[ri][kb] LI[kb]^T, the trailing update A[ri][cj] -= L[ri][kb] L[cj][kb]^T (lower block triangle).
    -> (L, full lower triangular (16 nb) x (16 nb); LI, the list of the nb block inverses)"""
    A = np.tril(A).copy()
    LI = []
    for kb in range(nb):
        k0, k1 = 16 * kb, 16 * kb + 16
        nc = 16
        if n_real is not None:
            nc = min(16, max(0, n_real - k0))
        if last_ncols is not None and kb == nb - 1:
            nc = last_ncols
        Lkk, X = chol16(A[k0:k1, k0:k1], nc)
        A[k0:k1, k0:k1] = Lkk
        LI.append(X)
        for ri in range(kb + 1, nb):
            A[16 * ri:16 * ri + 16, k0:k1] = A[16 * ri:16 * ri + 16, k0:k1] @ X.T
        for ri in range(kb + 1, nb):
            for cj in range(kb + 1, ri + 1):
                r0, c0 = 16 * ri, 16 * cj
                A[r0:r0 + 16, c0:c0 + 16] = A[r0:r0 + 16, c0:c0 + 16] - A[r0:r0 + 16, k0:k1] @ A[c0:c0 + 16, k0:k1].T
    return np.tril(A), LI


def trsm_fwd(L, LI, nb, B):
    """X = L^-1 B block row by block row: X[bi] = LI[bi] (B[bi] - sum_{bj < bi} L[bi][bj] X[bj])"""
    X = B.copy()
    for bi in range(nb):
        r0 = 16 * bi
        X[r0:r0 + 16] = LI[bi] @ (X[r0:r0 + 16] - L[r0:r0 + 16, :r0] @ X[:r0]) if bi else LI[bi] @ X[r0:r0 + 16]
    return X


def trsm_bwd(L, LI, nb, B):
    """X = L^-T B from the last block row up: X[bi] = LI[bi]^T (B[bi] - sum_{bj > bi} L[bj][bi]^T X[bj])"""
    X = B.copy()
    for bi in range(nb - 1, -1, -1):
        r0 = 16 * bi
        rhs = X[r0:r0 + 16] - L[r0 + 16:, r0:r0 + 16].T @ X[r0 + 16:] if bi < nb - 1 else X[r0:r0 + 16]
        X[r0:r0 + 16] = LI[bi].T @ rhs
    return X


def tile_product(C0, A, B, neg):
    return C0 - A @ B if neg else C0 + A @ B


# ---- metrics ----------------------------------------------------------------------------------------------------------------------
def _hp(a):
    return np.asarray(a, dtype=np.longdouble) if LONGDOUBLE_OK else to_fraction(a)


def _worst(num, den):
    """-> (max over entries of num / den in units of u, (row, col)); 0 / 0 counts as 0, x / 0 as inf"""
    num = np.abs(num)
    if num.dtype != object:
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.where(num == 0, 0.0, np.where(den == 0, np.inf, num / den))
        v = np.where(np.isnan(num) | np.isnan(v), np.inf, v)
        where = np.unravel_index(int(np.argmax(v)), v.shape)
        return float(v[where]) / U, tuple(int(i) for i in where)
    best, where = 0.0, (0, 0)
    for idx in np.ndindex(num.shape):
        nu, de = num[idx], den[idx]
        if nu == 0:
            continue
        if nu != nu:
            return float("inf"), idx
        v = float("inf") if de == 0 else float(nu / de) / U
        if v > best:
            best, where = v, idx
    return best, where


def factor_metric(A, L):
    """worst entry of |A - L L^T| / (|L| |L|^T) over the lower triangle, A given by its lower triangle"""
    Ah, Lh = _hp(mirror_lower(A)), _hp(np.tril(L))
    num = np.tril(Ah - Lh @ Lh.T)
    return _worst(num, np.abs(Lh) @ np.abs(Lh).T)


def inverse_metric(X, L):
    """worst entry of |X L - I| / (|X| |L|)"""
    Xh, Lh = _hp(X), _hp(np.tril(L))
    n = Lh.shape[0]
    eye = _hp(np.eye(n))
    return _worst(Xh @ Lh - eye, np.abs(Xh) @ np.abs(Lh))


def solve_metric(L, X, B, transpose):
    """worst entry of |op(L) X - B| / (|op(L)| |X| + |B|), op(L) = L or L^T"""
    Lh, Xh, Bh = _hp(np.tril(L)), _hp(X), _hp(B)
    if transpose:
        Lh = Lh.T
    return _worst(Lh @ Xh - Bh, np.abs(Lh) @ np.abs(Xh) + np.abs(Bh))


def tile_metric(C, C0, A, B, neg):
    """worst entry of |C - (C0 +/- A B)| / (|C0| + |A| |B|)"""
    Ch, C0h, Ah, Bh = _hp(C), _hp(C0), _hp(A), _hp(B)
    ref = C0h - Ah @ Bh if neg else C0h + Ah @ Bh
    return _worst(Ch - ref, np.abs(C0h) + np.abs(Ah) @ np.abs(Bh))


def rsqrt_relative_error(d, r):
    """|r sqrt(d) - 1| per entry in units of u (the relative error of r against 1 / sqrt(d)), in longdouble"""
    dh, rh = np.asarray(d, dtype=np.longdouble), np.asarray(r, dtype=np.longdouble)
    return np.abs(rh * np.sqrt(dh) - 1).astype(np.float64) / U
