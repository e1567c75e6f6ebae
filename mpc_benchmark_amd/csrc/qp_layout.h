// qp_layout.h — the LDS plan of the batched QP kernel (qp_kernel.h): which of the five forms of k_qp_solve a problem shape runs
// (matrix-core or column-by-column linear algebra; H, A, C staged in LDS or read from global memory) and where every region of
// its workgroup's LDS lies.  Plain C++ without a HIP include, so that the host-side test (tests/_native/qp_layout_dump.cpp,
// tests/test_qp_layout.py) compiles the very rule the library uses.
#pragma once

struct QpLds {
  int P, Y, S, vec, H, A, C, mats, total_bytes;  // mats: 1 = H, A, C are staged in LDS too, 2 = A and C only
  // MF form: padded dimensions (np, ep: multiples of 16 ; ncb: 16-column blocks of [A^T | r1]), leading dimensions, inverted diagonal blocks
  int mf, np, ep, ncb, ldp, ldy, lds, LIp, LIs, ZD;
};
static inline QpLds make_qp_lds(int n, int neq, int nin, int m, bool want_mats = true, bool allow_mf = true) {
  QpLds s;
  auto layout = [&](bool mf, int mats) {
    int o = 0;
    auto take = [&](int c) { int r = o; o += (c + 1) & ~1; return r; };
    s.mf = mf ? 1 : 0;
    s.np = (n + 15) & ~15; s.ep = (neq + 15) & ~15; s.ncb = (neq + 1 + 15) / 16;
    if (mf) {
      // P and the Gram matrix G = [Y | w]^T [Y | w] (its leading block becomes S) as the tiles of their lower block triangles
      // (mfma_blocks.h ptile: 272 doubles each, the inverse of a diagonal factor block replaces the block)
      const int nbp = s.np / 16;
      s.ldp = s.lds = 17; s.ldy = 16 * s.ncb + 1; s.LIp = s.LIs = 0;
      s.P = take(nbp * (nbp + 1) / 2 * 272); s.Y = take(s.np * s.ldy);
      s.S = take(s.ncb * (s.ncb + 1) / 2 * 272); s.ZD = take((s.np > s.ep ? s.np : s.ep) * 17);
    } else {
      s.ldp = n + 1; s.ldy = neq + 1; s.lds = neq + 1; s.LIp = s.LIs = s.ZD = 0;
      s.P = take(n * (n + 1)); s.Y = take(n * (neq + 1)); s.S = take(neq * (neq + 1));
    }
    s.vec = take(11 * n + 6 * neq + 4 * m + nin + 64);
    s.H = s.A = s.C = 0;
    if (mats == 1) s.H = take(n * n);
    if (mats >= 1) { s.A = take(neq * n); s.C = take(nin * n); }
    s.mats = mats;
    s.total_bytes = o * 8;
    return o * 8 + 64 <= 160 * 1024;
  };
  // preference: matrix-core form with all / some / none of the problem matrices in LDS, then the column-by-column form
  const bool can_mf = allow_mf && neq > 0 && n >= 16;
  if (can_mf && want_mats && layout(true, 1)) return s;
  if (can_mf && want_mats && layout(true, 2)) return s;
  if (can_mf && layout(true, 0)) return s;
  if (want_mats && layout(false, 1)) return s;
  layout(false, 0);
  return s;
}
