// Host-side dump of the QP kernel's LDS plans (mpc_benchmark_amd/csrc/qp_layout.h) for tests/_qp_layout.py: the shapes come on the command line as
// groups of four integers (n neq nin box); one line per shape x batch (6, 300) x matrix cores allowed (1, 0), created as mpc_qp_create does
// (want_mats = batch <= 256).  Every region as name:start:length in doubles, the length being what k_qp_solve addresses in it.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "../../mpc_benchmark_amd/csrc/qp_layout.h"

int main(int argc, char** argv) {
  for (int a = 1; a + 3 < argc; a += 4) {
    const int n = atoi(argv[a]), neq = atoi(argv[a + 1]), nin = atoi(argv[a + 2]), box = atoi(argv[a + 3]), m = nin + (box ? n : 0);
    for (int batch : {6, 300})
      for (int allow_mf = 1; allow_mf >= 0; --allow_mf) {
        const QpLds s = make_qp_lds(n, neq, nin, m, batch <= 256, allow_mf != 0);
        const int nbp = s.np / 16;
        const int lenP = s.mf ? nbp * (nbp + 1) / 2 * 272 : n * s.ldp;                 // tiles of the lower block triangle / n rows of n + 1
        const int lenY = (s.mf ? s.np : n) * s.ldy;
        const int lenS = s.mf ? s.ncb * (s.ncb + 1) / 2 * 272 : neq * s.lds;
        const int lenZD = s.mf ? (s.np > s.ep ? s.np : s.ep) * 17 : 0;
        // the pointer chain of k_qp_solve: x .. tmpn (9 n), y .. tmpe (6 neq), z, zp, s, ds (4 m), red (16), hx0, hdx (2 n) doubles, then actl (nin ints)
        const int lenvec = 11 * n + 6 * neq + 4 * m + 16 + (nin + 1) / 2;
        printf("n=%d neq=%d nin=%d box=%d batch=%d allow_mf=%d mf=%d mats=%d total_bytes=%d np=%d ep=%d ncb=%d ldp=%d ldy=%d lds=%d | P:%d:%d Y:%d:%d S:%d:%d ZD:%d:%d vec:%d:%d H:%d:%d A:%d:%d C:%d:%d\n",
               n, neq, nin, box, batch, allow_mf, s.mf, s.mats, s.total_bytes, s.np, s.ep, s.ncb, s.ldp, s.ldy, s.lds, s.P, lenP, s.Y, lenY, s.S, lenS, s.ZD, lenZD,
               s.vec, lenvec, s.H, s.mats == 1 ? n * n : 0, s.A, s.mats >= 1 ? neq * n : 0, s.C, s.mats >= 1 ? nin * n : 0);
      }
  }
  return 0;
}
