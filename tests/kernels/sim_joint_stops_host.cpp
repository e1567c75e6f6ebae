// The body of k_sim_joint_stops (mpc_benchmark_amd/csrc/sim_joint_stops.h, included as it is) compiled for the host: a stand-alone program of
// tests/test_joint_stops_host.py (test infrastructure), built there with the address and undefined-behaviour sanitizers.  The lanes of a workgroup
// run one after the other, 63 down to 0, and the wave vote accumulates, so that lane 0, which writes the robot's counters, sees the vote of all.
//   usage: sim_joint_stops_host in.bin out.bin
//   in:  int32 B, nu, nq, nv, S ; double params[B][8], lo[B][nu], hi[B][nu], scale[nu] ; S times: x[B][nq + nv], tau[B][nu]
//   out: S times: out[B][nu], rows[B][5 nu + 2]
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
using std::fabs;
using std::fmax;
using std::fmin;
struct Idx { int x; };
static Idx blockIdx, threadIdx;
static int vote;
static int __any(int v) { vote |= v; return vote; }
#define __global__
#define __launch_bounds__(x)
#include "../../mpc_benchmark_amd/csrc/sim_joint_stops.h"

int main(int argc, char** argv) {
  if (argc != 3) return 1;
  FILE* f = fopen(argv[1], "rb");
  FILE* g = fopen(argv[2], "wb");
  int hdr[5];
  if (!f || !g || fread(hdr, sizeof(int), 5, f) != 5) return 1;
  const int B = hdr[0], nu = hdr[1], nq = hdr[2], nv = hdr[3], S = hdr[4];
  auto rd = [&](size_t n) {
    std::vector<double> v(n);
    if (fread(v.data(), sizeof(double), n, f) != n) exit(2);
    return v;
  };
  // (exactly sized vectors: an index out of a part's bounds is the sanitizer's to find)
  const auto params = rd((size_t)B * MPC_SIM_JOINT_STOPS_PARAMS), lo = rd((size_t)B * nu), hi = rd((size_t)B * nu), scale = rd(nu);
  std::vector<double> rows((size_t)B * (5 * nu + 2), 0.0), out((size_t)B * nu, 0.0);
  for (int s = 0; s < S; ++s) {
    const auto x = rd((size_t)B * (nq + nv)), tau = rd((size_t)B * nu);
    SimJointStopsArgs a;
    a.nq = nq; a.nv = nv; a.nu = nu;
    a.x = x.data(); a.tau = tau.data(); a.params = params.data(); a.lo = lo.data(); a.hi = hi.data(); a.scale = scale.data();
    a.out = out.data(); a.rows = rows.data();
    for (int b = 0; b < B; ++b) {
      vote = 0;
      blockIdx.x = b;
      for (int t = SIM_JS_THREADS - 1; t >= 0; --t) {
        threadIdx.x = t;
        k_sim_joint_stops(a);
      }
    }
    fwrite(out.data(), sizeof(double), out.size(), g);
    fwrite(rows.data(), sizeof(double), rows.size(), g);
  }
  fclose(f);
  fclose(g);
  return 0;
}
