// pass_kernels.h — which instantiation of the sweep, leg, forward and dual kernels serves a handle: chosen ONCE, when the handle is created
// (select_pass_kernels), into one table that the three host-side consumers read — create_impl (LDS carve-out attributes), launch_pass (the
// launches) and mpc_kernel_info (the occupancy report).  A new instantiation is added here and nowhere else.  The grids that both the
// launches and the report need are below the table.
#pragma once
#include "riccati_mfma.h"
#include "closed_loop.h"
#include "legs.h"
#include "legs_tree.h"

// Problems whose dimensions get compile-time instantiations of the sweep and the leg kernels (riccati_mfma.h "FN, FM"):
//   X(id, n, m, gfull, st_lds, NP, MP)   — (n, m): state / control dimension ; gfull, st_lds: the sweep's LDS plan for them (make_ric_lds) ;
//   NP, MP: padded state / control dimension (the template arguments of the tree and of k_leg_knot)
// 1: complete Talos (38 dofs), full dynamics   2: complete Talos, kinodynamic   3: Talos with the upper body locked as the scripts lock it
// (28 dofs), full dynamics   4: the same, kinodynamic.  The stage kernel has its own list (eval_multibody.hip).
#define MPC_FIXED_MODELS(X) X(1, 76, 32, 1, 1, 80, 32) X(2, 76, 44, 3, 0, 80, 48) X(3, 56, 22, 3, 1, 64, 32) X(4, 56, 34, 3, 1, 64, 48)

typedef void (*RicKernel)(SolverArgs, RicLds);                    // k_riccati_mfma
typedef void (*LegKnotKernel)(SolverArgs, LkLds, int, int);       // k_leg_knot
typedef void (*LegCondenseKernel)(SolverArgs, LcLds);             // k_leg_condense
typedef void (*LegTailKernel)(SolverArgs, LcLds, LkLds, int);     // k_leg_condense_tail
typedef void (*LegConsensusKernel)(SolverArgs, LxLds);            // k_leg_consensus
typedef void (*LegTreeKernel)(SolverArgs, LxLds, TreeDesc, int);  // k_leg_compose, k_leg_tree_down
typedef void (*PlainKernel)(SolverArgs);                          // k_forward_phi, k_forward_prefetch, k_forward, k_duals

// One kernel role of a pass: the instantiation, its name in the occupancy report, threads per workgroup, dynamic LDS bytes
template <class Fn> struct PassKernel {
  Fn fn;
  const char* name;
  int threads, lds;
};

struct PassKernels {
  PassKernel<RicKernel> sweep_legs;             // Riccati sweep, workgroup (instance, leg)
  PassKernel<RicKernel> sweep_serial;           // ... one workgroup per instance ; fn == nullptr: k_riccati_backward (no matrix cores)
  PassKernel<LegKnotKernel> leg_knot;
  PassKernel<LegCondenseKernel> leg_condense;   // the two forms of the condensation: separate,
  PassKernel<LegTailKernel> leg_condense_tail;  // ... fused with the last knots of the horizon (a workgroup runs either body: the larger carve-out)
  PassKernel<LegConsensusKernel> leg_consensus;
  PassKernel<LegTreeKernel> leg_compose, leg_tree_down;
  PassKernel<PlainKernel> forward_phi;          // forward sweeps of the legs (and the serial one after k_closed_loop, which needs m <= 32 as <4, 10> does)
  PassKernel<PlainKernel> forward_serial;       // the register-prefetch sweeps or k_forward
  bool forward_serial_leaves_abdz;              // ... and whether that form leaves [A B] [dx; du] of every knot behind for k_duals (the prefetch sweeps do)
  PassKernel<PlainKernel> duals;
  // f(kernel, bytes) for the roles whose carve-out may exceed what a kernel gets without asking (the sweeps and the leg kernels ; the
  // forward and dual kernels keep a few vectors).  The leg roles are empty (fn == nullptr) on a handle whose dimensions do not fit them.
  template <class F> void for_each_carve_out(F&& f) const {
    auto one = [&](const auto& k) { if (k.fn) f((const void*)k.fn, k.lds); };
    one(sweep_legs); one(sweep_serial); one(leg_knot); one(leg_condense); one(leg_condense_tail); one(leg_consensus); one(leg_compose); one(leg_tree_down);
  }
};

#define PK_STR_(x) #x
#define PK_STR(x) PK_STR_(x)  // (the workgroup sizes of the sweep in the names: as they were compiled, -DRIC_THREADS=256 of `make variants` included)

// `Handle` is mpc_solver (a template only because mpc_solver, which holds the table, is defined after this header).  Reads what is fixed
// when the handle is created: ric, ric_fixed, lk, lc, lx, use_mfma_riccati, legs_ok, env_duals_plain and the dimensions of L.
template <class Handle> static PassKernels select_pass_kernels(const Handle& s) {
  const Layout& L = s.L;
  PassKernels p{};
  const bool small = s.ric.np == 16 && s.ric.mp == 16 && L.c <= RIC_SMALL_THREADS;  // small problems (np = mp = 16): their own workgroup size
  const int rt = small ? RIC_SMALL_THREADS : RIC_THREADS, ric_lds = s.ric.total_bytes;
  if (s.use_mfma_riccati) {
    RicKernel f = k_riccati_mfma<RIC_THREADS, 96>;
    if (small) f = k_riccati_mfma<RIC_SMALL_THREADS, 16>;
    else if (s.ric.sq && s.ric.np <= 80) f = k_riccati_mfma<RIC_THREADS, 80, true>;
    else if (s.ric.sq) f = k_riccati_mfma<RIC_THREADS, 96, true>;
    else if (s.ric.np <= 80) f = k_riccati_mfma<RIC_THREADS, 80>;  // fewer tiles per wavefront: lower register pressure
    p.sweep_serial = {f, "k_riccati_mfma (serial sweep)", rt, ric_lds};
  } else p.sweep_serial = {nullptr, "k_riccati_backward (serial sweep, no matrix cores)", 256, (int)s.riccati_lds()};
  p.forward_phi = {L.m <= 32 ? k_forward_phi<4, 10> : k_forward_phi<6, 10>, "k_forward_phi (forward sweeps of the legs)", 512, (int)(2 * L.n * sizeof(double))};
  {
    const bool fits = L.nz <= 128 && L.n + L.m <= L.nz && L.n <= 80;
    const int fw_lds = (int)((L.nz + 2 * L.n) * sizeof(double));
    p.forward_serial_leaves_abdz = fits && L.m <= 48;
    if (fits && L.m <= 32) p.forward_serial = {k_forward_prefetch<4, 10>, "k_forward_prefetch<4,10>", 512, fw_lds};
    else if (fits && L.m <= 48) p.forward_serial = {k_forward_prefetch<6, 10>, "k_forward_prefetch<6,10>", 512, fw_lds};
    else p.forward_serial = {k_forward, "k_forward", 1024, fw_lds};
  }
  // (LDS: the step, three vectors of n, the partial sums, then three per-row scalars of the constraint block — four in the staged form)
  if (s.env_duals_plain) p.duals = {k_duals<true>, "k_duals<true> (MPC_DUALS_PLAIN)", 256, (int)((L.nz + 3 * L.n + 16 + 3 * L.c) * sizeof(double))};
  else p.duals = {k_duals<false>, "k_duals", 256, (int)((L.nz + 3 * L.n + 16 + 4 * L.c) * sizeof(double))};
  if (!s.legs_ok) return p;

  const int lk_lds = s.lk.total_bytes, lc_lds = s.lc.total_bytes, lx_lds = s.lx.total_bytes, tail_lds = lc_lds > lk_lds ? lc_lds : lk_lds;
  // the generic forms, by padded dimension
#define PK_BY_MP(K) (s.lk.mp <= 16 ? K<16> : s.lk.mp <= 32 ? K<32> : K<48>)
#define PK_BY_NP(K) (s.lx.np == 16 ? K<16> : s.lx.np == 32 ? K<32> : s.lx.np == 48 ? K<48> : s.lx.np == 64 ? K<64> : K<80>)
  if (small) p.sweep_legs = {k_riccati_mfma<RIC_SMALL_THREADS, 16, false, true>, "k_riccati_mfma<" PK_STR(RIC_SMALL_THREADS) ",16,false,true> (sweep, legs)", rt, ric_lds};
  else if (s.ric.sq) p.sweep_legs = {k_riccati_mfma<RIC_THREADS, 80, true, true>, "k_riccati_mfma<" PK_STR(RIC_THREADS) ",80,true,true> (sweep, legs)", rt, ric_lds};
  else p.sweep_legs = {k_riccati_mfma<RIC_THREADS, 80, false, true>, "k_riccati_mfma<" PK_STR(RIC_THREADS) ",80,false,true> (sweep, legs)", rt, ric_lds};
  p.leg_knot = {PK_BY_MP(k_leg_knot), "k_leg_knot", LK_THREADS, lk_lds};
  p.leg_condense = {k_leg_condense<0>, "k_leg_condense", LK_THREADS, lc_lds};
  p.leg_condense_tail = {PK_BY_MP(k_leg_condense_tail), "k_leg_condense_tail (condensation + the last leg's knots)", LK_THREADS, tail_lds};
  p.leg_consensus = {PK_BY_NP(k_leg_consensus), "k_leg_consensus", LK_THREADS, lx_lds};
  p.leg_compose = {PK_BY_NP(k_leg_compose), "k_leg_compose (first level of the tree over the cuts)", LCMP_THREADS, lx_lds};
  p.leg_tree_down = {PK_BY_NP(k_leg_tree_down), "k_leg_tree_down (last level)", LK_THREADS, lx_lds};
#undef PK_BY_MP
#undef PK_BY_NP
  // the fixed-dimension forms (the chain over the cuts, k_leg_consensus, has none)
#define X(ID, FN, FM, GF, ST, NPV, MPV) if (s.ric_fixed == ID) { \
    p.sweep_legs = {k_riccati_mfma<RIC_THREADS, 80, true, true, FN, FM, GF, ST>, "k_riccati_mfma<" PK_STR(RIC_THREADS) ",80,true,true," #FN "," #FM "," #GF "," #ST "> (sweep, legs, fixed dimensions)", rt, ric_lds}; \
    p.leg_knot = {k_leg_knot<MPV, FN, FM>, "k_leg_knot<" #MPV "," #FN "," #FM "> (fixed dimensions)", LK_THREADS, lk_lds}; \
    p.leg_condense = {k_leg_condense<FN>, "k_leg_condense<" #FN "> (fixed dimensions)", LK_THREADS, lc_lds}; \
    p.leg_condense_tail = {k_leg_condense_tail<MPV, FN, FM>, "k_leg_condense_tail<" #MPV "," #FN "," #FM "> (fixed dimensions)", LK_THREADS, tail_lds}; \
    p.leg_compose = {k_leg_compose<NPV, FN, FM>, "k_leg_compose<" #NPV "," #FN "," #FM "> (first level of the tree over the cuts, fixed dimensions)", LCMP_THREADS, lx_lds}; \
    p.leg_tree_down = {k_leg_tree_down<NPV, FN, FM>, "k_leg_tree_down<" #NPV "," #FN "," #FM "> (last level, fixed dimensions)", LK_THREADS, lx_lds}; }
  MPC_FIXED_MODELS(X)
#undef X
  return p;
}

// ---- grids: one rule each for the launch and for the report ----
// k_leg_knot: the knots before kmax = N - tail in chunks (the knots from kmax on: k_leg_condense_tail ; kmax >= leg_start(J - 1) >= 1)
static inline dim3 leg_knot_grid(int N, int B, int tail, int chunk) { return dim3((N - tail + chunk - 1) / chunk, B); }
// the condensation: the parametric legs, and in the fused form (tail > 0) one workgroup more per instance for the tail
static inline dim3 leg_condense_grid(int J, int B, int tail) { return dim3(tail > 0 ? J : J - 1, B); }
// the tree over the cuts, upwards: the nodes of the level and one workgroup more for a step of the K_0 path, two halves of a composition each (z)
static inline dim3 leg_compose_grid(const TreeDesc& T, int lev, int B) { return dim3(T.lev_cnt[lev] + 1, B, 2); }
// ... downwards: the nodes of the level ; at the last level (the first one launched) the root's step of the K_0 path beside them
static inline dim3 leg_tree_down_grid(const TreeDesc& T, int lev, int B) { return dim3(T.lev_cnt[lev] + (lev == T.nlev - 1 ? 1 : 0), B); }
static inline dim3 leg_apply_grid(int N, int J, int C, int B) { return dim3(leg_apply_chunks(N, J, C), B); }
static inline dim3 forward_phi_grid(int B, int J) { return dim3(B * J); }
static inline long long grid_workgroups(dim3 g) { return (long long)g.x * g.y * g.z; }
