// plan_latency.h — the per-robot hand-over latency of the plan (include/mpc_plan_latency.h), device side: the layout of a robot's HELD record (knot 1
// of the outgoing plan, by value), the publication kernel that writes it and draws the latency, and what the feedback kernels of the three device
// loops (pipeline_*glue.h) share to pick the record in force and to advance the countdown.  The host side (mpc_plan_latency, mpc_plan_latency_publish,
// mpc_plan_latency_read) is in pipeline_loops.h, with the loops.  The numpy mirror, the definition: mpc_benchmark_amd/plan_latency.py.
#pragma once
#include "../../include/mpc_plan_latency.h"
#include "plan_view.h"
#include "sim_sensors.h"  // sim_sen_philox

#define PLAN_LAT_THREADS 256

// What the second instantiation of a feedback kernel gets beside its own arguments (the first one's arguments stay as they are).
struct PlanLatencyArgs {
  double* state;       // [B][MPC_PLAN_LATENCY_STATE]
  const double* held;  // [B][W] held records: the feedback kernels only read them
  int W;
};

// Robot b's record in `held`.  The layout, here and nowhere else: x [nx] | u [m] | K [m][n] row-major | xd [MPC_PLAN_LATENCY_XDOT] (W = MPC_PLAN_LATENCY_HELD(nx, n, m))
template <class T> DEV PlanRecordOf<T> plan_held_record(T* held, int b, int W, int nx, int m, int n) {
  PlanRecordOf<T> r;
  r.x = held + (size_t)b * W; r.u = r.x + nx; r.K = r.u + m; r.xd = r.K + (size_t)m * n;
  return r;
}

// Does robot b read its held record on this step?  Every lane reads the row; plan_latency_count writes it behind a barrier.
DEV bool plan_latency_in_force(const PlanLatencyArgs& h, int b) {
  const double* s = h.state + (size_t)b * MPC_PLAN_LATENCY_STATE;
  return s[0] > 0.0 && s[6] != 0.0;
}

// The record in force for robot b: knot 0 of the plan, or (HELD, `h` is read by that instantiation alone) the held one while its latency runs.
template <bool HELD> DEV PlanRecord plan_record_in_force(const PlanView& v, const PlanLatencyArgs& h, int b, bool& held) {
  held = false;
  if (HELD) {
    held = plan_latency_in_force(h, b);
    if (held) return plan_held_record(h.held, b, h.W, v.nx, v.m, v.n);
  }
  return plan_knot(v, b, 0, v.slot0);
}

// One lane per robot advances the clock of a low-level step.  The barrier separates it from the other lanes' read of `remaining`.
DEV void plan_latency_count(const PlanLatencyArgs& h, int b, bool held, int lane) {
  __syncthreads();
  if (lane != 0) return;
  double* s = h.state + (size_t)b * MPC_PLAN_LATENCY_STATE;
  if (held) { s[0] -= 1.0; s[3] += 1.0; }
  s[4] += 1.0;
}

struct PlanPublishArgs {
  PlanView plan;         // the outgoing plan, where the loops read it
  int slot1;             // ring slot of knot 1's stage data
  const double* params;  // [B][MPC_PLAN_LATENCY_PARAMS]
  double *state, *held;  // [B][MPC_PLAN_LATENCY_STATE], [B][W]: the publication writes both
  int W;
};

// One workgroup of four wavefronts per robot.  The gain block is the bulk of the copy (32 x 76 of the complete full-dynamics plan, 44 x 76 of the
// complete kinodynamic one): it moves by rows, a wavefront per row and a lane per pair of columns, so a row is one or two coalesced passes and no
// index is divided.  (Rows of the source start at any multiple of 8 bytes — n = 9 of the centroidal plan, nx = 77 before the block in the record —
// so a pair travels as two doubles.)  Lane 0 draws the latency and resets the countdown; stream order serialises the publications.
__global__ void __launch_bounds__(PLAN_LAT_THREADS) k_plan_latency_publish(PlanPublishArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nx = a.plan.nx, n = a.plan.n, m = a.plan.m;
  const PlanRecord k1 = plan_knot(a.plan, b, 1, a.slot1);
  const PlanRecordOf<double> h = plan_held_record(a.held, b, a.W, nx, m, n);
  for (int i = tid; i < nx; i += PLAN_LAT_THREADS) h.x[i] = k1.x[i];
  for (int i = tid; i < m; i += PLAN_LAT_THREADS) h.u[i] = k1.u[i];
  for (int r = wave; r < m; r += PLAN_LAT_THREADS / 64) {
    const double* src = k1.K + (size_t)r * n;
    double* dst = h.K + (size_t)r * n;
    for (int c = 2 * lane; c < n; c += 128) {
      dst[c] = src[c];
      if (c + 1 < n) dst[c + 1] = src[c + 1];
    }
  }
  if (tid < MPC_PLAN_LATENCY_XDOT) h.xd[tid] = k1.xd[tid];
  if (tid == 0) {
    const double* p = a.params + (size_t)b * MPC_PLAN_LATENCY_PARAMS;
    double* s = a.state + (size_t)b * MPC_PLAN_LATENCY_STATE;
    const double plans = s[2] + 1.0;
    const unsigned long long cnt = (unsigned long long)plans;
    unsigned c[4] = {(unsigned)(cnt & 0xFFFFFFFFull), (unsigned)(cnt >> 32), 0u, 0u};
    sim_sen_philox(c, (unsigned)p[2], 0u);
    const double u = ((double)(((unsigned long long)c[1] << 20) | (unsigned long long)(c[0] >> 12)) + 0.5) * 2.220446049250313e-16;  // 2^-52
    const double L = p[0] + fmin(floor(u * (p[1] + 1.0)), p[1]);
    s[0] = L; s[1] = L; s[2] = plans; s[5] = fmax(s[5], L); s[6] = 1.0;
  }
}
