// pipeline_fd_glue.h — the one kernel between the plan and the simulator step of the full-dynamics control pipeline (mpc_feedback_low_level_steps,
// include/mpc_feedback_pipeline.h; fulldynamic_talos.py:512-530): the state-feedback law of the plan's knot 0 written into the simulator's torque input.
// One workgroup of one wavefront per robot; the per-robot GEMV is at most 32 x 76 (complete model).
#pragma once
#include "pipeline_glue.h"

struct FdPipeArgs {
  // the plan (full-dynamics MPC handle): solution of knot 0 and its Riccati gain, indexed as k_pipe_feedback reads them
  const double *xs, *us, *gains;
  int N, nx, nq, nv, n, m, gain_stride, oK;
  const double* x;  // [B][nx] measured states (the simulator handle's)
  double* sim_u;    // [B][m] torques of the simulator step (m = nv - 6)
};

// d = difference(x_measured, xs[0]) ; tau = us[0] - K_0 d, unclamped (the script executes it as it is)
// HELD (include/mpc_plan_latency.h; launched while a latency is armed on the plan, `h` is read by it alone): a robot whose hand-over latency has
// not run out takes xs, us and K from its held record (knot 1 of the plan before) instead; then one lane advances its clock.
template <bool HELD> __global__ void __launch_bounds__(64) k_pipe_state_feedback(FdPipeArgs p, PlanLatencyArgs h) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nx = p.nx, nq = p.nq, nv = p.nv, n = p.n, m = p.m;
  const double* x = p.x + (size_t)b * nx;
  const double* x0 = p.xs + (size_t)b * (p.N + 1) * nx;
  const double* us0 = p.us + (size_t)b * p.N * m;
  const double* K0 = p.gains + (size_t)b * (p.N + 1) * p.gain_stride + p.oK;
  bool held = false;
  if (HELD) {
    held = plan_latency_in_force(h, b);
    if (held) { x0 = h.held + (size_t)b * h.W; us0 = x0 + nx; K0 = us0 + m; }
  }
  __shared__ double dd[PIPE_MAX_N];
  if (lane == 0) {  // the base: log of the relative SE(3) placement, as k_pipe_feedback
    const M3 Rx = quat_to_rot(x + 3), R0 = quat_to_rot(x0 + 3);
    V3 ev, ew;
    log6(tmul(Rx, R0), tmul(Rx, v3(x0[0] - x[0], x0[1] - x[1], x0[2] - x[2])), ev, ew);
    dd[0] = ev.x; dd[1] = ev.y; dd[2] = ev.z; dd[3] = ew.x; dd[4] = ew.y; dd[5] = ew.z;
  }
  for (int i = 6 + lane; i < nv; i += 64) dd[i] = x0[i + 1] - x[i + 1];
  for (int i = lane; i < nv; i += 64) dd[nv + i] = x0[nq + i] - x[nq + i];
  __syncthreads();
  for (int i = lane; i < m; i += 64) {
    double su = 0.0;
    for (int j = 0; j < n; ++j) su += K0[(size_t)i * n + j] * dd[j];
    p.sim_u[(size_t)b * m + i] = us0[i] - su;
  }
  if (HELD) plan_latency_count(h, b, held, lane);
}
