// pipeline_fd_glue.h — the one kernel between the plan and the simulator step of the full-dynamics control pipeline (mpc_feedback_low_level_steps,
// include/mpc_feedback_pipeline.h; fulldynamic_talos.py:512-530): the state-feedback law of the plan's record in force written into the simulator's
// torque input.  One workgroup of one wavefront per robot; the per-robot GEMV is at most 32 x 76 (complete model).
#pragma once
#include "pipeline_glue.h"

struct FdPipeArgs {
  PlanView plan;    // the full-dynamics MPC handle's (m = nv - 6)
  int nq, nv;
  const double* x;  // [B][nx] measured states (the simulator handle's)
  double* sim_u;    // [B][m] torques of the simulator step
};

// With (x0, u0, K0) the plan's record in force (knot 0, or under HELD the held record while a robot's latency runs), the feedback law of pipeline_glue.h:
// d = difference(x_measured, x0) ; tau = u0 - K0 d, unclamped (the script executes it as it is)
template <bool HELD> __global__ void __launch_bounds__(64) k_pipe_state_feedback(FdPipeArgs p, PlanLatencyArgs h) {
  const int b = blockIdx.x, lane = threadIdx.x, m = p.plan.m;
  bool held;
  const PlanRecord r = plan_record_in_force<HELD>(p.plan, h, b, held);
  __shared__ double dd[PIPE_MAX_N];
  pipe_difference(p.x + (size_t)b * p.plan.nx, r.x, p.nq, p.nv, dd, lane);
  __syncthreads();
  for (int i = lane; i < m; i += 64) p.sim_u[(size_t)b * m + i] = pipe_feedback_row(r, dd, p.plan.n, i);
  if (HELD) plan_latency_count(h, b, held, lane);
}
