// pipeline_glue.h — the two small kernels that string the kinodynamic control pipeline together on the device (mpc_qp_low_level_steps,
// include/mpc_qp_abi.h; kinodynamic_talos.py:411-462): the feedback terms of the plan's record in force into the inputs of the inverse-dynamics QP, and
// the QP's torque into the simulator step.  One workgroup of one wavefront per robot; the vectors are a few hundred bytes.  Shared: the feedback law
// of a multibody plan (pipe_difference, pipe_feedback_row) with the full-dynamics loop (pipeline_fd_glue.h), the torque kernel with the centroidal loop.
#pragma once
#include "solver_args.h"
#include "plan_latency.h"

struct PipeArgs {
  PlanView plan;      // the kinodynamic MPC handle's
  int nq, nv, nk;
  const double* x;    // [B][nx] measured states (the simulator handle's)
  double *xrob, *acc, *f;  // inputs of the inverse-dynamics QP's assembly kernel
};

#define PIPE_MAX_N 160  // tangent dimension 2 nv of the plan

// dd[0 .. 2 nv) = difference(x_measured, x0): the SE(3) log of the base on lane 0, joint and velocity differences on all lanes.  The caller's barrier follows.
DEV void pipe_difference(const double* x, const double* x0, int nq, int nv, double* dd, int lane) {
  if (lane == 0) {
    const M3 Rx = quat_to_rot(x + 3), R0 = quat_to_rot(x0 + 3);
    V3 ev, ew;
    log6(tmul(Rx, R0), tmul(Rx, v3(x0[0] - x[0], x0[1] - x[1], x0[2] - x[2])), ev, ew);
    dd[0] = ev.x; dd[1] = ev.y; dd[2] = ev.z; dd[3] = ew.x; dd[4] = ew.y; dd[5] = ew.z;
  }
  for (int i = 6 + lane; i < nv; i += 64) dd[i] = x0[i + 1] - x[i + 1];
  for (int i = lane; i < nv; i += 64) dd[nv + i] = x0[nq + i] - x[nq + i];
}

// row i of u - K dd
DEV double pipe_feedback_row(const PlanRecord& r, const double* dd, int n, int i) {
  double su = 0.0;
  for (int j = 0; j < n; ++j) su += r.K[(size_t)i * n + j] * dd[j];
  return r.u[i] - su;
}

// With (x0, u0, K0, xd0) the plan's record in force (knot 0, or under HELD — include/mpc_plan_latency.h — the held record while a robot's latency runs):
// d = difference(x_measured, x0) ; forces = u0[:6 nk] - K0[:6 nk] d ; a0 = [xd0: the base acceleration ; u0[6 nk:] - K0[6 nk:] d]
template <bool HELD> __global__ void __launch_bounds__(64) k_pipe_feedback(PipeArgs p, PlanLatencyArgs h) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nx = p.plan.nx, nv = p.nv, m = p.plan.m, nf = 6 * p.nk;
  const double* x = p.x + (size_t)b * nx;
  bool held;
  const PlanRecord r = plan_record_in_force<HELD>(p.plan, h, b, held);
  __shared__ double dd[PIPE_MAX_N];
  pipe_difference(x, r.x, p.nq, nv, dd, lane);
  __syncthreads();
  for (int i = lane; i < m; i += 64) {
    const double su = pipe_feedback_row(r, dd, p.plan.n, i);
    if (i < nf) p.f[(size_t)b * nf + i] = su;
    else p.acc[(size_t)b * nv + 6 + (i - nf)] = su;
  }
  if (lane < 6) p.acc[(size_t)b * nv + lane] = r.xd[lane];
  for (int i = lane; i < nx; i += 64) p.xrob[(size_t)b * nx + i] = x[i];
  if (HELD) plan_latency_count(h, b, held, lane);
}

struct PipeTorqueArgs {
  const double* sol;      // [B][qn] solution of the QP: (a [nv], df [6 nk], tau [nv - 6])
  int qn, nv, nk;
  const double* f;        // [B][6 nk] the forces the QP was assembled with
  double* f_new;          // [B][6 nk] forces + df
  const int32_t* used;    // [B][nk] contact set the QP worked with (pipeline_contacts.h), or nullptr: the caller's contact_states, f_new as it is
  double* sim_u;          // [B][nv - 6] torques of the simulator step
  const double* tau_max;  // [nv - 6] clamp (kinodynamic loop), or nullptr: the QP's torque box is the limit (centroidal loop, centroidal_talos.py:435-447)
};

// the QP's torque — clamped to +-tau_max where given — into the simulator's input ; forces + df (with `used`: 0 for a contact the QP did not use)
__global__ void __launch_bounds__(64) k_pipe_torque(PipeTorqueArgs p) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nv = p.nv, nf = 6 * p.nk, nu = nv - 6;
  const double* sol = p.sol + (size_t)b * p.qn;
  for (int i = lane; i < nu; i += 64) {
    double t = sol[nv + nf + i];
    if (p.tau_max) { const double lim = p.tau_max[i]; t = fmin(fmax(t, -lim), lim); }
    p.sim_u[(size_t)b * nu + i] = t;
  }
  if (!p.used) {
    for (int i = lane; i < nf; i += 64) p.f_new[(size_t)b * nf + i] = p.f[(size_t)b * nf + i] + sol[nv + i];
    return;
  }
  for (int i = lane; i < nf; i += 64) p.f_new[(size_t)b * nf + i] = p.used[(size_t)b * p.nk + i / 6] ? p.f[(size_t)b * nf + i] + sol[nv + i] : 0.0;
}
