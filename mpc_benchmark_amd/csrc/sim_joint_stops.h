// sim_joint_stops.h — the per-robot joint end-stops of a torque-driven simulator handle (mpc_sim_joint_stops, include/mpc_sim_joint_stops.h):
// before the dynamics of every simulator step of a handle with the model on, one wavefront per robot takes the joint positions and velocities of
// the TRUE state the step starts from and the torque the actuators apply (the step's torque buffer, after the actuator model), advances the robot's
// state row and writes into a buffer of the model's own what the dynamics integrate: the applied torque plus the stop torque where a stop acts, the
// applied torque copied (no add: every bit kept) elsewhere.  The step's torque buffer is only read: the record, the metrics and the `tau` of the
// loops keep the actuators' torque.  One lane per joint (a loop beyond 64 joints); the parts of a row are contiguous in the joint index, so a
// wavefront's loads and stores coalesce.  Plain fp64, no LDS; the one cross-lane value is a wave vote (did any stop act); one workgroup of one
// wavefront owns each row and stream order serialises the steps: no atomics.  The numpy mirror, the definition: mpc_benchmark_amd/joint_stops.py.
#pragma once
#include "../../include/mpc_sim_joint_stops.h"

#define SIM_JS_THREADS 64  // one wavefront: the vote below spans the workgroup

struct SimJointStopsArgs {
  int nq, nv, nu;
  const double* x;       // [B][nq + nv] the true states the step starts from
  const double* tau;     // [B][nu] the torque the actuators apply
  const double* params;  // [B][MPC_SIM_JOINT_STOPS_PARAMS]
  const double* lo;      // [B][nu]
  const double* hi;      // [B][nu]
  const double* scale;   // [nu]
  double* out;           // [B][nu] what the dynamics integrate
  double* rows;          // [B][5 nu + 2]: tau_stop[nu] | pen[nu] | peak_pen[nu] | stop_steps[nu] | hits[nu] | any_steps | steps
};

__global__ void __launch_bounds__(SIM_JS_THREADS) k_sim_joint_stops(SimJointStopsArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, nu = a.nu;
  double* row = a.rows + (size_t)b * ((size_t)5 * nu + 2);
  double *tau_stop = row, *pen = row + nu, *peak = pen + nu, *stop_steps = peak + nu, *hits = stop_steps + nu, *tail = hits + nu;
  const double* p = a.params + (size_t)b * MPC_SIM_JOINT_STOPS_PARAMS;
  const double k = p[0], d = p[1], cap = p[2];
  const double* q = a.x + (size_t)b * (a.nq + a.nv) + 7;
  const double* v = a.x + (size_t)b * (a.nq + a.nv) + a.nq + 6;
  const double *lo = a.lo + (size_t)b * nu, *hi = a.hi + (size_t)b * nu, *tau = a.tau + (size_t)b * nu;
  double* out = a.out + (size_t)b * nu;
  int acted = 0;
  for (int j = tid; j < nu; j += SIM_JS_THREADS) {
    const double qj = q[j], vj = v[j], lj = lo[j], hj = hi[j], u = tau[j];
    double pj = 0.0, ts = 0.0;
    if (qj > hj) {
      pj = qj - hj;
      const double t = fmax(0.0, k * pj + d * vj);
      if (t > 0.0) ts = -(a.scale[j] * fmin(t, cap));
    } else if (qj < lj) {
      pj = qj - lj;
      const double t = fmax(0.0, k * (lj - qj) - d * vj);
      if (t > 0.0) ts = a.scale[j] * fmin(t, cap);
    }
    if (pj != 0.0 && pen[j] == 0.0) hits[j] += 1.0;
    if (ts != 0.0) {
      stop_steps[j] += 1.0;
      acted = 1;
    }
    tau_stop[j] = ts;
    pen[j] = pj;
    peak[j] = fmax(peak[j], fabs(pj));
    out[j] = ts != 0.0 ? u + ts : u;
  }
  const int any = __any(acted);
  if (tid == 0) {
    if (any) tail[0] += 1.0;
    tail[1] += 1.0;
  }
}
