// sim_estimator.h — the per-robot base-state estimator of a torque-driven simulator handle (mpc_sim_estimator, include/mpc_sim_estimator.h): after
// every simulator step of a handle with the estimator on, one wavefront per robot takes the measured state (the sensor model's measurement, or the
// true state), runs the kinematics of the measured joints and orientation with the base at the origin and at rest, and replaces the base position
// and the base linear velocity by a blend of the measurement and of leg odometry through the soles the contact rule holds.  The ESTIMATE goes into
// the robot's state row and into the contiguous [B][nx] buffer the controllers of the device loops read.  Lanes stride over the state index (nx = 77
// of the complete model takes a second pass); the kinematics are those of body_kinematics.h (one body per lane), the sole
// placements the record's (sim_record.h); lanes 0 and 1 take one sole each, the rule itself is lane 0's scalar work.  A launch is a chain of short
// dependent phases for a few hundred bytes per robot: its time is latency, as k_sim_contacts'.  Plain fp64; one workgroup owns each row and stream
// order serialises the events: no atomics.  The numpy mirror, the definition: mpc_benchmark_amd/state_estimator.py.
#pragma once
#include "sim_record.h"
#include "../../include/mpc_sim_contacts.h"
#include "../../include/mpc_sim_estimator.h"

#define SIM_EST_MAX_NX (2 * (CG_MAX_NJ + 5) + 1)  // a floating base and CG_MAX_NJ - 1 one-dof joints

struct SimEstimatorArgs {
  const int32_t* mi;     // model tables of the simulator handle (contacts 0 and 1: the two soles)
  const double* md;
  int nq, nv;
  const double* xm;      // [B][nq + nv] the measured states
  const double* xt;      // [B][nq + nv] the true states (statistics only)
  const double* con;     // [B][con_width] the rows of the contact rule after the step (entries 0, 1: in_contact), or the rows of the contact
  int con_width;         // detector after this step's detection event (entries 0, 1: det) when it feeds the estimator (mpc_sim_foot_sensors_feed)
  const double* params;  // [B][MPC_SIM_ESTIMATOR_PARAMS]
  double* xe;            // [B][nq + nv] out: the estimate the controllers read
  double* rows;          // [B][nx + 17]: est[nx] | held[2] | anchor[2][3] | stats[8] | count
};

__global__ void __launch_bounds__(CG_THREADS) k_sim_estimator(SimEstimatorArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, nq = a.nq, nv = a.nv, nx = nq + nv;
  __shared__ CgBodies K;
  __shared__ double xk[SIM_EST_MAX_NX];
  __shared__ double sole[2][6];  // r_i, u_i
  __shared__ double hat[6];      // p_hat, v_hat
  const double* xm = a.xm + (size_t)b * nx;
  for (int e = tid; e < nx; e += CG_THREADS) xk[e] = (e < 3 || (e >= nq && e < nq + 3)) ? 0.0 : xm[e];
  __syncthreads();
  cg_kinematics(a.mi, a.md, nq, xk, K, tid);
  if (tid < 2) {
    M3 Rc;
    V3 pc;
    sim_sole_placement(a.mi, a.md, K, tid, Rc, pc);
    const int nj = a.mi[0], nframes = a.mi[3];
    const int body = a.mi[MPC_MODEL_HEADER_WORDS + MPC_MODEL_JOINT_WORDS * nj + nframes + tid];
    const S6 vo = ld6(K.ov + 6 * body);  // the body's spatial velocity at the world origin: the point moves with v_O + omega x r
    const V3 u = v3(vo.v[0], vo.v[1], vo.v[2]) + cross(v3(vo.v[3], vo.v[4], vo.v[5]), pc);
    sole[tid][0] = pc.x; sole[tid][1] = pc.y; sole[tid][2] = pc.z;
    sole[tid][3] = u.x; sole[tid][4] = u.y; sole[tid][5] = u.z;
  }
  __syncthreads();
  double* row = a.rows + (size_t)b * (nx + MPC_SIM_ESTIMATOR_TAIL);
  if (tid == 0) {
    const double* p = a.params + (size_t)b * MPC_SIM_ESTIMATOR_PARAMS;
    const double* c = a.con + (size_t)b * a.con_width;
    const double* xt = a.xt + (size_t)b * nx;
    double *held = row + nx, *anchor = held + 2, *stats = anchor + 6, *cnt = stats + 8;
    const double w_p = p[0], w_v = p[1], count = cnt[0] + 1.0;
    const V3 p_m = v3(xm[0], xm[1], xm[2]), v_m = v3(xm[nq], xm[nq + 1], xm[nq + 2]);
    const V3 r[2] = {ldv3(sole[0]), ldv3(sole[1])}, u[2] = {ldv3(sole[0] + 3), ldv3(sole[1] + 3)};
    bool on[2], kept[2];
    for (int i = 0; i < 2; ++i) {
      on[i] = c[i] != 0.0;
      kept[i] = on[i] && held[i] != 0.0 && count > 1.0;
    }
    V3 p_odo = p_m, v_odo = v_m;
    if (kept[0] && kept[1]) p_odo = 0.5 * ((ldv3(anchor) - r[0]) + (ldv3(anchor + 3) - r[1]));
    else if (kept[0]) p_odo = ldv3(anchor) - r[0];
    else if (kept[1]) p_odo = ldv3(anchor + 3) - r[1];
    if (on[0] || on[1]) {
      const V3 um = (on[0] && on[1]) ? 0.5 * (u[0] + u[1]) : (on[0] ? u[0] : u[1]);
      const V3 t = tmul(quat_to_rot(xk + 3), um);
      v_odo = v3(-t.x, -t.y, -t.z);
    }
    const V3 p_hat = (w_p == 0.0) ? p_m : p_m + w_p * (p_odo - p_m);
    const V3 v_hat = (w_v == 0.0) ? v_m : v_m + w_v * (v_odo - v_m);
    for (int i = 0; i < 2; ++i) {
      double* an = anchor + 3 * i;
      V3 n = ldv3(an);
      if (kept[i]) {
        if (w_p == 1.0) continue;
        n = n + (p_hat - p_odo);
      } else if (on[i]) {
        n = p_hat + r[i];
      } else {
        continue;
      }
      an[0] = n.x; an[1] = n.y; an[2] = n.z;
    }
    held[0] = c[0]; held[1] = c[1];
    hat[0] = p_hat.x; hat[1] = p_hat.y; hat[2] = p_hat.z;
    hat[3] = v_hat.x; hat[4] = v_hat.y; hat[5] = v_hat.z;
    if (count > 1.0) {
      const V3 p_t = v3(xt[0], xt[1], xt[2]), v_t = v3(xt[nq], xt[nq + 1], xt[nq + 2]);
      const V3 dp[2] = {p_hat - p_t, p_m - p_t}, dv[2] = {v_hat - v_t, v_m - v_t};
      for (int k = 0; k < 2; ++k) {
        const double ep = dot(dp[k], dp[k]), ev = dot(dv[k], dv[k]);
        double* s = stats + 4 * k;
        s[0] += ep;
        s[1] += ev;
        s[2] = fmax(s[2], sqrt(ep));
        s[3] = fmax(s[3], sqrt(ev));
      }
    }
    cnt[0] = count;
  }
  __syncthreads();
  double* xe = a.xe + (size_t)b * nx;
  for (int e = tid; e < nx; e += CG_THREADS) {
    const double v = (e < 3) ? hat[e] : ((e >= nq && e < nq + 3) ? hat[3 + e - nq] : xm[e]);
    row[e] = v;
    xe[e] = v;
  }
}
