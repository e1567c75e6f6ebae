// sim_disturbances.h — the per-robot push schedule of a torque-driven simulator handle (mpc_sim_disturbances, include/mpc_sim_disturbances.h):
// before every simulator step of a handle with the model on, one wavefront per robot advances that robot's disturbance clock, compares the
// in_contact pair of the contact rule's row with the pair it saw the step before (touchdowns, lift-offs), picks the active event of lowest index
// and writes what acts in the step: world force and world point into out[b][6], the link into link[b] (-1: nothing).  The step's stage kernel
// (k_eval_multibody<2>) reads the two in place of the armed push and applies the wrench on the dofs below that link.  The clock, the transitions
// and the pick are one lane's scalar work (the numpy mirror: mpc_benchmark_amd/disturbance_model.py); the forward kinematics
// (body_kinematics.h) run only when the acting event has a body-fixed frame, a branch the whole workgroup takes together.  One workgroup owns
// each row and stream order serialises the steps: plain stores, no atomics.
#pragma once
#include "body_kinematics.h"
#include "../../include/mpc_sim_contacts.h"
#include "../../include/mpc_sim_disturbances.h"

// offsets of the state row (include/mpc_sim_disturbances.h)
enum : int { SIM_DIS_O_STEP = 0, SIM_DIS_O_ACTING = 1, SIM_DIS_O_OCC = 2, SIM_DIS_O_FIRE = 6, SIM_DIS_O_IMPULSE = 14, SIM_DIS_O_PUSHED = 17,
             SIM_DIS_O_SHADOWED = 18, SIM_DIS_O_PEAK = 19, SIM_DIS_O_APPLIED = 20, SIM_DIS_O_LINK = 26, SIM_DIS_O_SEEN = 27 };

struct SimDisturbancesArgs {
  const int32_t* mi;     // model tables of the simulator handle
  const double* md;
  int nq, nv;
  const double* x;       // [B][nq + nv] the states the step starts from
  const double* con;     // [B][MPC_SIM_CONTACTS_WIDTH] the rows of the contact rule as the step before left them, or nullptr: the rule is off
  const double* events;  // [B][n_events][MPC_SIM_DISTURBANCES_EVENT]
  int n_events;
  double* rows;          // [B][MPC_SIM_DISTURBANCES_WIDTH]
  double* out;           // [B][6] world force, world point of the step
  int32_t* link;         // [B] the link they act on, -1: nothing acts
  double dt;             // length of the step (substeps * dt)
};

__global__ void __launch_bounds__(CG_THREADS) k_sim_disturbances(SimDisturbancesArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, ne = a.n_events;
  __shared__ CgBodies K;
  __shared__ int pick[2];  // the acting event (-1: none) and its step index
  const double* ev = a.events + (size_t)b * ne * MPC_SIM_DISTURBANCES_EVENT;
  double* r = a.rows + (size_t)b * MPC_SIM_DISTURBANCES_WIDTH;
  if (tid == 0) {
    const double t = r[SIM_DIS_O_STEP];
    if (a.con) {  // transitions of the soles: the pair of the rule's row against the pair of the step before
      const double* c = a.con + (size_t)b * MPC_SIM_CONTACTS_WIDTH;
      for (int i = 0; i < 2; ++i) {
        const double now = c[i] != 0.0 ? 1.0 : 0.0, was = r[SIM_DIS_O_SEEN + i];
        r[SIM_DIS_O_SEEN + i] = now;
        if (was < 0.0 || now == was) continue;  // (the sentinel: the first pair is taken without counting)
        const int which = 2 * i + (now > was ? 0 : 1);  // trigger - 2
        const double n = r[SIM_DIS_O_OCC + which] + 1.0;
        r[SIM_DIS_O_OCC + which] = n;
        for (int e = 0; e < ne; ++e) {
          const double* v = ev + MPC_SIM_DISTURBANCES_EVENT * e;
          if ((int)v[0] != which + 2 || n < v[1]) continue;
          if (n == v[1] || (v[4] > 0.0 && fmod(n - v[1], v[4]) == 0.0)) r[SIM_DIS_O_FIRE + e] = t + v[2];
        }
      }
    }
    int acting = -1, kstep = 0, shadowed = 0;
    for (int e = 0; e < ne; ++e) {
      const double* v = ev + MPC_SIM_DISTURBANCES_EVENT * e;
      const int trig = (int)v[0];
      double k = -1.0;
      if (trig == 1) {
        const double u = t - v[1] - v[2];
        if (u >= 0.0) k = v[4] > 0.0 ? fmod(u, v[4]) : u;
      } else if (trig >= 2 && r[SIM_DIS_O_FIRE + e] >= 0.0) {
        k = t - r[SIM_DIS_O_FIRE + e];
      }
      if (k < 0.0 || k >= v[3]) continue;
      if (acting < 0) { acting = e; kstep = (int)k; }
      else ++shadowed;
    }
    r[SIM_DIS_O_SHADOWED] += (double)shadowed;
    pick[0] = acting;
    pick[1] = kstep;
  }
  __syncthreads();
  const int e = pick[0];
  const double* v = ev + MPC_SIM_DISTURBANCES_EVENT * (e < 0 ? 0 : e);
  const bool body_fixed = e >= 0 && (v[7] != 0.0 || v[8] != 0.0);
  if (body_fixed) cg_kinematics(a.mi, a.md, a.nq, a.x + (size_t)b * (a.nq + a.nv), K, tid);  // (uniform in the workgroup)
  if (tid != 0) return;
  double* o = a.out + (size_t)b * 6;
  V3 f = v3(0, 0, 0), p = v3(0, 0, 0);
  int link = -1;
  if (e >= 0) {
    link = (int)v[6];
    const double w = v[5] != 0.0 ? sin(M_PI * ((double)pick[1] + 0.5) / v[3]) : 1.0;
    f = v3(w * v[9], w * v[10], w * v[11]);
    p = v3(v[12], v[13], v[14]);
    if (body_fixed) {
      const M3 R = ldm3(K.oR + 9 * link);
      if (v[7] != 0.0) f = mul(R, f);
      if (v[8] != 0.0) p = mul(R, p) + ldv3(K.op + 3 * link);
    }
    r[SIM_DIS_O_IMPULSE] += f.x * a.dt; r[SIM_DIS_O_IMPULSE + 1] += f.y * a.dt; r[SIM_DIS_O_IMPULSE + 2] += f.z * a.dt;
    r[SIM_DIS_O_PUSHED] += 1.0;
    r[SIM_DIS_O_PEAK] = fmax(r[SIM_DIS_O_PEAK], sqrt(f.x * f.x + f.y * f.y + f.z * f.z));
  }
  o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = p.x; o[4] = p.y; o[5] = p.z;
  a.link[b] = link;
  for (int i = 0; i < 6; ++i) r[SIM_DIS_O_APPLIED + i] = o[i];
  r[SIM_DIS_O_LINK] = (double)link;
  r[SIM_DIS_O_ACTING] = (double)e;
  r[SIM_DIS_O_STEP] += 1.0;
}
