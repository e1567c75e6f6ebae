// sim_tipping.h — per-robot sole tipping in a torque-driven simulator handle (mpc_sim_tipping, include/mpc_sim_tipping.h): after every simulator
// step of a handle with the model on, directly after the contact rule and friction, one lane per (robot, sole) takes the sole's LOCAL contact wrench
// of the step and the sole's in_contact flag as the rule left it, and updates the sole's tip velocity (v_z, w_x, w_y): a sole whose roll or pitch
// moment leaves h f_z rolls about the edge where the CoP saturates, with the added inertia I_tip.  The next step's stage kernel
// (k_eval_multibody<2>) holds the sole to that velocity instead of to rest, in the three components friction (sim_friction.h) leaves at zero.  The
// lane first accounts the step just integrated with the velocity it was integrated with: the angles, the counters, and the sole's anchor in the
// contact rule's row (Kp_z acts on the anchor's height, and a sole rotating about an edge raises its origin).  No kinematics, no LDS, no cross-lane
// traffic: a lane reads and writes the entries of its own sole only (lane 0 of a robot also the step count), stream order serialises the steps: no
// atomics, ordinary vector stores.  A launch moves a few hundred bytes: its time is launch latency and nothing here is tuned.  The numpy mirror, the
// definition: mpc_benchmark_amd/tipping_model.py.
#pragma once
#include "../../include/mpc_sim_contacts.h"
#include "../../include/mpc_sim_tipping.h"

#define SIM_TP_THREADS 64
// offsets in a state row: (v_z, w_x, w_y)[2] | (th_x, th_y)[2] | tipping[2] | tip_steps[2] | peak_angle[2] | peak_excess[2] | landings[2] | steps
#define SIM_TP_O_TH 6
#define SIM_TP_O_TIPPING 10
#define SIM_TP_O_STEPS 12
#define SIM_TP_O_ANGLE 14
#define SIM_TP_O_EXCESS 16
#define SIM_TP_O_LANDINGS 18
#define SIM_TP_O_COUNT 20
static_assert(SIM_TP_O_COUNT + 1 == MPC_SIM_TIPPING_WIDTH, "the state row of the tipping model");

struct SimTippingArgs {
  int B;
  const double* wr;      // [B][2][6] the wrenches of the step (LOCAL frame, ground on robot; 0 for a free sole)
  double* con;           // [B][MPC_SIM_CONTACTS_WIDTH] the rows of the contact rule after the step and friction: in_contact read, the anchors advanced
  const double* params;  // [B][MPC_SIM_TIPPING_PARAMS]
  double* rows;          // [B][MPC_SIM_TIPPING_WIDTH]
  double dt;             // length of the step
};

__device__ inline double sim_tipping_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

// the accounting of one axis over the step just integrated: the angle advances, and an angle that reaches or crosses 0 is a landing
__device__ inline void sim_tipping_advance(double& th, double& w, double dt, double& landings) {
  const double old = th;
  th = old + w * dt;
  if (old != 0.0 && th * old <= 0.0) { th = 0.0; w = 0.0; landings += 1.0; }
}

// the law of one axis of a held sole of finite extent h: the rate w under the moment tau with the limit lim = h n; `peak` keeps the largest excess
__device__ inline void sim_tipping_axis(double& w, double th, double tau, double lim, double k, double wmax, double thmax, double& peak) {
  if (th == 0.0 && w == 0.0) {
    const double excess = fabs(tau) - lim;
    if (excess > peak) peak = excess;
    if (excess > 0.0) w = -k * excess * sim_tipping_sign(tau);
  } else {
    const double s = th != 0.0 ? sim_tipping_sign(th) : sim_tipping_sign(w);
    w = w - k * (tau + s * lim);
  }
  if (fabs(w) > wmax) w = wmax * sim_tipping_sign(w);
  if (fabs(th) >= thmax && w * th > 0.0) w = 0.0;
}

__global__ void __launch_bounds__(SIM_TP_THREADS) k_sim_tipping(SimTippingArgs a) {
  const int idx = blockIdx.x * SIM_TP_THREADS + threadIdx.x;
  if (idx >= 2 * a.B) return;
  const int b = idx >> 1, i = idx & 1;
  const double* p = a.params + (size_t)b * MPC_SIM_TIPPING_PARAMS;
  double* r = a.rows + (size_t)b * MPC_SIM_TIPPING_WIDTH;
  double* c = a.con + (size_t)b * MPC_SIM_CONTACTS_WIDTH;
  const double* w = a.wr + (size_t)b * 12 + 6 * i;
  const double dt = a.dt;
  double vz = r[3 * i], wx = r[3 * i + 1], wy = r[3 * i + 2];
  double thx = r[SIM_TP_O_TH + 2 * i], thy = r[SIM_TP_O_TH + 2 * i + 1];
  // the step just integrated, with the velocities it was integrated with (a sole at rest: nothing is touched, so identity rows keep every bit)
  if (wx != 0.0 || wy != 0.0) {
    r[SIM_TP_O_STEPS + i] += 1.0;
    double* an = c + 8 + 12 * i;  // R2 (row-major, 9), p2 (3)
    an[9] += an[2] * (vz * dt);
    an[10] += an[5] * (vz * dt);
    an[11] += an[8] * (vz * dt);
    // R2 <- R2 Exp((wx, wy, 0) dt), Rodrigues: E = I + sa K + sc K K, K the cross-product matrix of (ax, ay, 0)
    const double ax = wx * dt, ay = wy * dt, t2 = ax * ax + ay * ay;
    if (t2 != 0.0) {  // (an angle whose square underflows: the identity)
      const double t = sqrt(t2);
      const double sa = sin(t) / t, sc = (1.0 - cos(t)) / t2;
      const double e00 = 1.0 - sc * ay * ay, e01 = sc * ax * ay, e02 = sa * ay;
      const double e11 = 1.0 - sc * ax * ax, e12 = -sa * ax, e22 = 1.0 - sc * t2;
      for (int k = 0; k < 3; ++k) {
        const double r0 = an[3 * k], r1 = an[3 * k + 1], r2 = an[3 * k + 2];
        an[3 * k] = r0 * e00 + r1 * e01 - r2 * e02;
        an[3 * k + 1] = r0 * e01 + r1 * e11 - r2 * e12;
        an[3 * k + 2] = r0 * e02 + r1 * e12 + r2 * e22;
      }
    }
    double landings = r[SIM_TP_O_LANDINGS + i];
    sim_tipping_advance(thx, wx, dt, landings);
    sim_tipping_advance(thy, wy, dt, landings);
    r[SIM_TP_O_LANDINGS + i] = landings;
    const double peak = fmax(r[SIM_TP_O_ANGLE + i], fmax(fabs(thx), fabs(thy)));
    r[SIM_TP_O_ANGLE + i] = peak;
  }
  // the velocities of the next step
  if (c[i] == 0.0) {
    vz = wx = wy = thx = thy = 0.0;
  } else {
    const double n = fmax(w[2], 0.0), L = p[i], W = p[2 + i], k = dt / p[4], wmax = p[5], thmax = p[6];
    double peak = r[SIM_TP_O_EXCESS + i];
    if (isinf(W)) wx = 0.0;
    else sim_tipping_axis(wx, thx, w[3], W * n, k, wmax, thmax, peak);
    if (isinf(L)) wy = 0.0;
    else sim_tipping_axis(wy, thy, w[4], L * n, k, wmax, thmax, peak);
    r[SIM_TP_O_EXCESS + i] = peak;
    // the origin's velocity when the sole turns about the carrying edge (an axis at rest adds nothing: its extent may be +inf)
    vz = 0.0;
    if (wx != 0.0) vz += (thx != 0.0 ? sim_tipping_sign(thx) : sim_tipping_sign(wx)) * W * wx;
    if (wy != 0.0) vz += (thy != 0.0 ? sim_tipping_sign(thy) : sim_tipping_sign(wy)) * L * wy;
  }
  r[3 * i] = vz; r[3 * i + 1] = wx; r[3 * i + 2] = wy;
  r[SIM_TP_O_TH + 2 * i] = thx; r[SIM_TP_O_TH + 2 * i + 1] = thy;
  r[SIM_TP_O_TIPPING + i] = (wx != 0.0 || wy != 0.0 || thx != 0.0 || thy != 0.0) ? 1.0 : 0.0;
  if (i == 0) r[SIM_TP_O_COUNT] += 1.0;
}
