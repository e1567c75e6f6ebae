// sim_metrics.h — the locomotion metrics of a torque-driven simulator handle (mpc_sim_metrics, include/mpc_sim_metrics.h): after every simulator
// step of a handle with metrics on, one wavefront per robot folds what the step left into that robot's row of accumulators, so that plot.py's
// evaluation of a run (centre of pressure against the support box, angular momentum, joint power and energy) and a fall verdict are read once at the
// end instead of downloading the per-step record.  The kinematics, centre of mass and centroidal momentum are those of body_kinematics.h
// (one body per lane), the sole placements the record's (sim_record.h).  One workgroup owns each row and stream order serialises the steps: no
// atomics, and the same sums in the same order on every run.  On a handle with a terrain (mpc_sim_terrain, sim_terrain.h) the heights of the fall
// verdict are taken above the ground: a sole's above the terrain under its origin, the base's above the mean anchor height of the soles in contact.
#pragma once
#include "sim_record.h"
#include "sim_terrain.h"
#include "../../include/mpc_sim_metrics.h"
#include "../../include/mpc_sim_contacts.h"

struct SimMetricsArgs {
  const int32_t* mi;    // model tables of the simulator handle (contacts 0 and 1: the two soles)
  const double* md;
  size_t md_stride;     // 0: one table for every robot; the plant model on (include/mpc_sim_plant.h): robot b's own table at md + b * md_stride
  int nq, nv;
  const double* x;      // [B][nq + nv] the states after the step
  const double* tau;    // [B][nv - 6] the joint torques of the step
  const double* wr;     // [B][2][6] the contact wrenches of the step (LOCAL frame)
  double dt;            // length of the step (substeps * dt of the call)
  mpc_sim_metrics_config cfg;
  double* acc;          // [B][MPC_SIM_METRICS_WIDTH] the rows (include/mpc_sim_metrics.h)
  double* frozen;       // [B] 1 after a non-finite state: the row no longer changes
  double* xs;           // [B][nq + nv] the state the step started from; left holding x for the next step
  SimTerrain ter;       // boxes nullptr: no terrain, absolute heights in the fall verdict
  const double* con;    // with a terrain: [B][MPC_SIM_CONTACTS_WIDTH] the rows of the contact rule the step was integrated with
  double ground_z;      // with a terrain: the rule's ground_z
};

__global__ void __launch_bounds__(CG_THREADS) k_sim_metrics(SimMetricsArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, nq = a.nq, nx = a.nq + a.nv, nu = a.nv - 6;
  if (a.frozen[b] != 0.0) return;  // (one value for the whole workgroup, before any barrier)
  __shared__ CgBodies K;
  __shared__ double body[10 * CG_MAX_NJ];
  __shared__ double cx[CG_NC];
  __shared__ double sole[2][12];
  const double* x = a.x + (size_t)b * nx;
  double* xs = a.xs + (size_t)b * nx;
  double* r = a.acc + (size_t)b * MPC_SIM_METRICS_WIDTH;
  TerrainBox bx = {};
  if (a.ter.boxes) bx = terrain_load_box(a.ter, b, tid);  // (one branch for the whole launch)
  // joint power sum_j |tau_j v_j| with v of the state the step started from (plot.py pairs u[i] with x[i]), reduced over the wavefront
  double p = 0.0;
  for (int j = tid; j < nu; j += CG_THREADS) p += fabs(a.tau[(size_t)b * nu + j] * xs[nq + 6 + j]);
  for (int off = CG_THREADS / 2; off > 0; off >>= 1) p += __shfl_xor(p, off, CG_THREADS);
  int bad = 0;
  for (int i = tid; i < nx; i += CG_THREADS) bad |= !isfinite(x[i]);
  bad = __syncthreads_or(bad);  // (also the barrier between the reads of xs above and the writes below)
  if (bad) {  // fallen at this step; the row freezes without it
    if (tid == 0) {
      if (r[11] < 0.0) r[11] = r[0];
      a.frozen[b] = 1.0;
    }
    return;
  }
  for (int i = tid; i < nx; i += CG_THREADS) xs[i] = x[i];
  const double* md = a.md + (size_t)b * a.md_stride;
  cg_kinematics(a.mi, md, nq, x, K, tid);
  cg_centroidal(a.mi, md, K, body, cx, tid);
  if (tid < 2) {
    M3 Rc;
    V3 pc;
    sim_sole_placement(a.mi, md, K, tid, Rc, pc);
    for (int e = 0; e < 9; ++e) sole[tid][e] = Rc.m[e];
    sole[tid][9] = pc.x; sole[tid][10] = pc.y; sole[tid][11] = pc.z;
  }
  __syncthreads();
  // with a terrain: the ground under the two soles' origins (lanes 0 - 15 sole 0, 16 - 31 sole 1), as the contact rule takes it
  double g0 = 0.0, g1 = 0.0;
  if (a.ter.boxes) {
    const int i = (tid / TERRAIN_GROUP) & 1;
    const double gi = terrain_height(bx, sole[i][9], sole[i][10], a.ground_z);
    g0 = __shfl(gi, 0);
    g1 = __shfl(gi, TERRAIN_GROUP);
  }
  if (tid != 0) return;
  const mpc_sim_metrics_config& c = a.cfg;
  const double n = r[0];
  const V3 pl = ldv3(sole[0] + 9), pr = ldv3(sole[1] + 9);
  // the heights of the fall rule: absolute, or above the ground (the base above the mean anchor height of the soles in contact; there is always one)
  double zb = x[2], zl = pl.z, zr = pr.z;
  if (a.ter.boxes) {
    const double* cr = a.con + (size_t)b * MPC_SIM_CONTACTS_WIDTH;
    const double al = cr[8 + 11], ar = cr[20 + 11];
    zb -= (cr[0] != 0.0 && cr[1] != 0.0) ? 0.5 * (al + ar) : (cr[0] != 0.0 ? al : ar);
    zl -= g0;
    zr -= g1;
  }
  if (n == 0.0) {  // the first step since the reset: the heights of the fall rule, the centre of mass the run starts from
    r[12] = zb; r[13] = zl; r[14] = zr;
    r[15] = cx[0]; r[16] = cx[1]; r[17] = cx[2];
  }
  r[0] = n + 1.0;
  r[1] += a.dt;
  r[2] += a.dt * p;
  if (p > r[3]) r[3] = p;
  // centre of pressure (talos_utils.computeCoP): per loaded sole (-tau_y / f_z, tau_x / f_z, 0) moved to the world, weighted by f_z
  const double* w = a.wr + (size_t)b * 12;
  const bool lf = w[2] > c.min_force, rf = w[8] > c.min_force;
  if (lf || rf) {
    V3 tot = v3(0.0, 0.0, 0.0);
    double fs = 0.0;
    for (int s = 0; s < 2; ++s) {
      const double* ws = w + 6 * s;
      const double fz = ws[2];
      if (!(fz > c.min_force)) continue;
      tot = tot + fz * (mul(ldm3(sole[s]), v3(-ws[4] / fz, ws[3] / fz, 0.0)) + ldv3(sole[s] + 9));
      fs += fz;
    }
    const double px = tot.x / fs, py = tot.y / fs;
    // plot.py:145-164: both soles loaded, the box spanning them; one sole, its own box
    double xlo, xhi, ylo, yhi;
    if (lf && rf) {
      xlo = fmin(pl.x, pr.x) - c.half_length; xhi = fmax(pl.x, pr.x) + c.half_length;
      ylo = pr.y - c.half_width; yhi = pl.y + c.half_width;
    } else {
      const V3 q = lf ? pl : pr;
      xlo = q.x - c.half_length; xhi = q.x + c.half_length;
      ylo = q.y - c.half_width; yhi = q.y + c.half_width;
    }
    const double mg = fmin(fmin(px - xlo, xhi - px), fmin(py - ylo, yhi - py));
    if (r[4] == 0.0 || mg < r[6]) r[6] = mg;
    r[4] += 1.0;
    if (mg < 0.0) r[5] += 1.0;
    r[7] += mg;
  }
  const double hl = sqrt(cx[3] * cx[3] + cx[4] * cx[4] + cx[5] * cx[5]), ha = sqrt(cx[6] * cx[6] + cx[7] * cx[7] + cx[8] * cx[8]);
  if (hl > r[8]) r[8] = hl;
  if (ha > r[9]) r[9] = ha;
  r[10] += cx[8] * cx[8];
  if (r[11] < 0.0 && (zb < r[12] - c.fall_drop || (zl > r[13] + c.sole_lift && zr > r[14] + c.sole_lift))) r[11] = n;
  r[18] = cx[0]; r[19] = cx[1]; r[20] = cx[2];
}
