// sim_contacts.h — the unilateral foot-contact rule of a torque-driven simulator handle (mpc_sim_contacts, include/mpc_sim_contacts.h): after every
// simulator step of a handle with the rule on, one wavefront per robot takes the sole heights of the state the step left and the step's LOCAL
// contact wrenches, and updates that robot's row: which soles are held, and where the ground side of each lies.  The next step's stage kernel
// (k_eval_multibody<2>) integrates the contacts of that row.  The kinematics are those of body_kinematics.h, the sole
// placements the record's (sim_record.h); the rule itself is one lane's scalar work, BulletRobot._update_contacts in its order (the numpy mirror:
// mpc_benchmark_amd/contact_rule.py).  One workgroup owns each row and stream order serialises the steps: no atomics.  With a terrain
// (mpc_sim_terrain, sim_terrain.h) the ground under each sole is the height function at the sole's origin: lanes 0 - 31 test the 2 x 16 boxes they
// loaded before the kinematics and reduce with max; the scalar rule then runs on g_0, g_1 in place of ground_z.
#pragma once
#include "sim_record.h"
#include "sim_terrain.h"
#include "../../include/mpc_sim_contacts.h"

struct SimContactsArgs {
  const int32_t* mi;    // model tables of the simulator handle (contacts 0 and 1: the two soles)
  const double* md;
  int nq, nv;
  const double* x;      // [B][nq + nv] the states after the step
  const double* wr;     // [B][2][6] the contact wrenches of the step (LOCAL frame; 0 for a free sole)
  mpc_sim_contacts_config cfg;
  double* rows;         // [B][MPC_SIM_CONTACTS_WIDTH] (include/mpc_sim_contacts.h)
  SimTerrain ter;       // boxes nullptr: the ground is the plane z = cfg.ground_z
};

__global__ void __launch_bounds__(CG_THREADS) k_sim_contacts(SimContactsArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, nx = a.nq + a.nv;
  __shared__ CgBodies K;
  __shared__ double sole[2][12];
  const double* x = a.x + (size_t)b * nx;
  TerrainBox bx = {};
  if (a.ter.boxes) bx = terrain_load_box(a.ter, b, tid);  // (one branch for the whole launch)
  cg_kinematics(a.mi, a.md, a.nq, x, K, tid);
  if (tid < 2) {
    M3 Rc;
    V3 pc;
    sim_sole_placement(a.mi, a.md, K, tid, Rc, pc);
    for (int e = 0; e < 9; ++e) sole[tid][e] = Rc.m[e];
    sole[tid][9] = pc.x; sole[tid][10] = pc.y; sole[tid][11] = pc.z;
  }
  __syncthreads();
  const mpc_sim_contacts_config& c = a.cfg;
  // the ground under the two soles: the plane, or the terrain at the soles' origins (lanes 0 - 15 sole 0, 16 - 31 sole 1; 32 - 63 repeat them)
  double g[2] = {c.ground_z, c.ground_z};
  if (a.ter.boxes) {
    const int i = (tid / TERRAIN_GROUP) & 1;
    const double gi = terrain_height(bx, sole[i][9], sole[i][10], c.ground_z);
    g[0] = __shfl(gi, 0);
    g[1] = __shfl(gi, TERRAIN_GROUP);
  }
  if (tid != 0) return;
  double* r = a.rows + (size_t)b * MPC_SIM_CONTACTS_WIDTH;
  const double* w = a.wr + (size_t)b * 12;
  const double n = r[40];
  for (int i = 0; i < 2; ++i) {
    const double z = sole[i][11];
    if (r[i] != 0.0) {
      r[4 + i] = (w[6 * i + 2] < -c.release_force) ? r[4 + i] + 1.0 : 0.0;
      if (r[4 + i] >= (double)c.release_steps && r[0] + r[1] > 1.0) {  // (the other sole's flag as it stands: foot 0's release counts for foot 1)
        r[i] = 0.0; r[2 + i] = 0.0; r[4 + i] = 0.0;
        r[34 + i] += 1.0;
        r[38 + i] = n;
      }
    } else if (z > g[i] + 2.0 * c.ground_tol) {
      r[2 + i] = 1.0;
    } else if ((z <= g[i] + c.ground_tol && r[2 + i] != 0.0) || (z < g[i] && z < r[6 + i])) {
      // caught: the anchor is the landing pose flattened onto the ground under the sole's origin, Rz(yaw) at (x, y, g_i)
      const double yaw = atan2(sole[i][3], sole[i][0]), cy = cos(yaw), sy = sin(yaw);
      double* an = r + 8 + 12 * i;
      an[0] = cy; an[1] = -sy; an[2] = 0.0;
      an[3] = sy; an[4] = cy;  an[5] = 0.0;
      an[6] = 0.0; an[7] = 0.0; an[8] = 1.0;
      an[9] = sole[i][9]; an[10] = sole[i][10]; an[11] = g[i];
      r[i] = 1.0;
      r[32 + i] += 1.0;
      r[36 + i] = n;
    }
    r[6 + i] = z;
  }
  r[40] = n + 1.0;
}
