// sim_foot_sensors.h — the per-robot foot force/torque sensors and contact detector of a torque-driven simulator handle (mpc_sim_foot_sensors,
// include/mpc_sim_foot_sensors.h): after every simulator step of a handle with the model on, one wavefront per robot takes the LOCAL-frame contact
// wrenches the step wrote ([2][6], 0 for a contact the step did not hold), pushes them into the robot's ring, measures the delayed wrench (constant
// offsets, noise), low-passes it, and runs a threshold detector with hysteresis and debounce counters on the two filtered normal forces.  Lanes 0 - 11
// take one wrench component each (ring slot, noise, filter); lanes 0 - 5 produce the six Philox blocks of each stream (two normals each; the sensor
// model's generator, sim_sensors.h, on streams it does not use); lane 0 does the scalar detector logic and the confusion counts.  The normals and the
// filtered wrench travel through LDS.  A launch is a chain of short dependent phases for a few hundred bytes per robot: its time is launch latency, as
// k_sim_contacts', and nothing here is tuned.  Plain fp64; one workgroup owns each row and stream order serialises the events: no atomics, ordinary
// vector stores.  The numpy mirror, the definition: mpc_benchmark_amd/foot_sensors.py.
#pragma once
#include "sim_sensors.h"
#include "../../include/mpc_sim_contacts.h"
#include "../../include/mpc_sim_foot_sensors.h"

#define SIM_FS_THREADS 64
// offsets in a state row: det[2] | above[2] | below[2] | wf[12] | wm[12] | counts[2][4] | ring[16][12] | head | count
#define SIM_FS_O_ABOVE 2
#define SIM_FS_O_BELOW 4
#define SIM_FS_O_WF 6
#define SIM_FS_O_WM 18
#define SIM_FS_O_COUNTS 30
#define SIM_FS_O_RING 38
#define SIM_FS_O_HEAD (SIM_FS_O_RING + 12 * MPC_SIM_FOOT_SENSORS_RING)
static_assert(SIM_FS_O_HEAD + 2 == MPC_SIM_FOOT_SENSORS_WIDTH, "the state row of the foot sensors");

struct SimFootSensorsArgs {
  const double* wr;      // [B][12] the wrenches of the step
  const double* con;     // [B][MPC_SIM_CONTACTS_WIDTH] the rows of the contact rule after the step (entries 0, 1: in_contact; the counts only)
  const double* params;  // [B][MPC_SIM_FOOT_SENSORS_PARAMS]
  double* rows;          // [B][MPC_SIM_FOOT_SENSORS_WIDTH]
  double dt;             // length of the step
};

__global__ void __launch_bounds__(SIM_FS_THREADS) k_sim_foot_sensors(SimFootSensorsArgs a) {
  __shared__ double n0[12], n1[12], zf[12];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int R = MPC_SIM_FOOT_SENSORS_RING;
  double* row = a.rows + (size_t)b * MPC_SIM_FOOT_SENSORS_WIDTH;
  double *ring = row + SIM_FS_O_RING, *hc = row + SIM_FS_O_HEAD;
  const double* p = a.params + (size_t)b * MPC_SIM_FOOT_SENSORS_PARAMS;
  const double delay = p[0], sf = p[1], sm = p[2], bf = p[3], bm = p[4], tc = p[5];
  const unsigned seed = (unsigned)(unsigned long long)p[10];
  // every lane reads head and count before lane 0 replaces them
  const int head = ((int)hc[0] + 1) & (R - 1);
  const double count = hc[1] + 1.0;
  __syncthreads();
  if (tid < 6) {
    if (sf != 0.0 || sm != 0.0) {
      const unsigned long long c = (unsigned long long)count;
      sim_sen_normal_pair(seed, (unsigned)c, (unsigned)(c >> 32), (unsigned)tid, 2u, n0[2 * tid], n0[2 * tid + 1]);
    }
    if (bf != 0.0 || bm != 0.0) sim_sen_normal_pair(seed, 0u, 0u, (unsigned)tid, 3u, n1[2 * tid], n1[2 * tid + 1]);
  }
  __syncthreads();
  if (tid < 12) {
    const double w = a.wr[(size_t)b * 12 + tid];
    const int back = (int)fmin(delay, count - 1.0);  // (the oldest wrench held while fewer than delay + 1 are)
    const int slot = (head - back) & (R - 1);
    const double wd = back == 0 ? w : ring[slot * 12 + tid];  // (slot != head then: written by an earlier event)
    ring[head * 12 + tid] = w;
    const bool force = (tid % 6) < 3;
    const double bias = force ? bf : bm, sigma = force ? sf : sm;
    double wm = wd;
    if (bias != 0.0) wm = wm + bias * n1[tid];
    if (sigma != 0.0) wm = wm + sigma * n0[tid];
    double wf = wm;
    if (tc != 0.0 && count != 1.0) {
      const double f0 = row[SIM_FS_O_WF + tid];
      wf = f0 + -expm1(-a.dt / tc) * (wm - f0);
    }
    row[SIM_FS_O_WM + tid] = wm;
    row[SIM_FS_O_WF + tid] = wf;
    zf[tid] = wf;
  }
  __syncthreads();
  if (tid == 0) {
    const double f_on = p[6], f_off = p[7], on_steps = p[8], off_steps = p[9];
    const double* t = a.con + (size_t)b * MPC_SIM_CONTACTS_WIDTH;
    double *above = row + SIM_FS_O_ABOVE, *below = row + SIM_FS_O_BELOW, *counts = row + SIM_FS_O_COUNTS;
    const double z[2] = {zf[2], zf[8]};
    bool det[2];
    double ab[2], be[2];
    for (int i = 0; i < 2; ++i) {
      det[i] = row[i] != 0.0;
      ab[i] = above[i];
      be[i] = below[i];
      if (!det[i]) {
        ab[i] = z[i] > f_on ? ab[i] + 1.0 : 0.0;
        if (ab[i] >= on_steps) { det[i] = true; ab[i] = be[i] = 0.0; }
      } else {
        be[i] = z[i] <= f_off ? be[i] + 1.0 : 0.0;
        if (be[i] >= off_steps) { det[i] = false; ab[i] = be[i] = 0.0; }
      }
    }
    if (!det[0] && !det[1]) {  // (never an empty set: the QPs need a contact, and the rule never releases the last one)
      const int k = z[1] > z[0] ? 1 : 0;
      det[k] = true;
      ab[k] = be[k] = 0.0;
    }
    for (int i = 0; i < 2; ++i) {
      row[i] = det[i] ? 1.0 : 0.0;
      above[i] = ab[i];
      below[i] = be[i];
      counts[4 * i + 2 * (t[i] != 0.0 ? 1 : 0) + (det[i] ? 1 : 0)] += 1.0;
    }
    hc[0] = (double)head;
    hc[1] = count;
  }
}
