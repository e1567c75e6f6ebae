// pipeline_contacts.h — the contact set of every robot's low-level QP from its own row of the simulator's contact rule (mpc_qp_contact_source,
// include/mpc_qp_contacts.h; the numpy mirror: mpc_benchmark_amd/contact_rule.py qp_contact_states / qp_contact_counts).  One step of the two device
// loops (mpc_qp_low_level_steps, mpc_qp_ikid_low_level_steps) with a source other than the schedule: before the QP assembly, every (robot, sole)
// reads the robot's two in_contact flags and its schedule pair and writes the QP's contact state, the log of it and one count.  The work per robot
// is a handful of compares: one lane per (robot, sole), 32 robots to a wavefront; each (b, c) has one writer and stream order serialises the steps:
// no atomics.  With the schedule as the source none of this is launched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mpc_qp_contacts.h"

struct PipeContactsArgs {
  const double* rows;     // [B][width] rows of the rule (include/mpc_sim_contacts.h): doubles 0, 1 are in_contact of soles 0, 1
  int width, B, source;   // MPC_QP_CONTACTS_PLANT or MPC_QP_CONTACTS_BOTH
  const int32_t* sched;   // [B][2] the caller's contact_states
  int32_t* cs;            // [B][2] contact states of the QP assembly
  int32_t* used;          // [B][2] log of cs (mpc_qp_contact_source_read)
  int32_t* counts;        // [B][2][4] counts[b][c][2 s + p]
};

// contact c of robot b
__device__ __forceinline__ void pipe_contact_state(const PipeContactsArgs& a, int b, int c) {
  const double* r = a.rows + (size_t)b * a.width;
  const int p0 = r[0] != 0.0, p1 = r[1] != 0.0;
  const int s0 = a.sched[2 * b] != 0, s1 = a.sched[2 * b + 1] != 0;
  const int pc = c ? p1 : p0, sc = c ? s1 : s0;
  int u = pc;
  if (a.source == MPC_QP_CONTACTS_BOTH && ((s0 & p0) | (s1 & p1))) u = sc & pc;  // (an empty intersection: the plant's set)
  a.cs[2 * b + c] = u;
  a.used[2 * b + c] = u;
  a.counts[(2 * b + c) * 4 + 2 * sc + pc] += 1;
}

// launch: ceil(2 B / 64) workgroups of 64
__global__ void __launch_bounds__(64) k_pipe_contact_states(PipeContactsArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < 2 * a.B) pipe_contact_state(a, i >> 1, i & 1);
}
