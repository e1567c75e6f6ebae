// sim_record.h — the per-step record of a torque-driven simulator handle (mpc_sim_record, include/mpc_sim_ext.h): after every simulator step of a
// handle with recording on, one wavefront per robot appends what the step left to the device ring, so that the 1 kHz response of the device loops
// (mpc_qp_low_level_steps, mpc_qp_ikid_low_level_steps) can be read without a host round trip per step.  The kinematics, centre of mass and
// centroidal momentum are those of body_kinematics.h.
#pragma once
#include "body_kinematics.h"

#define SIM_REC_TAIL 51  // doubles after x and tau: wrenches 12, com 3, momentum 6, soles 24, push 6
static inline __host__ __device__ int sim_record_width(int nx, int nu) { return nx + nu + SIM_REC_TAIL; }

struct SimRecordArgs {
  const int32_t* mi;    // model tables of the simulator handle (contacts 0 and 1: the two soles)
  const double* md;
  size_t md_stride;     // 0: one table for every robot; the plant model on (include/mpc_sim_plant.h): robot b's own table at md + b * md_stride
  int nq, nv;
  const double* x;      // [B][nq + nv] the states after the step
  const double* tau;    // [B][nv - 6] the joint torques of the step
  const double* wr;     // [B][2][6] the contact wrenches of the step (LOCAL frame)
  const double* push;   // the push armed for the step, or nullptr: [B][push_width]
  int push_width;
  double* out;          // [B][rec] this step's slot of the ring
};

// placement of the sole of contact c (contacts 0 and 1 of the model: left, right) in the bodies K: its body's placement times the contact placement
// (mpc_set_model contact table).  Shared with the metrics (sim_metrics.h).
DEV void sim_sole_placement(const int32_t* mi, const double* md, const CgBodies& K, int c, M3& Rc, V3& pc) {
  const int nj = mi[0], nframes = mi[3];
  const int i = mi[MPC_MODEL_HEADER_WORDS + MPC_MODEL_JOINT_WORDS * nj + nframes + c];
  const double* cm = md + MPC_MODEL_HEADER_DOUBLES + MPC_MODEL_JOINT_DOUBLES * nj + MPC_MODEL_FRAME_DOUBLES * nframes + MPC_MODEL_CONTACT_DOUBLES * c;
  const M3 Ri = ldm3(K.oR + 9 * i);
  Rc = mul(Ri, ldm3(cm));
  pc = mul(Ri, ldv3(cm + 9)) + ldv3(K.op + 3 * i);
}

// rec = [x | tau | wrenches (2 x 6) | com (3) | hg (linear, angular about the com) | soles (2 x (R row-major, p)) | push (f, p)]
__global__ void __launch_bounds__(CG_THREADS) k_sim_record(SimRecordArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, nx = a.nq + a.nv, nu = a.nv - 6;
  __shared__ CgBodies K;
  __shared__ double body[10 * CG_MAX_NJ];
  __shared__ double cx[CG_NC];
  const double* x = a.x + (size_t)b * nx;
  const double* md = a.md + (size_t)b * a.md_stride;
  cg_kinematics(a.mi, md, a.nq, x, K, tid);
  cg_centroidal(a.mi, md, K, body, cx, tid);
  double* o = a.out + (size_t)b * sim_record_width(nx, nu);
  for (int i = tid; i < nx; i += CG_THREADS) o[i] = x[i];
  o += nx;
  for (int i = tid; i < nu; i += CG_THREADS) o[i] = a.tau[(size_t)b * nu + i];
  o += nu;
  if (tid < 12) o[tid] = a.wr[(size_t)b * 12 + tid];
  if (tid < CG_NC) o[12 + tid] = cx[tid];
  o += 12 + CG_NC;
  if (tid < 2) {
    M3 Rc;
    V3 pc;
    sim_sole_placement(a.mi, md, K, tid, Rc, pc);
    double* so = o + 12 * tid;
    for (int e = 0; e < 9; ++e) so[e] = Rc.m[e];
    so[9] = pc.x; so[10] = pc.y; so[11] = pc.z;
  }
  o += 24;
  if (tid < 6) {  // width 3: the force acted at the base origin, recorded as the base position of x
    double pv = 0.0;
    if (a.push) pv = a.push_width == 6 ? a.push[(size_t)b * 6 + tid] : (tid < 3 ? a.push[(size_t)b * 3 + tid] : x[tid - 3]);
    o[tid] = pv;
  }
}
