// pipeline_ikid_glue.h — the kernels that string the centroidal control pipeline together on the device (mpc_qp_ikid_low_level_steps,
// include/mpc_qp_abi.h; centroidal_talos.py:353-468): the task errors of the IK + ID QP once per MPC period (talos_utils.py:375-402, mirror
// references.compute_ID_references), per low-level step the centroidal state of the measured robot (centre of mass, centroidal momentum about it)
// and the feedback forces of the plan's record in force ; the QP's torque goes on through k_pipe_torque (pipeline_glue.h).  One wavefront per robot (body_kinematics.h).
#pragma once
#include "body_kinematics.h"
#include "pipeline_glue.h"

#define CG_IK_DOUBLES(nv) (2 * (nv) + 42)  // task-error block of mpc_qp_solve_ikid

struct IkidGlueArgs {
  const int32_t* mi;  // model tables of the QP handle (mpc_qp_set_model)
  const double* md;
  int nq, nv, nk;
  PlanView plan;      // the centroidal MPC handle's (nx = n = CG_NC, m = 6 nk)
  // task errors (k_ikid_task_errors)
  const double* x_ik;    // [B][nq + nv] the measurement the errors are taken at
  const double* x_post;  // [nq + nv] posture reference
  const double* refs;    // [B][2 feet][2 samples][12] (R row-major, p)
  double ref_dt;
  int fr[4];             // model frame indices: left sole, right sole, base, torso
  double* ik;            // [B][2 nv + 42]
  // feedback (k_pipe_centroidal_feedback)
  const double* x;       // [B][nq + nv] measured states (the simulator handle's)
  double *xrob, *f;      // inputs of the QP assembly: state, forces [B][6 nk]
  double* c_prev;        // [B][9] new_x, written when `last` is set
  int last;
};

// Once per call: ik = [q_diff, dq_diff | LF e, de | RF e, de | base e, de | torso e, de | dH] at x_ik (references.compute_ID_references):
//   posture   d = - difference(x_posture, x_ik)
//   feet      e = [p_ref0 - p ; -log3(R_ref0^T R)],  de = [(p_ref1 - p_ref0) / dt - v_lin ; log3(R_ref0^T R_ref1) / dt - v_ang]   (LOCAL velocity)
//   base, torso  e = -log3(R_RFref0^T R),  de = log3(R_RFref0^T R_RFref1) / dt - v_ang
//   dH        xdot[3:9] of the plan's record in force (centroidal_talos.py:409): knot 0, or under HELD (include/mpc_plan_latency.h) the held record of
//             a robot whose first step of this call reads it ; the clock is not advanced here.
template <bool HELD> __global__ void __launch_bounds__(CG_THREADS) k_ikid_task_errors(IkidGlueArgs a, PlanLatencyArgs h) {
  const int b = blockIdx.x, tid = threadIdx.x, nq = a.nq, nv = a.nv, nx = nq + nv;
  __shared__ CgBodies K;
  const double* x = a.x_ik + (size_t)b * nx;
  cg_kinematics(a.mi, a.md, a.nq, x, K, tid);
  double* ik = a.ik + (size_t)b * CG_IK_DOUBLES(nv);
  const double* refs = a.refs + (size_t)b * 48;  // [foot][sample][12]
  const double idt = 1.0 / a.ref_dt;
  if (tid < 4) {  // one lane per task frame
    M3 Rc;
    V3 pc;
    S6 vl;
    cg_frame(a.mi, a.md, K, a.fr[tid], Rc, pc, vl);
    if (tid < 2) {
      const double *r0 = refs + 24 * tid, *r1 = r0 + 12;
      const M3 R0 = ldm3(r0), R1 = ldm3(r1);
      const V3 p0 = ldv3(r0 + 9), p1 = ldv3(r1 + 9);
      const V3 eo = log3(tmul(R0, Rc)), ro = log3(tmul(R0, R1));
      double* e = ik + 2 * nv + 12 * tid;
      e[0] = p0.x - pc.x; e[1] = p0.y - pc.y; e[2] = p0.z - pc.z;
      e[3] = -eo.x; e[4] = -eo.y; e[5] = -eo.z;
      e[6] = (p1.x - p0.x) * idt - vl.v[0]; e[7] = (p1.y - p0.y) * idt - vl.v[1]; e[8] = (p1.z - p0.z) * idt - vl.v[2];
      e[9] = ro.x * idt - vl.v[3]; e[10] = ro.y * idt - vl.v[4]; e[11] = ro.z * idt - vl.v[5];
    } else {
      const double *r0 = refs + 24, *r1 = r0 + 12;  // the right foot's reference rotation (talos_utils.py:392-400)
      const M3 R0 = ldm3(r0);
      const V3 eo = log3(tmul(R0, Rc)), yr = log3(tmul(R0, ldm3(r1)));
      double* e = ik + 2 * nv + 24 + 6 * (tid - 2);
      e[0] = -eo.x; e[1] = -eo.y; e[2] = -eo.z;
      e[3] = yr.x * idt - vl.v[3]; e[4] = yr.y * idt - vl.v[4]; e[5] = yr.z * idt - vl.v[5];
    }
  }
  // posture: difference(x0, x) = (q0 (-) q, v - v0), negated
  const int nj = a.mi[0];
  const int32_t* mj = a.mi + MPC_MODEL_HEADER_WORDS;
  const double* x0 = a.x_post;
  for (int j = tid; j < nj; j += CG_THREADS) {
    const int iq = mj[4 * j + 2], iv = mj[4 * j + 3];
    if (mj[4 * j + 1] == MPC_JOINT_FREEFLYER) {
      const M3 R0 = quat_to_rot(x0 + iq + 3), R1 = quat_to_rot(x + iq + 3);
      V3 ev, ew;
      log6(tmul(R0, R1), tmul(R0, v3(x[iq] - x0[iq], x[iq + 1] - x0[iq + 1], x[iq + 2] - x0[iq + 2])), ev, ew);
      ik[iv] = -ev.x; ik[iv + 1] = -ev.y; ik[iv + 2] = -ev.z; ik[iv + 3] = -ew.x; ik[iv + 4] = -ew.y; ik[iv + 5] = -ew.z;
    } else ik[iv] = -(x[iq] - x0[iq]);
  }
  for (int i = tid; i < nv; i += CG_THREADS) ik[nv + i] = -(x[nq + i] - x0[nq + i]);
  bool held;
  const PlanRecord r = plan_record_in_force<HELD>(a.plan, h, b, held);
  if (tid < 6) ik[2 * nv + 36 + tid] = r.xd[tid];
}

// Per step: new_x = [com ; hg] of the measured state, forces = u0 - K0 (x0 - new_x) (centroidal_talos.py:420-434) with (x0, u0, K0) the plan's record
// in force (knot 0, or under HELD — include/mpc_plan_latency.h — the held record of a robot whose hand-over latency has not run out), the QP inputs,
// and on the last step new_x into c_prev.
template <bool HELD> __global__ void __launch_bounds__(CG_THREADS) k_pipe_centroidal_feedback(IkidGlueArgs a, PlanLatencyArgs h) {
  const int b = blockIdx.x, tid = threadIdx.x, nx = a.nq + a.nv, nf = 6 * a.nk;
  __shared__ CgBodies K;
  __shared__ double body[10 * CG_MAX_NJ];
  __shared__ double cx[CG_NC];
  const double* x = a.x + (size_t)b * nx;
  cg_kinematics(a.mi, a.md, a.nq, x, K, tid);
  cg_centroidal(a.mi, a.md, K, body, cx, tid);
  bool held;
  const PlanRecord r = plan_record_in_force<HELD>(a.plan, h, b, held);
  for (int i = tid; i < nf; i += CG_THREADS) {
    double su = 0.0;
    for (int j = 0; j < CG_NC; ++j) su += r.K[i * CG_NC + j] * (r.x[j] - cx[j]);
    a.f[(size_t)b * nf + i] = r.u[i] - su;
  }
  for (int i = tid; i < nx; i += CG_THREADS) a.xrob[(size_t)b * nx + i] = x[i];
  if (a.last && tid < CG_NC) a.c_prev[(size_t)b * CG_NC + tid] = cx[tid];
  if (HELD) plan_latency_count(h, b, held, tid);
}
