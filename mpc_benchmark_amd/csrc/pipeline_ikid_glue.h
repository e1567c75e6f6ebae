// pipeline_ikid_glue.h — the kernels that string the centroidal control pipeline together on the device (mpc_qp_ikid_low_level_steps,
// include/mpc_qp_abi.h; centroidal_talos.py:353-468): the task errors of the IK + ID QP once per MPC period (talos_utils.py:375-402, mirror
// references.compute_ID_references), per low-level step the centroidal state of the measured robot (centre of mass, centroidal momentum about it)
// and the feedback forces of the plan's knot 0, and the QP's torque into the simulator step.  One workgroup of one wavefront per robot: the
// kinematics of ~30 bodies, one body per lane, and vectors of a few hundred bytes.
#pragma once
#include "solver_args.h"
#include "plan_latency.h"

#define CG_THREADS 64
#define CG_MAX_NJ 64        // moving joints of the model (one lane each)
#define CG_NC 9             // centroidal state [com ; h_lin ; h_ang]
#define CG_IK_DOUBLES(nv) (2 * (nv) + 42)  // task-error block of mpc_qp_solve_ikid

struct IkidGlueArgs {
  const int32_t* mi;  // model tables of the QP handle (mpc_qp_set_model)
  const double* md;
  int nq, nv;
  // the plan (centroidal MPC handle): solution of knot 0, its Riccati gain, xdot of its stage data
  const double *xs, *us, *gains, *knots;
  int N, m, gain_stride, oK, knot_stride, oXD, slot0;
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
  // torque (k_pipe_ikid_torque)
  const double* sol;     // [B][qn] (a, df, tau)
  int nk, qn;
  double* sim_u;         // [B][nv - 6]
  double* f_new;         // [B][6 nk] forces + df
  const int32_t* used;   // [B][nk] contact set the QP worked with (pipeline_contacts.h), or nullptr: the caller's contact_states, f_new as it is
};

struct CgBodies {  // LDS of the kinematics: per body local and world placement, spatial velocity at the world origin
  double lR[9 * CG_MAX_NJ], lp[3 * CG_MAX_NJ], oR[9 * CG_MAX_NJ], op[3 * CG_MAX_NJ], ov[6 * CG_MAX_NJ];
};

// world-frame column of dof `loc` of joint i (placement R, p): free-flyer translations move along the body axes, rotations about the axis through p
DEV S6 cg_col(int kind, int loc, const M3& R, V3 p) {
  if (kind == MPC_JOINT_FREEFLYER && loc < 3) return mk6(v3(R.m[loc], R.m[3 + loc], R.m[6 + loc]), v3(0, 0, 0));
  const int ax = (kind == MPC_JOINT_FREEFLYER) ? loc - 3 : kind - MPC_JOINT_RX;
  const V3 w = v3(R.m[ax], R.m[3 + ax], R.m[6 + ax]);
  return mk6(cross(p, w), w);
}

// forward kinematics with velocities of the state x = (q, v): every body's oR, op and ov (lane i: body i).  mi, md: model tables
// (mpc_set_model / mpc_qp_set_model layout); the helpers below are shared with the simulator record (sim_record.h).
DEV void cg_kinematics(const int32_t* mi, const double* md, int nq, const double* x, CgBodies& K, int tid) {
  const int nj = mi[0];
  const int32_t* mj = mi + MPC_MODEL_HEADER_WORDS;
  const double* jd = md + MPC_MODEL_HEADER_DOUBLES;
  const double *q = x, *v = x + nq;
  for (int i = tid; i < nj; i += CG_THREADS) {
    const int kind = mj[4 * i + 1], iq = mj[4 * i + 2];
    const M3 Rp = ldm3(jd + 25 * i);
    const V3 pp = ldv3(jd + 25 * i + 9);
    M3 Rl;
    V3 pl = pp;
    if (kind == MPC_JOINT_FREEFLYER) {
      Rl = mul(Rp, quat_to_rot(q + iq + 3));
      pl = mul(Rp, v3(q[iq], q[iq + 1], q[iq + 2])) + pp;
    } else {
      const double th = q[iq], c = cos(th), s = sin(th);
      const int ax = kind - MPC_JOINT_RX, b1 = (ax + 1) % 3, b2 = (ax + 2) % 3;
      M3 Rj;
      for (int e = 0; e < 9; ++e) Rj.m[e] = (e % 4 == 0) ? 1.0 : 0.0;
      Rj.m[3 * b1 + b1] = c; Rj.m[3 * b1 + b2] = -s; Rj.m[3 * b2 + b1] = s; Rj.m[3 * b2 + b2] = c;
      Rl = mul(Rp, Rj);
    }
    for (int e = 0; e < 9; ++e) K.lR[9 * i + e] = Rl.m[e];
    K.lp[3 * i] = pl.x; K.lp[3 * i + 1] = pl.y; K.lp[3 * i + 2] = pl.z;
  }
  __syncthreads();
  for (int i = tid; i < nj; i += CG_THREADS) {
    M3 R = ldm3(K.lR + 9 * i);
    V3 p = ldv3(K.lp + 3 * i);
    for (int j = mj[4 * i]; j >= 0; j = mj[4 * j]) { const M3 Rj = ldm3(K.lR + 9 * j); p = mul(Rj, p) + ldv3(K.lp + 3 * j); R = mul(Rj, R); }
    for (int e = 0; e < 9; ++e) K.oR[9 * i + e] = R.m[e];
    K.op[3 * i] = p.x; K.op[3 * i + 1] = p.y; K.op[3 * i + 2] = p.z;
  }
  __syncthreads();
  for (int i = tid; i < nj; i += CG_THREADS) {
    S6 vi = zero6();
    for (int j = i; j >= 0; j = mj[4 * j]) {
      const int kind = mj[4 * j + 1], iv = mj[4 * j + 3], nd = (kind == MPC_JOINT_FREEFLYER) ? 6 : 1;
      const M3 Rj = ldm3(K.oR + 9 * j);
      const V3 pj = ldv3(K.op + 3 * j);
      for (int d = 0; d < nd; ++d) vi = add6(vi, scale6(v[iv + d], cg_col(kind, d, Rj, pj)));
    }
    st6(K.ov + 6 * i, vi);
  }
  __syncthreads();
}

// placement (R, p) and LOCAL velocity of model frame fi
DEV void cg_frame(const int32_t* mi, const double* md, const CgBodies& K, int fi, M3& Rc, V3& pc, S6& vl) {
  const int nj = mi[0];
  const int i = mi[MPC_MODEL_HEADER_WORDS + MPC_MODEL_JOINT_WORDS * nj + fi];
  const double* fd = md + MPC_MODEL_HEADER_DOUBLES + MPC_MODEL_JOINT_DOUBLES * nj + MPC_MODEL_FRAME_DOUBLES * fi;
  const M3 Ri = ldm3(K.oR + 9 * i);
  Rc = mul(Ri, ldm3(fd));
  pc = mul(Ri, ldv3(fd + 9)) + ldv3(K.op + 3 * i);
  vl = adinv(Rc, pc, ld6(K.ov + 6 * i));
}

// Once per call: ik = [q_diff, dq_diff | LF e, de | RF e, de | base e, de | torso e, de | dH] at x_ik (references.compute_ID_references):
//   posture   d = - difference(x_posture, x_ik)
//   feet      e = [p_ref0 - p ; -log3(R_ref0^T R)],  de = [(p_ref1 - p_ref0) / dt - v_lin ; log3(R_ref0^T R_ref1) / dt - v_ang]   (LOCAL velocity)
//   base, torso  e = -log3(R_RFref0^T R),  de = log3(R_RFref0^T R_RFref1) / dt - v_ang
//   dH        xdot[3:9] of the plan's knot 0 (centroidal_talos.py:409)
// HELD (include/mpc_plan_latency.h): dH from the held record of a robot whose first step of this call reads it ; the clock is not advanced here.
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
  if (HELD) {
    if (plan_latency_in_force(h, b)) {  // (the record keeps xdot[3 .. 9) behind K_1)
      if (tid < 6) ik[2 * nv + 36 + tid] = h.held[(size_t)b * h.W + CG_NC + a.m + (size_t)a.m * CG_NC + tid];
      return;
    }
  }
  if (tid < 6) ik[2 * nv + 36 + tid] = a.knots[((size_t)b * (a.N + 1) + a.slot0) * a.knot_stride + a.oXD + 3 + tid];
}

// centroidal state of the bodies K: cx = [com ; hg.linear ; hg.angular] (Pinocchio's hg: momentum about the centre of mass, world axes).
// body: LDS scratch of 10 doubles per body (m c, linear momentum, angular momentum about the origin, m).  Ends with a barrier.
DEV void cg_centroidal(const int32_t* mi, const double* md, const CgBodies& K, double* body, double* cx, int tid) {
  const int nj = mi[0];
  const double* jd = md + MPC_MODEL_HEADER_DOUBLES;
  for (int i = tid; i < nj; i += CG_THREADS) {
    const M3 R = ldm3(K.oR + 9 * i);
    const double mass = jd[25 * i + 12];
    const V3 c = mul(R, ldv3(jd + 25 * i + 13)) + ldv3(K.op + 3 * i);
    const S6 vo = ld6(K.ov + 6 * i);
    const V3 w = ang(vo), vc = lin(vo) + cross(w, c), l = mass * vc;
    const V3 Iw = mul(R, mul(ldm3(jd + 25 * i + 16), tmul(R, w)));  // R I R^T w
    const V3 h = cross(c, l) + Iw;
    double* o = body + 10 * i;
    o[0] = mass * c.x; o[1] = mass * c.y; o[2] = mass * c.z; o[3] = l.x; o[4] = l.y; o[5] = l.z; o[6] = h.x; o[7] = h.y; o[8] = h.z; o[9] = mass;
  }
  __syncthreads();
  if (tid == 0) {
    double s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < nj; ++i) for (int e = 0; e < 10; ++e) s[e] += body[10 * i + e];
    const V3 com = v3(s[0] / s[9], s[1] / s[9], s[2] / s[9]), L = v3(s[3], s[4], s[5]);
    const V3 A = v3(s[6], s[7], s[8]) - cross(com, L);
    cx[0] = com.x; cx[1] = com.y; cx[2] = com.z; cx[3] = L.x; cx[4] = L.y; cx[5] = L.z; cx[6] = A.x; cx[7] = A.y; cx[8] = A.z;
  }
  __syncthreads();
}

// Per step: new_x = [com ; hg] of the measured state, forces = us[0] - K_0 (xs[0] - new_x) (centroidal_talos.py:420-434), the QP inputs, and on the
// last step new_x into c_prev.
// HELD (include/mpc_plan_latency.h): a robot whose hand-over latency has not run out takes xs, us and K from its held record (knot 1 of the plan
// before) instead; then one lane advances its clock.
template <bool HELD> __global__ void __launch_bounds__(CG_THREADS) k_pipe_centroidal_feedback(IkidGlueArgs a, PlanLatencyArgs h) {
  const int b = blockIdx.x, tid = threadIdx.x, nx = a.nq + a.nv, nf = 6 * a.nk;
  __shared__ CgBodies K;
  __shared__ double body[10 * CG_MAX_NJ];
  __shared__ double cx[CG_NC];
  const double* x = a.x + (size_t)b * nx;
  cg_kinematics(a.mi, a.md, a.nq, x, K, tid);
  cg_centroidal(a.mi, a.md, K, body, cx, tid);
  const double* xs0 = a.xs + (size_t)b * (a.N + 1) * CG_NC;
  const double* us0 = a.us + (size_t)b * a.N * a.m;
  const double* K0 = a.gains + (size_t)b * (a.N + 1) * a.gain_stride + a.oK;
  bool held = false;
  if (HELD) {
    held = plan_latency_in_force(h, b);
    if (held) { xs0 = h.held + (size_t)b * h.W; us0 = xs0 + CG_NC; K0 = us0 + a.m; }
  }
  for (int i = tid; i < nf; i += CG_THREADS) {
    double su = 0.0;
    for (int j = 0; j < CG_NC; ++j) su += K0[i * CG_NC + j] * (xs0[j] - cx[j]);
    a.f[(size_t)b * nf + i] = us0[i] - su;
  }
  for (int i = tid; i < nx; i += CG_THREADS) a.xrob[(size_t)b * nx + i] = x[i];
  if (a.last && tid < CG_NC) a.c_prev[(size_t)b * CG_NC + tid] = cx[tid];
  if (HELD) plan_latency_count(h, b, held, tid);
}

// the QP's torque into the simulator's input (no clamp: the QP's torque box is the limit, centroidal_talos.py:435-447) ; forces + df (with `used`: 0 for a
// contact the QP did not use)
__global__ void __launch_bounds__(CG_THREADS) k_pipe_ikid_torque(IkidGlueArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, nv = a.nv, nf = 6 * a.nk, nu = nv - 6;
  const double* sol = a.sol + (size_t)b * a.qn;
  for (int i = tid; i < nu; i += CG_THREADS) a.sim_u[(size_t)b * nu + i] = sol[nv + nf + i];
  if (!a.used) {
    for (int i = tid; i < nf; i += CG_THREADS) a.f_new[(size_t)b * nf + i] = a.f[(size_t)b * nf + i] + sol[nv + i];
    return;
  }
  for (int i = tid; i < nf; i += CG_THREADS) a.f_new[(size_t)b * nf + i] = a.used[(size_t)b * a.nk + i / 6] ? a.f[(size_t)b * nf + i] + sol[nv + i] : 0.0;
}
