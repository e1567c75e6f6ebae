// body_kinematics.h — the whole-body kinematics one wavefront computes for one robot in LDS, one body per lane: every body's world placement and
// spatial velocity (cg_kinematics), a frame's placement and local velocity (cg_frame), centre of mass and centroidal momentum (cg_centroidal).  Shared by
// the centroidal pipeline's glue (pipeline_ikid_glue.h) and the simulator's kernels (sim_record.h, sim_metrics.h, sim_contacts.h, sim_estimator.h, sim_disturbances.h).
#pragma once
#include "solver_args.h"

#define CG_THREADS 64
#define CG_MAX_NJ 64        // moving joints of the model (one lane each)
#define CG_NC 9             // centroidal state [com ; h_lin ; h_ang]

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

// forward kinematics with velocities of the state x = (q, v): every body's oR, op and ov (lane i: body i).  mi, md: model tables (mpc_set_model / mpc_qp_set_model layout)
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
