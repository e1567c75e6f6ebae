/*
 * mpc_qp_pipeline.h — HIP-library-only additions to the C-ABI of include/mpc_qp_abi.h.
 *
 * mpc_qp_abi.h lists what BOTH libraries export (the product libmpc_hip.so and the checker libmpc_oracle.so, tests/test_abi_library.py); the
 * entry points here are exported by libmpc_hip.so alone.  Their checker side is host glue built from calls both libraries have
 * (mpc_qp_solve_ikid, mpc_simulate_torque: mpc_benchmark_amd/pipeline.py CentroidalPipeline.tick(host_glue=True)).  Bindings look the
 * symbol up before they use it (mpc_benchmark_amd/_qp_capi.py).
 */
#ifndef MPC_QP_PIPELINE_H
#define MPC_QP_PIPELINE_H

#include "mpc_qp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- device-side glue of the centroidal control pipeline (centroidal_talos.py:408-447) ----
 * `steps` periods of the 1 kHz low-level loop of the centroidal script for every robot of the batch, without the host in between.
 * Once per call, on the device: the task errors of the IK + ID QP (talos_utils.py:375-402; the layout `ik` of mpc_qp_solve_ikid) at x_ik, from
 * x_posture, this period's two foot reference samples and ref_dt; dH = xdot[3:9] of the plan's knot 0 (centroidal_talos.py:408-409).  Per period:
 *     new_x   = [ com(q) ; hg.linear ; hg.angular ]  of the measured state (momentum about the centre of mass)       :420-424
 *     forces  = us[0] - K_0 (xs[0] - new_x)                                                                        :434
 *     (a, df, tau) = the IK + ID QP of mpc_qp_solve_ikid at (x_measured, ik, forces, contact_states)               :435-446
 *     x_measured <- one simulator step of length dt under tau (no clamp: the QP's torque box is the limit)          :447 (device.execute)
 * `plan`: the MPC handle of the centroidal problem (MPC_SPACE_VECTOR, nx = 9, controls = 6 nk contact wrench components); xs[0], us[0], K_0 and
 * xdot of knot 0 are read where the last run left them.  `sim`: the simulator handle as in mpc_qp_low_level_steps.  The three handles live on
 * one device and share the batch size; nk = 2.  frames, base_frame, torso_frame, weights, gains, cone, l_box, u_box as in mpc_qp_solve_ikid.
 * x_posture[nq+nv]: the posture reference (x0_multibody); foot_refs[B][2 feet][2 samples][12] (R row-major, p): LF_refs[0:2], RF_refs[0:2] of
 * this period (NULL on a plan with mpc_walk_poses_init: the samples its generator keeps on the device, include/mpc_walk_poses.h; an error on any
 * other plan); ref_dt: the dt of the rate terms (the MPC's).  x[B][nq+nv]: the states to start from (NULL: the simulator handle's).
 * x_ik[B][nq+nv]: the measurement the task errors are taken at (NULL: the x_prev the last call kept on the device).  Outputs (each may be NULL):
 * x_prev[B][nq+nv] the measured states BEFORE the last period, c_prev[B][9] their new_x (the next solve's x0, :454-458), x_out[B][nq+nv] after it,
 * tau[B][nv-6] and forces[B][6 nk] (= forces + df) of the last period, info[B] of its QP, ik_out[B][2 nv + 42] the task errors used. */
int mpc_qp_ikid_low_level_steps(mpc_qp_solver* s, const mpc_qp_settings* settings, mpc_solver* plan, mpc_solver* sim, int32_t nk, const int32_t* frames,
                                int32_t base_frame, int32_t torso_frame, const double* weights, const double* gains, const double* cone, const double* l_box,
                                const double* u_box, const double* x_posture, const double* foot_refs, double ref_dt, const int32_t* contact_states,
                                const double* x, const double* x_ik, int32_t steps, double dt, double* x_prev, double* c_prev, double* x_out, double* tau,
                                double* forces, mpc_qp_info* info, double* ik_out);

#ifdef __cplusplus
}
#endif
#endif
