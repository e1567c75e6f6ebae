/*
 * mpc_sim_ext.h — HIP-library-only additions to the C-ABI of include/mpc_abi.h: a push on the base and a per-step device record for the
 * torque-driven simulator (mpc_simulate_torque, and the simulator step inside mpc_qp_low_level_steps / mpc_qp_ikid_low_level_steps).
 *
 * mpc_abi.h lists what BOTH libraries export (tests/test_abi_library.py); the entry points here are exported by libmpc_hip.so alone.  Their
 * checks use physics (the momentum law of a pushed step) and host glue (mpc_simulate_torque one step at a time) instead of the checker library.
 * Bindings look the symbols up before they use them (mpc_benchmark_amd/_capi.py).
 *
 * Every call takes the simulator handle of mpc_simulate_torque: whole-body contact dynamics (stage 0 set) with nu = nv - 6.  They return 0, or -1
 * with the reason in mpc_last_error (mpc_sim_record_width: the width, or -1).
 */
#ifndef MPC_SIM_EXT_H
#define MPC_SIM_EXT_H

#include "mpc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Arm a push on a simulator handle, per robot, held for every torque-driven simulator step of this handle (mpc_simulate_torque, and the
 * simulator step inside mpc_qp_low_level_steps / mpc_qp_ikid_low_level_steps) until re-armed; NULL disarms (width is then ignored).
 *   width 3: f_ext[B][3], a world-frame force at the base origin (mpc_simulate_push's convention: the point moves with the base);
 *   width 6: f_ext[B][6] = (world-frame force, fixed world-frame point it acts at), as PyBullet's applyExternalForce(..., WORLD_FRAME): the moment
 *            (p - p_base) x f about the base origin is taken at the base position of every sub-step.  At p = p_base it is the width-3 push.
 * This push acts on the base link and is held until the host arms another; a per-robot schedule of pushes on any link, timed on the device, is
 * include/mpc_sim_disturbances.h (while one is on, a non-NULL push is refused here).  mpc_simulate and mpc_simulate_push (the feedback-law form) do not see it.  The upload is synchronous on
 * the handle's stream. */
int mpc_sim_set_push(mpc_solver* sim, const double* f_ext, int32_t width);

/* Record every torque-driven simulator step of this handle into a device ring of `cap` steps (0: off, frees the ring; a new cap empties it).
 * A step that would not fit fails its call before anything is enqueued (nothing is dropped): read the ring, or make it larger.  With recording
 * off no record kernel is launched.  One record per robot and step (per call of mpc_simulate_torque, whatever its substeps), rec doubles:
 *     [0, nx)                      x after the step (nx = nq + nv)
 *     [nx, nx + nu)                the joint torques of the step (nu = nv - 6)
 *     [+0, +12)                    contact wrenches [2][6] of the step, LOCAL frame of the contact, 0 for a contact the stage does not hold
 *     [+12, +15)                   centre of mass of x
 *     [+15, +21)                   centroidal momentum of x about the centre of mass, world axes: linear, then angular
 *     [+21, +45)                   the two soles (contacts 0 and 1 of the model): R row-major (9), p (3)
 *     [+45, +51)                   the push that acted: (force, world point); width 3: the point is the base position of x; unarmed: 0
 * rec = nx + nu + 51 (mpc_sim_record_width). */
int mpc_sim_record(mpc_solver* sim, int32_t cap);

/* Copy the recorded steps (oldest first) to out[count][B][rec], rec = mpc_sim_record_width(sim); *count = steps held; clears the ring.
 * out == NULL: only *count, nothing is copied or cleared. */
int mpc_sim_record_read(mpc_solver* sim, double* out, int32_t* count);

int32_t mpc_sim_record_width(mpc_solver* sim);

#ifdef __cplusplus
}
#endif
#endif
