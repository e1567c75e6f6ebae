/*
 * mpc_sim_friction.h — HIP-library-only addition to the C-ABI of include/mpc_abi.h: per-robot ground friction under the soles of a torque-driven
 * simulator handle.  A sole held by the contact rule (include/mpc_sim_contacts.h) transmits any tangential force and any yaw moment; with this model
 * on, each held sole of each robot is a Coulomb slider: when the tangential force of a step leaves the cone mu f_z the sole gets a slip velocity in
 * its contact's LOCAL frame, and the contact row of the dynamics becomes  acb + Kd (vcb - vs) - Kp e,  vs = (v_x, v_y, 0, 0, 0, w_z).  The contacts
 * carry Kp = 0 tangentially and in yaw: a sole is held there by velocity alone, so slip is a velocity the row is allowed to have, not a displaced
 * anchor.  Off by default; off launches and allocates nothing, and on with identity rows (mu = mu_spin = +inf) keeps every bit.
 *
 * The rule's numpy mirror, the definition the checks hold the kernel (csrc/sim_friction.h) to, is mpc_benchmark_amd/friction_model.py.  mpc_abi.h
 * lists what BOTH libraries export; the entry points here are exported by libmpc_hip.so alone.  Bindings look the symbols up before they use them
 * (mpc_benchmark_amd/_capi.py).  Every call takes the simulator handle of mpc_simulate_torque with the contact rule on, and returns 0, or -1 with the
 * reason in mpc_last_error (mpc_sim_friction_width: the width, or -1).
 */
#ifndef MPC_SIM_FRICTION_H
#define MPC_SIM_FRICTION_H

#include "mpc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One parameter row per robot; pairs are (left, right) = contacts (0, 1).
 *   0, 1   mu        Coulomb coefficient under each sole, >= 0; +inf: the sole never slides (the identity)
 *   2, 3   mu_spin   spinning coefficient (m): the yaw moment a sole transmits is at most mu_spin f_z; >= 0, +inf: never turns
 *   4      m_slip    added mass of the slider (kg), finite and > 0
 *   5      I_slip    its yaw counterpart (kg m^2), finite and > 0
 *   6      v_max     bound on the slip speed (m/s), finite and > 0
 *   7      w_max     bound on the yaw slip rate (rad/s), finite and > 0 */
#define MPC_SIM_FRICTION_PARAMS 8

/* One state row per robot.
 *   0 - 2   v_x, v_y, w_z of sole 0: its slip velocity in the contact's LOCAL frame, the one the NEXT step is integrated with
 *   3 - 5   the same of sole 1
 *   6, 7    sliding      1: a velocity of the sole is not 0
 *   8, 9    slip_steps   steps integrated with sliding = 1
 *  10, 11   slip_dist    sum of |v| dt over those steps (m)
 *  12, 13   slip_yaw     sum of |w_z| dt (rad)
 *  14, 15   peak_excess  largest |f| - mu f_z seen on a held sole of finite mu (N), 0 if none was positive
 *  16       steps        steps since the model was armed
 * The rule, once per step after the contact rule, on the step's LOCAL wrench w (ground on robot) of each sole, dt the step's length (substeps * dt):
 *   the step just integrated is accounted with the velocities it was integrated with: slip_steps, slip_dist, slip_yaw, and the sole's anchor in
 *   the contact rule's row:  p += R2 (v_x, v_y, 0) dt,  R2 <- Rz(w_z dt) R2.  Then, n = max(f_z, 0), f = (f_x, f_y), lim = mu n:
 *   sole free after the contact rule: v = 0, w_z = 0.
 *   mu = +inf: v = 0.  Else sticking (v == 0): if |f| > lim: v = -(dt / m_slip) (|f| - lim) f / |f|.
 *   sliding: v_new = v - (dt / m_slip) (f + lim v / |v|); dot(v_new, v) <= 0: v = 0, else v = v_new; then |v| is clamped to v_max.
 *   yaw: the same scalar law on w_z with the moment tau_z, lim_s = mu_spin n, I_slip and w_max.
 *   sliding = (v != 0 or w_z != 0). */
#define MPC_SIM_FRICTION_WIDTH 17

/* params[B][MPC_SIM_FRICTION_PARAMS]: the model on and reset (every state row 0); NULL: off (frees the rows).  Refused: the contact rule off
 * (mpc_sim_contacts first), a NaN or negative mu or mu_spin, m_slip, I_slip, v_max or w_max not finite and > 0.  A refused call leaves the
 * configuration in force.  mpc_sim_contacts(sim, NULL) drops the model, as it drops the terrain. */
int mpc_sim_friction(mpc_solver* sim, const double* params);

/* Impose state[B][MPC_SIM_FRICTION_WIDTH] (restore rows read earlier, or impose slip velocities).  Refused: a non-finite entry, a sliding flag other
 * than 0 or 1, a negative count, distance, excess or step number, a velocity on a sole whose flag is 0.  Synchronises the handle. */
int mpc_sim_friction_set(mpc_solver* sim, const double* state);

/* Copy the rows in force to params[B][MPC_SIM_FRICTION_PARAMS] and the state rows to state[B][MPC_SIM_FRICTION_WIDTH] (either may be NULL;
 * synchronises the handle's stream). */
int mpc_sim_friction_read(mpc_solver* sim, double* params, double* state);

int32_t mpc_sim_friction_width(mpc_solver* sim);

#ifdef __cplusplus
}
#endif
#endif
