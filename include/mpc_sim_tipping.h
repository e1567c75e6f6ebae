/*
 * mpc_sim_tipping.h — HIP-library-only addition to the C-ABI of include/mpc_abi.h: per-robot sole tipping in a torque-driven simulator handle.  A
 * sole held by the contact rule (include/mpc_sim_contacts.h) transmits any roll or pitch moment: the contacts carry Kp = 0 and Kd = 50 there, so the
 * plant never tests the bound the controllers plan with, the centre of pressure inside the sole.  With this model on, each held sole of each robot is
 * a rectangle |x| <= L, |y| <= W in its contact's LOCAL frame: when the roll or pitch moment of a step leaves W f_z or L f_z the sole starts to roll
 * about the edge where the CoP saturates, and the contact row of the dynamics becomes  acb + Kd (vcb - vs) - Kp e,
 * vs = friction's (v_x, v_y, 0, 0, 0, w_z) + (0, 0, v_z, w_x, w_y, 0)  (the ground-friction header: disjoint components; either model alone or both).
 * Off by default; off launches and allocates nothing, and on with identity rows (every extent +inf) keeps every bit.
 *
 * The rule's numpy mirror, the definition the checks hold the kernel (csrc/sim_tipping.h) to, is mpc_benchmark_amd/tipping_model.py.  mpc_abi.h
 * lists what BOTH libraries export; the entry points here are exported by libmpc_hip.so alone.  Bindings look the symbols up before they use them
 * (mpc_benchmark_amd/_capi.py).  Every call takes the simulator handle of mpc_simulate_torque with the contact rule on, and returns 0, or -1 with the
 * reason in mpc_last_error (mpc_sim_tipping_width: the width, or -1).
 */
#ifndef MPC_SIM_TIPPING_H
#define MPC_SIM_TIPPING_H

#include "mpc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One parameter row per robot; pairs are (left, right) = contacts (0, 1).
 *   0, 1   half_length  L of each sole (m), >= 0; +inf: the sole never pitches (the identity, by an explicit isinf test)
 *   2, 3   half_width   W of each sole (m), >= 0; +inf: the sole never rolls
 *   4      I_tip        added inertia of the slider (kg m^2), finite and > 0
 *   5      w_max        bound on a rate (rad/s), finite and > 0
 *   6      th_max       bound on an angle (rad), finite and > 0
 *   7      reserved     must be 0 */
#define MPC_SIM_TIPPING_PARAMS 8

/* One state row per robot.
 *   0 - 2   v_z, w_x, w_y of sole 0: its tip velocity in the contact's LOCAL frame, the one the NEXT step is integrated with
 *   3 - 5   the same of sole 1
 *   6 - 9   th_x, th_y of sole 0, then of sole 1: the accumulated angles; the sign says which edge carries the sole
 *           (th_x > 0: y = -W, th_x < 0: y = +W, th_y > 0: x = +L, th_y < 0: x = -L)
 *  10, 11   tipping      1: a rate or an angle of the sole is not 0
 *  12, 13   tip_steps    steps integrated with a rate that is not 0
 *  14, 15   peak_angle   largest |th_x|, |th_y| seen (rad)
 *  16, 17   peak_excess  largest |tau| - h f_z seen on a flat held sole of finite extent (N m), 0 if none was positive
 *  18, 19   landings     tips that ended with the sole flat again
 *  20       steps        steps since the model was armed
 * The rule, once per step after the contact rule and after friction, on the step's LOCAL wrench w = (f, tau) (ground on robot) of each sole, dt the
 * step's length (substeps * dt), n = max(f_z, 0); the axes are roll (h = W, tau_x) and pitch (h = L, tau_y):
 *   the step just integrated is accounted if w_x or w_y is not 0: tip_steps + 1; per axis th_a += w_a dt, and if th_a was not 0 before and
 *   th_a_new th_a_old <= 0 the sole has landed on that axis: th_a = 0, w_a = 0, landings + 1; peak_angle; and the sole's anchor in the contact
 *   rule's row follows the twist it was integrated with:  p += R2[:, 2] v_z dt,  R2 <- R2 Exp((w_x, w_y, 0) dt).  (A landing does not snap the anchor.)
 *   Then: sole free after the contact rule: rates, angles and v_z all 0.  Otherwise per axis, lim = h n:
 *   h = +inf: w_a = 0.  Else flat at rest (th_a == 0 and w_a == 0): excess = |tau_a| - lim, peak_excess; excess > 0: w_a = -(dt / I_tip) excess sign(tau_a).
 *   otherwise s = sign(th_a) if th_a != 0 else sign(w_a):  w_a <- w_a - (dt / I_tip) (tau_a + s lim)  (an edge transmits exactly -s lim).
 *   Then |w_a| is clamped to w_max, and |th_a| >= th_max with w_a th_a > 0: w_a = 0.
 *   v_z = s_x W w_x + s_y L w_y  (the origin's velocity when the sole turns about the carrying edge; an axis whose rate is 0 adds nothing).
 *   tipping = (a rate or an angle != 0). */
#define MPC_SIM_TIPPING_WIDTH 21

/* params[B][MPC_SIM_TIPPING_PARAMS]: the model on and reset (every state row 0); NULL: off (frees the rows).  Refused: the contact rule off
 * (mpc_sim_contacts first), a NaN or negative extent, I_tip, w_max or th_max not finite and > 0, reserved not 0.  A refused call leaves the
 * configuration in force.  mpc_sim_contacts(sim, NULL) drops the model, as it drops friction and the terrain. */
int mpc_sim_tipping(mpc_solver* sim, const double* params);

/* Impose state[B][MPC_SIM_TIPPING_WIDTH] (restore rows read earlier, or impose tip velocities).  Refused: a non-finite entry, a tipping flag other
 * than 0 or 1, a negative count, peak or step number, a rate or an angle on a sole whose flag is 0, |th| > th_max.  Synchronises the handle. */
int mpc_sim_tipping_set(mpc_solver* sim, const double* state);

/* Copy the rows in force to params[B][MPC_SIM_TIPPING_PARAMS] and the state rows to state[B][MPC_SIM_TIPPING_WIDTH] (either may be NULL;
 * synchronises the handle's stream). */
int mpc_sim_tipping_read(mpc_solver* sim, double* params, double* state);

int32_t mpc_sim_tipping_width(mpc_solver* sim);

#ifdef __cplusplus
}
#endif
#endif
