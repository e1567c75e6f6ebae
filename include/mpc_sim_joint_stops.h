/*
 * mpc_sim_joint_stops.h — HIP-library-only addition to the C-ABI of include/mpc_abi.h: per-robot joint end-stops in the torque-driven simulator.
 * With the model on, every simulator step of the handle (mpc_simulate_torque, and the simulator step inside mpc_qp_low_level_steps,
 * mpc_qp_ikid_low_level_steps and mpc_feedback_low_level_steps) adds to the torque of every actuated joint that stands beyond its range the torque
 * of a one-sided spring and damper that pushes it back, on the device, before the dynamics integrate the sum.  With it off nothing is launched,
 * nothing is allocated and every step is what it was: every joint turns freely.
 *
 * The rule is defined by its numpy mirror, mpc_benchmark_amd/joint_stops.py: the definition the checks hold the kernel (csrc/sim_joint_stops.h) to.
 * mpc_abi.h lists what BOTH libraries export (tests/test_abi_library.py); the entry points here are exported by libmpc_hip.so alone.  Bindings
 * look the symbols up before they use them (mpc_benchmark_amd/_capi.py).
 *
 * Every call takes the simulator handle of mpc_simulate_torque (whole-body, nu = nv - 6).  The calls return 0, or -1 with the reason in
 * mpc_last_error (mpc_sim_joint_stops_width: the width, or -1).
 *
 * Consequences of the model being on:
 *   - a stop is not a motor: the dynamics integrate the applied torque PLUS the stop torque, read from a buffer of the model's own, while the torque
 *     buffer of the step is left as it is.  The `tau` output of the device loops, the torque columns of the record (mpc_sim_record) and the joint
 *     power and energy of the metrics (mpc_sim_metrics) stay the actuators' torque (the applied torque of mpc_sim_actuators when that is on, the
 *     command otherwise);
 *   - the model runs after the actuator model and before the dynamics; everything else keeps its place in the order of a step;
 *   - the rule reads the TRUE state the step starts from, never the measurement of the sensor model or the estimate of the estimator;
 *   - the feedback-law simulators mpc_simulate and mpc_simulate_push do not see the model.
 */
#ifndef MPC_SIM_JOINT_STOPS_H
#define MPC_SIM_JOINT_STOPS_H

#include "mpc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One parameter row of MPC_SIM_JOINT_STOPS_PARAMS doubles per robot:
 *   0  k         stiffness in scale[j] per rad: finite, >= 0
 *   1  d         damping in scale[j] s per rad: finite, >= 0
 *   2  cap       bound on |tau_stop_j| as a multiple of scale[j]: > 0 (+inf: none)
 *   3 .. 7       reserved, 0
 * and two tables lo[B][nu], hi[B][nu] in rad, one pair of limits per robot and actuated joint (-inf / +inf: no stop on that side; lo == hi: a seized
 * joint; refused: lo > hi, NaN, lo == +inf, hi == -inf), and one vector scale[nu] in N m all robots share (NULL: ones; finite and > 0).  A row
 * whose limits are all infinite leaves the robot's torques untouched bit for bit. */
#define MPC_SIM_JOINT_STOPS_PARAMS 8
/* One state row of 5 nu + 2 doubles per robot: tau_stop[nu] the stop torque the latest step integrated, pen[nu] the signed penetration of the state
 * that step started from (q - hi > 0 above the range, q - lo < 0 below it, 0 inside or exactly on a limit), peak_pen[nu] the largest |pen| so far,
 * stop_steps[nu] the steps in which the joint's stop acted (tau_stop != 0), hits[nu] the steps whose pen != 0 followed a step with pen == 0,
 * any_steps the steps in which any stop of the robot acted, steps.  All 0 after a reset.
 *
 * A step is one call of mpc_simulate_torque (length substeps * dt; the stop torque is held over the substeps) or one step of a device loop (length
 * dt).  From q_j = x[7 + j] and v_j = x[nq + 6 + j] of the true state the step starts from, per actuated joint j:
 *   inside the range (lo <= q <= hi; always, with infinite limits):  tau_stop = 0
 *   above hi:  p = q - hi,  t = max(0, k p + d v),  tau_stop = -scale[j] min(t, cap)
 *   below lo:  p = lo - q,  t = max(0, k p - d v),  tau_stop = +scale[j] min(t, cap)
 * (t == 0: tau_stop = +0).  A stop only pushes back into the range and never pulls: the damper is cut off where it would hold a joint that is
 * already leaving.  With lo == hi the two branches together are a two-sided spring.  The dynamics integrate applied_j + tau_stop_j where
 * tau_stop_j != 0 and the applied torque itself, copied, elsewhere.
 * The rule is explicit (the state at the start of the step): the stop torque is held over a step's substeps, and scale[j] k dt_step^2 (and
 * scale[j] d dt_step) must stay small against the joint's reflected inertia, which is the caller's business, as for the viscous term of
 * mpc_sim_actuators. */

/* params[B][8], lo[B][nu], hi[B][nu], scale[nu] or NULL (ones).  params == NULL: off (frees everything, no kernel launched).  A call with
 * params != NULL turns the model on and resets the state rows; lo and hi must not be NULL then.  Validation as in the table.  A refused call leaves
 * the previous configuration in force. */
int mpc_sim_joint_stops(mpc_solver* sim, const double* params, const double* lo, const double* hi, const double* scale);

/* Copy the parameter rows to params[B][8], the limits to lo[B][nu] and hi[B][nu] and the state rows to state[B][5 nu + 2]; each may be NULL;
 * synchronises the handle's stream.  Fails while the model is off. */
int mpc_sim_joint_stops_read(mpc_solver* sim, double* params, double* lo, double* hi, double* state);

/* Impose state[B][5 nu + 2] (restore rows read earlier).  Rejected, with the rows in force kept: a non-finite entry, a negative peak_pen or count,
 * a |pen| above peak_pen.  Synchronises the handle. */
int mpc_sim_joint_stops_set(mpc_solver* sim, const double* state);

/* 5 nu + 2, or -1 */
int32_t mpc_sim_joint_stops_width(mpc_solver* sim);

#ifdef __cplusplus
}
#endif
#endif
