/*
 * mpc_sim_estimator.h — HIP-library-only addition to the C-ABI of include/mpc_abi.h: a per-robot base-state estimator between the sensor model of
 * the torque-driven simulator and the controllers.  With the estimator on, every simulator step of the handle (mpc_simulate_torque, and the
 * simulator step inside mpc_qp_low_level_steps, mpc_qp_ikid_low_level_steps and mpc_feedback_low_level_steps) is followed by one estimation event on
 * the device: the base position and the base linear velocity of the measured state are replaced by a blend of the measurement and of leg odometry
 * through the soles the plant holds, and the result is the state the controllers of the device loops read.  With it off nothing is launched,
 * nothing is allocated and every step is what it was.
 *
 * The rule is defined by its numpy mirror, mpc_benchmark_amd/state_estimator.py: the definition the checks hold the kernel (csrc/sim_estimator.h)
 * to.  mpc_abi.h lists what BOTH libraries export (tests/test_abi_library.py); the entry points here are exported by libmpc_hip.so alone.  Bindings
 * look the symbols up before they use them (mpc_benchmark_amd/_capi.py).
 *
 * Every call takes the simulator handle of mpc_simulate_torque (whole-body, nu = nv - 6).  The calls return 0, or -1 with the reason in
 * mpc_last_error (mpc_sim_estimator_width: the width, or -1).  The estimator needs the contact rule of the handle (mpc_sim_contacts): which soles
 * stand is the rule's `in_contact` pair.
 *
 * Consequences of the estimator being on:
 *   - an estimation event runs after every simulator step of the handle, last in the order of a step (after the dynamics, the record, the metrics,
 *     the contact rule and the sensor model): it reads the measurement of the sensor model when that model is on (mpc_sim_sensors), the true state
 *     otherwise, and the rows of the contact rule as the rule left them after this step;
 *   - what the controllers of the device loops read becomes the ESTIMATE: the state of the feedback kernels of the three loops, and with it the
 *     state their QPs are assembled at;
 *   - so does what the loops keep or return as `x_prev` / `c_prev`: the next solve's initial condition, the stale measurement of the centroidal
 *     loop's task errors and the state the device walk generators plan from;
 *   - the record (mpc_sim_record), the metrics (mpc_sim_metrics), the contact rule (mpc_sim_contacts) and the contact source of the low-level QPs
 *     (mpc_qp_contact_source) keep reading the TRUE state and the true contacts, `x_out` of every call stays the true state, and the measurement of
 *     the sensor model (mpc_sim_sensors_read) stays the measurement;
 *   - the estimator follows the states the simulator produces.  A caller that imposes a different state (the `x` argument of mpc_simulate_torque or
 *     of a device loop with another state than the handle holds, mpc_set_x0) arms again, after the sensor model: until the next event the estimate
 *     held is the old one;
 *   - turning the contact rule off (mpc_sim_contacts(sim, NULL)) drops the estimator, as it drops the terrain;
 *   - the feedback-law simulators mpc_simulate and mpc_simulate_push do not see the estimator.
 */
#ifndef MPC_SIM_ESTIMATOR_H
#define MPC_SIM_ESTIMATOR_H

#include "mpc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* State layout: x = [q (nq = nv + 1: base position 3, base quaternion xyzw 4, joints nu) ; v (nv: base linear 3 in the base frame, base angular 3,
 * joints nu)].  One parameter row of MPC_SIM_ESTIMATOR_PARAMS doubles per robot:
 *    0  w_p        weight of the leg odometry in the base position, in [0, 1]; per event
 *    1  w_v        weight of the leg odometry in the base linear velocity, in [0, 1]; per event
 *    2 - 15  reserved    0
 * The identity row (sixteen zeros) returns the measurement bit for bit. */
#define MPC_SIM_ESTIMATOR_PARAMS 16
/* One state row of nx + MPC_SIM_ESTIMATOR_TAIL doubles per robot: est[nx] the latest estimate, held[2] the in_contact pair of the event before,
 * anchor[2][3] the world points the origins of the two soles (contacts 0 and 1 of the model) are taken to stand on, stats[8], count (events since
 * arming, 1 after it).
 *
 * An event takes the measured state xm, the robot's in_contact pair c of the contact rule and the true state xt (statistics only):
 *   1. kinematics at xk = xm with the base position and the base linear velocity set to 0: r_i the world position of the origin of sole i, u_i the
 *      world velocity of that point;
 *   2. count + 1; kept: the soles with c_i = 1, held_i = 1 and count > 1; new: the soles with c_i = 1 that are not kept;
 *   3. p_odo = the mean over the kept soles of anchor_i - r_i (two: 0.5 (a + b)); none kept: p_odo = p_m;
 *   4. v_odo = - R_b^T mean(u_i) over all soles with c_i = 1, R_b the measured base rotation; none: v_odo = v_m;
 *   5. p_hat = p_m if w_p == 0, else p_m + w_p (p_odo - p_m);
 *   6. v_hat likewise with w_v;
 *   7. every kept anchor += p_hat - p_odo; nothing is added when w_p == 1;
 *   8. new soles: anchor_i = p_hat + r_i;
 *   9. held = c;
 *  10. est = xm with p_hat, v_hat in place of the base position and the base linear velocity;
 *  11. skipped on the arming event: stats[0..3] += / max the errors of est against xt — sum of |p error|^2, sum of |v_lin error|^2, largest
 *      |p error|, largest |v_lin error| (Euclidean norms) —, stats[4..7] the same four for xm. */
#define MPC_SIM_ESTIMATOR_TAIL 17

/* params[B][16], x0[B][nx].  params == NULL: off (frees everything, no kernel launched afterwards; x0 is not read).  A call with params != NULL
 * validates — finite entries, the weights in [0, 1], the reserved entries 0, x0 non-null and finite —, needs the contact rule on, turns the
 * estimator on, resets the state rows and runs the arming event on x0 (the first MEASURED states) with the in_contact pair of the rule's rows: no
 * sole is kept, every sole in contact is new (anchor_i = p_m + r_i), count is 1 afterwards and an estimate is always held.  A bad call leaves the
 * previous configuration in force. */
int mpc_sim_estimator(mpc_solver* sim, const double* params, const double* x0);

/* Copy the parameter rows to params[B][16], the state rows to state[B][nx + 17] and the estimate the controllers read to x_est[B][nx] (each may be
 * NULL); synchronises the handle's stream.  Fails while the estimator is off. */
int mpc_sim_estimator_read(mpc_solver* sim, double* params, double* state, double* x_est);

/* Impose state[B][nx + 17] (restore rows read earlier); the estimate the controllers read becomes the rows' est.  Rejected, with the rows in force
 * kept: a non-finite entry, a held flag that is not 0 or 1, a count < 1.  Synchronises the handle. */
int mpc_sim_estimator_set(mpc_solver* sim, const double* state);

/* nx + 17, or -1 */
int32_t mpc_sim_estimator_width(mpc_solver* sim);

#ifdef __cplusplus
}
#endif
#endif
