/*
 * mpc_sim_actuators.h — HIP-library-only addition to the C-ABI of include/mpc_abi.h: a per-robot actuator model between the controllers and the
 * torque-driven simulator.  With the model on, every simulator step of the handle (mpc_simulate_torque, and the simulator step inside
 * mpc_qp_low_level_steps, mpc_qp_ikid_low_level_steps and mpc_feedback_low_level_steps) passes the torque the controller commanded through the
 * robot's own transport delay, gain error, first-order lag, saturation and joint friction, on the device, before the dynamics integrate it.  With
 * it off nothing is launched and every step is what it was.
 *
 * The rule is defined by its numpy mirror, mpc_benchmark_amd/actuator_model.py: the definition the checks hold the kernel (csrc/sim_actuators.h)
 * to.  mpc_abi.h lists what BOTH libraries export (tests/test_abi_library.py); the entry points here are exported by libmpc_hip.so alone.  Bindings
 * look the symbols up before they use them (mpc_benchmark_amd/_capi.py).
 *
 * Every call takes the simulator handle of mpc_simulate_torque (whole-body, nu = nv - 6).  The calls return 0, or -1 with the reason in
 * mpc_last_error (mpc_sim_actuators_width: the width, or -1).
 *
 * Consequences of the model being on:
 *   - the `tau` output of the device loops, the torque columns of the record (mpc_sim_record) and the power and energy of the metrics
 *     (mpc_sim_metrics) are all the APPLIED torque, not the command: the model rewrites the torque buffer of the step in place before the step;
 *   - a contact rule (mpc_sim_contacts) or a push (mpc_sim_set_push) keep their place in the order of a step: the model runs before the dynamics,
 *     the record, the metrics and the contact rule after them, as before;
 *   - the feedback-law simulators mpc_simulate and mpc_simulate_push do not see the model.
 */
#ifndef MPC_SIM_ACTUATORS_H
#define MPC_SIM_ACTUATORS_H

#include "mpc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One parameter row of MPC_SIM_ACTUATORS_PARAMS doubles per robot:
 *   0  delay          transport delay in steps: an integer value in [0, MPC_SIM_ACTUATORS_RING - 1]
 *   1  scale          torque gain error: finite, > 0
 *   2  time_constant  first-order lag in seconds, >= 0 (0: none)
 *   3  damping        viscous joint friction in N m s / rad, >= 0
 *   4  coulomb        Coulomb friction in N m, >= 0
 *   5  v_eps          smoothing velocity of the Coulomb term, > 0 when coulomb > 0
 *   6  sat            saturation as a fraction of limit[j], >= 0 (0: none)
 *   7  reserved       0
 * The identity row (0, 1, 0, 0, 0, *, 0) applies the command bit for bit. */
#define MPC_SIM_ACTUATORS_PARAMS 8
/* One state row of 18 nu + 2 doubles per robot: ring[MPC_SIM_ACTUATORS_RING][nu] the latest commanded torques, y[nu] the lag state, applied[nu] the
 * torque the latest step integrated, head (the ring slot of the newest command), count (commands since the reset).  All 0 after a reset.
 *
 * A step is one call of mpc_simulate_torque (length substeps * dt; the applied torque is held over the substeps) or one step of a device loop
 * (length dt).  From the commanded torque u and the joint velocities v of the state the step starts from, per joint j:
 *   the command is pushed into the ring (head advances, count + 1); ud = the command pushed `delay` steps ago, the oldest one held while fewer than
 *   delay + 1 are (the line is primed with the first command); w = scale ud;
 *   lag: time_constant == 0 or count == 1: y = w; else y += -expm1(-dt_step / time_constant) (w - y);
 *   saturation, sat > 0: y_out = clamp(y, +- sat limit[j]) (the lag state keeps the unclamped y);
 *   friction, damping > 0 or coulomb > 0: tau = y_out - friction_shape[j] (damping v_j + coulomb tanh(v_j / v_eps));
 *   applied = tau: what the dynamics integrate.
 * The viscous term is explicit (the velocity at the start of the step): damping * dt_step must stay small against the joint's reflected inertia,
 * which is the caller's business. */
#define MPC_SIM_ACTUATORS_RING 16

/* params[B][8], limit[nu] or NULL, friction_shape[nu] or NULL (ones).  params == NULL: off (frees the rows, no kernel launched).  A call with
 * params != NULL turns the model on and resets the state rows.  Validation as in the table; limit is needed when any row has sat > 0; limit and
 * friction_shape are finite and >= 0.  A bad row fails the call and leaves the previous configuration in force. */
int mpc_sim_actuators(mpc_solver* sim, const double* params, const double* limit, const double* friction_shape);

/* Copy the parameter rows to params[B][8] (or NULL) and the state rows to state[B][18 nu + 2] (or NULL); synchronises the handle's stream.  Fails
 * while the model is off. */
int mpc_sim_actuators_read(mpc_solver* sim, double* params, double* state);

/* Impose state[B][18 nu + 2] (restore rows read earlier).  Rejected, with the rows in force kept: a non-finite entry, a head that is not an integer
 * value in [0, 16), a count < 0.  Synchronises the handle. */
int mpc_sim_actuators_set(mpc_solver* sim, const double* state);

/* 18 nu + 2, or -1 */
int32_t mpc_sim_actuators_width(mpc_solver* sim);

#ifdef __cplusplus
}
#endif
#endif
