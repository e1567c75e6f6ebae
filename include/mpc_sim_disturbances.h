/*
 * mpc_sim_disturbances.h — HIP-library-only addition to the C-ABI of include/mpc_abi.h: a per-robot schedule of pushes on any link of a
 * torque-driven simulator handle, timed on the device at the simulator's own rate.  mpc_sim_set_push (include/mpc_sim_ext.h) holds one vector per
 * robot until the host arms another, so inside a device loop (one MPC period per call) it switches at period boundaries only, and it acts on the base.
 * With this model on, every robot carries a table of up to MPC_SIM_DISTURBANCES_MAX_EVENTS events; before each simulator step one workgroup per
 * robot (csrc/sim_disturbances.h, k_sim_disturbances) advances the robot's clock, sees the touchdowns and lift-offs of its soles in the rows of the
 * contact rule (include/mpc_sim_contacts.h), picks the event that acts and writes its world force, world point and link; the dynamics of the step
 * apply it on that link's chain.  Off by default; off launches and allocates nothing, and an armed table none of whose events is active keeps
 * every bit of the step.
 *
 * The numpy mirror, the definition the checks hold the kernel to, is mpc_benchmark_amd/disturbance_model.py.  mpc_abi.h lists what BOTH libraries
 * export; the entry points here are exported by libmpc_hip.so alone.  Bindings look the symbols up before they use them
 * (mpc_benchmark_amd/_capi.py).  Every call takes the simulator handle of mpc_simulate_torque, and returns 0, or -1 with the reason in
 * mpc_last_error (mpc_sim_disturbances_width: the width, or -1).
 */
#ifndef MPC_SIM_DISTURBANCES_H
#define MPC_SIM_DISTURBANCES_H

#include "mpc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One event is 16 doubles.  Integers are held as doubles and must be integral; everything must be finite.
 *
 * | idx   | field         | meaning                                                                                                             |
 * |-------|---------------|---------------------------------------------------------------------------------------------------------------------|
 * | 0     | `trigger`     | 0 empty slot; 1 absolute step; 2 left touchdown; 3 left lift-off; 4 right touchdown; 5 right lift-off (sole 0 =   |
 * |       |               | left, 1 = right).                                                                                                   |
 * | 1     | `start`       | Trigger 1: step of the handle's disturbance clock at which the event begins (>= 0).  The clock is 0 at arming or    |
 * |       |               | reset and advances by one per simulator step, whatever the step's substeps.  Triggers 2 to 5: which occurrence of   |
 * |       |               | that transition since arming or reset (>= 1).                                                                       |
 * | 2     | `delay`       | Steps between the trigger and the first pushed step (>= 0).                                                         |
 * | 3     | `steps`       | Duration in simulator steps (>= 1).                                                                                 |
 * | 4     | `period`      | 0 means once.  Trigger 1: repeat every `period` steps (>= `steps`).  Triggers 2 to 5: fire again at every           |
 * |       |               | `period`-th further occurrence.                                                                                     |
 * | 5     | `shape`       | 0 rectangular.  1 half sine: step k of n carries sin(pi (k + 1/2) / n) times the force.                             |
 * | 6     | `link`        | The moving joint of the model the force acts on, numbered as the plant rows of include/mpc_sim_plant.h number their |
 * |       |               | link (table joint indices, 0 .. nj - 1).  The floating base is the first.                                           |
 * | 7     | `force_frame` | 0 world axes.  1 the link's own axes.                                                                               |
 * | 8     | `point_frame` | 0 a fixed world point.  1 a point of the link, in the link's frame, carried with it.                                |
 * | 9-11  | `force`       | N.                                                                                                                  |
 * | 12-14 | `point`       | m.                                                                                                                  |
 * | 15    | reserved      | Must be 0.                                                                                                          |
 */
#define MPC_SIM_DISTURBANCES_EVENT 16
#define MPC_SIM_DISTURBANCES_MAX_EVENTS 8

/* One state row per robot.
 *   0        step            the disturbance clock: simulator steps since arming or reset
 *   1        acting          index of the event that acted in the last step, -1: none (also before the first step)
 *   2 - 5    occurrences     left touchdowns, left lift-offs, right touchdowns, right lift-offs seen since arming or reset (triggers 2, 3, 4, 5)
 *   6 - 13   fire_step       per event slot: the clock step at which a contact-triggered event begins (its latest firing), -1: none
 *  14 - 16   impulse         sum of the world force that acted times the step's length (substeps * dt), N s
 *  17        pushed_steps    steps in which an event acted
 *  18        shadowed_steps  active events that did not act because one of lower index did, summed over the steps
 *  19        peak_force      largest |world force| that acted, N
 *  20 - 25   applied         what the dynamics of the last step got: world force (3), world point (3); 0 when nothing acted
 *  26        link            ... and the link it acted on, -1 when nothing acted
 *  27, 28    seen            the in_contact pair of the contact rule the step before read; -1: none yet (the sentinel: the first pair is
 *                            taken without counting a transition)
 *  29 - 31   reserved        0
 * The rule, once per simulator step BEFORE the step's dynamics, t = step, on the state x the step starts from and the in_contact pair the contact
 * rule's rows hold then (what the step before left):
 *   transitions: with seen = -1 the pair is taken; else sole i with in_contact 0 -> 1 is a touchdown, 1 -> 0 a lift-off: its occurrence counter
 *     advances to n, and every event e of that trigger with n >= start and (n == start, or period > 0 and (n - start) % period == 0) gets
 *     fire_step[e] = t + delay.  Without the contact rule nothing is compared.
 *   event e is active with step index k of n = steps:  trigger 1: u = t - start - delay >= 0, k = u (period 0) or u % period, k < n;
 *     triggers 2 to 5: fire_step[e] >= 0, k = t - fire_step[e], 0 <= k < n.
 *   the active event of lowest index acts, every other active one adds 1 to shadowed_steps.  Its weight w is 1, or sin(pi (k + 1/2) / n).
 *   frames 1 are evaluated by the forward kinematics of x (link placement R, p) and held for the step, all substeps included:
 *     f = w force (force_frame 0) or w R force ; point = point (point_frame 0) or R point + p.
 *   applied = (f, point, link); impulse += f (substeps dt); pushed_steps += 1; peak_force = max(peak_force, |f|).  Nothing active: applied = 0,
 *     link = -1, acting = -1, and the step's dynamics skip the term.
 *   step = t + 1. */
#define MPC_SIM_DISTURBANCES_WIDTH 32

/* events[B][n_events][MPC_SIM_DISTURBANCES_EVENT], 1 <= n_events <= MPC_SIM_DISTURBANCES_MAX_EVENTS: the model on, the state rows reset.  NULL:
 * off (frees everything; n_events is ignored).  Every check runs before anything changes, and an error names the robot, the event and the field.
 * Refused: a non-finite entry, a non-integral integer field, a trigger outside 0 .. 5, start < 0 (trigger 1) or < 1 (triggers 2 to 5), delay < 0,
 * steps < 1, period < 0 or (trigger 1) 0 < period < steps, a shape or frame other than 0 or 1, a link outside the model's moving joints, a
 * non-zero reserved entry; a contact trigger (2 to 5) with the contact rule off (mpc_sim_contacts first); a push armed on the handle
 * (mpc_sim_set_push(sim, NULL, 0) first).  While the model is on, mpc_sim_set_push with a non-NULL push is refused.  mpc_sim_contacts(sim, NULL)
 * drops an armed table that uses a contact trigger, as it drops the terrain.  The links are checked against the model on the handle; while the
 * model is on, mpc_set_model with another joint count is refused (a model of the same joint count, e.g. with a frame more, keeps every link valid).  The record's push slot (include/mpc_sim_ext.h) shows what acted. */
int mpc_sim_disturbances(mpc_solver* sim, const double* events, int32_t n_events);

/* Copy the table in force to events[B][n_events][MPC_SIM_DISTURBANCES_EVENT], the state rows to state[B][MPC_SIM_DISTURBANCES_WIDTH] and what the
 * dynamics of the last step got to applied[B][7] = (world force, world point, link; -1: nothing acted), read from the buffers the dynamics read.
 * Any pointer may be NULL; synchronises the handle's stream.  (n_events of the table in force: mpc_sim_disturbances_events.) */
int mpc_sim_disturbances_read(mpc_solver* sim, double* events, double* state, double* applied);

/* Clock, counters and accumulators back to the state after arming; the table is kept. */
int mpc_sim_disturbances_reset(mpc_solver* sim);

/* MPC_SIM_DISTURBANCES_WIDTH on a simulator handle, -1 otherwise. */
int32_t mpc_sim_disturbances_width(mpc_solver* sim);

/* n_events of the table in force, 0 while the model is off, -1 on a handle that is no simulator handle. */
int32_t mpc_sim_disturbances_events(mpc_solver* sim);

#ifdef __cplusplus
}
#endif
#endif
