/*
 * mpc_sim_contacts.h — HIP-library-only addition to the C-ABI of include/mpc_abi.h: unilateral foot contacts of every robot of a torque-driven
 * simulator handle, decided on the device after every simulator step (mpc_simulate_torque, and the simulator step inside mpc_qp_low_level_steps,
 * mpc_qp_ikid_low_level_steps and mpc_feedback_low_level_steps) from the robot's own state.  With the rule on, each robot has its own feet on the
 * ground, each with its own ground-side placement; with it off the simulator integrates the contacts of its stage 0, as before.
 *
 * The rule is the headless BulletRobot's (mpc_benchmark_amd/bullet_robot.py, _update_contacts), applied per robot in the same order; its numpy
 * mirror, the definition the checks hold the kernel to, is mpc_benchmark_amd/contact_rule.py.  mpc_abi.h lists what BOTH libraries export
 * (tests/test_abi_library.py); the entry points here are exported by libmpc_hip.so alone.  Bindings look the symbols up before they use them
 * (mpc_benchmark_amd/_capi.py).
 *
 * Every call takes the simulator handle of mpc_simulate_torque: whole-body contact dynamics with nu = nv - 6, a model that holds the two sole
 * contacts (contacts 0 and 1: left, right).  While the rule is on, stage 0 of the handle must be the double-support stage (its contacts are 0 and 1):
 * every stepping call checks this and fails otherwise.  The stage's contact gains stay in use; the rule decides which of its two contacts each
 * robot integrates and where the ground side of each lies.  The calls return 0, or -1 with the reason in mpc_last_error (mpc_sim_contacts_width:
 * the width, or -1).
 */
#ifndef MPC_SIM_CONTACTS_H
#define MPC_SIM_CONTACTS_H

#include "mpc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpc_sim_contacts_config {
  double ground_z;        /* height of the ground plane (BulletRobot: the lower sole at initializeJoints)                                    */
  double ground_tol;      /* catch tolerance, >= 0: 5e-3 m (BulletRobot ground_tol)                                                         */
  double release_force;   /* >= 0: a contact "pulls" when its LOCAL-frame f_z < -release_force: 1 N                                         */
  int32_t release_steps;  /* consecutive pulling steps before the release, >= 1: 5                                                          */
  int32_t reserved;       /* 0                                                                                                              */
} mpc_sim_contacts_config;

/* One row of MPC_SIM_CONTACTS_WIDTH doubles per robot; pairs are (left, right) = contacts (0, 1).  A step is one call of mpc_simulate_torque
 * (whatever its substeps) or one step of a device loop; the rule runs once per step, on the state after it and the step's contact wrenches.
 *   0, 1    in_contact       1: the sole is held by its 6-D contact at its anchor; 0: free
 *   2, 3    lifted           1: the free sole has been above ground_z + 2 ground_tol since its release (cleared by a release)
 *   4, 5    pulling          consecutive steps in contact with LOCAL f_z < -release_force
 *   6, 7    z_prev           sole height after the latest step (after a reset: the anchor's height)
 *   8 - 19  anchor of sole 0: the ground side of its contact, R (row-major, 9) then p (3); after a reset the model's contact placement
 *  20 - 31  anchor of sole 1
 *  32, 33   touchdowns       catches since the reset
 *  34, 35   liftoffs         releases since the reset
 *  36, 37   last_touchdown   index (steps before it) of the step of the latest catch, -1 if none
 *  38, 39   last_liftoff     index of the step of the latest release, -1 if none
 *  40       steps            steps since the reset
 * The rule, foot 0 then foot 1 (foot 0's release counts for foot 1's test of the same step):
 *   in contact: pulling = pulling + 1 if f_z < -release_force else 0; at pulling >= release_steps, if the other sole is in contact: released
 *               (in_contact, lifted, pulling = 0).  The last contact is never released.
 *   free:       z > ground_z + 2 ground_tol: lifted = 1; else caught if (z <= ground_z + ground_tol and lifted) or (z < ground_z and z < z_prev):
 *               in_contact = 1, anchor = (Rz(yaw), (x, y, ground_z)) of the sole's placement (yaw = atan2(R[1][0], R[0][0])).
 *   z_prev = z for both soles.
 * With a terrain (include/mpc_sim_terrain.h) the free branch reads g_i, the terrain height under the origin of sole i, wherever it says ground_z. */
#define MPC_SIM_CONTACTS_WIDTH 41

/* cfg != NULL: the rule on and reset (allocates the device rows: both soles in contact at the model's anchors, counters at zero; a second call
 * resets them); NULL: off (frees them; the stage table decides the contacts again). */
int mpc_sim_contacts(mpc_solver* sim, const mpc_sim_contacts_config* cfg);

/* Impose rows[B][MPC_SIM_CONTACTS_WIDTH] (restore a state read earlier).  Rejected: a non-finite entry, a flag other than 0 or 1, a row with no
 * sole in contact, a negative count, an anchor whose R is not a rotation (|R^T R - I| > 1e-9 or det R < 0).  Synchronises the handle. */
int mpc_sim_contacts_set(mpc_solver* sim, const double* rows);

/* Copy the rows to rows[B][MPC_SIM_CONTACTS_WIDTH] (synchronises the handle's stream). */
int mpc_sim_contacts_read(mpc_solver* sim, double* rows);

int32_t mpc_sim_contacts_width(mpc_solver* sim);

#ifdef __cplusplus
}
#endif
#endif
