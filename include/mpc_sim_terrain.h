/*
 * mpc_sim_terrain.h — HIP-library-only addition to the C-ABI of include/mpc_abi.h: a per-robot box terrain under the unilateral foot-contact rule of
 * a torque-driven simulator handle (include/mpc_sim_contacts.h).  The rule knows one ground, the plane z = ground_z; with a terrain the ground under
 * a sole is the height function
 *
 *     h(x, y) = max( ground_z, max{ z_top of the boxes with x_lo <= x <= x_hi and y_lo <= y <= y_hi } )
 *
 * of up to MPC_SIM_TERRAIN_MAX_BOXES axis-aligned boxes (x_lo, x_hi, y_lo, y_hi, z_top), one set for all robots or one set per robot (64 robots on 64
 * staircases in one launch).  Boxes may overlap (the higher wins); a box whose top is below ground_z has no effect; the intervals are closed.
 * Only comparisons and max: the device and the numpy definition (mpc_benchmark_amd/contact_rule.py, terrain_height) agree bit for bit.
 *
 * The ground under sole i is g_i = h at the ORIGIN of the sole frame, and the rule is that of mpc_sim_contacts.h with g_i in place of ground_z in its
 * free-foot branch, nothing else: lifted when z > g_i + 2 ground_tol; caught when (z <= g_i + ground_tol and lifted) or (z < g_i and z < z_prev); the
 * anchor of a catch is (Rz(yaw), (x, y, g_i)).  The in-contact branch, the order of the feet, z_prev, the counters and the row layout do not change,
 * and without a terrain g_i is ground_z itself: rows and states keep their bits.  With a terrain the fall verdict of the metrics
 * (include/mpc_sim_metrics.h) is taken above the ground: sole i by z_i - g_i, the base by z_base minus the mean anchor height of the soles in
 * contact (the row the step was integrated with), and base_z0 / sole_z0 are latched in the same terms.
 * Not modelled: risers (nothing stops a foot horizontally), a sole that hangs over an edge or has its toe inside the next step, slopes.
 *
 * mpc_abi.h lists what BOTH libraries export (tests/test_abi_library.py); the entry points here are exported by libmpc_hip.so alone.  Bindings look
 * the symbols up before they use them (mpc_benchmark_amd/_capi.py).  Every call takes the simulator handle of mpc_simulate_torque with the contact
 * rule on (mpc_sim_contacts(cfg) first) and fails otherwise.  mpc_sim_contacts(NULL) drops the terrain with the rows; a repeated mpc_sim_contacts(cfg)
 * (a reset) keeps it and uses the new ground_z.  Setting a terrain does not touch the rows: robots that are to start on a box get their anchors through
 * mpc_sim_contacts_set.  The terrain applies at every stepping site of the rule (mpc_simulate_torque, mpc_qp_low_level_steps,
 * mpc_qp_ikid_low_level_steps, mpc_feedback_low_level_steps).  The calls return 0, or -1 with the reason in mpc_last_error.
 */
#ifndef MPC_SIM_TERRAIN_H
#define MPC_SIM_TERRAIN_H

#include "mpc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPC_SIM_TERRAIN_MAX_BOXES 16
#define MPC_SIM_TERRAIN_BOX_WIDTH 5

typedef struct mpc_sim_terrain_config {
  int32_t n_boxes;            /* 0 .. MPC_SIM_TERRAIN_MAX_BOXES */
  int32_t per_robot;          /* 0: boxes[n_boxes][5] for every robot; 1: boxes[B][n_boxes][5] */
} mpc_sim_terrain_config;

/* cfg != NULL: the terrain of boxes (copied; synchronises the handle); cfg NULL: terrain off (the plane again).  Rejected: n_boxes out of range,
 * per_robot other than 0 / 1, boxes == NULL with n_boxes > 0, a non-finite number, x_lo > x_hi or y_lo > y_hi, the rule off, a handle that is not a
 * torque-driven simulator. */
int mpc_sim_terrain(mpc_solver* sim, const mpc_sim_terrain_config* cfg, const double* boxes);

/* The terrain in force: cfg (n_boxes = 0, per_robot = 0 when none is set) and, unless boxes is NULL, the boxes in the form they were given. */
int mpc_sim_terrain_read(mpc_solver* sim, mpc_sim_terrain_config* cfg, double* boxes);

/* h of robot b's terrain at xy[B][n][2] -> h[B][n], evaluated by the device's height function (ground_z where no terrain is set). */
int mpc_sim_terrain_height(mpc_solver* sim, const double* xy, int32_t n, double* h);

#ifdef __cplusplus
}
#endif
#endif
