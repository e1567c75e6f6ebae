/*
 * mpc_walk_commands.h — HIP-library-only addition to the C-ABI of include/mpc_abi.h and include/mpc_walk_poses.h: a walk command per robot.  The two
 * device generators (mpc_walk_update: k_walk_refs ; mpc_walk_poses_update: k_walk_poses) plan every robot of an ensemble with the step offsets, the
 * foot yaw per step and the swing apex of ONE configuration; with a command table robot b plans with row b.
 *
 * mpc_abi.h lists what BOTH libraries export (tests/test_abi_library.py); the entry points here are exported by libmpc_hip.so alone.  Their checker
 * side is the numpy generator with the same table (mpc_benchmark_amd/references.py: walk_commands, stopped_commands, FootTrajectoryBatch.set_commands;
 * EnsembleMPC.enable_walk(per_instance=True, commands=...)), which runs on either library.  Bindings look the symbols up before they use them
 * (mpc_benchmark_amd/_capi.py).
 */
#ifndef MPC_WALK_COMMANDS_H
#define MPC_WALK_COMMANDS_H

#include "mpc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One row per robot: t_left[3] | t_right[3] | rot_diff[9] row-major | swing_apex — the foothold offsets in the stance foot's yaw frame, the rotation
 * applied to the right foothold and the apex of the swing curve: the fields of the same names of mpc_walk_config / mpc_walk_poses_config. */
#define MPC_WALK_COMMAND_WIDTH 16

/* The table of a handle is sticky and lives on the device: set once, it stays in force for every later update until another one or NULL replaces it
 * (or the generator is initialised again, which starts from the shared configuration).  The generator must have been turned on first (mpc_walk_init
 * for the first pair, mpc_walk_poses_init for the second: a handle keeps one table per generator), and every value must be finite.
 *
 * While a table is set
 *   - robot b's plan is made with row b of it: t_left, t_right, rot_diff and swing_apex of the configuration are ignored;
 *   - forward != NULL in mpc_walk_update / mpc_walk_poses_update is an error (forward[7] rewrites the configuration's offsets, which nobody reads: the
 *     call fails and mpc_last_error names the table) — the caller sets a table with the stopped rows instead;
 *   - floor_z, z_follow and every offset of the configuration stay what they are, shared by the robots.
 *
 * When a new table (or NULL) takes effect: the footholds are planned with it at the next replanning tick — a foot without a pending landing, a
 * take-off inside the double-support window: when the foothold rules run — and a plan already made keeps its footholds until then.  The swing curve
 * follows the new apex from the next update on: mpc_walk_set_commands makes the next mpc_walk_update rewrite the references of every knot (as
 * mpc_walk_set_state does), and mpc_walk_poses_update rewrites every knot on every tick anyway.
 *
 * The table is not part of mpc_get_state / mpc_set_state, nor of the plans of mpc_walk_get_state / mpc_walk_poses_get_state (as the per-instance
 * parameter tables are not): a caller that restores a checkpoint restores its table. */
int mpc_walk_set_commands(mpc_solver* s, const double* cmd);        /* cmd[B][16] ; NULL: back to the shared configuration */
int mpc_walk_get_commands(mpc_solver* s, double* out);              /* out[B][16] ; an error when no table is set */
int mpc_walk_poses_set_commands(mpc_solver* plan, const double* cmd);
int mpc_walk_poses_get_commands(mpc_solver* plan, double* out);

#ifdef __cplusplus
}
#endif
#endif
