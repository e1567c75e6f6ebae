// walk_commands.h — include/mpc_walk_commands.h: a walk command per robot for the two device generators.  The table of a handle is a [B][16] device
// buffer that k_walk_refs (solver_kernels.h) / k_walk_poses (walk_poses.h) get as their last argument while it is in force, nullptr otherwise.
// Included at the end of mpc_hip.hip (mpc_solver, MPC_TRY, copy_sync).
#pragma once
#include "../../include/mpc_walk_commands.h"

// who: the entry point's name ; on: the generator was initialised ; d_cmd / cmd_on: the handle's table of that generator
static void walk_commands_set(mpc_solver* s, const char* who, bool on, double*& d_cmd, bool& cmd_on, const double* cmd) {
  const std::string w(who);
  if (!on) throw std::runtime_error(w + ": the generator is not on (mpc_walk_init / mpc_walk_poses_init first)");
  if (!cmd) { cmd_on = false; return; }
  const size_t n = (size_t)s->L.B * MPC_WALK_COMMAND_WIDTH;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(cmd[i])) throw std::runtime_error(w + ": non-finite value in the command of robot " + std::to_string(i / MPC_WALK_COMMAND_WIDTH));
  if (!d_cmd) d_cmd = s->alloc<double>(n);
  copy_sync(s, d_cmd, cmd, n * sizeof(double), hipMemcpyHostToDevice);  // (stream-ordered: behind the generator launches of the ticks in flight)
  cmd_on = true;
}

static void walk_commands_get(mpc_solver* s, const char* who, bool on, const double* d_cmd, bool cmd_on, double* out) {
  const std::string w(who);
  if (!on) throw std::runtime_error(w + ": the generator is not on (mpc_walk_init / mpc_walk_poses_init first)");
  if (!cmd_on) throw std::runtime_error(w + ": no command table is set (every robot walks the shared configuration)");
  if (!out) throw std::runtime_error(w + ": null output");
  copy_sync(s, out, d_cmd, (size_t)s->L.B * MPC_WALK_COMMAND_WIDTH * sizeof(double), hipMemcpyDeviceToHost);
}

extern "C" {

int mpc_walk_set_commands(mpc_solver* s, const double* cmd) {
  MPC_TRY(s, {
    walk_commands_set(s, "walk_set_commands", s->walk_on, s->d_walk_cmd, s->walk_cmd_on, cmd);
    s->walk_force_all = true;  // the apex of the swing curve may have changed: the next update rewrites every knot's references
  })
}

int mpc_walk_get_commands(mpc_solver* s, double* out) {
  MPC_TRY(s, { walk_commands_get(s, "walk_get_commands", s->walk_on, s->d_walk_cmd, s->walk_cmd_on, out); })
}

int mpc_walk_poses_set_commands(mpc_solver* s, const double* cmd) {
  MPC_TRY(s, { walk_commands_set(s, "walk_poses_set_commands", s->poses_on, s->d_poses_cmd, s->poses_cmd_on, cmd); })
}

int mpc_walk_poses_get_commands(mpc_solver* s, double* out) {
  MPC_TRY(s, { walk_commands_get(s, "walk_poses_get_commands", s->poses_on, s->d_poses_cmd, s->poses_cmd_on, out); })
}

}  // extern "C"
