// walk_poses.h — include/mpc_walk_poses.h: the walk generator of the centroidal problem for every robot of an ensemble with per-instance parameter
// tables, planned from the soles of the robot's own measured whole-body state (centroidal_talos.py:369-384).  Included at the end of mpc_hip.hip
// (mpc_solver, MPC_TRY, slot_of, copy_sync); the generator's rules are the functions of walk_generator.h that k_walk_refs uses.
#pragma once
#include "../../include/mpc_walk_poses.h"

// grid B, block 128.  On a replanning tick two threads run the forward kinematics of the two sole frames at the robot's measured state x[b] (model
// tables mi / md of another handle) and one applies the foothold rules to the robot's plan; then a thread per knot forms the references of both
// feet and stores the translation at the three places of every foot whose contact state in the knot's own table is on — ring-indexed as the
// stage tables are, BEFORE the rotation of this tick.  The threads of knots 0 and 1 also keep the two reference samples of both feet.
// cmd: nullptr or the [B][16] command table of include/mpc_walk_commands.h, staged as in k_walk_refs.
__global__ void __launch_bounds__(128) k_walk_poses(SolverArgs a, const int32_t* mi, const double* md, const double* x, int nx, mpc_walk_poses_config c,
                                                    double* state, double* samples, int takeoff_RF, int takeoff_LF, int land_RF, int land_LF, int replanning,
                                                    const double* cmd) {
  const Layout& L = a.L;
  const int b = blockIdx.x, tid = threadIdx.x, N = L.N;
  __shared__ double st[48], meas[24], cw[MPC_WALK_COMMAND_WIDTH];
  double* gst = state + (size_t)b * 48;
  if (replanning) {
    if (tid < 2) {
      M3 R; V3 p;
      walk_frame_placement(mi, md, x + (size_t)b * nx, tid == 0 ? c.frame_lf : c.frame_rf, R, p);
      walk_pose_store(meas + 12 * tid, R, p);
    }
    if (tid >= 64 && tid < 112) st[tid - 64] = gst[tid - 64];
    else if (cmd && tid >= 112) cw[tid - 112] = cmd[(size_t)b * MPC_WALK_COMMAND_WIDTH + (tid - 112)];
    __syncthreads();
    if (tid == 0) {
      if (cmd) walk_plan(st, meas, meas + 12, takeoff_RF, takeoff_LF, land_RF, land_LF, c.T_ds, cw, cw + 3, cw + 6, c.floor_z);
      else walk_plan(st, meas, meas + 12, takeoff_RF, takeoff_LF, land_RF, land_LF, c.T_ds, c.t_left, c.t_right, c.rot_diff, c.floor_z);
    }
    __syncthreads();
    if (tid < 48) gst[tid] = st[tid];
  } else {
    if (tid < 48) st[tid] = gst[tid];
    else if (cmd && tid < 48 + MPC_WALK_COMMAND_WIDTH) cw[tid - 48] = cmd[(size_t)b * MPC_WALK_COMMAND_WIDTH + (tid - 48)];
    __syncthreads();
  }
  const double apex = cmd ? cw[15] : c.swing_apex;
  double* tables = const_cast<double*>(a.inst_params) + (size_t)b * (N + 1) * L.max_stage_doubles;
  for (int j = tid; j < N; j += blockDim.x) {
    double ref[2][12];
    walk_ref(ref[0], st, st + 12, land_LF, j, c.T_ss, apex);
    walk_ref(ref[1], st + 24, st + 36, land_RF, j, c.T_ss, apex);
    double* tab = tables + (size_t)stage_slot(a, j) * L.max_stage_doubles;
    for (int i = 0; i < 2; ++i) {
      if (tab[c.state_offs[2 * i]] == 0.0) continue;  // a foot that does not stand in this knot's stage keeps its pose (centroidal_talos.py:376, 381)
      for (int k = 0; k < 3; ++k)
        for (int e = 0; e < 3; ++e) tab[c.pose_offs[3 * i + k] + e] = ref[i][9 + e];
    }
    if (j < 2)
      for (int i = 0; i < 2; ++i)
        for (int e = 0; e < 12; ++e) samples[(size_t)b * 48 + 24 * i + 12 * j + e] = ref[i][e];
  }
}

static void walk_poses_check_model(const mpc_solver* s, const mpc_solver* model, const mpc_walk_poses_config& c, const char* who) {
  const std::string w(who);
  if (!model || !model->d_model_i || model->L.space != MPC_SPACE_MULTIBODY) throw std::runtime_error(w + ": the model handle needs a whole-body model (mpc_set_model)");
  if (model->dims.device != s->dims.device) throw std::runtime_error(w + ": the plan and the model handle must live on one device");
  const int nf = model->h_model_i.size() > 3 ? model->h_model_i[3] : 0;
  if (c.frame_lf < 0 || c.frame_lf >= nf || c.frame_rf < 0 || c.frame_rf >= nf) throw std::runtime_error(w + ": frame index out of range");
}

extern "C" {

int mpc_walk_poses_init(mpc_solver* s, mpc_solver* model, const mpc_walk_poses_config* cfg) {
  MPC_TRY(s, {
    const Layout& L = s->L;
    if (!cfg) throw std::runtime_error("walk_poses_init: null configuration");
    if (!s->d_inst_params) throw std::runtime_error("walk_poses_init: mpc_enable_instance_params first");
    if (L.N < 2) throw std::runtime_error("walk_poses_init: a horizon of at least two knots is needed (two reference samples)");
    walk_poses_check_model(s, model, *cfg, "walk_poses_init");
    for (int off : cfg->pose_offs) if (off < 0 || off + 3 > L.max_stage_doubles) throw std::runtime_error("walk_poses_init: pose offset out of range");
    for (int off : cfg->state_offs) if (off < 0 || off >= L.max_stage_doubles) throw std::runtime_error("walk_poses_init: state offset out of range");
    if (cfg->T_ss <= 0 || cfg->T_ds < 0) throw std::runtime_error("walk_poses_init: T_ss must be positive and T_ds non-negative");
    s->poses = *cfg;
    if (!s->d_poses_state) { s->d_poses_state = s->alloc<double>((size_t)L.B * 48); s->d_poses_samples = s->alloc<double>((size_t)L.B * 48); }
    std::vector<double> st((size_t)L.B * 48);
    for (int b = 0; b < L.B; ++b) {
      double* p = st.data() + (size_t)b * 48;
      std::memcpy(p, cfg->lf0, 96); std::memcpy(p + 12, cfg->lf0, 96); std::memcpy(p + 24, cfg->rf0, 96); std::memcpy(p + 36, cfg->rf0, 96);
    }
    copy_sync(s, s->d_poses_state, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice);
    copy_sync(s, s->d_poses_samples, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice);  // (the same layout: both samples at the initial footholds)
    s->poses_on = true;
    s->poses_cmd_on = false;  // (include/mpc_walk_commands.h: a new configuration starts without a table)
  })
}

int mpc_walk_poses_update(mpc_solver* s, mpc_solver* model, const double* x, mpc_qp_solver* qp, int32_t takeoff_RF, int32_t takeoff_LF, int32_t land_RF,
                          int32_t land_LF, const double* forward) {
  MPC_TRY(s, {
    const Layout& L = s->L;
    if (!s->poses_on) throw std::runtime_error("walk_poses_update: mpc_walk_poses_init first");
    mpc_walk_poses_config& c = s->poses;
    walk_poses_check_model(s, model, c, "walk_poses_update");
    if (s->async_pending > 0) throw std::runtime_error("walk_poses_update: the plan has ticks in flight (mpc_wait first)");
    const size_t nx = (size_t)model->L.nx;
    const double* d_x = nullptr;
    if (x) {
      if (!s->d_poses_x || s->poses_x_cap < (size_t)L.B * nx) { s->d_poses_x = s->alloc<double>((size_t)L.B * nx); s->poses_x_cap = (size_t)L.B * nx; }
      copy_sync(s, s->d_poses_x, x, (size_t)L.B * nx * sizeof(double), hipMemcpyHostToDevice);
      d_x = s->d_poses_x;
    } else if (qp) {  // x_prev of the centroidal device loop: the head of its scratch (mpc_qp_ikid_low_level_steps), complete once that call returned
      const QpIdBuffers q = qp_id_buffers(qp);
      if (q.B != L.B || (size_t)(q.nq + q.nv) != nx || q.device != s->dims.device)
        throw std::runtime_error("walk_poses_update: the QP handle must have the plan's batch size and device and the model handle's state size");
      bool* kept = nullptr;
      const double* scr = qp_ikid_scratch(qp, 0, &kept);
      if (!scr || !*kept) throw std::runtime_error("walk_poses_update: the QP handle keeps no measurement (mpc_qp_ikid_low_level_steps first, or pass x)");
      d_x = scr;
    } else throw std::runtime_error("walk_poses_update: measured states are needed (x, or the QP handle that keeps them)");
    if (forward && s->poses_cmd_on)
      throw std::runtime_error("walk_poses_update: forward is refused while a command table is set (mpc_walk_poses_set_commands: every robot walks its own row; set the stopped rows instead)");
    if (forward) { std::memcpy(c.t_left, forward, 24); std::memcpy(c.t_right, forward + 3, 24); c.swing_apex = forward[6]; }
    const bool replanning = land_LF < 0 || land_RF < 0 || (takeoff_RF >= 0 && takeoff_RF < c.T_ds) || (takeoff_LF >= 0 && takeoff_LF < c.T_ds);
    hipLaunchKernelGGL(k_walk_poses, dim3(L.B), dim3(128), 0, s->stream, s->args(), (const int32_t*)model->d_model_i, (const double*)model->d_model_d, d_x, (int)nx,
                       c, s->d_poses_state, s->d_poses_samples, (int)takeoff_RF, (int)takeoff_LF, (int)land_RF, (int)land_LF, replanning ? 1 : 0,
                       (const double*)(s->poses_cmd_on ? s->d_poses_cmd : nullptr));
    HIP_OK(hipGetLastError());
    // every knot's references were rewritten: records kept for tick reuse are stale, and the host mirror of the written ranges no longer says what the
    // device holds (poisoned once per slot until a host patch or a stage upload rewrites it, as in mpc_walk_update)
    for (int k = 0; k < L.N; ++k) s->slot_dirty[slot_of(s, k)] = 1;
    if (s->walk_poisoned.size() != (size_t)(L.N + 1)) s->walk_poisoned.assign(L.N + 1, 0);
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    const size_t istride = (size_t)(L.N + 1) * L.max_stage_doubles;
    for (int k = 0; k < L.N; ++k) {
      const int sl = slot_of(s, k);
      if (s->walk_poisoned[sl]) continue;
      for (int off : c.pose_offs)
        for (int b = 0; b < L.B; ++b) std::fill_n(s->h_inst_params.data() + (size_t)b * istride + (size_t)sl * L.max_stage_doubles + off, 3, qnan);
      s->walk_poisoned[sl] = 1;
    }
  })
}

int mpc_walk_poses_get_state(mpc_solver* s, double* out) {
  MPC_TRY(s, {
    if (!s->poses_on || !out) throw std::runtime_error("walk_poses_get_state: mpc_walk_poses_init first");
    copy_sync(s, out, s->d_poses_state, (size_t)s->L.B * 48 * sizeof(double), hipMemcpyDeviceToHost);
  })
}

int mpc_walk_poses_set_state(mpc_solver* s, const double* in) {
  MPC_TRY(s, {
    if (!s->poses_on || !in) throw std::runtime_error("walk_poses_set_state: mpc_walk_poses_init first");
    copy_sync(s, s->d_poses_state, in, (size_t)s->L.B * 48 * sizeof(double), hipMemcpyHostToDevice);
  })
}

int mpc_walk_poses_get_samples(mpc_solver* s, double* out) {
  MPC_TRY(s, {
    if (!s->poses_on || !out) throw std::runtime_error("walk_poses_get_samples: mpc_walk_poses_init first");
    copy_sync(s, out, s->d_poses_samples, (size_t)s->L.B * 48 * sizeof(double), hipMemcpyDeviceToHost);
  })
}

}  // extern "C"
