// pipeline_loops.h — the device loops of the three control pipelines: per period the controller's kernels, then one step of the plant (sim_host.h
// sim_step_enqueue), with nothing but kernels in between.  mpc_qp_low_level_steps (kinodynamic, include/mpc_qp_abi.h), mpc_qp_ikid_low_level_steps
// (centroidal, the same header) and mpc_feedback_low_level_steps (full dynamics, include/mpc_feedback_pipeline.h).  The controllers read sim_measured(sim): the measurement of
// the sensor model when it is on (include/mpc_sim_sensors.h), the true state otherwise; x_out, the record, the metrics and the contact rule are the
// true state's.  What the loops share is written once, ahead of them: where the plan lives (plan_view), the checks (loop_check_*), the choice of a
// feedback kernel's instantiation (loop_launch_feedback: HELD while a hand-over latency is armed on the plan, include/mpc_plan_latency.h, host side
// below) and the read-backs (loop_finish).  Each loop keeps its model checks, scratch, arguments and step.  Included at the end of mpc_hip.hip, after sim_host.h.
#pragma once

// the plan of a handle as the kernels find it (plan_view.h)
static PlanView plan_view(const mpc_solver* plan) {
  const Layout& P = plan->L;
  PlanView v;
  v.xs = plan->d_xs; v.us = plan->d_us; v.gains = plan->d_gains; v.knots = plan->d_knots;
  v.N = P.N; v.nx = P.nx; v.n = P.n; v.m = P.m; v.gain_stride = P.gain_stride; v.oK = P.oK; v.knot_stride = P.knot_stride; v.oXD = P.oXD;
  v.xd_off = P.space == MPC_SPACE_MULTIBODY ? P.n / 2 : 3;
  v.slot0 = plan->khead % P.N;
  return v;
}

// include/mpc_plan_latency.h: the three parts of the handle's buffer, and what the second instantiations of the feedback kernels get
static size_t plan_latency_width(const Layout& P) { return (size_t)MPC_PLAN_LATENCY_HELD(P.nx, P.n, P.m); }
static double* plan_latency_state(const mpc_solver* plan) { return plan->d_plan_lat + (size_t)plan->L.B * MPC_PLAN_LATENCY_PARAMS; }
static double* plan_latency_held(const mpc_solver* plan) { return plan_latency_state(plan) + (size_t)plan->L.B * MPC_PLAN_LATENCY_STATE; }
static PlanLatencyArgs plan_latency_args(const mpc_solver* plan) {
  PlanLatencyArgs h;
  h.state = plan_latency_state(plan); h.held = plan_latency_held(plan); h.W = (int)plan_latency_width(plan->L);
  return h;
}

// include/mpc_qp_contacts.h: a loop call on a QP handle whose contact source is not the schedule.  The checks (throws), then the arguments of
// k_pipe_contact_states: the caller's contact_states go to the schedule buffer and q.cs becomes an output of that kernel, once per step.
static PipeContactsArgs pipe_contacts_args(const char* who, const QpContactSource& qc, const mpc_solver* sim, int nk, int B, int32_t* cs) {
  if (nk != 2) throw std::runtime_error(std::string(who) + ": a contact source other than the schedule needs two contacts (nk = 2: the soles of mpc_sim_contacts)");
  if (!sim->plant.d_con)
    throw std::runtime_error(std::string(who) + ": a contact source other than the schedule needs the contact rule on the simulator handle (mpc_sim_contacts first)");
  PipeContactsArgs c;
  const SimContactRows cr = sim_contact_rows(sim, MPC_SIM_FOOT_SENSORS_FEED_QP);  // (the detected pair when the contact detector feeds the QPs)
  c.rows = cr.rows; c.width = cr.width; c.B = B; c.source = qc.source;
  c.sched = qc.sched; c.cs = cs; c.used = qc.used; c.counts = qc.counts;
  return c;
}
// (before the QP of a step: the rows as the contact rule left them after the step before are the state this QP is solved at)
static void pipe_contacts_enqueue(const PipeContactsArgs& c, hipStream_t st) {
  hipLaunchKernelGGL(k_pipe_contact_states, dim3((unsigned)((2 * c.B + 63) / 64)), dim3(64), 0, st, c);
}

// The frame of a loop, part one: its handles (`handles`: "two" or "three" of them) live on one device and hold one batch size ...
static void loop_check_handles(const char* who, const char* handles, const mpc_solver* plan, const mpc_solver* sim, int device, int B) {
  if (plan->dims.device != device || sim->dims.device != device) throw std::runtime_error(std::string(who) + ": the " + handles + " handles must live on one device");
  if (plan->L.B != B || sim->L.B != B) throw std::runtime_error(std::string(who) + ": the " + handles + " handles must have the same batch size");
}
// ... part two, behind the loop's own model checks: the plan is at rest, the simulator can take the steps, the streams other than the loop's are drained
static void loop_check_idle(const char* who, const mpc_solver* plan, mpc_solver* sim, int need, int steps, hipStream_t st) {
  if (plan->async_pending > 0) throw std::runtime_error(std::string(who) + ": the plan has ticks in flight (mpc_wait first)");
  sim_steps_check(sim, who, need, steps);
  HIP_OK(hipStreamSynchronize(plan->stream));
  if (sim->stream != st) HIP_OK(hipStreamSynchronize(sim->stream));
}
// the measurement a step starts from, kept (before the last step of a call: x_prev)
static void loop_keep_measurement(const mpc_solver* sim, hipStream_t st, double* d_xprev) {
  HIP_OK(hipMemcpyAsync(d_xprev, sim_measured(sim), (size_t)sim->L.B * sim->L.nx * sizeof(double), hipMemcpyDeviceToDevice, st));
}
// one workgroup of one wavefront per robot of a feedback kernel: its HELD instantiation while a latency is armed on the plan, its plain one otherwise
template <class Args> static void loop_launch_feedback(void (*held)(Args, PlanLatencyArgs), void (*plain)(Args, PlanLatencyArgs), const mpc_solver* plan, hipStream_t st, const Args& a) {
  const dim3 grid((unsigned)plan->L.B), block(64);
  if (plan->d_plan_lat) hipLaunchKernelGGL(held, grid, block, 0, st, a, plan_latency_args(plan));
  else hipLaunchKernelGGL(plain, grid, block, 0, st, a, PlanLatencyArgs{});
}
// ... part three, behind the last step: what the caller asked for into its arrays and the one synchronisation.  d_forces [B][nf]: forces + df, or wrenches
static void loop_finish(mpc_solver* sim, hipStream_t st, const double* d_xprev, double* x_prev, double* x_out, double* tau, const double* d_forces, int nf,
                        double* forces, const mpc_qp_info* d_info = nullptr, mpc_qp_info* info = nullptr) {
  const size_t B = sim->L.B, nx = sim->L.nx, nu = sim->L.m;
  if (x_prev) HIP_OK(hipMemcpyAsync(x_prev, d_xprev, B * nx * sizeof(double), hipMemcpyDeviceToHost, st));
  if (x_out) HIP_OK(hipMemcpyAsync(x_out, sim->d_x0, B * nx * sizeof(double), hipMemcpyDeviceToHost, st));
  if (tau) HIP_OK(hipMemcpyAsync(tau, sim->plant.d_simu, B * nu * sizeof(double), hipMemcpyDeviceToHost, st));
  if (forces) HIP_OK(hipMemcpyAsync(forces, d_forces, B * nf * sizeof(double), hipMemcpyDeviceToHost, st));
  if (info) HIP_OK(hipMemcpyAsync(info, d_info, B * sizeof(mpc_qp_info), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  sim->perfect_feedback = false;
}

// the two QP loops: the contact states of a call go to the QP, or (a source other than the schedule) to the schedule buffer k_pipe_contact_states reads
static PipeContactsArgs loop_contacts_begin(const char* who, const QpContactSource& qc, const QpIdBuffers& q, const mpc_solver* sim, int nk, const int32_t* contact_states) {
  const bool from_plant = qc.source != MPC_QP_CONTACTS_SCHEDULE;
  HIP_OK(hipMemcpyAsync(from_plant ? qc.sched : q.cs, contact_states, (size_t)q.B * nk * sizeof(int32_t), hipMemcpyHostToDevice, q.stream));
  return from_plant ? pipe_contacts_args(who, qc, sim, nk, q.B, q.cs) : PipeContactsArgs{};
}
// ... and their torque kernel (pipeline_glue.h): one wavefront per robot behind the QP's solve
static void loop_torque_enqueue(const QpIdBuffers& q, const QpContactSource& qc, int nk, const mpc_solver* sim, double* d_fnew, const double* d_taumax) {
  PipeTorqueArgs t;
  t.sol = q.sol; t.qn = q.n; t.nv = q.nv; t.nk = nk; t.f = q.f; t.f_new = d_fnew; t.sim_u = sim->plant.d_simu; t.tau_max = d_taumax;
  t.used = qc.source != MPC_QP_CONTACTS_SCHEDULE ? qc.used : nullptr;
  hipLaunchKernelGGL(k_pipe_torque, dim3((unsigned)q.B), dim3(64), 0, q.stream, t);
}

extern "C" {

// include/mpc_qp_abi.h: the low-level loop of the kinodynamic pipeline with nothing but the kernels between its stages.  Everything is enqueued on
// the QP handle's stream (the plan and the simulator are idle: their streams are drained first); one synchronisation at the end.
int mpc_qp_low_level_steps(mpc_qp_solver* qp, const mpc_qp_settings* S, mpc_solver* plan, mpc_solver* sim, int32_t nk, const int32_t* frames,
                           const double* weights, const double* cone, double kd, const int32_t* contact_states, const double* tau_max,
                           const double* x, int32_t steps, double dt, double* x_prev, double* x_out, double* tau, double* forces, mpc_qp_info* info) {
  if (!qp) return -2;
  try {
    const char* who = "qp_low_level_steps";
    if (!S || !plan || !sim || !contact_states || !tau_max) throw std::runtime_error("qp_low_level_steps: null argument");
    if (steps <= 0 || !(dt > 0.0)) throw std::runtime_error("qp_low_level_steps: steps and dt must be positive");
    const QpContactSource qc = qp_contact_source(qp);
    const bool from_plant = qc.source != MPC_QP_CONTACTS_SCHEDULE;
    if (from_plant) (void)pipe_contacts_args(who, qc, sim, nk, 0, nullptr);  // (the checks, before anything is allocated for another nk)
    qp_id_prepare(qp, nk, frames, weights, cone);
    const QpIdBuffers q = qp_id_buffers(qp);
    const Layout& P = plan->L;
    const Layout& Z = sim->L;
    const int nx = q.nq + q.nv, nu = q.nv - 6, nf = 6 * nk;
    loop_check_handles(who, "three", plan, sim, q.device, q.B);
    if (P.space != MPC_SPACE_MULTIBODY || P.nx != nx || P.n != 2 * q.nv || P.m != nf + nu || P.n > PIPE_MAX_N)
      throw std::runtime_error("qp_low_level_steps: the plan must be a multibody problem with nx = nq + nv and controls (6 nk contact wrench components, nv - 6 joint accelerations)");
    if (Z.nx != nx || Z.m != nu) throw std::runtime_error("qp_low_level_steps: the simulator handle must have the QP's model (nx = nq + nv, nu = nv - 6)");
    hipStream_t st = q.stream;
    loop_check_idle(who, plan, sim, SIM_STAGE0, steps, st);
    const size_t B = q.B;
    double* scr = qp_scratch(qp, B * nx + B * nf + nu);  // x before the last period | forces + df | tau_max
    double *d_xprev = scr, *d_fnew = scr + B * nx, *d_taumax = d_fnew + B * nf;
    sim_steps_begin(sim, st, x);
    const PipeContactsArgs pc = loop_contacts_begin(who, qc, q, sim, nk, contact_states);
    HIP_OK(hipMemcpyAsync(d_taumax, tau_max, nu * sizeof(double), hipMemcpyHostToDevice, st));
    PipeArgs p;
    p.plan = plan_view(plan); p.nq = q.nq; p.nv = q.nv; p.nk = nk;
    p.x = sim_measured(sim); p.xrob = q.xrob; p.acc = q.acc; p.f = q.f;
    const SolverArgs za = sim->args();
    for (int step = 0; step < steps; ++step) {
      if (step == steps - 1 && x_prev) loop_keep_measurement(sim, st, d_xprev);
      loop_launch_feedback(k_pipe_feedback<true>, k_pipe_feedback<false>, plan, st, p);
      if (from_plant) pipe_contacts_enqueue(pc, st);
      qp_id_enqueue(qp, S, kd);
      qp_launch_solve(qp, S);
      loop_torque_enqueue(q, qc, nk, sim, d_fnew, d_taumax);
      sim_step_enqueue(sim, st, za, 1, dt, false);
    }
    loop_finish(sim, st, d_xprev, x_prev, x_out, tau, d_fnew, nf, forces, q.info, info);
    return 0;
  } catch (const std::exception& e) {
    qp_set_error(qp, e.what());
    return -1;
  }
}

// include/mpc_qp_abi.h: the low-level loop of the centroidal pipeline (centroidal_talos.py:408-447) with nothing but the kernels between its stages:
// the task errors once, then per step the centroidal state of the measurement and the feedback forces, the IK + ID QP and the simulator step.  Everything
// is enqueued on the QP handle's stream (the plan and the simulator are idle: their streams are drained first); one synchronisation at the end.
int mpc_qp_ikid_low_level_steps(mpc_qp_solver* qp, const mpc_qp_settings* S, mpc_solver* plan, mpc_solver* sim, int32_t nk, const int32_t* frames,
                                int32_t base_frame, int32_t torso_frame, const double* weights, const double* gains, const double* cone, const double* l_box,
                                const double* u_box, const double* x_posture, const double* foot_refs, double ref_dt, const int32_t* contact_states,
                                const double* x, const double* x_ik, int32_t steps, double dt, double* x_prev, double* c_prev, double* x_out, double* tau,
                                double* forces, mpc_qp_info* info, double* ik_out) {
  if (!qp) return -2;
  try {
    const char* who = "qp_ikid_low_level_steps";
    if (!S || !plan || !sim || !frames || !weights || !gains || !cone || !l_box || !u_box || !x_posture || !contact_states)
      throw std::runtime_error("qp_ikid_low_level_steps: null argument");
    // foot_refs = NULL: the samples the plan's own generator keeps on the device (mpc_walk_poses_update) ; without one that is the null argument it was
    if (!foot_refs && !plan->poses_on) throw std::runtime_error("qp_ikid_low_level_steps: null argument");
    if (steps <= 0 || !(dt > 0.0) || !(ref_dt > 0.0)) throw std::runtime_error("qp_ikid_low_level_steps: steps, dt and ref_dt must be positive");
    if (nk != 2) throw std::runtime_error("qp_ikid_low_level_steps: two contacts (nk = 2) expected");
    const QpContactSource qc = qp_contact_source(qp);
    const bool from_plant = qc.source != MPC_QP_CONTACTS_SCHEDULE;
    if (from_plant) (void)pipe_contacts_args(who, qc, sim, nk, 0, nullptr);
    qp_ikid_prepare(qp, nk, frames, base_frame, torso_frame, weights, gains, cone, l_box, u_box);
    const QpIdBuffers q = qp_id_buffers(qp);
    const Layout& P = plan->L;
    const Layout& Z = sim->L;
    const int nx = q.nq + q.nv, nu = q.nv - 6, nf = 6 * nk, nik = CG_IK_DOUBLES(q.nv);
    loop_check_handles(who, "three", plan, sim, q.device, q.B);
    if (P.space != MPC_SPACE_VECTOR || P.nx != CG_NC || P.n != CG_NC || P.m != nf)
      throw std::runtime_error("qp_ikid_low_level_steps: the plan must be a centroidal problem (vector space, nx = 9) with controls of 6 nk contact wrench components");
    if (Z.nx != nx || Z.m != nu) throw std::runtime_error("qp_ikid_low_level_steps: the simulator handle must have the QP's model (nx = nq + nv, nu = nv - 6)");
    if (q.nj > CG_MAX_NJ) throw std::runtime_error("qp_ikid_low_level_steps: more moving joints than the glue kernels hold (64)");
    hipStream_t st = q.stream;
    loop_check_idle(who, plan, sim, SIM_STAGE0, steps, st);
    const size_t B = q.B;
    bool* kept = nullptr;
    // x before the last step (kept for the next call) | its new_x | forces + df | x_posture | foot references
    double* scr = qp_ikid_scratch(qp, B * nx + B * CG_NC + B * nf + nx + B * 48, &kept);
    double *d_xprev = scr, *d_cprev = d_xprev + B * nx, *d_fnew = d_cprev + B * CG_NC, *d_xpost = d_fnew + B * nf, *d_refs = d_xpost + nx;
    if (!x_ik && !*kept) throw std::runtime_error("qp_ikid_low_level_steps: x_ik is NULL and no earlier call kept a measurement");
    sim_steps_begin(sim, st, x);
    if (x_ik) HIP_OK(hipMemcpyAsync(d_xprev, x_ik, B * nx * sizeof(double), hipMemcpyHostToDevice, st));
    const PipeContactsArgs pc = loop_contacts_begin(who, qc, q, sim, nk, contact_states);
    HIP_OK(hipMemcpyAsync(d_xpost, x_posture, nx * sizeof(double), hipMemcpyHostToDevice, st));
    if (foot_refs) HIP_OK(hipMemcpyAsync(d_refs, foot_refs, B * 48 * sizeof(double), hipMemcpyHostToDevice, st));
    else HIP_OK(hipMemcpyAsync(d_refs, plan->d_poses_samples, B * 48 * sizeof(double), hipMemcpyDeviceToDevice, st));
    IkidGlueArgs g = {};
    g.mi = q.mi; g.md = q.md; g.nq = q.nq; g.nv = q.nv; g.nk = nk; g.plan = plan_view(plan);
    g.x_ik = d_xprev; g.x_post = d_xpost; g.refs = d_refs; g.ref_dt = ref_dt;
    g.fr[0] = frames[0]; g.fr[1] = frames[1]; g.fr[2] = base_frame; g.fr[3] = torso_frame; g.ik = q.ik;
    g.x = sim_measured(sim); g.xrob = q.xrob; g.f = q.f; g.c_prev = d_cprev;
    loop_launch_feedback(k_ikid_task_errors<true>, k_ikid_task_errors<false>, plan, st, g);
    HIP_OK(hipGetLastError());
    if (ik_out) HIP_OK(hipMemcpyAsync(ik_out, q.ik, B * nik * sizeof(double), hipMemcpyDeviceToHost, st));
    const SolverArgs za = sim->args();
    for (int step = 0; step < steps; ++step) {
      g.last = (step == steps - 1);
      if (g.last) loop_keep_measurement(sim, st, d_xprev);
      loop_launch_feedback(k_pipe_centroidal_feedback<true>, k_pipe_centroidal_feedback<false>, plan, st, g);
      if (from_plant) pipe_contacts_enqueue(pc, st);
      qp_ikid_enqueue(qp, S);
      qp_launch_solve(qp, S);
      loop_torque_enqueue(q, qc, nk, sim, d_fnew, nullptr);  // (no clamp: the QP's torque box is the limit)
      sim_step_enqueue(sim, st, za, 1, dt, false);
    }
    if (c_prev) HIP_OK(hipMemcpyAsync(c_prev, d_cprev, B * CG_NC * sizeof(double), hipMemcpyDeviceToHost, st));
    loop_finish(sim, st, d_xprev, x_prev, x_out, tau, d_fnew, nf, forces, q.info, info);
    *kept = true;
    return 0;
  } catch (const std::exception& e) {
    qp_set_error(qp, e.what());
    return -1;
  }
}

// include/mpc_feedback_pipeline.h: the low-level loop of the full-dynamics pipeline (fulldynamic_talos.py:512-530) with one kernel between the plan and
// the simulator step.  Everything is enqueued on the simulator handle's stream (the plan's is drained first); one synchronisation at the end.  Errors
// are reported on the plan's handle.
int mpc_feedback_low_level_steps(mpc_solver* plan, mpc_solver* sim, const double* x, int32_t steps, double dt, double* x_prev, double* x_out, double* tau,
                                 double* wrenches) {
  MPC_TRY(plan, {
    const char* who = "feedback_low_level_steps";
    if (!plan || !sim) throw std::runtime_error("feedback_low_level_steps: null handle");
    if (steps <= 0 || !(dt > 0.0)) throw std::runtime_error("feedback_low_level_steps: steps and dt must be positive");
    const Layout& P = plan->L;
    const Layout& Z = sim->L;
    loop_check_handles(who, "two", plan, sim, sim->dims.device, Z.B);
    if (P.space != MPC_SPACE_MULTIBODY || P.nx != Z.nx || P.n != Z.n || P.m != Z.m || P.n > PIPE_MAX_N)
      throw std::runtime_error("feedback_low_level_steps: the plan must be a multibody problem with the simulator's nx and joint-torque controls (m = nu = nv - 6)");
    hipStream_t st = sim->stream;
    loop_check_idle(who, plan, sim, SIM_NU | SIM_STAGE0, steps, st);
    if (x_prev && !sim->plant.d_xlast) sim->plant.d_xlast = sim->alloc<double>((size_t)Z.B * Z.nx);
    sim_steps_begin(sim, st, x);
    FdPipeArgs p;
    p.plan = plan_view(plan); p.nv = Z.n / 2; p.nq = Z.nx - Z.n / 2;
    p.x = sim_measured(sim); p.sim_u = sim->plant.d_simu;
    const SolverArgs za = sim->args();
    for (int step = 0; step < steps; ++step) {
      if (step == steps - 1 && x_prev) loop_keep_measurement(sim, st, sim->plant.d_xlast);
      loop_launch_feedback(k_pipe_state_feedback<true>, k_pipe_state_feedback<false>, plan, st, p);
      sim_step_enqueue(sim, st, za, 1, dt, wrenches != nullptr);
    }
    loop_finish(sim, st, sim->plant.d_xlast, x_prev, x_out, tau, sim->plant.d_simwr, 12, wrenches);
  })
}

// include/mpc_plan_latency.h: arm and reset, or (params = NULL) turn off and free.  Every check comes before anything changes.
int mpc_plan_latency(mpc_solver* plan, const double* params) {
  MPC_TRY(plan, {
    if (!plan) throw std::runtime_error("plan_latency: null handle");
    if (plan->async_pending > 0) throw std::runtime_error("plan_latency: the plan has ticks in flight (mpc_wait first)");
    const Layout& P = plan->L;
    const size_t B = P.B;
    if (params) {
      if (P.N < 2) throw std::runtime_error("plan_latency: the held record is knot 1 of the plan: a horizon of at least 2 knots is needed");
      if (P.n < (P.space == MPC_SPACE_MULTIBODY ? 12 : 9))  // (the xdot part: xdot[n/2 .. n/2 + 6) or xdot[3 .. 9))
        throw std::runtime_error("plan_latency: the plan must be one of the three pipelines' (multibody with a free-flyer base, or centroidal with n = 9)");
      const double hi[MPC_PLAN_LATENCY_PARAMS] = {MPC_PLAN_LATENCY_MAX_STEPS, MPC_PLAN_LATENCY_MAX_STEPS, 4294967295.0, 0.0};
      const char* name[MPC_PLAN_LATENCY_PARAMS] = {"steps", "jitter", "seed", "the reserved entry"};
      for (size_t b = 0; b < B; ++b)
        for (int i = 0; i < MPC_PLAN_LATENCY_PARAMS; ++i) {
          const double v = params[b * MPC_PLAN_LATENCY_PARAMS + i];
          const std::string who = std::string(name[i]) + " of robot " + std::to_string(b);
          if (!std::isfinite(v)) throw std::runtime_error("plan_latency: non-finite " + who);
          if (v != std::floor(v)) throw std::runtime_error("plan_latency: " + who + " is not an integer");
          if (v < 0.0 || v > hi[i]) throw std::runtime_error("plan_latency: " + who + " out of range (0 .. " + std::to_string((long long)hi[i]) + ")");
        }
    }
    HIP_OK(hipStreamSynchronize(plan->stream));
    if (!params) {
      if (plan->d_plan_lat) { HIP_OK(hipFree(plan->d_plan_lat)); plan->d_plan_lat = nullptr; }
      return 0;
    }
    const size_t doubles = B * (MPC_PLAN_LATENCY_PARAMS + MPC_PLAN_LATENCY_STATE + plan_latency_width(P));
    if (!plan->d_plan_lat) HIP_OK(hipMalloc((void**)&plan->d_plan_lat, doubles * sizeof(double)));
    HIP_OK(hipMemsetAsync(plan->d_plan_lat, 0, doubles * sizeof(double), plan->stream));
    copy_sync(plan, plan->d_plan_lat, params, B * MPC_PLAN_LATENCY_PARAMS * sizeof(double), hipMemcpyHostToDevice);
  })
}

// include/mpc_plan_latency.h: every robot's held record from knot 1 of the plan in the buffers, its draw and its countdown.  On the plan's stream:
// behind the run that made the plan, ahead of the run that replaces it ; the loops drain that stream before they read the rows.
int mpc_plan_latency_publish(mpc_solver* plan) {
  MPC_TRY(plan, {
    if (!plan) throw std::runtime_error("plan_latency_publish: null handle");
    if (!plan->d_plan_lat) throw std::runtime_error("plan_latency_publish: the latency model is off on this handle (arm it with mpc_plan_latency)");
    if (plan->async_pending > 0) throw std::runtime_error("plan_latency_publish: the plan has ticks in flight (mpc_wait first)");
    if (!plan->has_run) throw std::runtime_error("plan_latency_publish: the handle has never run: there is no plan to hold");
    PlanPublishArgs a;
    a.plan = plan_view(plan); a.slot1 = (plan->khead + 1) % plan->L.N;
    a.params = plan->d_plan_lat; a.state = plan_latency_state(plan); a.held = plan_latency_held(plan); a.W = (int)plan_latency_width(plan->L);
    hipLaunchKernelGGL(k_plan_latency_publish, dim3((unsigned)plan->L.B), dim3(PLAN_LAT_THREADS), 0, plan->stream, a);
    HIP_OK(hipGetLastError());
  })
}

int mpc_plan_latency_read(mpc_solver* plan, double* params, double* state, double* held) {
  MPC_TRY(plan, {
    if (!plan) throw std::runtime_error("plan_latency_read: null handle");
    if (!plan->d_plan_lat) throw std::runtime_error("plan_latency_read: the latency model is off on this handle (arm it with mpc_plan_latency)");
    const size_t B = plan->L.B;
    if (params) copy_sync(plan, params, plan->d_plan_lat, B * MPC_PLAN_LATENCY_PARAMS * sizeof(double), hipMemcpyDeviceToHost);
    if (state) copy_sync(plan, state, plan_latency_state(plan), B * MPC_PLAN_LATENCY_STATE * sizeof(double), hipMemcpyDeviceToHost);
    if (held) copy_sync(plan, held, plan_latency_held(plan), B * plan_latency_width(plan->L) * sizeof(double), hipMemcpyDeviceToHost);
  })
}

}  // extern "C"
