// sim_host.h — host side of the torque-driven simulator (the plant): mpc_simulate_torque and the entry points of include/mpc_sim_ext.h (push, record),
// mpc_sim_metrics.h, mpc_sim_contacts.h, mpc_sim_terrain.h, mpc_sim_actuators.h, mpc_sim_sensors.h, mpc_sim_estimator.h, mpc_sim_foot_sensors.h, mpc_sim_plant.h, mpc_sim_friction.h and mpc_sim_disturbances.h.  Its state is mpc_solver::plant (SimPlant); its kernels
// are in sim_record.h, sim_metrics.h, sim_contacts.h, sim_terrain.h, sim_actuators.h, sim_sensors.h, sim_estimator.h, sim_foot_sensors.h, sim_plant.h, sim_friction.h and sim_disturbances.h.  Every caller that steps the plant — mpc_simulate_torque here, the device
// loops of the three pipelines in pipeline_loops.h — goes through sim_steps_check, sim_steps_begin and sim_step_enqueue: an extension of the simulator
// is added there, once.  Included at the end of mpc_hip.hip (mpc_solver, MPC_TRY, copy_sync, slot_of).
#pragma once

// Which handles an entry point takes.  Every simulator handle is a whole-body handle; SIM_NU: with nu = nv - 6 (the handle of mpc_simulate_torque) ;
// SIM_STAGE0: whose stage 0 holds contact dynamics (what a step integrates: the pipelines set stage 0 per contact state, so only the stepping calls ask)
enum : int { SIM_NU = 1, SIM_STAGE0 = 2 };
static void sim_check(const mpc_solver* s, const char* who, int need = SIM_NU) {
  const Layout& L = s->L;
  bool ok = L.space == MPC_SPACE_MULTIBODY;
  if (need & SIM_NU) ok = ok && L.m == L.n / 2 - 6 && L.nx == L.n / 2 + (L.n / 2 + 1);
  if (need & SIM_STAGE0) ok = ok && s->h_desc[(size_t)slot_of(s, 0) * L.max_stage_ints] == MPC_DYN_MULTIBODY_CONSTRAINT_SEMIEULER;
  if (!ok)
    throw std::runtime_error(std::string(who) + ": the simulator handle must be a whole-body handle" + ((need & SIM_NU) ? " with nu = nv - 6" : "") +
                             ((need & SIM_STAGE0) ? " and contact dynamics in stage 0" : "") + " (the handle of mpc_simulate_torque)");
}
// the kernels of the record, the metrics and the contact rule read the two sole contacts of the model and hold at most CG_MAX_NJ moving joints
static void sim_model_check(const mpc_solver* s, const char* who) {
  if (s->h_model_i.size() < 5 || s->h_model_i[4] < 2)
    throw std::runtime_error(std::string(who) + ": the model of the simulator handle must hold the two sole contacts (contacts 0 and 1)");
  if (s->L.nj > CG_MAX_NJ) throw std::runtime_error(std::string(who) + ": more moving joints than the simulator's kernels hold (" + std::to_string(CG_MAX_NJ) + ")");
}
// the torques and wrenches of a step.  alloc zero-fills on the handle's own stream: it is drained here, so that the buffers may be used from any stream at
// once (the loops of the QP pipelines step the plant on the QP handle's)
static void sim_ensure(mpc_solver* s) {
  if (s->plant.d_simu) return;
  s->plant.d_simu = s->alloc<double>((size_t)s->L.B * s->L.m);
  s->plant.d_simwr = s->alloc<double>((size_t)s->L.B * 12);
  HIP_OK(hipStreamSynchronize(s->stream));
}
// a buffer the plant owns (SimPlant::free_owned) is replaced by one of `count` doubles, 0: dropped; nothing in flight on the handle's stream reads the old one
static void sim_realloc(mpc_solver* s, double*& buf, size_t count) {
  HIP_OK(hipStreamSynchronize(s->stream));
  if (buf) { HIP_OK(hipFree(buf)); buf = nullptr; }
  if (count) { void* p = nullptr; HIP_OK(hipMalloc(&p, count * sizeof(double))); buf = (double*)p; }
}
// the *_width entry points: the width on a simulator handle, -1 otherwise
template <class F> static int32_t sim_width(mpc_solver* s, const char* who, F&& width) {
  if (!s) return -1;
  try {
    sim_check(s, who);
    return (int32_t)width();
  } catch (const std::exception& e) {
    s->err = e.what();
    return -1;
  }
}

// the model tables the plant is integrated and recorded with (include/mpc_sim_plant.h): robot b's own table at sim_plant_md + b * sim_plant_stride
// while the plant model is on, the handle's one table (stride 0) otherwise.  Everything else keeps s->d_model_d, the controllers' belief
static double* sim_plant_tables(const mpc_solver* s) { return s->plant.d_plant + s->plant.plant_off; }
static const double* sim_plant_md(const mpc_solver* s) { return s->plant.d_plant ? sim_plant_tables(s) : s->d_model_d; }
static size_t sim_plant_stride(const mpc_solver* s) { return s->plant.d_plant ? s->plant.plant_nd : 0; }

// the disturbance schedule (include/mpc_sim_disturbances.h), one allocation: events | state rows | what acts in the step [B][6] | its link int32 [B]
static double* sim_disturbances_rows(const mpc_solver* s) { return s->plant.d_dis + (size_t)s->L.B * s->plant.dis_ne * MPC_SIM_DISTURBANCES_EVENT; }
static double* sim_disturbances_out(const mpc_solver* s) { return sim_disturbances_rows(s) + (size_t)s->L.B * MPC_SIM_DISTURBANCES_WIDTH; }
static size_t sim_disturbances_doubles(const Layout& L, int ne) {
  return (size_t)L.B * ((size_t)ne * MPC_SIM_DISTURBANCES_EVENT + MPC_SIM_DISTURBANCES_WIDTH + 6) + ((size_t)L.B + 1) / 2;
}
// the schedule's event of the step of length dt_step about to be enqueued on stream st (sim_disturbances.h), when the model is on: it reads the state
// the step starts from and the rows the contact rule left after the step before
static void sim_disturbances_enqueue(mpc_solver* s, hipStream_t st, double dt_step) {
  const SimPlant& p = s->plant;
  if (!p.d_dis) return;
  const Layout& L = s->L;
  SimDisturbancesArgs a;
  a.mi = s->d_model_i; a.md = s->d_model_d; a.nv = L.n / 2; a.nq = L.nx - L.n / 2;
  a.x = s->d_x0; a.con = p.d_con; a.events = p.d_dis; a.n_events = p.dis_ne;
  a.rows = sim_disturbances_rows(s); a.out = sim_disturbances_out(s); a.link = (int32_t*)(a.out + (size_t)L.B * 6); a.dt = dt_step;
  hipLaunchKernelGGL(k_sim_disturbances, dim3((unsigned)L.B), dim3(CG_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
}
// the state rows, what acts and its link after arming or a reset: clock 0, nothing counted, nothing fired, no pair seen, nothing acting
static void sim_disturbances_reset(mpc_solver* s) {
  const Layout& L = s->L;
  const size_t head = (size_t)L.B * s->plant.dis_ne * MPC_SIM_DISTURBANCES_EVENT, count = sim_disturbances_doubles(L, s->plant.dis_ne) - head;
  std::vector<double> h(count, 0.0);
  for (int b = 0; b < L.B; ++b) {
    double* r = h.data() + (size_t)b * MPC_SIM_DISTURBANCES_WIDTH;
    r[SIM_DIS_O_ACTING] = r[SIM_DIS_O_LINK] = r[SIM_DIS_O_SEEN] = r[SIM_DIS_O_SEEN + 1] = -1.0;
    for (int e = 0; e < MPC_SIM_DISTURBANCES_MAX_EVENTS; ++e) r[SIM_DIS_O_FIRE + e] = -1.0;
  }
  int32_t* link = (int32_t*)(h.data() + (size_t)L.B * (MPC_SIM_DISTURBANCES_WIDTH + 6));
  for (int b = 0; b < L.B; ++b) link[b] = -1;
  HIP_OK(hipStreamSynchronize(s->stream));
  copy_sync(s, sim_disturbances_rows(s), h.data(), count * sizeof(double), hipMemcpyHostToDevice);
}
static void sim_disturbances_drop(mpc_solver* s) {
  sim_realloc(s, s->plant.d_dis, 0);
  s->plant.h_dis.clear();
  s->plant.dis_ne = 0;
  s->plant.dis_contact = false;
}

// the record of the step just enqueued on stream st (sim_record.h), when recording is on
static void sim_record_enqueue(mpc_solver* s, hipStream_t st) {
  SimPlant& p = s->plant;
  if (p.rec_cap <= 0) return;
  const Layout& L = s->L;
  SimRecordArgs r;
  r.mi = s->d_model_i; r.md = sim_plant_md(s); r.md_stride = sim_plant_stride(s); r.nv = L.n / 2; r.nq = L.nx - L.n / 2;
  r.x = s->d_x0; r.tau = p.d_simu; r.wr = p.d_simwr; r.push = p.d_dis ? sim_disturbances_out(s) : (p.push_width ? p.d_push : nullptr); r.push_width = p.d_dis ? 6 : p.push_width;  // (the schedule: what acted)
  r.out = p.d_rec + (size_t)p.rec_count * L.B * sim_record_width(L.nx, L.m);
  hipLaunchKernelGGL(k_sim_record, dim3((unsigned)L.B), dim3(CG_THREADS), 0, st, r);
  HIP_OK(hipGetLastError());
  p.rec_count++;
}
// the terrain of the contact rule as the kernels take it (sim_terrain.h): boxes nullptr without one
static SimTerrain sim_terrain_args(const mpc_solver* s) {
  const SimPlant& p = s->plant;
  SimTerrain t;
  t.boxes = p.d_con ? p.d_ter : nullptr;
  t.n = p.ter_cfg.n_boxes;
  t.stride = p.ter_cfg.per_robot ? p.ter_cfg.n_boxes * MPC_SIM_TERRAIN_BOX_WIDTH : 0;
  return t;
}
// the metrics of the step of length dt just enqueued on stream st (sim_metrics.h), when they are on
static void sim_metrics_enqueue(mpc_solver* s, hipStream_t st, double dt) {
  const SimPlant& p = s->plant;
  if (!p.d_met) return;
  const Layout& L = s->L;
  SimMetricsArgs m;
  m.mi = s->d_model_i; m.md = sim_plant_md(s); m.md_stride = sim_plant_stride(s); m.nv = L.n / 2; m.nq = L.nx - L.n / 2;
  m.x = s->d_x0; m.tau = p.d_simu; m.wr = p.d_simwr; m.dt = dt; m.cfg = p.met_cfg;
  m.acc = p.d_met; m.frozen = p.d_met + (size_t)L.B * MPC_SIM_METRICS_WIDTH; m.xs = m.frozen + L.B;
  m.ter = sim_terrain_args(s); m.con = p.d_con; m.ground_z = p.con_cfg.ground_z;
  hipLaunchKernelGGL(k_sim_metrics, dim3((unsigned)L.B), dim3(CG_THREADS), 0, st, m);
  HIP_OK(hipGetLastError());
}
// the rows after a reset: nothing accumulated, no fall, nothing latched (the margin's minimum, the heights and the centres of mass NaN); not frozen
static void sim_metrics_reset(mpc_solver* s) {
  const Layout& L = s->L;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> h((size_t)L.B * (MPC_SIM_METRICS_WIDTH + 1), 0.0);
  for (int b = 0; b < L.B; ++b) {
    double* r = h.data() + (size_t)b * MPC_SIM_METRICS_WIDTH;
    r[6] = nan;
    r[11] = -1.0;
    for (int i = 12; i < MPC_SIM_METRICS_WIDTH; ++i) r[i] = nan;
  }
  copy_sync(s, s->plant.d_met, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
}
// the contact rule after the step just enqueued on stream st (sim_contacts.h), when it is on
static void sim_contacts_enqueue(mpc_solver* s, hipStream_t st) {
  const SimPlant& p = s->plant;
  if (!p.d_con) return;
  const Layout& L = s->L;
  SimContactsArgs c;
  c.mi = s->d_model_i; c.md = s->d_model_d; c.nv = L.n / 2; c.nq = L.nx - L.n / 2;
  c.x = s->d_x0; c.wr = p.d_simwr; c.cfg = p.con_cfg; c.rows = p.d_con; c.ter = sim_terrain_args(s);
  hipLaunchKernelGGL(k_sim_contacts, dim3((unsigned)L.B), dim3(CG_THREADS), 0, st, c);
  HIP_OK(hipGetLastError());
}
// the rows after a reset: both soles in contact at the model's ground-side placements (contacts 0 and 1), nothing counted
static void sim_contacts_reset(mpc_solver* s) {
  const Layout& L = s->L;
  const int nj = s->h_model_i[0], nframes = s->h_model_i[3];
  const size_t off = MPC_MODEL_HEADER_DOUBLES + (size_t)MPC_MODEL_JOINT_DOUBLES * nj + (size_t)MPC_MODEL_FRAME_DOUBLES * nframes;
  double cm[2 * MPC_MODEL_CONTACT_DOUBLES];
  copy_sync(s, cm, s->d_model_d + off, sizeof(cm), hipMemcpyDeviceToHost);
  std::vector<double> h((size_t)L.B * MPC_SIM_CONTACTS_WIDTH, 0.0);
  for (int b = 0; b < L.B; ++b) {
    double* r = h.data() + (size_t)b * MPC_SIM_CONTACTS_WIDTH;
    for (int i = 0; i < 2; ++i) {
      const double* c = cm + MPC_MODEL_CONTACT_DOUBLES * i;
      r[i] = 1.0;
      r[6 + i] = c[23];                                          // z_prev: the anchor's height
      for (int e = 0; e < 12; ++e) r[8 + 12 * i + e] = c[12 + e];  // R2 (9), p2 (3)
      r[36 + i] = r[38 + i] = -1.0;
    }
  }
  copy_sync(s, s->plant.d_con, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
}

static size_t sim_actuators_width(const Layout& L) { return (size_t)(MPC_SIM_ACTUATORS_RING + 2) * L.m + 2; }
static double* sim_actuators_rows(const mpc_solver* s) { return s->plant.d_act + (size_t)s->L.B * MPC_SIM_ACTUATORS_PARAMS + 2 * (size_t)s->L.m; }
// the actuator model of the step of length dt_step about to be enqueued on stream st (sim_actuators.h), when it is on
static void sim_actuators_enqueue(mpc_solver* s, hipStream_t st, double dt_step) {
  const SimPlant& p = s->plant;
  if (!p.d_act) return;
  const Layout& L = s->L;
  SimActuatorsArgs a;
  a.nv = L.n / 2; a.nq = L.nx - L.n / 2; a.nu = L.m;
  a.x = s->d_x0; a.tau = p.d_simu;
  a.params = p.d_act; a.limit = p.d_act + (size_t)L.B * MPC_SIM_ACTUATORS_PARAMS; a.shape = a.limit + L.m;
  a.rows = sim_actuators_rows(s); a.dt = dt_step;
  hipLaunchKernelGGL(k_sim_actuators, dim3((unsigned)L.B), dim3(SIM_ACT_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
}

static size_t sim_sensors_width(const Layout& L) { return (size_t)(MPC_SIM_SENSORS_RING + 1) * L.nx + 2 * (size_t)L.m + 2; }
static double* sim_sensors_meas(const mpc_solver* s) { return s->plant.d_sen + (size_t)s->L.B * MPC_SIM_SENSORS_PARAMS; }
static double* sim_sensors_stage(const mpc_solver* s) { return sim_sensors_meas(s) + (size_t)s->L.B * s->L.nx; }
static double* sim_sensors_rows(const mpc_solver* s) { return sim_sensors_stage(s) + (size_t)s->L.B * s->L.nx; }
// what the sensors deliver, [B][nx]: the measurement of the sensor model when it is on, the true state otherwise
static const double* sim_sensed(const mpc_solver* s) { return s->plant.d_sen ? sim_sensors_meas(s) : s->d_x0; }
static double* sim_estimator_est(const mpc_solver* s) { return s->plant.d_est + (size_t)s->L.B * MPC_SIM_ESTIMATOR_PARAMS; }
static double* sim_estimator_stage(const mpc_solver* s) { return sim_estimator_est(s) + (size_t)s->L.B * s->L.nx; }
static double* sim_estimator_rows(const mpc_solver* s) { return sim_estimator_stage(s) + (size_t)s->L.B * s->L.nx; }
static size_t sim_estimator_width(const Layout& L) { return (size_t)L.nx + MPC_SIM_ESTIMATOR_TAIL; }
// the state the controllers read, [B][nx]: the estimate of the base-state estimator when it is on, what the sensors deliver otherwise
static const double* sim_measured(const mpc_solver* s) { return s->plant.d_est ? sim_estimator_est(s) : sim_sensed(s); }
// the measurement event of the true states x, produced by a step of length dt_step, on stream st (sim_sensors.h), when the model is on
static void sim_sensors_enqueue(mpc_solver* s, hipStream_t st, const double* x, double dt_step) {
  const SimPlant& p = s->plant;
  if (!p.d_sen) return;
  const Layout& L = s->L;
  SimSensorsArgs a;
  a.nv = L.n / 2; a.nq = L.nx - L.n / 2; a.nu = L.m;
  a.x = x; a.params = p.d_sen; a.xm = sim_sensors_meas(s); a.rows = sim_sensors_rows(s); a.dt = dt_step;
  hipLaunchKernelGGL(k_sim_sensors, dim3((unsigned)L.B), dim3(SIM_SEN_THREADS), sim_sensors_lds_bytes(a.nv), st, a);
  HIP_OK(hipGetLastError());
}

static double* sim_foot_sensors_rows(const mpc_solver* s) { return s->plant.d_fs + (size_t)s->L.B * MPC_SIM_FOOT_SENSORS_PARAMS; }
// the rows a consumer of contact flags indexes by 0 and 1, and their width: the state rows of the contact detector when it feeds that consumer
// (mpc_sim_foot_sensors_feed: one MPC_SIM_FOOT_SENSORS_FEED_* bit), the rows of the contact rule otherwise
struct SimContactRows { const double* rows; int width; };
static SimContactRows sim_contact_rows(const mpc_solver* s, int consumer) {
  const SimPlant& p = s->plant;
  if (p.d_fs && (p.fs_feed & consumer)) return {sim_foot_sensors_rows(s), MPC_SIM_FOOT_SENSORS_WIDTH};
  return {p.d_con, MPC_SIM_CONTACTS_WIDTH};
}
// the detection event of the wrenches of the step of length dt_step just enqueued on stream st (sim_foot_sensors.h), when the model is on
static void sim_foot_sensors_enqueue(mpc_solver* s, hipStream_t st, double dt_step) {
  const SimPlant& p = s->plant;
  if (!p.d_fs) return;
  SimFootSensorsArgs a;
  a.wr = p.d_simwr; a.con = p.d_con; a.params = p.d_fs; a.rows = sim_foot_sensors_rows(s); a.dt = dt_step;
  hipLaunchKernelGGL(k_sim_foot_sensors, dim3((unsigned)s->L.B), dim3(SIM_FS_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
}
// the state rows after arming: det = the in_contact pair of the contact rule's rows (`con` the rows on the host, NULL: read from the device),
// everything else 0.  Host work, not part of the steady loop
static void sim_foot_sensors_arm(mpc_solver* s, const double* con) {
  if (!s->plant.d_fs) return;
  const Layout& L = s->L;
  std::vector<double> c;
  if (!con) {
    c.resize((size_t)L.B * MPC_SIM_CONTACTS_WIDTH);
    HIP_OK(hipStreamSynchronize(s->stream));
    copy_sync(s, c.data(), s->plant.d_con, c.size() * sizeof(double), hipMemcpyDeviceToHost);
    con = c.data();
  }
  std::vector<double> h((size_t)L.B * MPC_SIM_FOOT_SENSORS_WIDTH, 0.0);
  for (int b = 0; b < L.B; ++b)
    for (int i = 0; i < 2; ++i) h[(size_t)b * MPC_SIM_FOOT_SENSORS_WIDTH + i] = con[(size_t)b * MPC_SIM_CONTACTS_WIDTH + i] != 0.0 ? 1.0 : 0.0;
  HIP_OK(hipStreamSynchronize(s->stream));
  copy_sync(s, sim_foot_sensors_rows(s), h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
}
static void sim_foot_sensors_drop(mpc_solver* s) {
  sim_realloc(s, s->plant.d_fs, 0);
  s->plant.h_fs.clear();
  s->plant.fs_feed = 0;
}

// the estimation event of the measured states xm and the true states xt on stream st (sim_estimator.h), when the estimator is on: it reads the rows
// of the contact rule, or of the contact detector when that feeds it (sim_contact_rows), as they stand on the stream
static void sim_estimator_enqueue(mpc_solver* s, hipStream_t st, const double* xm, const double* xt) {
  const SimPlant& p = s->plant;
  if (!p.d_est) return;
  const Layout& L = s->L;
  SimEstimatorArgs a;
  a.mi = s->d_model_i; a.md = s->d_model_d; a.nv = L.n / 2; a.nq = L.nx - L.n / 2;
  const SimContactRows cr = sim_contact_rows(s, MPC_SIM_FOOT_SENSORS_FEED_ESTIMATOR);
  a.xm = xm; a.xt = xt; a.con = cr.rows; a.con_width = cr.width; a.params = p.d_est; a.xe = sim_estimator_est(s); a.rows = sim_estimator_rows(s);
  hipLaunchKernelGGL(k_sim_estimator, dim3((unsigned)L.B), dim3(CG_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
}
// the friction model of the step of length dt_step just enqueued on stream st, after the contact rule (sim_friction.h), when the model is on
static double* sim_friction_rows(const mpc_solver* s) { return s->plant.d_fr + (size_t)s->L.B * MPC_SIM_FRICTION_PARAMS; }
static void sim_friction_enqueue(mpc_solver* s, hipStream_t st, double dt_step) {
  const SimPlant& p = s->plant;
  if (!p.d_fr) return;
  SimFrictionArgs a;
  a.B = s->L.B; a.wr = p.d_simwr; a.con = p.d_con; a.params = p.d_fr; a.rows = sim_friction_rows(s); a.dt = dt_step;
  hipLaunchKernelGGL(k_sim_friction, dim3((unsigned)((2 * s->L.B + SIM_FR_THREADS - 1) / SIM_FR_THREADS)), dim3(SIM_FR_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
}
static void sim_friction_drop(mpc_solver* s) {
  sim_realloc(s, s->plant.d_fr, 0);
  s->plant.h_fr.clear();
}
static void sim_estimator_drop(mpc_solver* s) {
  sim_realloc(s, s->plant.d_est, 0);
  s->plant.h_est.clear();
}

// the plant model's tables, built from the rows in force (h_plant) and the handle's nominal table: when the model is armed, and when mpc_set_model
// replaced the nominal table of an armed handle (the joint count is then unchanged; the table may have grown by a frame).  Synchronous: the tables
// may be read from any stream at once (the loops of the QP pipelines step the plant on the QP handle's).  Host work, not part of the steady loop
static void sim_plant_build(mpc_solver* s) {
  SimPlant& p = s->plant;
  if (!p.d_plant) return;
  const Layout& L = s->L;
  const size_t head = p.plant_off;
  if (p.plant_nd != s->model_nd) {
    sim_realloc(s, p.d_plant, head + (size_t)L.B * s->model_nd);
    p.plant_nd = s->model_nd;
  }
  copy_sync(s, p.d_plant, p.h_plant.data(), head * sizeof(double), hipMemcpyHostToDevice);
  SimPlantArgs a;
  a.md = s->d_model_d; a.nd = (int)p.plant_nd; a.nj = L.nj;
  a.params = p.d_plant; a.link_scale = p.d_plant + (size_t)L.B * MPC_SIM_PLANT_PARAMS; a.tables = sim_plant_tables(s);
  hipLaunchKernelGGL(k_sim_plant_models, dim3((unsigned)L.B), dim3(SIM_PLANT_THREADS), 0, s->stream, a);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(s->stream));
}

// A call that steps the plant `steps` times, part one: everything that can fail, before anything is enqueued.  `need`: sim_check.
static void sim_steps_check(mpc_solver* s, const char* who, int need, int steps) {
  const SimPlant& p = s->plant;
  sim_check(s, who, need);
  if (p.rec_cap > 0 && p.rec_count + steps > p.rec_cap)  // (every step gets its record slot)
    throw std::runtime_error("sim_record: the record ring is full (" + std::to_string(p.rec_count) + " of " + std::to_string(p.rec_cap) + " steps held, " +
                             std::to_string(steps) + " more asked for): read it with mpc_sim_record_read or enlarge it with mpc_sim_record");
  const int32_t* d = s->h_desc.data() + (size_t)slot_of(s, 0) * s->L.max_stage_ints;
  if (p.d_con && (d[0] != MPC_DYN_MULTIBODY_CONSTRAINT_SEMIEULER || d[1] != 2 || !((d[2] == 0 && d[3] == 1) || (d[2] == 1 && d[3] == 0))))
    throw std::runtime_error(std::string(who) + ": the contact rule is on (mpc_sim_contacts), so stage 0 of the simulator handle must be the double-support "
                             "stage (contact dynamics of contacts 0 and 1): the rule picks each robot's contacts out of its two");
  sim_ensure(s);
}
// ... part two, on the stream st the steps will be enqueued on: the state they start from (x NULL: the one the handle holds), which the metrics keep
// for the joint power of the first step
static void sim_steps_begin(mpc_solver* s, hipStream_t st, const double* x) {
  const Layout& L = s->L;
  if (x) HIP_OK(hipMemcpyAsync(s->d_x0, x, (size_t)L.B * L.nx * sizeof(double), hipMemcpyHostToDevice, st));
  if (s->plant.d_met)
    HIP_OK(hipMemcpyAsync(s->plant.d_met + (size_t)L.B * (MPC_SIM_METRICS_WIDTH + 1), s->d_x0, (size_t)L.B * L.nx * sizeof(double), hipMemcpyDeviceToDevice, st));
}
// One step of the plant on stream st: `substeps` integration steps of length dt under the torque the caller put into plant.d_simu.  The order is the
// contract of the extensions.  The disturbance schedule (include/mpc_sim_disturbances.h) before everything: from the state the step starts from and the
// rows the contact rule left after the step before it writes the force, point and link that act in this step's dynamics, in place of the armed push.
// The actuator model next: it turns the command into the applied torque in place, over the whole step (substeps * dt),
// and everything after it sees the applied torque.  Then the dynamics, with the armed push and the contacts the rule's rows held when the step BEFORE
// ended (the rows the low-level QPs of pipeline_loops.h read for this step); wrenches are written when the caller, the record, the metrics or the rule
// want them.  Then the record and the metrics of the step: the new state, the applied torque, its wrenches, the rows it was integrated with.  The
// contact rule: it rewrites the rows for the NEXT step from the new state and this step's wrenches.  The sensor model last: the measurement event of
// the new state, over the whole step.  The base-state estimator after it: the estimation event of that measurement (the true state without a
// sensor model) and of the rows the contact rule just wrote; nothing of this step reads either, the controllers of the next step do (sim_measured).  Between the two, the foot force sensors and
// the contact detector: the detection event of this step's wrenches (which the dynamics then always write), so that an estimator fed by detection reads
// the pair this step's event left, and the low-level QPs of the next step the same pair.  The friction model (include/mpc_sim_friction.h) directly
// after the contact rule: from this step's wrenches and the flags the rule just wrote it sets the slip velocity each held sole has in the NEXT
// step's dynamics, and advances the anchors of the soles that slid in this one.  In one line: disturbances -> actuator model -> dynamics -> record -> metrics
// -> contact rule -> friction -> sensors -> foot sensors -> estimator.  The plant model (include/mpc_sim_plant.h) launches nothing here: the dynamics, the record and
// the metrics read robot b's own model table, built when the model was armed.
static void sim_step_enqueue(mpc_solver* s, hipStream_t st, const SolverArgs& args, int substeps, double dt, bool want_wrenches) {
  const SimPlant& p = s->plant;
  sim_disturbances_enqueue(s, st, substeps * dt);
  sim_actuators_enqueue(s, st, substeps * dt);
  const double* push = p.d_dis ? sim_disturbances_out(s) : (p.push_width ? p.d_push : nullptr);  // (the two exclude each other: mpc_sim_set_push)
  launch_eval_multibody(st, args, s->LT, s->d_tknots, s->d_mbwork, s->mb_work_stride, true, 0, 1, substeps, dt, false, push, true,
                        p.d_simu, (want_wrenches || p.rec_cap > 0 || p.d_met || p.d_con || p.d_fs || p.d_fr) ? p.d_simwr : nullptr,
                        p.d_dis ? 6 : (p.push_width ? p.push_width : 3), p.d_con,
                        p.d_plant ? sim_plant_tables(s) : nullptr, sim_plant_stride(s), p.d_fr ? sim_friction_rows(s) : nullptr, p.d_dis != nullptr);
  HIP_OK(hipGetLastError());
  sim_record_enqueue(s, st);
  sim_metrics_enqueue(s, st, substeps * dt);
  sim_contacts_enqueue(s, st);
  sim_friction_enqueue(s, st, substeps * dt);
  sim_sensors_enqueue(s, st, s->d_x0, substeps * dt);
  sim_foot_sensors_enqueue(s, st, substeps * dt);
  sim_estimator_enqueue(s, st, sim_sensed(s), s->d_x0);
}

extern "C" {

// ---- include/mpc_sim_ext.h: push and record -----------------------------------------------------------------------------------------------
int mpc_sim_set_push(mpc_solver* s, const double* f_ext, int32_t width) {
  MPC_TRY(s, {
    sim_check(s, "sim_set_push");
    if (!f_ext) { s->plant.push_width = 0; return 0; }
    if (s->plant.d_dis)
      throw std::runtime_error("sim_set_push: the disturbance schedule is on (mpc_sim_disturbances): its events are the pushes of this handle; turn it off "
                               "with mpc_sim_disturbances(sim, NULL, 0) before arming a push");
    if (width != 3 && width != 6) throw std::runtime_error("sim_set_push: width must be 3 (force at the base origin) or 6 (force, world point)");
    const Layout& L = s->L;
    if (!s->plant.d_push) s->plant.d_push = s->alloc<double>((size_t)L.B * 6);
    // (a small synchronous upload: the push changes a few times per run, not part of the steady loop)
    copy_sync(s, s->plant.d_push, f_ext, (size_t)L.B * width * sizeof(double), hipMemcpyHostToDevice);
    s->plant.push_width = width;
  })
}

int mpc_sim_record(mpc_solver* s, int32_t cap) {
  MPC_TRY(s, {
    if (cap < 0) throw std::runtime_error("sim_record: cap must be >= 0 (0: recording off)");
    sim_check(s, "sim_record");
    const Layout& L = s->L;
    if (cap > 0) sim_model_check(s, "sim_record");
    s->plant.rec_cap = s->plant.rec_count = 0;
    sim_realloc(s, s->plant.d_rec, (size_t)cap * L.B * sim_record_width(L.nx, L.m));
    s->plant.rec_cap = cap;
    if (cap > 0) sim_ensure(s);
  })
}

int mpc_sim_record_read(mpc_solver* s, double* out, int32_t* count) {
  MPC_TRY(s, {
    if (!count) throw std::runtime_error("sim_record_read: count must not be null");
    sim_check(s, "sim_record_read");
    HIP_OK(hipStreamSynchronize(s->stream));
    *count = s->plant.rec_count;
    if (out) {
      const Layout& L = s->L;
      if (s->plant.rec_count > 0) copy_sync(s, out, s->plant.d_rec, (size_t)s->plant.rec_count * L.B * sim_record_width(L.nx, L.m) * sizeof(double), hipMemcpyDeviceToHost);
      s->plant.rec_count = 0;
    }
  })
}

int32_t mpc_sim_record_width(mpc_solver* s) { return sim_width(s, "sim_record_width", [&] { return sim_record_width(s->L.nx, s->L.m); }); }

// ---- include/mpc_sim_metrics.h ---------------------------------------------------------------------------------------------------------------
int mpc_sim_metrics(mpc_solver* s, const mpc_sim_metrics_config* cfg) {
  MPC_TRY(s, {
    sim_check(s, "sim_metrics");
    const Layout& L = s->L;
    if (cfg) {
      sim_model_check(s, "sim_metrics");
      for (double v : {cfg->min_force, cfg->half_length, cfg->half_width, cfg->fall_drop, cfg->sole_lift})
        if (!std::isfinite(v) || v < 0.0) throw std::runtime_error("sim_metrics: every field of the configuration must be finite and >= 0");
    }
    sim_realloc(s, s->plant.d_met, cfg ? (size_t)L.B * (MPC_SIM_METRICS_WIDTH + 1 + L.nx) : 0);
    if (cfg) {
      s->plant.met_cfg = *cfg;
      sim_ensure(s);
      sim_metrics_reset(s);
    }
  })
}

int mpc_sim_metrics_read(mpc_solver* s, double* out, int32_t reset) {
  MPC_TRY(s, {
    if (!out) throw std::runtime_error("sim_metrics_read: out must not be null");
    sim_check(s, "sim_metrics_read");
    if (!s->plant.d_met) throw std::runtime_error("sim_metrics_read: metrics are off on this handle (turn them on with mpc_sim_metrics)");
    HIP_OK(hipStreamSynchronize(s->stream));
    copy_sync(s, out, s->plant.d_met, (size_t)s->L.B * MPC_SIM_METRICS_WIDTH * sizeof(double), hipMemcpyDeviceToHost);
    if (reset) sim_metrics_reset(s);
  })
}

int32_t mpc_sim_metrics_width(mpc_solver* s) { return sim_width(s, "sim_metrics_width", [&] { return MPC_SIM_METRICS_WIDTH; }); }

// ---- include/mpc_sim_contacts.h, include/mpc_sim_terrain.h: the contact rule and the terrain under it -----------------------------------------
static void sim_terrain_drop(mpc_solver* s) {
  sim_realloc(s, s->plant.d_ter, 0);
  s->plant.ter_cfg = {};
  s->plant.h_ter.clear();
}

int mpc_sim_contacts(mpc_solver* s, const mpc_sim_contacts_config* cfg) {
  MPC_TRY(s, {
    sim_check(s, "sim_contacts");
    const Layout& L = s->L;
    if (cfg) {
      sim_model_check(s, "sim_contacts");
      if (!std::isfinite(cfg->ground_z) || !std::isfinite(cfg->ground_tol) || !std::isfinite(cfg->release_force))
        throw std::runtime_error("sim_contacts: ground_z, ground_tol and release_force must be finite");
      if (cfg->ground_tol < 0.0 || cfg->release_force < 0.0) throw std::runtime_error("sim_contacts: ground_tol and release_force must be >= 0");
      if (cfg->release_steps < 1) throw std::runtime_error("sim_contacts: release_steps must be >= 1");
    }
    sim_realloc(s, s->plant.d_con, cfg ? (size_t)L.B * MPC_SIM_CONTACTS_WIDTH : 0);
    if (!cfg) {  // (the terrain, the friction model, the estimator and the contact detector go with the rows; a reset keeps them)
      sim_terrain_drop(s);
      sim_friction_drop(s);
      sim_estimator_drop(s);
      sim_foot_sensors_drop(s);
      if (s->plant.dis_contact) sim_disturbances_drop(s);  // (a table with a contact trigger reads the rows)
    }
    if (cfg) {
      s->plant.con_cfg = *cfg;
      s->plant.con_cfg.reserved = 0;
      sim_ensure(s);
      sim_contacts_reset(s);
      sim_foot_sensors_arm(s, nullptr);  // (the contact detector starts again from the rows just reset)
    }
  })
}

int mpc_sim_contacts_set(mpc_solver* s, const double* rows) {
  MPC_TRY(s, {
    if (!rows) throw std::runtime_error("sim_contacts_set: rows must not be null");
    sim_check(s, "sim_contacts_set");
    if (!s->plant.d_con) throw std::runtime_error("sim_contacts_set: the contact rule is off on this handle (turn it on with mpc_sim_contacts)");
    const Layout& L = s->L;
    for (int b = 0; b < L.B; ++b) {
      const double* r = rows + (size_t)b * MPC_SIM_CONTACTS_WIDTH;
      const std::string row = "sim_contacts_set: row " + std::to_string(b);
      for (int e = 0; e < MPC_SIM_CONTACTS_WIDTH; ++e)
        if (!std::isfinite(r[e])) throw std::runtime_error(row + " holds a non-finite entry (" + std::to_string(e) + ")");
      for (int e = 0; e < 4; ++e)
        if (r[e] != 0.0 && r[e] != 1.0) throw std::runtime_error(row + ": in_contact and lifted must be 0 or 1");
      if (r[0] == 0.0 && r[1] == 0.0) throw std::runtime_error(row + " has no sole in contact (flight phases are not simulated)");
      for (int e : {4, 5, 32, 33, 34, 35, 40})
        if (r[e] < 0.0) throw std::runtime_error(row + ": pulling, the counts and steps must be >= 0");
      for (int i = 0; i < 2; ++i) {
        const double* R = r + 8 + 12 * i;
        double dev = 0.0;
        for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) {
          double d = (a == c) ? -1.0 : 0.0;
          for (int k = 0; k < 3; ++k) d += R[3 * k + a] * R[3 * k + c];
          dev = std::fmax(dev, std::fabs(d));
        }
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (dev > 1e-9 || det < 0.0) throw std::runtime_error(row + ": the anchor of sole " + std::to_string(i) + " is not a rotation");
      }
    }
    HIP_OK(hipStreamSynchronize(s->stream));
    copy_sync(s, s->plant.d_con, rows, (size_t)L.B * MPC_SIM_CONTACTS_WIDTH * sizeof(double), hipMemcpyHostToDevice);
    sim_foot_sensors_arm(s, rows);  // (... and from rows imposed)
  })
}

int mpc_sim_contacts_read(mpc_solver* s, double* rows) {
  MPC_TRY(s, {
    if (!rows) throw std::runtime_error("sim_contacts_read: rows must not be null");
    sim_check(s, "sim_contacts_read");
    if (!s->plant.d_con) throw std::runtime_error("sim_contacts_read: the contact rule is off on this handle (turn it on with mpc_sim_contacts)");
    HIP_OK(hipStreamSynchronize(s->stream));
    copy_sync(s, rows, s->plant.d_con, (size_t)s->L.B * MPC_SIM_CONTACTS_WIDTH * sizeof(double), hipMemcpyDeviceToHost);
  })
}

int mpc_sim_terrain(mpc_solver* s, const mpc_sim_terrain_config* cfg, const double* boxes) {
  MPC_TRY(s, {
    sim_check(s, "sim_terrain");
    if (!s->plant.d_con) throw std::runtime_error("sim_terrain: the contact rule is off on this handle (turn it on with mpc_sim_contacts first)");
    const Layout& L = s->L;
    size_t count = 0;
    if (cfg) {
      if (cfg->n_boxes < 0 || cfg->n_boxes > MPC_SIM_TERRAIN_MAX_BOXES)
        throw std::runtime_error("sim_terrain: n_boxes must be 0 .. " + std::to_string(MPC_SIM_TERRAIN_MAX_BOXES));
      if (cfg->per_robot != 0 && cfg->per_robot != 1) throw std::runtime_error("sim_terrain: per_robot must be 0 or 1");
      if (cfg->n_boxes > 0 && !boxes) throw std::runtime_error("sim_terrain: boxes must not be null with n_boxes > 0");
      count = (size_t)(cfg->per_robot ? L.B : 1) * cfg->n_boxes;
      for (size_t k = 0; k < count; ++k) {
        const double* bx = boxes + k * MPC_SIM_TERRAIN_BOX_WIDTH;
        for (int e = 0; e < MPC_SIM_TERRAIN_BOX_WIDTH; ++e)
          if (!std::isfinite(bx[e])) throw std::runtime_error("sim_terrain: box " + std::to_string(k) + " holds a non-finite number");
        if (bx[0] > bx[1] || bx[2] > bx[3]) throw std::runtime_error("sim_terrain: box " + std::to_string(k) + " has x_lo > x_hi or y_lo > y_hi");
      }
    }
    sim_terrain_drop(s);
    if (cfg) {
      s->plant.ter_cfg = *cfg;
      s->plant.h_ter.assign(boxes, boxes + count * MPC_SIM_TERRAIN_BOX_WIDTH);
      if (count > 0) {  // (zero boxes: the plane, by the old path)
        std::vector<double> h(s->plant.h_ter);
        for (size_t k = 0; k < count; ++k) h[k * MPC_SIM_TERRAIN_BOX_WIDTH + 4] += 0.0;  // (a top of -0 counts as +0, as in the numpy definition)
        sim_realloc(s, s->plant.d_ter, h.size());
        copy_sync(s, s->plant.d_ter, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
      }
    }
  })
}

int mpc_sim_terrain_read(mpc_solver* s, mpc_sim_terrain_config* cfg, double* boxes) {
  MPC_TRY(s, {
    if (!cfg) throw std::runtime_error("sim_terrain_read: cfg must not be null");
    sim_check(s, "sim_terrain_read");
    if (!s->plant.d_con) throw std::runtime_error("sim_terrain_read: the contact rule is off on this handle (turn it on with mpc_sim_contacts first)");
    *cfg = s->plant.ter_cfg;
    if (boxes) std::copy(s->plant.h_ter.begin(), s->plant.h_ter.end(), boxes);
  })
}

int mpc_sim_terrain_height(mpc_solver* s, const double* xy, int32_t n, double* h) {
  MPC_TRY(s, {
    sim_check(s, "sim_terrain_height");
    if (!s->plant.d_con) throw std::runtime_error("sim_terrain_height: the contact rule is off on this handle (turn it on with mpc_sim_contacts first)");
    if (n < 0) throw std::runtime_error("sim_terrain_height: n must be >= 0");
    if (n > 0 && (!xy || !h)) throw std::runtime_error("sim_terrain_height: xy and h must not be null");
    const Layout& L = s->L;
    const size_t np = (size_t)L.B * n;
    for (size_t i = 0; i < 2 * np; ++i)
      if (!std::isfinite(xy[i])) throw std::runtime_error("sim_terrain_height: xy holds a non-finite number");
    if (n > 0) {
      void* p = nullptr;
      HIP_OK(hipMalloc(&p, 3 * np * sizeof(double)));
      double* d_xy = (double*)p;
      try {
        copy_sync(s, d_xy, xy, 2 * np * sizeof(double), hipMemcpyHostToDevice);
        SimTerrainHeightArgs a;
        a.t = sim_terrain_args(s); a.ground_z = s->plant.con_cfg.ground_z; a.xy = d_xy; a.n = n; a.h = d_xy + 2 * np;
        hipLaunchKernelGGL(k_sim_terrain_height, dim3((unsigned)L.B), dim3(64), 0, s->stream, a);
        HIP_OK(hipGetLastError());
        copy_sync(s, h, a.h, np * sizeof(double), hipMemcpyDeviceToHost);
      } catch (...) {
        (void)hipFree(p);
        throw;
      }
      HIP_OK(hipFree(p));
    }
  })
}

int32_t mpc_sim_contacts_width(mpc_solver* s) { return sim_width(s, "sim_contacts_width", [&] { return MPC_SIM_CONTACTS_WIDTH; }); }

// ---- include/mpc_sim_actuators.h: the per-robot actuator model of the torque-driven simulator steps ------------------------------------------
int mpc_sim_actuators(mpc_solver* s, const double* params, const double* limit, const double* friction_shape) {
  MPC_TRY(s, {
    sim_check(s, "sim_actuators");
    const Layout& L = s->L;
    const size_t nu = L.m, np = (size_t)L.B * MPC_SIM_ACTUATORS_PARAMS;
    std::vector<double> h;
    if (params) {  // (every check before anything changes: a bad row leaves the previous configuration in force)
      h.assign(np + 2 * nu, 0.0);
      bool any_sat = false;
      for (int b = 0; b < L.B; ++b) {
        const double* r = params + (size_t)b * MPC_SIM_ACTUATORS_PARAMS;
        const std::string row = "sim_actuators: row " + std::to_string(b);
        for (int e = 0; e < MPC_SIM_ACTUATORS_PARAMS; ++e)
          if (!std::isfinite(r[e])) throw std::runtime_error(row + " holds a non-finite entry (" + std::to_string(e) + ")");
        if (r[0] != std::floor(r[0]) || r[0] < 0.0 || r[0] > MPC_SIM_ACTUATORS_RING - 1)
          throw std::runtime_error(row + ": delay must be an integer value in [0, " + std::to_string(MPC_SIM_ACTUATORS_RING - 1) + "]");
        if (!(r[1] > 0.0)) throw std::runtime_error(row + ": scale must be > 0");
        for (int e = 2; e < 7; ++e)
          if (r[e] < 0.0) throw std::runtime_error(row + ": time_constant, damping, coulomb, v_eps and sat must be >= 0");
        if (r[4] > 0.0 && !(r[5] > 0.0)) throw std::runtime_error(row + ": coulomb > 0 needs v_eps > 0");
        if (r[6] > 0.0) any_sat = true;
        std::copy(r, r + MPC_SIM_ACTUATORS_PARAMS, h.begin() + (size_t)b * MPC_SIM_ACTUATORS_PARAMS);
        h[(size_t)b * MPC_SIM_ACTUATORS_PARAMS + 7] = 0.0;
      }
      if (any_sat && !limit) throw std::runtime_error("sim_actuators: a row with sat > 0 needs the effort limits (limit must not be null)");
      for (size_t j = 0; j < nu; ++j) {
        const double l = limit ? limit[j] : 0.0, f = friction_shape ? friction_shape[j] : 1.0;
        if (!std::isfinite(l) || l < 0.0 || !std::isfinite(f) || f < 0.0)
          throw std::runtime_error("sim_actuators: limit and friction_shape must be finite and >= 0");
        h[np + j] = l;
        h[np + nu + j] = f;
      }
    }
    const size_t rows = (size_t)L.B * sim_actuators_width(L);
    sim_realloc(s, s->plant.d_act, params ? h.size() + rows : 0);
    s->plant.h_act = h;
    if (params) {
      h.resize(h.size() + rows, 0.0);  // (the state rows after a reset: all 0)
      copy_sync(s, s->plant.d_act, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
    }
  })
}

int mpc_sim_actuators_read(mpc_solver* s, double* params, double* state) {
  MPC_TRY(s, {
    sim_check(s, "sim_actuators_read");
    if (!s->plant.d_act) throw std::runtime_error("sim_actuators_read: the actuator model is off on this handle (turn it on with mpc_sim_actuators)");
    const Layout& L = s->L;
    if (params) std::copy(s->plant.h_act.begin(), s->plant.h_act.begin() + (size_t)L.B * MPC_SIM_ACTUATORS_PARAMS, params);
    HIP_OK(hipStreamSynchronize(s->stream));
    if (state) copy_sync(s, state, sim_actuators_rows(s), (size_t)L.B * sim_actuators_width(L) * sizeof(double), hipMemcpyDeviceToHost);
  })
}

int mpc_sim_actuators_set(mpc_solver* s, const double* state) {
  MPC_TRY(s, {
    if (!state) throw std::runtime_error("sim_actuators_set: state must not be null");
    sim_check(s, "sim_actuators_set");
    if (!s->plant.d_act) throw std::runtime_error("sim_actuators_set: the actuator model is off on this handle (turn it on with mpc_sim_actuators)");
    const Layout& L = s->L;
    const size_t W = sim_actuators_width(L);
    for (int b = 0; b < L.B; ++b) {
      const double* r = state + (size_t)b * W;
      const std::string row = "sim_actuators_set: row " + std::to_string(b);
      for (size_t e = 0; e < W; ++e)
        if (!std::isfinite(r[e])) throw std::runtime_error(row + " holds a non-finite entry (" + std::to_string(e) + ")");
      const double head = r[W - 2], count = r[W - 1];
      if (head != std::floor(head) || head < 0.0 || head >= MPC_SIM_ACTUATORS_RING)
        throw std::runtime_error(row + ": head must be an integer value in [0, " + std::to_string(MPC_SIM_ACTUATORS_RING) + ")");
      if (count < 0.0) throw std::runtime_error(row + ": count must be >= 0");
    }
    HIP_OK(hipStreamSynchronize(s->stream));
    copy_sync(s, sim_actuators_rows(s), state, (size_t)L.B * W * sizeof(double), hipMemcpyHostToDevice);
  })
}

int32_t mpc_sim_actuators_width(mpc_solver* s) { return sim_width(s, "sim_actuators_width", [&] { return sim_actuators_width(s->L); }); }

// ---- include/mpc_sim_sensors.h: the per-robot sensor model between the simulator steps and the controllers -----------------------------------
int mpc_sim_sensors(mpc_solver* s, const double* params, const double* x0) {
  MPC_TRY(s, {
    sim_check(s, "sim_sensors");
    const Layout& L = s->L;
    const size_t np = (size_t)L.B * MPC_SIM_SENSORS_PARAMS, nxs = (size_t)L.B * L.nx;
    if (params) {  // (every check before anything changes: a bad row leaves the previous configuration in force)
      for (int b = 0; b < L.B; ++b) {
        const double* r = params + (size_t)b * MPC_SIM_SENSORS_PARAMS;
        const std::string row = "sim_sensors: row " + std::to_string(b);
        for (int e = 0; e < MPC_SIM_SENSORS_PARAMS; ++e)
          if (!std::isfinite(r[e])) throw std::runtime_error(row + " holds a non-finite entry (" + std::to_string(e) + ")");
        if (r[0] != std::floor(r[0]) || r[0] < 0.0 || r[0] > MPC_SIM_SENSORS_RING - 1)
          throw std::runtime_error(row + ": delay must be an integer value in [0, " + std::to_string(MPC_SIM_SENSORS_RING - 1) + "]");
        for (int e : {1, 2, 3, 4, 5, 6, 7, 8, 10})
          if (r[e] < 0.0) throw std::runtime_error(row + ": the noise levels (sigma_*), quantum, q_bias and v_time_constant must be >= 0");
        if (r[9] != 0.0 && r[9] != 1.0) throw std::runtime_error(row + ": v_from_q must be 0 or 1");
        if (r[11] != std::floor(r[11]) || r[11] < 0.0 || r[11] >= 4294967296.0) throw std::runtime_error(row + ": seed must be an integer value in [0, 2^32)");
        for (int e = 12; e < MPC_SIM_SENSORS_PARAMS; ++e)
          if (r[e] != 0.0) throw std::runtime_error(row + ": the reserved entries must be 0");
      }
      if (!x0) throw std::runtime_error("sim_sensors: x0 must not be null (the first measurement is taken of it)");
      for (size_t e = 0; e < nxs; ++e)
        if (!std::isfinite(x0[e])) throw std::runtime_error("sim_sensors: x0 holds a non-finite entry");
    }
    sim_realloc(s, s->plant.d_sen, params ? np + 2 * nxs + (size_t)L.B * sim_sensors_width(L) : 0);
    s->plant.h_sen.clear();
    if (params) {
      s->plant.h_sen.assign(params, params + np);
      // the rows after a reset: all 0, then the arming event (count 1) on x0
      HIP_OK(hipMemsetAsync(s->plant.d_sen, 0, (np + 2 * nxs + (size_t)L.B * sim_sensors_width(L)) * sizeof(double), s->stream));
      copy_sync(s, s->plant.d_sen, params, np * sizeof(double), hipMemcpyHostToDevice);
      copy_sync(s, sim_sensors_stage(s), x0, nxs * sizeof(double), hipMemcpyHostToDevice);
      sim_sensors_enqueue(s, s->stream, sim_sensors_stage(s), 0.0);
      HIP_OK(hipStreamSynchronize(s->stream));
    }
  })
}

int mpc_sim_sensors_read(mpc_solver* s, double* params, double* state, double* x_meas) {
  MPC_TRY(s, {
    sim_check(s, "sim_sensors_read");
    if (!s->plant.d_sen) throw std::runtime_error("sim_sensors_read: the sensor model is off on this handle (turn it on with mpc_sim_sensors)");
    const Layout& L = s->L;
    if (params) std::copy(s->plant.h_sen.begin(), s->plant.h_sen.end(), params);
    HIP_OK(hipStreamSynchronize(s->stream));
    if (state) copy_sync(s, state, sim_sensors_rows(s), (size_t)L.B * sim_sensors_width(L) * sizeof(double), hipMemcpyDeviceToHost);
    if (x_meas) copy_sync(s, x_meas, sim_sensors_meas(s), (size_t)L.B * L.nx * sizeof(double), hipMemcpyDeviceToHost);
  })
}

int mpc_sim_sensors_set(mpc_solver* s, const double* state) {
  MPC_TRY(s, {
    if (!state) throw std::runtime_error("sim_sensors_set: state must not be null");
    sim_check(s, "sim_sensors_set");
    if (!s->plant.d_sen) throw std::runtime_error("sim_sensors_set: the sensor model is off on this handle (turn it on with mpc_sim_sensors)");
    const Layout& L = s->L;
    const size_t W = sim_sensors_width(L), o_meas = (size_t)MPC_SIM_SENSORS_RING * L.nx;
    std::vector<double> xm((size_t)L.B * L.nx);
    for (int b = 0; b < L.B; ++b) {
      const double* r = state + (size_t)b * W;
      const std::string row = "sim_sensors_set: row " + std::to_string(b);
      for (size_t e = 0; e < W; ++e)
        if (!std::isfinite(r[e])) throw std::runtime_error(row + " holds a non-finite entry (" + std::to_string(e) + ")");
      const double head = r[W - 2], count = r[W - 1];
      if (head != std::floor(head) || head < 0.0 || head >= MPC_SIM_SENSORS_RING)
        throw std::runtime_error(row + ": head must be an integer value in [0, " + std::to_string(MPC_SIM_SENSORS_RING) + ")");
      if (count < 1.0) throw std::runtime_error(row + ": count must be >= 1 (a measurement is always held)");
      std::copy(r + o_meas, r + o_meas + L.nx, xm.begin() + (size_t)b * L.nx);
    }
    HIP_OK(hipStreamSynchronize(s->stream));
    copy_sync(s, sim_sensors_rows(s), state, (size_t)L.B * W * sizeof(double), hipMemcpyHostToDevice);
    copy_sync(s, sim_sensors_meas(s), xm.data(), xm.size() * sizeof(double), hipMemcpyHostToDevice);  // (the controllers read the rows' measurement)
  })
}

int32_t mpc_sim_sensors_width(mpc_solver* s) { return sim_width(s, "sim_sensors_width", [&] { return sim_sensors_width(s->L); }); }

// ---- include/mpc_sim_estimator.h: the per-robot base-state estimator between the sensor model and the controllers ----------------------------
int mpc_sim_estimator(mpc_solver* s, const double* params, const double* x0) {
  MPC_TRY(s, {
    sim_check(s, "sim_estimator");
    const Layout& L = s->L;
    const size_t np = (size_t)L.B * MPC_SIM_ESTIMATOR_PARAMS, nxs = (size_t)L.B * L.nx;
    if (params) {  // (every check before anything changes: a bad call leaves the previous configuration in force)
      sim_model_check(s, "sim_estimator");
      if (L.nx > SIM_EST_MAX_NX) throw std::runtime_error("sim_estimator: a longer state than the estimator's kernel holds (" + std::to_string(SIM_EST_MAX_NX) + ")");
      for (int b = 0; b < L.B; ++b) {
        const double* r = params + (size_t)b * MPC_SIM_ESTIMATOR_PARAMS;
        const std::string row = "sim_estimator: row " + std::to_string(b);
        for (int e = 0; e < MPC_SIM_ESTIMATOR_PARAMS; ++e)
          if (!std::isfinite(r[e])) throw std::runtime_error(row + " holds a non-finite entry (" + std::to_string(e) + ")");
        for (int e = 0; e < 2; ++e)
          if (r[e] < 0.0 || r[e] > 1.0) throw std::runtime_error(row + ": the weights w_p and w_v must be in [0, 1]");
        for (int e = 2; e < MPC_SIM_ESTIMATOR_PARAMS; ++e)
          if (r[e] != 0.0) throw std::runtime_error(row + ": the reserved entries must be 0");
      }
      if (!x0) throw std::runtime_error("sim_estimator: x0 must not be null (the arming event is run on it)");
      for (size_t e = 0; e < nxs; ++e)
        if (!std::isfinite(x0[e])) throw std::runtime_error("sim_estimator: x0 holds a non-finite entry");
      if (!s->plant.d_con) throw std::runtime_error("sim_estimator: the contact rule is off on this handle (turn it on with mpc_sim_contacts first)");
    }
    const size_t total = np + 2 * nxs + (size_t)L.B * sim_estimator_width(L);
    sim_realloc(s, s->plant.d_est, params ? total : 0);
    s->plant.h_est.clear();
    if (params) {
      s->plant.h_est.assign(params, params + np);
      // the rows after a reset: all 0, then the arming event (count 1) on x0
      HIP_OK(hipMemsetAsync(s->plant.d_est, 0, total * sizeof(double), s->stream));
      copy_sync(s, s->plant.d_est, params, np * sizeof(double), hipMemcpyHostToDevice);
      copy_sync(s, sim_estimator_stage(s), x0, nxs * sizeof(double), hipMemcpyHostToDevice);
      sim_estimator_enqueue(s, s->stream, sim_estimator_stage(s), sim_estimator_stage(s));
      HIP_OK(hipStreamSynchronize(s->stream));
    }
  })
}

int mpc_sim_estimator_read(mpc_solver* s, double* params, double* state, double* x_est) {
  MPC_TRY(s, {
    sim_check(s, "sim_estimator_read");
    if (!s->plant.d_est) throw std::runtime_error("sim_estimator_read: the estimator is off on this handle (turn it on with mpc_sim_estimator)");
    const Layout& L = s->L;
    if (params) std::copy(s->plant.h_est.begin(), s->plant.h_est.end(), params);
    HIP_OK(hipStreamSynchronize(s->stream));
    if (state) copy_sync(s, state, sim_estimator_rows(s), (size_t)L.B * sim_estimator_width(L) * sizeof(double), hipMemcpyDeviceToHost);
    if (x_est) copy_sync(s, x_est, sim_estimator_est(s), (size_t)L.B * L.nx * sizeof(double), hipMemcpyDeviceToHost);
  })
}

int mpc_sim_estimator_set(mpc_solver* s, const double* state) {
  MPC_TRY(s, {
    if (!state) throw std::runtime_error("sim_estimator_set: state must not be null");
    sim_check(s, "sim_estimator_set");
    if (!s->plant.d_est) throw std::runtime_error("sim_estimator_set: the estimator is off on this handle (turn it on with mpc_sim_estimator)");
    const Layout& L = s->L;
    const size_t W = sim_estimator_width(L);
    std::vector<double> xe((size_t)L.B * L.nx);
    for (int b = 0; b < L.B; ++b) {
      const double* r = state + (size_t)b * W;
      const std::string row = "sim_estimator_set: row " + std::to_string(b);
      for (size_t e = 0; e < W; ++e)
        if (!std::isfinite(r[e])) throw std::runtime_error(row + " holds a non-finite entry (" + std::to_string(e) + ")");
      for (int i = 0; i < 2; ++i)
        if (r[L.nx + i] != 0.0 && r[L.nx + i] != 1.0) throw std::runtime_error(row + ": held must be 0 or 1");
      if (r[W - 1] < 1.0) throw std::runtime_error(row + ": count must be >= 1 (an estimate is always held)");
      std::copy(r, r + L.nx, xe.begin() + (size_t)b * L.nx);
    }
    HIP_OK(hipStreamSynchronize(s->stream));
    copy_sync(s, sim_estimator_rows(s), state, (size_t)L.B * W * sizeof(double), hipMemcpyHostToDevice);
    copy_sync(s, sim_estimator_est(s), xe.data(), xe.size() * sizeof(double), hipMemcpyHostToDevice);  // (the controllers read the rows' estimate)
  })
}

int32_t mpc_sim_estimator_width(mpc_solver* s) { return sim_width(s, "sim_estimator_width", [&] { return sim_estimator_width(s->L); }); }

// ---- include/mpc_sim_foot_sensors.h: the per-robot foot force sensors and the contact detector ----------------------------------------------------
int mpc_sim_foot_sensors(mpc_solver* s, const double* params) {
  MPC_TRY(s, {
    sim_check(s, "sim_foot_sensors");
    const Layout& L = s->L;
    const size_t np = (size_t)L.B * MPC_SIM_FOOT_SENSORS_PARAMS;
    if (!params) {
      sim_foot_sensors_drop(s);
      return 0;
    }
    for (int b = 0; b < L.B; ++b) {  // (every check before anything changes: a bad row leaves the previous configuration in force)
      const double* r = params + (size_t)b * MPC_SIM_FOOT_SENSORS_PARAMS;
      const std::string row = "sim_foot_sensors: row " + std::to_string(b);
      for (int e = 0; e < MPC_SIM_FOOT_SENSORS_PARAMS; ++e)
        if (!std::isfinite(r[e])) throw std::runtime_error(row + " holds a non-finite entry (" + std::to_string(e) + ")");
      if (r[0] != std::floor(r[0]) || r[0] < 0.0 || r[0] > MPC_SIM_FOOT_SENSORS_RING - 1)
        throw std::runtime_error(row + ": delay must be an integer value in [0, " + std::to_string(MPC_SIM_FOOT_SENSORS_RING - 1) + "]");
      for (int e = 1; e < 6; ++e)
        if (r[e] < 0.0) throw std::runtime_error(row + ": sigma_f, sigma_m, bias_f, bias_m and time_constant must be >= 0");
      if (r[7] > r[6]) throw std::runtime_error(row + ": f_off must be <= f_on");
      for (int e = 8; e < 10; ++e)
        if (r[e] != std::floor(r[e]) || r[e] < 1.0) throw std::runtime_error(row + ": on_steps and off_steps must be integer values >= 1");
      if (r[10] != std::floor(r[10]) || r[10] < 0.0 || r[10] >= 4294967296.0) throw std::runtime_error(row + ": seed must be an integer value in [0, 2^32)");
      for (int e = 11; e < MPC_SIM_FOOT_SENSORS_PARAMS; ++e)
        if (r[e] != 0.0) throw std::runtime_error(row + ": the reserved entries must be 0");
    }
    if (!s->plant.d_con) throw std::runtime_error("sim_foot_sensors: the contact rule is off on this handle (turn it on with mpc_sim_contacts first)");
    sim_realloc(s, s->plant.d_fs, np + (size_t)L.B * MPC_SIM_FOOT_SENSORS_WIDTH);
    s->plant.h_fs.assign(params, params + np);
    sim_ensure(s);
    copy_sync(s, s->plant.d_fs, params, np * sizeof(double), hipMemcpyHostToDevice);
    sim_foot_sensors_arm(s, nullptr);
  })
}

int mpc_sim_foot_sensors_read(mpc_solver* s, double* params, double* state) {
  MPC_TRY(s, {
    sim_check(s, "sim_foot_sensors_read");
    if (!s->plant.d_fs) throw std::runtime_error("sim_foot_sensors_read: the foot sensors are off on this handle (turn them on with mpc_sim_foot_sensors)");
    if (params) std::copy(s->plant.h_fs.begin(), s->plant.h_fs.end(), params);
    HIP_OK(hipStreamSynchronize(s->stream));
    if (state) copy_sync(s, state, sim_foot_sensors_rows(s), (size_t)s->L.B * MPC_SIM_FOOT_SENSORS_WIDTH * sizeof(double), hipMemcpyDeviceToHost);
  })
}

int mpc_sim_foot_sensors_set(mpc_solver* s, const double* state) {
  MPC_TRY(s, {
    if (!state) throw std::runtime_error("sim_foot_sensors_set: state must not be null");
    sim_check(s, "sim_foot_sensors_set");
    if (!s->plant.d_fs) throw std::runtime_error("sim_foot_sensors_set: the foot sensors are off on this handle (turn them on with mpc_sim_foot_sensors)");
    const Layout& L = s->L;
    const size_t W = MPC_SIM_FOOT_SENSORS_WIDTH;
    for (int b = 0; b < L.B; ++b) {
      const double* r = state + (size_t)b * W;
      const std::string row = "sim_foot_sensors_set: row " + std::to_string(b);
      for (size_t e = 0; e < W; ++e)
        if (!std::isfinite(r[e])) throw std::runtime_error(row + " holds a non-finite entry (" + std::to_string(e) + ")");
      for (int i = 0; i < 2; ++i)
        if (r[i] != 0.0 && r[i] != 1.0) throw std::runtime_error(row + ": det must be 0 or 1");
      if (r[0] == 0.0 && r[1] == 0.0) throw std::runtime_error(row + " has no sole detected (the detector never reports an empty set)");
      for (int e = SIM_FS_O_ABOVE; e < SIM_FS_O_WF; ++e)
        if (r[e] < 0.0) throw std::runtime_error(row + ": the counters above and below must be >= 0");
      for (int e = SIM_FS_O_COUNTS; e < SIM_FS_O_RING; ++e)
        if (r[e] < 0.0) throw std::runtime_error(row + ": the confusion counts must be >= 0");
      const double head = r[W - 2], count = r[W - 1];
      if (head != std::floor(head) || head < 0.0 || head >= MPC_SIM_FOOT_SENSORS_RING)
        throw std::runtime_error(row + ": head must be an integer value in [0, " + std::to_string(MPC_SIM_FOOT_SENSORS_RING) + ")");
      if (count < 0.0) throw std::runtime_error(row + ": count must be >= 0");
    }
    HIP_OK(hipStreamSynchronize(s->stream));
    copy_sync(s, sim_foot_sensors_rows(s), state, (size_t)L.B * W * sizeof(double), hipMemcpyHostToDevice);
  })
}

int32_t mpc_sim_foot_sensors_width(mpc_solver* s) { return sim_width(s, "sim_foot_sensors_width", [&] { return MPC_SIM_FOOT_SENSORS_WIDTH; }); }

int mpc_sim_foot_sensors_feed(mpc_solver* s, int32_t consumers) {
  MPC_TRY(s, {
    sim_check(s, "sim_foot_sensors_feed");
    if (!s->plant.d_fs) throw std::runtime_error("sim_foot_sensors_feed: the foot sensors are off on this handle (turn them on with mpc_sim_foot_sensors)");
    if (consumers & ~(MPC_SIM_FOOT_SENSORS_FEED_ESTIMATOR | MPC_SIM_FOOT_SENSORS_FEED_QP))
      throw std::runtime_error("sim_foot_sensors_feed: unknown consumer bit in " + std::to_string(consumers) + " (1: the estimator, 2: the low-level QPs)");
    HIP_OK(hipStreamSynchronize(s->stream));
    s->plant.fs_feed = consumers;
  })
}

// ---- include/mpc_sim_plant.h: per-robot plant inertias ------------------------------------------------------------------------------------------
int mpc_sim_plant(mpc_solver* s, const double* params, const double* link_scale) {
  MPC_TRY(s, {
    sim_check(s, "sim_plant");
    const Layout& L = s->L;
    if (!params) {
      sim_realloc(s, s->plant.d_plant, 0);
      s->plant.h_plant.clear();
      s->plant.plant_nd = s->plant.plant_off = 0;
      return 0;
    }
    // (every check before anything changes: a bad row leaves the previous configuration in force)
    if (!s->have_model || !s->d_model_d || s->h_model_i.empty()) throw std::runtime_error("sim_plant: no model is set on this handle (mpc_set_model first)");
    const int nj = L.nj;
    const size_t np = (size_t)L.B * MPC_SIM_PLANT_PARAMS;
    std::vector<double> h(np + (size_t)L.B * nj, 1.0);
    for (int b = 0; b < L.B; ++b) {
      const double* r = params + (size_t)b * MPC_SIM_PLANT_PARAMS;
      const std::string row = "sim_plant: row " + std::to_string(b);
      for (int e = 0; e < MPC_SIM_PLANT_PARAMS; ++e)
        if (!std::isfinite(r[e])) throw std::runtime_error(row + " holds a non-finite entry (" + std::to_string(e) + ")");
      if (!(r[0] > 0.0) || !(r[1] > 0.0)) throw std::runtime_error(row + ": mass_scale and inertia_scale must be > 0");
      if (r[7] < 0.0) throw std::runtime_error(row + ": payload_mass must be >= 0");
      for (int e : {2, 6})
        if (r[e] != std::floor(r[e]) || r[e] < 0.0 || r[e] > nj - 1)
          throw std::runtime_error(row + ": shift_body and payload_body must be integer values in [0, " + std::to_string(nj - 1) + "] (table joint indices)");
      for (int e = 11; e < MPC_SIM_PLANT_PARAMS; ++e)
        if (r[e] != 0.0) throw std::runtime_error(row + ": the reserved entries must be 0");
      std::copy(r, r + MPC_SIM_PLANT_PARAMS, h.begin() + (size_t)b * MPC_SIM_PLANT_PARAMS);
    }
    if (link_scale)
      for (size_t e = 0; e < (size_t)L.B * nj; ++e) {
        if (!std::isfinite(link_scale[e]) || !(link_scale[e] > 0.0))
          throw std::runtime_error("sim_plant: link_scale must be finite and > 0 (robot " + std::to_string(e / nj) + ", joint " + std::to_string(e % nj) + ")");
        h[np + e] = link_scale[e];
      }
    sim_realloc(s, s->plant.d_plant, h.size() + (size_t)L.B * s->model_nd);
    s->plant.plant_nd = s->model_nd;
    s->plant.plant_off = h.size();
    s->plant.h_plant = h;
    sim_plant_build(s);
  })
}

int mpc_sim_plant_read(mpc_solver* s, double* params, double* link_scale, double* tables) {
  MPC_TRY(s, {
    sim_check(s, "sim_plant_read");
    if (!s->plant.d_plant) throw std::runtime_error("sim_plant_read: the plant model is off on this handle (turn it on with mpc_sim_plant)");
    const Layout& L = s->L;
    const size_t np = (size_t)L.B * MPC_SIM_PLANT_PARAMS;
    if (params) std::copy(s->plant.h_plant.begin(), s->plant.h_plant.begin() + np, params);
    if (link_scale) std::copy(s->plant.h_plant.begin() + np, s->plant.h_plant.end(), link_scale);
    HIP_OK(hipStreamSynchronize(s->stream));
    if (tables) copy_sync(s, tables, sim_plant_tables(s), (size_t)L.B * s->plant.plant_nd * sizeof(double), hipMemcpyDeviceToHost);
  })
}

int32_t mpc_sim_plant_width(mpc_solver* s) {
  return sim_width(s, "sim_plant_width", [&] {
    if (!s->have_model || !s->d_model_d) throw std::runtime_error("sim_plant_width: no model is set on this handle (mpc_set_model first)");
    return s->model_nd;
  });
}

// ---- include/mpc_sim_friction.h: per-robot ground friction under the soles ----------------------------------------------------------------------
int mpc_sim_friction(mpc_solver* s, const double* params) {
  MPC_TRY(s, {
    sim_check(s, "sim_friction");
    const Layout& L = s->L;
    const size_t np = (size_t)L.B * MPC_SIM_FRICTION_PARAMS;
    if (!params) {
      sim_friction_drop(s);
      return 0;
    }
    for (int b = 0; b < L.B; ++b) {  // (every check before anything changes: a bad row leaves the previous configuration in force)
      const double* r = params + (size_t)b * MPC_SIM_FRICTION_PARAMS;
      const std::string row = "sim_friction: row " + std::to_string(b);
      for (int e = 0; e < 4; ++e)
        if (std::isnan(r[e]) || r[e] < 0.0) throw std::runtime_error(row + ": mu and mu_spin must be >= 0 (+inf: the sole never slides), entry " + std::to_string(e));
      for (int e = 4; e < MPC_SIM_FRICTION_PARAMS; ++e)
        if (!std::isfinite(r[e]) || !(r[e] > 0.0)) throw std::runtime_error(row + ": m_slip, I_slip, v_max and w_max must be finite and > 0, entry " + std::to_string(e));
    }
    if (!s->plant.d_con) throw std::runtime_error("sim_friction: the contact rule is off on this handle (turn it on with mpc_sim_contacts first)");
    sim_realloc(s, s->plant.d_fr, np + (size_t)L.B * MPC_SIM_FRICTION_WIDTH);
    s->plant.h_fr.assign(params, params + np);
    sim_ensure(s);
    std::vector<double> h(s->plant.h_fr);
    h.resize(np + (size_t)L.B * MPC_SIM_FRICTION_WIDTH, 0.0);  // (the state rows after a reset: all 0)
    copy_sync(s, s->plant.d_fr, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
  })
}

int mpc_sim_friction_read(mpc_solver* s, double* params, double* state) {
  MPC_TRY(s, {
    sim_check(s, "sim_friction_read");
    if (!s->plant.d_fr) throw std::runtime_error("sim_friction_read: the friction model is off on this handle (turn it on with mpc_sim_friction)");
    if (params) std::copy(s->plant.h_fr.begin(), s->plant.h_fr.end(), params);
    HIP_OK(hipStreamSynchronize(s->stream));
    if (state) copy_sync(s, state, sim_friction_rows(s), (size_t)s->L.B * MPC_SIM_FRICTION_WIDTH * sizeof(double), hipMemcpyDeviceToHost);
  })
}

int mpc_sim_friction_set(mpc_solver* s, const double* state) {
  MPC_TRY(s, {
    if (!state) throw std::runtime_error("sim_friction_set: state must not be null");
    sim_check(s, "sim_friction_set");
    if (!s->plant.d_fr) throw std::runtime_error("sim_friction_set: the friction model is off on this handle (turn it on with mpc_sim_friction)");
    const Layout& L = s->L;
    const size_t W = MPC_SIM_FRICTION_WIDTH;
    for (int b = 0; b < L.B; ++b) {
      const double* r = state + (size_t)b * W;
      const std::string row = "sim_friction_set: row " + std::to_string(b);
      for (size_t e = 0; e < W; ++e)
        if (!std::isfinite(r[e])) throw std::runtime_error(row + " holds a non-finite entry (" + std::to_string(e) + ")");
      for (int i = 0; i < 2; ++i) {
        const double fl = r[SIM_FR_O_SLIDING + i];
        if (fl != 0.0 && fl != 1.0) throw std::runtime_error(row + ": sliding must be 0 or 1");
        if (fl == 0.0 && (r[3 * i] != 0.0 || r[3 * i + 1] != 0.0 || r[3 * i + 2] != 0.0))
          throw std::runtime_error(row + ": sole " + std::to_string(i) + " holds a velocity but its sliding flag is 0");
      }
      for (size_t e = SIM_FR_O_STEPS; e < W; ++e)
        if (r[e] < 0.0) throw std::runtime_error(row + ": slip_steps, slip_dist, slip_yaw, peak_excess and steps must be >= 0");
    }
    HIP_OK(hipStreamSynchronize(s->stream));
    copy_sync(s, sim_friction_rows(s), state, (size_t)L.B * W * sizeof(double), hipMemcpyHostToDevice);
  })
}

int32_t mpc_sim_friction_width(mpc_solver* s) { return sim_width(s, "sim_friction_width", [&] { return MPC_SIM_FRICTION_WIDTH; }); }

// ---- include/mpc_sim_disturbances.h: per-robot push schedules on any link ----------------------------------------------------------------------
int mpc_sim_disturbances(mpc_solver* s, const double* events, int32_t n_events) {
  MPC_TRY(s, {
    sim_check(s, "sim_disturbances");
    const Layout& L = s->L;
    if (!events) {
      sim_disturbances_drop(s);
      return 0;
    }
    // (every check before anything changes: a bad event leaves the previous configuration in force)
    if (n_events < 1 || n_events > MPC_SIM_DISTURBANCES_MAX_EVENTS)
      throw std::runtime_error("sim_disturbances: n_events must be 1 .. " + std::to_string(MPC_SIM_DISTURBANCES_MAX_EVENTS));
    if (!s->have_model || s->h_model_i.empty()) throw std::runtime_error("sim_disturbances: no model is set on this handle (mpc_set_model first)");
    if (L.nj > CG_MAX_NJ) throw std::runtime_error("sim_disturbances: more moving joints than the simulator's kernels hold (" + std::to_string(CG_MAX_NJ) + ")");
    static const char* const field[MPC_SIM_DISTURBANCES_EVENT] = {"trigger", "start", "delay", "steps", "period", "shape", "link", "force_frame", "point_frame",
                                                                  "force[0]", "force[1]", "force[2]", "point[0]", "point[1]", "point[2]", "reserved"};
    bool contact = false;
    for (int b = 0; b < L.B; ++b)
      for (int e = 0; e < n_events; ++e) {
        const double* v = events + ((size_t)b * n_events + e) * MPC_SIM_DISTURBANCES_EVENT;
        const std::string ev = "sim_disturbances: robot " + std::to_string(b) + ", event " + std::to_string(e) + ": ";
        for (int i = 0; i < MPC_SIM_DISTURBANCES_EVENT; ++i)
          if (!std::isfinite(v[i])) throw std::runtime_error(ev + field[i] + " is not finite");
        for (int i : {0, 1, 2, 3, 4, 5, 6, 7, 8})
          if (v[i] != std::floor(v[i])) throw std::runtime_error(ev + field[i] + " must be an integer value");
        if (v[0] < 0.0 || v[0] > 5.0) throw std::runtime_error(ev + "trigger must be 0 .. 5");
        if (v[15] != 0.0) throw std::runtime_error(ev + "reserved must be 0");
        if (v[0] == 0.0) continue;  // (an empty slot: the other fields are not read)
        if (v[0] == 1.0 && v[1] < 0.0) throw std::runtime_error(ev + "start must be >= 0 (a step of the clock)");
        if (v[0] >= 2.0 && v[1] < 1.0) throw std::runtime_error(ev + "start must be >= 1 (an occurrence of the transition)");
        if (v[2] < 0.0) throw std::runtime_error(ev + "delay must be >= 0");
        if (v[3] < 1.0) throw std::runtime_error(ev + "steps must be >= 1");
        if (v[4] < 0.0 || (v[0] == 1.0 && v[4] > 0.0 && v[4] < v[3])) throw std::runtime_error(ev + "period must be 0 (once) or, on an absolute trigger, >= steps");
        for (int i : {5, 7, 8})
          if (v[i] != 0.0 && v[i] != 1.0) throw std::runtime_error(ev + field[i] + " must be 0 or 1");
        if (v[6] < 0.0 || v[6] > L.nj - 1) throw std::runtime_error(ev + "link must be in [0, " + std::to_string(L.nj - 1) + "] (table joint indices)");
        if (v[0] >= 2.0) contact = true;
      }
    if (contact && !s->plant.d_con)
      throw std::runtime_error("sim_disturbances: a contact trigger (2 to 5) needs the contact rule, which is off on this handle (turn it on with mpc_sim_contacts first)");
    if (s->plant.push_width)
      throw std::runtime_error("sim_disturbances: a push is armed on this handle (mpc_sim_set_push): disarm it with mpc_sim_set_push(sim, NULL, 0) before arming a schedule");
    const size_t head = (size_t)L.B * n_events * MPC_SIM_DISTURBANCES_EVENT;
    sim_ensure(s);
    {  // (the new buffer before the old one goes: an allocation that fails leaves the table in force as it was)
      void* fresh = nullptr;
      HIP_OK(hipMalloc(&fresh, sim_disturbances_doubles(L, n_events) * sizeof(double)));
      HIP_OK(hipStreamSynchronize(s->stream));
      if (s->plant.d_dis) (void)hipFree(s->plant.d_dis);
      s->plant.d_dis = (double*)fresh;
    }
    s->plant.h_dis.assign(events, events + head);
    s->plant.dis_ne = n_events;
    s->plant.dis_contact = contact;
    copy_sync(s, s->plant.d_dis, events, head * sizeof(double), hipMemcpyHostToDevice);
    sim_disturbances_reset(s);
  })
}

int mpc_sim_disturbances_read(mpc_solver* s, double* events, double* state, double* applied) {
  MPC_TRY(s, {
    sim_check(s, "sim_disturbances_read");
    if (!s->plant.d_dis) throw std::runtime_error("sim_disturbances_read: the disturbance schedule is off on this handle (turn it on with mpc_sim_disturbances)");
    const Layout& L = s->L;
    if (events) std::copy(s->plant.h_dis.begin(), s->plant.h_dis.end(), events);
    HIP_OK(hipStreamSynchronize(s->stream));
    if (state) copy_sync(s, state, sim_disturbances_rows(s), (size_t)L.B * MPC_SIM_DISTURBANCES_WIDTH * sizeof(double), hipMemcpyDeviceToHost);
    if (applied) {
      std::vector<double> h((size_t)L.B * 6 + ((size_t)L.B + 1) / 2);
      copy_sync(s, h.data(), sim_disturbances_out(s), h.size() * sizeof(double), hipMemcpyDeviceToHost);
      const int32_t* link = (const int32_t*)(h.data() + (size_t)L.B * 6);
      for (int b = 0; b < L.B; ++b) {
        std::copy(h.begin() + (size_t)b * 6, h.begin() + (size_t)b * 6 + 6, applied + (size_t)b * 7);
        applied[(size_t)b * 7 + 6] = (double)link[b];
      }
    }
  })
}

int mpc_sim_disturbances_reset(mpc_solver* s) {
  MPC_TRY(s, {
    sim_check(s, "sim_disturbances_reset");
    if (!s->plant.d_dis) throw std::runtime_error("sim_disturbances_reset: the disturbance schedule is off on this handle (turn it on with mpc_sim_disturbances)");
    sim_disturbances_reset(s);
  })
}

int32_t mpc_sim_disturbances_width(mpc_solver* s) { return sim_width(s, "sim_disturbances_width", [&] { return MPC_SIM_DISTURBANCES_WIDTH; }); }

int32_t mpc_sim_disturbances_events(mpc_solver* s) { return sim_width(s, "sim_disturbances_events", [&] { return s->plant.dis_ne; }); }

// ---- include/mpc_abi.h: one step under the caller's torques -------------------------------------------------------------------------------------
int mpc_simulate_torque(mpc_solver* s, const double* x, const double* tau, int32_t substeps, double dt, double* wrenches) {
  MPC_TRY(s, {
    if (substeps <= 0 || !(dt > 0.0)) throw std::runtime_error("simulate_torque: substeps and dt must be positive");
    if (!tau) throw std::runtime_error("simulate_torque: tau must not be null");
    const Layout& L = s->L;
    sim_steps_check(s, "simulate_torque", SIM_STAGE0, 1);
    // (synchronous uploads: the caller's arrays are free when the call returns)
    if (x) copy_sync(s, s->d_x0, x, (size_t)L.B * L.nx * sizeof(double), hipMemcpyHostToDevice);
    copy_sync(s, s->plant.d_simu, tau, (size_t)L.B * L.m * sizeof(double), hipMemcpyHostToDevice);
    sim_steps_begin(s, s->stream, nullptr);
    sim_step_enqueue(s, s->stream, s->args(), substeps, dt, wrenches != nullptr);
    if (wrenches) copy_sync(s, wrenches, s->plant.d_simwr, (size_t)L.B * 12 * sizeof(double), hipMemcpyDeviceToHost);
    s->perfect_feedback = false;
  })
}

}  // extern "C"
