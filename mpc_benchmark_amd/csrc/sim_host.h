// sim_host.h — host side of the torque-driven simulator (the plant): mpc_simulate_torque and the entry points of include/mpc_sim_*.h.  Its state is
// mpc_solver::plant (SimPlant: one SimModel owner per model); its kernels are in the sim_*.h of the same names.  Every caller that steps the plant —
// mpc_simulate_torque here, the device loops of the three pipelines in pipeline_loops.h — goes through sim_steps_check, sim_steps_begin and
// sim_step_enqueue: an extension of the simulator is added there, once, with one layout function and its row checks from the helpers below.
// Included at the end of mpc_hip.hip (mpc_solver, MPC_TRY, copy_sync, slot_of).
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
// a model goes off: its allocation, its mirror and what the plant keeps beside the owner
static void sim_drop(mpc_solver* s, SimModel& m) {
  SimPlant& p = s->plant;
  sim_realloc(s, m.d, 0);
  m.h.clear();
  if (&m == &p.ter) p.ter_cfg = {};
  if (&m == &p.fs) p.fs_feed = 0;
  if (&m == &p.pm) p.plant_nd = p.plant_off = 0;
  if (&m == &p.dis) { p.dis_ne = 0; p.dis_contact = false; }
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

// ---- refusals: every wording is built here, once ---------------------------------------------------------------------------------------------------
static void sim_on_check(const SimModel& m, const char* who) {
  if (!m.on()) throw std::runtime_error(std::string(who) + ": " + m.off);
}
// the contact rule is on: for what reads its rows (`first`: an arming call, which names the order of the two)
static void sim_rule_check(const mpc_solver* s, const char* who, bool first = true) {
  if (!s->plant.d_con)
    throw std::runtime_error(std::string(who) + ": the contact rule is off on this handle (turn it on with mpc_sim_contacts" + (first ? " first)" : ")"));
}
// The caller's rows [B][W], one after the other: every entry of a row finite, then the model's own rules of that row, rest(row, r, b), where `row` opens
// the message ("who: row b") and r is the row.  The helpers below are what those rules are written with
template <class F> static void sim_check_rows(const char* who, const double* rows, int B, size_t W, F&& rest) {
  for (int b = 0; b < B; ++b) {
    const double* r = rows + (size_t)b * W;
    const std::string row = std::string(who) + ": row " + std::to_string(b);
    for (size_t e = 0; e < W; ++e)
      if (!std::isfinite(r[e])) throw std::runtime_error(row + " holds a non-finite entry (" + std::to_string(e) + ")");
    rest(row, r, b);
  }
}
static bool sim_is_index(double v, double n) { return v == std::floor(v) && v >= 0.0 && v < n; }
// v is one of the integers 0 .. n - 1; `bound` is the upper end as the message prints it ("7]", "2^32)")
static void sim_int_check(const std::string& row, const char* what, double v, double n, const std::string& bound) {
  if (!sim_is_index(v, n)) throw std::runtime_error(row + ": " + what + " must be an integer value in [0, " + bound);
}
static void sim_flags_check(const std::string& row, const char* what, const double* r, int n) {
  for (int e = 0; e < n; ++e)
    if (r[e] != 0.0 && r[e] != 1.0) throw std::runtime_error(row + ": " + what + " must be 0 or 1");
}
static void sim_nonneg_check(const std::string& row, const char* what, const double* r, int n) {
  for (int e = 0; e < n; ++e)
    if (r[e] < 0.0) throw std::runtime_error(row + ": " + what + " must be >= 0");
}
static void sim_nonneg_check(const std::string& row, const char* what, const double* r, std::initializer_list<int> entries) {
  for (int e : entries) sim_nonneg_check(row, what, r + e, 1);
}
static void sim_reserved_check(const std::string& row, const double* r, int lo, int hi) {
  for (int e = lo; e < hi; ++e)
    if (r[e] != 0.0) throw std::runtime_error(row + ": the reserved entries must be 0");
}
// the last entry of a state row counts the events so far; `held`: why a model that always holds something starts at 1
static void sim_count_check(const std::string& row, double count, int min, const char* held = nullptr) {
  if (count < min) throw std::runtime_error(row + ": count must be >= " + std::to_string(min) + (held ? std::string(" (") + held + ")" : std::string()));
}
// the last two entries of a state row with a ring of `ring` slots: head, count
static void sim_ring_check(const std::string& row, const double* r, size_t W, int ring, int min_count, const char* held = nullptr) {
  sim_int_check(row, "head", r[W - 2], ring, std::to_string(ring) + ")");
  sim_count_check(row, r[W - 1], min_count, held);
}
// the states [B][nx] a model is armed on; `why`: what the model does with them
static void sim_x0_check(const mpc_solver* s, const char* who, const double* x0, const char* why) {
  if (!x0) throw std::runtime_error(std::string(who) + ": x0 must not be null (" + why + ")");
  for (size_t e = 0; e < (size_t)s->L.B * s->L.nx; ++e)
    if (!std::isfinite(x0[e])) throw std::runtime_error(std::string(who) + ": x0 holds a non-finite entry");
}

// ---- layouts ------------------------------------------------------------------------------------------------------------------------------------------
// Where the parts of a model's one allocation start, in doubles from SimModel::d.  The params (the schedule: the events) come first, at 0; a model fills
// the parts it has, its layout function says which
struct SimLayout {
  size_t np = 0;                  // doubles of the params: what follows them starts here
  size_t tables = 0, tables_b = 0;  // what all the rows share, or the caller's second array
  size_t tables_c = 0;            // ... and third
  size_t out = 0;                 // what the model hands on (the consumers read it in place)
  size_t stage = 0;               // staging of the states to arm on
  size_t rows = 0, width = 0;     // the state rows [B][width]
  size_t tail = 0;                // what follows `out`
  size_t total = 0;
};
// params [B][P] | state rows [B][W]: the foot sensors and the contact detector (P 16, W 232), the friction model (P 8, W 17), the tipping model (P 8, W 21)
static SimLayout sim_rows_layout(const Layout& L, size_t P, size_t W) {
  SimLayout l;
  l.np = l.rows = (size_t)L.B * P;
  l.width = W;
  l.total = l.rows + (size_t)L.B * W;
  return l;
}
static SimLayout sim_foot_sensors_layout(const Layout& L) { return sim_rows_layout(L, MPC_SIM_FOOT_SENSORS_PARAMS, MPC_SIM_FOOT_SENSORS_WIDTH); }
static SimLayout sim_friction_layout(const Layout& L) { return sim_rows_layout(L, MPC_SIM_FRICTION_PARAMS, MPC_SIM_FRICTION_WIDTH); }
static SimLayout sim_tipping_layout(const Layout& L) { return sim_rows_layout(L, MPC_SIM_TIPPING_PARAMS, MPC_SIM_TIPPING_WIDTH); }
// the actuator model: params [B][8] | tables: limit [nu] | tables_b: friction shape [nu] | state rows [B][18 nu + 2].  The mirror holds all before the rows
static SimLayout sim_actuators_layout(const Layout& L) {
  SimLayout l;
  l.np = l.tables = (size_t)L.B * MPC_SIM_ACTUATORS_PARAMS;
  l.tables_b = l.tables + L.m;
  l.rows = l.tables_b + L.m;
  l.width = (size_t)(MPC_SIM_ACTUATORS_RING + 2) * L.m + 2;
  l.total = l.rows + (size_t)L.B * l.width;
  return l;
}
// the joint stops: params [B][8] | tables: lo [B][nu] | tables_b: hi [B][nu] | tables_c: scale [nu] | out: what the dynamics integrate [B][nu] |
// state rows [B][5 nu + 2].  The mirror holds all before `out`
static SimLayout sim_joint_stops_layout(const Layout& L) {
  SimLayout l;
  l.np = l.tables = (size_t)L.B * MPC_SIM_JOINT_STOPS_PARAMS;
  l.tables_b = l.tables + (size_t)L.B * L.m;
  l.tables_c = l.tables_b + (size_t)L.B * L.m;
  l.out = l.tables_c + L.m;
  l.rows = l.out + (size_t)L.B * L.m;
  l.width = (size_t)5 * L.m + 2;
  l.total = l.rows + (size_t)L.B * l.width;
  return l;
}
// the two models between the plant and the controllers: params [B][P] | out: what the controllers read [B][nx] | stage [B][nx] | state rows [B][W]
static SimLayout sim_filter_layout(const Layout& L, size_t P, size_t W) {
  SimLayout l;
  l.np = l.out = (size_t)L.B * P;
  l.stage = l.out + (size_t)L.B * L.nx;
  l.rows = l.stage + (size_t)L.B * L.nx;
  l.width = W;
  l.total = l.rows + (size_t)L.B * W;
  return l;
}
// the sensor model: P 16, out: the measurement, W 17 nx + 2 nu + 2 ; the base-state estimator: P 16, out: the estimate, W nx + 17
static SimLayout sim_sensors_layout(const Layout& L) {
  return sim_filter_layout(L, MPC_SIM_SENSORS_PARAMS, (size_t)(MPC_SIM_SENSORS_RING + 1) * L.nx + 2 * (size_t)L.m + 2);
}
static SimLayout sim_estimator_layout(const Layout& L) { return sim_filter_layout(L, MPC_SIM_ESTIMATOR_PARAMS, (size_t)L.nx + MPC_SIM_ESTIMATOR_TAIL); }
// the plant model: params [B][16] | tables: link_scale [B][nj] | out: the model tables [B][nd], built on the device.  The mirror holds all before `out`;
// SimPlant::plant_off keeps `out` and plant_nd keeps nd for the steps
static SimLayout sim_plant_layout(const Layout& L, size_t nd) {
  SimLayout l;
  l.np = l.tables = (size_t)L.B * MPC_SIM_PLANT_PARAMS;
  l.out = l.tables + (size_t)L.B * L.nj;
  l.total = l.out + (size_t)L.B * nd;
  return l;
}
// the disturbance schedule: events [B][ne][16] | state rows [B][32] | out: what acts in the step [B][6] | tail: its link, int32 [B]
static SimLayout sim_disturbances_layout(const Layout& L, int ne) {
  SimLayout l;
  l.np = l.rows = (size_t)L.B * ne * MPC_SIM_DISTURBANCES_EVENT;
  l.width = MPC_SIM_DISTURBANCES_WIDTH;
  l.out = l.rows + (size_t)L.B * l.width;
  l.tail = l.out + (size_t)L.B * 6;
  l.total = l.tail + ((size_t)L.B + 1) / 2;
  return l;
}

// ---- what *_read and *_set share --------------------------------------------------------------------------------------------------------------------
// *_read: the params from the mirror, then, the stream drained, the state rows and what the model hands on from the device
static void sim_model_read(mpc_solver* s, const char* who, const SimModel& m, const SimLayout& l, double* params, double* state, double* out = nullptr) {
  sim_check(s, who);
  sim_on_check(m, who);
  if (params) std::copy(m.h.begin(), m.h.begin() + l.np, params);
  HIP_OK(hipStreamSynchronize(s->stream));
  if (state) copy_sync(s, state, m.d + l.rows, (size_t)s->L.B * l.width * sizeof(double), hipMemcpyDeviceToHost);
  if (out) copy_sync(s, out, m.d + l.out, (size_t)s->L.B * s->L.nx * sizeof(double), hipMemcpyDeviceToHost);
}
// *_set: the state rows are replaced by the caller's.  The checks (state, the handle, the model on, then row by row: finite, `rest`), the stream
// drained, the upload.  slice >= 0 (the sensor model, the estimator): entries slice .. slice + nx - 1 of every row are what the controllers read, and
// go to `out`
template <class F> static void sim_rows_set(mpc_solver* s, const char* who, SimModel& m, const SimLayout& l, const double* state, long slice, F&& rest) {
  const Layout& L = s->L;
  if (!state) throw std::runtime_error(std::string(who) + ": state must not be null");
  sim_check(s, who);
  sim_on_check(m, who);
  sim_check_rows(who, state, L.B, l.width, rest);
  std::vector<double> out;
  if (slice >= 0)
    for (int b = 0; b < L.B; ++b) out.insert(out.end(), state + b * l.width + slice, state + b * l.width + slice + L.nx);
  HIP_OK(hipStreamSynchronize(s->stream));
  copy_sync(s, m.d + l.rows, state, (size_t)L.B * l.width * sizeof(double), hipMemcpyHostToDevice);
  if (slice >= 0) copy_sync(s, m.d + l.out, out.data(), out.size() * sizeof(double), hipMemcpyHostToDevice);
}

// ---- the stages of a step ---------------------------------------------------------------------------------------------------------------------------
// the model tables the plant is integrated and recorded with (include/mpc_sim_plant.h): robot b's own table at sim_plant_md + b * sim_plant_stride
// while the plant model is on, the handle's one table (stride 0) otherwise.  Everything else keeps s->d_model_d, the controllers' belief
static double* sim_plant_tables(const mpc_solver* s) { return s->plant.pm.d + s->plant.plant_off; }
static const double* sim_plant_md(const mpc_solver* s) { return s->plant.pm.on() ? sim_plant_tables(s) : s->d_model_d; }
static size_t sim_plant_stride(const mpc_solver* s) { return s->plant.pm.on() ? s->plant.plant_nd : 0; }

static SimLayout sim_disturbances_layout(const mpc_solver* s) { return sim_disturbances_layout(s->L, s->plant.dis_ne); }
// the push of a step and its width: what the schedule wrote when it is on, the armed push otherwise (the two exclude each other: mpc_sim_set_push)
static const double* sim_push(const mpc_solver* s) {
  const SimPlant& p = s->plant;
  return p.dis.on() ? p.dis.d + sim_disturbances_layout(s).out : (p.push_width ? p.d_push : nullptr);
}
// the schedule's event of the step of length dt_step about to be enqueued on stream st (sim_disturbances.h), when the model is on: it reads the state
// the step starts from and the rows the contact rule left after the step before
static void sim_disturbances_enqueue(mpc_solver* s, hipStream_t st, double dt_step) {
  const SimPlant& p = s->plant;
  if (!p.dis.on()) return;
  const Layout& L = s->L;
  const SimLayout l = sim_disturbances_layout(s);
  SimDisturbancesArgs a;
  a.mi = s->d_model_i; a.md = s->d_model_d; a.nv = L.n / 2; a.nq = L.nx - L.n / 2;
  a.x = s->d_x0; a.con = p.d_con; a.events = p.dis.d; a.n_events = p.dis_ne;
  a.rows = p.dis.d + l.rows; a.out = p.dis.d + l.out; a.link = (int32_t*)(p.dis.d + l.tail); a.dt = dt_step;
  hipLaunchKernelGGL(k_sim_disturbances, dim3((unsigned)L.B), dim3(CG_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
}
// the state rows, what acts and its link after arming or a reset: clock 0, nothing counted, nothing fired, no pair seen, nothing acting
static void sim_disturbances_reset(mpc_solver* s) {
  const Layout& L = s->L;
  const SimLayout l = sim_disturbances_layout(s);
  std::vector<double> h(l.total - l.rows, 0.0);
  for (int b = 0; b < L.B; ++b) {
    double* r = h.data() + (size_t)b * l.width;
    r[SIM_DIS_O_ACTING] = r[SIM_DIS_O_LINK] = r[SIM_DIS_O_SEEN] = r[SIM_DIS_O_SEEN + 1] = -1.0;
    for (int e = 0; e < MPC_SIM_DISTURBANCES_MAX_EVENTS; ++e) r[SIM_DIS_O_FIRE + e] = -1.0;
  }
  int32_t* link = (int32_t*)(h.data() + (l.tail - l.rows));
  for (int b = 0; b < L.B; ++b) link[b] = -1;
  HIP_OK(hipStreamSynchronize(s->stream));
  copy_sync(s, s->plant.dis.d + l.rows, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
}

// the record of the step just enqueued on stream st (sim_record.h), when recording is on
static void sim_record_enqueue(mpc_solver* s, hipStream_t st) {
  SimPlant& p = s->plant;
  if (p.rec_cap <= 0) return;
  const Layout& L = s->L;
  SimRecordArgs r;
  r.mi = s->d_model_i; r.md = sim_plant_md(s); r.md_stride = sim_plant_stride(s); r.nv = L.n / 2; r.nq = L.nx - L.n / 2;
  r.x = s->d_x0; r.tau = p.d_simu; r.wr = p.d_simwr; r.push = sim_push(s); r.push_width = p.dis.on() ? 6 : p.push_width;  // (the schedule: what acted)
  r.out = p.d_rec + (size_t)p.rec_count * L.B * sim_record_width(L.nx, L.m);
  hipLaunchKernelGGL(k_sim_record, dim3((unsigned)L.B), dim3(CG_THREADS), 0, st, r);
  HIP_OK(hipGetLastError());
  p.rec_count++;
}
// the terrain of the contact rule as the kernels take it (sim_terrain.h): boxes nullptr without one
static SimTerrain sim_terrain_args(const mpc_solver* s) {
  const SimPlant& p = s->plant;
  SimTerrain t;
  t.boxes = p.d_con ? p.ter.d : nullptr;
  t.n = p.ter_cfg.n_boxes;
  t.stride = p.ter_cfg.per_robot ? p.ter_cfg.n_boxes * MPC_SIM_TERRAIN_BOX_WIDTH : 0;
  return t;
}
// the metrics of the step of length dt just enqueued on stream st (sim_metrics.h), when they are on.  One allocation: rows [B][W] | frozen flags [B] |
// the state the next step starts from [B][nx]
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

// the actuator model of the step of length dt_step about to be enqueued on stream st (sim_actuators.h), when it is on
static void sim_actuators_enqueue(mpc_solver* s, hipStream_t st, double dt_step) {
  const SimPlant& p = s->plant;
  if (!p.act.on()) return;
  const Layout& L = s->L;
  const SimLayout l = sim_actuators_layout(L);
  SimActuatorsArgs a;
  a.nv = L.n / 2; a.nq = L.nx - L.n / 2; a.nu = L.m;
  a.x = s->d_x0; a.tau = p.d_simu;
  a.params = p.act.d; a.limit = p.act.d + l.tables; a.shape = p.act.d + l.tables_b;
  a.rows = p.act.d + l.rows; a.dt = dt_step;
  hipLaunchKernelGGL(k_sim_actuators, dim3((unsigned)L.B), dim3(SIM_ACT_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
}

// the joint stops of the step about to be enqueued on stream st (sim_joint_stops.h), when they are on: after the actuator model, before the dynamics
static void sim_joint_stops_enqueue(mpc_solver* s, hipStream_t st) {
  const SimPlant& p = s->plant;
  if (!p.js.on()) return;
  const Layout& L = s->L;
  const SimLayout l = sim_joint_stops_layout(L);
  SimJointStopsArgs a;
  a.nv = L.n / 2; a.nq = L.nx - L.n / 2; a.nu = L.m;
  a.x = s->d_x0; a.tau = p.d_simu;
  a.params = p.js.d; a.lo = p.js.d + l.tables; a.hi = p.js.d + l.tables_b; a.scale = p.js.d + l.tables_c;
  a.out = p.js.d + l.out; a.rows = p.js.d + l.rows;
  hipLaunchKernelGGL(k_sim_joint_stops, dim3((unsigned)L.B), dim3(SIM_JS_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
}
// the torque the dynamics of a step integrate, [B][nu]: what the joint stops wrote when they are on, the step's torque buffer otherwise
static const double* sim_integrated_torques(const mpc_solver* s) {
  return s->plant.js.on() ? s->plant.js.d + sim_joint_stops_layout(s->L).out : s->plant.d_simu;
}

// what the sensors deliver, [B][nx]: the measurement of the sensor model when it is on, the true state otherwise
static const double* sim_sensed(const mpc_solver* s) { return s->plant.sen.on() ? s->plant.sen.d + sim_sensors_layout(s->L).out : s->d_x0; }
// the state the controllers read, [B][nx]: the estimate of the base-state estimator when it is on, what the sensors deliver otherwise
static const double* sim_measured(const mpc_solver* s) { return s->plant.est.on() ? s->plant.est.d + sim_estimator_layout(s->L).out : sim_sensed(s); }
// the measurement event of the true states x, produced by a step of length dt_step, on stream st (sim_sensors.h), when the model is on
static void sim_sensors_enqueue(mpc_solver* s, hipStream_t st, const double* x, double dt_step) {
  const SimPlant& p = s->plant;
  if (!p.sen.on()) return;
  const Layout& L = s->L;
  const SimLayout l = sim_sensors_layout(L);
  SimSensorsArgs a;
  a.nv = L.n / 2; a.nq = L.nx - L.n / 2; a.nu = L.m;
  a.x = x; a.params = p.sen.d; a.xm = p.sen.d + l.out; a.rows = p.sen.d + l.rows; a.dt = dt_step;
  hipLaunchKernelGGL(k_sim_sensors, dim3((unsigned)L.B), dim3(SIM_SEN_THREADS), sim_sensors_lds_bytes(a.nv), st, a);
  HIP_OK(hipGetLastError());
}

// the rows a consumer of contact flags indexes by 0 and 1, and their width: the state rows of the contact detector when it feeds that consumer
// (mpc_sim_foot_sensors_feed: one MPC_SIM_FOOT_SENSORS_FEED_* bit), the rows of the contact rule otherwise
struct SimContactRows { const double* rows; int width; };
static SimContactRows sim_contact_rows(const mpc_solver* s, int consumer) {
  const SimPlant& p = s->plant;
  if (p.fs.on() && (p.fs_feed & consumer)) return {p.fs.d + sim_foot_sensors_layout(s->L).rows, MPC_SIM_FOOT_SENSORS_WIDTH};
  return {p.d_con, MPC_SIM_CONTACTS_WIDTH};
}
// the detection event of the wrenches of the step of length dt_step just enqueued on stream st (sim_foot_sensors.h), when the model is on
static void sim_foot_sensors_enqueue(mpc_solver* s, hipStream_t st, double dt_step) {
  const SimPlant& p = s->plant;
  if (!p.fs.on()) return;
  SimFootSensorsArgs a;
  a.wr = p.d_simwr; a.con = p.d_con; a.params = p.fs.d; a.rows = p.fs.d + sim_foot_sensors_layout(s->L).rows; a.dt = dt_step;
  hipLaunchKernelGGL(k_sim_foot_sensors, dim3((unsigned)s->L.B), dim3(SIM_FS_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
}
// the state rows after arming: det = the in_contact pair of the contact rule's rows (`con` the rows on the host, NULL: read from the device),
// everything else 0.  Host work, not part of the steady loop
static void sim_foot_sensors_arm(mpc_solver* s, const double* con) {
  if (!s->plant.fs.on()) return;
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
  copy_sync(s, s->plant.fs.d + sim_foot_sensors_layout(L).rows, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
}

// the estimation event of the measured states xm and the true states xt on stream st (sim_estimator.h), when the estimator is on: it reads the rows
// of the contact rule, or of the contact detector when that feeds it (sim_contact_rows), as they stand on the stream
static void sim_estimator_enqueue(mpc_solver* s, hipStream_t st, const double* xm, const double* xt) {
  const SimPlant& p = s->plant;
  if (!p.est.on()) return;
  const Layout& L = s->L;
  const SimLayout l = sim_estimator_layout(L);
  SimEstimatorArgs a;
  a.mi = s->d_model_i; a.md = s->d_model_d; a.nv = L.n / 2; a.nq = L.nx - L.n / 2;
  const SimContactRows cr = sim_contact_rows(s, MPC_SIM_FOOT_SENSORS_FEED_ESTIMATOR);
  a.xm = xm; a.xt = xt; a.con = cr.rows; a.con_width = cr.width; a.params = p.est.d; a.xe = p.est.d + l.out; a.rows = p.est.d + l.rows;
  hipLaunchKernelGGL(k_sim_estimator, dim3((unsigned)L.B), dim3(CG_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
}
// the friction model of the step of length dt_step just enqueued on stream st, after the contact rule (sim_friction.h), when the model is on
static void sim_friction_enqueue(mpc_solver* s, hipStream_t st, double dt_step) {
  const SimPlant& p = s->plant;
  if (!p.fr.on()) return;
  SimFrictionArgs a;
  a.B = s->L.B; a.wr = p.d_simwr; a.con = p.d_con; a.params = p.fr.d; a.rows = p.fr.d + sim_friction_layout(s->L).rows; a.dt = dt_step;
  hipLaunchKernelGGL(k_sim_friction, dim3((unsigned)((2 * s->L.B + SIM_FR_THREADS - 1) / SIM_FR_THREADS)), dim3(SIM_FR_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
}
// the tipping model of the step of length dt_step just enqueued on stream st, after the contact rule and friction (sim_tipping.h), when the model is on
static void sim_tipping_enqueue(mpc_solver* s, hipStream_t st, double dt_step) {
  const SimPlant& p = s->plant;
  if (!p.tip.on()) return;
  SimTippingArgs a;
  a.B = s->L.B; a.wr = p.d_simwr; a.con = p.d_con; a.params = p.tip.d; a.rows = p.tip.d + sim_tipping_layout(s->L).rows; a.dt = dt_step;
  hipLaunchKernelGGL(k_sim_tipping, dim3((unsigned)((2 * s->L.B + SIM_TP_THREADS - 1) / SIM_TP_THREADS)), dim3(SIM_TP_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
}

// the plant model's tables, built from the rows in force (the mirror) and the handle's nominal table: when the model is armed, and when mpc_set_model
// replaced the nominal table of an armed handle (the joint count is then unchanged; the table may have grown by a frame).  Synchronous: the tables
// may be read from any stream at once (the loops of the QP pipelines step the plant on the QP handle's).  Host work, not part of the steady loop
static void sim_plant_build(mpc_solver* s) {
  SimPlant& p = s->plant;
  if (!p.pm.on()) return;
  const Layout& L = s->L;
  const SimLayout l = sim_plant_layout(L, s->model_nd);
  if (p.plant_nd != s->model_nd) {
    sim_realloc(s, p.pm.d, l.total);
    p.plant_nd = s->model_nd;
  }
  copy_sync(s, p.pm.d, p.pm.h.data(), l.out * sizeof(double), hipMemcpyHostToDevice);
  SimPlantArgs a;
  a.md = s->d_model_d; a.nd = (int)p.plant_nd; a.nj = L.nj;
  a.params = p.pm.d; a.link_scale = p.pm.d + l.tables; a.tables = p.pm.d + l.out;
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
// the dynamics write the wrenches of the step when the caller or anything after the dynamics reads them
static bool sim_wrenches_wanted(const SimPlant& p, bool by_caller) {
  return by_caller || p.rec_cap > 0 || p.d_met || p.d_con || p.fs.on() || p.fr.on() || p.tip.on();
}
// One step of the plant on stream st: `substeps` integration steps of length dt under the torque the caller put into plant.d_simu.  The order is the
// contract of the extensions; a stage whose model is off launches nothing.  Each event covers the whole step (substeps * dt).
//    1 disturbances  reads the state the step starts from and the contact rows of the step BEFORE ; writes the force, point and link that act in
//                    this step's dynamics, in place of the armed push
//    2 actuators     reads the commanded torque and the state ; writes the applied torque in place: everything after it sees the applied torque
//    2b joint stops  reads the TRUE state the step starts from and the applied torque ; writes, into a buffer of its own, the applied torque plus the
//                    stop torque of every joint beyond its range: the dynamics alone read that buffer, everything after them keeps the applied torque
//    3 dynamics      reads the applied torque (with the joint stops on: their sum), the push, the contact rows of the step BEFORE (the rows the low-level QPs of pipeline_loops.h read
//                    for this step), the slip and tip velocities friction and tipping set after the step before, robot b's own model table (the plant model, built
//                    when it was armed: it launches nothing here) ; writes the new state and, when wanted (sim_wrenches_wanted), the wrenches
//    4 record        reads the new state, the applied torque, the wrenches, the push, the plant's model tables ; writes its slot of the ring
//    5 metrics       reads the same and the contact rows the step was integrated with ; writes the metric rows
//    6 contact rule  reads the new state and this step's wrenches ; rewrites the contact rows, for the NEXT step
//    7 friction      reads this step's wrenches and the flags the rule just wrote ; writes the slip velocity each held sole has in the NEXT step's
//                    dynamics and advances the anchors of the soles that slid in this one
//    8 tipping       reads this step's wrenches, the flags the rule just wrote and the anchors as friction left them ; writes the tip velocity
//                    (v_z, w_x, w_y) each held sole has in the NEXT step's dynamics and advances the anchors of the soles that tipped in this one
//    9 sensors       reads the new state ; writes the measurement
//   10 foot sensors  reads this step's wrenches ; writes the detected pair: an estimator fed by detection reads the pair this step's event left,
//                    and the low-level QPs of the next step the same pair
//   11 estimator     reads that measurement (the true state without a sensor model) and the contact rows the rule, or the detector, just wrote ;
//                    writes the estimate.  Nothing of this step reads 9 to 11: the controllers of the next step do (sim_measured)
static void sim_step_enqueue(mpc_solver* s, hipStream_t st, const SolverArgs& args, int substeps, double dt, bool want_wrenches) {
  const SimPlant& p = s->plant;
  sim_disturbances_enqueue(s, st, substeps * dt);
  sim_actuators_enqueue(s, st, substeps * dt);
  sim_joint_stops_enqueue(s, st);
  MbSimStep step;
  step.substeps = substeps; step.dt = dt;
  step.push = sim_push(s); step.width = p.dis.on() ? 6 : (p.push_width ? p.push_width : 3); step.linked = p.dis.on();
  step.torques = sim_integrated_torques(s); step.wrenches = sim_wrenches_wanted(p, want_wrenches) ? p.d_simwr : nullptr;
  step.contact_rows = p.d_con;
  step.model_tables = p.pm.on() ? sim_plant_tables(s) : nullptr; step.model_stride = sim_plant_stride(s);
  step.friction_rows = p.fr.on() ? p.fr.d + sim_friction_layout(s->L).rows : nullptr;
  step.tipping_rows = p.tip.on() ? p.tip.d + sim_tipping_layout(s->L).rows : nullptr;
  launch_sim_multibody(st, args, s->LT, s->d_tknots, s->d_mbwork, s->mb_work_stride, step);
  HIP_OK(hipGetLastError());
  sim_record_enqueue(s, st);
  sim_metrics_enqueue(s, st, substeps * dt);
  sim_contacts_enqueue(s, st);
  sim_friction_enqueue(s, st, substeps * dt);
  sim_tipping_enqueue(s, st, substeps * dt);
  sim_sensors_enqueue(s, st, s->d_x0, substeps * dt);
  sim_foot_sensors_enqueue(s, st, substeps * dt);
  sim_estimator_enqueue(s, st, sim_sensed(s), s->d_x0);
}

// Arming the sensor model or the estimator (params NULL: off), after the model's own checks of the params: the checks of x0, then of the contact
// rule if the model reads its rows — every check before anything changes, so that a bad call leaves the previous configuration in force.  Then the
// rows all 0 and the arming event (count 1) on x0, which `event` enqueues on the staged states; synchronous
template <class E> static void sim_filter_arm(mpc_solver* s, const char* who, SimModel& m, const SimLayout& l, const double* params, const double* x0,
                                              const char* x0_why, E&& event) {
  if (!params) { sim_drop(s, m); return; }
  sim_x0_check(s, who, x0, x0_why);
  if (m.needs_rule) sim_rule_check(s, who);
  sim_realloc(s, m.d, l.total);
  m.h.assign(params, params + l.np);
  HIP_OK(hipMemsetAsync(m.d, 0, l.total * sizeof(double), s->stream));
  copy_sync(s, m.d, params, l.np * sizeof(double), hipMemcpyHostToDevice);
  copy_sync(s, m.d + l.stage, x0, (size_t)s->L.B * s->L.nx * sizeof(double), hipMemcpyHostToDevice);
  event(m.d + l.stage);
  HIP_OK(hipStreamSynchronize(s->stream));
}

extern "C" {

// ---- include/mpc_sim_ext.h: push and record -----------------------------------------------------------------------------------------------
int mpc_sim_set_push(mpc_solver* s, const double* f_ext, int32_t width) {
  MPC_TRY(s, {
    sim_check(s, "sim_set_push");
    if (!f_ext) { s->plant.push_width = 0; return 0; }
    if (s->plant.dis.on())
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
int mpc_sim_contacts(mpc_solver* s, const mpc_sim_contacts_config* cfg) {
  MPC_TRY(s, {
    sim_check(s, "sim_contacts");
    SimPlant& p = s->plant;
    if (cfg) {
      sim_model_check(s, "sim_contacts");
      if (!std::isfinite(cfg->ground_z) || !std::isfinite(cfg->ground_tol) || !std::isfinite(cfg->release_force))
        throw std::runtime_error("sim_contacts: ground_z, ground_tol and release_force must be finite");
      if (cfg->ground_tol < 0.0 || cfg->release_force < 0.0) throw std::runtime_error("sim_contacts: ground_tol and release_force must be >= 0");
      if (cfg->release_steps < 1) throw std::runtime_error("sim_contacts: release_steps must be >= 1");
    }
    sim_realloc(s, p.d_con, cfg ? (size_t)s->L.B * MPC_SIM_CONTACTS_WIDTH : 0);
    if (!cfg)  // (what reads the rows goes with them, a schedule when one of its triggers is a contact; a reset keeps them all)
      for (SimModel* m : p.models)
        if (m->needs_rule || (m == &p.dis && p.dis_contact)) sim_drop(s, *m);
    if (cfg) {
      p.con_cfg = *cfg;
      p.con_cfg.reserved = 0;
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
    sim_rule_check(s, "sim_contacts_set", false);
    const Layout& L = s->L;
    sim_check_rows("sim_contacts_set", rows, L.B, MPC_SIM_CONTACTS_WIDTH, [&](const std::string& row, const double* r, int) {
      sim_flags_check(row, "in_contact and lifted", r, 4);
      if (r[0] == 0.0 && r[1] == 0.0) throw std::runtime_error(row + " has no sole in contact (flight phases are not simulated)");
      sim_nonneg_check(row, "pulling, the counts and steps", r, {4, 5, 32, 33, 34, 35, 40});
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
    });
    HIP_OK(hipStreamSynchronize(s->stream));
    copy_sync(s, s->plant.d_con, rows, (size_t)L.B * MPC_SIM_CONTACTS_WIDTH * sizeof(double), hipMemcpyHostToDevice);
    sim_foot_sensors_arm(s, rows);  // (... and from rows imposed)
  })
}

int mpc_sim_contacts_read(mpc_solver* s, double* rows) {
  MPC_TRY(s, {
    if (!rows) throw std::runtime_error("sim_contacts_read: rows must not be null");
    sim_check(s, "sim_contacts_read");
    sim_rule_check(s, "sim_contacts_read", false);
    HIP_OK(hipStreamSynchronize(s->stream));
    copy_sync(s, rows, s->plant.d_con, (size_t)s->L.B * MPC_SIM_CONTACTS_WIDTH * sizeof(double), hipMemcpyDeviceToHost);
  })
}

int mpc_sim_terrain(mpc_solver* s, const mpc_sim_terrain_config* cfg, const double* boxes) {
  MPC_TRY(s, {
    sim_check(s, "sim_terrain");
    sim_rule_check(s, "sim_terrain");
    SimPlant& p = s->plant;
    size_t count = 0;
    if (cfg) {
      if (cfg->n_boxes < 0 || cfg->n_boxes > MPC_SIM_TERRAIN_MAX_BOXES)
        throw std::runtime_error("sim_terrain: n_boxes must be 0 .. " + std::to_string(MPC_SIM_TERRAIN_MAX_BOXES));
      if (cfg->per_robot != 0 && cfg->per_robot != 1) throw std::runtime_error("sim_terrain: per_robot must be 0 or 1");
      if (cfg->n_boxes > 0 && !boxes) throw std::runtime_error("sim_terrain: boxes must not be null with n_boxes > 0");
      count = (size_t)(cfg->per_robot ? s->L.B : 1) * cfg->n_boxes;
      for (size_t k = 0; k < count; ++k) {
        const double* bx = boxes + k * MPC_SIM_TERRAIN_BOX_WIDTH;
        for (int e = 0; e < MPC_SIM_TERRAIN_BOX_WIDTH; ++e)
          if (!std::isfinite(bx[e])) throw std::runtime_error("sim_terrain: box " + std::to_string(k) + " holds a non-finite number");
        if (bx[0] > bx[1] || bx[2] > bx[3]) throw std::runtime_error("sim_terrain: box " + std::to_string(k) + " has x_lo > x_hi or y_lo > y_hi");
      }
    }
    sim_drop(s, p.ter);
    if (cfg) {
      p.ter_cfg = *cfg;
      p.ter.h.assign(boxes, boxes + count * MPC_SIM_TERRAIN_BOX_WIDTH);
      if (count > 0) {  // (zero boxes: the plane, by the old path)
        std::vector<double> h(p.ter.h);
        for (size_t k = 0; k < count; ++k) h[k * MPC_SIM_TERRAIN_BOX_WIDTH + 4] += 0.0;  // (a top of -0 counts as +0, as in the numpy definition)
        sim_realloc(s, p.ter.d, h.size());
        copy_sync(s, p.ter.d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
      }
    }
  })
}

int mpc_sim_terrain_read(mpc_solver* s, mpc_sim_terrain_config* cfg, double* boxes) {
  MPC_TRY(s, {
    if (!cfg) throw std::runtime_error("sim_terrain_read: cfg must not be null");
    sim_check(s, "sim_terrain_read");
    sim_rule_check(s, "sim_terrain_read");
    *cfg = s->plant.ter_cfg;
    if (boxes) std::copy(s->plant.ter.h.begin(), s->plant.ter.h.end(), boxes);
  })
}

int mpc_sim_terrain_height(mpc_solver* s, const double* xy, int32_t n, double* h) {
  MPC_TRY(s, {
    sim_check(s, "sim_terrain_height");
    sim_rule_check(s, "sim_terrain_height");
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
    const SimLayout l = sim_actuators_layout(L);
    SimModel& m = s->plant.act;
    if (!params) { sim_drop(s, m); return 0; }
    // (every check before anything changes: a bad row leaves the previous configuration in force)
    std::vector<double> h(params, params + l.np);
    h.resize(l.total, 0.0);  // (params | limit | shape, then the state rows after a reset: all 0)
    bool any_sat = false;
    sim_check_rows("sim_actuators", params, L.B, MPC_SIM_ACTUATORS_PARAMS, [&](const std::string& row, const double* r, int b) {
      sim_int_check(row, "delay", r[0], MPC_SIM_ACTUATORS_RING, std::to_string(MPC_SIM_ACTUATORS_RING - 1) + "]");
      if (!(r[1] > 0.0)) throw std::runtime_error(row + ": scale must be > 0");
      sim_nonneg_check(row, "time_constant, damping, coulomb, v_eps and sat", r + 2, 5);
      if (r[4] > 0.0 && !(r[5] > 0.0)) throw std::runtime_error(row + ": coulomb > 0 needs v_eps > 0");
      if (r[6] > 0.0) any_sat = true;
      h[(size_t)b * MPC_SIM_ACTUATORS_PARAMS + 7] = 0.0;  // (the reserved entry)
    });
    if (any_sat && !limit) throw std::runtime_error("sim_actuators: a row with sat > 0 needs the effort limits (limit must not be null)");
    for (int j = 0; j < L.m; ++j) {
      const double lim = limit ? limit[j] : 0.0, f = friction_shape ? friction_shape[j] : 1.0;
      if (!std::isfinite(lim) || lim < 0.0 || !std::isfinite(f) || f < 0.0)
        throw std::runtime_error("sim_actuators: limit and friction_shape must be finite and >= 0");
      h[l.tables + j] = lim;
      h[l.tables_b + j] = f;
    }
    sim_realloc(s, m.d, l.total);
    m.h.assign(h.begin(), h.begin() + l.rows);
    copy_sync(s, m.d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
  })
}

int mpc_sim_actuators_read(mpc_solver* s, double* params, double* state) {
  MPC_TRY(s, { sim_model_read(s, "sim_actuators_read", s->plant.act, sim_actuators_layout(s->L), params, state); })
}

int mpc_sim_actuators_set(mpc_solver* s, const double* state) {
  MPC_TRY(s, {
    const SimLayout l = sim_actuators_layout(s->L);
    sim_rows_set(s, "sim_actuators_set", s->plant.act, l, state, -1,
                 [&](const std::string& row, const double* r, int) { sim_ring_check(row, r, l.width, MPC_SIM_ACTUATORS_RING, 0); });
  })
}

int32_t mpc_sim_actuators_width(mpc_solver* s) { return sim_width(s, "sim_actuators_width", [&] { return sim_actuators_layout(s->L).width; }); }

// ---- include/mpc_sim_joint_stops.h: the per-robot joint end-stops of the torque-driven simulator steps -----------------------------------------
int mpc_sim_joint_stops(mpc_solver* s, const double* params, const double* lo, const double* hi, const double* scale) {
  MPC_TRY(s, {
    sim_check(s, "sim_joint_stops");
    const Layout& L = s->L;
    const SimLayout l = sim_joint_stops_layout(L);
    SimModel& m = s->plant.js;
    if (!params) { sim_drop(s, m); return 0; }
    // (every check before anything changes: a refused call leaves the previous configuration in force; cap and the limits may be infinite)
    if (!lo || !hi) throw std::runtime_error("sim_joint_stops: lo and hi must not be null");
    const size_t nu = L.m;
    std::vector<double> h(params, params + l.np);
    h.resize(l.total, 0.0);  // (params | lo | hi | scale | out, then the state rows after a reset: all 0)
    for (int b = 0; b < L.B; ++b) {
      const double* r = params + (size_t)b * MPC_SIM_JOINT_STOPS_PARAMS;
      const std::string row = "sim_joint_stops: row " + std::to_string(b);
      if (!std::isfinite(r[0]) || !std::isfinite(r[1])) throw std::runtime_error(row + ": k and d must be finite");
      sim_nonneg_check(row, "k and d", r, 2);
      if (!(r[2] > 0.0)) throw std::runtime_error(row + ": cap must be > 0 (+inf: none)");
      sim_reserved_check(row, r, 3, MPC_SIM_JOINT_STOPS_PARAMS);
      for (size_t j = 0; j < nu; ++j) {
        const double lj = lo[b * nu + j], hj = hi[b * nu + j];
        const std::string joint = row + ", joint " + std::to_string(j);
        if (std::isnan(lj) || std::isnan(hj)) throw std::runtime_error(joint + ": a limit is NaN");
        if (lj > hj) throw std::runtime_error(joint + ": lo > hi");
        if (lj == std::numeric_limits<double>::infinity() || hj == -std::numeric_limits<double>::infinity())
          throw std::runtime_error(joint + ": lo must be < +inf and hi > -inf (-inf / +inf: no stop on that side)");
        h[l.tables + b * nu + j] = lj;
        h[l.tables_b + b * nu + j] = hj;
      }
    }
    for (size_t j = 0; j < nu; ++j) {
      const double sc = scale ? scale[j] : 1.0;
      if (!std::isfinite(sc) || !(sc > 0.0)) throw std::runtime_error("sim_joint_stops: scale must be finite and > 0 (joint " + std::to_string(j) + ")");
      h[l.tables_c + j] = sc;
    }
    sim_realloc(s, m.d, l.total);
    m.h.assign(h.begin(), h.begin() + l.out);
    copy_sync(s, m.d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
  })
}

int mpc_sim_joint_stops_read(mpc_solver* s, double* params, double* lo, double* hi, double* state) {
  MPC_TRY(s, {
    const SimLayout l = sim_joint_stops_layout(s->L);
    const SimModel& m = s->plant.js;
    sim_model_read(s, "sim_joint_stops_read", m, l, params, state);
    if (lo) std::copy(m.h.begin() + l.tables, m.h.begin() + l.tables_b, lo);
    if (hi) std::copy(m.h.begin() + l.tables_b, m.h.begin() + l.tables_c, hi);
  })
}

int mpc_sim_joint_stops_set(mpc_solver* s, const double* state) {
  MPC_TRY(s, {
    const SimLayout l = sim_joint_stops_layout(s->L);
    const int nu = s->L.m;
    sim_rows_set(s, "sim_joint_stops_set", s->plant.js, l, state, -1, [&](const std::string& row, const double* r, int) {
      sim_nonneg_check(row, "peak_pen, stop_steps, hits, any_steps and steps", r + 2 * nu, 3 * nu + 2);
      for (int j = 0; j < nu; ++j)
        if (std::fabs(r[nu + j]) > r[2 * nu + j]) throw std::runtime_error(row + ": joint " + std::to_string(j) + " holds a |pen| above its peak_pen");
    });
  })
}

int32_t mpc_sim_joint_stops_width(mpc_solver* s) { return sim_width(s, "sim_joint_stops_width", [&] { return sim_joint_stops_layout(s->L).width; }); }

// ---- include/mpc_sim_sensors.h, include/mpc_sim_estimator.h: the two per-robot models between the simulator steps and the controllers ----------
int mpc_sim_sensors(mpc_solver* s, const double* params, const double* x0) {
  MPC_TRY(s, {
    sim_check(s, "sim_sensors");
    if (params)
      sim_check_rows("sim_sensors", params, s->L.B, MPC_SIM_SENSORS_PARAMS, [&](const std::string& row, const double* r, int) {
        sim_int_check(row, "delay", r[0], MPC_SIM_SENSORS_RING, std::to_string(MPC_SIM_SENSORS_RING - 1) + "]");
        sim_nonneg_check(row, "the noise levels (sigma_*), quantum, q_bias and v_time_constant", r, {1, 2, 3, 4, 5, 6, 7, 8, 10});
        sim_flags_check(row, "v_from_q", r + 9, 1);
        sim_int_check(row, "seed", r[11], 4294967296.0, "2^32)");
        sim_reserved_check(row, r, 12, MPC_SIM_SENSORS_PARAMS);
      });
    sim_filter_arm(s, "sim_sensors", s->plant.sen, sim_sensors_layout(s->L), params, x0, "the first measurement is taken of it",
                   [&](const double* stage) { sim_sensors_enqueue(s, s->stream, stage, 0.0); });
  })
}

int mpc_sim_sensors_read(mpc_solver* s, double* params, double* state, double* x_meas) {
  MPC_TRY(s, { sim_model_read(s, "sim_sensors_read", s->plant.sen, sim_sensors_layout(s->L), params, state, x_meas); })
}

int mpc_sim_sensors_set(mpc_solver* s, const double* state) {
  MPC_TRY(s, {
    const SimLayout l = sim_sensors_layout(s->L);  // (the controllers read the rows' measurement: the slice behind the ring)
    sim_rows_set(s, "sim_sensors_set", s->plant.sen, l, state, (long)MPC_SIM_SENSORS_RING * s->L.nx, [&](const std::string& row, const double* r, int) {
      sim_ring_check(row, r, l.width, MPC_SIM_SENSORS_RING, 1, "a measurement is always held");
    });
  })
}

int32_t mpc_sim_sensors_width(mpc_solver* s) { return sim_width(s, "sim_sensors_width", [&] { return sim_sensors_layout(s->L).width; }); }

int mpc_sim_estimator(mpc_solver* s, const double* params, const double* x0) {
  MPC_TRY(s, {
    sim_check(s, "sim_estimator");
    if (params) {
      sim_model_check(s, "sim_estimator");
      if (s->L.nx > SIM_EST_MAX_NX) throw std::runtime_error("sim_estimator: a longer state than the estimator's kernel holds (" + std::to_string(SIM_EST_MAX_NX) + ")");
      sim_check_rows("sim_estimator", params, s->L.B, MPC_SIM_ESTIMATOR_PARAMS, [&](const std::string& row, const double* r, int) {
        for (int e = 0; e < 2; ++e)
          if (r[e] < 0.0 || r[e] > 1.0) throw std::runtime_error(row + ": the weights w_p and w_v must be in [0, 1]");
        sim_reserved_check(row, r, 2, MPC_SIM_ESTIMATOR_PARAMS);
      });
    }
    sim_filter_arm(s, "sim_estimator", s->plant.est, sim_estimator_layout(s->L), params, x0, "the arming event is run on it",
                   [&](const double* stage) { sim_estimator_enqueue(s, s->stream, stage, stage); });
  })
}

int mpc_sim_estimator_read(mpc_solver* s, double* params, double* state, double* x_est) {
  MPC_TRY(s, { sim_model_read(s, "sim_estimator_read", s->plant.est, sim_estimator_layout(s->L), params, state, x_est); })
}

int mpc_sim_estimator_set(mpc_solver* s, const double* state) {
  MPC_TRY(s, {
    const SimLayout l = sim_estimator_layout(s->L);  // (the controllers read the rows' estimate: the slice at 0)
    sim_rows_set(s, "sim_estimator_set", s->plant.est, l, state, 0, [&](const std::string& row, const double* r, int) {
      sim_flags_check(row, "held", r + s->L.nx, 2);
      sim_count_check(row, r[l.width - 1], 1, "an estimate is always held");
    });
  })
}

int32_t mpc_sim_estimator_width(mpc_solver* s) { return sim_width(s, "sim_estimator_width", [&] { return sim_estimator_layout(s->L).width; }); }

// ---- include/mpc_sim_foot_sensors.h: the per-robot foot force sensors and the contact detector ----------------------------------------------------
int mpc_sim_foot_sensors(mpc_solver* s, const double* params) {
  MPC_TRY(s, {
    sim_check(s, "sim_foot_sensors");
    const SimLayout l = sim_foot_sensors_layout(s->L);
    SimModel& m = s->plant.fs;
    if (!params) { sim_drop(s, m); return 0; }
    // (every check before anything changes: a bad row leaves the previous configuration in force)
    sim_check_rows("sim_foot_sensors", params, s->L.B, MPC_SIM_FOOT_SENSORS_PARAMS, [&](const std::string& row, const double* r, int) {
      sim_int_check(row, "delay", r[0], MPC_SIM_FOOT_SENSORS_RING, std::to_string(MPC_SIM_FOOT_SENSORS_RING - 1) + "]");
      sim_nonneg_check(row, "sigma_f, sigma_m, bias_f, bias_m and time_constant", r + 1, 5);
      if (r[7] > r[6]) throw std::runtime_error(row + ": f_off must be <= f_on");
      for (int e = 8; e < 10; ++e)
        if (r[e] != std::floor(r[e]) || r[e] < 1.0) throw std::runtime_error(row + ": on_steps and off_steps must be integer values >= 1");
      sim_int_check(row, "seed", r[10], 4294967296.0, "2^32)");
      sim_reserved_check(row, r, 11, MPC_SIM_FOOT_SENSORS_PARAMS);
    });
    if (m.needs_rule) sim_rule_check(s, "sim_foot_sensors");
    sim_realloc(s, m.d, l.total);
    m.h.assign(params, params + l.np);
    sim_ensure(s);
    copy_sync(s, m.d, params, l.np * sizeof(double), hipMemcpyHostToDevice);
    sim_foot_sensors_arm(s, nullptr);
  })
}

int mpc_sim_foot_sensors_read(mpc_solver* s, double* params, double* state) {
  MPC_TRY(s, { sim_model_read(s, "sim_foot_sensors_read", s->plant.fs, sim_foot_sensors_layout(s->L), params, state); })
}

int mpc_sim_foot_sensors_set(mpc_solver* s, const double* state) {
  MPC_TRY(s, {
    const SimLayout l = sim_foot_sensors_layout(s->L);
    sim_rows_set(s, "sim_foot_sensors_set", s->plant.fs, l, state, -1, [&](const std::string& row, const double* r, int) {
      sim_flags_check(row, "det", r, 2);
      if (r[0] == 0.0 && r[1] == 0.0) throw std::runtime_error(row + " has no sole detected (the detector never reports an empty set)");
      sim_nonneg_check(row, "the counters above and below", r + SIM_FS_O_ABOVE, SIM_FS_O_WF - SIM_FS_O_ABOVE);
      sim_nonneg_check(row, "the confusion counts", r + SIM_FS_O_COUNTS, SIM_FS_O_RING - SIM_FS_O_COUNTS);
      sim_ring_check(row, r, l.width, MPC_SIM_FOOT_SENSORS_RING, 0);
    });
  })
}

int32_t mpc_sim_foot_sensors_width(mpc_solver* s) { return sim_width(s, "sim_foot_sensors_width", [&] { return MPC_SIM_FOOT_SENSORS_WIDTH; }); }

int mpc_sim_foot_sensors_feed(mpc_solver* s, int32_t consumers) {
  MPC_TRY(s, {
    sim_check(s, "sim_foot_sensors_feed");
    sim_on_check(s->plant.fs, "sim_foot_sensors_feed");
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
    SimPlant& p = s->plant;
    if (!params) { sim_drop(s, p.pm); return 0; }
    // (every check before anything changes: a bad row leaves the previous configuration in force)
    if (!s->have_model || !s->d_model_d || s->h_model_i.empty()) throw std::runtime_error("sim_plant: no model is set on this handle (mpc_set_model first)");
    const int nj = L.nj;
    const SimLayout l = sim_plant_layout(L, s->model_nd);
    std::vector<double> h(params, params + l.np);
    h.resize(l.out, 1.0);  // (link_scale: ones when none is given)
    sim_check_rows("sim_plant", params, L.B, MPC_SIM_PLANT_PARAMS, [&](const std::string& row, const double* r, int) {
      if (!(r[0] > 0.0) || !(r[1] > 0.0)) throw std::runtime_error(row + ": mass_scale and inertia_scale must be > 0");
      sim_nonneg_check(row, "payload_mass", r + 7, 1);
      for (int e : {2, 6})
        if (!sim_is_index(r[e], nj))
          throw std::runtime_error(row + ": shift_body and payload_body must be integer values in [0, " + std::to_string(nj - 1) + "] (table joint indices)");
      sim_reserved_check(row, r, 11, MPC_SIM_PLANT_PARAMS);
    });
    if (link_scale)
      for (size_t e = 0; e < (size_t)L.B * nj; ++e) {
        if (!std::isfinite(link_scale[e]) || !(link_scale[e] > 0.0))
          throw std::runtime_error("sim_plant: link_scale must be finite and > 0 (robot " + std::to_string(e / nj) + ", joint " + std::to_string(e % nj) + ")");
        h[l.tables + e] = link_scale[e];
      }
    sim_realloc(s, p.pm.d, l.total);
    p.plant_nd = s->model_nd;
    p.plant_off = l.out;
    p.pm.h = h;
    sim_plant_build(s);
  })
}

int mpc_sim_plant_read(mpc_solver* s, double* params, double* link_scale, double* tables) {
  MPC_TRY(s, {
    sim_check(s, "sim_plant_read");
    const SimPlant& p = s->plant;
    sim_on_check(p.pm, "sim_plant_read");
    const SimLayout l = sim_plant_layout(s->L, p.plant_nd);
    if (params) std::copy(p.pm.h.begin(), p.pm.h.begin() + l.np, params);
    if (link_scale) std::copy(p.pm.h.begin() + l.tables, p.pm.h.end(), link_scale);
    HIP_OK(hipStreamSynchronize(s->stream));
    if (tables) copy_sync(s, tables, p.pm.d + l.out, (l.total - l.out) * sizeof(double), hipMemcpyDeviceToHost);
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
    const SimLayout l = sim_friction_layout(L);
    SimModel& m = s->plant.fr;
    if (!params) { sim_drop(s, m); return 0; }
    for (int b = 0; b < L.B; ++b) {  // (every check before anything changes: a bad row leaves the previous configuration in force; mu may be +inf)
      const double* r = params + (size_t)b * MPC_SIM_FRICTION_PARAMS;
      const std::string row = "sim_friction: row " + std::to_string(b);
      for (int e = 0; e < 4; ++e)
        if (std::isnan(r[e]) || r[e] < 0.0) throw std::runtime_error(row + ": mu and mu_spin must be >= 0 (+inf: the sole never slides), entry " + std::to_string(e));
      for (int e = 4; e < MPC_SIM_FRICTION_PARAMS; ++e)
        if (!std::isfinite(r[e]) || !(r[e] > 0.0)) throw std::runtime_error(row + ": m_slip, I_slip, v_max and w_max must be finite and > 0, entry " + std::to_string(e));
    }
    if (m.needs_rule) sim_rule_check(s, "sim_friction");
    sim_realloc(s, m.d, l.total);
    m.h.assign(params, params + l.np);
    sim_ensure(s);
    std::vector<double> h(m.h);
    h.resize(l.total, 0.0);  // (the state rows after a reset: all 0)
    copy_sync(s, m.d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
  })
}

int mpc_sim_friction_read(mpc_solver* s, double* params, double* state) {
  MPC_TRY(s, { sim_model_read(s, "sim_friction_read", s->plant.fr, sim_friction_layout(s->L), params, state); })
}

int mpc_sim_friction_set(mpc_solver* s, const double* state) {
  MPC_TRY(s, {
    const SimLayout l = sim_friction_layout(s->L);
    sim_rows_set(s, "sim_friction_set", s->plant.fr, l, state, -1, [&](const std::string& row, const double* r, int) {
      for (int i = 0; i < 2; ++i) {
        sim_flags_check(row, "sliding", r + SIM_FR_O_SLIDING + i, 1);
        if (r[SIM_FR_O_SLIDING + i] == 0.0 && (r[3 * i] != 0.0 || r[3 * i + 1] != 0.0 || r[3 * i + 2] != 0.0))
          throw std::runtime_error(row + ": sole " + std::to_string(i) + " holds a velocity but its sliding flag is 0");
      }
      sim_nonneg_check(row, "slip_steps, slip_dist, slip_yaw, peak_excess and steps", r + SIM_FR_O_STEPS, (int)l.width - SIM_FR_O_STEPS);
    });
  })
}

int32_t mpc_sim_friction_width(mpc_solver* s) { return sim_width(s, "sim_friction_width", [&] { return MPC_SIM_FRICTION_WIDTH; }); }

// ---- include/mpc_sim_tipping.h: per-robot sole tipping ---------------------------------------------------------------------------------------------
int mpc_sim_tipping(mpc_solver* s, const double* params) {
  MPC_TRY(s, {
    sim_check(s, "sim_tipping");
    const Layout& L = s->L;
    const SimLayout l = sim_tipping_layout(L);
    SimModel& m = s->plant.tip;
    if (!params) { sim_drop(s, m); return 0; }
    for (int b = 0; b < L.B; ++b) {  // (every check before anything changes: a bad row leaves the previous configuration in force; an extent may be +inf)
      const double* r = params + (size_t)b * MPC_SIM_TIPPING_PARAMS;
      const std::string row = "sim_tipping: row " + std::to_string(b);
      for (int e = 0; e < 4; ++e)
        if (std::isnan(r[e]) || r[e] < 0.0)
          throw std::runtime_error(row + ": half_length and half_width must be >= 0 (+inf: the sole never tips on that axis), entry " + std::to_string(e));
      for (int e = 4; e < 7; ++e)
        if (!std::isfinite(r[e]) || !(r[e] > 0.0)) throw std::runtime_error(row + ": I_tip, w_max and th_max must be finite and > 0, entry " + std::to_string(e));
      sim_reserved_check(row, r, 7, MPC_SIM_TIPPING_PARAMS);
    }
    if (m.needs_rule) sim_rule_check(s, "sim_tipping");
    sim_realloc(s, m.d, l.total);
    m.h.assign(params, params + l.np);
    sim_ensure(s);
    std::vector<double> h(m.h);
    h.resize(l.total, 0.0);  // (the state rows after a reset: all 0)
    copy_sync(s, m.d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
  })
}

int mpc_sim_tipping_read(mpc_solver* s, double* params, double* state) {
  MPC_TRY(s, { sim_model_read(s, "sim_tipping_read", s->plant.tip, sim_tipping_layout(s->L), params, state); })
}

int mpc_sim_tipping_set(mpc_solver* s, const double* state) {
  MPC_TRY(s, {
    const SimLayout l = sim_tipping_layout(s->L);
    SimModel& m = s->plant.tip;
    sim_rows_set(s, "sim_tipping_set", m, l, state, -1, [&](const std::string& row, const double* r, int b) {
      const double th_max = m.h[(size_t)b * MPC_SIM_TIPPING_PARAMS + 6];
      for (int i = 0; i < 2; ++i) {
        sim_flags_check(row, "tipping", r + SIM_TP_O_TIPPING + i, 1);
        const double* th = r + SIM_TP_O_TH + 2 * i;
        if (r[SIM_TP_O_TIPPING + i] == 0.0 && (r[3 * i] != 0.0 || r[3 * i + 1] != 0.0 || r[3 * i + 2] != 0.0 || th[0] != 0.0 || th[1] != 0.0))
          throw std::runtime_error(row + ": sole " + std::to_string(i) + " holds a rate or an angle but its tipping flag is 0");
        if (std::fabs(th[0]) > th_max || std::fabs(th[1]) > th_max)
          throw std::runtime_error(row + ": sole " + std::to_string(i) + " holds an angle beyond th_max (" + std::to_string(th_max) + ")");
      }
      sim_nonneg_check(row, "tip_steps, peak_angle, peak_excess, landings and steps", r + SIM_TP_O_STEPS, (int)l.width - SIM_TP_O_STEPS);
    });
  })
}

int32_t mpc_sim_tipping_width(mpc_solver* s) { return sim_width(s, "sim_tipping_width", [&] { return MPC_SIM_TIPPING_WIDTH; }); }

// ---- include/mpc_sim_disturbances.h: per-robot push schedules on any link ----------------------------------------------------------------------
int mpc_sim_disturbances(mpc_solver* s, const double* events, int32_t n_events) {
  MPC_TRY(s, {
    sim_check(s, "sim_disturbances");
    const Layout& L = s->L;
    SimPlant& p = s->plant;
    if (!events) { sim_drop(s, p.dis); return 0; }
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
    if (contact && !p.d_con)
      throw std::runtime_error("sim_disturbances: a contact trigger (2 to 5) needs the contact rule, which is off on this handle (turn it on with mpc_sim_contacts first)");
    if (p.push_width)
      throw std::runtime_error("sim_disturbances: a push is armed on this handle (mpc_sim_set_push): disarm it with mpc_sim_set_push(sim, NULL, 0) before arming a schedule");
    const SimLayout l = sim_disturbances_layout(L, n_events);
    sim_ensure(s);
    {  // (the new buffer before the old one goes: an allocation that fails leaves the table in force as it was)
      void* fresh = nullptr;
      HIP_OK(hipMalloc(&fresh, l.total * sizeof(double)));
      HIP_OK(hipStreamSynchronize(s->stream));
      if (p.dis.d) (void)hipFree(p.dis.d);
      p.dis.d = (double*)fresh;
    }
    p.dis.h.assign(events, events + l.np);
    p.dis_ne = n_events;
    p.dis_contact = contact;
    copy_sync(s, p.dis.d, events, l.np * sizeof(double), hipMemcpyHostToDevice);
    sim_disturbances_reset(s);
  })
}

int mpc_sim_disturbances_read(mpc_solver* s, double* events, double* state, double* applied) {
  MPC_TRY(s, {
    const Layout& L = s->L;
    const SimLayout l = sim_disturbances_layout(s);
    sim_model_read(s, "sim_disturbances_read", s->plant.dis, l, events, state);
    if (applied) {
      std::vector<double> h(l.total - l.out);
      copy_sync(s, h.data(), s->plant.dis.d + l.out, h.size() * sizeof(double), hipMemcpyDeviceToHost);
      const int32_t* link = (const int32_t*)(h.data() + (l.tail - l.out));
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
    sim_on_check(s->plant.dis, "sim_disturbances_reset");
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
