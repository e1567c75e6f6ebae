/*
 * mpc_sim_plant.h — HIP-library-only addition to the C-ABI of include/mpc_abi.h: per-robot plant inertias in the torque-driven simulator.  With the
 * model on, every simulator step of the handle (mpc_simulate_torque, and the simulator step inside mpc_qp_low_level_steps,
 * mpc_qp_ikid_low_level_steps and mpc_feedback_low_level_steps) integrates robot b with its OWN model table: the table of mpc_set_model with the
 * link masses, centres of mass and rotational inertias rewritten by robot b's parameter row (a payload, a mass error, a displaced centre of
 * mass).  With it off nothing is allocated, nothing is launched and every step is what it was.
 *
 * The rule is defined by its numpy mirror, mpc_benchmark_amd/plant_model.py: the definition the checks hold the kernel (csrc/sim_plant.h) to.
 * mpc_abi.h lists what BOTH libraries export (tests/test_abi_library.py); the entry points here are exported by libmpc_hip.so alone.  Bindings look
 * the symbols up before they use them (mpc_benchmark_amd/_capi.py).
 *
 * Every call takes the simulator handle of mpc_simulate_torque (whole-body, nu = nv - 6).  The calls return 0, or -1 with the reason in
 * mpc_last_error (mpc_sim_plant_width: the width, or -1).
 *
 * Who reads which table while the model is on:
 *   - the dynamics of the step (the stage kernel's simulator instantiation), the centre of mass and centroidal momentum of the record
 *     (mpc_sim_record) and with them the metrics (mpc_sim_metrics): robot b's own table, the TRUE plant;
 *   - the contact rule, the base-state estimator, the foot sensors, the walk generators, the low-level QPs, the glue kernels of the pipelines and
 *     every MPC handle: the nominal table of mpc_set_model.  They need kinematics only (which the model never touches), or they are what the
 *     controllers believe;
 *   - the feedback-law simulators mpc_simulate and mpc_simulate_push do not see the model.
 * The tables are built when the model is armed and when mpc_set_model is called on an armed handle; nothing is launched per step.
 */
#ifndef MPC_SIM_PLANT_H
#define MPC_SIM_PLANT_H

#include "mpc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One parameter row of MPC_SIM_PLANT_PARAMS doubles per robot; "table joint index": the joint index of the model tables (0 is the base):
 *   0      mass_scale      every link's mass and I_com multiplied by it: finite, > 0 (1: nominal)
 *   1      inertia_scale   every link's I_com multiplied by it once more: finite, > 0 (1: nominal)
 *   2      shift_body      table joint index whose centre of mass is displaced: an integer value in [0, njoints)
 *   3-5    com_shift       added to that link's lever, in the joint frame, in metres
 *   6      payload_body    table joint index carrying a point mass: an integer value in [0, njoints)
 *   7      payload_mass    kg, >= 0 (0: none)
 *   8-10   payload_point   where the point mass sits, in the joint frame
 *   11-15  reserved        0
 * link_scale[B][njoints] (optional): link j's mass and I_com multiplied by its entry, finite and > 0.
 * Per link, in this order, every step a branch on its parameter (m, c, I: mass, lever, I_com):
 *   mass_scale != 1: m, I *= mass_scale;  inertia_scale != 1: I *= inertia_scale;  link_scale[j] != 1: m, I *= link_scale[j];
 *   j == shift_body and com_shift != 0: c += com_shift;
 *   j == payload_body and payload_mass > 0: m' = m + m_p, c' = (m c + m_p r) / m', I' = I + m (|d|^2 1 - d d^T) + m_p (|e|^2 1 - e e^T) with
 *   d = c - c', e = r - c' (the parallel-axis rule).
 * The identity row (1, 1, 0, ...) without link_scale, or with ones, leaves the nominal entries bit for bit.  Joint placements, frames, contact
 * placements and gains, gravity and prox_mu are never touched. */
#define MPC_SIM_PLANT_PARAMS 16

/* params[B][16], link_scale[B][njoints] or NULL.  params == NULL: off (frees everything).  Validation as in the table, before anything changes: a
 * bad row fails the call and leaves the previous configuration in force; a model must have been set (mpc_set_model).  Then every robot's table is
 * built on the device.  mpc_set_model on an armed handle rebuilds the tables from the rows in force when the joint count is unchanged (a contact
 * frame lowered again after a catch); with another joint count mpc_set_model fails before it changes anything. */
int mpc_sim_plant(mpc_solver* sim, const double* params, const double* link_scale);

/* The rows in force to params[B][16] and link_scale[B][njoints] (ones when none was given), the built tables to tables[B][nd]; any pointer may be
 * NULL.  Synchronises the handle's stream.  Fails while the model is off. */
int mpc_sim_plant_read(mpc_solver* sim, double* params, double* link_scale, double* tables);

/* nd, the doubles of the handle's model table (one robot's row of `tables`); -1: not a simulator handle, or no model set */
int32_t mpc_sim_plant_width(mpc_solver* sim);

#ifdef __cplusplus
}
#endif
#endif
