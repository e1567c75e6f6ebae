/*
 * mpc_plan_latency.h — HIP-library-only addition to the C-ABI of include/mpc_abi.h: a hand-over latency per robot for the plan in the three device
 * control loops (mpc_qp_low_level_steps and mpc_qp_ikid_low_level_steps of include/mpc_qp_abi.h, mpc_feedback_low_level_steps of
 * include/mpc_feedback_pipeline.h).
 *
 * mpc_abi.h lists what BOTH libraries export (tests/test_abi_library.py); the entry points here are exported by libmpc_hip.so alone.  Their checker
 * side is host glue built from calls both libraries have (mpc_get_results, mpc_get_gain, mpc_get_stage_data) around the numpy mirror that defines
 * the model (mpc_benchmark_amd/plan_latency.py; the pipelines' tick(host_glue=True) in mpc_benchmark_amd/pipeline.py).  Bindings look the symbols up
 * before they use them (mpc_benchmark_amd/_capi.py).
 */
#ifndef MPC_PLAN_LATENCY_H
#define MPC_PLAN_LATENCY_H

#include "mpc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Without the model every robot follows knot 0 of a new plan from the first low-level step after the solve: the plan arrives instantly.  With it
 * robot b keeps running the plan it already has for its first L_b low-level steps after a new plan is published.  The plan it already has is knot 1
 * of the OUTGOING plan, which covers the same period as knot 0 of the new one; mpc_plan_latency_publish copies it by value into the robot's HELD
 * record.  After those steps the robot follows knot 0 of the new plan as without the model.
 *
 *   - L_b = 0 is the loop without the model, bit for bit.
 *   - A latency longer than a period acts as one period: at the next publication the held record becomes knot 1 of the then-outgoing plan and the
 *     countdown starts again for every robot, whether or not it had handed over.  Nothing is refused for it.
 *   - The countdown lives on the device and is advanced by the loops' own kernels, one per low-level step: a period split over two calls of a loop
 *     (3 + 7 steps) is one call of 10.
 *   - While the model is off the loops launch the kernels they launch without it and nothing of it is allocated.
 *
 * params[B][4], one row per robot: steps | jitter | seed | reserved (0).  steps and jitter are integer-valued in 0 .. MPC_PLAN_LATENCY_MAX_STEPS,
 * seed in 0 .. 2^32 - 1.  At a publication the robot's count `plans` goes up by one and
 *     L_b = steps + min(floor(u (jitter + 1)), jitter),
 * u the first uniform of the Philox4x32-10 block of counter (plans mod 2^32, plans / 2^32, 0, 0) and key (seed, 0) — the generator of the sensor
 * model (include/mpc_sim_sensors.h), u = ((w1 << 20 | w0 >> 12) + 0.5) 2^-52.  A robot's draws depend on its row and its count only, never on its
 * place in the batch.
 *
 * state[B][8], one row per robot, every entry integer-valued: remaining (steps the robot still runs the held record for) | drawn (L_b of the last
 * publication) | plans (publications so far) | late_steps (low-level steps run on a held record) | steps_total (low-level steps) | max_drawn |
 * held_valid (1 once a publication took a record) | reserved (0).  A robot reads the held record on a step when remaining > 0 and held_valid; then
 * remaining goes down and late_steps up by one; steps_total goes up either way.  The task errors of the centroidal loop, computed once per call, take
 * the record the robot's first step of that call uses and count nothing.
 *
 * held[B][MPC_PLAN_LATENCY_HELD(nx, n, m)], one record per robot, nx / n / m the plan's state, tangent and control dimensions:
 *     xs[1] (nx) | us[1] (m) | K_1 (m x n, row-major, as mpc_get_gain) | the part of knot 1's xdot (mpc_get_stage_data) the loops read (6):
 *     xdot[n/2 .. n/2 + 6) of a multibody plan (the base acceleration), xdot[3 .. 9) of a vector-space plan (the rate of the centroidal momentum).
 *
 * mpc_set_state on an armed handle sets remaining to 0 and invalidates the held record of every robot: a restored checkpoint is followed at once.
 * The parameters, the counters and the held records are not part of mpc_get_state. */
#define MPC_PLAN_LATENCY_PARAMS 4
#define MPC_PLAN_LATENCY_STATE 8
#define MPC_PLAN_LATENCY_MAX_STEPS 1000
#define MPC_PLAN_LATENCY_XDOT 6
#define MPC_PLAN_LATENCY_HELD(nx, n, m) ((nx) + (m) + (m) * (n) + MPC_PLAN_LATENCY_XDOT)

/* Arm and reset: remaining = 0, no held record, counters 0.  params = NULL turns the model off and frees everything it allocated.  Every check is
 * made before anything changes (finite values, integer values, ranges, a reserved entry of 0, a horizon of at least 2 knots, no ticks in flight): a
 * refused call leaves the model as it was. */
int mpc_plan_latency(mpc_solver* plan, const double* params);

/* A publication: called while the OUTGOING plan is still in the handle's buffers, before the run that replaces it (and after the low-level loop of
 * the period: the loops' slot rule for the stage data still holds for the outgoing plan).  One kernel, one workgroup per robot, takes the held
 * record from knot 1, draws L_b and sets remaining = drawn = L_b.  Refused when the model is not armed, with ticks in flight, and on a handle that
 * has never run; a refused call changes nothing. */
int mpc_plan_latency_publish(mpc_solver* plan);

/* The model as it stands; each output may be NULL.  Refused when the model is not armed. */
int mpc_plan_latency_read(mpc_solver* plan, double* params, double* state, double* held);

#ifdef __cplusplus
}
#endif
#endif
