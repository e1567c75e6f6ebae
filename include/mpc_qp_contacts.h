/*
 * mpc_qp_contacts.h — HIP-library-only addition to the C-ABI of include/mpc_qp_abi.h: where the low-level QPs of the two device loops
 * (mpc_qp_low_level_steps, include/mpc_qp_abi.h; mpc_qp_ikid_low_level_steps, include/mpc_qp_pipeline.h) take every robot's contact set from.
 *
 * By default each QP of a loop call works with the caller's contact_states[B][nk] (the schedule: what the plan's stage says), whatever the plant
 * does.  On a simulator handle with the unilateral contact rule on (mpc_sim_contacts, include/mpc_sim_contacts.h) the plant decides every robot's
 * foot contacts on the device after every step; with a source other than the schedule each robot's QP takes its contact set from its own row of
 * that rule, step by step, on the device, with no host round trip inside the call.  The numpy mirror, the definition the checks hold the kernel to, is
 * mpc_benchmark_amd/contact_rule.py (QP_SOURCES, qp_contact_states, qp_contact_counts).  mpc_qp_abi.h lists what BOTH libraries export
 * (tests/test_abi_library.py); the entry points here are exported by libmpc_hip.so alone.  Bindings look the symbols up before they use them
 * (mpc_benchmark_amd/_qp_capi.py).
 *
 * Per robot, with s = the caller's contact_states pair and p = doubles 0 and 1 (in_contact) of the robot's row of the rule:
 *   MPC_QP_CONTACTS_SCHEDULE   used = s
 *   MPC_QP_CONTACTS_PLANT      used = p
 *   MPC_QP_CONTACTS_BOTH       used = s & p ; a robot for which that is empty takes p (the rule never releases the last contact, so p holds one)
 * The QP of step k reads the rows as they stand BEFORE step k: the state the rule left after step k - 1, which is the state the QP is solved at.  The
 * first step of a call reads the rows the previous call, mpc_sim_contacts or mpc_sim_contacts_set left.  With a source other than the schedule the
 * six `forces` components (forces + df) of a contact the QP did not use are returned as 0, and every step counts counts[b][c][2 s + p] += 1 for
 * both contacts c: how often plan and plant agreed (indices 0, 3) and disagreed (1: the plant holds a foot the plan has in the air; 2: the plan stands
 * on a foot the plant has released).
 *
 * The calls return 0, or -1 with the reason in mpc_qp_last_error.
 */
#ifndef MPC_QP_CONTACTS_H
#define MPC_QP_CONTACTS_H

#include "mpc_qp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPC_QP_CONTACTS_SCHEDULE 0
#define MPC_QP_CONTACTS_PLANT    1
#define MPC_QP_CONTACTS_BOTH     2

/* Sticky on the QP handle: the source of every later loop call.  Zeroes the counts.  -1 on an unknown value (the source stays what it was).
 * With MPC_QP_CONTACTS_SCHEDULE the two loops enqueue exactly what they enqueue on a handle that never saw this call.  With another source they
 * need the rule on their simulator handle (mpc_sim_contacts) and nk = 2 (the two soles), and fail otherwise. */
int mpc_qp_contact_source(mpc_qp_solver* s, int32_t source);

/* Any pointer may be NULL.  source: the value in force.  used[B][2]: the contact set of the last QP of the last loop call (with
 * MPC_QP_CONTACTS_SCHEDULE: the contact_states the handle's last QP was given; zeros before any).  counts[B][2][4]: as above, since the last
 * mpc_qp_contact_source (zeros while the source is the schedule: nothing is read from the plant then).  Synchronises the handle's stream. */
int mpc_qp_contact_source_read(mpc_qp_solver* s, int32_t* source, int32_t* used, int32_t* counts);

#ifdef __cplusplus
}
#endif
#endif
