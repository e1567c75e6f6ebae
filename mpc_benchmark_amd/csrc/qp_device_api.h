// qp_device_api.h — what the two translation units of libmpc_hip.so share about a QP handle (qp.hip owns mpc_qp_solver; mpc_hip.hip strings the
// inverse-dynamics QPs between the plan's feedback terms and the simulator step in mpc_qp_low_level_steps, pipeline_glue.h, and
// mpc_qp_ikid_low_level_steps, pipeline_ikid_glue.h; the contact set of those QPs from the simulator's rule, pipeline_contacts.h).  Internal: not part
// of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mpc_qp_pipeline.h"
#include "../../include/mpc_qp_contacts.h"

struct QpIdBuffers {
  hipStream_t stream;
  double *xrob, *acc, *f;   // inputs of the assembly kernel: [B][nq + nv], [B][nv], [B][6 nk]
  int32_t* cs;              // [B][nk]
  double* sol;              // [B][n] = (da, df, tau)
  mpc_qp_info* info;        // [B]
  int B, n, nq, nv, nk, device;
  double* ik;               // [B][2 nv + 42] task errors of the IK + ID QP
  const int32_t* mi;        // model tables (mpc_qp_set_model)
  const double* md;
  int nj;
};
void qp_id_prepare(mpc_qp_solver* s, int32_t nk, const int32_t* frames, const double* weights, const double* cone);  // throws
QpIdBuffers qp_id_buffers(mpc_qp_solver* s);
void qp_id_enqueue(mpc_qp_solver* s, const mpc_qp_settings* S, double kd);   // assembly (+ zeroed start unless warm_start) on the handle's stream
void qp_launch_solve(mpc_qp_solver* s, const mpc_qp_settings* S);            // the solve kernel on the handle's stream
double* qp_scratch(mpc_qp_solver* s, size_t doubles);                         // device scratch owned by the handle
void qp_set_error(mpc_qp_solver* s, const char* what);
// the IK + ID QP (mpc_qp_solve_ikid) for mpc_qp_ikid_low_level_steps
void qp_ikid_prepare(mpc_qp_solver* s, int32_t nk, const int32_t* frames, int32_t base_frame, int32_t torso_frame, const double* weights, const double* gains,
                     const double* cone, const double* l_box, const double* u_box);  // throws
void qp_ikid_enqueue(mpc_qp_solver* s, const mpc_qp_settings* S);            // assembly (+ zeroed start unless warm_start) on the handle's stream
double* qp_ikid_scratch(mpc_qp_solver* s, size_t doubles, bool** kept);       // device scratch of the centroidal loop; *kept: its x_prev holds a measurement
// where the loops' QPs take their contact sets from (mpc_qp_contact_source, include/mpc_qp_contacts.h)
struct QpContactSource {
  int source;             // MPC_QP_CONTACTS_*
  int32_t *sched, *used;  // [B][2] the caller's contact_states ; the set of the last QP          (nullptr while the source is the schedule)
  int32_t* counts;        // [B][2][4]
};
QpContactSource qp_contact_source(mpc_qp_solver* s);
