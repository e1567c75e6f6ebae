// plan_view.h — where the plan of an MPC handle lives on the device, for the kernels that read one knot of it: the feedback kernels of the three
// device loops (pipeline_*glue.h) and the publication of the held record (plan_latency.h).  What they read of a knot is its record: state, control,
// Riccati gain and six entries of xdot out of the knot's stage data.  The host fills the view from a handle in one place (pipeline_loops.h plan_view).
#pragma once
#include <hip/hip_runtime.h>

struct PlanView {
  const double *xs, *us, *gains, *knots;  // [B][N + 1][nx], [B][N][m], [B][N + 1][gain_stride], [B][N + 1][knot_stride]
  int N, nx, n, m;                        // horizon ; state, tangent and control dimensions
  int gain_stride, oK;                    // K (m x n, row-major) inside a knot's gain block
  int knot_stride, oXD;                   // xdot inside a knot's stage data
  int xd_off;                             // first of the six entries of xdot the pipelines read: n / 2 (multibody: the base acceleration), 3 (centroidal: dH)
  int slot0;                              // ring slot of knot 0's stage data (knot k: (slot0 + k) % N)
};

// One record of a plan, in the buffers or held by value (plan_latency.h): x [nx], u [m], K [m][n] row-major, xd [6].
template <class T> struct PlanRecordOf { T *x, *u, *K, *xd; };
using PlanRecord = PlanRecordOf<const double>;

// doubles from one robot's gain blocks to the next robot's
static inline __host__ __device__ size_t plan_gain_pitch(int N, int gain_stride) { return (size_t)(N + 1) * gain_stride; }

// knot k of robot b ; slot: the ring slot of that knot's stage data
__device__ __forceinline__ PlanRecord plan_knot(const PlanView& v, int b, int k, int slot) {
  PlanRecord r;
  r.x = v.xs + ((size_t)b * (v.N + 1) + k) * v.nx;
  r.u = v.us + ((size_t)b * v.N + k) * v.m;
  r.K = v.gains + (size_t)b * plan_gain_pitch(v.N, v.gain_stride) + (size_t)k * v.gain_stride + v.oK;
  r.xd = v.knots + ((size_t)b * (v.N + 1) + slot) * v.knot_stride + v.oXD + v.xd_off;
  return r;
}
