// mfma_blocks_probe.hip — test infrastructure, not product: one thin __global__ wrapper per routine of mfma_blocks.h, so that
// tests/test_gpu_mfma_blocks.py can hold every routine to an exact or a high-precision reference by name.
//
// Every wrapper does the same thing.  A case is one flat image of the LDS (`words` doubles) that the test lays out: one workgroup per
// case (blockIdx.x = case index) copies its image from global memory into dynamic LDS, calls ONE routine on operands at the offsets
// the launch names, and copies the WHOLE image back out together with the returned flag — so every cell a routine may touch, the
// padding columns of a leading dimension included, comes back, and nothing outside the image is ever addressed.  The launch shapes
// are the callers': 64 threads for the one-wavefront routines, 512 for the workgroup forms and the solves dealt over wavefronts.
//
// The form of chol16_wave is chosen by macros, so this file is built more than once (Makefile): the default build is the left-looking
// inverse of mpc_hip.hip, -DCHOL16_RIGHT_LOOKING the build of eval_multibody.hip, -DCHOL16_FUSED the one-pass form.
#include <hip/hip_runtime.h>
#include "../../mpc_benchmark_amd/csrc/mfma_blocks.h"

enum ProbeOp {
  OP_MMA_TILE = 0,        // p: neg, A, a_is, a_ks, B, b_ks, b_js, K, C, ldc
  OP_MMA_TILE2 = 1,       // p: A0, A1, a_is, a_ks, B, b_ks, b_js, K, C0, C1, ldc
  OP_MMA_TILE_2A = 2,     // p: A0, a0_is, a0_ks, A1, a1_is, a1_ks, B, b_ks, b_js, K, C0, C1, ldc
  OP_MMA_TILE_RB = 3,     // p: neg, A, a_is, a_ks, B, ldb, C, ldc
  OP_CHOL16 = 4,          // p: D, ld, LIb, ncols                 chol16_wave(D, ld, LIb, lane, ncols)
  OP_CHOL16_MFMA = 5,     // p: D, ld, LIb, ncols                 chol16_wave_mfma
  OP_CHOL16_N4 = 6,       // p: D, ld, LIb                        chol16_wave_n<4>
  OP_CHOL16_N6 = 7,
  OP_CHOL16_N8 = 8,
  OP_CHOL16_N12 = 9,
  OP_CHOL16_NC = 10,      // p: D, ld, LIb, ncols                 chol16_wave_nc
  OP_CHOL_BLOCKED_WAVE = 11,  // p: A, ld, nb, LI, n_real
  OP_CHOL_BLOCKED = 12,       // p: A, ld, nb, LI
  OP_CHOL_TILES_WAVE = 13,    // p: T, nb
  OP_CHOL_TILES = 14,         // p: T, nb
  OP_CHOL_TILES_LAST6 = 15,   // p: T, nb     the stage kernel's composition: chol16_wave_n<NLAST> on the last diagonal tile
  OP_CHOL_TILES_LAST12 = 16,
  OP_TRSM_FWD_BLOCKED = 17,   // p: L, ld, LI, nb, B, ldb, ncb     (wv, nw from the launch: 512 threads = 8 wavefronts, 64 = one)
  OP_TRSM_BWD_BLOCKED = 18,
  OP_TRSM_FWD_TILES = 19,     // p: T, nb, B, ldb, ncb
  OP_TRSM_BWD_TILES = 20,
  OP_COUNT = 21
};

struct ProbeArgs { int words; int p[15]; };

// eval_multibody.h's chol_tiles_wave_last, restated (that header cannot be included alone): chol_tiles_wave with NLAST real columns
// in the last diagonal tile
template <int NLAST> DEV bool probe_chol_tiles_wave_last(double* T, int nb, int lane) {
  bool ok = true;
  for (int kb = 0; kb < nb && ok; ++kb) {
    double* Dk = ptile(T, kb, kb);
    ok = (kb == nb - 1) ? chol16_wave_n<NLAST>(Dk, 17, Dk, lane) : chol16_wave(Dk, 17, Dk, lane);
    for (int ri = kb + 1; ri < nb; ++ri) {
      double* Pt = ptile(T, ri, kb);
      d4_t acc = d4_t{0, 0, 0, 0};
      mma_tile<false>(acc, Pt, 17, 1, Dk, 1, 17, 16, lane);
      tile_store(Pt, 17, acc, lane);
    }
    for (int ri = kb + 1; ri < nb; ++ri)
      for (int cj = kb + 1; cj <= ri; ++cj) {
        double* Ct = ptile(T, ri, cj);
        d4_t acc = tile_load(Ct, 17, lane);
        mma_tile<true>(acc, ptile(T, ri, kb), 17, 1, ptile(T, cj, kb), 1, 17, 16, lane);
        tile_store(Ct, 17, acc, lane);
      }
  }
  return ok;
}

template <int OP, int THREADS>
__global__ void __launch_bounds__(THREADS) k_probe(ProbeArgs a, const double* __restrict__ in, double* __restrict__ out, int* __restrict__ flags) {
  extern __shared__ double lds[];
  __shared__ int iflag;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
  const double* src = in + (size_t)blockIdx.x * a.words;
  double* dst = out + (size_t)blockIdx.x * a.words;
  for (int i = tid; i < a.words; i += blockDim.x) lds[i] = src[i];
  __syncthreads();
  const int* p = a.p;
  bool ok = true;
  if constexpr (OP == OP_MMA_TILE) {
    d4_t acc = tile_load(lds + p[8], p[9], lane);
    if (p[0]) mma_tile<true>(acc, lds + p[1], p[2], p[3], lds + p[4], p[5], p[6], p[7], lane);
    else mma_tile<false>(acc, lds + p[1], p[2], p[3], lds + p[4], p[5], p[6], p[7], lane);
    tile_store(lds + p[8], p[9], acc, lane);
  } else if constexpr (OP == OP_MMA_TILE2) {
    d4_t acc0 = tile_load(lds + p[8], p[10], lane), acc1 = tile_load(lds + p[9], p[10], lane);
    mma_tile2(acc0, acc1, lds + p[0], lds + p[1], p[2], p[3], lds + p[4], p[5], p[6], p[7], lane);
    tile_store(lds + p[8], p[10], acc0, lane);
    tile_store(lds + p[9], p[10], acc1, lane);
  } else if constexpr (OP == OP_MMA_TILE_2A) {
    d4_t acc0 = tile_load(lds + p[10], p[12], lane), acc1 = tile_load(lds + p[11], p[12], lane);
    mma_tile_2a(acc0, acc1, lds + p[0], p[1], p[2], lds + p[3], p[4], p[5], lds + p[6], p[7], p[8], p[9], lane);
    tile_store(lds + p[10], p[12], acc0, lane);
    tile_store(lds + p[11], p[12], acc1, lane);
  } else if constexpr (OP == OP_MMA_TILE_RB) {
    const d4_t b = tile_load(lds + p[4], p[5], lane);
    d4_t acc = tile_load(lds + p[6], p[7], lane);
    if (p[0]) mma_tile_rb<true>(acc, lds + p[1], p[2], p[3], b, lane);
    else mma_tile_rb<false>(acc, lds + p[1], p[2], p[3], b, lane);
    tile_store(lds + p[6], p[7], acc, lane);
  } else if constexpr (OP == OP_CHOL16) {
    ok = chol16_wave(lds + p[0], p[1], lds + p[2], lane, p[3]);
  } else if constexpr (OP == OP_CHOL16_MFMA) {
    ok = chol16_wave_mfma(lds + p[0], p[1], lds + p[2], lane, p[3]);
  } else if constexpr (OP == OP_CHOL16_N4) {
    ok = chol16_wave_n<4>(lds + p[0], p[1], lds + p[2], lane);
  } else if constexpr (OP == OP_CHOL16_N6) {
    ok = chol16_wave_n<6>(lds + p[0], p[1], lds + p[2], lane);
  } else if constexpr (OP == OP_CHOL16_N8) {
    ok = chol16_wave_n<8>(lds + p[0], p[1], lds + p[2], lane);
  } else if constexpr (OP == OP_CHOL16_N12) {
    ok = chol16_wave_n<12>(lds + p[0], p[1], lds + p[2], lane);
  } else if constexpr (OP == OP_CHOL16_NC) {
    ok = chol16_wave_nc(lds + p[0], p[1], lds + p[2], lane, p[3]);
  } else if constexpr (OP == OP_CHOL_BLOCKED_WAVE) {
    ok = chol_blocked_wave(lds + p[0], p[1], p[2], lds + p[3], lane, p[4]);
  } else if constexpr (OP == OP_CHOL_BLOCKED) {
    ok = chol_blocked(lds + p[0], p[1], p[2], lds + p[3], tid, &iflag);
  } else if constexpr (OP == OP_CHOL_TILES_WAVE) {
    ok = chol_tiles_wave(lds + p[0], p[1], lane);
  } else if constexpr (OP == OP_CHOL_TILES) {
    ok = chol_tiles(lds + p[0], p[1], tid, &iflag);
  } else if constexpr (OP == OP_CHOL_TILES_LAST6) {
    ok = probe_chol_tiles_wave_last<6>(lds + p[0], p[1], lane);
  } else if constexpr (OP == OP_CHOL_TILES_LAST12) {
    ok = probe_chol_tiles_wave_last<12>(lds + p[0], p[1], lane);
  } else if constexpr (OP == OP_TRSM_FWD_BLOCKED) {
    trsm_fwd_blocked(lds + p[0], p[1], lds + p[2], p[3], lds + p[4], p[5], p[6], wv, nw, lane);
  } else if constexpr (OP == OP_TRSM_BWD_BLOCKED) {
    trsm_bwd_blocked(lds + p[0], p[1], lds + p[2], p[3], lds + p[4], p[5], p[6], wv, nw, lane);
  } else if constexpr (OP == OP_TRSM_FWD_TILES) {
    trsm_fwd_tiles(lds + p[0], p[1], lds + p[2], p[3], p[4], wv, nw, lane);
  } else if constexpr (OP == OP_TRSM_BWD_TILES) {
    trsm_bwd_tiles(lds + p[0], p[1], lds + p[2], p[3], p[4], wv, nw, lane);
  }
  __syncthreads();
  for (int i = tid; i < a.words; i += blockDim.x) dst[i] = lds[i];
  if (tid == 0) flags[blockIdx.x] = ok ? 1 : 0;
}

__global__ void k_rsqrt(int n, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = rsqrt_refined(in[i]);
}

namespace {
constexpr size_t kMaxLdsBytes = 160 * 1024 - 64;  // the CU's LDS less the static flag word (and its alignment)

template <int OP, int THREADS>
hipError_t launch(const ProbeArgs& a, int ncases, size_t bytes, const double* din, double* dout, int* dflags) {
  if (bytes > 64 * 1024) {  // (as create_impl does for the product kernels)
    hipError_t e = hipFuncSetAttribute((const void*)k_probe<OP, THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_probe<OP, THREADS>), dim3(ncases), dim3(THREADS), bytes, 0, a, din, dout, dflags);
  return hipGetLastError();
}

hipError_t dispatch(int op, int threads, const ProbeArgs& a, int ncases, size_t bytes, const double* din, double* dout, int* dflags) {
#define ONE_WAVE(OP) case OP: return threads == 64 ? launch<OP, 64>(a, ncases, bytes, din, dout, dflags) : hipErrorInvalidValue;
#define WORKGROUP(OP) case OP: return threads == 512 ? launch<OP, 512>(a, ncases, bytes, din, dout, dflags) : hipErrorInvalidValue;
#define EITHER(OP) case OP: return threads == 512 ? launch<OP, 512>(a, ncases, bytes, din, dout, dflags) \
                                 : threads == 64 ? launch<OP, 64>(a, ncases, bytes, din, dout, dflags) : hipErrorInvalidValue;
  switch (op) {
    ONE_WAVE(OP_MMA_TILE) ONE_WAVE(OP_MMA_TILE2) ONE_WAVE(OP_MMA_TILE_2A) ONE_WAVE(OP_MMA_TILE_RB)
    ONE_WAVE(OP_CHOL16) ONE_WAVE(OP_CHOL16_MFMA) ONE_WAVE(OP_CHOL16_N4) ONE_WAVE(OP_CHOL16_N6) ONE_WAVE(OP_CHOL16_N8)
    ONE_WAVE(OP_CHOL16_N12) ONE_WAVE(OP_CHOL16_NC)
    ONE_WAVE(OP_CHOL_BLOCKED_WAVE) WORKGROUP(OP_CHOL_BLOCKED) ONE_WAVE(OP_CHOL_TILES_WAVE) WORKGROUP(OP_CHOL_TILES)
    ONE_WAVE(OP_CHOL_TILES_LAST6) ONE_WAVE(OP_CHOL_TILES_LAST12)
    EITHER(OP_TRSM_FWD_BLOCKED) EITHER(OP_TRSM_BWD_BLOCKED) EITHER(OP_TRSM_FWD_TILES) EITHER(OP_TRSM_BWD_TILES)
    default: return hipErrorInvalidValue;
  }
#undef ONE_WAVE
#undef WORKGROUP
#undef EITHER
}
}  // namespace

// Host entry points: host pointers in and out; hipMalloc, copy, ONE launch, hipDeviceSynchronize, copy back, free.  -> hipError_t
extern "C" int mfma_probe_run(int op, int threads, int ncases, int words, const int* params, int nparams, const double* in, double* out, int* flags) {
  if (ncases < 1 || ncases > 65535 || words < 1 || nparams < 0 || nparams > 15) return (int)hipErrorInvalidValue;
  const size_t bytes = (size_t)words * sizeof(double);
  if (bytes > kMaxLdsBytes) return (int)hipErrorInvalidValue;
  ProbeArgs a;
  a.words = words;
  for (int i = 0; i < 15; ++i) a.p[i] = i < nparams ? params[i] : 0;
  const size_t total = bytes * (size_t)ncases;
  double *din = nullptr, *dout = nullptr;
  int* dflags = nullptr;
  hipError_t e = hipMalloc(&din, total);
  if (e == hipSuccess) e = hipMalloc(&dout, total);
  if (e == hipSuccess) e = hipMalloc(&dflags, sizeof(int) * (size_t)ncases);
  if (e == hipSuccess) e = hipMemcpy(din, in, total, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dflags, 0xff, sizeof(int) * (size_t)ncases);
  if (e == hipSuccess) e = dispatch(op, threads, a, ncases, bytes, din, dout, dflags);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, total, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(flags, dflags, sizeof(int) * (size_t)ncases, hipMemcpyDeviceToHost);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  if (dflags) (void)hipFree(dflags);
  return (int)e;
}

extern "C" int mfma_probe_rsqrt(int n, const double* in, double* out) {
  if (n < 1) return (int)hipErrorInvalidValue;
  double *din = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&din, sizeof(double) * (size_t)n);
  if (e == hipSuccess) e = hipMalloc(&dout, sizeof(double) * (size_t)n);
  if (e == hipSuccess) e = hipMemcpy(din, in, sizeof(double) * (size_t)n, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_rsqrt, dim3((n + 255) / 256), dim3(256), 0, 0, n, din, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return (int)e;
}

// which form of chol16_wave this build holds
extern "C" const char* mfma_probe_form() {
#if defined(CHOL16_FUSED)
  return "fused";
#elif defined(CHOL16_RIGHT_LOOKING)
  return "right-looking";
#else
  return "left-looking";
#endif
}
extern "C" const char* mfma_probe_error_string(int e) { return hipGetErrorString((hipError_t)e); }
