// cross.hip -- include/ff_hip_cross.h: the elementwise combine of a DCNv2 low-rank cross layer, x_{l+1} = x_0 (.) v_l + x_l, and its backward.
//
// Both entries are one memory-bound pass over [batch][dim] operands with independent row strides (16 batch dim bytes forward, 12 to 32
// batch dim backward): a grid-stride walk of at most 2048 workgroups, every lane moving V = 4 floats (16 bytes) where dim, the strides and
// the base addresses allow it and one float otherwise -- decided on the host, once per launch.  A lane keeps its position as (row, column
// group) and advances it by the grid's stride split the same way, so the loop has no division and row * ld is 64-bit arithmetic.
// Products and sums are fmul_rn / fadd_rn: two roundings, never an fma (the contract is bit for bit a float32 numpy expression).  hipcc
// compiles with -ffp-contract=fast, and HIP's __fmul_rn / __fadd_rn are a plain * and + inside its own header, which the backend fused
// across the inlined calls (v_pk_fma_f32 / v_fmac_f32 in this file's first build).  So mul_rn / add_rn below spell the two operations
// themselves, under `#pragma clang fp contract(off)`: an operation without the contract flag is never fused.
// No pointer is __restrict__: x0 and xl are one buffer in layer 0, and so are dx0 and dxl.
#include "ffh_common.h"

#include "../../include/ff_hip_cross.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;

template <int V> struct Vec;
template <> struct Vec<4> { typedef float4 T; };
template <> struct Vec<1> { typedef float T; };

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float4 mul_rn(float4 a, float4 b) { return make_float4(mul_rn(a.x, b.x), mul_rn(a.y, b.y), mul_rn(a.z, b.z), mul_rn(a.w, b.w)); }
__device__ __forceinline__ float4 add_rn(float4 a, float4 b) { return make_float4(add_rn(a.x, b.x), add_rn(a.y, b.y), add_rn(a.z, b.z), add_rn(a.w, b.w)); }

// the walk: groups of V columns, `groups` per row; (step_r, step_c) = the grid's stride in rows and groups, step_c < groups
struct Walk {
  int64_t batch, groups, step_r, step_c;
};

template <int V>
__global__ __launch_bounds__(kThreads) void cross_fwd_kernel(float* y, int64_t ldy, const float* x0, int64_t ldx0, const float* v, int64_t ldv,
                                                             const float* xl, int64_t ldxl, const Walk w) {
  ffh_kernel_prio();
  typedef typename Vec<V>::T T;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int64_t r = t / w.groups, c = t - r * w.groups;
  while (r < w.batch) {
    const int64_t j = c * V;
    const T a = *reinterpret_cast<const T*>(x0 + r * ldx0 + j);
    const T b = *reinterpret_cast<const T*>(v + r * ldv + j);
    const T x = *reinterpret_cast<const T*>(xl + r * ldxl + j);
    *reinterpret_cast<T*>(y + r * ldy + j) = add_rn(mul_rn(a, b), x);
    r += w.step_r; c += w.step_c;
    if (c >= w.groups) { c -= w.groups; r++; }
  }
}

// SAME: dx0 and dxl are one buffer, written once under mode_x0
template <int V, bool SAME>
__global__ __launch_bounds__(kThreads) void cross_bwd_kernel(const float* dy, int64_t lddy, const float* x0, int64_t ldx0, const float* v, int64_t ldv,
                                                             float* dv, int64_t lddv, float* dx0, int64_t lddx0, int mode_x0, float* dxl, int64_t lddxl,
                                                             int mode_xl, const Walk w) {
  ffh_kernel_prio();
  typedef typename Vec<V>::T T;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int64_t r = t / w.groups, c = t - r * w.groups;
  while (r < w.batch) {
    const int64_t j = c * V;
    const T g = *reinterpret_cast<const T*>(dy + r * lddy + j);
    const T a = *reinterpret_cast<const T*>(x0 + r * ldx0 + j);
    *reinterpret_cast<T*>(dv + r * lddv + j) = mul_rn(g, a);
    if (mode_x0 != FFH_CROSS_SKIP) {      // (the modes are launch arguments: uniform branches)
      T g0 = mul_rn(g, *reinterpret_cast<const T*>(v + r * ldv + j));
      if (SAME) g0 = add_rn(g0, g);
      T* d = reinterpret_cast<T*>(dx0 + r * lddx0 + j);
      *d = mode_x0 == FFH_CROSS_ADD ? add_rn(*d, g0) : g0;
    }
    if (!SAME && mode_xl != FFH_CROSS_SKIP) {
      T* d = reinterpret_cast<T*>(dxl + r * lddxl + j);
      *d = mode_xl == FFH_CROSS_ADD ? add_rn(*d, g) : g;
    }
    r += w.step_r; c += w.step_c;
    if (c >= w.groups) { c -= w.groups; r++; }
  }
}

bool mode_ok(int m) { return m == FFH_CROSS_SKIP || m == FFH_CROSS_STORE || m == FFH_CROSS_ADD; }

// the launch geometry of `batch` rows of `dim` floats moved V at a time
Walk make_walk(int64_t batch, int64_t dim, int V, unsigned* grid) {
  Walk w;
  w.batch = batch;
  w.groups = dim / V;
  *grid = ffh_grid(batch * w.groups, kThreads);
  const int64_t stride = (int64_t)*grid * kThreads;
  w.step_r = stride / w.groups;
  w.step_c = stride % w.groups;
  return w;
}

}  // namespace

extern "C" {

int ffh_cross_abi_version(void) { return FFH_CROSS_ABI_VERSION; }

int ffh_cross_fwd(ffh_ctx* c, float* y, int64_t ldy, const float* x0, int64_t ldx0, const float* v, int64_t ldv, const float* xl, int64_t ldxl,
                  int64_t batch, int64_t dim, ffh_stream s) {
  FFH_REQUIRE(c, batch >= 0 && dim >= 1, "cross_fwd: batch must be >= 0 and dim >= 1");
  FFH_REQUIRE(c, y && x0 && v && xl, "cross_fwd: null operand");
  FFH_REQUIRE(c, ldy >= dim && ldx0 >= dim && ldv >= dim && ldxl >= dim, "cross_fwd: a row stride is smaller than dim");
  const uintptr_t addr = (uintptr_t)y | (uintptr_t)x0 | (uintptr_t)v | (uintptr_t)xl;
  FFH_REQUIRE(c, (addr & 3) == 0, "cross_fwd: operands must be 4-byte aligned");
  if (batch == 0) return FFH_OK;
  const bool v4 = (addr & 15) == 0 && ((dim | ldy | ldx0 | ldv | ldxl) & 3) == 0;
  unsigned grid;
  const Walk w = make_walk(batch, dim, v4 ? 4 : 1, &grid);
  if (v4) hipLaunchKernelGGL((cross_fwd_kernel<4>), dim3(grid), dim3(kThreads), 0, as_stream(s), y, ldy, x0, ldx0, v, ldv, xl, ldxl, w);
  else hipLaunchKernelGGL((cross_fwd_kernel<1>), dim3(grid), dim3(kThreads), 0, as_stream(s), y, ldy, x0, ldx0, v, ldv, xl, ldxl, w);
  FFH_LAUNCH_CHECK(c, "cross_fwd");
  return FFH_OK;
}

int ffh_cross_bwd(ffh_ctx* c, const float* dy, int64_t lddy, const float* x0, int64_t ldx0, const float* v, int64_t ldv, float* dv, int64_t lddv,
                  float* dx0, int64_t lddx0, int mode_x0, float* dxl, int64_t lddxl, int mode_xl, int64_t batch, int64_t dim, ffh_stream s) {
  FFH_REQUIRE(c, batch >= 0 && dim >= 1, "cross_bwd: batch must be >= 0 and dim >= 1");
  FFH_REQUIRE(c, mode_ok(mode_x0) && mode_ok(mode_xl), "cross_bwd: a mode is none of FFH_CROSS_SKIP / _STORE / _ADD");
  FFH_REQUIRE(c, dy && x0 && v && dv, "cross_bwd: null operand");
  FFH_REQUIRE(c, (dx0 || mode_x0 == FFH_CROSS_SKIP) && (dxl || mode_xl == FFH_CROSS_SKIP), "cross_bwd: a destination that is not skipped is null");
  const bool use_x0 = mode_x0 != FFH_CROSS_SKIP, use_xl = mode_xl != FFH_CROSS_SKIP;
  const bool same = use_x0 && use_xl && dx0 == dxl;
  FFH_REQUIRE(c, !same || (mode_x0 == mode_xl && lddx0 == lddxl), "cross_bwd: dx0 == dxl needs mode_xl == mode_x0 (and one row stride)");
  FFH_REQUIRE(c, !(dx0 && dx0 == dxl) || same, "cross_bwd: dx0 == dxl needs mode_xl == mode_x0, neither of them FFH_CROSS_SKIP");
  FFH_REQUIRE(c, lddy >= dim && ldx0 >= dim && ldv >= dim && lddv >= dim && (!use_x0 || lddx0 >= dim) && (!use_xl || lddxl >= dim),
              "cross_bwd: a row stride is smaller than dim");
  uintptr_t addr = (uintptr_t)dy | (uintptr_t)x0 | (uintptr_t)v | (uintptr_t)dv;
  int64_t lds = dim | lddy | ldx0 | ldv | lddv;
  if (use_x0) { addr |= (uintptr_t)dx0; lds |= lddx0; }
  if (use_xl) { addr |= (uintptr_t)dxl; lds |= lddxl; }
  FFH_REQUIRE(c, (addr & 3) == 0, "cross_bwd: operands must be 4-byte aligned");
  if (batch == 0) return FFH_OK;
  const bool v4 = (addr & 15) == 0 && (lds & 3) == 0;
  unsigned grid;
  const Walk w = make_walk(batch, dim, v4 ? 4 : 1, &grid);
#define FFH_CROSS_BWD(V, SAME)                                                                                                                  \
  hipLaunchKernelGGL((cross_bwd_kernel<V, SAME>), dim3(grid), dim3(kThreads), 0, as_stream(s), dy, lddy, x0, ldx0, v, ldv, dv, lddv, dx0, lddx0, \
                     mode_x0, dxl, lddxl, mode_xl, w)
  if (v4 && same) FFH_CROSS_BWD(4, true);
  else if (v4) FFH_CROSS_BWD(4, false);
  else if (same) FFH_CROSS_BWD(1, true);
  else FFH_CROSS_BWD(1, false);
#undef FFH_CROSS_BWD
  FFH_LAUNCH_CHECK(c, "cross_bwd");
  return FFH_OK;
}

}  // extern "C"
