// linear_q8.hip -- Linear layers on the int8 matrix pipe for held-out evaluation (include/ffh_q8_linear.h).
//
// Two kernels.  The rule they compute -- symmetric codes with a scale per row, an exact int32 sum, three fp32 operations each rounded on its
// own -- is stated in the header; nothing here is contracted into a fused multiply-add (the pragma below).
//
//   q8l_quantize_kernel<G>   fp32 rows -> int8 image rows + a scale per row; the weights of every layer of a call, or the activations of one
//     layer, in one grid-capped, grid-stride launch.  G lanes (a power of two, 4 .. 64) own a row, a lane 16 columns per trip: pass 1 takes the
//     row's absmax (4-byte-aligned 16-byte loads, a butterfly of __shfl_xor over the group), pass 2 reads the row again (it is in cache), rounds
//     with v_rndne_f32 and stores 16 codes per lane as one 16-byte store.  Pass 2 runs to the image's padded width, so the pad columns get 0.
//
//   q8l_gemm_kernel<T, VEC>  y = act(acc * (sx * sw) + bias) from the two images.
//     WORK SPLIT.  A 4-wave workgroup owns a 64 T x 64 T tile of y (T = 2: 128 x 128, T = 1: 64 x 64 for outputs with too few big tiles to
//       fill the chip); the waves lie 2 x 2 on it, each with T x T accumulators of v_mfma_i32_32x32x32_i8.  The MFMA's A operand is the WEIGHT
//       fragment and its B operand the ACTIVATION fragment, so the accumulator is a block of y TRANSPOSED: a lane holds, for one sample
//       (lane & 31), four consecutive output columns per register quad -- which is what a 16-byte store of a y row wants.
//     K WALK.  64 bytes of every row per step (two MFMA k-steps of 32); the images are zero-padded to a multiple of 64, so there is no tail.
//       Rows of an edge tile past the matrix are CLAMPED to its last row in the loader (valid addresses, results the epilogue never stores).
//     STAGING.  Both operands go global -> registers -> LDS as 16-byte pieces (a thread moves T pieces of each operand per step: piece
//       tid & 3 of row (tid >> 2) + 64 i, so four lanes read one row's 64 contiguous bytes), double-buffered: the global loads of step t + 1
//       are in flight under the MFMAs of step t, their LDS stores follow the MFMAs, one barrier per step.  LDS: 2 buffers x 2 operands x
//       64 T rows x 64 bytes = 32 KiB (T = 2) or 16 KiB (T = 1).
//     LDS LAYOUT.  An operand image is [row][64 bytes]; the four 16-byte chunks of a row are XOR-swizzled by row:
//           byte offset of (row, chunk c) = 64 row + 16 (c ^ ((row >> 2) & 3)).
//       A 256-byte bank window holds sixteen 16-byte units; unit of (row, c) = 4 (row & 3) + (c ^ ((row >> 2) & 3)).  The MFMA operand fetch is
//       one ds_read_b128 per lane -- lane (r = lane & 31, h = lane >> 5) takes the 16 consecutive k-bytes of chunk 2 kk + h of row r -- and the
//       LDS serves sixteen consecutive lanes at a time: rows r .. r + 15 of one chunk, whose units are all different (row & 3 gives the four
//       groups of four, (row >> 2) & 3 permutes the chunk inside a group).  The loader's stores are conflict-free the same way: sixteen
//       consecutive lanes write the four chunks of four consecutive rows.  (Both MFMA operands map lane -> k alike, and an integer sum does
//       not care about the order of k, so the k-bytes need no further arrangement.)
//     EPILOGUE.  v_cvt_f32_i32, the scale product, the multiply, the add, the activation; 16-byte stores (VEC: ldy % 4 == 0 and y 16-byte
//       aligned) or dword stores; rows >= batch and columns >= out_dim are masked here and only here.
//     No atomics, no split of K, no workspace: bit-identical from run to run whatever the grid.
#include "ffh_common.h"

#include "../../include/ffh_q8_linear.h"

#pragma clang fp contract(off)

namespace {

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x16_t __attribute__((ext_vector_type(16)));

constexpr int kQuantCap = 2048;                       // the quantizers' grid cap (ffh_q8_linear_quantize_max_workgroups)
constexpr int kStep = FFH_Q8_LINEAR_KSTEP;            // bytes of a row per main-loop step

inline int64_t q8l_ldq(int in_dim) { return ((int64_t)in_dim + kStep - 1) / kStep * kStep; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- the quantizer ---------------------------------------------------------------------------------------------------------------------------
struct QuantArgs {
  ffh_q8_linear_rows m[FFH_Q8_LINEAR_MAX_LAYERS];
  int64_t row0[FFH_Q8_LINEAR_MAX_LAYERS + 1];         // first row of matrix i in the call's row numbering; row0[n] = all rows
  int n;
};

// columns k .. k + 3 of a row of K columns (zeros behind its end)
__device__ __forceinline__ float4 q8l_load4(const float* row, int k, int K) {
  if (k + 3 < K) return ld4u(row + k);
  return make_float4(k < K ? row[k] : 0.0f, k + 1 < K ? row[k + 1] : 0.0f, k + 2 < K ? row[k + 2] : 0.0f, 0.0f);
}

__device__ __forceinline__ int q8l_pack4(const float4 v, const float inv) {
  const int a = (int)rintf(v.x * inv), b = (int)rintf(v.y * inv), c = (int)rintf(v.z * inv), d = (int)rintf(v.w * inv);
  return (a & 0xff) | ((b & 0xff) << 8) | ((c & 0xff) << 16) | ((d & 0xff) << 24);
}

template <int G>
__global__ __launch_bounds__(256) void q8l_quantize_kernel(const QuantArgs a) {
  ffh_kernel_prio();
  constexpr int RPB = 256 / G;                        // rows of a workgroup per trip
  const int sub = threadIdx.x % G, slot = threadIdx.x / G;
  const int64_t total = a.row0[a.n];
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < total; base += (int64_t)gridDim.x * RPB) {
    // (a group behind the last row stays in the loop -- the butterfly wants whole waves -- and touches no memory)
    const int64_t gr = base + slot;
    const bool live = gr < total;
    int li = 0;
    if (live) while (li + 1 < a.n && gr >= a.row0[li + 1]) li++;
    const int K = a.m[li].in_dim;
    const int64_t r = live ? gr - a.row0[li] : 0;
    const float* src = a.m[li].src + r * a.m[li].ld;
    float amax = 0.0f;
    if (live)
      for (int k0 = 16 * sub; k0 < K; k0 += 16 * G)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const float4 v = q8l_load4(src, k0 + 4 * q, K);
          amax = fmaxf(fmaxf(amax, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
#pragma unroll
    for (int d = G / 2; d > 0; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d, G));
    if (!live) continue;
    const float inv = amax > 0.0f ? 127.0f / amax : 0.0f;
    if (sub == 0) a.m[li].scales[r] = amax / 127.0f;
    const int ldq = (K + kStep - 1) / kStep * kStep;
    int8_t* dst = a.m[li].codes + r * (int64_t)ldq;
    for (int k0 = 16 * sub; k0 < ldq; k0 += 16 * G) {
      i32x4_t out;
      out.x = q8l_pack4(q8l_load4(src, k0, K), inv);
      out.y = q8l_pack4(q8l_load4(src, k0 + 4, K), inv);
      out.z = q8l_pack4(q8l_load4(src, k0 + 8, K), inv);
      out.w = q8l_pack4(q8l_load4(src, k0 + 12, K), inv);
      *reinterpret_cast<i32x4_t*>(dst + k0) = out;
    }
  }
}

int quantize_launch(ffh_ctx* c, const ffh_q8_linear_rows* layers, int n, hipStream_t s, const char* what) {
  QuantArgs a;
  memset(&a, 0, sizeof a);
  int64_t total = 0, widest = 0;
  for (int i = 0; i < n; i++) {
    const ffh_q8_linear_rows& m = layers[i];
    FFH_REQUIRE(c, m.rows >= 0 && m.in_dim >= 1 && m.in_dim <= FFH_Q8_LINEAR_MAX_IN && m.ld >= m.in_dim, what);
    FFH_REQUIRE(c, m.rows == 0 || (m.src && m.codes && m.scales && aligned16(m.codes)), what);
    a.m[i] = m;
    a.row0[i] = total;
    total += m.rows;
    if (m.rows > 0 && q8l_ldq(m.in_dim) > widest) widest = q8l_ldq(m.in_dim);
  }
  a.row0[n] = total;
  a.n = n;
  if (total == 0) return FFH_OK;
  const int64_t pieces = widest / 16;                 // 16-column pieces of the widest row: the lane group is the power of two that covers them, up to a wave
#define FFH_Q8L_QUANT(G) hipLaunchKernelGGL(q8l_quantize_kernel<G>, dim3(ffh_grid(total, 256 / G, kQuantCap)), dim3(256), 0, s, a)
  if (pieces <= 4) FFH_Q8L_QUANT(4);
  else if (pieces <= 8) FFH_Q8L_QUANT(8);
  else if (pieces <= 16) FFH_Q8L_QUANT(16);
  else if (pieces <= 32) FFH_Q8L_QUANT(32);
  else FFH_Q8L_QUANT(64);
#undef FFH_Q8L_QUANT
  FFH_LAUNCH_CHECK(c, what);
  return FFH_OK;
}

// ---- the GEMM --------------------------------------------------------------------------------------------------------------------------------
struct GemmArgs {
  const int8_t* xq; const int8_t* wq;
  const float* sx; const float* sw; const float* bias;
  float* y;
  int64_t ldy, M;                                     // M = batch
  int N, ldq, ntn, act;                               // N = out_dim; ntn = tiles along N
};

__device__ __forceinline__ unsigned q8l_off(int row, int chunk) { return (unsigned)(row * kStep + ((chunk ^ ((row >> 2) & 3)) << 4)); }

__device__ __forceinline__ float q8l_act(float v, int act) {
  if (act == FFH_AC_MODE_RELU) return v > 0.0f ? v : 0.0f;
  if (act == FFH_AC_MODE_SIGMOID) return 1.0f / (1.0f + expf(-v));
  if (act == FFH_AC_MODE_GELU) {
    constexpr float B = 0.7978845608028654f, C = 0.035677408136300125f;
    return v * (0.5f + 0.5f * tanhf(v * (C * v * v + B)));
  }
  return v;
}

template <int T, bool VEC>
__global__ __launch_bounds__(256) void q8l_gemm_kernel(const GemmArgs g) {
  ffh_kernel_prio();
  constexpr int BT = 64 * T;                          // the tile's edge, both ways
  constexpr int IMG = BT * kStep;                     // bytes of one operand image
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * IMG];      // buffer b: x image at 2 b IMG, w image behind it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;            // the wave's 32 T samples x 32 T output columns of the tile
  const int r = lane & 31, h = lane >> 5;
  const int64_t m0 = (int64_t)(blockIdx.x / (unsigned)g.ntn) * BT;
  const int n0 = (int)(blockIdx.x % (unsigned)g.ntn) * BT;
  const int nk = g.ldq / kStep;

  // the loader: piece (tid & 3) of tile rows (tid >> 2) + 64 i; rows past the matrix are clamped to its last row
  const int8_t* px[T];
  const int8_t* pw[T];
  unsigned dst[T];
#pragma unroll
  for (int i = 0; i < T; i++) {
    const int row = (tid >> 2) + 64 * i;
    const int64_t m = m0 + row < g.M ? m0 + row : g.M - 1;
    const int n = n0 + row < g.N ? n0 + row : g.N - 1;
    px[i] = g.xq + m * g.ldq + 16 * (tid & 3);
    pw[i] = g.wq + (int64_t)n * g.ldq + 16 * (tid & 3);
    dst[i] = q8l_off(row, tid & 3);
  }
  i32x4_t rx[T], rw[T];
  auto load = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < T; i++) {
      rx[i] = *reinterpret_cast<const i32x4_t*>(px[i] + kt * kStep);
      rw[i] = *reinterpret_cast<const i32x4_t*>(pw[i] + kt * kStep);
    }
  };
  auto stage = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < T; i++) {
      *reinterpret_cast<i32x4_t*>(smem + 2 * buf * IMG + dst[i]) = rx[i];
      *reinterpret_cast<i32x4_t*>(smem + (2 * buf + 1) * IMG + dst[i]) = rw[i];
    }
  };

  i32x16_t acc[T][T];                                 // [output-column block i][sample block j]
#pragma unroll
  for (int i = 0; i < T; i++)
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int v = 0; v < 16; v++) acc[i][j][v] = 0;

  load(0);
  stage(0);
  __syncthreads();
  for (int kt = 0; kt < nk; kt++) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load(kt + 1);
    const unsigned char* ximg = smem + 2 * buf * IMG;
    const unsigned char* wimg = ximg + IMG;
#pragma unroll
    for (int kk = 0; kk < 2; kk++) {
      i32x4_t fa[T], fb[T];
#pragma unroll
      for (int i = 0; i < T; i++) {
        fa[i] = *reinterpret_cast<const i32x4_t*>(wimg + q8l_off(wn * 32 * T + 32 * i + r, 2 * kk + h));
        fb[i] = *reinterpret_cast<const i32x4_t*>(ximg + q8l_off(wm * 32 * T + 32 * i + r, 2 * kk + h));
      }
#pragma unroll
      for (int i = 0; i < T; i++)
#pragma unroll
        for (int j = 0; j < T; j++) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) stage(buf ^ 1);                  // (read last in step kt - 1, behind that step's barrier)
    __syncthreads();
  }

  // accumulator [i][j], register v: sample m0 + 32 T wm + 32 j + r, output column n0 + 32 T wn + 32 i + 8 (v / 4) + 4 h + v % 4
#pragma unroll
  for (int j = 0; j < T; j++) {
    const int64_t m = m0 + wm * 32 * T + 32 * j + r;
    if (m >= g.M) continue;
    const float sxm = g.sx[m];
    float* yrow = g.y + m * g.ldy;
#pragma unroll
    for (int i = 0; i < T; i++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int o = n0 + wn * 32 * T + 32 * i + 8 * q + 4 * h;
        if (o >= g.N) continue;
        float out[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
          out[e] = 0.0f;
          if (o + e < g.N) {
            const float s = sxm * g.sw[o + e];
            float t = (float)acc[i][j][4 * q + e] * s;
            if (g.bias) t = t + g.bias[o + e];
            out[e] = q8l_act(t, g.act);
          }
        }
        if (VEC && o + 3 < g.N) {
          *reinterpret_cast<float4*>(yrow + o) = make_float4(out[0], out[1], out[2], out[3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; e++)
            if (o + e < g.N) yrow[o + e] = out[e];
        }
      }
  }
}

}  // namespace

extern "C" {

int ffh_q8_linear_abi_version(void) { return FFH_Q8_LINEAR_ABI_VERSION; }

int64_t ffh_q8_linear_ldq(int in_dim) { return in_dim >= 1 && in_dim <= FFH_Q8_LINEAR_MAX_IN ? q8l_ldq(in_dim) : 0; }

int ffh_q8_linear_quantize_max_workgroups(void) { return kQuantCap; }

int ffh_q8_linear_quantize_weights(ffh_ctx* c, const ffh_q8_linear_rows* layers, int nlayers, ffh_stream s) {
  FFH_REQUIRE(c, layers && nlayers >= 1 && nlayers <= FFH_Q8_LINEAR_MAX_LAYERS, "q8_linear_quantize_weights: bad args");
  return quantize_launch(c, layers, nlayers, as_stream(s), "q8_linear_quantize_weights: bad args");
}

int ffh_q8_linear_quantize_rows(ffh_ctx* c, const float* x, int64_t ldx, int8_t* xq, float* sx, int64_t batch, int in_dim, ffh_stream s) {
  const ffh_q8_linear_rows m = {x, ldx, xq, sx, batch, in_dim, 0};
  return quantize_launch(c, &m, 1, as_stream(s), "q8_linear_quantize_rows: bad args");
}

int ffh_q8_linear_fwd(ffh_ctx* c, const int8_t* xq, const int8_t* wq, const float* sx, const float* sw, const float* bias, float* y, int64_t ldy,
                      int64_t batch, int in_dim, int out_dim, int act, ffh_stream s) {
  FFH_REQUIRE(c, batch >= 0 && in_dim >= 1 && in_dim <= FFH_Q8_LINEAR_MAX_IN && out_dim >= 1 && ldy >= out_dim &&
                     (act == FFH_AC_MODE_NONE || act == FFH_AC_MODE_RELU || act == FFH_AC_MODE_SIGMOID || act == FFH_AC_MODE_GELU) &&
                     ((xq && wq && sx && sw && y && aligned16(xq) && aligned16(wq)) || (batch == 0 && (!xq || aligned16(xq)) && (!wq || aligned16(wq)))),
              "q8_linear_fwd: bad args");
  if (batch == 0) return FFH_OK;
  GemmArgs g;
  g.xq = xq; g.wq = wq; g.sx = sx; g.sw = sw; g.bias = bias; g.y = y; g.ldy = ldy; g.M = batch; g.N = out_dim; g.ldq = (int)q8l_ldq(in_dim); g.act = act;
  const bool vec = ldy % 4 == 0 && aligned16(y);
  const int64_t big = ((batch + 127) / 128) * (((int64_t)out_dim + 127) / 128);
  const bool t2 = big >= FFH_Q8_LINEAR_BIG_TILES;
  const int bt = t2 ? 128 : 64;
  g.ntn = (out_dim + bt - 1) / bt;
  const int64_t tiles = ((batch + bt - 1) / bt) * (int64_t)g.ntn;
  if (tiles > 0x7fffffffLL) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "q8_linear_fwd: more than 2^31 - 1 output tiles");
  const dim3 grid((unsigned)tiles);
  if (t2) { if (vec) hipLaunchKernelGGL((q8l_gemm_kernel<2, true>), grid, dim3(256), 0, as_stream(s), g); else hipLaunchKernelGGL((q8l_gemm_kernel<2, false>), grid, dim3(256), 0, as_stream(s), g); }
  else { if (vec) hipLaunchKernelGGL((q8l_gemm_kernel<1, true>), grid, dim3(256), 0, as_stream(s), g); else hipLaunchKernelGGL((q8l_gemm_kernel<1, false>), grid, dim3(256), 0, as_stream(s), g); }
  FFH_LAUNCH_CHECK(c, "q8_linear_fwd");
  return FFH_OK;
}

}  // extern "C"
