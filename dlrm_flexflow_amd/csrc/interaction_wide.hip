// interaction_wide.hip -- the pairwise-dot feature interaction for 33 .. 128 feature vectors (include/ffh_dot_wide.h).
//
// interaction.hip stops at 32 rows because a WAVE owns a sample there and the whole Z Z^T is one v_mfma_f32_32x32x2_f32 accumulator.  Here a
// 4-wave WORKGROUP owns a sample and the grid is persistent (a workgroup walks the batch with the grid as its stride):
//   forward   Z goes global -> LDS once per sample, in k-chunks of 128 columns (an image of 32 T rows x 512 bytes, T = ceil(c / 32) <= 4; two
//             images, so the next chunk -- of this sample or of the next -- streams in under this chunk's MFMAs).  With 16-byte aligned rows
//             the copy is LDS-DMA (global_load_lds_dwordx4: a 1-KiB piece = two rows per instruction), the image lane-linear with the
//             source-side swizzle of dot_interaction_fwd_lds_kernel (position p of row r holds 16-byte chunk p ^ (r & 15)), which keeps the
//             operand ds_read_b128s off each other's banks.  The gram matrix is cut into 32 x 32 tiles and only the T (T + 1) / 2 tiles with
//             ti >= tj are computed (10 of 16 at c = 128), dealt round-robin to the four waves: at most three f32x16 accumulators a wave.  A
//             diagonal tile feeds A and B from the same registers; an off-diagonal one reads two row blocks.  Rows >= c of the image hold
//             whatever the LDS held: they only reach accumulator entries with i >= c or j >= c, which are never stored.
//   backward  dZ = S Z with S = G + G^T (zero diagonal, zero padding to 32 T) assembled once per sample in LDS from the gradient's triangle,
//             row stride 32 T + 4 floats (consecutive rows one float4 apart in the banks: the A operand is four ds_read_b128 a k-block).
//             dZ[ib] = sum_jb S(ib, jb) Z[jb] runs as 32x32x2 MFMAs, A from S, B from Z in global memory with the column permutation of the
//             narrow backward (column NT n' + t belongs to lane n' of tile t, so a lane loads and stores NT consecutive floats).  NT = 2 and
//             64-column items, as in dot_interaction_bwd_d128_kernel: T row blocks x ceil(d / 64) column blocks are dealt to the four
//             waves, which at T = 4, d = 128 is one row block a wave and two items each, and at T = 2 still keeps all four busy.  Z rows
//             >= c are clamped to row c - 1 (their S columns are zero).  The next sample's triangle is loaded into registers under this
//             sample's MFMAs.
// Exact fp32, no atomics, every sample computed the same way whatever the grid: bit-identical from run to run.
#include "ffh_common.h"
#include "../../include/ffh_dot_wide.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void* dotw_lds_ptr_t;

constexpr int kMaxRows = FFH_DOT_WIDE_MAX_ROWS;
constexpr int kChunk = 128;                    // columns of a forward k-chunk
constexpr int kRowBytes = kChunk * 4;          // an image row

// ---- forward -----------------------------------------------------------------------------------------------------------------------------
// tile n of the lower triangle, row-major: n = ti (ti + 1) / 2 + tj
__device__ __forceinline__ void tile_of(int n, int& ti, int& tj) {
  ti = n >= 6 ? 3 : n >= 3 ? 2 : n >= 1 ? 1 : 0;
  tj = n - ti * (ti + 1) / 2;
}

// VEC 4: LDS-DMA (d % 4 == 0, 16-byte aligned rows); VEC 1: plain loads + ds_write.  OV: floats per store of the pass-through columns.
template <int VEC, int OV>
__global__ __launch_bounds__(256, 2) void dot_wide_fwd_kernel(const float* __restrict__ z, int64_t ldz, float* __restrict__ out, int64_t ldo,
                                                              int64_t batch, int c, int d, const float* __restrict__ zeros) {
  ffh_kernel_prio();
  extern __shared__ __attribute__((aligned(16))) unsigned char dotw_fwd_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int T = (c + 31) >> 5, ntiles = T * (T + 1) / 2;
  const int image = 32 * T * kRowBytes;                                 // bytes of one image
  const int nchunks = (d + kChunk - 1) / kChunk;
  const int npieces = (c + 1) / 2;                                      // DMA instructions per chunk: two rows each (<= 64, <= 16 a wave)
  const unsigned lds_base = (unsigned)(size_t)(dotw_lds_ptr_t)dotw_fwd_smem;

  // VEC 4: piece i of chunk kc -> LDS bytes [1024 i, 1024 i + 1024) of image `buf`: rows 2 i (lanes 0-31) and 2 i + 1 (lanes 32-63), position
  // p = lane & 31 holding chunk p ^ (row & 15).  A chunk behind the row's end comes from the ctx's zero block, the odd row behind the last one
  // from row c - 1 (a valid address, an unused image row).
  auto issue_piece = [&](const float* zb, int kc, int buf, int i) {
    int row = 2 * i + (lane >> 5);
    if (row >= c) row = c - 1;
    const int col = kc * kChunk + 4 * ((lane & 31) ^ (row & 15));
    const float* src = col < d ? zb + (int64_t)row * d + col : zeros;
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)(buf * image + i * 1024));
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
  };
  // VEC 1: the same image through registers, every element guarded (rows < c; columns behind d are zeros)
  auto copy_chunk = [&](const float* zb, int kc, int buf) {
    unsigned char* img = dotw_fwd_smem + buf * image;
    for (int e = threadIdx.x; e < c * kChunk; e += 256) {
      const int row = e >> 7, k = e & (kChunk - 1), col = kc * kChunk + k;
      const float v = col < d ? zb[(int64_t)row * d + col] : 0.0f;
      *reinterpret_cast<float*>(img + row * kRowBytes + ((((k >> 2) ^ (row & 15))) << 4) + ((k & 3) << 2)) = v;
    }
  };

  f32x16 acc[3];
  int64_t b = blockIdx.x;
  int kc = 0, buf = 0;
  if (b < batch) {
    if (VEC == 4) { for (int i = wave; i < npieces; i += 4) issue_piece(z + b * ldz, 0, 0, i); }
    else copy_chunk(z + b * ldz, 0, 0);
  }
  while (b < batch) {
    if (VEC == 4) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of the chunk have landed ...
    __syncthreads();                                                    // ... and everybody's; every read of the other image has returned
    // the item behind this one: the sample's next chunk, or the first chunk of the workgroup's next sample
    const bool last = kc + 1 == nchunks;
    const int64_t bn = last ? b + gridDim.x : b;
    const int kn = last ? 0 : kc + 1;
    const bool more = bn < batch;
    const float* zn = z + (more ? bn : b) * ldz;
    int pend = more ? wave : npieces;                                   // VEC 4: the next piece this wave issues, one per four MFMAs
    if (VEC == 1 && more) copy_chunk(zn, kn, buf ^ 1);

    const unsigned char* img = dotw_fwd_smem + buf * image;
    const int dk = min(kChunk, d - kc * kChunk);                        // columns of this chunk
    const int jmax = (dk + 7) >> 3;                                     // MFMA groups of 8 columns (chunks 2 j and 2 j + 1; one behind dk is zeros)
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int n = wave + 4 * q;
      if (n >= ntiles) continue;
      int ti, tj;
      tile_of(n, ti, tj);
      if (kc == 0) {
#pragma unroll
        for (int i = 0; i < 16; i++) acc[q][i] = 0.0f;
      }
      const unsigned char* ia = img + (32 * ti + r) * kRowBytes;
      const unsigned char* ib = img + (32 * tj + r) * kRowBytes;
      for (int j = 0; j < jmax; j++) {
        const int at = ((2 * j + h) ^ (r & 15)) << 4;
        const float4 va = *reinterpret_cast<const float4*>(ia + at);
        const float4 vb = ti == tj ? va : *reinterpret_cast<const float4*>(ib + at);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(va.x, vb.x, acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(va.y, vb.y, acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(va.z, vb.z, acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(va.w, vb.w, acc[q], 0, 0, 0);
        if (VEC == 4 && pend < npieces) { issue_piece(zn, kn, buf ^ 1, pend); pend += 4; }
      }
    }
    if (VEC == 4) for (; pend < npieces; pend += 4) issue_piece(zn, kn, buf ^ 1, pend);

    float* ob = out + b * ldo;
    // the bottom-MLP output passes through: out[0 .. d) = Z[0][:], from row 0 of the image (position p holds chunk p ^ 0)
    if (wave == 3) {
      if (OV == 4) {
        if (lane < 32 && 4 * lane < dk) *reinterpret_cast<float4*>(ob + kc * kChunk + 4 * lane) = *reinterpret_cast<const float4*>(img + 16 * lane);
      } else {
        for (int k = lane; k < dk; k += 64) ob[kc * kChunk + k] = *reinterpret_cast<const float*>(img + 4 * k);
      }
    }
    if (last) {
      // accumulator of tile (ti, tj): lane holds column j = 32 tj + r, rows i = 32 ti + 8 (v / 4) + 4 h + v % 4
      float* tri = ob + d;
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const int n = wave + 4 * q;
        if (n >= ntiles) continue;
        int ti, tj;
        tile_of(n, ti, tj);
        const int j = 32 * tj + r;
#pragma unroll
        for (int v = 0; v < 16; v++) {
          const int i = 32 * ti + 8 * (v >> 2) + 4 * h + (v & 3);
          if (i < c && j < i) tri[i * (i - 1) / 2 + j] = acc[q][v];
        }
      }
    }
    b = bn; kc = kn; buf ^= 1;
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------------
constexpr int bwd_s_stride(int T) { return 32 * T + 4; }                                 // floats
constexpr int bwd_s_bytes(int T) { return 32 * T * bwd_s_stride(T) * 4; }
constexpr int bwd_lds_bytes(int T) { return bwd_s_bytes(T) + 32 * T * (32 * T - 1); }    // + the pair table: uint16_t per pair of 32 T rows

// T: row blocks of 32 (c <= 32 T); VEC 4: 8-byte accesses of z and z_grad (even columns, 16-byte aligned rows); VEC 1: every element guarded
template <int T, int VEC, bool ACCUM>
__global__ __launch_bounds__(256, T <= 3 ? 2 : 1) void dot_wide_bwd_kernel(const float* __restrict__ z, int64_t ldz, const float* __restrict__ og, int64_t ldg,
                                                              float* __restrict__ zg, int64_t ldzg, int64_t batch, int c, int d) {
  ffh_kernel_prio();
  extern __shared__ __attribute__((aligned(16))) unsigned char dotw_bwd_smem[];
  constexpr int LD = bwd_s_stride(T);
  constexpr int NQ = (32 * T * (32 * T - 1) / 2 + 255) / 256;           // triangle entries per thread (32 at T = 4)
  float* S = reinterpret_cast<float*>(dotw_bwd_smem);
  uint16_t* pair = reinterpret_cast<uint16_t*>(dotw_bwd_smem + bwd_s_bytes(T));          // p -> i * 128 + j
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int P = c * (c - 1) / 2;
  for (int p = threadIdx.x; p < P; p += 256) {
    int i = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
    while (i * (i - 1) / 2 > p) i--;
    while ((i + 1) * i / 2 <= p) i++;
    pair[p] = (uint16_t)(i * 128 + (p - i * (i - 1) / 2));
  }
  for (int e = threadIdx.x; e < 32 * T * LD; e += 256) S[e] = 0.0f;     // diagonal and padding stay zero for every sample
  float gq[NQ];
  auto load_g = [&](int64_t s) {
    const float* gt = og + s * ldg + d;
#pragma unroll
    for (int q = 0; q < NQ; q++) { const int p = threadIdx.x + 256 * q; gq[q] = p < P ? gt[p] : 0.0f; }
  };
  int64_t b = blockIdx.x;
  if (b < batch) load_g(b);
  __syncthreads();
  const int nitems = T * ((d + 63) >> 6);
  for (; b < batch; b += gridDim.x) {
    // the strict lower triangle of the gradient -> S = G + G^T
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int p = threadIdx.x + 256 * q;
      if (p < P) {
        const int ij = pair[p], i = ij >> 7, j = ij & 127;
        S[i * LD + j] = gq[q];
        S[j * LD + i] = gq[q];
      }
    }
    __syncthreads();
    if (b + gridDim.x < batch) load_g(b + gridDim.x);                   // in flight under this sample's MFMAs
    const float* gb = og + b * ldg;
    const float* zb = z + b * ldz;
    float* zgb = zg + b * ldzg;
    for (int it = wave; it < nitems; it += 4) {
      const int ib = it % T, col = (it / T) * 64 + 2 * r;                // row block; this lane's two columns (of tiles 0 and 1)
      float bv[2][16][2];
      // B operand of k-block jb: Z[32 jb + 16 h + s][col + t] at step s, rows >= c clamped to c - 1
      auto load_b = [&](float (&dst)[16][2], int jb) {
#pragma unroll
        for (int s = 0; s < 16; s++) {
          int k = 32 * jb + 16 * h + s;
          k = k < c ? k : c - 1;
          asm volatile("" : "+v"(k));                                    // (opaque: sixty-four row addresses hoisted out of the sample loop cost the registers they save)
          const float* p = zb + (int64_t)k * d + col;
          if (VEC == 4) {
            float2 t2 = make_float2(0.0f, 0.0f);
            if (col < d) t2 = *reinterpret_cast<const float2*>(p);
            dst[s][0] = t2.x; dst[s][1] = t2.y;
          } else {
            dst[s][0] = col < d ? p[0] : 0.0f;
            dst[s][1] = col + 1 < d ? p[1] : 0.0f;
          }
        }
      };
      f32x16 acc[2];
#pragma unroll
      for (int t = 0; t < 2; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[t][i] = 0.0f;
      load_b(bv[0], 0);
#pragma unroll
      for (int jb = 0; jb < T; jb++) {
        if (jb + 1 < T) load_b(bv[(jb + 1) & 1], jb + 1);               // under this k-block's MFMAs
        // A operand: S[32 ib + r][32 jb + 16 h + s] at step s
        float a[16];
        const float4* sa = reinterpret_cast<const float4*>(S + (32 * ib + r) * LD + 32 * jb + 16 * h);
#pragma unroll
        for (int u = 0; u < 4; u++) { const float4 t4 = sa[u]; a[4 * u] = t4.x; a[4 * u + 1] = t4.y; a[4 * u + 2] = t4.z; a[4 * u + 3] = t4.w; }
#pragma unroll
        for (int s = 0; s < 16; s++)
#pragma unroll
          for (int t = 0; t < 2; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bv[jb & 1][s][t], acc[t], 0, 0, 0);
      }
      // accumulator of tile t: lane holds column col + t, rows i = 32 ib + 8 (v / 4) + 4 h + v % 4
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const int i = 32 * ib + 8 * (v >> 2) + 4 * h + (v & 3);
        if (i >= c) continue;
        float o0 = acc[0][v], o1 = acc[1][v];
        if (i == 0) {                                                    // direct path of the bottom-MLP output
          if (col < d) o0 += gb[col];
          if (col + 1 < d) o1 += gb[col + 1];
        }
        float* dst = zgb + (int64_t)i * d + col;
        if (VEC == 4) {
          if (col < d) {
            float2* d2 = reinterpret_cast<float2*>(dst);
            if (ACCUM) { const float2 old = *d2; o0 += old.x; o1 += old.y; }
            *d2 = make_float2(o0, o1);
          }
        } else {
          if (col < d) dst[0] = ACCUM ? dst[0] + o0 : o0;
          if (col + 1 < d) dst[1] = ACCUM ? dst[1] + o1 : o1;
        }
      }
    }
    __syncthreads();                                                     // S is rewritten for the next sample
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

unsigned wide_grid(const ffh_ctx* c, int64_t batch, int per_cu) {
  const int64_t cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * per_cu;
  return (unsigned)(batch < cap ? batch : cap);
}

template <class K>
bool allow_lds(K kernel, int bytes) {
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
}

template <int T>
int launch_bwd(ffh_ctx* c, const float* z, int64_t ldz, const float* og, int64_t ldg, float* zg, int64_t ldzg, int64_t batch, int nrows, int d,
               bool v4, bool over, hipStream_t s) {
  constexpr int lds = bwd_lds_bytes(T);
  static const bool ok = allow_lds(dot_wide_bwd_kernel<T, 4, true>, lds) && allow_lds(dot_wide_bwd_kernel<T, 4, false>, lds) &&
                         allow_lds(dot_wide_bwd_kernel<T, 1, true>, lds) && allow_lds(dot_wide_bwd_kernel<T, 1, false>, lds);
  if (!ok) { (void)hipGetLastError(); return ffh_fail(c, FFH_ERR_HIP, "dot_interaction_wide_bwd: the device refuses the kernel's LDS size"); }
  const unsigned grid = wide_grid(c, batch, FFH_DOT_WIDE_BWD_PER_CU(nrows));
#define FFH_DOTW_BWD(V, A) hipLaunchKernelGGL((dot_wide_bwd_kernel<T, V, A>), dim3(grid), dim3(256), lds, s, z, ldz, og, ldg, zg, ldzg, batch, nrows, d)
  if (v4) { if (over) FFH_DOTW_BWD(4, false); else FFH_DOTW_BWD(4, true); }
  else { if (over) FFH_DOTW_BWD(1, false); else FFH_DOTW_BWD(1, true); }
#undef FFH_DOTW_BWD
  FFH_LAUNCH_CHECK(c, "dot_interaction_wide_bwd");
  return FFH_OK;
}

}  // namespace

extern "C" {

int ffh_dot_wide_abi_version(void) { return FFH_DOT_WIDE_ABI_VERSION; }

int ffh_dot_interaction_wide_fwd(ffh_ctx* c, const float* z, int64_t ldz, float* out, int64_t ldo, int64_t batch, int nrows, int d, ffh_stream s) {
  FFH_REQUIRE(c, batch >= 0 && nrows >= 2 && nrows <= kMaxRows && d >= 1 && ldz >= (int64_t)nrows * d &&
                     ldo >= d + (int64_t)nrows * (nrows - 1) / 2 && ((z && out) || batch == 0),
              "dot_interaction_wide_fwd: bad args");
  if (batch == 0) return FFH_OK;
  // (a chunk behind a row's end is DMA'd from the ctx's zero block: without one, rows that are no whole number of chunks take the scalar form)
  const bool v4 = d % 4 == 0 && ldz % 4 == 0 && aligned16(z) && (c->zeros || d % kChunk == 0);
  const bool o4 = v4 && ldo % 4 == 0 && aligned16(out);
  const int T = (nrows + 31) / 32, lds = 2 * 32 * T * kRowBytes;         // two images: 32 KB a row block
  static const bool ok = allow_lds(dot_wide_fwd_kernel<4, 4>, 2 * kMaxRows * kRowBytes) && allow_lds(dot_wide_fwd_kernel<4, 1>, 2 * kMaxRows * kRowBytes) &&
                         allow_lds(dot_wide_fwd_kernel<1, 1>, 2 * kMaxRows * kRowBytes);
  if (!ok) { (void)hipGetLastError(); return ffh_fail(c, FFH_ERR_HIP, "dot_interaction_wide_fwd: the device refuses the kernel's LDS size"); }
  const unsigned grid = wide_grid(c, batch, FFH_DOT_WIDE_FWD_PER_CU(nrows));
  if (o4) hipLaunchKernelGGL((dot_wide_fwd_kernel<4, 4>), dim3(grid), dim3(256), lds, as_stream(s), z, ldz, out, ldo, batch, nrows, d, (const float*)c->zeros);
  else if (v4) hipLaunchKernelGGL((dot_wide_fwd_kernel<4, 1>), dim3(grid), dim3(256), lds, as_stream(s), z, ldz, out, ldo, batch, nrows, d, (const float*)c->zeros);
  else hipLaunchKernelGGL((dot_wide_fwd_kernel<1, 1>), dim3(grid), dim3(256), lds, as_stream(s), z, ldz, out, ldo, batch, nrows, d, (const float*)c->zeros);
  FFH_LAUNCH_CHECK(c, "dot_interaction_wide_fwd");
  return FFH_OK;
}

int ffh_dot_interaction_wide_bwd(ffh_ctx* c, const float* z, int64_t ldz, const float* out_grad, int64_t ldg, float* z_grad, int64_t ldzg,
                                 int64_t batch, int nrows, int d, int flags, ffh_stream s) {
  FFH_REQUIRE(c, batch >= 0 && nrows >= 2 && nrows <= kMaxRows && d >= 1 && ldz >= (int64_t)nrows * d && ldzg >= (int64_t)nrows * d &&
                     ldg >= d + (int64_t)nrows * (nrows - 1) / 2 && ((z && out_grad && z_grad) || batch == 0) &&
                     (flags & ~FFH_DOT_BWD_OVERWRITE) == 0,
              "dot_interaction_wide_bwd: bad args");
  if (batch == 0) return FFH_OK;
  const bool v4 = d % 4 == 0 && ldz % 4 == 0 && ldzg % 4 == 0 && aligned16(z) && aligned16(z_grad);
  const bool over = (flags & FFH_DOT_BWD_OVERWRITE) != 0;
  switch ((nrows + 31) / 32) {
    case 1: return launch_bwd<1>(c, z, ldz, out_grad, ldg, z_grad, ldzg, batch, nrows, d, v4, over, as_stream(s));
    case 2: return launch_bwd<2>(c, z, ldz, out_grad, ldg, z_grad, ldzg, batch, nrows, d, v4, over, as_stream(s));
    case 3: return launch_bwd<3>(c, z, ldz, out_grad, ldg, z_grad, ldzg, batch, nrows, d, v4, over, as_stream(s));
    default: return launch_bwd<4>(c, z, ldz, out_grad, ldg, z_grad, ldzg, batch, nrows, d, v4, over, as_stream(s));
  }
}

}  // extern "C"
