// embedding.hip -- Embedding forward (gather + bag-sum), the reference's dense atomic
// backward, and the fused backward + sparse SGD, hand-written for gfx950.
//
// HBM-bound integer/byte work.  Design rules applied:
//   * a table row is read by `D/4` adjacent lanes with one 16-B load each, so a
//     wave-instruction covers 64/(D/4) whole rows (512-B rows: two per instruction,
//     64-B rows: sixteen) -- full-line coalesced reads and writes;
//   * every lane-group keeps several independent row loads in flight (UNROLL);
//   * all tables of a model go in ONE launch (grid.y = table) instead of the
//     reference's one task per table;
//   * 64-bit addressing everywhere (a 200M x 256 table is 204.8 GB; the reference's
//     `int outputSize` [ref: src/ops/embedding.cu:226,229] would overflow);
//   * the backward never materialises the dense [R][D] gradient: row ids are radix-sorted
//     per table with LDS histograms and wave-ballot ranking, duplicate rows are reduced
//     in registers by the lane-group that owns the run, and each touched row is
//     read-modified-written exactly once.
// This file: the gather, the dense backward, the sort launches, validation, the workspace layout and every entry point.  The sort
// kernels are emb_sort.h; the apply phase's kernels (emb_reduce.h) and the row rules (emb_row_rules.h) are compiled per weight type in
// embedding_update_f32.hip / embedding_update_bf16.hip and reached through emb_update_launch_f32 / _bf16.  The update of tables with a bag
// size per table (include/ff_hip_bags_update.h): the entry and its layout are here, its kernels in emb_bags_update.h, compiled in
// embedding_update_bags_f32.hip / _bf16.hip.
#include "emb_reduce.h"
#include "fold_sum.h"
#include "lr_state.h"
#include "../../include/ff_hip_bags.h"
#include "../../include/ff_hip_bags_update.h"
#include "emb_bags_update.h"

#include <type_traits>

namespace {

using namespace ffh_emb;

struct EmbArgs {
  ffh_emb_table t[FFH_MAX_TABLES];
  unsigned short* out16[FFH_MAX_TABLES];   // forward, tensor-op mode: bf16 twin of t[i].io (same leading dimension) or null
  char* out3[FFH_MAX_TABLES];              // forward, split mode: the I32 image group that holds t[i].io[0] (ffh_ctx_bf16x3_mirror_set) or null ...
  int   out3c[FFH_MAX_TABLES];             // ... and that element's position in its group
  int64_t batch;
  int     ntables;
  int     L;
  int     D;
  int     aggr;
  int64_t nt_rows;       // tables of more rows: the 16-byte row loads carry a nontemporal hint, which the compiler drops (emb_fwd_launch)
};

// ---------------------------------------------------------------------------
// forward: out[b][:] = sum_j W[idx[b][j]][:]
// ---------------------------------------------------------------------------
// VEC = table elements per lane per access: 4 (fp32 tables: 16-B accesses; bf16 tables, WT = uint16_t (ff_hip_bf16.h): 8-B accesses)
// or 1 (any D / alignment).  A bf16 element widens exactly and the sums run in the same order: the same bits as the fp32 gather on
// the widened table.
template <int VEC, class WT> struct RowVec { typedef typename std::conditional<VEC == 4, float4, float>::type type; };
template <> struct RowVec<4, uint16_t> { typedef uint2 type; };
template <> struct RowVec<1, uint16_t> { typedef unsigned short type; };
template <int VEC, class WT>
__device__ __forceinline__ float row_elem(const typename RowVec<VEC, WT>::type& v, int k) {
  if constexpr (std::is_same<WT, float>::value) return reinterpret_cast<const float*>(&v)[k];
  else return ffh_bf16_to_f32(reinterpret_cast<const unsigned short*>(&v)[k]);
}

template <int VEC, int UNROLL, class WT = float>
__global__ __launch_bounds__(256) void emb_fwd_kernel(const EmbArgs a) {
  ffh_kernel_prio();
  using vec_t = typename RowVec<VEC, WT>::type;
  constexpr int NQ = VEC / 4;                     // 16-B groups of output floats per lane-access (0: scalar)
  const ffh_emb_table tb = a.t[blockIdx.y];
  const WT* const wt = reinterpret_cast<const WT*>(tb.weight);
  unsigned short* const o16 = a.out16[blockIdx.y];
  char* const o3 = a.out3[blockIdx.y];
  const int o3c = a.out3c[blockIdx.y];
  const int D = a.D, L = a.L;
  const int nvec = D / VEC;                       // vectors per row
  const int lpr = nvec < 64 ? nvec : 64;          // lanes per row
  const int rpw = 64 / lpr;                       // rows per wave-instruction
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int rsub = lane / lpr;                    // which of the wave's rows
  const int c0 = lane - rsub * lpr;               // first vector of the row for this lane
  const bool active = rsub < rpw;
  const int64_t rows_per_block = (int64_t)(blockDim.x >> 6) * rpw * UNROLL;
  const float inv = 1.0f / (float)L;
  const bool avg = a.aggr == FFH_AGGR_MODE_AVG;

  for (int64_t base = (int64_t)blockIdx.x * rows_per_block; base < a.batch; base += (int64_t)gridDim.x * rows_per_block) {
    const int64_t b0 = base + (int64_t)wave * rpw * UNROLL + rsub;
    for (int c = c0; c < nvec; c += lpr) {
      float acc[UNROLL][VEC];
#pragma unroll
      for (int u = 0; u < UNROLL; u++)
#pragma unroll
        for (int v = 0; v < VEC; v++) acc[u][v] = 0.0f;
      for (int j = 0; j < L; j++) {
        int64_t row[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
          const int64_t b = b0 + (int64_t)u * rpw;
          row[u] = (active && b < a.batch) ? tb.idx[b * L + j] : -1;
        }
        vec_t val[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++)
          if (row[u] >= 0) {
            const vec_t* src = reinterpret_cast<const vec_t*>(wt + row[u] * (int64_t)D) + c;
            if (sizeof(vec_t) == 16 && tb.num_entries > a.nt_rows) { typedef float f4 __attribute__((ext_vector_type(4))); const f4 t = __builtin_nontemporal_load(reinterpret_cast<const f4*>(src)); val[u] = *reinterpret_cast<const vec_t*>(&t); }
            else val[u] = *src;
          }
#pragma unroll
        for (int u = 0; u < UNROLL; u++)
          if (row[u] >= 0) {
#pragma unroll
            for (int v = 0; v < VEC; v++) acc[u][v] = acc[u][v] + row_elem<VEC, WT>(val[u], v);   // 0 + w first: (+0)+(-0) = +0 as the reference
          }
      }
#pragma unroll
      for (int u = 0; u < UNROLL; u++) {
        const int64_t b = b0 + (int64_t)u * rpw;
        if (active && b < a.batch) {
          float f[VEC];
#pragma unroll
          for (int v = 0; v < VEC; v++) f[v] = avg ? acc[u][v] * inv : acc[u][v];
          if constexpr (NQ == 0) {
            tb.io[b * tb.ld + c] = f[0];
          } else {
#pragma unroll
            for (int h = 0; h < NQ; h++) {
              const int q = c * NQ + h;                 // float4 index in the output row
              const float* g = f + 4 * h;
              typedef float f4 __attribute__((ext_vector_type(4)));
              const f4 o = {g[0], g[1], g[2], g[3]};
              reinterpret_cast<f4*>(tb.io + b * tb.ld)[q] = o;
              if (o16) {      // the twin the first top-MLP GEMM reads its operand from (ffh_ctx_bf16_mirror_set)
                typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
                const bf2 lo = {(__bf16)g[0], (__bf16)g[1]}, hi = {(__bf16)g[2], (__bf16)g[3]};
                reinterpret_cast<uint2*>(o16 + b * tb.ld)[q] = make_uint2(__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi));
              }
              if (o3) {       // split mode: the three-plane image of the row piece (ffh_ctx_bf16x3_mirror_set; ld a multiple of 32)
                uint2 p1, p2, p3;
                ffh_split_bf16x3(make_float4(g[0], g[1], g[2], g[3]), p1, p2, p3);
                char* d = o3 + b * tb.ld * 6 + ffh_i32_off(o3c + 4 * q);
                *reinterpret_cast<uint2*>(d) = p1; *reinterpret_cast<uint2*>(d + 64) = p2; *reinterpret_cast<uint2*>(d + 128) = p3;
              }
            }
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// forward with a bag size per table (include/ff_hip_bags.h): the same sums, per table, as emb_fwd_kernel -- acc = +0, then
// acc = acc + W[idx[b][j]] for j ascending, AVG times the table's own 1 / L -- so a table's output is the bits of emb_fwd_kernel on
// that table alone.  What differs is how the work is laid over the chip:
//   * a FLAT grid.  Table t gets bag_blocks() workgroups, in proportion to its lookups batch * L_t (at least one, at most one per
//     row block); workgroup -> (table, first row block) is a scan over the <= 64 bag sizes in the kernel arguments.  The scan is
//     block-uniform (SGPRs), and host and kernel compute it with the one function below.
//   * long bags (L >= kBagLong) keep JU consecutive j of a row in flight beside U rows: a bag's ids are contiguous, the loads of
//     JU ids and then of JU table rows are issued together, and the adds follow in ascending j.  Short bags run U = 4 rows with one
//     j each, as emb_fwd_kernel does.  Long bags take half the rows per workgroup, so a table of few rows and long bags still
//     splits into enough row blocks.
// Kernel arguments: 64 tables of 40 bytes plus two pointer arrays are 3584 bytes; a bag size in 16 bits and the image column (< 32)
// in 8 bits per table keep the struct below EmbArgs' size, and the prefix of the workgroup map is derived, not passed.
// ---------------------------------------------------------------------------
constexpr int kBagLong = 4;        // bags of at least this many ids take the JU = 4 form
constexpr int kBagMaxL = 65535;    // BagArgs::L is 16 bits (FFH_BAGS_MAX_IN_DIM)
struct BagArgs {
  ffh_emb_table t[FFH_MAX_TABLES];
  unsigned short* out16[FFH_MAX_TABLES];   // as EmbArgs::out16
  char* out3[FFH_MAX_TABLES];              // as EmbArgs::out3 ...
  uint16_t L[FFH_MAX_TABLES];              // bag size of table i
  uint8_t  out3c[FFH_MAX_TABLES];          // ... and EmbArgs::out3c (0 .. 31)
  int64_t batch;
  int64_t nrb[2];        // row blocks of the batch: [0] short bags (U = 4), [1] long bags (U = 2)
  int     ntables;
  int     D;
  int     aggr;
  int     shift;         // workgroups of table i = clamp((batch * L[i]) >> shift, 1, nrb)
};
static_assert(sizeof(BagArgs) <= sizeof(EmbArgs) && sizeof(BagArgs) <= 4096, "kernel arguments");

__host__ __device__ inline int64_t bag_blocks(int64_t batch, int L, int shift, int64_t nrb) {
  int64_t w = (batch * (int64_t)L) >> shift;
  w = w < 1 ? 1 : w;
  return w > nrb ? nrb : w;
}

// the rows [first, first + step, ...) x rows_per_block of table t; U rows x JU ids in flight per lane-group
template <int VEC, int U, int JU, class WT>
__device__ __forceinline__ void bag_rows(const BagArgs& a, const int t, const int64_t first, const int64_t step) {
  using vec_t = typename RowVec<VEC, WT>::type;
  constexpr int NQ = VEC / 4;
  const ffh_emb_table tb = a.t[t];
  const WT* const wt = reinterpret_cast<const WT*>(tb.weight);
  unsigned short* const o16 = a.out16[t];
  char* const o3 = a.out3[t];
  const int o3c = a.out3c[t];
  const int D = a.D, L = a.L[t];
  const int nvec = D / VEC;
  const int lpr = nvec < 64 ? nvec : 64;
  const int rpw = 64 / lpr;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int rsub = lane / lpr;
  const int c0 = lane - rsub * lpr;
  const bool active = rsub < rpw;
  const int64_t rows_per_block = 4LL * rpw * U;      // 256 threads
  const float inv = 1.0f / (float)L;
  const bool avg = a.aggr == FFH_AGGR_MODE_AVG;

  for (int64_t base = first * rows_per_block; base < a.batch; base += step * rows_per_block) {
    const int64_t b0 = base + (int64_t)wave * rpw * U + rsub;
    bool ok[U];
    const int64_t* ids[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t b = b0 + (int64_t)u * rpw;
      ok[u] = active && b < a.batch;
      ids[u] = tb.idx + b * L;
    }
    for (int c = c0; c < nvec; c += lpr) {
      float acc[U][VEC];
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int v = 0; v < VEC; v++) acc[u][v] = 0.0f;
      int j = 0;
      if constexpr (JU > 1) {
        for (; j + JU <= L; j += JU) {
          int64_t row[U][JU];
#pragma unroll
          for (int u = 0; u < U; u++)
#pragma unroll
            for (int k = 0; k < JU; k++) row[u][k] = ok[u] ? ids[u][j + k] : 0;
          vec_t val[U][JU];
#pragma unroll
          for (int u = 0; u < U; u++)
#pragma unroll
            for (int k = 0; k < JU; k++)
              if (ok[u]) val[u][k] = *(reinterpret_cast<const vec_t*>(wt + row[u][k] * (int64_t)D) + c);
#pragma unroll
          for (int u = 0; u < U; u++)
            if (ok[u]) {
#pragma unroll
              for (int k = 0; k < JU; k++)           // ascending j: the order of emb_fwd_kernel
#pragma unroll
                for (int v = 0; v < VEC; v++) acc[u][v] = acc[u][v] + row_elem<VEC, WT>(val[u][k], v);
            }
        }
      }
      for (; j < L; j++) {
        int64_t row[U];
#pragma unroll
        for (int u = 0; u < U; u++) row[u] = ok[u] ? ids[u][j] : 0;
        vec_t val[U];
#pragma unroll
        for (int u = 0; u < U; u++)
          if (ok[u]) val[u] = *(reinterpret_cast<const vec_t*>(wt + row[u] * (int64_t)D) + c);
#pragma unroll
        for (int u = 0; u < U; u++)
          if (ok[u]) {
#pragma unroll
            for (int v = 0; v < VEC; v++) acc[u][v] = acc[u][v] + row_elem<VEC, WT>(val[u], v);   // 0 + w first, as emb_fwd_kernel
          }
      }
      // the stores of emb_fwd_kernel, statement by statement (that kernel is left as it compiles today)
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int64_t b = b0 + (int64_t)u * rpw;
        if (ok[u]) {
          float f[VEC];
#pragma unroll
          for (int v = 0; v < VEC; v++) f[v] = avg ? acc[u][v] * inv : acc[u][v];
          if constexpr (NQ == 0) {
            tb.io[b * tb.ld + c] = f[0];
          } else {
#pragma unroll
            for (int h = 0; h < NQ; h++) {
              const int q = c * NQ + h;
              const float* g = f + 4 * h;
              typedef float f4 __attribute__((ext_vector_type(4)));
              const f4 o = {g[0], g[1], g[2], g[3]};
              reinterpret_cast<f4*>(tb.io + b * tb.ld)[q] = o;
              if (o16) {
                typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
                const bf2 lo = {(__bf16)g[0], (__bf16)g[1]}, hi = {(__bf16)g[2], (__bf16)g[3]};
                reinterpret_cast<uint2*>(o16 + b * tb.ld)[q] = make_uint2(__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi));
              }
              if (o3) {
                uint2 p1, p2, p3;
                ffh_split_bf16x3(make_float4(g[0], g[1], g[2], g[3]), p1, p2, p3);
                char* d = o3 + b * tb.ld * 6 + ffh_i32_off(o3c + 4 * q);
                *reinterpret_cast<uint2*>(d) = p1; *reinterpret_cast<uint2*>(d + 64) = p2; *reinterpret_cast<uint2*>(d + 128) = p3;
              }
            }
          }
        }
      }
    }
  }
}

template <int VEC, class WT>
__global__ __launch_bounds__(256) void emb_fwd_bags_kernel(const BagArgs a) {
  ffh_kernel_prio();
  // workgroup -> (table, first row block of the table): block-uniform
  int t = 0;
  int64_t first = blockIdx.x, w = 0;
  for (; t < a.ntables; t++) {
    const int L = a.L[t];
    w = bag_blocks(a.batch, L, a.shift, L >= kBagLong ? a.nrb[1] : a.nrb[0]);
    if (first < w) break;
    first -= w;
  }
  if (t >= a.ntables) return;
  if (a.L[t] >= kBagLong) bag_rows<VEC, 2, 4, WT>(a, t, first, w);
  else bag_rows<VEC, 4, 1, WT>(a, t, first, w);
}

// ---------------------------------------------------------------------------
// reference-parity dense backward: fp32 atomics into the full-table gradient.
// One dword per lane, lanes contiguous along the row: each atomic wave-instruction is
// 256 contiguous bytes, the shape the memory-side atomic units run at full rate.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void emb_bwd_dense_kernel(const int64_t* __restrict__ idx, const float* __restrict__ g,
                                                            float* __restrict__ wg, int L, int D, int64_t batch,
                                                            int64_t gld, int avg) {
  ffh_kernel_prio();
  const int64_t total = batch * D;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t b = i / D;
    const int off = (int)(i - b * D);
    float gr = g[b * gld + off];
    if (avg) gr = gr / (float)L;
    for (int j = 0; j < L; j++) {
      const int64_t row = idx[b * L + j];
      atomicAdd(wg + row * (int64_t)D + off, gr);
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct BwdLayout {
  size_t kp_a, kp_b, hist, partial, meta, partial1, meta1, arrive, bstart, total;
  int nblk, nchunks, nchunks1;
};

// entries per thread of the sort kernels: enough workgroups to cover the chip, tiles as large as that allows
inline int sort_per_thread(int nt, int64_t N) {
  const int64_t want = N * nt / (512LL * kSortThreads);
  int e = 1;
  while (e * 2 <= want && e < kSortMaxPerThread) e *= 2;
  // every scatter workgroup walks the table's [tiles][radix] histogram matrix: keep <= 32 tiles per table
  while ((N + (int64_t)kSortThreads * e - 1) / ((int64_t)kSortThreads * e) > 32 && e < kSortMaxPerThread) e *= 2;
  return e;
}
inline int reduce_tile(int nt, int64_t N) {
  const int64_t want = N * nt / 1024;
  int t = 128;
  while (t * 2 <= want && t < kRedTile) t *= 2;
  return t;
}

inline BwdLayout bwd_layout(int nt, int L, int D, int64_t batch) {
  BwdLayout l;
  const int64_t N = batch * L;
  const int sort_tile = kSortThreads * sort_per_thread(nt, N);
  l.nblk = (int)((N + sort_tile - 1) / sort_tile);
  l.nchunks = (int)((N + FFH_EMB_CHUNK - 1) / FFH_EMB_CHUNK);
  const size_t arr = align_up((size_t)nt * (size_t)N * sizeof(uint2), 256);
  size_t o = 0;
  l.kp_a = o; o += arr;
  l.kp_b = o; o += arr;
  l.hist = o; o += align_up((size_t)nt * (size_t)l.nblk * kMaxRadix * sizeof(uint32_t), 256);
  l.partial = o; o += align_up((size_t)nt * 2 * (size_t)l.nchunks * (size_t)D * sizeof(float), 256);
  l.meta = o; o += align_up((size_t)nt * 2 * (size_t)l.nchunks * sizeof(uint2), 256);
  l.nchunks1 = (int)((N + FFH_EMB_CHUNK1 - 1) / FFH_EMB_CHUNK1);
  l.partial1 = o; o += align_up((size_t)nt * 2 * (size_t)l.nchunks1 * (size_t)D * sizeof(float), 256);
  l.meta1 = o; o += align_up((size_t)nt * 2 * (size_t)l.nchunks1 * sizeof(uint2), 256);
  l.arrive = o; o += align_up((size_t)nt * ((size_t)l.nchunks1 + 1) * sizeof(uint32_t), 256);
  l.bstart = o; o += align_up((size_t)nt * (kMaxRadix + 1) * sizeof(uint32_t), 256);      // (bucket form; its nextkey array lives in `hist`, free by then)
  l.total = o;
  return l;
}

int validate_tables(ffh_ctx* c, const ffh_emb_table* t, int nt, int L, int D, int64_t batch, int aggr, const char* who) {
  if (nt < 0 || nt > FFH_MAX_TABLES) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding: ntables out of range");
  if (L <= 0 || D <= 0 || batch < 0) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding: bad dims");
  if (aggr != FFH_AGGR_MODE_SUM && aggr != FFH_AGGR_MODE_AVG) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding: aggr must be SUM or AVG");
  for (int i = 0; i < nt; i++) {
    if (batch > 0 && (!t[i].idx || !t[i].weight || !t[i].io)) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding: null pointer");
    if (t[i].ld < D || t[i].num_entries <= 0) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding: ld < out_dim or num_entries <= 0");
  }
  (void)who;
  return FFH_OK;
}

bool can_vec4(const ffh_emb_table* t, int nt, int D) {
  if (D % 4) return false;
  for (int i = 0; i < nt; i++)
    if (!aligned16(t[i].weight) || !aligned16(t[i].io) || (t[i].ld % 4)) return false;
  return true;
}

}  // namespace

// row-wise sharded table: global id -> local id, rows held elsewhere -> the zero row behind the local slice
__global__ __launch_bounds__(256) void emb_localize_kernel(const int64_t* __restrict__ idx, int64_t* __restrict__ local, int64_t n,
                                                           int64_t row_begin, int64_t rows_local) {
  ffh_kernel_prio();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = idx[i] - row_begin;
    local[i] = (r >= 0 && r < rows_local) ? r : rows_local;
  }
}

// WT = float: ffh_embedding_fwd_multi; WT = uint16_t: ffh_embedding_fwd_multi_bf16 (`tables[i].weight` holds bf16 bits)
template <class WT>
static int emb_fwd_launch(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int D, int64_t batch, int aggr, ffh_stream s) {
  int rc = validate_tables(c, tables, nt, L, D, batch, aggr, "embedding_fwd");
  if (rc) return rc;
  if (nt == 0 || batch == 0) return FFH_OK;
  constexpr bool b16 = std::is_same<WT, uint16_t>::value;
  const bool v4 = can_vec4(tables, nt, D);
  int vec = v4 ? 4 : 1;
  if (b16) {
    // 4 bf16 per 8-B access, the output side as in the fp32 form.  (8 per 16-B access -- the lanes per row halved, the same bytes in
    // flight per wave -- was measured at the Terabyte shape and was slower: 107 VGPRs, occupancy 4, 163 against 146 us; UNROLL 2
    // did not help. profiles/bf16_table_bench.txt)
    bool ok = D % 4 == 0;
    for (int i = 0; i < nt; i++) ok = ok && ((uintptr_t)tables[i].weight & 7) == 0 && aligned16(tables[i].io) && tables[i].ld % 4 == 0;
    vec = ok ? 4 : 1;
  }
  const int nvec = D / vec;
  if ((nvec + 63) / 64 > kMaxChunks * 64) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_fwd: out_dim too large");
  EmbArgs a;
  memset(&a, 0, sizeof a);
  for (int i = 0; i < nt; i++) {
    a.t[i] = tables[i];
    // tensor-op mode with a registered twin of the destination: the gather writes the bf16 roundings beside the fp32 rows
    a.out16[i] = (vec >= 4 && tables[i].ld % 4 == 0) ? ffh_mirror_of(c, tables[i].io, (size_t)((batch - 1) * tables[i].ld + D) * 4) : nullptr;
    // split mode with a registered image of the destination (rows a whole number of 32-element groups apart): the three terms beside the fp32 rows
    int col0 = 0;
    a.out3[i] = (vec >= 4 && tables[i].ld % 32 == 0) ? ffh_planes_of(c, tables[i].io, (size_t)((batch - 1) * tables[i].ld + D) * 4, &col0) : nullptr;
    a.out3c[i] = col0;
    if (a.out3[i] && (col0 & 3)) a.out3[i] = nullptr;
  }
  a.batch = batch; a.ntables = nt; a.L = L; a.D = D; a.aggr = aggr;
  // Cache policy (round 6): the output is written once and read much later by a GEMM -- 436 MB per launch at the Terabyte shape, more than the
  // Infinity Cache holds -- and a row of a table too big to stay cached is touched once per launch: both as NONTEMPORAL accesses, so that they do
  // not evict the rows of the 18 small tables (62 MB) that do live in L2 / Infinity Cache.  One box, interleaved: 139.4 -> 133.7 (stores) / 133.8
  // (loads) / 130.9 us (both) = 0.79 -> 0.84 of 8 TB/s by the algorithmic-bytes formula; the step unchanged.  Same bits.
  // As compiled, neither hint survives: the compiler merged each hinted access with its plain twin and dropped the hint, so the
  // kernel's loads and stores are plain.  The stores are now written plain; making the policy real is a change of its own, to be measured.
  a.nt_rows = (int64_t)FFH_LAB_INT("FFH_EMB_NT_MB", 64) * (1 << 20) / ((int64_t)D * (int64_t)sizeof(WT));      // tables above 64 MB (bytes, not rows)
  const int lpr = nvec < 64 ? nvec : 64;
  const int rpw = 64 / lpr;
  constexpr int U = 4;
  const int64_t rows_per_block = 4LL * rpw * U;
  // fill 256 CUs x 8 workgroups across all tables, grid-stride the rest
  int64_t gx = (batch + rows_per_block - 1) / rows_per_block;
  static const int cap_env = FFH_LAB_INT("FFH_EMB_FWD_CAP", 1024);   // A/B switch: workgroups over all tables
  const int64_t cap = cap_env / nt > 0 ? cap_env / nt : 1;
  if (gx > cap) gx = cap;
  dim3 grid((unsigned)gx, (unsigned)nt);
  if (vec == 4) hipLaunchKernelGGL((emb_fwd_kernel<4, U, WT>), grid, dim3(256), 0, as_stream(s), a);
  else hipLaunchKernelGGL((emb_fwd_kernel<1, U, WT>), grid, dim3(256), 0, as_stream(s), a);
  FFH_LAUNCH_CHECK(c, "emb_fwd_kernel");
  return FFH_OK;
}

// include/ff_hip_bags.h.  WT as in emb_fwd_launch; the 16-byte form under the same conditions, so a table's bits are those of its own
// ffh_embedding_fwd call wherever that call and this one take the same form (all tables aligned alike, or D % 4 != 0).
template <class WT>
static int emb_fwd_bags_launch(ffh_ctx* c, const ffh_emb_table* tables, const int* in_dims, int nt, int D, int64_t batch, int aggr, ffh_stream s) {
  int rc = validate_tables(c, tables, nt, 1, D, batch, aggr, "embedding_fwd_bags");
  if (rc) return rc;
  if (nt > 0 && !in_dims) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_fwd_multi_bags: null in_dims");
  for (int i = 0; i < nt; i++) {
    if (in_dims[i] < 1) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_fwd_multi_bags: in_dims[i] < 1");
    if (in_dims[i] > kBagMaxL) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_fwd_multi_bags: in_dims[i] > FFH_BAGS_MAX_IN_DIM (65535)");
  }
  if (nt == 0 || batch == 0) return FFH_OK;
  constexpr bool b16 = std::is_same<WT, uint16_t>::value;
  int vec = can_vec4(tables, nt, D) ? 4 : 1;
  if (b16) {
    bool ok = D % 4 == 0;
    for (int i = 0; i < nt; i++) ok = ok && ((uintptr_t)tables[i].weight & 7) == 0 && aligned16(tables[i].io) && tables[i].ld % 4 == 0;
    vec = ok ? 4 : 1;
  }
  const int nvec = D / vec;
  if ((nvec + 63) / 64 > kMaxChunks * 64) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_fwd_multi_bags: out_dim too large");
  BagArgs a;
  memset(&a, 0, sizeof a);
  for (int i = 0; i < nt; i++) {
    a.t[i] = tables[i];
    a.L[i] = (uint16_t)in_dims[i];
    // the twin / the image of the destination, under emb_fwd_launch's conditions
    a.out16[i] = (vec >= 4 && tables[i].ld % 4 == 0) ? ffh_mirror_of(c, tables[i].io, (size_t)((batch - 1) * tables[i].ld + D) * 4) : nullptr;
    int col0 = 0;
    a.out3[i] = (vec >= 4 && tables[i].ld % 32 == 0) ? ffh_planes_of(c, tables[i].io, (size_t)((batch - 1) * tables[i].ld + D) * 4, &col0) : nullptr;
    a.out3c[i] = (uint8_t)col0;
    if (a.out3[i] && (col0 & 3)) a.out3[i] = nullptr;
  }
  a.batch = batch; a.ntables = nt; a.D = D; a.aggr = aggr;
  const int lpr = nvec < 64 ? nvec : 64;
  const int rpw = 64 / lpr;
  const int64_t rpb_short = 4LL * rpw * 4, rpb_long = 4LL * rpw * 2;      // bag_rows<.., U = 4 / 2, ..> at 256 threads
  a.nrb[0] = (batch + rpb_short - 1) / rpb_short;
  a.nrb[1] = (batch + rpb_long - 1) / rpb_long;
  // workgroups in proportion to the lookups: the smallest shift at which the tables' shares fit 256 CUs x 8 workgroups
  static const int cap_env = FFH_LAB_INT("FFH_EMB_BAGS_CAP", 2048);      // A/B switch: workgroups over all tables (>= FFH_MAX_TABLES)
  const int64_t cap = cap_env > FFH_MAX_TABLES ? cap_env : FFH_MAX_TABLES;
  int64_t total = 0;
  for (int sh = 0; sh < 63; sh++) {
    total = 0;
    for (int i = 0; i < nt; i++) total += bag_blocks(batch, in_dims[i], sh, a.nrb[in_dims[i] >= kBagLong ? 1 : 0]);
    a.shift = sh;
    if (total <= cap) break;
  }
  if (vec == 4) hipLaunchKernelGGL((emb_fwd_bags_kernel<4, WT>), dim3((unsigned)total), dim3(256), 0, as_stream(s), a);
  else hipLaunchKernelGGL((emb_fwd_bags_kernel<1, WT>), dim3((unsigned)total), dim3(256), 0, as_stream(s), a);
  FFH_LAUNCH_CHECK(c, "emb_fwd_bags_kernel");
  return FFH_OK;
}

extern "C" {

int ffh_embedding_fwd_multi(ffh_ctx* c,const ffh_emb_table* tables, int nt, int L, int D, int64_t batch, int aggr, ffh_stream s) {
  return emb_fwd_launch<float>(c, tables, nt, L, D, batch, aggr, s);
}

int ffh_embedding_fwd(ffh_ctx* c, const int64_t* idx, float* out, const float* weight, int L, int D, int64_t batch,
                      int64_t num_entries, int64_t out_ld, int aggr, ffh_stream s) {
  ffh_emb_table t{idx, const_cast<float*>(weight), out, num_entries, out_ld};
  return ffh_embedding_fwd_multi(c, &t, 1, L, D, batch, aggr, s);
}

int ffh_embedding_bwd_dense(ffh_ctx* c, const int64_t* idx, const float* g, float* wg, int L, int D, int64_t batch,
                            int64_t num_entries, int64_t gld, int aggr, ffh_stream s) {
  ffh_emb_table t{idx, wg, const_cast<float*>(g), num_entries, gld};
  int rc = validate_tables(c, &t, 1, L, D, batch, aggr, "embedding_bwd_dense");
  if (rc) return rc;
  if (batch == 0) return FFH_OK;
  hipLaunchKernelGGL(emb_bwd_dense_kernel, dim3(ffh_grid(batch * D, 256, 4096)), dim3(256), 0, as_stream(s),
                     idx, g, wg, L, D, batch, gld, aggr == FFH_AGGR_MODE_AVG ? 1 : 0);
  FFH_LAUNCH_CHECK(c, "emb_bwd_dense_kernel");
  return FFH_OK;
}

int ffh_embedding_localize_rows(ffh_ctx* c, const int64_t* idx, int64_t* local, int64_t n, int64_t row_begin, int64_t rows_local, ffh_stream s) {
  FFH_REQUIRE(c, n >= 0 && row_begin >= 0 && rows_local >= 0 && ((idx && local) || n == 0), "embedding_localize_rows: bad args");
  if (n == 0) return FFH_OK;
  hipLaunchKernelGGL(emb_localize_kernel, dim3(ffh_grid(n, 256)), dim3(256), 0, as_stream(s), idx, local, n, row_begin, rows_local);
  FFH_LAUNCH_CHECK(c, "embedding_localize_rows");
  return FFH_OK;
}

size_t ffh_embedding_bwd_workspace_bytes(int nt, int L, int D, int64_t batch) {
  if (nt <= 0 || L <= 0 || D <= 0 || batch <= 0) return 0;
  return bwd_layout(nt, L, D, batch).total;
}

// The fused update in two phases: the stable sort of (row id, position) needs the indices only, so a caller that knows them
// early (the DLRM step: at the gather) can run it off the critical path (ffh_embedding_bwd_sort_multi) and do the part that
// needs the output gradients -- segmented reduce, folds, the SGD step -- when they exist (ffh_embedding_bwd_sgd_apply_multi).
// Same launches in the same order on the same workspace: the fused entry is both phases back to back.
// `opt` / `states`: the row rule (ffh_sparse_opt) and the per-table optimizer state it updates; null opt = plain SGD with `lr`
// `b16`: bf16 tables (ff_hip_bf16.h; `tables[i].weight` holds bf16 bits): the rule on uint16_t weight rows (emb_row_rules.h)
struct Bf16Cfg { const ffh_bf16_rounding* r; Bf16Keys keys; };
// the update kernels' translation units, by weight type (emb_reduce.h: the launch table)
typedef bool (*UpdateOfFn)(const UpdateLaunch&);
static constexpr UpdateOfFn kUpdateOf[2] = {emb_update_launch_f32, emb_update_launch_bf16};
// the bf16 keys into a kernel's arguments: beside the s0 / s1 pointers already set (Adam: s1 moves into Bf16AdamKeys)
// (`keys` and `adam` are the same union of the arguments)
static void set_bf16_keys(Bf16Keys& keys, Bf16AdamKeys& adam, const Bf16Cfg& b16, const ffh_emb_state* states, int nt, int kind) {
  if (kind != FFH_SPARSE_OPT_ADAM) { keys = b16.keys; return; }
  Bf16AdamKeys k;
  memset(&k, 0, sizeof k);
  for (int i = 0; i < nt; i++) { k.s1[i] = states[i].s1; k.table[i] = b16.keys.table[i]; k.col0[i] = b16.keys.col0[i]; }
  adam = k;
}
// the stable passes of the sort, one digit of rb bits each: pass p reads buffer p % 2 (pass 0: the int64 ids) and writes buffer (p + 1) % 2
static void launch_sort_passes(SortArgs& sa, uint2* const kbuf[2], int passes, int rb, int E, dim3 sgrid, ffh_stream s) {
  for (int p = 0; p < passes; p++) {
    sa.shift = p * rb;
    sa.pass = p;
    sa.src = kbuf[p & 1];
    sa.dst = kbuf[(p + 1) & 1];
#define FFH_SORT_PASS(FIRSTV, EV)                                                                              \
    hipLaunchKernelGGL((radix_hist_kernel<FIRSTV, EV>), sgrid, dim3(kSortThreads), 0, as_stream(s), sa);      \
    hipLaunchKernelGGL((radix_scatter_kernel<FIRSTV, EV>), sgrid, dim3(kSortThreads), 0, as_stream(s), sa);
    if (p == 0) {
      switch (E) { case 1: FFH_SORT_PASS(true, 1) break; case 2: FFH_SORT_PASS(true, 2) break; case 4: FFH_SORT_PASS(true, 4) break; default: FFH_SORT_PASS(true, 8) break; }
    } else {
      switch (E) { case 1: FFH_SORT_PASS(false, 1) break; case 2: FFH_SORT_PASS(false, 2) break; case 4: FFH_SORT_PASS(false, 4) break; default: FFH_SORT_PASS(false, 8) break; }
    }
#undef FFH_SORT_PASS
  }
}

// The row rule of an update call: its parameters (OptP), its kind and the argument checks that go with them.  Shared by the uniform entries
// (emb_bwd_phases) and the ragged one (emb_bwd_bags).
struct UpdatePlan { OptP op; int kind; RowRule rule; bool v4; int64_t maxR; };
static int emb_update_rule(ffh_ctx* c, int nt, int D, int64_t batch, float lr, const bool do_apply, const ffh_sparse_opt* opt, const ffh_emb_state* states,
                           const Bf16Cfg* b16, const ffh_lr_state* lr_block, UpdatePlan* plan) {
  OptP op{};
  op.lr = lr;
  if (b16 && do_apply) {
    const ffh_bf16_rounding* r = b16->r;
    if (!r) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_bf16: null ffh_bf16_rounding");
    if (r->mode != FFH_BF16_ROUND_STOCHASTIC && r->mode != FFH_BF16_ROUND_NEAREST) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_bf16: unknown rounding mode");
    if (r->mode == FFH_BF16_ROUND_STOCHASTIC && !r->counter) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_bf16: stochastic rounding needs the update counter");
    op.sr_mode = r->mode; op.sr_seed = r->seed; op.sr_counter = r->counter;
  }
  // (round 6) the rows of a table above 64 MB are read and written back NONTEMPORAL by the plain-SGD apply step: a row of such a table is touched once
  // per launch and must not evict the small tables' rows from L2 / Infinity Cache (as in the gather): 26 tables x 32768 lookups 198.0 -> 188.2 us
  // = 0.83 -> 0.875 of 8 TB/s, interleaved on one box; same bits
  op.nt_rows = (int64_t)FFH_LAB_INT("FFH_EMB_APPLY_NT_MB", 64) * (int64_t)(1 << 20) / ((int64_t)D * (b16 ? 2 : 4));      // (bytes, not rows)
  int kind = FFH_SPARSE_OPT_SGD;
  RowRule rule = RowRule::Sgd;
  if (opt && do_apply) {
    kind = opt->kind;
    if (!row_rule_of(kind, &rule)) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt: unknown ffh_sparse_opt.kind");
    if (b16 && (kind == FFH_SPARSE_OPT_SGD_MOMENTUM || kind == FFH_SPARSE_OPT_ADAM) && nt > FFH_BF16_MAX_STATEFUL_TABLES)      // (Adagrad: one state pointer, the Bf16Keys layout)
      return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_multi_bf16: momentum / Adam take at most FFH_BF16_MAX_STATEFUL_TABLES (32) tables per call");
    op.lr = opt->lr; op.wd = opt->weight_decay; op.mom = opt->momentum; op.nesterov = opt->nesterov ? 1 : 0;
    op.b1 = opt->beta1; op.b2 = opt->beta2; op.eps = opt->epsilon; op.omb1 = 1.0f - opt->beta1; op.omb2 = 1.0f - opt->beta2;
    if (kind == FFH_SPARSE_OPT_SGD && (op.wd != 0.0f || op.mom != 0.0f)) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt: FFH_SPARSE_OPT_SGD takes no weight decay / momentum (use FFH_SPARSE_OPT_SGD_MOMENTUM)");
    if (lr_block) { op.lr = 0.0f; opt_set_lr_src(op, ffh_lr_rate_ptr(lr_block, kind == FFH_SPARSE_OPT_ADAM)); }      // (include/ff_hip_lr.h: opt->lr is ignored)
    const bool need0 = kind == FFH_SPARSE_OPT_ADAM || kind == FFH_SPARSE_OPT_ADAGRAD || kind == FFH_SPARSE_OPT_ROWWISE_ADAGRAD || (kind == FFH_SPARSE_OPT_SGD_MOMENTUM && op.mom > 0.0f);
    for (int i = 0; i < nt && batch > 0; i++) {
      if (need0 && (!states || !states[i].s0)) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt: optimizer state (s0) missing");
      if (kind == FFH_SPARSE_OPT_ADAM && !states[i].s1) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt: optimizer state (s1) missing");
    }
  }
  plan->op = op; plan->kind = kind; plan->rule = rule;
  return FFH_OK;
}
// ... and what depends on the tables: the largest row count and whether every row and state row takes the 16-byte form
static int emb_update_form(ffh_ctx* c, const ffh_emb_table* tables, int nt, int D, const ffh_emb_state* states, UpdatePlan* plan) {
  const int kind = plan->kind;
  int64_t maxR = 1;
  for (int i = 0; i < nt; i++) maxR = tables[i].num_entries > maxR ? tables[i].num_entries : maxR;
  if (maxR > (1LL << 32)) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_sgd_fused: num_entries > 2^32");
  bool v4 = can_vec4(tables, nt, D);
  for (int i = 0; i < nt && v4 && kind != FFH_SPARSE_OPT_SGD && kind != FFH_SPARSE_OPT_ROWWISE_ADAGRAD; i++)      // (row-wise: s0 is one float per row, never read as a vector)
    v4 = (!states[i].s0 || aligned16(states[i].s0)) && (kind == FFH_SPARSE_OPT_ADAGRAD || !states[i].s1 || aligned16(states[i].s1));      // (Adagrad: s1 is unused)
  const int nvec = v4 ? D / 4 : D;
  if ((nvec + 63) / 64 > kMaxChunks * 64) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_sgd_fused: out_dim too large");
  if (kind == FFH_SPARSE_OPT_ROWWISE_ADAGRAD && (nvec + 63) / 64 > kMaxChunks)      // (apply_row_rowwise keeps the row in registers)
    return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_opt: FFH_SPARSE_OPT_ROWWISE_ADAGRAD takes out_dim <= 1024 (16-byte form) / 256 (include/ff_hip_rowwise.h)");
  plan->v4 = v4; plan->maxR = maxR;
  return FFH_OK;
}

static int emb_bwd_phases(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int D, int64_t batch,
                          int aggr, float lr, ffh_stream s, const bool do_sort, const bool do_apply,
                          const ffh_sparse_opt* opt = nullptr, const ffh_emb_state* states = nullptr, const Bf16Cfg* b16 = nullptr,
                          const ffh_lr_state* lr_block = nullptr) {
  int rc = validate_tables(c, tables, nt, L, D, batch, aggr, "embedding_bwd_sgd_fused");
  if (rc) return rc;
  UpdatePlan plan;
  rc = emb_update_rule(c, nt, D, batch, lr, do_apply, opt, states, b16, lr_block, &plan);
  if (rc) return rc;
  if (nt == 0 || batch == 0) return FFH_OK;
  const int64_t N = batch * L;
  if (N >= (1LL << 31)) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_sgd_fused: batch*in_dim >= 2^31");
  rc = emb_update_form(c, tables, nt, D, states, &plan);
  if (rc) return rc;
  const OptP& op = plan.op;
  const int kind = plan.kind;
  const RowRule rule = plan.rule;
  const bool v4 = plan.v4;
  const int64_t maxR = plan.maxR;
  const BwdLayout lay = bwd_layout(nt, L, D, batch);
  if (!c->ws || c->ws_bytes < lay.total) return ffh_fail(c, FFH_ERR_WORKSPACE, "embedding_bwd_sgd_fused: workspace too small (ffh_embedding_bwd_workspace_bytes)");
  char* ws = (char*)c->ws;
  if (!aligned16(ws)) return ffh_fail(c, FFH_ERR_WORKSPACE, "embedding_bwd_sgd_fused: workspace must be 16-byte aligned");
  // The apply phase CONSUMES what the sort phase left in the workspace: besides the sorted list, the arrival counters and level-1
  // slots that only the sort's first histogram pass clears -- a second apply on the same sort would find them used (no workgroup
  // would be "last", rows whose runs cross tiles would silently miss their update).  The two-call form is therefore one-shot: the
  // sort notes (workspace, shape) in the ctx, the apply requires and clears that note; the fused call needs no note but spoils one
  // that sits on the workspace it overwrites.
  const int64_t sig[4] = {nt, L, D, batch};
  if (do_sort && do_apply) {
    if (c->emb_sorted_ws == c->ws) c->emb_sorted_ws = nullptr;
  } else if (do_sort) {
    c->emb_sorted_ws = c->ws;
    memcpy(c->emb_sorted_sig, sig, sizeof sig);
  } else {
    if (c->emb_sorted_ws != c->ws || memcmp(c->emb_sorted_sig, sig, sizeof sig) != 0)
      return ffh_fail(c, FFH_ERR_WORKSPACE, "embedding_bwd_sgd_apply_multi: no fresh ffh_embedding_bwd_sort_multi of the same tables / batch on this ctx's "
                                           "workspace (the apply phase consumes the sort: one apply per sort)");
    c->emb_sorted_ws = nullptr;
  }

  if (N <= kSmallMax) {
    // small-batch path: one launch, one workgroup per table (see emb_sgd_small_kernel): the sort lives inside it
    snprintf(c->emb_route, sizeof c->emb_route, "small");
    if (!do_apply) return FFH_OK;
    int bits_s = 1;
    while (bits_s < 32 && ((maxR - 1) >> bits_s) != 0) bits_s++;
    const int passes_s = (bits_s + kMaxRadixBits - 1) / kMaxRadixBits;
    const int rb_s = (bits_s + passes_s - 1) / passes_s;
    SmallArgs sm;
    memset(&sm, 0, sizeof sm);
    for (int i = 0; i < nt; i++) {
      sm.t[i] = tables[i];
      int tb = 1;
      while (tb < 32 && ((tables[i].num_entries - 1) >> tb) != 0) tb++;
      sm.npass[i] = (uint8_t)((tb + rb_s - 1) / rb_s);
    }
    sm.kp = (uint2*)(ws + lay.kp_a);
    sm.partial0 = (float*)(ws + lay.partial); sm.meta0 = (uint2*)(ws + lay.meta);
    sm.partial1 = (float*)(ws + lay.partial1); sm.meta1 = (uint2*)(ws + lay.meta1);
    sm.N = N; sm.nch0 = lay.nchunks; sm.nch1 = lay.nchunks1; sm.rb = rb_s; sm.L = L; sm.D = D;
    sm.avg = aggr == FFH_AGGR_MODE_AVG ? 1 : 0; sm.op = op;
    for (int i = 0; i < nt && kind != FFH_SPARSE_OPT_SGD; i++) { sm.s0[i] = states[i].s0; sm.s1[i] = states[i].s1; }
    if (b16) set_bf16_keys(sm.b16, sm.b16a, *b16, states, nt, kind);
    int tile = (int)((N + kSmallRedParts - 1) / kSmallRedParts);          // one tile per 256-thread team
    tile = (tile + FFH_EMB_CHUNK - 1) / FFH_EMB_CHUNK * FFH_EMB_CHUNK;
    sm.tile = tile < FFH_EMB_CHUNK ? FFH_EMB_CHUNK : tile;
    if (!kUpdateOf[b16 ? 1 : 0](UpdateLaunch{rule, v4, lr_block != nullptr, false, &sm, nullptr, dim3(nt), as_stream(s)}))
      return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd: no small-batch kernel for this rule / weight type");
    FFH_LAUNCH_CHECK(c, "emb_sgd_small_kernel");
    return FFH_OK;
  }
  // radix plan: digits of <= 9 bits covering bit_length(maxR-1); a table only runs the passes its own ids need
  int bits = 1;
  while (bits < 32 && ((maxR - 1) >> bits) != 0) bits++;
  // bucket form (msd_window): one pass on the top digit, the rest inside the apply launch.  Where the LSD form would need >= 2 passes
  // and a bucket averages <= 128 entries (N <= 64 K at 512 buckets); the digit: ~32 entries per bucket, 4 .. 9 bits
  static const int msd_env = FFH_LAB_INT("FFH_EMB_MSD", 1);          // A/B switch: 0 = never, 1 = by shape, 2 = wherever it is valid
  static const int msd_max_tables = FFH_LAB_INT("FFH_EMB_MSD_MAX_TABLES", FFH_MAX_TABLES);      // (first rule: <= 8 tables; at 26 tables x 32768 lookups the form takes 196 instead of 238 us)
  int mb = 4;
  while (mb < kMaxRadixBits && (N >> (mb + 1)) >= 32) mb++;
  const bool msd = msd_env != 0 && bits > kMaxRadixBits && N <= 65536 && (N >> mb) <= 128 && (msd_env == 2 || nt <= msd_max_tables) &&
                   (size_t)lay.nblk * kMaxRadix >= (size_t)lay.nchunks1;
  const int passes = msd ? 1 : (bits + kMaxRadixBits - 1) / kMaxRadixBits;
  const int rb = msd ? mb : (bits + passes - 1) / passes;
  if (msd) snprintf(c->emb_route, sizeof c->emb_route, "buckets:bits=%d", rb); else snprintf(c->emb_route, sizeof c->emb_route, "lsd:passes=%d", passes);

  SortArgs sa;
  memset(&sa, 0, sizeof sa);
  RedArgs ra;
  memset(&ra, 0, sizeof ra);
  for (int i = 0; i < nt; i++) {
    sa.idx[i] = tables[i].idx;
    int tb = 1;
    while (tb < 32 && ((tables[i].num_entries - 1) >> tb) != 0) tb++;
    const int np = msd ? 1 : (tb + rb - 1) / rb;
    sa.npass[i] = (uint8_t)np;
    ra.parity[i] = (uint8_t)(np & 1);
    sa.shift_t[i] = ra.shift_t[i] = (uint8_t)(msd && tb > rb ? tb - rb : 0);
  }
  sa.msd = msd ? 1 : 0;
  sa.bstart = (uint32_t*)(ws + lay.bstart);
  ra.bstart = sa.bstart; ra.nextkey = (uint32_t*)(ws + lay.hist); ra.radix = 1 << rb;
  sa.hist = (uint32_t*)(ws + lay.hist);
  sa.N = N; sa.nblk = lay.nblk; sa.bits = rb;
  sa.clear[0] = (uint32_t*)(ws + lay.meta1); sa.nclear[0] = 4 * lay.nchunks1;     // uint2 slots, two per 1024-block
  sa.clear[1] = (uint32_t*)(ws + lay.arrive); sa.nclear[1] = lay.nchunks1 + 1;
  uint2* kbuf[2] = {(uint2*)(ws + lay.kp_a), (uint2*)(ws + lay.kp_b)};
  dim3 sgrid((unsigned)lay.nblk, (unsigned)nt);
  const int E = sort_per_thread(nt, N);
  if (do_sort) launch_sort_passes(sa, kbuf, passes, rb, E, sgrid, s);
  FFH_LAUNCH_CHECK(c, "radix sort");
  if (!do_apply) return FFH_OK;

  for (int i = 0; i < nt; i++) ra.t[i] = tables[i];
  ra.kp[0] = kbuf[0]; ra.kp[1] = kbuf[1];
  ra.tile = reduce_tile(nt, N);
  {
    static const int msd_tile = FFH_LAB_INT("FFH_EMB_MSD_TILE", 0);      // A/B switch: the bucket form's tile
    if (msd && msd_tile >= 128 && msd_tile <= kRedTile && (msd_tile & (msd_tile - 1)) == 0) ra.tile = msd_tile;
  }
  ra.partial = (float*)(ws + lay.partial);
  ra.meta = (uint2*)(ws + lay.meta);
  ra.N = N; ra.nchunks = lay.nchunks; ra.L = L; ra.D = D;
  ra.avg = aggr == FFH_AGGR_MODE_AVG ? 1 : 0;
  ra.op = op;
  for (int i = 0; i < nt && kind != FFH_SPARSE_OPT_SGD; i++) { ra.s0[i] = states[i].s0; ra.s1[i] = states[i].s1; }
  if (b16) set_bf16_keys(ra.b16, ra.b16a, *b16, states, nt, kind);
  ra.partial1 = (float*)(ws + lay.partial1);
  ra.meta1 = (uint2*)(ws + lay.meta1); ra.nchunks1 = lay.nchunks1;
  ra.arrive = (uint32_t*)(ws + lay.arrive);
  // segmented sums + both folds (32-block partials -> 1024-block partials -> row totals) + the SGD step: one launch
  dim3 rgrid((unsigned)((N + ra.tile - 1) / ra.tile), (unsigned)nt);
  if (!kUpdateOf[b16 ? 1 : 0](UpdateLaunch{rule, v4, lr_block != nullptr, msd, nullptr, &ra, rgrid, as_stream(s)}))
    return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd: no reduce kernel for this rule / weight type");
  FFH_LAUNCH_CHECK(c, "emb_sgd_reduce/fold");
  return FFH_OK;
}

int ffh_embedding_bwd_sgd_fused_multi(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int D, int64_t batch,
                                      int aggr, float lr, ffh_stream s) {
  return emb_bwd_phases(c, tables, nt, L, D, batch, aggr, lr, s, true, true);
}

int ffh_embedding_bwd_sort_multi(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int D, int64_t batch, ffh_stream s) {
  return emb_bwd_phases(c, tables, nt, L, D, batch, FFH_AGGR_MODE_SUM, 0.0f, s, true, false);
}

int ffh_embedding_bwd_sgd_apply_multi(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int D, int64_t batch,
                                      int aggr, float lr, ffh_stream s) {
  return emb_bwd_phases(c, tables, nt, L, D, batch, aggr, lr, s, false, true);
}

int ffh_embedding_bwd_opt_fused_multi(ffh_ctx* c, const ffh_emb_table* tables, const ffh_emb_state* states, int nt, int L, int D, int64_t batch,
                                      int aggr, const ffh_sparse_opt* opt, ffh_stream s) {
  if (!opt) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_fused_multi: null ffh_sparse_opt");
  return emb_bwd_phases(c, tables, nt, L, D, batch, aggr, opt->lr, s, true, true, opt, states);
}

int ffh_embedding_bwd_opt_apply_multi(ffh_ctx* c, const ffh_emb_table* tables, const ffh_emb_state* states, int nt, int L, int D, int64_t batch,
                                      int aggr, const ffh_sparse_opt* opt, ffh_stream s) {
  if (!opt) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_apply_multi: null ffh_sparse_opt");
  return emb_bwd_phases(c, tables, nt, L, D, batch, aggr, opt->lr, s, false, true, opt, states);
}

// include/ff_hip_lr.h: the row rule's rate read from a state block in device memory
int ffh_embedding_bwd_opt_fused_multi_lr(ffh_ctx* c, const ffh_emb_table* tables, const ffh_emb_state* states, int nt, int L, int D, int64_t batch,
                                         int aggr, const ffh_sparse_opt* opt, const ffh_lr_state* block, ffh_stream s) {
  if (!opt || !block) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_fused_multi_lr: null ffh_sparse_opt or ffh_lr_state");
  return emb_bwd_phases(c, tables, nt, L, D, batch, aggr, 0.0f, s, true, true, opt, states, nullptr, block);
}

int ffh_embedding_bwd_opt_apply_multi_lr(ffh_ctx* c, const ffh_emb_table* tables, const ffh_emb_state* states, int nt, int L, int D, int64_t batch,
                                         int aggr, const ffh_sparse_opt* opt, const ffh_lr_state* block, ffh_stream s) {
  if (!opt || !block) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_apply_multi_lr: null ffh_sparse_opt or ffh_lr_state");
  return emb_bwd_phases(c, tables, nt, L, D, batch, aggr, 0.0f, s, false, true, opt, states, nullptr, block);
}

int ffh_embedding_bwd_sgd_fused(ffh_ctx* c, const int64_t* idx, const float* g, float* weight, int L, int D, int64_t batch,
                                int64_t num_entries, int64_t gld, int aggr, float lr, ffh_stream s) {
  ffh_emb_table t{idx, weight, const_cast<float*>(g), num_entries, gld};
  return ffh_embedding_bwd_sgd_fused_multi(c, &t, 1, L, D, batch, aggr, lr, s);
}

}  // extern "C"

// fold_sum.h: the sort alone, complete (no bucket form, no one-launch form), for a caller that reduces the list itself.  Every table runs
// the passes its own ids need; its result lies in buffer (passes % 2).
int ffh_emb::emb_sort_full(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int D, int64_t batch, ffh_stream s, FullSort* out) {
  const int64_t N = batch * L;
  const BwdLayout lay = bwd_layout(nt, L, D, batch);
  char* ws = (char*)c->ws;
  if (c->emb_sorted_ws == c->ws) c->emb_sorted_ws = nullptr;
  int64_t maxR = 1;
  for (int i = 0; i < nt; i++) maxR = tables[i].num_entries > maxR ? tables[i].num_entries : maxR;
  if (maxR > (1LL << 32)) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_segment_sum: num_entries > 2^32");
  int bits = 1;
  while (bits < 32 && ((maxR - 1) >> bits) != 0) bits++;
  const int passes = (bits + kMaxRadixBits - 1) / kMaxRadixBits;
  const int rb = (bits + passes - 1) / passes;
  SortArgs sa;
  memset(&sa, 0, sizeof sa);
  uint2* kbuf[2] = {(uint2*)(ws + lay.kp_a), (uint2*)(ws + lay.kp_b)};
  for (int i = 0; i < nt; i++) {
    sa.idx[i] = tables[i].idx;
    int tb = 1;
    while (tb < 32 && ((tables[i].num_entries - 1) >> tb) != 0) tb++;
    const int np = (tb + rb - 1) / rb;
    sa.npass[i] = (uint8_t)np;
    out->kp[i] = kbuf[np & 1] + (int64_t)i * N;
  }
  sa.bstart = (uint32_t*)(ws + lay.bstart);
  sa.hist = (uint32_t*)(ws + lay.hist);
  sa.N = N; sa.nblk = lay.nblk; sa.bits = rb;
  sa.clear[0] = (uint32_t*)(ws + lay.meta1); sa.clear[1] = (uint32_t*)(ws + lay.arrive);      // (nclear = 0: this caller has no counters to clear)
  launch_sort_passes(sa, kbuf, passes, rb, sort_per_thread(nt, N), dim3((unsigned)lay.nblk, (unsigned)nt), s);
  FFH_LAUNCH_CHECK(c, "radix sort");
  out->partial0 = (float*)(ws + lay.partial);
  out->partial1 = (float*)(ws + lay.partial1);
  out->passes = passes;
  return FFH_OK;
}

// ---------------------------------------------------------------------------
// bf16 tables (include/ff_hip_bf16.h): the fp32 launchers with 16-bit weight rows, the numerics of include/ffh_bf16.h
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void init_uniform_bf16_kernel(uint16_t* __restrict__ p, int64_t n, uint64_t seed, float lo, float hi) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    p[i] = ffh_bf16_rne(ffh_uniform(ffh_hash(seed, (uint64_t)i), lo, hi));
}

__global__ void bf16_counter_advance_kernel(uint64_t* counter) { *counter = *counter + 1; }

// the tables as ffh_emb_table (the weight pointer carries the bf16 bits; the kernels read it through WT) and their keys
static int bf16_tables(ffh_ctx* c, const ffh_emb_table_bf16* in, int nt, ffh_emb_table* out, Bf16Keys* keys) {
  if (nt < 0 || nt > FFH_MAX_TABLES) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bf16: ntables out of range");
  if (nt > 0 && !in) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bf16: null tables");
  for (int i = 0; i < nt; i++) {
    if (in[i].table < 0 || in[i].col0 < 0) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bf16: negative table index or col0");
    out[i] = ffh_emb_table{in[i].idx, reinterpret_cast<float*>(in[i].weight), in[i].io, in[i].num_entries, in[i].ld};
    if (keys) { keys->table[i] = in[i].table; keys->col0[i] = in[i].col0; }
  }
  return FFH_OK;
}

static int emb_bwd_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, int nt, int L, int D, int64_t batch, int aggr, float lr,
                        const ffh_bf16_rounding* r, ffh_stream s, bool do_sort, bool do_apply,
                        const ffh_sparse_opt* opt = nullptr, const ffh_emb_state* states = nullptr, const ffh_lr_state* lr_block = nullptr) {
  ffh_emb_table t[FFH_MAX_TABLES];
  Bf16Cfg cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.r = r;
  const int rc = bf16_tables(c, tables, nt, t, &cfg.keys);
  if (rc) return rc;
  return emb_bwd_phases(c, t, nt, L, D, batch, aggr, lr, s, do_sort, do_apply, opt, states, &cfg, lr_block);
}

extern "C" {

int ffh_bf16_abi_version(void) { return FFH_BF16_ABI_VERSION; }

int ffh_embedding_fwd_multi_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, int nt, int L, int D, int64_t batch, int aggr, ffh_stream s) {
  ffh_emb_table t[FFH_MAX_TABLES];
  const int rc = bf16_tables(c, tables, nt, t, nullptr);
  if (rc) return rc;
  return emb_fwd_launch<uint16_t>(c, t, nt, L, D, batch, aggr, s);
}

int ffh_embedding_bwd_sgd_fused_multi_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, int nt, int L, int D, int64_t batch,
                                           int aggr, float lr, const ffh_bf16_rounding* r, ffh_stream s) {
  return emb_bwd_bf16(c, tables, nt, L, D, batch, aggr, lr, r, s, true, true);
}

int ffh_embedding_bwd_sort_multi_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, int nt, int L, int D, int64_t batch, ffh_stream s) {
  return emb_bwd_bf16(c, tables, nt, L, D, batch, FFH_AGGR_MODE_SUM, 0.0f, nullptr, s, true, false);
}

int ffh_embedding_bwd_sgd_apply_multi_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, int nt, int L, int D, int64_t batch,
                                           int aggr, float lr, const ffh_bf16_rounding* r, ffh_stream s) {
  return emb_bwd_bf16(c, tables, nt, L, D, batch, aggr, lr, r, s, false, true);
}

int ffh_embedding_bwd_opt_fused_multi_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, const ffh_emb_state* states, int nt, int L, int D,
                                           int64_t batch, int aggr, const ffh_sparse_opt* opt, const ffh_bf16_rounding* r, ffh_stream s) {
  if (!opt) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_fused_multi_bf16: null ffh_sparse_opt");
  return emb_bwd_bf16(c, tables, nt, L, D, batch, aggr, opt->lr, r, s, true, true, opt, states);
}

int ffh_embedding_bwd_opt_apply_multi_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, const ffh_emb_state* states, int nt, int L, int D,
                                           int64_t batch, int aggr, const ffh_sparse_opt* opt, const ffh_bf16_rounding* r, ffh_stream s) {
  if (!opt) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_apply_multi_bf16: null ffh_sparse_opt");
  return emb_bwd_bf16(c, tables, nt, L, D, batch, aggr, opt->lr, r, s, false, true, opt, states);
}

int ffh_embedding_bwd_opt_fused_multi_bf16_lr(ffh_ctx* c, const ffh_emb_table_bf16* tables, const ffh_emb_state* states, int nt, int L, int D,
                                              int64_t batch, int aggr, const ffh_sparse_opt* opt, const ffh_bf16_rounding* r, const ffh_lr_state* block,
                                              ffh_stream s) {
  if (!opt || !block) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_fused_multi_bf16_lr: null ffh_sparse_opt or ffh_lr_state");
  return emb_bwd_bf16(c, tables, nt, L, D, batch, aggr, 0.0f, r, s, true, true, opt, states, block);
}

int ffh_embedding_bwd_opt_apply_multi_bf16_lr(ffh_ctx* c, const ffh_emb_table_bf16* tables, const ffh_emb_state* states, int nt, int L, int D,
                                              int64_t batch, int aggr, const ffh_sparse_opt* opt, const ffh_bf16_rounding* r, const ffh_lr_state* block,
                                              ffh_stream s) {
  if (!opt || !block) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_apply_multi_bf16_lr: null ffh_sparse_opt or ffh_lr_state");
  return emb_bwd_bf16(c, tables, nt, L, D, batch, aggr, 0.0f, r, s, false, true, opt, states, block);
}

int ffh_init_uniform_bf16(ffh_ctx* c, uint16_t* p, int64_t n, uint64_t seed, float lo, float hi, ffh_stream s) {
  FFH_REQUIRE(c, n >= 0 && (p || n == 0), "init_uniform_bf16: bad args");
  if (n == 0) return FFH_OK;
  hipLaunchKernelGGL(init_uniform_bf16_kernel, dim3(ffh_grid(n, 256, 8192)), dim3(256), 0, as_stream(s), p, n, seed, lo, hi);
  FFH_LAUNCH_CHECK(c, "init_uniform_bf16");
  return FFH_OK;
}

int ffh_bf16_counter_advance(ffh_ctx* c, uint64_t* counter, ffh_stream s) {
  FFH_REQUIRE(c, counter != nullptr, "bf16_counter_advance: null counter");
  hipLaunchKernelGGL(bf16_counter_advance_kernel, dim3(1), dim3(1), 0, as_stream(s), counter);
  FFH_LAUNCH_CHECK(c, "bf16_counter_advance");
  return FFH_OK;
}

int ffh_rowwise_abi_version(void) { return FFH_ROWWISE_ABI_VERSION; }      // include/ff_hip_rowwise.h: the row rule lives in this file

// include/ff_hip_bags.h: the gather with a bag size per table
int ffh_bags_abi_version(void) { return FFH_BAGS_ABI_VERSION; }
size_t ffh_bags_kernarg_bytes(void) { return sizeof(BagArgs); }

int ffh_embedding_fwd_multi_bags(ffh_ctx* c, const ffh_emb_table* tables, const int* in_dims, int nt, int D, int64_t batch, int aggr, ffh_stream s) {
  return emb_fwd_bags_launch<float>(c, tables, in_dims, nt, D, batch, aggr, s);
}

int ffh_embedding_fwd_multi_bags_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, const int* in_dims, int nt, int D, int64_t batch, int aggr, ffh_stream s) {
  ffh_emb_table t[FFH_MAX_TABLES];
  const int rc = bf16_tables(c, tables, nt, t, nullptr);
  if (rc) return rc;
  return emb_fwd_bags_launch<uint16_t>(c, t, in_dims, nt, D, batch, aggr, s);
}

}  // extern "C"
// ---------------------------------------------------------------------------
// include/ff_hip_bags_update.h: the fused update with a bag size per table.  One call, the kernels of emb_bags_update.h.
// ---------------------------------------------------------------------------
namespace {

// The workspace: bwd_layout's arrays with every table's share sized by its own N_t = batch * L_t (with equal bag sizes: bwd_layout's bytes).
// `bstart` keeps the place of the bucket form's array, which no ragged kernel uses yet.
struct BagsLayout {
  size_t kp_a, kp_b, hist, partial, meta, partial1, meta1, arrive, bstart, total;
  BagsGeo g;           // (sort_sh and red_sh set: the tiles the call runs with)
  BagsAt tot;          // totals over the tables; tot.local = reduce tiles
  int64_t sort_tiles, maxN;
  int E;
};

inline int log2_of(int v) { int s = 0; while ((1 << s) < v) s++; return s; }

// in_dims checked by the caller: 1 .. kBagMaxL, batch * in_dims[i] < 2^31
inline BagsLayout bags_layout(const int* in_dims, int nt, int D, int64_t batch) {
  BagsLayout l;
  memset(&l, 0, sizeof l);
  int64_t total = 0, maxN = 0;
  for (int i = 0; i < nt; i++) {
    l.g.L[i] = (uint16_t)in_dims[i];
    const int64_t N = batch * in_dims[i];
    total += N;
    maxN = N > maxN ? N : maxN;
  }
  l.g.batch = batch; l.g.nt = nt;
  l.maxN = maxN;
  // sort_per_thread / reduce_tile on the call's lookups: enough workgroups to cover the chip, tiles as large as that allows
  int e = 1;
  while (e * 2 <= total / (512LL * kSortThreads) && e < kSortMaxPerThread) e *= 2;
  while ((maxN + (int64_t)kSortThreads * e - 1) / ((int64_t)kSortThreads * e) > 32 && e < kSortMaxPerThread) e *= 2;
  l.E = e;
  l.g.sort_sh = log2_of(kSortThreads * e);
  int t = 128;
  while (t * 2 <= total / 1024 && t < kRedTile) t *= 2;
  l.g.red_sh = log2_of(t);
  bags_locate(l.g, l.g.red_sh, INT64_MAX, &l.tot);
  l.sort_tiles = l.tot.sblk0;
  const size_t arr = align_up((size_t)l.tot.key0 * sizeof(uint2), 256);
  size_t o = 0;
  l.kp_a = o; o += arr;
  l.kp_b = o; o += arr;
  l.hist = o; o += align_up((size_t)l.tot.sblk0 * kMaxRadix * sizeof(uint32_t), 256);
  l.partial = o; o += align_up(2 * (size_t)l.tot.ch0 * (size_t)D * sizeof(float), 256);
  l.meta = o; o += align_up(2 * (size_t)l.tot.ch0 * sizeof(uint2), 256);
  l.partial1 = o; o += align_up(2 * (size_t)l.tot.ch1 * (size_t)D * sizeof(float), 256);
  l.meta1 = o; o += align_up(2 * (size_t)l.tot.ch1 * sizeof(uint2), 256);
  l.arrive = o; o += align_up(((size_t)l.tot.ch1 + (size_t)nt) * sizeof(uint32_t), 256);
  l.bstart = o; o += align_up((size_t)nt * (kMaxRadix + 1) * sizeof(uint32_t), 256);
  l.total = o;
  return l;
}

// FFH_OK, or the code the entry returns for these bag sizes (no message: the callers add their own)
inline int bags_dims_check(const int* in_dims, int nt, int64_t batch) {
  if (nt < 0 || nt > FFH_BAGS_UPDATE_MAX_TABLES || (nt > 0 && !in_dims) || batch < 0) return FFH_ERR_BAD_ARG;
  for (int i = 0; i < nt; i++)
    if (in_dims[i] < 1) return FFH_ERR_BAD_ARG;
  for (int i = 0; i < nt; i++) {
    if (in_dims[i] > kBagMaxL) return FFH_ERR_UNSUPPORTED;
    if (batch * (int64_t)in_dims[i] >= (1LL << 31)) return FFH_ERR_UNSUPPORTED;
  }
  return FFH_OK;
}

typedef bool (*BagsUpdateOfFn)(const BagsUpdateLaunch&);
constexpr BagsUpdateOfFn kBagsUpdateOf[2] = {emb_bags_update_launch_f32, emb_bags_update_launch_bf16};

int emb_bwd_bags(ffh_ctx* c, const ffh_emb_table* tables, const int* in_dims, int nt, int D, int64_t batch, int aggr, float lr, ffh_stream s,
                 const ffh_sparse_opt* opt, const ffh_emb_state* states, const Bf16Cfg* b16, const ffh_lr_state* lr_block) {
  int rc = bags_dims_check(in_dims, nt, batch);
  if (rc == FFH_ERR_BAD_ARG) return ffh_fail(c, rc, "embedding_bwd_fused_multi_bags: ntables out of range, null in_dims or in_dims[i] < 1");
  if (rc) return ffh_fail(c, rc, "embedding_bwd_fused_multi_bags: in_dims[i] > FFH_BAGS_MAX_IN_DIM (65535) or batch*in_dims[i] >= 2^31");
  rc = validate_tables(c, tables, nt, 1, D, batch, aggr, "embedding_bwd_fused_multi_bags");
  if (rc) return rc;
  UpdatePlan plan;
  rc = emb_update_rule(c, nt, D, batch, lr, true, opt, states, b16, lr_block, &plan);
  if (rc) return rc;
  if (nt == 0 || batch == 0) return FFH_OK;
  rc = emb_update_form(c, tables, nt, D, states, &plan);
  if (rc) return rc;
  const int kind = plan.kind;
  const BagsLayout lay = bags_layout(in_dims, nt, D, batch);
  if (!c->ws || c->ws_bytes < lay.total) return ffh_fail(c, FFH_ERR_WORKSPACE, "embedding_bwd_fused_multi_bags: workspace too small (ffh_embedding_bwd_bags_workspace_bytes)");
  char* ws = (char*)c->ws;
  if (!aligned16(ws)) return ffh_fail(c, FFH_ERR_WORKSPACE, "embedding_bwd_fused_multi_bags: workspace must be 16-byte aligned");
  if (c->emb_sorted_ws == c->ws) c->emb_sorted_ws = nullptr;      // (as the uniform fused call: a pending sort on this workspace is overwritten)

  int bits = 1;
  while (bits < 32 && ((plan.maxR - 1) >> bits) != 0) bits++;
  const int passes = (bits + kMaxRadixBits - 1) / kMaxRadixBits;
  const int rb = (bits + passes - 1) / passes;
  const int avg = aggr == FFH_AGGR_MODE_AVG ? 1 : 0;

  if (lay.maxN <= kSmallMax) {
    snprintf(c->emb_route, sizeof c->emb_route, "bags:small");
    BagsSmallArgs sm;
    memset(&sm, 0, sizeof sm);
    for (int i = 0; i < nt; i++) {
      sm.t[i] = tables[i];
      int tb = 1;
      while (tb < 32 && ((tables[i].num_entries - 1) >> tb) != 0) tb++;
      sm.npass[i] = (uint8_t)((tb + rb - 1) / rb);
    }
    sm.kp = (uint2*)(ws + lay.kp_a);
    sm.partial0 = (float*)(ws + lay.partial); sm.meta0 = (uint2*)(ws + lay.meta);
    sm.partial1 = (float*)(ws + lay.partial1); sm.meta1 = (uint2*)(ws + lay.meta1);
    sm.rb = rb; sm.D = D; sm.avg = avg; sm.g = lay.g; sm.op = plan.op;
    for (int i = 0; i < nt && kind != FFH_SPARSE_OPT_SGD; i++) { sm.s0[i] = states[i].s0; sm.s1[i] = states[i].s1; }
    if (b16) set_bf16_keys(sm.b16, sm.b16a, *b16, states, nt, kind);
    if (!kBagsUpdateOf[b16 ? 1 : 0](BagsUpdateLaunch{plan.rule, plan.v4, lr_block != nullptr, &sm, nullptr, dim3((unsigned)nt), as_stream(s)}))
      return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_fused_multi_bags: no small-route kernel for this rule / weight type");
    FFH_LAUNCH_CHECK(c, "emb_bags_small_kernel");
    return FFH_OK;
  }

  snprintf(c->emb_route, sizeof c->emb_route, "bags:lsd:passes=%d", passes);
  BagsSortArgs sa;
  memset(&sa, 0, sizeof sa);
  BagsRedArgs ra;
  memset(&ra, 0, sizeof ra);
  for (int i = 0; i < nt; i++) {
    sa.idx[i] = tables[i].idx;
    int tb = 1;
    while (tb < 32 && ((tables[i].num_entries - 1) >> tb) != 0) tb++;
    const int np = (tb + rb - 1) / rb;
    sa.npass[i] = (uint8_t)np;
    ra.parity[i] = (uint8_t)(np & 1);
    ra.t[i] = tables[i];
  }
  sa.hist = (uint32_t*)(ws + lay.hist);
  sa.bits = rb; sa.g = lay.g;
  sa.clear[0] = (uint32_t*)(ws + lay.meta1); sa.nclear[0] = (int)(4 * lay.tot.ch1);      // uint2 slots, two per 1024-block
  sa.clear[1] = (uint32_t*)(ws + lay.arrive); sa.nclear[1] = (int)(lay.tot.ch1 + nt);
  uint2* kbuf[2] = {(uint2*)(ws + lay.kp_a), (uint2*)(ws + lay.kp_b)};
  const dim3 sgrid((unsigned)lay.sort_tiles), rgrid((unsigned)lay.tot.local);      // the flat map: every table's own tiles
  for (int p = 0; p < passes; p++) {
    sa.shift = p * rb; sa.pass = p;
    sa.src = kbuf[p & 1]; sa.dst = kbuf[(p + 1) & 1];
    if (!emb_bags_sort_pass(sa, p == 0, lay.E, sgrid, as_stream(s))) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_fused_multi_bags: no sort kernel");
  }
  FFH_LAUNCH_CHECK(c, "bags radix sort");

  ra.kp[0] = kbuf[0]; ra.kp[1] = kbuf[1];
  ra.partial = (float*)(ws + lay.partial); ra.meta = (uint2*)(ws + lay.meta);
  ra.partial1 = (float*)(ws + lay.partial1); ra.meta1 = (uint2*)(ws + lay.meta1);
  ra.arrive = (uint32_t*)(ws + lay.arrive);
  ra.D = D; ra.avg = avg; ra.g = lay.g; ra.op = plan.op;
  for (int i = 0; i < nt && kind != FFH_SPARSE_OPT_SGD; i++) { ra.s0[i] = states[i].s0; ra.s1[i] = states[i].s1; }
  if (b16) set_bf16_keys(ra.b16, ra.b16a, *b16, states, nt, kind);
  if (!kBagsUpdateOf[b16 ? 1 : 0](BagsUpdateLaunch{plan.rule, plan.v4, lr_block != nullptr, nullptr, &ra, rgrid, as_stream(s)}))
    return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_fused_multi_bags: no reduce kernel for this rule / weight type");
  FFH_LAUNCH_CHECK(c, "emb_bags_reduce/fold");
  return FFH_OK;
}

}  // namespace

extern "C" {

int ffh_bags_update_abi_version(void) { return FFH_BAGS_UPDATE_ABI_VERSION; }
size_t ffh_bags_update_kernarg_bytes(void) { return kBagsKernargBytes; }

size_t ffh_embedding_bwd_bags_workspace_bytes(const int* in_dims, int nt, int D, int64_t batch) {
  if (nt <= 0 || D <= 0 || batch <= 0 || bags_dims_check(in_dims, nt, batch) != FFH_OK) return 0;
  return bags_layout(in_dims, nt, D, batch).total;
}

int ffh_embedding_bwd_fused_multi_bags(ffh_ctx* c, const ffh_bags_update* u, ffh_stream s) {
  if (!u) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_fused_multi_bags: null descriptor");
  if ((u->tables != nullptr) == (u->tables_bf16 != nullptr)) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_fused_multi_bags: exactly one of tables / tables_bf16");
  if (u->lr_block && !u->opt) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_fused_multi_bags: lr_block needs opt");
  if (u->tables) return emb_bwd_bags(c, u->tables, u->in_dims, u->ntables, u->out_dim, u->batch, u->aggr, u->lr, s, u->opt, u->states, nullptr, u->lr_block);
  ffh_emb_table t[FFH_MAX_TABLES];
  Bf16Cfg cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.r = u->rounding;
  const int rc = bf16_tables(c, u->tables_bf16, u->ntables, t, &cfg.keys);
  if (rc) return rc;
  return emb_bwd_bags(c, t, u->in_dims, u->ntables, u->out_dim, u->batch, u->aggr, u->lr, s, u->opt, u->states, &cfg, u->lr_block);
}

}  // extern "C"
static_assert(sizeof(EmbArgs) <= 4096, "kernel arguments");
static_assert(kBagMaxL == FFH_BAGS_MAX_IN_DIM, "include/ff_hip_bags.h");
