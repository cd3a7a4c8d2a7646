// embedding_fwd.hip -- Embedding forward (gather + bag-sum), hand-written for gfx950.
//
// HBM-bound integer/byte work.  Design rules applied:
//   * a table row is read by `D/4` adjacent lanes with one 16-B load each, so a
//     wave-instruction covers 64/(D/4) whole rows (512-B rows: two per instruction,
//     64-B rows: sixteen) -- full-line coalesced reads and writes;
//   * every lane-group keeps several independent row loads in flight (UNROLL);
//   * all tables of a model go in ONE launch instead of the reference's one task per table;
//   * 64-bit addressing everywhere (a 200M x 256 table is 204.8 GB; the reference's
//     `int outputSize` [ref: src/ops/embedding.cu:226,229] would overflow).
// What is here:
//   * emb_fwd_kernel: one bag size for all tables (grid.y = table);
//   * emb_fwd_bags_kernel: a bag size per table (include/ff_hip_bags.h), a flat grid; its PAD form skips ids < 0 (include/ff_hip_pad.h), its
//     MEAN form also divides by the count of the ids it did not skip (include/ff_hip_pad_mean.h);
//   * gather_form: the 16-byte form, on the host, for both launchers; the entries
//     ffh_embedding_fwd*, fp32 and bf16 tables.
//   * RowLanes: the lane geometry of both kernels;
// What is where: store_row (the store epilogue of both kernels), bag_blocks and gather_dests
// (every destination's twin / image) are emb_gather.h, shared with the gather from 8-bit rows
// (embedding_q8.hip); the table update, the dense backward and the
// bf16 helpers are embedding.hip; the checks on a table list shared with them are emb_tables.h.
#include "emb_gather.h"
#include "../../include/ff_hip_pad_mean.h"

#include <type_traits>

namespace {

using namespace ffh_emb;

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

// How a wave covers rows of D elements, `vec` per lane per access; the host sizes its grids with the first three.
struct RowLanes {
  int nvec;        // vectors per row
  int lpr;         // lanes per row
  int rpw;         // rows per wave-instruction
  int rsub;        // which of the wave's rows lane `lane` works on ...
  int c0;          // ... and its first vector of that row
  bool active;
  __host__ __device__ RowLanes(int D, int vec, int lane = 0) {
    nvec = D / vec;
    lpr = nvec < 64 ? nvec : 64;
    rpw = 64 / lpr;
    rsub = lane / lpr;
    c0 = lane - rsub * lpr;
    active = rsub < rpw;
  }
  // rows a 256-thread workgroup takes per trip with U rows in flight per lane-group
  __host__ __device__ int64_t block_rows(int U) const { return 4LL * rpw * U; }
};

// ---------------------------------------------------------------------------
// forward: out[b][:] = sum_j W[idx[b][j]][:]
// ---------------------------------------------------------------------------
struct EmbArgs {
  ffh_emb_table t[FFH_MAX_TABLES];
  unsigned short* out16[FFH_MAX_TABLES];   // forward, tensor-op mode: bf16 twin of t[i].io (same leading dimension) or null
  char* out3[FFH_MAX_TABLES];              // forward, split mode: the I32 image group that holds t[i].io[0] (ffh_ctx_bf16x3_mirror_set) or null ...
  int   out3c[FFH_MAX_TABLES];             // ... and that element's position in its group
  int64_t batch;
  int     ntables, L, D, aggr;
  int64_t nt_rows;      // tables of more rows: the 16-byte row loads carry a nontemporal hint, which the compiler drops (emb_fwd_launch)
};
static_assert(sizeof(EmbArgs) <= 4096, "kernel arguments");

template <int VEC, int UNROLL, class WT = float>
__global__ __launch_bounds__(256) void emb_fwd_kernel(const EmbArgs a) {
  ffh_kernel_prio();
  using vec_t = typename RowVec<VEC, WT>::type;
  const ffh_emb_table tb = a.t[blockIdx.y];
  const WT* const wt = reinterpret_cast<const WT*>(tb.weight);
  unsigned short* const o16 = a.out16[blockIdx.y];
  char* const o3 = a.out3[blockIdx.y];
  const int o3c = a.out3c[blockIdx.y];
  const int D = a.D, L = a.L;
  const RowLanes g(D, VEC, threadIdx.x & 63);
  const int wave = threadIdx.x >> 6;
  const int64_t rows_per_block = (int64_t)(blockDim.x >> 6) * g.rpw * UNROLL;
  const float inv = 1.0f / (float)L;
  const bool avg = a.aggr == FFH_AGGR_MODE_AVG;

  for (int64_t base = (int64_t)blockIdx.x * rows_per_block; base < a.batch; base += (int64_t)gridDim.x * rows_per_block) {
    const int64_t b0 = base + (int64_t)wave * g.rpw * UNROLL + g.rsub;
    for (int c = g.c0; c < g.nvec; c += g.lpr) {
      float acc[UNROLL][VEC];
#pragma unroll
      for (int u = 0; u < UNROLL; u++)
#pragma unroll
        for (int v = 0; v < VEC; v++) acc[u][v] = 0.0f;
      for (int j = 0; j < L; j++) {
        int64_t row[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
          const int64_t b = b0 + (int64_t)u * g.rpw;
          row[u] = (g.active && b < a.batch) ? tb.idx[b * L + j] : -1;
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
        const int64_t b = b0 + (int64_t)u * g.rpw;
        if (g.active && b < a.batch) store_row<VEC>(tb, o16, o3, o3c, b, c, acc[u], avg, inv);
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
struct BagArgs {
  ffh_emb_table t[FFH_MAX_TABLES];
  unsigned short* out16[FFH_MAX_TABLES];   // as EmbArgs::out16
  char* out3[FFH_MAX_TABLES];              // as EmbArgs::out3 ...
  uint16_t L[FFH_MAX_TABLES];              // bag size of table i (<= kBagMaxL)
  uint8_t  out3c[FFH_MAX_TABLES];          // ... and EmbArgs::out3c (0 .. 31)
  int64_t batch;
  int64_t nrb[2];        // row blocks of the batch: [0] short bags (U = 4), [1] long bags (U = 2)
  int     ntables, D, aggr;
  int     shift;        // workgroups of table i = clamp((batch * L[i]) >> shift, 1, nrb)
};
static_assert(sizeof(BagArgs) <= sizeof(EmbArgs) && sizeof(BagArgs) <= 4096, "kernel arguments");

// the rows [first, first + step, ...) x rows_per_block of table t; U rows x JU ids in flight per lane-group
// PAD (include/ff_hip_pad.h): an id < 0 is no lookup.  The id is the same in the lanes that share a row and differs between the row groups of a
// wave, so the row load and the add are predicated on it beside ok[u], not branched around; acc keeps its +0 where nothing is added.
// MEAN (include/ff_hip_pad_mean.h; PAD forms only): the lanes that share a row count its ids >= 0 where the add is predicated, and the row is
// stored times 1 / max(count, 1) -- store_row's AVG epilogue with a divisor per row.  With PAD or MEAN false the kernel is what it was.
template <int VEC, int U, int JU, class WT, bool PAD = false, bool MEAN = false>
__device__ __forceinline__ void bag_rows(const BagArgs& a, const int t, const int64_t first, const int64_t step) {
  using vec_t = typename RowVec<VEC, WT>::type;
  const ffh_emb_table tb = a.t[t];
  const WT* const wt = reinterpret_cast<const WT*>(tb.weight);
  unsigned short* const o16 = a.out16[t];
  char* const o3 = a.out3[t];
  const int o3c = a.out3c[t];
  const int D = a.D, L = a.L[t];
  const RowLanes g(D, VEC, threadIdx.x & 63);
  const int wave = threadIdx.x >> 6;
  const int64_t rows_per_block = g.block_rows(U);
  const float inv = 1.0f / (float)L;
  const bool avg = a.aggr == FFH_AGGR_MODE_AVG;

  for (int64_t base = first * rows_per_block; base < a.batch; base += step * rows_per_block) {
    const int64_t b0 = base + (int64_t)wave * g.rpw * U + g.rsub;
    bool ok[U];
    const int64_t* ids[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t b = b0 + (int64_t)u * g.rpw;
      ok[u] = g.active && b < a.batch;
      ids[u] = tb.idx + b * L;
    }
    for (int c = g.c0; c < g.nvec; c += g.lpr) {
      float acc[U][VEC];
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int v = 0; v < VEC; v++) acc[u][v] = 0.0f;
      int live[U];      // (MEAN: the row's lookups that are there)
#pragma unroll
      for (int u = 0; u < U; u++) live[u] = 0;
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
              if (PAD ? ok[u] && row[u][k] >= 0 : ok[u]) val[u][k] = *(reinterpret_cast<const vec_t*>(wt + row[u][k] * (int64_t)D) + c);
#pragma unroll
          for (int u = 0; u < U; u++)
            if (ok[u]) {
#pragma unroll
              for (int k = 0; k < JU; k++)           // ascending j: the order of emb_fwd_kernel
                if (!PAD || row[u][k] >= 0) {
#pragma unroll
                  for (int v = 0; v < VEC; v++) acc[u][v] = acc[u][v] + row_elem<VEC, WT>(val[u][k], v);
                  if constexpr (MEAN) live[u]++;
                }
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
          if (PAD ? ok[u] && row[u] >= 0 : ok[u]) val[u] = *(reinterpret_cast<const vec_t*>(wt + row[u] * (int64_t)D) + c);
#pragma unroll
        for (int u = 0; u < U; u++)
          if (PAD ? ok[u] && row[u] >= 0 : ok[u]) {
#pragma unroll
            for (int v = 0; v < VEC; v++) acc[u][v] = acc[u][v] + row_elem<VEC, WT>(val[u], v);   // 0 + w first, as emb_fwd_kernel
            if constexpr (MEAN) live[u]++;
          }
      }
#pragma unroll
      for (int u = 0; u < U; u++)
        if (ok[u]) {
          if constexpr (MEAN) store_row<VEC>(tb, o16, o3, o3c, b0 + (int64_t)u * g.rpw, c, acc[u], true, 1.0f / (float)(live[u] > 1 ? live[u] : 1));
          else store_row<VEC>(tb, o16, o3, o3c, b0 + (int64_t)u * g.rpw, c, acc[u], avg, inv);
        }
    }
  }
}

template <int VEC, class WT, bool PAD = false, bool MEAN = false>
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
  if (a.L[t] >= kBagLong) bag_rows<VEC, 2, 4, WT, PAD, MEAN>(a, t, first, w);
  else bag_rows<VEC, 4, 1, WT, PAD, MEAN>(a, t, first, w);
}

// ---- host side, both launchers.  WT = float: fp32 tables; WT = uint16_t: `tables[i].weight` holds bf16 bits. ----
// The form of a call, *vec = 4 or 1: the 16-byte form where every table and destination row allows it, so a table's bits are those of
// its own call wherever that call takes the same form (all tables aligned alike, or D % 4 != 0).
template <class WT>
int gather_form(ffh_ctx* c, const ffh_emb_table* tables, int nt, int D, const char* too_large, int* vec) {
  bool v4 = can_vec4(tables, nt, D);
  if (std::is_same<WT, uint16_t>::value) {
    // 4 bf16 per 8-B access, the output side as in the fp32 form.  (8 per 16-B access -- the lanes per row halved, the same bytes in
    // flight per wave -- was measured at the Terabyte shape and was slower: 107 VGPRs, occupancy 4, 163 against 146 us; UNROLL 2
    // did not help. profiles/bf16_table_bench.txt)
    v4 = D % 4 == 0;
    for (int i = 0; i < nt; i++) v4 = v4 && ((uintptr_t)tables[i].weight & 7) == 0 && aligned16(tables[i].io) && tables[i].ld % 4 == 0;
  }
  *vec = v4 ? 4 : 1;
  if ((D / *vec + 63) / 64 > kMaxChunks * 64) return ffh_fail(c, FFH_ERR_UNSUPPORTED, too_large);
  return FFH_OK;
}

template <class WT>
int emb_fwd_launch(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int D, int64_t batch, int aggr, ffh_stream s) {
  int rc = validate_tables(c, tables, nt, L, D, batch, aggr);
  if (rc) return rc;
  if (nt == 0 || batch == 0) return FFH_OK;
  int vec;
  rc = gather_form<WT>(c, tables, nt, D, "embedding_fwd: out_dim too large", &vec);
  if (rc) return rc;
  EmbArgs a;
  memset(&a, 0, sizeof a);
  gather_dests(c, tables, nt, D, batch, vec, a);
  a.batch = batch; a.ntables = nt; a.L = L; a.D = D; a.aggr = aggr;
  // Cache policy (round 6): the output is written once and read much later by a GEMM -- 436 MB per launch at the Terabyte shape, more than the
  // Infinity Cache holds -- and a row of a table too big to stay cached is touched once per launch: both as NONTEMPORAL accesses, so that they do
  // not evict the rows of the 18 small tables (62 MB) that do live in L2 / Infinity Cache.  One box, interleaved: 139.4 -> 133.7 (stores) / 133.8
  // (loads) / 130.9 us (both) = 0.79 -> 0.84 of 8 TB/s by the algorithmic-bytes formula; the step unchanged.  Same bits.
  // As compiled, neither hint survives: the compiler merged each hinted access with its plain twin and dropped the hint, so the
  // kernel's loads and stores are plain.  The stores are now written plain; making the policy real is a change of its own, to be measured.
  a.nt_rows = (int64_t)FFH_LAB_INT("FFH_EMB_NT_MB", 64) * (1 << 20) / ((int64_t)D * (int64_t)sizeof(WT));      // tables above 64 MB (bytes, not rows)
  constexpr int U = 4;
  const int64_t rows_per_block = RowLanes(D, vec).block_rows(U);
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

template <class WT, bool PAD = false, bool MEAN = false>
int emb_fwd_bags_launch(ffh_ctx* c, const ffh_emb_table* tables, const int* in_dims, int nt, int D, int64_t batch, int aggr, ffh_stream s) {
  int rc = validate_tables(c, tables, nt, 1, D, batch, aggr);
  if (rc) return rc;
  if (PAD && !MEAN && aggr == FFH_AGGR_MODE_AVG)      // (a mean over the lookups that are there needs each bag's count: include/ff_hip_pad_mean.h)
    return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_fwd_multi_bags_pad: FFH_AGGR_MODE_AVG is not supported with pad ids");
  if (MEAN && aggr != FFH_AGGR_MODE_AVG)
    return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_fwd_multi_bags_pad_mean: aggr must be FFH_AGGR_MODE_AVG (for a sum call ffh_embedding_fwd_multi_bags_pad)");
  if (nt > 0 && !in_dims) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_fwd_multi_bags: null in_dims");
  for (int i = 0; i < nt; i++) {
    if (in_dims[i] < 1) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_fwd_multi_bags: in_dims[i] < 1");
    if (in_dims[i] > kBagMaxL) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_fwd_multi_bags: in_dims[i] > FFH_BAGS_MAX_IN_DIM (65535)");
  }
  if (nt == 0 || batch == 0) return FFH_OK;
  int vec;
  rc = gather_form<WT>(c, tables, nt, D, "embedding_fwd_multi_bags: out_dim too large", &vec);
  if (rc) return rc;
  BagArgs a;
  memset(&a, 0, sizeof a);
  gather_dests(c, tables, nt, D, batch, vec, a);
  for (int i = 0; i < nt; i++) a.L[i] = (uint16_t)in_dims[i];
  a.batch = batch; a.ntables = nt; a.D = D; a.aggr = aggr;
  const RowLanes g(D, vec);
  const int64_t rpb_short = g.block_rows(4), rpb_long = g.block_rows(2);      // bag_rows<.., U = 4 / 2, ..>
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
  if (vec == 4) hipLaunchKernelGGL((emb_fwd_bags_kernel<4, WT, PAD, MEAN>), dim3((unsigned)total), dim3(256), 0, as_stream(s), a);
  else hipLaunchKernelGGL((emb_fwd_bags_kernel<1, WT, PAD, MEAN>), dim3((unsigned)total), dim3(256), 0, as_stream(s), a);
  FFH_LAUNCH_CHECK(c, "emb_fwd_bags_kernel");
  return FFH_OK;
}

}  // namespace

extern "C" {

int ffh_embedding_fwd_multi(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int D, int64_t batch, int aggr, ffh_stream s) {
  return emb_fwd_launch<float>(c, tables, nt, L, D, batch, aggr, s);
}

int ffh_embedding_fwd(ffh_ctx* c, const int64_t* idx, float* out, const float* weight, int L, int D, int64_t batch,
                      int64_t num_entries, int64_t out_ld, int aggr, ffh_stream s) {
  ffh_emb_table t{idx, const_cast<float*>(weight), out, num_entries, out_ld};
  return ffh_embedding_fwd_multi(c, &t, 1, L, D, batch, aggr, s);
}

int ffh_embedding_fwd_multi_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, int nt, int L, int D, int64_t batch, int aggr, ffh_stream s) {
  ffh_emb_table t[FFH_MAX_TABLES];
  const int rc = bf16_tables(c, tables, nt, t, nullptr);
  if (rc) return rc;
  return emb_fwd_launch<uint16_t>(c, t, nt, L, D, batch, aggr, s);
}

// include/ff_hip_bags.h: the gather with a bag size per table
int ffh_bags_abi_version(void) { return FFH_BAGS_ABI_VERSION; }
size_t ffh_bags_kernarg_bytes(void) { return sizeof(BagArgs); }

int ffh_embedding_fwd_multi_bags(ffh_ctx* c, const ffh_emb_table* tables, const int* in_dims, int nt, int D, int64_t batch, int aggr, ffh_stream s) {
  return emb_fwd_bags_launch<float>(c, tables, in_dims, nt, D, batch, aggr, s);
}

int ffh_embedding_fwd_multi_bags_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, const int* in_dims, int nt, int D, int64_t batch, int aggr,
                                      ffh_stream s) {
  ffh_emb_table t[FFH_MAX_TABLES];
  const int rc = bf16_tables(c, tables, nt, t, nullptr);
  if (rc) return rc;
  return emb_fwd_bags_launch<uint16_t>(c, t, in_dims, nt, D, batch, aggr, s);
}

// include/ff_hip_pad.h: the ragged gather in which an id < 0 is no lookup
int ffh_embedding_fwd_multi_bags_pad(ffh_ctx* c, const ffh_emb_table* tables, const int* in_dims, int nt, int D, int64_t batch, int aggr, ffh_stream s) {
  return emb_fwd_bags_launch<float, true>(c, tables, in_dims, nt, D, batch, aggr, s);
}

int ffh_embedding_fwd_multi_bags_pad_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, const int* in_dims, int nt, int D, int64_t batch, int aggr,
                                          ffh_stream s) {
  ffh_emb_table t[FFH_MAX_TABLES];
  const int rc = bf16_tables(c, tables, nt, t, nullptr);
  if (rc) return rc;
  return emb_fwd_bags_launch<uint16_t, true>(c, t, in_dims, nt, D, batch, aggr, s);
}

// include/ff_hip_pad_mean.h: the pad gather with a mean over the lookups that are there
int ffh_pad_mean_abi_version(void) { return FFH_PAD_MEAN_ABI_VERSION; }

int ffh_embedding_fwd_multi_bags_pad_mean(ffh_ctx* c, const ffh_emb_table* tables, const int* in_dims, int nt, int D, int64_t batch, int aggr, ffh_stream s) {
  return emb_fwd_bags_launch<float, true, true>(c, tables, in_dims, nt, D, batch, aggr, s);
}

int ffh_embedding_fwd_multi_bags_pad_mean_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, const int* in_dims, int nt, int D, int64_t batch, int aggr,
                                               ffh_stream s) {
  ffh_emb_table t[FFH_MAX_TABLES];
  const int rc = bf16_tables(c, tables, nt, t, nullptr);
  if (rc) return rc;
  return emb_fwd_bags_launch<uint16_t, true, true>(c, t, in_dims, nt, D, batch, aggr, s);
}

}  // extern "C"
