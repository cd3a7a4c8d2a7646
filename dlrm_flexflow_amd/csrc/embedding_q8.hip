// embedding_q8.hip -- include/ff_hip_q8.h: embedding tables as 8-bit rows with a scale and a bias each (fbgemm's fused 8-bit row-wise
// format), hand-written for gfx950.  Evaluation only: nothing here updates a table.
//
// What is here:
//   * q8_fwd_kernel / q8_fwd_bags_kernel: the gathers, with the lane geometry, the grids and the store epilogue of emb_fwd_kernel /
//     emb_fwd_bags_kernel (emb_gather.h).  D / 4 adjacent lanes take one row; a lane loads ONE dword of four codes (a quarter of the fp32
//     gather's bytes) and the row's 8-byte tail (scale, bias: one address across the lane-group, one request), widens the codes with the
//     byte-select conversions (v_cvt_f32_ubyte0..3) and produces four floats: w = code * scale + bias, then acc = acc + w, in the order
//     of the fp32 gather.  So the output is the bits of the fp32 gather on the dequantized table.
//   * q8_quantize_kernel: fp32 / bf16 table -> rows, all tables of a call in one grid-capped, grid-stride launch.  Where D % 16 == 0 a lane
//     takes 16 elements -- four 16-byte loads (bf16: 8-byte) in flight, one 16-byte store of codes -- else 4 elements and a dword of codes.
//     P lanes (the least power of two >= the lanes a row needs, at most 64) share a row; min and max cross them in a butterfly (neither
//     depends on the order); the group's first lane stores scale and bias as 8 bytes.  Rows that need more than 64 lanes loop, and re-read
//     the chunks behind the first from cache for the codes.
// Every product and sum that the contract names is rounded on its own: the file is compiled with contraction off (cross.hip says why
// __fmul_rn / __fadd_rn do not do that).
#include "emb_gather.h"

#include "../../include/ff_hip_q8.h"

#pragma clang fp contract(off)

namespace {

using namespace ffh_emb;

// The lane geometry of embedding_fwd.hip (its RowLanes, the same struct: that file keeps its own, where the tests of the grid caps read it).
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

constexpr int kQ8QuantCap = 2048;      // workgroups of the quantizer: 256 CUs x 8

// Kernel arguments of both gathers.  t[i].weight carries the rows' address; a bag size in 16 bits, a row size in 32 and the image column
// in 8 keep 64 tables inside the 4 KB of kernel arguments.
struct Q8Args {
  ffh_emb_table t[FFH_MAX_TABLES];
  unsigned short* out16[FFH_MAX_TABLES];   // as EmbArgs::out16
  char* out3[FFH_MAX_TABLES];              // as EmbArgs::out3 ...
  uint32_t rb[FFH_MAX_TABLES];             // row_bytes of table i
  uint16_t L[FFH_MAX_TABLES];              // ragged: bag size of table i (<= kBagMaxL)
  uint8_t  out3c[FFH_MAX_TABLES];          // ... and EmbArgs::out3c (0 .. 31)
  int64_t batch;
  int64_t nrb[2];       // ragged: row blocks of the batch, [0] short bags (U = 4), [1] long bags (U = 2)
  int     ntables, D, aggr;
  int     shift;        // ragged: workgroups of table i = clamp((batch * L[i]) >> shift, 1, nrb)
  int     Lu;           // uniform: the bag size
};
static_assert(sizeof(Q8Args) <= 4096, "kernel arguments");

// one lane's share of a row: four codes, and the row's scale and bias
struct Q8Val { unsigned codes; float scale, bias; };
typedef unsigned q8_tail_t __attribute__((ext_vector_type(2), aligned(4)));      // a row's tail sits at a dword address (row_bytes % 4 == 0)

__device__ __forceinline__ Q8Val q8_load(const uint8_t* rows, const int64_t row, const uint32_t rb, const int D, const int c) {
  const uint8_t* p = rows + row * (int64_t)rb;
  Q8Val v;
  v.codes = *reinterpret_cast<const unsigned*>(p + 4 * c);
  const q8_tail_t sb = *reinterpret_cast<const q8_tail_t*>(p + D);
  v.scale = __uint_as_float(sb.x);
  v.bias = __uint_as_float(sb.y);
  return v;
}

// acc = acc + (code * scale + bias): three roundings per element, none fused
__device__ __forceinline__ void q8_add(float (&acc)[4], const Q8Val& v) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float w = (float)((v.codes >> (8 * k)) & 0xffu) * v.scale + v.bias;
    acc[k] = acc[k] + w;       // 0 + w first: (+0) + (-0) = +0, as the fp32 gather
  }
}

// ---- one bag size for all tables: emb_fwd_kernel<4, UNROLL> on 8-bit rows (grid.y = table) ----
template <int UNROLL>
__global__ __launch_bounds__(256) void q8_fwd_kernel(const Q8Args a) {
  ffh_kernel_prio();
  const ffh_emb_table tb = a.t[blockIdx.y];
  const uint8_t* const rows = reinterpret_cast<const uint8_t*>(tb.weight);
  const uint32_t rb = a.rb[blockIdx.y];
  unsigned short* const o16 = a.out16[blockIdx.y];
  char* const o3 = a.out3[blockIdx.y];
  const int o3c = a.out3c[blockIdx.y];
  const int D = a.D, L = a.Lu;
  const RowLanes g(D, 4, threadIdx.x & 63);
  const int wave = threadIdx.x >> 6;
  const int64_t rows_per_block = g.block_rows(UNROLL);
  const float inv = 1.0f / (float)L;
  const bool avg = a.aggr == FFH_AGGR_MODE_AVG;

  for (int64_t base = (int64_t)blockIdx.x * rows_per_block; base < a.batch; base += (int64_t)gridDim.x * rows_per_block) {
    const int64_t b0 = base + (int64_t)wave * g.rpw * UNROLL + g.rsub;
    for (int c = g.c0; c < g.nvec; c += g.lpr) {
      float acc[UNROLL][4];
#pragma unroll
      for (int u = 0; u < UNROLL; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) acc[u][v] = 0.0f;
      for (int j = 0; j < L; j++) {
        int64_t row[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
          const int64_t b = b0 + (int64_t)u * g.rpw;
          row[u] = (g.active && b < a.batch) ? tb.idx[b * L + j] : -1;
        }
        Q8Val val[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++)
          if (row[u] >= 0) val[u] = q8_load(rows, row[u], rb, D, c);
#pragma unroll
        for (int u = 0; u < UNROLL; u++)
          if (row[u] >= 0) q8_add(acc[u], val[u]);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; u++) {
        const int64_t b = b0 + (int64_t)u * g.rpw;
        if (g.active && b < a.batch) store_row<4>(tb, o16, o3, o3c, b, c, acc[u], avg, inv);
      }
    }
  }
}

// ---- a bag size per table: bag_rows / emb_fwd_bags_kernel of embedding_fwd.hip on 8-bit rows (the flat grid, bag_blocks, U x JU) ----
template <int U, int JU>
__device__ __forceinline__ void q8_bag_rows(const Q8Args& a, const int t, const int64_t first, const int64_t step) {
  const ffh_emb_table tb = a.t[t];
  const uint8_t* const rows = reinterpret_cast<const uint8_t*>(tb.weight);
  const uint32_t rb = a.rb[t];
  unsigned short* const o16 = a.out16[t];
  char* const o3 = a.out3[t];
  const int o3c = a.out3c[t];
  const int D = a.D, L = a.L[t];
  const RowLanes g(D, 4, threadIdx.x & 63);
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
      float acc[U][4];
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) acc[u][v] = 0.0f;
      int j = 0;
      if constexpr (JU > 1) {
        for (; j + JU <= L; j += JU) {
          int64_t row[U][JU];
#pragma unroll
          for (int u = 0; u < U; u++)
#pragma unroll
            for (int k = 0; k < JU; k++) row[u][k] = ok[u] ? ids[u][j + k] : 0;
          Q8Val val[U][JU];
#pragma unroll
          for (int u = 0; u < U; u++)
#pragma unroll
            for (int k = 0; k < JU; k++)
              if (ok[u]) val[u][k] = q8_load(rows, row[u][k], rb, D, c);
#pragma unroll
          for (int u = 0; u < U; u++)
            if (ok[u]) {
#pragma unroll
              for (int k = 0; k < JU; k++) q8_add(acc[u], val[u][k]);      // ascending j: the order of the uniform kernel
            }
        }
      }
      for (; j < L; j++) {
        int64_t row[U];
#pragma unroll
        for (int u = 0; u < U; u++) row[u] = ok[u] ? ids[u][j] : 0;
        Q8Val val[U];
#pragma unroll
        for (int u = 0; u < U; u++)
          if (ok[u]) val[u] = q8_load(rows, row[u], rb, D, c);
#pragma unroll
        for (int u = 0; u < U; u++)
          if (ok[u]) q8_add(acc[u], val[u]);
      }
#pragma unroll
      for (int u = 0; u < U; u++)
        if (ok[u]) store_row<4>(tb, o16, o3, o3c, b0 + (int64_t)u * g.rpw, c, acc[u], avg, inv);
    }
  }
}

__global__ __launch_bounds__(256) void q8_fwd_bags_kernel(const Q8Args a) {
  ffh_kernel_prio();
  // workgroup -> (table, first row block of the table): block-uniform, as emb_fwd_bags_kernel
  int t = 0;
  int64_t first = blockIdx.x, w = 0;
  for (; t < a.ntables; t++) {
    const int L = a.L[t];
    w = bag_blocks(a.batch, L, a.shift, L >= kBagLong ? a.nrb[1] : a.nrb[0]);
    if (first < w) break;
    first -= w;
  }
  if (t >= a.ntables) return;
  if (a.L[t] >= kBagLong) q8_bag_rows<2, 4>(a, t, first, w);
  else q8_bag_rows<4, 1>(a, t, first, w);
}

// ---- the quantizer ----
struct Q8QuantArgs {
  ffh_q8_source s[FFH_MAX_TABLES];
  int64_t trip0[FFH_MAX_TABLES + 1];     // the first trip of table i; [ntables]: all trips
  int ntables, D;
};
static_assert(sizeof(Q8QuantArgs) <= 4096, "kernel arguments");

// A lane takes V float4 vectors of a row at a time: V = 4 (16 elements: four 16-byte loads in flight, ONE 16-byte store of codes) where D % 16 == 0,
// else V = 1 (4 elements, a dword of codes).  Lanes that share a row: the least power of two >= D / (4 V), at most 64 (the butterfly wants a power
// of two; lanes past the row's end idle).
__host__ __device__ inline int q8_vecs(int D) { return D % 16 == 0 ? 4 : 1; }
__host__ __device__ inline int q8_group(int D) {
  const int n = D / (4 * q8_vecs(D));
  int p = 1;
  while (p < n && p < 64) p <<= 1;
  return p;
}

__device__ __forceinline__ float4 q8_src(const ffh_q8_source& s, const int64_t r, const int D, const int c) {
  if (s.bf16) {
    const uint2 h = *(reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(s.weight) + r * D) + c);
    return make_float4(ffh_bf16_lo_as_f32(h.x), ffh_bf16_hi_as_f32(h.x), ffh_bf16_lo_as_f32(h.y), ffh_bf16_hi_as_f32(h.y));
  }
  return *(reinterpret_cast<const float4*>(reinterpret_cast<const float*>(s.weight) + r * D) + c);
}

__device__ __forceinline__ unsigned q8_code(const float x, const float mn, const float inv) {
  return (unsigned)rintf((x - mn) * inv) & 0xffu;
}
__device__ __forceinline__ unsigned q8_codes(const float4 v, const float mn, const float inv) {
  return q8_code(v.x, mn, inv) | (q8_code(v.y, mn, inv) << 8) | (q8_code(v.z, mn, inv) << 16) | (q8_code(v.w, mn, inv) << 24);
}

typedef unsigned q8_u4 __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes of codes at a dword address (rows are row_bytes apart: D + 8)

template <int V>
__global__ __launch_bounds__(256) void q8_quantize_kernel(const Q8QuantArgs a) {
  ffh_kernel_prio();
  const int D = a.D, nvec = D / 4, nchunk = nvec / V;      // chunks of V vectors: one lane's share per turn
  const int P = q8_group(D);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rpw = 64 / P, rsub = lane / P, c0 = lane & (P - 1);
  const int64_t rows_per_trip = 4 * rpw;
  const int64_t trips = a.trip0[a.ntables];
  int t = 0;
  for (int64_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {      // block-uniform
    while (trip >= a.trip0[t + 1]) t++;                                   // trips ascend: t only grows (trip < trips = trip0[ntables])
    const ffh_q8_source s = a.s[t];
    const int64_t r = (trip - a.trip0[t]) * rows_per_trip + wave * rpw + rsub;
    const bool ok = r < s.num_entries;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    float4 v0[V];
#pragma unroll
    for (int k = 0; k < V; k++) v0[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (ok)
      for (int c = c0; c < nchunk; c += P) {      // a second turn only where P == 64
        float4 v[V];
#pragma unroll
        for (int k = 0; k < V; k++) v[k] = q8_src(s, r, D, c * V + k);
#pragma unroll
        for (int k = 0; k < V; k++) {
          if (c == c0) v0[k] = v[k];
          mn = fminf(fminf(fminf(mn, v[k].x), fminf(v[k].y, v[k].z)), v[k].w);
          mx = fmaxf(fmaxf(fmaxf(mx, v[k].x), fmaxf(v[k].y, v[k].z)), v[k].w);
        }
      }
    for (int m = 32; m >= 1; m >>= 1)             // every lane of the wave takes part; partners stay inside the group of P lanes
      if (m < P) {
        mn = fminf(mn, __shfl_xor(mn, m));
        mx = fmaxf(mx, __shfl_xor(mx, m));
      }
    if (!ok) continue;
    mn = mn + 0.0f;                               // a zero minimum is +0
    const float range = mx - mn;
    const float scale = range / 255.0f;
    const float inv = 255.0f / (range + 1e-8f);
    uint8_t* const out = s.rows + r * s.row_bytes;
    for (int c = c0; c < nchunk; c += P) {
      unsigned q[V];
#pragma unroll
      for (int k = 0; k < V; k++) q[k] = q8_codes(c == c0 ? v0[k] : q8_src(s, r, D, c * V + k), mn, inv);
      if constexpr (V == 4) {
        const q8_u4 o = {q[0], q[1], q[2], q[3]};
        *reinterpret_cast<q8_u4*>(out + 16 * c) = o;
      } else {
        *reinterpret_cast<unsigned*>(out + 4 * c) = q[0];
      }
    }
    // the tail: scale and bias as one 8-byte store by the group's first lane, then zeros up to row_bytes -- dword nvec + 2 + k by lane k
    if (c0 == 0) {
      const q8_tail_t sb = {__float_as_uint(scale), __float_as_uint(mn)};
      *reinterpret_cast<q8_tail_t*>(out + D) = sb;
    }
    const int ndw = (int)(s.row_bytes / 4);
    for (int w = nvec + 2 + c0; w < ndw; w += P) *reinterpret_cast<unsigned*>(out + 4 * (int64_t)w) = 0u;
  }
}

// ---- host side ----
// the checks of both gathers; on success t[] holds the tables as ffh_emb_table (weight = rows) for gather_dests
int q8_tables(ffh_ctx* c, const ffh_emb_table_q8* in, int nt, int D, int64_t batch, int aggr, ffh_emb_table* t) {
  if (nt < 0 || nt > FFH_MAX_TABLES) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_q8: ntables out of range");
  if (nt > 0 && !in) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_q8: null tables");
  if (D <= 0 || batch < 0) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_q8: bad dims");
  if (aggr != FFH_AGGR_MODE_SUM && aggr != FFH_AGGR_MODE_AVG) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_q8: aggr must be SUM or AVG");
  for (int i = 0; i < nt; i++) {
    if (!in[i].idx || !in[i].rows || !in[i].io) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_q8: null pointer");
    if (in[i].ld < D || in[i].num_entries <= 0) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_q8: ld < out_dim or num_entries <= 0");
    if (in[i].row_bytes < (int64_t)D + 8 || in[i].row_bytes % 4) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_q8: row_bytes < out_dim + 8 or no multiple of 4");
  }
  if (D % 4) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_q8: out_dim must be a multiple of 4");
  for (int i = 0; i < nt; i++) {
    if (!aligned16(in[i].io) || in[i].ld % 4) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_q8: io must be 16-byte aligned with ld a multiple of 4 (there is no scalar form)");
    if ((uintptr_t)in[i].rows & 3) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_q8: rows must be 4-byte aligned");
    if (in[i].row_bytes > (int64_t)UINT32_MAX) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_q8: row_bytes >= 2^32");
    t[i] = ffh_emb_table{in[i].idx, reinterpret_cast<float*>(const_cast<uint8_t*>(in[i].rows)), in[i].io, in[i].num_entries, in[i].ld};
  }
  return FFH_OK;
}

void q8_args(const ffh_ctx* c, const ffh_emb_table_q8* in, const ffh_emb_table* t, int nt, int D, int64_t batch, int aggr, Q8Args& a) {
  memset(&a, 0, sizeof a);
  gather_dests(c, t, nt, D, batch, 4, a);
  for (int i = 0; i < nt; i++) a.rb[i] = (uint32_t)in[i].row_bytes;
  a.batch = batch; a.ntables = nt; a.D = D; a.aggr = aggr;
}

}  // namespace

extern "C" {

int ffh_q8_abi_version(void) { return FFH_Q8_ABI_VERSION; }
size_t ffh_q8_row_bytes(int out_dim) { return (size_t)out_dim + 8; }
int ffh_q8_quantize_max_workgroups(void) { return kQ8QuantCap; }

int ffh_embedding_fwd_multi_q8(ffh_ctx* c, const ffh_emb_table_q8* tables, int nt, int L, int D, int64_t batch, int aggr, ffh_stream s) {
  if (L <= 0) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_fwd_multi_q8: in_dim < 1");
  ffh_emb_table t[FFH_MAX_TABLES];
  const int rc = q8_tables(c, tables, nt, D, batch, aggr, t);
  if (rc) return rc;
  if (nt == 0 || batch == 0) return FFH_OK;
  Q8Args a;
  q8_args(c, tables, t, nt, D, batch, aggr, a);
  a.Lu = L;
  // the grid of emb_fwd_launch: 1024 workgroups over all tables, grid-stride the rest
  constexpr int U = 4;
  const int64_t rows_per_block = RowLanes(D, 4).block_rows(U);
  int64_t gx = (batch + rows_per_block - 1) / rows_per_block;
  const int64_t cap = 1024 / nt;
  if (gx > cap) gx = cap;
  hipLaunchKernelGGL((q8_fwd_kernel<U>), dim3((unsigned)gx, (unsigned)nt), dim3(256), 0, as_stream(s), a);
  FFH_LAUNCH_CHECK(c, "q8_fwd_kernel");
  return FFH_OK;
}

int ffh_embedding_fwd_multi_bags_q8(ffh_ctx* c, const ffh_emb_table_q8* tables, const int* in_dims, int nt, int D, int64_t batch, int aggr,
                                    ffh_stream s) {
  ffh_emb_table t[FFH_MAX_TABLES];
  int rc = q8_tables(c, tables, nt, D, batch, aggr, t);
  if (rc) return rc;
  if (nt > 0 && !in_dims) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_fwd_multi_bags_q8: null in_dims");
  for (int i = 0; i < nt; i++) {
    if (in_dims[i] < 1) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_fwd_multi_bags_q8: in_dims[i] < 1");
    if (in_dims[i] > kBagMaxL) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_fwd_multi_bags_q8: in_dims[i] > FFH_BAGS_MAX_IN_DIM (65535)");
  }
  if (nt == 0 || batch == 0) return FFH_OK;
  Q8Args a;
  q8_args(c, tables, t, nt, D, batch, aggr, a);
  for (int i = 0; i < nt; i++) a.L[i] = (uint16_t)in_dims[i];
  // the workgroup map of emb_fwd_bags_launch: workgroups in proportion to the lookups, at most 2048 over all tables
  const RowLanes g(D, 4);
  const int64_t rpb_short = g.block_rows(4), rpb_long = g.block_rows(2);      // q8_bag_rows<U = 4 / 2, ..>
  a.nrb[0] = (batch + rpb_short - 1) / rpb_short;
  a.nrb[1] = (batch + rpb_long - 1) / rpb_long;
  const int64_t cap = 2048;
  int64_t total = 0;
  for (int sh = 0; sh < 63; sh++) {
    total = 0;
    for (int i = 0; i < nt; i++) total += bag_blocks(batch, in_dims[i], sh, a.nrb[in_dims[i] >= kBagLong ? 1 : 0]);
    a.shift = sh;
    if (total <= cap) break;
  }
  hipLaunchKernelGGL(q8_fwd_bags_kernel, dim3((unsigned)total), dim3(256), 0, as_stream(s), a);
  FFH_LAUNCH_CHECK(c, "q8_fwd_bags_kernel");
  return FFH_OK;
}

int ffh_embedding_quantize_q8(ffh_ctx* c, const ffh_q8_source* src, int nt, int D, ffh_stream s) {
  if (nt < 0 || nt > FFH_MAX_TABLES) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_quantize_q8: ntables out of range");
  if (nt > 0 && !src) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_quantize_q8: null sources");
  if (D <= 0) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_quantize_q8: bad out_dim");
  for (int i = 0; i < nt; i++) {
    if (!src[i].weight || !src[i].rows) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_quantize_q8: null pointer");
    if (src[i].num_entries < 0 || (src[i].bf16 != 0 && src[i].bf16 != 1)) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_quantize_q8: num_entries < 0 or bf16 not 0 / 1");
    if (src[i].row_bytes < (int64_t)D + 8 || src[i].row_bytes % 4) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_quantize_q8: row_bytes < out_dim + 8 or no multiple of 4");
  }
  if (D % 4) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_quantize_q8: out_dim must be a multiple of 4");
  for (int i = 0; i < nt; i++) {
    if ((uintptr_t)src[i].weight & (src[i].bf16 ? 7 : 15)) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_quantize_q8: weight must be 16-byte aligned (bf16: 8)");
    if ((uintptr_t)src[i].rows & 3) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_quantize_q8: rows must be 4-byte aligned");
    if (src[i].row_bytes > (int64_t)UINT32_MAX) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_quantize_q8: row_bytes >= 2^32");
  }
  Q8QuantArgs a;
  memset(&a, 0, sizeof a);
  const int64_t rows_per_trip = 4 * (64 / q8_group(D));
  for (int i = 0; i < nt; i++) {
    a.s[i] = src[i];
    a.trip0[i + 1] = a.trip0[i] + (src[i].num_entries + rows_per_trip - 1) / rows_per_trip;
  }
  a.ntables = nt; a.D = D;
  const int64_t trips = a.trip0[nt];
  if (trips == 0) return FFH_OK;
  const unsigned grid = (unsigned)(trips < kQ8QuantCap ? trips : kQ8QuantCap);
  if (q8_vecs(D) == 4) hipLaunchKernelGGL(q8_quantize_kernel<4>, dim3(grid), dim3(256), 0, as_stream(s), a);
  else hipLaunchKernelGGL(q8_quantize_kernel<1>, dim3(grid), dim3(256), 0, as_stream(s), a);
  FFH_LAUNCH_CHECK(c, "q8_quantize_kernel");
  return FFH_OK;
}

}  // extern "C"
