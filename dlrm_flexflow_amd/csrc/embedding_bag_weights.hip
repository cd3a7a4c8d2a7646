// embedding_bag_weights.hip -- include/ffh_bag_weights.h: per-sample weights on embedding bags, hand-written for gfx950.
// The entries are weighted forms of the pad ragged entries (include/ff_hip_pad.h): a bag size per table, an id < 0 is no lookup, SUM only.
//
// What is here:
//   * bagw_fwd_kernel: the weighted gather.  The workgroup map (bag_blocks), the lane geometry, both bag shapes (U = 4 rows x 1 slot for short
//     bags, U = 2 rows x JU = 4 slots for bags of kBagLong and more) and the store epilogue (store_row) are those of emb_fwd_bags_kernel.  What is
//     added: the lanes that share a row load the slot's weight from ONE address, as they load its id (one request per lane-group; 4 bytes per
//     lookup beside the 8 of the id and the 4 D of the row), predicated with the row load on id >= 0, and the add becomes a multiply and an add:
//     acc = acc + w * W[id][d].  The weight pointers need room in the kernel arguments that BagArgs does not have (64 tables x 40 bytes and three
//     pointer arrays are past 4 KB), so this kernel has a table record of its own: the gather never reads num_entries, and the weight pointer
//     takes its 8 bytes.
//   * emb_bagw_reduce_kernel / emb_bagw_small_kernel: the weighted apply kernels of the ragged update (reduce_tile_body in emb_reduce.h says
//     what its WGT form does) and the launch table embedding.hip reaches them through.  The sort is the pad form's.
//   * the five entries.
// Every product is rounded on its own: the file is compiled with contraction off, ahead of the headers whose templates it instantiates
// (cross.hip says why __fmul_rn / __fadd_rn do not do that).  The row rules are written with explicit fmaf or under their own pragma, and
// neither the segmented sum nor the folds hold a product, so with every weight 1.0f the kernels here give the bits of the pad kernels.
#pragma clang fp contract(off)

#include "emb_gather.h"
#include "emb_bags_update.h"
#include "../../include/ffh_bag_weights.h"

#include <type_traits>

namespace {

using namespace ffh_emb;

// a BagWTable lies in an ffh_emb_table's place in the kernel arguments (emb_bags_update.h): the three pointers the kernels read through either
// view sit where they sit there, the two narrowed fields share num_entries' eight bytes, and the weight pointer takes ld's
static_assert(offsetof(BagWTable, idx) == offsetof(ffh_emb_table, idx) && offsetof(BagWTable, weight) == offsetof(ffh_emb_table, weight) &&
              offsetof(BagWTable, io) == offsetof(ffh_emb_table, io) && offsetof(BagWTable, num_entries) == offsetof(ffh_emb_table, num_entries) &&
              offsetof(BagWTable, ld) == offsetof(ffh_emb_table, num_entries) + 4 && offsetof(BagWTable, w) == offsetof(ffh_emb_table, ld), "BagWTable layout");

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

// VEC table elements per lane per access: fp32 rows 16 / 4 bytes, bf16 rows (WT = uint16_t) 8 / 2 bytes; a bf16 element widens exactly
template <int VEC, class WT> struct RowVec { typedef typename std::conditional<VEC == 4, float4, float>::type type; };
template <> struct RowVec<4, uint16_t> { typedef uint2 type; };
template <> struct RowVec<1, uint16_t> { typedef unsigned short type; };
template <int VEC, class WT>
__device__ __forceinline__ float row_elem(const typename RowVec<VEC, WT>::type& v, int k) {
  if constexpr (std::is_same<WT, float>::value) return reinterpret_cast<const float*>(&v)[k];
  else return ffh_bf16_to_f32(reinterpret_cast<const unsigned short*>(&v)[k]);
}

// ---------------------------------------------------------------------------
// the weighted gather
// ---------------------------------------------------------------------------
struct BagWFwdTable {
  const int64_t* idx;      // [batch][L]
  const void*    weight;   // the table's rows, fp32 or bf16 bits
  float*         io;       // out [batch][ld]
  const float*   w;        // [batch][L]
  int64_t        ld;
};
struct BagWArgs {
  BagWFwdTable t[FFH_MAX_TABLES];
  unsigned short* out16[FFH_MAX_TABLES];   // as BagArgs::out16 (embedding_fwd.hip)
  char* out3[FFH_MAX_TABLES];              // as BagArgs::out3 ...
  uint16_t L[FFH_MAX_TABLES];              // bag size of table i (<= kBagMaxL)
  uint8_t  out3c[FFH_MAX_TABLES];          // ... and its column (0 .. 31)
  int64_t batch;
  int64_t nrb[2];        // row blocks of the batch: [0] short bags (U = 4), [1] long bags (U = 2)
  int     ntables, D;
  int     shift;         // workgroups of table i = clamp((batch * L[i]) >> shift, 1, nrb)
};
static_assert(sizeof(BagWArgs) <= 4096, "kernel arguments");

// the rows [first, first + step, ...) x rows_per_block of table t; U rows x JU slots in flight per lane-group.  The id and the weight of a slot
// are the same in the lanes that share a row and differ between the row groups of a wave, so the weight load, the row load and the
// multiply-add are predicated on id >= 0 beside ok[u], not branched around; acc keeps its +0 where nothing is added.
template <int VEC, int U, int JU, class WT>
__device__ __forceinline__ void bagw_rows(const BagWArgs& a, const int t, const int64_t first, const int64_t step) {
  using vec_t = typename RowVec<VEC, WT>::type;
  const BagWFwdTable tw = a.t[t];
  const ffh_emb_table tb = {tw.idx, nullptr, tw.io, 0, tw.ld};      // what store_row reads: io and ld
  const WT* const wt = reinterpret_cast<const WT*>(tw.weight);
  unsigned short* const o16 = a.out16[t];
  char* const o3 = a.out3[t];
  const int o3c = a.out3c[t];
  const int D = a.D, L = a.L[t];
  const RowLanes g(D, VEC, threadIdx.x & 63);
  const int wave = threadIdx.x >> 6;
  const int64_t rows_per_block = g.block_rows(U);

  for (int64_t base = first * rows_per_block; base < a.batch; base += step * rows_per_block) {
    const int64_t b0 = base + (int64_t)wave * g.rpw * U + g.rsub;
    bool ok[U];
    const int64_t* ids[U];
    const float* wts[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t b = b0 + (int64_t)u * g.rpw;
      ok[u] = g.active && b < a.batch;
      ids[u] = tw.idx + b * L;      // (read where ok[u] only)
      wts[u] = tw.w + b * L;
    }
    for (int c = g.c0; c < g.nvec; c += g.lpr) {
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
            for (int k = 0; k < JU; k++) row[u][k] = ok[u] ? ids[u][j + k] : -1;
          float wv[U][JU];
          vec_t val[U][JU];
#pragma unroll
          for (int u = 0; u < U; u++)
#pragma unroll
            for (int k = 0; k < JU; k++)
              if (row[u][k] >= 0) {
                wv[u][k] = wts[u][j + k];
                val[u][k] = *(reinterpret_cast<const vec_t*>(wt + row[u][k] * (int64_t)D) + c);
              }
#pragma unroll
          for (int u = 0; u < U; u++)
#pragma unroll
            for (int k = 0; k < JU; k++)           // ascending j
              if (row[u][k] >= 0) {
#pragma unroll
                for (int v = 0; v < VEC; v++) {
                  const float p = wv[u][k] * row_elem<VEC, WT>(val[u][k], v);
                  acc[u][v] = acc[u][v] + p;
                }
              }
        }
      }
      for (; j < L; j++) {
        int64_t row[U];
#pragma unroll
        for (int u = 0; u < U; u++) row[u] = ok[u] ? ids[u][j] : -1;
        float wv[U];
        vec_t val[U];
#pragma unroll
        for (int u = 0; u < U; u++)
          if (row[u] >= 0) {
            wv[u] = wts[u][j];
            val[u] = *(reinterpret_cast<const vec_t*>(wt + row[u] * (int64_t)D) + c);
          }
#pragma unroll
        for (int u = 0; u < U; u++)
          if (row[u] >= 0) {
#pragma unroll
            for (int v = 0; v < VEC; v++) {
              const float p = wv[u] * row_elem<VEC, WT>(val[u], v);
              acc[u][v] = acc[u][v] + p;
            }
          }
      }
#pragma unroll
      for (int u = 0; u < U; u++)
        if (ok[u]) store_row<VEC>(tb, o16, o3, o3c, b0 + (int64_t)u * g.rpw, c, acc[u], false, 1.0f);
    }
  }
}

template <int VEC, class WT>
__global__ __launch_bounds__(256) void bagw_fwd_kernel(const BagWArgs a) {
  ffh_kernel_prio();
  // workgroup -> (table, first row block of the table): block-uniform, the map of emb_fwd_bags_kernel
  int t = 0;
  int64_t first = blockIdx.x, w = 0;
  for (; t < a.ntables; t++) {
    const int L = a.L[t];
    w = bag_blocks(a.batch, L, a.shift, L >= kBagLong ? a.nrb[1] : a.nrb[0]);
    if (first < w) break;
    first -= w;
  }
  if (t >= a.ntables) return;
  if (a.L[t] >= kBagLong) bagw_rows<VEC, 2, 4, WT>(a, t, first, w);
  else bagw_rows<VEC, 4, 1, WT>(a, t, first, w);
}

// what gather_dests fills: the tables and their destinations' twins / images
struct BagWDests {
  ffh_emb_table t[FFH_MAX_TABLES];
  unsigned short* out16[FFH_MAX_TABLES];
  char* out3[FFH_MAX_TABLES];
  int out3c[FFH_MAX_TABLES];
};

template <class WT>
int bagw_fwd_launch(ffh_ctx* c, const ffh_emb_table* tables, const float* const* weights, const int* in_dims, int nt, int D, int64_t batch, int aggr,
                    ffh_stream s) {
  int rc = validate_tables(c, tables, nt, 1, D, batch, aggr);
  if (rc) return rc;
  if (aggr != FFH_AGGR_MODE_SUM)
    return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_fwd_multi_bags_weighted: aggr must be FFH_AGGR_MODE_SUM (weights with mean pooling are not supported; the unweighted "
                                        "mean is ffh_embedding_fwd_multi_bags_pad_mean)");
  if (nt > 0 && !in_dims) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_fwd_multi_bags_weighted: null in_dims");
  if (nt > 0 && !weights) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_fwd_multi_bags_weighted: null weights");
  for (int i = 0; i < nt; i++) {
    if (in_dims[i] < 1) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_fwd_multi_bags_weighted: in_dims[i] < 1");
    if (in_dims[i] > kBagMaxL) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_fwd_multi_bags_weighted: in_dims[i] > FFH_BAGS_MAX_IN_DIM (65535)");
    if ((batch > 0 && !weights[i]) || ((uintptr_t)weights[i] & 3))
      return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_fwd_multi_bags_weighted: weights[i] is null or not 4-byte aligned");
  }
  if (nt == 0 || batch == 0) return FFH_OK;
  // the form of the pad gather: 16-byte (bf16 rows: 8-byte) accesses where every table and destination row allows them
  bool v4 = can_vec4(tables, nt, D);
  if (std::is_same<WT, uint16_t>::value) {
    v4 = D % 4 == 0;
    for (int i = 0; i < nt; i++) v4 = v4 && ((uintptr_t)tables[i].weight & 7) == 0 && aligned16(tables[i].io) && tables[i].ld % 4 == 0;
  }
  const int vec = v4 ? 4 : 1;
  if ((D / vec + 63) / 64 > kMaxChunks * 64) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_fwd_multi_bags_weighted: out_dim too large");
  BagWDests d;
  memset(&d, 0, sizeof d);
  gather_dests(c, tables, nt, D, batch, vec, d);
  BagWArgs a;
  memset(&a, 0, sizeof a);
  for (int i = 0; i < nt; i++) {
    a.t[i] = BagWFwdTable{tables[i].idx, tables[i].weight, tables[i].io, weights[i], tables[i].ld};
    a.out16[i] = d.out16[i]; a.out3[i] = d.out3[i]; a.out3c[i] = (uint8_t)d.out3c[i];
    a.L[i] = (uint16_t)in_dims[i];
  }
  a.batch = batch; a.ntables = nt; a.D = D;
  const RowLanes g(D, vec);
  const int64_t rpb_short = g.block_rows(4), rpb_long = g.block_rows(2);      // bagw_rows<.., U = 4 / 2, ..>
  a.nrb[0] = (batch + rpb_short - 1) / rpb_short;
  a.nrb[1] = (batch + rpb_long - 1) / rpb_long;
  // workgroups in proportion to the lookups: the smallest shift at which the tables' shares fit 256 CUs x 8 workgroups
  constexpr int64_t cap = 2048;
  int64_t total = 0;
  for (int sh = 0; sh < 63; sh++) {
    total = 0;
    for (int i = 0; i < nt; i++) total += bag_blocks(batch, in_dims[i], sh, a.nrb[in_dims[i] >= kBagLong ? 1 : 0]);
    a.shift = sh;
    if (total <= cap) break;
  }
  if (vec == 4) hipLaunchKernelGGL((bagw_fwd_kernel<4, WT>), dim3((unsigned)total), dim3(256), 0, as_stream(s), a);
  else hipLaunchKernelGGL((bagw_fwd_kernel<1, WT>), dim3((unsigned)total), dim3(256), 0, as_stream(s), a);
  FFH_LAUNCH_CHECK(c, "bagw_fwd_kernel");
  return FFH_OK;
}

// ---------------------------------------------------------------------------
// the weighted update's apply kernels: emb_bags_reduce_kernel / emb_bags_small_kernel (emb_bags_update.h) in their pad form, statement by
// statement, on table descriptors that carry the weights (BagWTable) and with reduce_tile_body's WGT form.  They are copies and not one more
// template parameter of those kernels: the existing instantiations then keep the instructions they had.
// ---------------------------------------------------------------------------
template <int VEC, RowRule R, class WT, bool LRP>
__global__ __launch_bounds__(kRedThreads, (red_waves_per_simd<VEC, R, WT, false>())) void emb_bagw_reduce_kernel(const BagsRedArgs a) {
  ffh_kernel_prio();
  FFH_OPT_OF(LRP, op, a.op);
  __shared__ RedSmem smem;
  __shared__ int s_last;
  RedShared& sh = smem.sh;
  uint2* const s_fmeta = smem.fmeta;
  BagsAt at;
  if (!bags_locate(a.g, a.g.red_sh, blockIdx.x, &at)) return;
  const int tix = at.t;
  const int64_t N = at.N;
  const int tile = 1 << a.g.red_sh;
  const int nchunks = bags_nchunks(N), nchunks1 = bags_nchunks1(N);
  const int L = a.g.L[tix];
  ffh_emb_table tb;
  const float* const wgt = bag_w_unpack(a.t[tix], &tb);
  const uint2* keys = a.kp[a.parity[tix]] + at.key0;
  float* p0 = a.partial + at.ch0 * 2 * a.D;
  uint2* m0 = a.meta + at.ch0 * 2;
  float* const st0 = opt_state(R) ? a.s0[tix] : nullptr;
  float* const st1 = state1_of<R, WT>(a, tix);
  const SrKey sk = sr_key<R, WT>(a, tix);
  reduce_tile_body<VEC, true, R, WT, true, false, true>(tb, keys, p0, m0, N, nchunks, tile, (int)at.local, L, a.D, a.avg != 0, op, st0, st1, sk, sh, threadIdx.x, false,
                                                nullptr, wgt);

  const int nvec = a.D / VEC;
  const int lpr = nvec < 64 ? nvec : 64;
  const int rpw = 64 / lpr;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t group0 = (int64_t)wave * rpw + lane / lpr;
  const int64_t ngroups = (int64_t)(kRedThreads / 64) * rpw;
  uint32_t* arrive = a.arrive + at.ch1 + tix;
  float* p1 = a.partial1 + at.ch1 * 2 * a.D;
  uint2* m1 = a.meta1 + at.ch1 * 2;
  constexpr int kRatio = FFH_EMB_CHUNK1 / FFH_EMB_CHUNK;

  // this tile's partials and slots are out (written through, completed), then count it in
  const int64_t tile0 = at.local * tile;
  const int64_t B1 = tile0 / FFH_EMB_CHUNK1;
  const int64_t blk_end = (B1 + 1) * FFH_EMB_CHUNK1 < N ? (B1 + 1) * FFH_EMB_CHUNK1 : N;
  const uint32_t tiles_in_block = (uint32_t)((blk_end - B1 * FFH_EMB_CHUNK1 + tile - 1) / tile);
  xwg_stores_done();
  __syncthreads();
  if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(&arrive[B1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tiles_in_block - 1u;
  __syncthreads();
  if (!s_last) return;
  auto stage = [&](const uint2* m, int64_t lo, int64_t hi) -> bool {
    const int n = (int)(hi - lo < kFoldStage ? hi - lo : kFoldStage);
    bool any = false;
    for (int i = threadIdx.x; i < n; i += kRedThreads) {
      const uint2 v = xwg_load2<true>(m + lo + i);
      s_fmeta[i] = v;
      any |= v.x != kMetaNone;
    }
    for (int64_t i = lo + kFoldStage + threadIdx.x; i < hi; i += kRedThreads) any |= xwg_load2<true>(m + i).x != kMetaNone;   // (beyond the stage)
    return __syncthreads_or(any);
  };
  if (nchunks1 > 1) {
    const int64_t lo = 2 * B1 * kRatio;
    const int64_t hi = lo + 2 * kRatio < 2 * (int64_t)nchunks ? lo + 2 * kRatio : 2 * (int64_t)nchunks;
    if (stage(m0, lo, hi))
      fold_table_body<VEC, true, R, WT>(tb, p0, m0, p1, m1, nchunks, kRatio, a.D, op, st0, st1, sk, lo, hi, group0, ngroups, keys, s_fmeta, lo, (int)(hi - lo), nullptr);
    xwg_stores_done();
    __syncthreads();
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(&arrive[nchunks1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)nchunks1 - 1u;
    __syncthreads();
    if (!s_last) return;
    const int64_t hi1 = 2 * (int64_t)nchunks1;
    if (stage(m1, 0, hi1))
      fold_table_body<VEC, true, R, WT>(tb, p1, m1, p1, m1, nchunks1, 0, a.D, op, st0, st1, sk, 0, hi1, group0, ngroups, nullptr, s_fmeta, 0, (int)(hi1 < kFoldStage ? hi1 : kFoldStage));
  } else {
    const int64_t hi0 = 2 * (int64_t)nchunks;
    if (stage(m0, 0, hi0))
      fold_table_body<VEC, true, R, WT>(tb, p0, m0, p1, m1, nchunks, 0, a.D, op, st0, st1, sk, 0, hi0, group0, ngroups, nullptr, s_fmeta, 0, (int)hi0);
  }
}


template <int VEC, RowRule R, class WT, bool LRP>
__global__ __launch_bounds__(kSmallThreads) void emb_bagw_small_kernel(const BagsSmallArgs a) {
  ffh_kernel_prio();
  FFH_OPT_OF(LRP, op, a.op);
  constexpr int NW = kSmallWaves;
  constexpr int E = kSmallMax / kSmallThreads;
  __shared__ SmallShared sm;
  uint32_t* s_k = sm.sort.k;
  uint32_t* s_p = sm.sort.p;
  uint32_t (*s_off)[kMaxRadix] = sm.sort.off;
  BagsAt at;
  if (!bags_locate(a.g, -1, blockIdx.x, &at)) return;
  const int tix = at.t;
  ffh_emb_table tb;
  const float* const wgt = bag_w_unpack(a.t[tix], &tb);
  float* const st0 = opt_state(R) ? a.s0[tix] : nullptr;
  float* const st1 = state1_of<R, WT>(a, tix);
  const SrKey sk = sr_key<R, WT>(a, tix);
  const int64_t N = at.N;                              // <= kSmallMax (the host's route rule)
  const int L = a.g.L[tix];
  const int nch0 = bags_nchunks(N), nch1 = bags_nchunks1(N);
  int tile = (int)((N + kSmallRedParts - 1) / kSmallRedParts);          // one tile per 256-thread team, as the uniform call picks it
  tile = (tile + FFH_EMB_CHUNK - 1) / FFH_EMB_CHUNK * FFH_EMB_CHUNK;
  tile = tile < FFH_EMB_CHUNK ? FFH_EMB_CHUNK : tile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int radix = 1 << a.rb;
  const uint32_t mask = radix - 1;

  uint32_t key[E], pos[E];
  bool valid[E];
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int i = wave * (kSmallMax / NW) + e * 64 + lane;
    valid[e] = i < N;
    key[e] = valid[e] ? bags_first_key<true>(tb.idx[i], (uint32_t)tb.num_entries) : 0u;
    pos[e] = (uint32_t)i;
  }
  const int npass = a.npass[tix];
  for (int p = 0; p < npass; p++) {
    const int shift = p * a.rb;
    for (int d = threadIdx.x; d < NW * kMaxRadix; d += kSmallThreads) (&s_off[0][0])[d] = 0;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; e++)
      if (valid[e]) atomicAdd(&s_off[wave][(key[e] >> shift) & mask], 1u);
    __syncthreads();
    uint32_t all_d[1] = {0};
    const uint32_t before_d[1] = {0};
    if ((int)threadIdx.x < radix) {
      uint32_t t = 0;
#pragma unroll
      for (int w2 = 0; w2 < NW; w2++) t += s_off[w2][threadIdx.x];
      all_d[0] = t;
    }
    sort_scan_offsets<NW, 1>(all_d, before_d, radix, s_off, sm.sort.scan, sm.sort.wsum);
    sort_rank_and_scatter<E>(key, pos, valid, shift, a.rb, mask, s_off[wave], SortOutLds{s_k, s_p});
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int i = wave * (kSmallMax / NW) + e * 64 + lane;
      if (valid[e]) { key[e] = s_k[i]; pos[e] = s_p[i]; }
    }
    __syncthreads();
  }
  uint2* keys = a.kp + at.key0;
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int i = wave * (kSmallMax / NW) + e * 64 + lane;
    if (valid[e]) keys[i] = make_uint2(key[e], pos[e]);
  }
  uint2* m1 = a.meta1 + at.ch1 * 2;
  for (int i = threadIdx.x; i < 2 * nch1; i += kSmallThreads) m1[i] = make_uint2(kMetaNone, 0);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

  float* p0 = a.partial + at.ch0 * 2 * a.D;
  uint2* m0 = a.meta + at.ch0 * 2;
  const int team = threadIdx.x / kRedThreads, ttid = threadIdx.x % kRedThreads;
  const int ntiles = (int)((N + tile - 1) / tile);
  for (int t0 = 0; t0 < ntiles; t0 += kSmallRedParts) {
    reduce_tile_body<VEC, false, R, WT, true, false, true>(tb, keys, p0, m0, N, nch0, tile, t0 + team, L, a.D, a.avg != 0, op, st0, st1, sk, sm.red[team], ttid, false,
                                                   nullptr, wgt);
    __syncthreads();
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

  const int nvec = a.D / VEC;
  const int lpr = nvec < 64 ? nvec : 64;
  const int rpw = 64 / lpr;
  const int64_t group0 = (int64_t)wave * rpw + lane / lpr;
  const int64_t ngroups = (int64_t)NW * rpw;
  float* p1 = a.partial1 + at.ch1 * 2 * a.D;
  if (nch1 > 1) {
    fold_table_body<VEC, false, R, WT>(tb, p0, m0, p1, m1, nch0, FFH_EMB_CHUNK1 / FFH_EMB_CHUNK, a.D, op, st0, st1, sk, 0, 2 * (int64_t)nch0, group0, ngroups);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    fold_table_body<VEC, false, R, WT>(tb, p1, m1, p1, m1, nch1, 0, a.D, op, st0, st1, sk, 0, 2 * (int64_t)nch1, group0, ngroups);
  } else {
    fold_table_body<VEC, false, R, WT>(tb, p0, m0, p1, m1, nch0, 0, a.D, op, st0, st1, sk, 0, 2 * (int64_t)nch0, group0, ngroups);
  }
}


template <class WT, int I> void launch_bagw_small(const BagsUpdateLaunch& u) {
  hipLaunchKernelGGL((emb_bagw_small_kernel<(I >> 1 & 1) ? 4 : 1, (RowRule)(I >> 2), WT, (I & 1) != 0>), u.grid, dim3(kSmallThreads), 0, u.stream, *u.small);
}
template <class WT, int I> void launch_bagw_reduce(const BagsUpdateLaunch& u) {
  hipLaunchKernelGGL((emb_bagw_reduce_kernel<(I >> 1 & 1) ? 4 : 1, (RowRule)(I >> 2), WT, (I & 1) != 0>), u.grid, dim3(kRedThreads), 0, u.stream, *u.red);
}
template <class WT, int... I>
bool bagw_update_launch(const BagsUpdateLaunch& u, std::integer_sequence<int, I...>) {      // (rule, VEC, LRP) -> kernel, as emb_bags_update_launch
  static constexpr BagsUpdateFn kSmall[] = {launch_bagw_small<WT, I>...};
  static constexpr BagsUpdateFn kReduce[] = {launch_bagw_reduce<WT, I>...};
  const int i = update_index(u.rule, u.v4, u.lrp);
  if (i < 0 || i >= (int)sizeof...(I) || (u.small != nullptr) == (u.red != nullptr)) return false;
  if (u.small) kSmall[i](u); else kReduce[i](u);
  return true;
}

}  // namespace

namespace ffh_emb {
bool emb_bagw_update_launch_f32(const BagsUpdateLaunch& u) { return bagw_update_launch<float>(u, std::make_integer_sequence<int, kUpdateEntries>()); }
bool emb_bagw_update_launch_bf16(const BagsUpdateLaunch& u) { return bagw_update_launch<uint16_t>(u, std::make_integer_sequence<int, kUpdateEntries>()); }
}  // namespace ffh_emb

extern "C" {

int ffh_bag_weights_abi_version(void) { return FFH_BAG_WEIGHTS_ABI_VERSION; }

int ffh_embedding_fwd_multi_bags_weighted(ffh_ctx* c, const ffh_emb_table* tables, const float* const* weights, const int* in_dims, int nt, int D,
                                          int64_t batch, int aggr, ffh_stream s) {
  return bagw_fwd_launch<float>(c, tables, weights, in_dims, nt, D, batch, aggr, s);
}

int ffh_embedding_fwd_multi_bags_weighted_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, const float* const* weights, const int* in_dims, int nt,
                                               int D, int64_t batch, int aggr, ffh_stream s) {
  ffh_emb_table t[FFH_MAX_TABLES];
  const int rc = bf16_tables(c, tables, nt, t, nullptr);
  if (rc) return rc;
  return bagw_fwd_launch<uint16_t>(c, t, weights, in_dims, nt, D, batch, aggr, s);
}

int ffh_embedding_bwd_fused_multi_bags_weighted(ffh_ctx* c, const ffh_bags_update_weighted* u, ffh_stream s) {
  if (!u) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_fused_multi_bags_weighted: null descriptor");
  return emb_bwd_bags_weighted(c, &u->u, u->weights, s, true);
}

int ffh_embedding_bwd_apply_multi_bags_weighted(ffh_ctx* c, const ffh_bags_update_weighted* u, ffh_stream s) {
  if (!u) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_apply_multi_bags_weighted: null descriptor");
  return emb_bwd_bags_weighted(c, &u->u, u->weights, s, false);
}

}  // extern "C"
