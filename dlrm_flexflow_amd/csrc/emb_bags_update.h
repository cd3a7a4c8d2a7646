// emb_bags_update.h -- the fused table update of tables with a bag size PER TABLE, in one call (include/ff_hip_bags_update.h): ragged forms
// of the sort kernels (emb_sort.h) and of the apply phase's kernels (emb_reduce.h).  Every table keeps its own geometry -- N_t = batch * L_t
// entries, its own share of the key buffers, histogram matrix, level-0 / level-1 slots and arrival counters, its own nchunks / nchunks1 --
// and the arithmetic is the uniform kernels' device bodies (reduce_tile_body, fold_table_body, sort_scan_offsets, sort_rank_and_scatter, the
// row rules), so a table ends with the bits of its own uniform call.  Nothing here is reached by the uniform entries.  The kernels' PAD forms
// (include/ff_hip_pad.h: an id < 0 is no lookup) are instantiated only for the pad entries; with PAD = false a kernel is what it was.
// Included by the two translation units that instantiate the kernels (embedding_update_bags_f32.hip / _bf16.hip) and by embedding.hip for the
// argument structs and the geometry.
#pragma once
#include "emb_reduce.h"

namespace ffh_emb {

// ---------------------------------------------------------------------------
// Geometry.  The kernel arguments carry the bag sizes in 16 bits and nothing else per table: the tables' offsets are DERIVED, by the one
// function below, on the host (workspace layout, grid sizes) and in every workgroup (a uniform loop over <= 64 entries of the kernel
// arguments: scalar loads and scalar arithmetic).  64 tables with explicit 64-bit offsets for five arrays would not fit the 4 KB of kernel
// arguments beside the table descriptors and the state pointers; a table in device memory would be rewritten by the host under a captured
// launch.
// The workgroup map is FLAT: table t owns exactly ceil(N_t / tile) consecutive workgroups of the grid (a (largest table's tiles x tables)
// grid is almost all empty workgroups at bag sizes 1 .. 100).
// ---------------------------------------------------------------------------
struct BagsGeo {
  uint16_t L[FFH_MAX_TABLES];   // bag size of table t (1 .. FFH_BAGS_MAX_IN_DIM)
  int64_t  batch;
  int      nt;
  int      sort_sh;             // log2 of the sort kernels' tile (256 * E entries)
  int      red_sh;              // log2 of the reduce kernel's tile (128 .. 1024 entries)
};

// where a table's shares begin, in units of: entries (key buffers), sort tiles (histogram rows), FFH_EMB_CHUNK blocks (level-0 slots: two
// per block), FFH_EMB_CHUNK1 blocks (level-1 slots: two per block; arrival counters: one per block and one more per table)
struct BagsAt {
  int     t;
  int64_t local;                // the workgroup's tile inside table t
  int64_t N;                    // the table's entries
  int64_t key0, sblk0, ch0, ch1;
};

__host__ __device__ inline int64_t bags_ceil_sh(int64_t n, int sh) { return (n + ((int64_t)1 << sh) - 1) >> sh; }
__host__ __device__ inline int bags_nchunks(int64_t N) { return (int)((N + FFH_EMB_CHUNK - 1) / FFH_EMB_CHUNK); }
__host__ __device__ inline int bags_nchunks1(int64_t N) { return (int)((N + FFH_EMB_CHUNK1 - 1) / FFH_EMB_CHUNK1); }

// The table that holds tile `w` of the flat map with 2^map_sh entries per tile (map_sh < 0: the table w itself, local = 0) and the offsets
// of its shares.  False: w lies behind the last table -- `o` then holds the totals (t = nt, local = the tiles of all tables).
__host__ __device__ inline bool bags_locate(const BagsGeo& g, const int map_sh, const int64_t w, BagsAt* o) {
  BagsAt a;
  a.t = 0; a.local = w; a.N = 0; a.key0 = 0; a.sblk0 = 0; a.ch0 = 0; a.ch1 = 0;
  int64_t tiles = 0;
  for (int t = 0; t < g.nt; t++) {
    const int64_t N = g.batch * (int64_t)g.L[t];
    const int64_t nb = map_sh < 0 ? 1 : bags_ceil_sh(N, map_sh);
    if (a.local < nb) { a.t = t; a.N = N; *o = a; return true; }
    a.local -= nb;
    tiles += nb;
    a.key0 += N;
    a.sblk0 += bags_ceil_sh(N, g.sort_sh);
    a.ch0 += bags_nchunks(N);
    a.ch1 += bags_nchunks1(N);
  }
  a.t = g.nt; a.local = tiles;
  *o = a;
  return false;
}

// ---------------------------------------------------------------------------
// Kernel arguments.  The per-call table cap is FFH_MAX_TABLES (64): the byte counts are asserted below.
// ---------------------------------------------------------------------------
struct BagsSortArgs {
  const int64_t* idx[FFH_MAX_TABLES];   // pass 0 source
  const uint2* src;                     // [sum N_t] {row id, position}, table t at key0(t)
  uint2*    dst;
  uint32_t* hist;                       // [sum nblk_t][radix], table t at sblk0(t)
  int       shift, bits, pass;
  int       nclear[2];                  // dwords the pass-0 histogram kernel zeroes for the apply phase: every table's level-1 slots, counters
  uint32_t* clear[2];
  uint8_t   npass[FFH_MAX_TABLES];      // digits table t really has
  BagsGeo   g;
  uint32_t  padkey[FFH_MAX_TABLES];     // the pad forms' pass 0 (include/ff_hip_pad.h): an id < 0 sorts as this key, the table's num_entries
};

struct BagsRedArgs {
  ffh_emb_table t[FFH_MAX_TABLES];
  const uint2* kp[2];                   // sorted {row id, position}: table t ends in buffer parity[t], at key0(t)
  uint8_t   parity[FFH_MAX_TABLES];
  float*    partial;  uint2* meta;      // level-0 slots [2 * sum nchunks_t], table t at 2 * ch0(t)
  float*    partial1; uint2* meta1;     // level-1 slots [2 * sum nchunks1_t], table t at 2 * ch1(t) (cleared by the sort phase)
  uint32_t* arrive;                     // [sum (nchunks1_t + 1)], table t at ch1(t) + t (cleared by the sort phase)
  int       D, avg;
  BagsGeo   g;
  OptP      op;
  float*    s0[FFH_MAX_TABLES];
  union { float* s1[FFH_MAX_TABLES]; Bf16Keys b16; Bf16AdamKeys b16a; };     // as in RedArgs
  const uint16_t* cnt;                  // the mean forms (include/ff_hip_pad_mean.h): real lookups per bag, [table][batch]; else null and never read
};

struct BagsSmallArgs {
  ffh_emb_table t[FFH_MAX_TABLES];
  uint8_t   npass[FFH_MAX_TABLES];
  uint2*    kp;                         // [sum N_t] sorted {row id, position}   (workspace)
  float*    partial;  uint2* meta;
  float*    partial1; uint2* meta1;
  int       rb, D, avg, pad_;
  BagsGeo   g;
  OptP      op;
  float*    s0[FFH_MAX_TABLES];
  union { float* s1[FFH_MAX_TABLES]; Bf16Keys b16; Bf16AdamKeys b16a; };
  const uint16_t* cnt;                  // as BagsRedArgs::cnt
};

// the count kernel of the mean forms (include/ff_hip_pad_mean.h): cnt[t][b] = ids >= 0 in bag b of table t
struct BagsCountArgs {
  const int64_t* idx[FFH_MAX_TABLES];
  uint16_t  L[FFH_MAX_TABLES];
  uint16_t* cnt;                        // [nt][batch]
  int64_t   batch;
  int       nt;
};
constexpr int kCountThreads = 256;
constexpr int kCountSlots = 1024;       // id slots a workgroup takes at most, in whole bags; a longer bag has a workgroup to itself
// the bags of a table with bag size L that one workgroup counts, and the table's workgroups: host and kernel compute the flat map with these
__host__ __device__ inline int count_bags_per_wg(int L) { return L >= kCountSlots ? 1 : kCountSlots / L; }
__host__ __device__ inline int64_t count_wgs(int64_t batch, int L) { const int b = count_bags_per_wg(L); return (batch + b - 1) / b; }

constexpr size_t kBagsKernargBytes = sizeof(BagsRedArgs) > sizeof(BagsSmallArgs)
                                         ? (sizeof(BagsRedArgs) > sizeof(BagsSortArgs) ? sizeof(BagsRedArgs) : sizeof(BagsSortArgs))
                                         : (sizeof(BagsSmallArgs) > sizeof(BagsSortArgs) ? sizeof(BagsSmallArgs) : sizeof(BagsSortArgs));
static_assert(sizeof(BagsGeo) == 2 * FFH_MAX_TABLES + 24, "BagsGeo: 16-bit bag sizes");
static_assert(sizeof(BagsRedArgs) == 3944 && sizeof(BagsSmallArgs) == 3936 && kBagsKernargBytes <= 4096 && sizeof(BagsCountArgs) <= 4096, "kernel arguments: 64 tables inside 4 KB");
static_assert(offsetof(BagsRedArgs, cnt) == 3936 && offsetof(BagsSmallArgs, cnt) == 3928, "the counts lie behind the members the existing kernels read");

namespace {

// ---------------------------------------------------------------------------
// sort: radix_hist_kernel / radix_scatter_kernel (emb_sort.h) on the flat map
// ---------------------------------------------------------------------------
// PAD (pass 0 only; include/ff_hip_pad.h): an id < 0 is no lookup and sorts as the table's largest key, padkey[t] = num_entries
template <bool PAD>
__device__ __forceinline__ uint32_t bags_first_key(const int64_t id, const uint32_t padkey) {
  if (PAD) return id < 0 ? padkey : (uint32_t)id;
  return (uint32_t)id;
}

template <bool FIRST, int E, bool PAD = false>
__global__ __launch_bounds__(kSortThreads) void bags_radix_hist_kernel(const BagsSortArgs a) {
  ffh_kernel_prio();
  constexpr int kSortTile = kSortThreads * E;
  __shared__ uint32_t s_hist[kMaxRadix];
  if (FIRST) {     // every table has a pass 0: the apply phase finds every level-1 slot empty and every arrival counter at zero
#pragma unroll
    for (int r = 0; r < 2; r++)
      for (int64_t i = (int64_t)blockIdx.x * kSortThreads + threadIdx.x; i < a.nclear[r]; i += (int64_t)gridDim.x * kSortThreads)
        a.clear[r][i] = 0u;
  }
  BagsAt at;
  if (!bags_locate(a.g, a.g.sort_sh, blockIdx.x, &at)) return;
  const int t = at.t;
  if (a.pass >= a.npass[t]) return;
  const int radix = 1 << a.bits;
  const uint32_t mask = radix - 1;
  for (int d = threadIdx.x; d < radix; d += kSortThreads) s_hist[d] = 0;
  __syncthreads();
  const int64_t tile0 = at.local * kSortTile;
  const int64_t* __restrict__ idx = a.idx[t];
  const uint2* __restrict__ src = a.src + at.key0;
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int64_t i = tile0 + e * kSortThreads + threadIdx.x;
    if (i < at.N) atomicAdd(&s_hist[((FIRST ? bags_first_key<PAD>(idx[i], a.padkey[t]) : src[i].x) >> a.shift) & mask], 1u);
  }
  __syncthreads();
  uint32_t* out = a.hist + (at.sblk0 + at.local) * radix;
  for (int d = threadIdx.x; d < radix; d += kSortThreads) out[d] = s_hist[d];
}

template <bool FIRST, int E, bool PAD = false>
__global__ __launch_bounds__(kSortThreads) void bags_radix_scatter_kernel(const BagsSortArgs a) {
  ffh_kernel_prio();
  constexpr int kSortTile = kSortThreads * E;
  BagsAt at;
  if (!bags_locate(a.g, a.g.sort_sh, blockIdx.x, &at)) return;
  const int t = at.t;
  if (a.pass >= a.npass[t]) return;
  __shared__ uint32_t s_off[4][kMaxRadix];
  __shared__ uint32_t s_scan[kMaxRadix];
  __shared__ uint32_t s_wsum[4];
  const int blk = (int)at.local;
  const int nblk = (int)bags_ceil_sh(at.N, a.g.sort_sh);
  const int radix = 1 << a.bits;
  const uint32_t mask = radix - 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile0 = (int64_t)blk * kSortTile;
  const int shift = a.shift;
  const int64_t* __restrict__ idx = a.idx[t];
  const uint2* __restrict__ src = a.src + at.key0;

  for (int d = threadIdx.x; d < 4 * kMaxRadix; d += kSortThreads) (&s_off[0][0])[d] = 0;
  __syncthreads();

  uint32_t key[E], pos[E];
  bool valid[E];
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int64_t i = tile0 + wave * (kSortTile / 4) + e * 64 + lane;
    valid[e] = i < at.N;
    if (FIRST) {
      key[e] = valid[e] ? bags_first_key<PAD>(idx[i], a.padkey[t]) : 0u;
      pos[e] = (uint32_t)i;
    } else {
      const uint2 kp = valid[e] ? src[i] : make_uint2(0u, 0u);
      key[e] = kp.x; pos[e] = kp.y;
    }
    if (valid[e]) atomicAdd(&s_off[wave][(key[e] >> shift) & mask], 1u);
  }
  __syncthreads();

  // global base of every digit for this tile, inside the table: digits below (all the table's tiles) + same digit, earlier tiles
  const uint32_t* hist_t = a.hist + at.sblk0 * radix;
  uint32_t all_d[2] = {0, 0}, before_d[2] = {0, 0};
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const int d = threadIdx.x + q * kSortThreads;
    if (d < radix) {
      uint32_t all = 0, before = 0;
      int b2 = 0;
      for (; b2 + 8 <= nblk; b2 += 8) {
        uint32_t h[8];
#pragma unroll
        for (int u = 0; u < 8; u++) h[u] = hist_t[(int64_t)(b2 + u) * radix + d];
#pragma unroll
        for (int u = 0; u < 8; u++) { all += h[u]; before += (b2 + u < blk) ? h[u] : 0u; }
      }
      for (; b2 < nblk; b2++) {
        const uint32_t h = hist_t[(int64_t)b2 * radix + d];
        all += h;
        before += (b2 < blk) ? h : 0u;
      }
      all_d[q] = all; before_d[q] = before;
    }
  }
  sort_scan_offsets<4, 2>(all_d, before_d, radix, s_off, s_scan, s_wsum);
  sort_rank_and_scatter<E>(key, pos, valid, shift, a.bits, mask, s_off[wave], SortOutGlobal{a.dst + at.key0});
}

// ---------------------------------------------------------------------------
// apply, sorted route: emb_sgd_reduce_kernel's LSD form on the flat map.  Cross-workgroup traffic as there: a tile's partial rows and slot
// records go out written through and completed before it counts itself in; the last tile of a 1024-block folds the block, the last folded
// block of a table folds the table.  No workgroup waits for another.
// ---------------------------------------------------------------------------
template <int VEC, RowRule R, class WT, bool LRP, bool PAD = false, bool MEAN = false>
__global__ __launch_bounds__(kRedThreads, (red_waves_per_simd<VEC, R, WT, false>())) void emb_bags_reduce_kernel(const BagsRedArgs a) {
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
  const ffh_emb_table& tb = a.t[tix];
  const uint2* keys = a.kp[a.parity[tix]] + at.key0;
  float* p0 = a.partial + at.ch0 * 2 * a.D;
  uint2* m0 = a.meta + at.ch0 * 2;
  float* const st0 = opt_state(R) ? a.s0[tix] : nullptr;
  float* const st1 = state1_of<R, WT>(a, tix);
  const SrKey sk = sr_key<R, WT>(a, tix);
  reduce_tile_body<VEC, true, R, WT, PAD, MEAN>(tb, keys, p0, m0, N, nchunks, tile, (int)at.local, L, a.D, a.avg != 0, op, st0, st1, sk, sh, threadIdx.x, false,
                                                MEAN ? a.cnt + (int64_t)tix * a.g.batch : nullptr);

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

// ---------------------------------------------------------------------------
// apply, small route (every N_t <= kSmallMax): emb_sgd_small_kernel with the table's own N_t -- sort, reduce and folds of a table in its
// one workgroup
// ---------------------------------------------------------------------------
template <int VEC, RowRule R, class WT, bool LRP, bool PAD = false, bool MEAN = false>
__global__ __launch_bounds__(kSmallThreads) void emb_bags_small_kernel(const BagsSmallArgs a) {
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
  const ffh_emb_table tb = a.t[tix];
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
    key[e] = valid[e] ? bags_first_key<PAD>(tb.idx[i], (uint32_t)tb.num_entries) : 0u;
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
    reduce_tile_body<VEC, false, R, WT, PAD, MEAN>(tb, keys, p0, m0, N, nch0, tile, t0 + team, L, a.D, a.avg != 0, op, st0, st1, sk, sm.red[team], ttid, false,
                                                   MEAN ? a.cnt + (int64_t)tix * a.g.batch : nullptr);
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

}  // namespace

// ---------------------------------------------------------------------------
// The launch tables, as emb_reduce.h keeps them: (rule, VEC, LRP) index one table per weight type and translation unit.
// ---------------------------------------------------------------------------
struct BagsUpdateLaunch {
  RowRule rule; bool v4, lrp;
  const BagsSmallArgs* small;           // the small route's arguments, or null: ...
  const BagsRedArgs* red;               // ... the sorted route's
  dim3 grid;
  hipStream_t stream;
};
typedef void (*BagsUpdateFn)(const BagsUpdateLaunch&);
namespace {
template <class WT, bool PAD, bool MEAN, int I> void launch_bags_small(const BagsUpdateLaunch& u) {
  hipLaunchKernelGGL((emb_bags_small_kernel<(I >> 1 & 1) ? 4 : 1, (RowRule)(I >> 2), WT, (I & 1) != 0, PAD, MEAN>), u.grid, dim3(kSmallThreads), 0, u.stream, *u.small);
}
template <class WT, bool PAD, bool MEAN, int I> void launch_bags_reduce(const BagsUpdateLaunch& u) {
  hipLaunchKernelGGL((emb_bags_reduce_kernel<(I >> 1 & 1) ? 4 : 1, (RowRule)(I >> 2), WT, (I & 1) != 0, PAD, MEAN>), u.grid, dim3(kRedThreads), 0, u.stream, *u.red);
}
// PAD: the pad forms (include/ff_hip_pad.h), compiled in translation units of their own (embedding_update_pad_f32.hip / _bf16.hip)
// MEAN: their mean forms (include/ff_hip_pad_mean.h), likewise (embedding_update_padmean_f32.hip / _bf16.hip)
template <class WT, bool PAD, bool MEAN = false, int... I>
bool emb_bags_update_launch(const BagsUpdateLaunch& u, std::integer_sequence<int, I...>) {
  static constexpr BagsUpdateFn kSmall[] = {launch_bags_small<WT, PAD, MEAN, I>...};
  static constexpr BagsUpdateFn kReduce[] = {launch_bags_reduce<WT, PAD, MEAN, I>...};
  const int i = update_index(u.rule, u.v4, u.lrp);
  if (i < 0 || i >= (int)sizeof...(I) || (u.small != nullptr) == (u.red != nullptr)) return false;
  if (u.small) kSmall[i](u); else kReduce[i](u);
  return true;
}
}  // namespace

__attribute__((visibility("hidden"))) bool emb_bags_update_launch_f32(const BagsUpdateLaunch& u);      // embedding_update_bags_f32.hip
__attribute__((visibility("hidden"))) bool emb_bags_update_launch_bf16(const BagsUpdateLaunch& u);     // embedding_update_bags_bf16.hip
// one pass of the ragged sort (histogram + scatter; `first`: pass 0, which reads the int64 ids), E = entries per thread; embedding_update_bags_f32.hip
__attribute__((visibility("hidden"))) bool emb_bags_sort_pass(const BagsSortArgs& a, bool first, int E, dim3 grid, hipStream_t stream);
// the pad forms (include/ff_hip_pad.h): the apply kernels that drop the pad key's segment, and pass 0 of the sort, which loads a pad as that key
__attribute__((visibility("hidden"))) bool emb_pad_update_launch_f32(const BagsUpdateLaunch& u);       // embedding_update_pad_f32.hip
__attribute__((visibility("hidden"))) bool emb_pad_update_launch_bf16(const BagsUpdateLaunch& u);      // embedding_update_pad_bf16.hip
__attribute__((visibility("hidden"))) bool emb_pad_sort_first_pass(const BagsSortArgs& a, int E, dim3 grid, hipStream_t stream);      // embedding_update_pad_f32.hip
// the mean forms (include/ff_hip_pad_mean.h): the apply kernels that divide a gradient row by its bag's count of real lookups, and the kernel that counts
__attribute__((visibility("hidden"))) bool emb_padmean_update_launch_f32(const BagsUpdateLaunch& u);   // embedding_update_padmean_f32.hip
__attribute__((visibility("hidden"))) bool emb_padmean_update_launch_bf16(const BagsUpdateLaunch& u);  // embedding_update_padmean_bf16.hip
__attribute__((visibility("hidden"))) void emb_padmean_count(const BagsCountArgs& a, hipStream_t stream);      // embedding_update_padmean_f32.hip

}  // namespace ffh_emb
