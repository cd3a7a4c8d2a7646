// emb_reduce.h -- the apply phase of the fused table update (embedding.hip): segmented reduce of the sorted list, the folds, the row rule;
// the sorted routes' kernel (emb_sgd_reduce_kernel), the small-batch kernel (emb_sgd_small_kernel) and the table their launches go through.
// Included by the two translation units that instantiate the kernels, one per weight type, and by embedding.hip for the argument structs.
#pragma once
#include "emb_row_rules.h"
#include "emb_sort.h"

#include <utility>

namespace ffh_emb {

// ---------------------------------------------------------------------------
// fused backward + SGD, step 2: segmented reduce of the sorted list + row update
// ---------------------------------------------------------------------------
constexpr int kRedThreads = 256;
constexpr int kRedTile = 1024;                        // max sorted entries per workgroup; the call picks 128..1024
constexpr int kRedChunksPerTile = kRedTile / FFH_EMB_CHUNK;
static_assert(kRedTile % FFH_EMB_CHUNK == 0, "tile must hold whole chunks");

enum : uint32_t { kMetaNone = 0, kMetaFirst = 1, kMetaCont = 2 };

struct RedArgs {
  ffh_emb_table t[FFH_MAX_TABLES];
  const uint2* kp[2];       // sorted {row id, position} [nt][N]: table t ends in buffer parity[t]
  uint8_t   parity[FFH_MAX_TABLES];
  int       tile;           // sorted entries per workgroup: multiple of FFH_EMB_CHUNK, <= kRedTile
  float*    partial;        // level-0 partial rows [nt][2*nchunks][D] (2 slots per FFH_EMB_CHUNK block)
  uint2*    meta;           // [nt][2*nchunks] {kind, key}
  int64_t   N;
  int       nchunks;
  int       L;
  int       D;
  int       avg;
  float*    partial1;       // level-1 partial rows [nt][2*nchunks1][D]
  uint2*    meta1;          // level-1 slots [nt][2*nchunks1] (cleared by the sort phase)
  uint32_t* arrive;         // [nt][nchunks1 + 1] (cleared by the sort phase): tiles done per 1024-block, then 1024-blocks folded
  int       nchunks1;
  OptP      op;             // the row rule's parameters (op.lr = the plain update's lr)
  float*    s0[FFH_MAX_TABLES];   // Momentum: V; Adam: M; Adagrad: S -- [num_entries][D] like the table; RowwiseAdagrad: S [num_entries]; or null
  union {
    float*  s1[FFH_MAX_TABLES];   // Adam: second moment V
    Bf16Keys b16;                 // bf16 rows: the tables' rounding keys
    Bf16AdamKeys b16a;            // Adam on bf16 rows: s1 and the keys of at most FFH_BF16_MAX_STATEFUL_TABLES tables
  };
  // bucket form (emb_sgd_reduce_kernel<.., MSD = true>): kp[parity] is ordered by the top digit only
  uint8_t   shift_t[FFH_MAX_TABLES];   // the digit's position (0: the table is completely sorted)
  const uint32_t* bstart;         // [nt][kMaxRadix + 1] bucket starts
  uint32_t* nextkey;              // [nt][nchunks1]: the row id behind each 1024-block (written by the block's last tile, read by its fold)
  int       radix;
};

// the small-batch kernel's arguments (emb_sgd_small_kernel)
struct SmallArgs {
  ffh_emb_table t[FFH_MAX_TABLES];
  uint8_t   npass[FFH_MAX_TABLES];
  uint2*    kp;        // [nt][N] sorted {row id, position}   (workspace)
  float*    partial;   uint2* meta;    // level-0 slots [nt][2*nch0]   (the slots' names are RedArgs': the host fills both alike)
  float*    partial1;  uint2* meta1;   // level-1 slots [nt][2*nch1]
  int64_t   N;
  int nch0, nch1, rb, L, D, avg;
  int tile;            // sorted entries per reduce team (multiple of FFH_EMB_CHUNK, <= kRedTile)
  OptP op;
  float* s0[FFH_MAX_TABLES];
  union { float* s1[FFH_MAX_TABLES]; Bf16Keys b16; Bf16AdamKeys b16a; };     // as in RedArgs
};

// The byte layout of the kernel arguments is fixed: the kernels read every member at the offset they always did
static_assert(sizeof(RedArgs) == 3904 && offsetof(RedArgs, op) == 2720 && offsetof(RedArgs, s0) == 2792 && offsetof(RedArgs, s1) == 3304 &&
              offsetof(RedArgs, b16) == 3304, "RedArgs layout");
static_assert(sizeof(SmallArgs) == 3800 && offsetof(SmallArgs, op) == 2704 && offsetof(SmallArgs, s0) == 2776 && offsetof(SmallArgs, s1) == 3288 &&
              offsetof(SmallArgs, b16) == 3288, "SmallArgs layout");
static_assert(sizeof(RedArgs) <= 4096 && sizeof(SmallArgs) <= 4096, "kernel arguments");

namespace {

template <int VEC>
__device__ __forceinline__ void load_grad(float (&dst)[VEC], const float* rowp, int c, float invdiv, bool avg) {
  if (VEC == 4) {
    const float4 v = reinterpret_cast<const float4*>(rowp)[c];
    dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
  } else {
    dst[0] = rowp[c];
  }
  if (avg) {
#pragma unroll
    for (int v = 0; v < VEC; v++) dst[v] = dst[v] / invdiv;
  }
}

// Partial rows and slot records that one workgroup writes and ANOTHER reads inside the same launch (the folds in the tail of
// emb_sgd_reduce_kernel).  The eight XCDs' L2s are not coherent with each other for ordinary accesses inside a kernel, and an
// agent-scope fence pays for that with a write-back of the whole L2 (measured: 4x on the kernel, the L2 is full of the table
// rows just written).  Instead these few accesses are agent-scope relaxed atomics -- `sc1` stores (written through) and `sc1`
// loads (served behind the L2) -- ordered by completion: the writer waits for its stores (vmcnt) before it counts itself in, the
// reader loads after it has seen the count.  AGENT = false: the one-workgroup small-batch kernel, ordinary accesses.
__device__ __forceinline__ void xwg_stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
template <bool AGENT>
__device__ __forceinline__ void xwg_store2(uint2* p, uint2 v) {
  if (AGENT) __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), ((unsigned long long)v.y << 32) | v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
template <bool AGENT>
__device__ __forceinline__ uint2 xwg_load2(const uint2* p) {
  if (!AGENT) return *p;
  const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
}
template <int VEC, bool AGENT>
__device__ __forceinline__ void xwg_store_row(float* rowp, int c, const float (&v)[VEC]) {
  if (VEC == 4) {
    if (AGENT) {
      xwg_store2<true>(reinterpret_cast<uint2*>(rowp) + 2 * c, make_uint2(__float_as_uint(v[0]), __float_as_uint(v[1])));
      xwg_store2<true>(reinterpret_cast<uint2*>(rowp) + 2 * c + 1, make_uint2(__float_as_uint(v[2]), __float_as_uint(v[3])));
    } else {
      reinterpret_cast<float4*>(rowp)[c] = make_float4(v[0], v[1], v[2], v[3]);
    }
  } else {
    if (AGENT) __hip_atomic_store(rowp + c, v[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else rowp[c] = v[0];
  }
}
template <int VEC, bool AGENT>
__device__ __forceinline__ void xwg_load_row(float (&dst)[VEC], const float* rowp, int c) {
  if (VEC == 4) {
    if (AGENT) {
      const uint2 lo = xwg_load2<true>(reinterpret_cast<const uint2*>(rowp) + 2 * c), hi = xwg_load2<true>(reinterpret_cast<const uint2*>(rowp) + 2 * c + 1);
      dst[0] = __uint_as_float(lo.x); dst[1] = __uint_as_float(lo.y); dst[2] = __uint_as_float(hi.x); dst[3] = __uint_as_float(hi.y);
    } else {
      const float4 v = reinterpret_cast<const float4*>(rowp)[c];
      dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
  } else {
    dst[0] = AGENT ? __hip_atomic_load(rowp + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : rowp[c];
  }
}

constexpr int kFoldStage = 1024;     // slot records of one fold staged in LDS (a 1024-block has 64; a table's 1024-blocks: 2 N / 1024)
struct RedShared {
  uint32_t key[kRedTile + 2];     // [0] = key before the tile, [1+i], [1+n] = key after
  uint32_t pos[kRedTile];
  uint16_t start[kRedTile + 1];
  uint32_t cnt[(kRedTile / 64) + 1];
  uint2    meta[2 * kRedChunksPerTile];   // 64 at FFH_EMB_CHUNK = 32
};

// one tile of one table; `partial_t` / `meta_t` are the table's level-0 slot arrays
// PAD (include/ff_hip_pad.h; the ragged kernels' pad forms only): the sort loaded "no lookup" as key tb.num_entries, the largest key.  Its
// sub-runs are dropped here: no sum, no row, no partial row and no slot record -- the folds walk slot records, so they never see the segment.
// MEAN (include/ff_hip_pad_mean.h; PAD forms only): the divisor of entry i is the count of real lookups of its sample, cnt[s_pos[i]] (the
// table's 16-bit counts, [batch]), read where the gradient row is loaded, in place of (float)L.  An entry that is summed is a real lookup, so
// its count is at least 1.  With MEAN false the body is what it was.
template <int VEC, bool AGENT, RowRule R, class WT, bool PAD = false, bool MEAN = false>
__device__ __forceinline__ void reduce_tile_body(const ffh_emb_table& tb, const uint2* kp,
                                                 float* partial_t, uint2* meta_t, int64_t N, int nchunks, int tile, int tile_index,
                                                 int L, int D_, bool avg_, const OptP& op, float* st0, float* st1, const SrKey& sk, RedShared& sh, const int tid = threadIdx.x,
                                                 const bool preloaded = false, const uint16_t* __restrict__ cnt = nullptr) {
  uint32_t* s_key = sh.key;
  uint32_t* s_pos = sh.pos;
  uint16_t* s_start = sh.start;
  uint32_t* s_cnt = sh.cnt;
  uint2* s_meta = sh.meta;
  struct { int64_t N; int nchunks, L, D, avg; } a = {N, nchunks, L, D_, avg_ ? 1 : 0};
  const int64_t tile0 = (int64_t)tile_index * tile;
  const int n = tile0 >= N ? 0 : (int)((N - tile0) < tile ? (N - tile0) : tile);   // a tile past the end still walks the barriers
  const int lane = tid & 63, wave = tid >> 6;

  if (!preloaded) {       // (preloaded: the caller has filled s_key[0 .. n + 1] and s_pos[0 .. n) -- the bucket form, msd_window)
    for (int i = tid; i < n; i += kRedThreads) {
      const uint2 e = kp[tile0 + i];
      s_key[1 + i] = e.x;
      s_pos[i] = a.L == 1 ? e.y : e.y / (uint32_t)a.L;      // the sample (gradient row) of the entry
    }
    if (tid == 0) {
      s_key[0] = (tile0 > 0 && tile0 < N) ? kp[tile0 - 1].x : 0xFFFFFFFFu;   // no valid key equals it when tile0 == 0 (checked below)
      s_key[1 + n] = (tile0 + n < N) ? kp[tile0 + n].x : 0xFFFFFFFFu;
    }
  }
  const int metas = 2 * (tile / FFH_EMB_CHUNK);
  if (tid < metas) s_meta[tid] = make_uint2(kMetaNone, 0);
  __syncthreads();

  // sub-run starts: chunk boundaries and changes of row id; compacted in order
  // entry handled by (wave, e, lane) = wave*256 + e*64 + lane keeps the list sorted
  const bool at_table_start = tile0 == 0;
  bool st[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int i = wave * 256 + e * 64 + lane;
    bool s = false;
    if (i < n) s = (i % FFH_EMB_CHUNK == 0) || (s_key[1 + i] != s_key[i]) || (i == 0 && at_table_start);
    st[e] = s;
    const unsigned long long bal = __ballot(s);
    if (lane == 0) s_cnt[wave * 4 + e] = __popcll(bal);
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t run = 0;
    for (int q = 0; q < kRedTile / 64; q++) { const uint32_t c = s_cnt[q]; s_cnt[q] = run; run += c; }
    s_cnt[kRedTile / 64] = run;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int i = wave * 256 + e * 64 + lane;
    const unsigned long long bal = __ballot(st[e]);
    if (st[e]) s_start[s_cnt[wave * 4 + e] + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)i;
  }
  const int S = (int)s_cnt[kRedTile / 64];
  if (tid == 0) s_start[S] = (uint16_t)n;
  __syncthreads();

  // lane-groups walk the sub-runs
  const int D = a.D;
  const int nvec = D / VEC;
  const int lpr = nvec < 64 ? nvec : 64;
  const int rpw = 64 / lpr;
  const int rsub = lane / lpr;
  const int c0 = lane - rsub * lpr;
  const int groups = (kRedThreads / 64) * rpw;
  const int gid = wave * rpw + rsub;
  const float Lf = (float)a.L;
  const bool avg = a.avg != 0;
  auto div_of = [&](const int q) -> float {      // the divisor of sorted entry q of the tile
    if constexpr (MEAN) return (float)cnt[s_pos[q]];
    else return Lf;
  };

  // (Several sub-runs per lane-group in flight at once were tried -- 2 and 4, with and without the registers capped for eight
  //  waves per SIMD -- and changed nothing: with every tile resident the kernel runs at the rate the memory system takes random
  //  512-B reads and read-modify-writes, ~5 TB/s of real traffic, not at a latency chain's.)
  if (rsub < rpw) {
    for (int k = gid; k < S; k += groups) {
      const int s = s_start[k], e = s_start[k + 1];
      const uint32_t key = s_key[1 + s];
      if constexpr (PAD) {
        if (key == (uint32_t)tb.num_entries) continue;
      }
      const bool head = (s_key[s] != key) || (s == 0 && at_table_start);
      const bool tail = (s_key[1 + e] != key) || (tile0 + e >= N);
      const int64_t chunk = (tile0 + s) / FFH_EMB_CHUNK;
      const int odd = (s % FFH_EMB_CHUNK) ? 1 : 0;
      const bool single = head && tail;
      if (!single && c0 == 0) s_meta[(int)(chunk - tile0 / FFH_EMB_CHUNK) * 2 + odd] = make_uint2(head ? kMetaFirst : kMetaCont, key);
      float* wrow = weight_row<WT>(tb.weight, key, D);
      const uint64_t rkey = single ? sr_row_key<WT>(op, sk, key) : 0;
      float* prow = partial_t + (chunk * 2 + odd) * D;
      if constexpr (opt_rowwise(R)) {
        if (single) {      // the whole row at once; the sub-run's sum of vector c as the loop below forms it, in order
          apply_row_rowwise<VEC, WT>(op, wrow, st0 + key, D, nvec, lpr, c0, lane, [&](int c, float (&acc)[VEC]) {
            load_grad<VEC>(acc, tb.io + (int64_t)s_pos[s] * tb.ld, c, div_of(s), avg);
            for (int q = s + 1; q < e; q++) {
              float v0[VEC];
              load_grad<VEC>(v0, tb.io + (int64_t)s_pos[q] * tb.ld, c, div_of(q), avg);
#pragma unroll
              for (int v = 0; v < VEC; v++) acc[v] = acc[v] + v0[v];
            }
          }, sk, rkey);
          continue;
        }
      }
      for (int c = c0; c < nvec; c += lpr) {
        float acc[VEC];
        load_grad<VEC>(acc, tb.io + (int64_t)s_pos[s] * tb.ld, c, div_of(s), avg);
        int q = s + 1;
        // four independent row loads in flight, summed in order
        for (; q + 4 <= e; q += 4) {
          float v0[VEC], v1[VEC], v2[VEC], v3[VEC];
          load_grad<VEC>(v0, tb.io + (int64_t)s_pos[q] * tb.ld, c, div_of(q), avg);
          load_grad<VEC>(v1, tb.io + (int64_t)s_pos[q + 1] * tb.ld, c, div_of(q + 1), avg);
          load_grad<VEC>(v2, tb.io + (int64_t)s_pos[q + 2] * tb.ld, c, div_of(q + 2), avg);
          load_grad<VEC>(v3, tb.io + (int64_t)s_pos[q + 3] * tb.ld, c, div_of(q + 3), avg);
#pragma unroll
          for (int v = 0; v < VEC; v++) acc[v] = (((acc[v] + v0[v]) + v1[v]) + v2[v]) + v3[v];
        }
        for (; q < e; q++) {
          float v0[VEC];
          load_grad<VEC>(v0, tb.io + (int64_t)s_pos[q] * tb.ld, c, div_of(q), avg);
#pragma unroll
          for (int v = 0; v < VEC; v++) acc[v] = acc[v] + v0[v];
        }
        if (single) {
          if constexpr (!opt_rowwise(R))      // (a row-wise rule took the row whole, above)
            apply_row<VEC, R, WT>(op, wrow, opt_state(R) ? st0 + (int64_t)key * D : nullptr, R == RowRule::Adam ? st1 + (int64_t)key * D : nullptr, c, acc, tb.num_entries > op.nt_rows, sk, rkey);
        } else {
          xwg_store_row<VEC, AGENT>(prow, c, acc);
        }
      }
    }
  }
  __syncthreads();
  if (tid < metas) {
    const int64_t slot = (tile0 / FFH_EMB_CHUNK) * 2 + tid;
    if (slot < 2 * (int64_t)a.nchunks) xwg_store2<AGENT>(meta_t + slot, s_meta[tid]);
  }
}

// step 3: fold.  A row whose run crosses block boundaries left one partial per block at level k (slot 2b:
// the run enters block b from the left; slot 2b+1: the run starts inside block b and leaves it to the
// right).  One lane-group per starting slot adds the row's consecutive level-k partials left to right,
// stopping at the boundary of the enclosing level-(k+1) block (`ratio` level-k blocks; 0 = no boundary,
// last level).  A run that is now complete is applied to the table; otherwise its level-(k+1) partial
// is written with the same two-slots-per-block convention.  Chains are <= ratio steps long.
// one table; the lane-groups numbered group0, group0+ngroups, ... share the slots [slot_lo, slot_hi).
// `keys` (the table's sorted ids; level-0 input only, ratio > 0): whether a run goes on past the end of its level-(k+1) block is
// read off the sorted list instead of the next block's first slot -- the workgroup that folds one block (the last of the
// block's reduce tiles to finish, see emb_sgd_reduce_kernel) then needs nothing another block's tiles write.
template <int VEC, bool AGENT, RowRule R, class WT>
__device__ __forceinline__ void fold_table_body(const ffh_emb_table& tb, const float* part, const uint2* meta, float* pout_t, uint2* mout_t,
                                                int nin, int ratio, int D, const OptP& op, float* st0, float* st1, const SrKey& sk, int64_t slot_lo, int64_t slot_hi,
                                                int64_t group0, int64_t ngroups, const uint2* keys = nullptr,
                                                const uint2* staged = nullptr, int64_t staged_lo = 0, int staged_n = 0,
                                                const uint32_t* nextkey = nullptr) {
  // `staged`: an LDS copy of meta[staged_lo, staged_lo + staged_n) the caller fetched with one parallel load (the in-kernel folds:
  // a dependent memory round trip per slot and lane-group would otherwise be most of the fold)
  auto slot_meta = [&](int64_t sl) -> uint2 {
    if (sl >= staged_lo && sl < staged_lo + staged_n) return staged[sl - staged_lo];      // (staged_n = 0: nothing staged)
    return xwg_load2<AGENT>(meta + sl);
  };
  const int nvec = D / VEC;
  const int lpr = nvec < 64 ? nvec : 64;
  const int rpw = 64 / lpr;
  const int lane = threadIdx.x & 63;
  const int rsub = lane / lpr;
  const int c0 = lane - rsub * lpr;
  if (rsub >= rpw) return;
  for (int64_t slot = slot_lo + group0; slot < slot_hi; slot += ngroups) {
    const uint2 m = slot_meta(slot);
    if (m.x == kMetaNone) continue;
    const int64_t b = slot >> 1;
    const bool at_block_start = ratio > 0 && (b % ratio == 0) && ((slot & 1) == 0);
    if (!(m.x == kMetaFirst || (m.x == kMetaCont && at_block_start))) continue;   // consumed by the walk that starts left of it
    const int64_t B = ratio > 0 ? b / ratio : 0;
    int64_t bend = ratio > 0 ? (B + 1) * (int64_t)ratio : (int64_t)nin;
    if (bend > nin) bend = nin;
    // length of the walk (same for every column chunk): the lanes of the group look at lpr candidate blocks at once -- one
    // parallel load and a ballot instead of up to `ratio` dependent loads (which were most of this kernel's time on the
    // tables whose rows are hit thousands of times)
    int64_t b2 = b + 1;
    {
      const uint64_t gmask = (lpr == 64 ? ~0ull : ((1ull << lpr) - 1ull)) << (rsub * lpr);
      for (int64_t base = b + 1; base < bend; base += lpr) {
        const int64_t idx = base + c0;
        bool ok = false;
        if (idx < bend) { const uint2 m2 = slot_meta(2 * idx); ok = m2.x == kMetaCont && m2.y == m.y; }
        const uint64_t stop = ~(uint64_t)__ballot(ok) & gmask;          // lanes of this group whose block ends the run (or lies past bend)
        if (stop) { b2 = base + (__ffsll((unsigned long long)stop) - 1 - rsub * lpr); break; }
        b2 = base + lpr;
      }
      if (b2 > bend) b2 = bend;
    }
    bool cont_after = false;
    if (b2 == bend && bend < nin) {
      // the run reached the end of the block: it continues iff the entry behind the block carries the same id (sorted list);
      // equivalently the next block's first slot is a continuation of this id
      if (nextkey) cont_after = __hip_atomic_load(nextkey + B, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == m.y;    // (bucket form: the list in memory is not sorted)
      else if (keys) cont_after = keys[bend * FFH_EMB_CHUNK].x == m.y;
      else { const uint2 m3 = slot_meta(2 * bend); cont_after = (m3.x == kMetaCont && m3.y == m.y); }
    }
    const bool head = m.x == kMetaFirst;
    const bool complete = head && !cont_after;
    const int64_t oslot = 2 * B + (at_block_start ? 0 : 1);
    if (!complete && c0 == 0) xwg_store2<AGENT>(mout_t + oslot, make_uint2(head ? kMetaFirst : kMetaCont, m.y));
    float* wrow = weight_row<WT>(tb.weight, m.y, D);
    const uint64_t rkey = complete ? sr_row_key<WT>(op, sk, m.y) : 0;
    float* orow = pout_t + oslot * D;
    if constexpr (opt_rowwise(R)) {
      if (complete) {      // the whole row at once; the walk's sum of vector c as the loop below forms it, left to right
        apply_row_rowwise<VEC, WT>(op, wrow, st0 + m.y, D, nvec, lpr, c0, lane, [&](int c, float (&acc)[VEC]) {
          xwg_load_row<VEC, AGENT>(acc, part + slot * D, c);
          for (int64_t q = b + 1; q < b2; q++) {
            float v0[VEC];
            xwg_load_row<VEC, AGENT>(v0, part + 2 * q * D, c);
#pragma unroll
            for (int v = 0; v < VEC; v++) acc[v] = acc[v] + v0[v];
          }
        }, sk, rkey);
        continue;
      }
    }
    for (int c = c0; c < nvec; c += lpr) {
      float acc[VEC];
      xwg_load_row<VEC, AGENT>(acc, part + slot * D, c);
      int64_t q = b + 1;
      for (; q + 4 <= b2; q += 4) {   // four partial rows in flight, added in order
        float v0[VEC], v1[VEC], v2[VEC], v3[VEC];
        xwg_load_row<VEC, AGENT>(v0, part + 2 * q * D, c);
        xwg_load_row<VEC, AGENT>(v1, part + 2 * (q + 1) * D, c);
        xwg_load_row<VEC, AGENT>(v2, part + 2 * (q + 2) * D, c);
        xwg_load_row<VEC, AGENT>(v3, part + 2 * (q + 3) * D, c);
#pragma unroll
        for (int v = 0; v < VEC; v++) acc[v] = (((acc[v] + v0[v]) + v1[v]) + v2[v]) + v3[v];
      }
      for (; q < b2; q++) {
        float v0[VEC];
        xwg_load_row<VEC, AGENT>(v0, part + 2 * q * D, c);
#pragma unroll
        for (int v = 0; v < VEC; v++) acc[v] = acc[v] + v0[v];
      }
      if (complete) {
        if constexpr (!opt_rowwise(R))      // (a row-wise rule took the row whole, above)
          apply_row<VEC, R, WT>(op, wrow, opt_state(R) ? st0 + (int64_t)m.y * D : nullptr, R == RowRule::Adam ? st1 + (int64_t)m.y * D : nullptr, c, acc, tb.num_entries > op.nt_rows, sk, rkey);
      } else {
        xwg_store_row<VEC, AGENT>(orow, c, acc);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// bucket form of the fused update (round 5; calls of <= 64 K lookups per table): ONE stable pass on the top digit of the row ids
// (radix_hist_kernel + radix_scatter_kernel with msd set: the list ends up grouped by bucket, in position order inside a bucket),
// and every tile of the apply launch makes the rest of the order for ITSELF in LDS -- three launches instead of seven at the
// per-rank shape of the 8-GPU job, where the sort was six dependent launches of ~7 us with a few kilobytes of work each.
//   * A tile needs the sorted entries [tile0 - 1, tile0 + n] (its own and the row id on either side).  An entry's sorted index
//     is its bucket's start plus its rank inside the bucket, so the tile loads every bucket that overlaps that index range WHOLE
//     (the window: ~tile + two average buckets), sorts the window by row id with the stable LDS radix passes of the small-batch
//     kernel (ids relative to the window's first bucket: two or three passes), and reads its entries off the window at
//     offset (tile0 - 1) - start(first bucket).  The canonical order (FFH_EMB_CHUNK cuts of the SORTED index) is untouched: what the
//     tile adds and where its partial rows go is decided by exactly the same list as before, so the result is bit-identical.
//   * A window larger than kWinMax entries (a hot row: thousands of hits in one bucket) is cut down to exactly the entries wanted:
//     the row id and occurrence number of the entry at a given rank of a bucket are found by counting (msd_select: one pass over
//     the bucket per nine id bits), and one more pass copies the entries between the two bounds in list order (msd_collect).  Cost
//     ~ bucket size per overlapping tile; no fallback launch, no second code path on the host.
//   * The fold of a 1024-block asks whether a run goes on behind the block: the last tile of every block leaves the row id behind
//     it in `nextkey` (the list in memory is no longer sorted).
// ---------------------------------------------------------------------------
constexpr int kWinMax = 1536;                     // entries of a tile's window: tile (<= 1024) + 2 + the two edge buckets
constexpr int kWinE = kWinMax / kRedThreads;      // ... per thread
struct alignas(16) MsdShared {
  uint32_t k[kWinMax], p[kWinMax];                // the window: row id relative to its first bucket, position
  uint32_t off[4][kMaxRadix];
  uint32_t scan[kMaxRadix];
  uint32_t bs[kMaxRadix + 1];                     // the table's bucket starts
  uint32_t wsum[4];
  uint32_t w[3][4];
  uint32_t misc[8];
};

// stable LSD radix sort of the window's `cnt` entries on the low `bitsw` bits of k[]
__device__ __forceinline__ void msd_sort_window(MsdShared& ms, const uint32_t cnt, const int bitsw) {
  if (bitsw <= 0 || cnt <= 1) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int np = (bitsw + kMaxRadixBits - 1) / kMaxRadixBits, rbw = (bitsw + np - 1) / np;
  const int radixw = 1 << rbw;
  const uint32_t mask = (uint32_t)radixw - 1u;
  const int span = (((int)cnt + 3) / 4 + 63) / 64 * 64;       // consecutive entries per wave
  const int ne = span / 64;                                   // <= kWinE
  uint32_t key[kWinE], pos[kWinE];
  bool valid[kWinE];
  auto fetch = [&]() {
#pragma unroll
    for (int e = 0; e < kWinE; e++) {
      const int i = wave * span + e * 64 + lane;
      valid[e] = e < ne && i < (int)cnt;
      key[e] = valid[e] ? ms.k[i] : 0u;
      pos[e] = valid[e] ? ms.p[i] : 0u;
    }
  };
  fetch();
  __syncthreads();
  for (int p = 0; p < np; p++) {
    for (int w2 = 0; w2 < 4; w2++)
      for (int d = threadIdx.x; d < radixw; d += kRedThreads) ms.off[w2][d] = 0;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kWinE; e++)
      if (valid[e]) atomicAdd(&ms.off[wave][(key[e] >> (p * rbw)) & mask], 1u);
    __syncthreads();
    uint32_t all_d[2] = {0, 0};
    const uint32_t before_d[2] = {0, 0};
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int d = threadIdx.x + q * kRedThreads;
      if (d < radixw) all_d[q] = ms.off[0][d] + ms.off[1][d] + ms.off[2][d] + ms.off[3][d];
    }
    sort_scan_offsets<4, 2>(all_d, before_d, radixw, ms.off, ms.scan, ms.wsum);
    sort_rank_and_scatter<kWinE>(key, pos, valid, p * rbw, rbw, mask, ms.off[wave], SortOutLds{ms.k, ms.p}, ne);
    __syncthreads();
    if (p + 1 < np) { fetch(); __syncthreads(); }
  }
}

// The usual window (whole buckets, a few dozen entries each) without a single workgroup barrier: buckets are independent sort
// domains, so every wave takes a run of whole buckets (those that start in its quarter of the window), holds its <= 256 entries in
// registers and runs the stable passes on its own 128-counter table -- seven-bit digits of the id relative to its first bucket, two
// counters per lane for the scan, the ranking of sort_rank_and_scatter.  (A count-the-smaller-ones sort was tried first: n^2 / 256
// 64-bit compares per thread cost more than the three radix passes it replaced.)  False: some wave's share is larger -- the caller
// runs the workgroup-wide passes instead.
constexpr int kWaveE = 4;
struct SortOutLdsBase {
  uint32_t* k; uint32_t* p; uint32_t kb;
  __device__ __forceinline__ void put(uint32_t d, uint32_t key, uint32_t pos) const { k[d] = key + kb; p[d] = pos; }
};
__device__ __forceinline__ bool msd_sort_waves(MsdShared& ms, const uint32_t cnt, const int d_lo, const int d_hi, const int shift, const uint32_t ws) {
  typedef __attribute__((address_space(3))) uint32_t lds_u32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t t_lo = (uint32_t)(((unsigned long long)wave * cnt) >> 2), t_hi = (uint32_t)(((unsigned long long)(wave + 1) * cnt) >> 2);
  int n_lo = 0, n_hi = 0;                        // buckets from d_lo on that start below t_lo / t_hi
  for (int b0 = d_lo; b0 <= d_hi; b0 += 64) {
    const int b = b0 + lane;
    const uint32_t st = b <= d_hi ? ms.bs[b] - ws : 0xFFFFFFFFu;
    n_lo += __popcll(__ballot(st < t_lo));
    n_hi += __popcll(__ballot(st < t_hi));
  }
  if (wave == 3) n_hi = d_hi - d_lo + 1;
  const int fb = d_lo + n_lo, lb = d_lo + n_hi;  // this wave's buckets [fb, lb)
  const uint32_t seg0 = ms.bs[fb] - ws, seg1 = ms.bs[lb] - ws;      // (bs[d_hi + 1] - ws = cnt)
  const uint32_t m = seg1 - seg0;
  if (lane == 0) ms.wsum[wave] = m;
  __syncthreads();
  const bool ok = ms.wsum[0] <= 64u * kWaveE && ms.wsum[1] <= 64u * kWaveE && ms.wsum[2] <= 64u * kWaveE && ms.wsum[3] <= 64u * kWaveE;
  __syncthreads();
  if (!ok) return false;
  if (m > 1) {
    int bitsw = shift;
    for (uint32_t sp = (uint32_t)(lb - fb - 1); sp; sp >>= 1) bitsw++;
    const int np = (bitsw + 6) / 7, rbw = (bitsw + np - 1) / np;
    const uint32_t mask = (1u << rbw) - 1u;
    const uint32_t kb = (uint32_t)(fb - d_lo) << shift;               // ms.k holds ids relative to bucket d_lo
    const int ne = ((int)m + 63) / 64;
    volatile lds_u32* const K = (volatile lds_u32*)(ms.k + seg0);
    volatile lds_u32* const P = (volatile lds_u32*)(ms.p + seg0);
    volatile lds_u32* const H = (volatile lds_u32*)ms.off[wave];
    uint32_t key[kWaveE], pos[kWaveE];
    bool valid[kWaveE];
#pragma unroll
    for (int e = 0; e < kWaveE; e++) {
      const uint32_t i = (uint32_t)(e * 64 + lane);
      valid[e] = e < ne && i < m;
      key[e] = valid[e] ? K[i] - kb : 0u;
      pos[e] = valid[e] ? P[i] : 0u;
    }
    for (int p = 0; p < np; p++) {
      H[lane] = 0u; H[lane + 64] = 0u;
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int e = 0; e < kWaveE; e++)
        if (valid[e]) __hip_atomic_fetch_add((lds_u32*)(H + ((key[e] >> (p * rbw)) & mask)), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      __builtin_amdgcn_wave_barrier();
      const uint32_t c0 = H[2 * lane], c1 = H[2 * lane + 1], cs = c0 + c1;
      uint32_t incl = cs;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t nb = __shfl_up(incl, o);
        if (lane >= o) incl += nb;
      }
      __builtin_amdgcn_wave_barrier();
      H[2 * lane] = incl - cs; H[2 * lane + 1] = incl - cs + c0;
      __builtin_amdgcn_wave_barrier();
      sort_rank_and_scatter<kWaveE>(key, pos, valid, p * rbw, rbw, mask, ms.off[wave], SortOutLdsBase{ms.k + seg0, ms.p + seg0, kb}, ne);
      __builtin_amdgcn_wave_barrier();
      if (p + 1 < np) {
#pragma unroll
        for (int e = 0; e < kWaveE; e++) {
          const uint32_t i = (uint32_t)(e * 64 + lane);
          if (valid[e]) { key[e] = K[i] - kb; pos[e] = P[i]; }
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  return true;
}

// the entry of rank r (by row id, then list order) of the bucket kp[s, e) (every id there has the top digit dbase >> shift): its row id
// and how many entries with that id precede it.  r < e - s.
__device__ __forceinline__ void msd_select(const uint2* __restrict__ kp, const int64_t s, const int64_t e, const uint32_t r, const int shift,
                                           const uint32_t dbase, MsdShared& ms, uint32_t& row, uint32_t& app) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t* h = ms.off[0];
  uint32_t pv = 0, rr = r;
  int pl = 0;
  while (pl < shift) {
    const int dg = (shift - pl) < kMaxRadixBits ? (shift - pl) : kMaxRadixBits;
    const int up = shift - pl, sh2 = up - dg;
    const uint32_t dmask = (1u << dg) - 1u;
    for (int d = tid; d < kMaxRadix; d += kRedThreads) h[d] = 0;
    __syncthreads();
    for (int64_t base = s; base < e; base += kRedThreads * 8) {
      uint32_t kk[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int64_t i = base + u * kRedThreads + tid;
        kk[u] = i < e ? kp[i].x - dbase : 0u;
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int64_t i = base + u * kRedThreads + tid;
        if (i < e && (kk[u] >> up) == pv) atomicAdd(&h[(kk[u] >> sh2) & dmask], 1u);      // (up < 32; ids below the bucket's digit: kk < 2^shift)
      }
    }
    __syncthreads();
    // the digit whose candidates hold rank rr: thread t owns digits 2t, 2t + 1
    const uint32_t c0 = h[2 * tid], c1 = h[2 * tid + 1], cc = c0 + c1;
    uint32_t incl = cc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t nb = __shfl_up(incl, o);
      if (lane >= o) incl += nb;
    }
    if (lane == 63) ms.wsum[wave] = incl;
    __syncthreads();
    uint32_t woff = 0;
    for (int w2 = 0; w2 < wave; w2++) woff += ms.wsum[w2];
    const uint32_t excl = woff + incl - cc;
    if (rr >= excl && rr < excl + cc) {
      const bool second = rr >= excl + c0;
      ms.misc[0] = 2u * tid + (second ? 1u : 0u);
      ms.misc[1] = rr - excl - (second ? c0 : 0u);
    }
    __syncthreads();
    pv = (pv << dg) | ms.misc[0];
    rr = ms.misc[1];
    pl += dg;
    __syncthreads();
  }
  row = dbase + pv;
  app = rr;
}

// appends, in list order, the entries of kp[s, e) from (row0, occurrence app0) on [has_lo] and before (row1, occurrence app1) [has_hi]
// to the window; `count` (uniform) = entries in the window
__device__ __forceinline__ void msd_collect(const uint2* __restrict__ kp, const int64_t s, const int64_t e, const bool has_lo, const uint32_t row0, const uint32_t app0,
                                            const bool has_hi, const uint32_t row1, const uint32_t app1, const uint32_t kbase, MsdShared& ms, uint32_t& count) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long lt = (1ull << lane) - 1ull;
  uint32_t run0 = 0, run1 = 0;
  for (int64_t base = s; base < e; base += 4 * kRedThreads) {
    uint2 v[4];
    bool val[4], m0[4], m1[4];
    uint32_t i0[4], i1[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int64_t i = base + wave * 256 + r * 64 + lane;
      val[r] = i < e;
      v[r] = val[r] ? kp[i] : make_uint2(0u, 0u);
    }
    uint32_t w0 = 0, w1 = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      m0[r] = val[r] && has_lo && v[r].x == row0;
      m1[r] = val[r] && has_hi && v[r].x == row1;
      const unsigned long long b0 = __ballot(m0[r]), b1 = __ballot(m1[r]);
      i0[r] = w0 + __popcll(b0 & lt); i1[r] = w1 + __popcll(b1 & lt);
      w0 += __popcll(b0); w1 += __popcll(b1);
    }
    if (lane == 0) { ms.w[0][wave] = w0; ms.w[1][wave] = w1; }
    __syncthreads();
    uint32_t o0 = run0, o1 = run1, t0 = 0, t1 = 0;
#pragma unroll
    for (int w2 = 0; w2 < 4; w2++) {
      const uint32_t q0 = ms.w[0][w2], q1 = ms.w[1][w2];
      if (w2 < wave) { o0 += q0; o1 += q1; }
      t0 += q0; t1 += q1;
    }
    bool take[4];
    uint32_t tp[4], wt = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const bool ge = !has_lo || v[r].x > row0 || (m0[r] && o0 + i0[r] >= app0);
      const bool ltb = !has_hi || v[r].x < row1 || (m1[r] && o1 + i1[r] < app1);
      take[r] = val[r] && ge && ltb;
      const unsigned long long bt = __ballot(take[r]);
      tp[r] = wt + __popcll(bt & lt);
      wt += __popcll(bt);
    }
    if (lane == 0) ms.w[2][wave] = wt;
    __syncthreads();
    uint32_t ot = count, tt = 0;
#pragma unroll
    for (int w2 = 0; w2 < 4; w2++) {
      const uint32_t q = ms.w[2][w2];
      if (w2 < wave) ot += q;
      tt += q;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const uint32_t dst = ot + tp[r];
      if (take[r] && dst < (uint32_t)kWinMax) { ms.k[dst] = v[r].x - kbase; ms.p[dst] = v[r].y; }
    }
    run0 += t0; run1 += t1; count += tt;
    __syncthreads();
  }
}

// The sorted entries [tile0 - 1, tile0 + n] of table `kp` (grouped by top digit, bucket starts bs_g) for the reduce body: thread t
// gets elements j = t + 256 r (r < 5) of the array { id before the tile, the tile's n ids, id behind it } in okey[r] and the
// position of entry j - 1 in opos[r]; the caller copies them into RedShared (which shares its memory with ms) behind a barrier.
__device__ __forceinline__ void msd_window(const uint2* __restrict__ kp, const uint32_t* __restrict__ bs_g, const int radix, const int shift,
                                           const int64_t N, const int64_t tile0, const int n, MsdShared& ms, uint32_t (&okey)[5], uint32_t (&opos)[5]) {
  const int tid = threadIdx.x, lane = tid & 63;
  const bool have_before = tile0 > 0, have_after = tile0 + n < N;
  const uint32_t a = (uint32_t)(have_before ? tile0 - 1 : tile0), b = (uint32_t)(tile0 + n + (have_after ? 1 : 0));      // sorted indices [a, b)
  for (int d = tid; d <= radix; d += kRedThreads) ms.bs[d] = bs_g[d];
  if (tid < 2) ms.misc[tid] = 0;
  __syncthreads();
  {
    uint32_t ca = 0, cb = 0;
    for (int d = tid; d < radix; d += kRedThreads) {
      const uint32_t v = ms.bs[d];
      ca += v <= a ? 1u : 0u;
      cb += v <= b - 1u ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ca += __shfl_xor(ca, o); cb += __shfl_xor(cb, o); }
    if (lane == 0) { atomicAdd(&ms.misc[0], ca); atomicAdd(&ms.misc[1], cb); }
  }
  __syncthreads();
  const int d_lo = (int)ms.misc[0] - 1, d_hi = (int)ms.misc[1] - 1;           // the buckets holding index a and index b - 1
  const uint32_t ws = ms.bs[d_lo], we = ms.bs[d_hi + 1];
  const uint32_t kbase = (uint32_t)d_lo << shift;
  uint32_t cnt, o;
  __syncthreads();                                                            // (misc is reused below)
  const bool whole_buckets = we - ws <= (uint32_t)kWinMax;
  if (whole_buckets) {
    cnt = we - ws; o = a - ws;
    for (uint32_t i = tid; i < cnt; i += kRedThreads) {
      const uint2 v = kp[ws + i];
      ms.k[i] = v.x - kbase; ms.p[i] = v.y;
    }
  } else {
    // cut the edge buckets down to the ranks wanted
    cnt = 0; o = 0;
    const uint32_t s_lo = ws, e_lo = ms.bs[d_lo + 1], s_hi = ms.bs[d_hi], e_hi = we;
    uint32_t row0 = 0, app0 = 0, row1 = 0, app1 = 0;
    const bool has_lo = a > s_lo, has_hi = b < e_hi;
    if (has_lo) msd_select(kp, s_lo, e_lo, a - s_lo, shift, kbase, ms, row0, app0);
    if (has_hi) msd_select(kp, s_hi, e_hi, b - s_hi, shift, (uint32_t)d_hi << shift, ms, row1, app1);
    if (d_lo == d_hi) {
      msd_collect(kp, s_lo, e_lo, has_lo, row0, app0, has_hi, row1, app1, kbase, ms, cnt);
    } else {
      msd_collect(kp, s_lo, e_lo, has_lo, row0, app0, false, 0u, 0u, kbase, ms, cnt);
      if (s_hi > e_lo) msd_collect(kp, e_lo, s_hi, false, 0u, 0u, false, 0u, 0u, kbase, ms, cnt);
      msd_collect(kp, s_hi, e_hi, false, 0u, 0u, has_hi, row1, app1, kbase, ms, cnt);
    }
  }
  __syncthreads();
  int bitsw = shift;
  for (uint32_t span = (uint32_t)(d_hi - d_lo); span; span >>= 1) bitsw++;
  if (!whole_buckets || !msd_sort_waves(ms, cnt, d_lo, d_hi, shift, ws)) msd_sort_window(ms, cnt, bitsw);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 5; r++) {
    const int j = tid + kRedThreads * r;
    okey[r] = 0xFFFFFFFFu; opos[r] = 0u;
    if (j <= n + 1) {
      const bool real = (j > 0 || have_before) && (j <= n || have_after);
      const uint32_t wi = o + (uint32_t)j - (have_before ? 0u : 1u);
      if (real) { okey[r] = ms.k[wi] + kbase; opos[r] = ms.p[wi]; }
    }
  }
}

// step 2 + 3 in one launch.  The folds (step 3, above) used to be two more launches; now the LAST tile of a 1024-block to finish
// folds that block's 32-block partials (the classic last-arriver reduction: an arrival counter per block, with write-through
// stores / sc1 loads of the few cross-workgroup values in place of fences, see xwg_*), and the last 1024-block of a table to be
// folded folds the table's 1024-block partials.  Who folds is decided by timing, what is added to what is not: the same additions
// in the same order as the separate launches.
// Compiled for 8 waves per SIMD (64 VGPRs; the few spills sit in the fold path): a tile's time is a chain of dependent row round
// trips, so every tile of the launch should be resident at once -- at 74 registers 1,536 of the 26-table shape's 1,664 tiles are,
// and the launch takes 336 instead of 230 us.
// The stateful rules (momentum / weight-decay SGD, Adam, Adagrad on the touched rows): the row rule holds up to three more rows' worth of registers;
// those instantiations are compiled for 4 waves per SIMD instead of spilling.  Plain SGD on bf16 rows (the rounding hash): 6 waves per
// SIMD -- at 8 it spilled 30 VGPRs; 6 and 4 were measured 193 / 192 against 200 us at the Terabyte shape.
// Row-wise Adagrad on bf16 rows in the 16-byte form: 3 -- a row of up to four vectors per lane (gradient and packed weights) stays in registers
// across the sum beside the rounding hash; at 4 (128 VGPRs) it spilled 49 dwords.
// MSD: the bucket form above (the list is grouped by top digit only; six workgroups per CU: the window needs 25 KB of LDS).
template <int VEC, RowRule R, class WT, bool MSD>
constexpr int red_waves_per_simd() {
  if (VEC == 4 && opt_rowwise(R) && is_bf16<WT>()) return 3;
  if (MSD) return opt_plain(R) ? 6 : 4;
  return !opt_plain(R) ? 4 : is_bf16<WT>() ? 6 : 8;
}
struct RedSmem { RedShared sh; uint2 fmeta[kFoldStage]; };
union MsdSmem { RedSmem red; MsdShared ms; };          // the window is dead once the tile's entries sit in registers
template <bool MSD> struct RedSmemOf { typedef RedSmem type; static __device__ __forceinline__ RedSmem& red(RedSmem& s) { return s; } };
template <> struct RedSmemOf<true> { typedef MsdSmem type; static __device__ __forceinline__ RedSmem& red(MsdSmem& s) { return s.red; } };
template <int VEC, RowRule R, class WT, bool MSD, bool LRP>
__global__ __launch_bounds__(kRedThreads, (red_waves_per_simd<VEC, R, WT, MSD>())) void emb_sgd_reduce_kernel(const RedArgs a) {
  ffh_kernel_prio();
  FFH_OPT_OF(LRP, op, a.op);
  __shared__ typename RedSmemOf<MSD>::type smem;
  __shared__ int s_last;
  RedShared& sh = RedSmemOf<MSD>::red(smem).sh;
  uint2* const s_fmeta = RedSmemOf<MSD>::red(smem).fmeta;
  const int tix = blockIdx.y;
  const ffh_emb_table& tb = a.t[tix];
  const uint2* keys = a.kp[a.parity[tix]] + (int64_t)tix * a.N;
  float* p0 = a.partial + (int64_t)tix * 2 * a.nchunks * a.D;
  uint2* m0 = a.meta + (int64_t)tix * 2 * a.nchunks;
  float* const st0 = opt_state(R) ? a.s0[tix] : nullptr;
  float* const st1 = state1_of<R, WT>(a, tix);
  const SrKey sk = sr_key<R, WT>(a, tix);
  bool preloaded = false;
  if constexpr (MSD) {
    const int shift = a.shift_t[tix];
    const int64_t tile0m = (int64_t)blockIdx.x * a.tile;
    const int nm = tile0m >= a.N ? 0 : (int)((a.N - tile0m) < a.tile ? (a.N - tile0m) : a.tile);
    if (shift > 0 && nm > 0) {         // (shift 0: the one pass sorted the table completely)
      uint32_t okey[5], opos[5];
      msd_window(keys, a.bstart + (int64_t)tix * (kMaxRadix + 1), a.radix, shift, a.N, tile0m, nm, smem.ms, okey, opos);
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 5; r++) {
        const int j = (int)threadIdx.x + kRedThreads * r;
        if (j <= nm + 1) {
          sh.key[j] = okey[r];
          if (j >= 1 && j <= nm) sh.pos[j - 1] = a.L == 1 ? opos[r] : opos[r] / (uint32_t)a.L;
        }
      }
      preloaded = true;
    }
  }
  reduce_tile_body<VEC, true, R, WT>(tb, keys, p0, m0, a.N, a.nchunks, a.tile,
                        (int)blockIdx.x, a.L, a.D, a.avg != 0, op, st0, st1, sk, sh, threadIdx.x, preloaded);

  const int nvec = a.D / VEC;
  const int lpr = nvec < 64 ? nvec : 64;
  const int rpw = 64 / lpr;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t group0 = (int64_t)wave * rpw + lane / lpr;
  const int64_t ngroups = (int64_t)(kRedThreads / 64) * rpw;
  uint32_t* arrive = a.arrive + (int64_t)tix * (a.nchunks1 + 1);
  float* p1 = a.partial1 + (int64_t)tix * 2 * a.nchunks1 * a.D;
  uint2* m1 = a.meta1 + (int64_t)tix * 2 * a.nchunks1;
  constexpr int kRatio = FFH_EMB_CHUNK1 / FFH_EMB_CHUNK;

  // this tile's partials and slots are out (written through, completed), then count it in
  const int64_t tile0 = (int64_t)blockIdx.x * a.tile;
  const int64_t B1 = tile0 / FFH_EMB_CHUNK1;
  const int64_t blk_end = (B1 + 1) * FFH_EMB_CHUNK1 < a.N ? (B1 + 1) * FFH_EMB_CHUNK1 : a.N;
  const uint32_t tiles_in_block = (uint32_t)((blk_end - B1 * FFH_EMB_CHUNK1 + a.tile - 1) / a.tile);
  uint32_t* const nextkey = MSD ? a.nextkey + (int64_t)tix * a.nchunks1 : nullptr;
  if constexpr (MSD) {
    // the block's last tile: the row id behind the block, for whoever folds it
    const int64_t tend = tile0 + a.tile < a.N ? tile0 + a.tile : a.N;
    if (threadIdx.x == 0 && tend == blk_end) __hip_atomic_store(nextkey + B1, sh.key[1 + (int)(tend - tile0)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  xwg_stores_done();
  __syncthreads();
  if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(&arrive[B1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tiles_in_block - 1u;
  __syncthreads();
  if (!s_last) return;
  // the slot records the fold walks over, fetched by the whole workgroup at once; nothing to fold (the usual case on the big
  // tables, whose rows are hit once): no walk at all
  auto stage = [&](const uint2* m, int64_t lo, int64_t hi) -> bool {
    const int n = (int)(hi - lo < kFoldStage ? hi - lo : kFoldStage);
    bool any = false;
    for (int i = threadIdx.x; i < n; i += kRedThreads) {
      const uint2 v = xwg_load2<true>(m + lo + i);
      s_fmeta[i] = v;
      any |= v.x != kMetaNone;
    }
    for (int64_t i = lo + kFoldStage + threadIdx.x; i < hi; i += kRedThreads) any |= xwg_load2<true>(m + i).x != kMetaNone;   // (beyond the stage: N > 512 K)
    return __syncthreads_or(any);
  };
  if (a.nchunks1 > 1) {
    const int64_t lo = 2 * B1 * kRatio;
    const int64_t hi = lo + 2 * kRatio < 2 * (int64_t)a.nchunks ? lo + 2 * kRatio : 2 * (int64_t)a.nchunks;
    if (stage(m0, lo, hi))
      fold_table_body<VEC, true, R, WT>(tb, p0, m0, p1, m1, a.nchunks, kRatio, a.D, op, st0, st1, sk, lo, hi, group0, ngroups, MSD ? nullptr : keys, s_fmeta, lo, (int)(hi - lo), nextkey);
    xwg_stores_done();
    __syncthreads();
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(&arrive[a.nchunks1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)a.nchunks1 - 1u;
    __syncthreads();
    if (!s_last) return;
    const int64_t hi1 = 2 * (int64_t)a.nchunks1;
    if (stage(m1, 0, hi1))
      fold_table_body<VEC, true, R, WT>(tb, p1, m1, p1, m1, a.nchunks1, 0, a.D, op, st0, st1, sk, 0, hi1, group0, ngroups, nullptr, s_fmeta, 0, (int)(hi1 < kFoldStage ? hi1 : kFoldStage));
  } else {
    const int64_t hi0 = 2 * (int64_t)a.nchunks;
    if (stage(m0, 0, hi0))
      fold_table_body<VEC, true, R, WT>(tb, p0, m0, p1, m1, a.nchunks, 0, a.D, op, st0, st1, sk, 0, hi0, group0, ngroups, nullptr, s_fmeta, 0, (int)hi0);
  }
}

// ---------------------------------------------------------------------------
// small batches (N = batch*bag <= 2048 per table, e.g. the 2048-sample Criteo-Kaggle step): the whole
// chain -- LDS-resident radix sort, segmented reduce, both folds -- in ONE launch, one workgroup per
// table.  At this size the ten-launch pipeline is pure launch latency (and host issue time); the
// arithmetic and its order are identical (same device bodies), so the result is bit-identical too.
// ---------------------------------------------------------------------------
constexpr int kSmallMax = 2048;

constexpr int kSmallWaves = 8;                        // threads per table = 64 x this: sort ranks kSmallMax / threads entries per thread, reduce = teams of 256
constexpr int kSmallThreads = kSmallWaves * 64;
constexpr int kSmallRedParts = kSmallThreads / kRedThreads;

struct SmallSortShared {
  uint32_t k[kSmallMax], p[kSmallMax];
  uint32_t off[kSmallWaves][kMaxRadix];
  uint32_t scan[kMaxRadix];
  uint32_t wsum[kSmallWaves];
};
union SmallShared {                                    // the sort arrays are dead once the sorted list is in global memory
  SmallSortShared sort;
  RedShared red[kSmallRedParts];
};

template <int VEC, RowRule R, class WT, bool LRP>
__global__ __launch_bounds__(kSmallThreads) void emb_sgd_small_kernel(const SmallArgs a) {
  ffh_kernel_prio();
  FFH_OPT_OF(LRP, op, a.op);
  constexpr int NW = kSmallWaves;
  constexpr int E = kSmallMax / kSmallThreads;         // 2 entries per thread, wave w owns [128 w, 128 w + 128)
  __shared__ SmallShared sm;
  uint32_t* s_k = sm.sort.k;
  uint32_t* s_p = sm.sort.p;
  uint32_t (*s_off)[kMaxRadix] = sm.sort.off;
  const int tix = blockIdx.x;
  const ffh_emb_table tb = a.t[tix];
  float* const st0 = opt_state(R) ? a.s0[tix] : nullptr;
  float* const st1 = state1_of<R, WT>(a, tix);
  const SrKey sk = sr_key<R, WT>(a, tix);
  const int64_t N = a.N;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int radix = 1 << a.rb;
  const uint32_t mask = radix - 1;

  uint32_t key[E], pos[E];
  bool valid[E];
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int i = wave * (kSmallMax / NW) + e * 64 + lane;
    valid[e] = i < N;
    key[e] = valid[e] ? (uint32_t)tb.idx[i] : 0u;
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
  uint2* keys = a.kp + (int64_t)tix * N;
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int i = wave * (kSmallMax / NW) + e * 64 + lane;
    if (valid[e]) keys[i] = make_uint2(key[e], pos[e]);
  }
  uint2* m1 = a.meta1 + (int64_t)tix * 2 * a.nch1;
  for (int i = threadIdx.x; i < 2 * a.nch1; i += kSmallThreads) m1[i] = make_uint2(kMetaNone, 0);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

  // reduce: the 1024 threads act as four 256-thread teams, one tile of a.tile sorted entries each
  float* p0 = a.partial + (int64_t)tix * 2 * a.nch0 * a.D;
  uint2* m0 = a.meta + (int64_t)tix * 2 * a.nch0;
  const int team = threadIdx.x / kRedThreads, ttid = threadIdx.x % kRedThreads;
  const int ntiles = (int)((N + a.tile - 1) / a.tile);
  for (int t0 = 0; t0 < ntiles; t0 += kSmallRedParts) {
    reduce_tile_body<VEC, false, R, WT>(tb, keys, p0, m0, N, a.nch0, a.tile, t0 + team, a.L, a.D, a.avg != 0, op, st0, st1, sk, sm.red[team], ttid);
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
  float* p1 = a.partial1 + (int64_t)tix * 2 * a.nch1 * a.D;
  if (a.nch1 > 1) {
    fold_table_body<VEC, false, R, WT>(tb, p0, m0, p1, m1, a.nch0, FFH_EMB_CHUNK1 / FFH_EMB_CHUNK, a.D, op, st0, st1, sk, 0, 2 * (int64_t)a.nch0, group0, ngroups);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    fold_table_body<VEC, false, R, WT>(tb, p1, m1, p1, m1, a.nch1, 0, a.D, op, st0, st1, sk, 0, 2 * (int64_t)a.nch1, group0, ngroups);
  } else {
    fold_table_body<VEC, false, R, WT>(tb, p0, m0, p1, m1, a.nch0, 0, a.D, op, st0, st1, sk, 0, 2 * (int64_t)a.nch0, group0, ngroups);
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// The launch table.  An update launch is picked by (rule, weight type, VEC, LRP[, MSD]).  The weight type picks the translation unit that
// holds the kernels (emb_update_launch_f32 / _bf16: emb_update_launch below for its WT); the rest is an index into that unit's tables,
// which hold every combination exactly once: 20 small-batch and 40 sorted-route kernels per weight type.
// ---------------------------------------------------------------------------
struct UpdateLaunch {
  RowRule rule; bool v4, lrp, msd;      // (msd: the sorted routes only)
  const SmallArgs* small;               // the small-batch route's arguments, or null: ...
  const RedArgs* red;                   // ... a sorted route's
  dim3 grid;
  hipStream_t stream;
};
typedef void (*UpdateFn)(const UpdateLaunch&);
constexpr int kUpdateEntries = 5 * 2 * 2;      // rule x VEC x LRP
constexpr int update_index(RowRule r, bool v4, bool lrp) { return ((int)r * 2 + (v4 ? 1 : 0)) * 2 + (lrp ? 1 : 0); }
static_assert(update_index(RowRule::RowwiseAdagrad, true, true) == kUpdateEntries - 1, "the table holds every rule");
namespace {

template <class WT, int I> void launch_small(const UpdateLaunch& u) {
  hipLaunchKernelGGL((emb_sgd_small_kernel<(I >> 1 & 1) ? 4 : 1, (RowRule)(I >> 2), WT, (I & 1) != 0>), u.grid, dim3(kSmallThreads), 0, u.stream, *u.small);
}
template <class WT, int I, bool MSD> void launch_reduce(const UpdateLaunch& u) {
  hipLaunchKernelGGL((emb_sgd_reduce_kernel<(I >> 1 & 1) ? 4 : 1, (RowRule)(I >> 2), WT, MSD, (I & 1) != 0>), u.grid, dim3(kRedThreads), 0, u.stream, *u.red);
}
// false: the tables hold no such entry
template <class WT, int... I>
bool emb_update_launch(const UpdateLaunch& u, std::integer_sequence<int, I...>) {
  static constexpr UpdateFn kSmall[] = {launch_small<WT, I>...};
  static constexpr UpdateFn kReduce[2][sizeof...(I)] = {{launch_reduce<WT, I, false>...}, {launch_reduce<WT, I, true>...}};
  const int i = update_index(u.rule, u.v4, u.lrp);
  if (i < 0 || i >= (int)sizeof...(I) || (u.small != nullptr) == (u.red != nullptr)) return false;
  if (u.small) kSmall[i](u); else kReduce[u.msd ? 1 : 0][i](u);
  return true;
}
}  // namespace

__attribute__((visibility("hidden"))) bool emb_update_launch_f32(const UpdateLaunch& u);      // embedding_update_f32.hip
__attribute__((visibility("hidden"))) bool emb_update_launch_bf16(const UpdateLaunch& u);     // embedding_update_bf16.hip

}  // namespace ffh_emb
