#pragma once
#include "ffh_common.h"

namespace ffh_emb {

// ---------------------------------------------------------------------------
// fused backward + SGD, step 1: per-table stable LSD radix sort of (row id, position)
// ---------------------------------------------------------------------------
constexpr int kSortThreads = 256;
constexpr int kSortMaxPerThread = 8;                        // tile = 256 * E entries, E in {1,2,4,8} chosen per call
constexpr int kMaxRadixBits = 9;
constexpr int kMaxRadix = 1 << kMaxRadixBits;

struct SortArgs {
  const int64_t* idx[FFH_MAX_TABLES];   // pass 0 source
  const uint2* src;                     // [nt][N] {row id, position}: ONE 8-byte element per entry -- a pass scatters one store per
  uint2*    dst;                        //   entry instead of two 4-byte ones into two arrays (the scattered stores are most of a pass)
  uint32_t* hist;                       // [nt][nblk][radix]
  int64_t   N;                          // entries per table (batch * L)
  int       nblk;
  int       shift;
  int       bits;
  int       pass;
  uint8_t   npass[FFH_MAX_TABLES];      // digits table t really has; later passes would be the identity and are skipped
  uint32_t* clear[2];                   // [nt][nclear[i]] dwords the pass-0 histogram kernel zeroes for the apply phase
  int       nclear[2];                  //   (level-1 meta slots, arrival counters)
  // bucket form (one stable pass on every table's TOP digit, the rest of the order made inside the apply launch, see msd_window):
  int       msd;                        // != 0: the digit of table t sits at shift_t[t] (0: its ids fit the digit -- the pass sorts it completely)
  uint8_t   shift_t[FFH_MAX_TABLES];
  uint32_t* bstart;                     // [nt][kMaxRadix + 1]: first sorted index of every bucket, [radix] = N (written by tile 0 of the scatter)
};

namespace {

template <bool FIRST>
__device__ __forceinline__ uint32_t sort_load_key(const SortArgs& a, int t, int64_t i) {
  if (FIRST) return (uint32_t)a.idx[t][i];
  return a.src[(int64_t)t * a.N + i].x;
}

// histogram of the current digit per 2048-entry tile (LDS-staged bucketing)
template <bool FIRST, int E>
__global__ __launch_bounds__(kSortThreads) void radix_hist_kernel(const SortArgs a) {
  ffh_kernel_prio();
  constexpr int kSortTile = kSortThreads * E;
  constexpr int kSortPerThread = E;
  __shared__ uint32_t s_hist[kMaxRadix];
  const int t = blockIdx.y, blk = blockIdx.x;
  if (FIRST) {     // every table has a pass 0: the apply phase finds its level-1 slots empty and its arrival counters at zero
#pragma unroll
    for (int r = 0; r < 2; r++) {
      uint32_t* z = a.clear[r] + (int64_t)t * a.nclear[r];
      for (int i = blk * kSortThreads + threadIdx.x; i < a.nclear[r]; i += gridDim.x * kSortThreads) z[i] = 0u;
    }
  }
  if (a.pass >= a.npass[t]) return;
  const int radix = 1 << a.bits;
  const uint32_t mask = radix - 1;
  const int shift = (FIRST && a.msd) ? (int)a.shift_t[t] : a.shift;
  for (int d = threadIdx.x; d < radix; d += kSortThreads) s_hist[d] = 0;
  __syncthreads();
  const int64_t tile0 = (int64_t)blk * kSortTile;
#pragma unroll
  for (int e = 0; e < kSortPerThread; e++) {
    const int64_t i = tile0 + e * kSortThreads + threadIdx.x;
    if (i < a.N) atomicAdd(&s_hist[(sort_load_key<FIRST>(a, t, i) >> shift) & mask], 1u);
  }
  __syncthreads();
  uint32_t* out = a.hist + ((int64_t)t * a.nblk + blk) * radix;
  for (int d = threadIdx.x; d < radix; d += kSortThreads) out[d] = s_hist[d];
}

// exclusive scan of the per-digit totals over digits (digit d = threadIdx.x + q*256) plus `before_d`, then the
// per-wave starting offsets: s_off[w][d] (in: count of digit d in wave w's entries) becomes the first
// destination of wave w's entries with digit d.
// NW = waves of the workgroup (4 in the tiled sort kernels, 16 in the small-batch kernel); a thread owns the digits
// threadIdx.x + q * 64 NW, q < QN = ceil(kMaxRadix / (64 NW))
template <int NW, int QN>
__device__ __forceinline__ void sort_scan_offsets(const uint32_t (&all_d)[QN], const uint32_t (&before_d)[QN], int radix,
                                                  uint32_t (*s_off)[kMaxRadix], uint32_t* s_scan, uint32_t* s_wsum) {
  constexpr int NT = NW * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
#pragma unroll
  for (int q = 0; q < QN; q++) {
    if (q * NT >= radix) break;
    uint32_t v = all_d[q];
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t n = __shfl_up(incl, o);
      if (lane >= o) incl += n;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    uint32_t woff = 0, total = 0;
#pragma unroll
    for (int w2 = 0; w2 < NW; w2++) {
      const uint32_t t = s_wsum[w2];
      if (w2 < wave) woff += t;
      total += t;
    }
    const int d = threadIdx.x + q * NT;
    if (d < radix) s_scan[d] = carry + woff + incl - v + before_d[q];
    carry += total;
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < QN; q++) {
    const int d = threadIdx.x + q * NT;
    if (d < radix) {
      uint32_t run = s_scan[d];
#pragma unroll
      for (int w2 = 0; w2 < NW; w2++) {
        const uint32_t cnt = s_off[w2][d];
        s_off[w2][d] = run;
        run += cnt;
      }
    }
  }
  __syncthreads();
}

// stable ranking of a wave's E x 64 entries, 64 at a time: the lanes holding the same digit find each other with
// `bits` ballots (a match-any), the rank inside the group is a popcount of the lower lanes, and the group's
// lowest lane advances the wave's running offset in LDS.  `out.put(dest, key, pos)` stores an entry (SortOutGlobal / SortOutLds).
struct SortOutGlobal { uint2* kp; __device__ __forceinline__ void put(uint32_t d, uint32_t k, uint32_t p) const { kp[d] = make_uint2(k, p); } };
struct SortOutLds { uint32_t* k; uint32_t* p; __device__ __forceinline__ void put(uint32_t d, uint32_t key, uint32_t pos) const { k[d] = key; p[d] = pos; } };
template <int E, class Out>
__device__ __forceinline__ void sort_rank_and_scatter(const uint32_t (&key)[E], const uint32_t (&pos)[E], const bool (&valid)[E],
                                                      int shift, int bits, uint32_t mask, uint32_t* wave_off, const Out out, const int ne = E) {
  const int lane = threadIdx.x & 63;
  // (an LDS-typed pointer: as a generic one the volatile accesses below stayed flat instructions -- and, in the bucket form's window
  //  sort, tripped a code-generation error of this compiler on the flat null check)
  typedef __attribute__((address_space(3))) uint32_t lds_u32;
  volatile lds_u32* my_off = (volatile lds_u32*)wave_off;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
#pragma unroll
  for (int e = 0; e < E; e++) {
    if (e >= ne) break;                  // (uniform: rounds past the caller's live ones hold no entry)
    const uint32_t d = (key[e] >> shift) & mask;
    unsigned long long peers = __ballot(valid[e]);
    // (unrolled over the largest digit with a uniform exit: as a loop with a run-time trip count the compiler kept `peers` under an
    //  exec-mask loop, ~13 instructions per bit; straight-line it is a compare, two selects and two ands)
#pragma unroll
    for (int bit = 0; bit < kMaxRadixBits; bit++) {
      if (bit < bits) {
        const bool one = (d >> bit) & 1u;
        const unsigned long long bal = __ballot(one);
        peers &= one ? bal : ~bal;
      }
    }
    if (valid[e]) {
      const uint32_t base = my_off[d];
      const uint32_t rank = __popcll(peers & lt_mask);
      const uint32_t dest = base + rank;
      out.put(dest, key[e], pos[e]);
      if (rank == 0) my_off[d] = base + __popcll(peers);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// stable scatter.  Each wave owns 512 consecutive entries of the tile and ranks them 64 at a
// time: the lanes holding the same digit find each other with `bits` ballots (a match-any),
// the rank inside the group is a popcount of the lower lanes, and the group's lowest lane
// advances the wave's running offset in LDS.
template <bool FIRST, int E>
__global__ __launch_bounds__(kSortThreads) void radix_scatter_kernel(const SortArgs a) {
  ffh_kernel_prio();
  constexpr int kSortTile = kSortThreads * E;
  constexpr int kSortPerThread = E;
  if (a.pass >= a.npass[blockIdx.y]) return;
  __shared__ uint32_t s_off[4][kMaxRadix];
  __shared__ uint32_t s_scan[kMaxRadix];
  __shared__ uint32_t s_wsum[4];
  const int t = blockIdx.y, blk = blockIdx.x;
  const int radix = 1 << a.bits;
  const uint32_t mask = radix - 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile0 = (int64_t)blk * kSortTile;
  const int shift = (FIRST && a.msd) ? (int)a.shift_t[t] : a.shift;

  for (int d = threadIdx.x; d < 4 * kMaxRadix; d += kSortThreads) (&s_off[0][0])[d] = 0;
  __syncthreads();

  uint32_t key[kSortPerThread], pos[kSortPerThread];
  bool valid[kSortPerThread];
#pragma unroll
  for (int e = 0; e < kSortPerThread; e++) {
    const int64_t i = tile0 + wave * (kSortTile / 4) + e * 64 + lane;
    valid[e] = i < a.N;
    if (FIRST) {
      key[e] = valid[e] ? (uint32_t)a.idx[t][i] : 0u;
      pos[e] = (uint32_t)i;
    } else {
      const uint2 kp = valid[e] ? a.src[(int64_t)t * a.N + i] : make_uint2(0u, 0u);
      key[e] = kp.x; pos[e] = kp.y;
    }
    if (valid[e]) atomicAdd(&s_off[wave][(key[e] >> shift) & mask], 1u);
  }
  __syncthreads();

  // global base of every digit for this tile: digits below (all tiles) + same digit, earlier tiles.
  // The column walk over the [tiles][radix] matrix is unrolled so that 8 L2 loads are in flight.
  const uint32_t* hist_t = a.hist + (int64_t)t * a.nblk * radix;
  uint32_t all_d[2] = {0, 0}, before_d[2] = {0, 0};
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const int d = threadIdx.x + q * kSortThreads;
    if (d < radix) {
      uint32_t all = 0, before = 0;
      int b2 = 0;
      for (; b2 + 8 <= a.nblk; b2 += 8) {
        uint32_t h[8];
#pragma unroll
        for (int u = 0; u < 8; u++) h[u] = hist_t[(int64_t)(b2 + u) * radix + d];
#pragma unroll
        for (int u = 0; u < 8; u++) { all += h[u]; before += (b2 + u < blk) ? h[u] : 0u; }
      }
      for (; b2 < a.nblk; b2++) {
        const uint32_t h = hist_t[(int64_t)b2 * radix + d];
        all += h;
        before += (b2 < blk) ? h : 0u;
      }
      all_d[q] = all; before_d[q] = before;
    }
  }
  sort_scan_offsets<4, 2>(all_d, before_d, radix, s_off, s_scan, s_wsum);
  if (FIRST && a.msd && blk == 0) {      // tile 0 has nothing before it: its scan is the table's bucket starts
    uint32_t* bs = a.bstart + (int64_t)t * (kMaxRadix + 1);
    for (int d = threadIdx.x; d < radix; d += kSortThreads) bs[d] = s_scan[d];
    if (threadIdx.x == 0) bs[radix] = (uint32_t)a.N;
  }
  sort_rank_and_scatter<kSortPerThread>(key, pos, valid, shift, a.bits, mask, s_off[wave], SortOutGlobal{a.dst + (int64_t)t * a.N});
}

}  // namespace

}  // namespace ffh_emb
