// fold_sum.hip -- ffh_fold_segment_sum for wide rows (include/ff_hip_fold.h): G_t[r] = the sum of dy[b] over the hits of row r, in the canonical order
// of include/ff_hip.h, without arrival counters, write-through stores or last-arriver folds.
//
// The fused table update's reduce kernel (emb_reduce.h) is shaped for rows of 128 floats; the rows here are the layer's out_dim (1024 floats in the
// flagship model) and the tables have few rows, so nearly every run of the sorted list is long.  Two launches behind the complete LSD sort
// (embedding.hip, emb_sort_full):
//
//   fold_sum_block_kernel  one workgroup per (table, 1024-block of the sorted list, slice of kFsSlice columns); lane l of every wave owns the 16 bytes
//                          at column 4 l of the slice.  The four waves take the block's 32-blocks in turn: 16 dy row pieces are requested, added in
//                          list order, one fp32 chain per run, then the next 16.  A run that neither enters its 32-block from the left nor leaves it to
//                          the right is complete at the 1024-block level; the at most two open partials of a 32-block (slot 0: enters, slot 1: leaves
//                          only) go to the level-0 slots of the workspace and are read back by the SAME workgroup behind its barrier (64 KB of LDS for
//                          them would not fit beside a persistent GEMM's workgroup): every chain of open partials -- slot 1 of the 32-block where the
//                          row starts, then slot 0 of each following one -- is added left to right by one wave.  A row's 1024-block sum goes to G when
//                          the row lies inside the block, and to the block's two level-1 slots (slot 0: the row enters from the block before, slot 1:
//                          it only leaves) when it does not.
//   fold_sum_join_kernel   one wave per (table, slice) walks the 1024-blocks in order and adds every open row's level-1 slots left to right.
//
// Nothing is read inside a launch that another workgroup of that launch wrote; all stores are plain vector stores; no atomics.  Rows not hit are
// zeroed by the block kernel: the gap between two consecutive ids of the sorted list by the wave that holds the second, the rows in front of the
// first id and behind the last by the waves that hold those -- no memset of G (80 MB at the flagship shape, of which under 2 % stay zero).
#include "fold_sum.h"

#include "../../include/ff_hip_fold.h"

#include <utility>

using namespace ffh_emb;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kFsSlice = 256;                 // columns per workgroup: 64 lanes x 16 bytes
constexpr int kFsBlock = FFH_EMB_CHUNK1;      // 1024 sorted entries per workgroup
constexpr int kFsChunk = FFH_EMB_CHUNK;       // 32
constexpr int kFsWaves = 4;
static_assert(kFsChunk == 32, "a 32-block's entries are held by lanes 0..31 of a wave, its two neighbours by lanes 32 and 33");

struct FoldSumTable { const uint2* kp; const float* dy; int64_t ld; float* g; int64_t rows; };
struct FoldSumArgs {
  FoldSumTable t[FFH_MAX_TABLES];
  float*  partial0;      // [nt][nchunks][2][width]: the open partials of the 32-blocks, written and read back by the same workgroup
  float*  partial;       // [nt][nblk1][2][width]: the open partials of the 1024-blocks, block kernel -> join kernel
  int64_t N, nchunks;
  int L, width, nblk1, nslices;
};
static_assert(sizeof(FoldSumArgs) <= 4096, "kernel arguments");

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

template <int... I, class F>
__device__ __forceinline__ void fs_static_for_impl(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N_, class F>
__device__ __forceinline__ void fs_static_for(F&& f) { fs_static_for_impl(std::make_integer_sequence<int, N_>{}, static_cast<F&&>(f)); }

// quarter Q (8 entries) of a 32-block whose lanes 0..31 hold the dy row numbers `brow` and which has n entries: into v[8 (Q & 1) ...]
template <int Q>
__device__ __forceinline__ void fs_issue(f32x4 (&v)[16], const float* dyc, int64_t ld, uint32_t brow, int n) {
#pragma unroll
  for (int u = 0; u < 8; u++)
    if (8 * Q + u < n) v[8 * (Q & 1) + u] = *reinterpret_cast<const f32x4*>(dyc + (int64_t)__builtin_amdgcn_readlane(brow, 8 * Q + u) * ld);
}

__global__ __launch_bounds__(256) void fold_sum_block_kernel(const FoldSumArgs a) {
  __shared__ uint32_t s_key[kFsBlock];
  ffh_kernel_prio();
  const int lane = threadIdx.x & 63;
  const int wave = (int)uni(threadIdx.x >> 6);
  const int t = blockIdx.y;
  const int slice = (int)(blockIdx.x % (unsigned)a.nslices), blk = (int)(blockIdx.x / (unsigned)a.nslices);
  const FoldSumTable T = a.t[t];
  const int64_t N = a.N, base = (int64_t)blk * kFsBlock;
  const int cnt = (int)(N - base < kFsBlock ? N - base : kFsBlock);      // >= 1
  const int nb32 = (cnt + kFsChunk - 1) / kFsChunk;
  const int col = slice * kFsSlice + 4 * lane;
  const float* const dyc = T.dy + col;
  float* const gc = T.g + col;
  float* const pc = a.partial + ((int64_t)t * a.nblk1 + blk) * 2 * a.width + col;
  float* const p0 = a.partial0 + ((int64_t)t * a.nchunks + base / kFsChunk) * 2 * a.width + col;      // slot s of 32-block B at + (2 B + s) width
  const int L = a.L;

  // the row continues from the block before / into the block behind (the block's first and last row)
  const bool cont_prev = blk > 0 && T.kp[base - 1].x == T.kp[base].x;
  const bool cont_next = base + cnt < N && T.kp[base + cnt].x == T.kp[base + cnt - 1].x;

  // lanes 0..31: the entries of 32-block B; lane 32: the entry in front of it; lane 33: the entry behind it
  auto fetch = [&](int B, uint2& kp, bool& ok) {
    const int64_t e = base + (int64_t)B * kFsChunk + (lane < 32 ? lane : lane == 32 ? -1 : kFsChunk);
    ok = lane < 34 && B < nb32 && e >= 0 && e < N;
    kp = ok ? T.kp[e] : make_uint2(0u, 0u);
  };
  auto count_of = [&](int B) { return B >= nb32 ? 0 : cnt - B * kFsChunk < kFsChunk ? cnt - B * kFsChunk : kFsChunk; };
  auto dy_row = [&](uint32_t pos) { return L == 1 ? pos : pos / (uint32_t)L; };

  // The wave's 32-blocks as one stream of halves of 16 row pieces: 16 loads of 16 bytes per lane are requested, then added in list order, then the next
  // half -- of this 32-block or of the wave's next one, whose entries were fetched one 32-block ahead -- is requested.  (The compiler waits for ALL
  // outstanding loads at the first add behind a uniform branch, so a second half in flight behind the first would only be waited for as well: what
  // hides the latency is the number of waves, and 16 pieces keep the kernel under 100 VGPRs, which is what fits beside a persistent GEMM's wave.)
  uint2 kp_cur, kp_nxt;
  bool ok_cur, ok_nxt;
  fetch(wave, kp_cur, ok_cur);
  fetch(wave + kFsWaves, kp_nxt, ok_nxt);
  f32x4 v[16];
  fs_issue<0>(v, dyc, T.ld, dy_row(kp_cur.y), count_of(wave));
  fs_issue<1>(v, dyc, T.ld, dy_row(kp_cur.y), count_of(wave));

  for (int B = wave; B < nb32; B += kFsWaves) {
    const unsigned long long okm = __ballot(ok_cur);
    const uint32_t key = kp_cur.x, brow = dy_row(kp_cur.y);
    const int n = count_of(B);      // 1 .. 32
    if (lane < n) s_key[B * kFsChunk + lane] = key;
    const uint32_t k_first = __builtin_amdgcn_readlane(key, 0), k_last = __builtin_amdgcn_readlane(key, n - 1);
    const bool prev_same = ((okm >> 32) & 1) && (uint32_t)__builtin_amdgcn_readlane(key, 32) == k_first;
    const bool next_same = ((okm >> 33) & 1) && (uint32_t)__builtin_amdgcn_readlane(key, 33) == k_last;
    const bool in_prev = B > 0, in_next = B < nb32 - 1;

    // the run of `row` is over: where its sum goes
    auto close = [&](uint32_t row, const f32x4 acc, bool at_start, bool at_end) {
      const bool from_left = at_start && prev_same, to_right = at_end && next_same;
      float* dst;
      if (from_left && in_prev) dst = p0 + (int64_t)(2 * B) * a.width;
      else if (to_right && in_next) dst = p0 + (int64_t)(2 * B + 1) * a.width;
      else dst = from_left ? pc : to_right ? pc + a.width : gc + (int64_t)row * a.width;
      *reinterpret_cast<f32x4*>(dst) = acc;
    };
    // rows nobody hits: the gap in front of a run belongs to whoever holds the run's first entry, the rows behind the list's last entry to its holder
    auto zero_rows = [&](int64_t lo, int64_t hi) {
      for (int64_t r = lo; r < hi; r++) *reinterpret_cast<f32x4*>(gc + r * a.width) = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    if (!prev_same) zero_rows(((okm >> 32) & 1) ? (int64_t)(uint32_t)__builtin_amdgcn_readlane(key, 32) + 1 : 0, k_first);
    if (base + (int64_t)B * kFsChunk + n == N) zero_rows((int64_t)k_last + 1, T.rows);
    f32x4 acc = v[0];
    uint32_t row = k_first;
    bool at_start = true;
    fs_static_for<kFsChunk>([&](auto jc) {      // (straight-line code: v[] has to stay in registers)
      constexpr int j = jc + 1;
      if constexpr (j == 16) { fs_issue<2>(v, dyc, T.ld, brow, n); fs_issue<3>(v, dyc, T.ld, brow, n); }      // (entries 0..15 have been added)
      if constexpr (j < kFsChunk) {
        if (j < n) {
          const uint32_t kj = __builtin_amdgcn_readlane(key, j);
          if (kj != row) {
            close(row, acc, at_start, false);
            zero_rows((int64_t)row + 1, kj);
            acc = v[j & 15]; row = kj; at_start = false;
          } else {
            acc += v[j & 15];
          }
        }
      }
      if constexpr (j == 32) { fs_issue<0>(v, dyc, T.ld, dy_row(kp_nxt.y), count_of(B + kFsWaves)); fs_issue<1>(v, dyc, T.ld, dy_row(kp_nxt.y), count_of(B + kFsWaves)); }
    });
    close(row, acc, at_start, true);
    kp_cur = kp_nxt; ok_cur = ok_nxt;
    fetch(B + 2 * kFsWaves, kp_nxt, ok_nxt);
  }
  // the open partials of the 32-blocks were written by this workgroup's own waves: workgroup-scope release / acquire around the barrier
  __syncthreads();

  // chains of open 32-block partials: slot 1 of the 32-block where the row starts, then slot 0 of every following one while the row goes on
  auto last_of = [&](int B) { const int e = B * kFsChunk + kFsChunk - 1; return uni(s_key[e < cnt ? e : cnt - 1]); };
  for (int B = wave; B < nb32 - 1; B += kFsWaves) {
    const uint32_t first = uni(s_key[B * kFsChunk]), row = last_of(B);
    if (row != uni(s_key[(B + 1) * kFsChunk])) continue;                        // nothing leaves to the right
    if (B > 0 && first == row && uni(s_key[B * kFsChunk - 1]) == row) continue;    // passes through: part of a chain that started further left
    int B2 = B + 1;
    while (B2 < nb32 - 1 && last_of(B2) == row && uni(s_key[(B2 + 1) * kFsChunk]) == row) B2++;      // the chain ends in 32-block B2
    f32x4 acc = *reinterpret_cast<const f32x4*>(p0 + (int64_t)(2 * B + 1) * a.width);
    for (int b0 = B + 1; b0 <= B2; b0 += 8) {      // eight partials in flight, added in order
      f32x4 p[8];
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (b0 + u <= B2) p[u] = *reinterpret_cast<const f32x4*>(p0 + (int64_t)(2 * (b0 + u)) * a.width);
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (b0 + u <= B2) acc += p[u];
    }
    const bool from_left = cont_prev && uni(s_key[0]) == row, to_right = cont_next && uni(s_key[cnt - 1]) == row;
    float* dst = from_left ? pc : to_right ? pc + a.width : gc + (int64_t)row * a.width;
    *reinterpret_cast<f32x4*>(dst) = acc;
  }
}

// the rows that are open at 1024-block boundaries: slot 1 of the block where the row starts, then slot 0 of every following block, left to right
__global__ __launch_bounds__(64) void fold_sum_join_kernel(const FoldSumArgs a) {
  ffh_kernel_prio();
  const int lane = threadIdx.x;
  const int t = blockIdx.y;
  const FoldSumTable T = a.t[t];
  const int64_t N = a.N;
  const int col = (int)blockIdx.x * kFsSlice + 4 * lane;
  const float* const part = a.partial + (int64_t)t * a.nblk1 * 2 * a.width + col;
  float* const gc = T.g + col;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < a.nblk1; k0 += 4) {
    // lane 4 i + j: of block k0 + i, the entry in front (j = 0), the first (1), the last (2), the entry behind (3)
    uint32_t key = 0;
    bool ok = false;
    {
      const int k = k0 + (lane >> 2), j = lane & 3;
      if (lane < 16 && k < a.nblk1) {
        const int64_t b0 = (int64_t)k * kFsBlock, b1 = b0 + kFsBlock < N ? b0 + kFsBlock : N;
        const int64_t e = j == 0 ? b0 - 1 : j == 1 ? b0 : j == 2 ? b1 - 1 : b1;
        ok = e >= 0 && e < N;
        if (ok) key = T.kp[e].x;
      }
    }
    const unsigned long long okm = __ballot(ok);
    f32x4 vl[4], vr[4];
    uint32_t first[4];
    bool open_l[4], open_r[4], through[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int k = k0 + i;
      open_l[i] = open_r[i] = through[i] = false;
      first[i] = 0;
      if (k < a.nblk1) {
        first[i] = __builtin_amdgcn_readlane(key, 4 * i + 1);
        const uint32_t last = __builtin_amdgcn_readlane(key, 4 * i + 2);
        open_l[i] = ((okm >> (4 * i)) & 1) && (uint32_t)__builtin_amdgcn_readlane(key, 4 * i) == first[i];
        open_r[i] = ((okm >> (4 * i + 3)) & 1) && (uint32_t)__builtin_amdgcn_readlane(key, 4 * i + 3) == last;
        through[i] = open_l[i] && open_r[i] && first[i] == last;
        if (open_l[i]) vl[i] = *reinterpret_cast<const f32x4*>(part + (int64_t)(2 * k) * a.width);
        if (open_r[i] && !through[i]) vr[i] = *reinterpret_cast<const f32x4*>(part + (int64_t)(2 * k + 1) * a.width);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (open_l[i]) {
        acc += vl[i];
        if (!through[i]) *reinterpret_cast<f32x4*>(gc + (int64_t)first[i] * a.width) = acc;
      }
      if (open_r[i] && !through[i]) acc = vr[i];
    }
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int ffh_emb::fold_sum_wide(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int width, int64_t batch, ffh_stream s) {
  if (width % kFsSlice) return 0;
  for (int t = 0; t < nt; t++)
    if (!al16(tables[t].weight) || !al16(tables[t].io) || tables[t].ld % 4) return 0;
  FullSort srt;
  const int rc = emb_sort_full(c, tables, nt, L, width, batch, s, &srt);
  if (rc != FFH_OK) return rc;
  FoldSumArgs a;
  memset(&a, 0, sizeof a);
  for (int t = 0; t < nt; t++) a.t[t] = FoldSumTable{srt.kp[t], tables[t].io, tables[t].ld, tables[t].weight, tables[t].num_entries};
  a.partial0 = srt.partial0; a.partial = srt.partial1;
  a.N = batch * L; a.L = L; a.width = width;
  a.nblk1 = (int)((a.N + kFsBlock - 1) / kFsBlock);
  a.nchunks = (a.N + kFsChunk - 1) / kFsChunk;
  a.nslices = width / kFsSlice;
  hipLaunchKernelGGL(fold_sum_block_kernel, dim3((unsigned)a.nblk1 * (unsigned)a.nslices, (unsigned)nt), dim3(64 * kFsWaves), 0, as_stream(s), a);
  if (a.nblk1 > 1) hipLaunchKernelGGL(fold_sum_join_kernel, dim3((unsigned)a.nslices, (unsigned)nt), dim3(64), 0, as_stream(s), a);
  FFH_LAUNCH_CHECK(c, "fold_sum_block_kernel / fold_sum_join_kernel");
  snprintf(c->emb_route, sizeof c->emb_route, "fold_sum:wide|slice=%d|lsd:passes=%d", kFsSlice, srt.passes);
  return 1;
}
