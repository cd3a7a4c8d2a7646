// embedding_bag_weights_grad.hip -- include/ffh_bag_weights_grad.h: the gradient of per-sample bag weights, hand-written for gfx950.
//     gw[b][l] = sum_d dY[b][d] * W[idx[b][l]][d]
// A gather-shaped read with a 4-byte result per lookup: the kernel reads the rows the weighted gather reads and keeps none of them.
//
// How the work is split.  A group of G lanes (G the power of two >= min(D / VEC, 64)) owns one bag (table, b) at a time.  It loads the bag's
// gradient row dY[b] into registers ONCE -- lane c holds vectors c, c + G, ... of it, CH of them -- and walks the bag's slots.  Per trip a group
// has U bags x JU slots in flight: 4 x 1 for bags of fewer than kBagLong slots, 2 x 4 for longer ones, the two shapes of emb_fwd_bags_kernel, so
// a lane has 4 (8) row loads of 16 bytes outstanding before it multiplies.  The id of a slot is loaded by every lane of the group from one address
// (one request per group).  Each lane adds its products over ascending d with fmaf, the lanes of the group are combined in a butterfly (level k
// pairs lanes that differ in bit k: two DPP quad permutes, three ds_swizzle steps, one ds_bpermute for the halves of the wave), and lane k mod G of
// the group stores slot k's result.  No LDS, no atomics, nothing kept between trips but dY.
// Workgroups are handed out in proportion to each table's lookups over one flat grid (bag_blocks, emb_gather.h), the grid is capped at kGridCap and
// a table's workgroups walk its batch with a stride.  The geometry of up to FFH_MAX_TABLES tables lies in the kernel arguments (40 bytes a table).
#include "emb_gather.h"
#include "../../include/ffh_bag_weights_grad.h"

#include <type_traits>

namespace {

using namespace ffh_emb;

constexpr int64_t kGridCap = 2048;      // 256 CUs x 8 workgroups
constexpr int kMaxCH = 4;               // vectors of dY a lane keeps: rows of up to 64 * kMaxCH vectors

// The lanes that share a row: G of them, a power of two, so that 64 / G bags lie side by side in a wave and the butterfly is whole.
struct DotLanes {
  int nvec;        // vectors per row
  int G, gsh;      // lanes per bag, and its log2
  int rpw;         // bags per wave-instruction
  int rsub;        // which of the wave's bags lane `lane` works on ...
  int c0;          // ... and its first vector of the row
  __host__ __device__ DotLanes(int D, int vec, int lane = 0) {
    nvec = D / vec;
    const int n = nvec < 64 ? nvec : 64;
    G = 1; gsh = 0;
    while (G < n) { G <<= 1; gsh++; }
    rpw = 64 >> gsh;
    rsub = lane >> gsh;
    c0 = lane & (G - 1);
  }
  // bags a 256-thread workgroup takes per trip with U bags in flight per lane-group
  __host__ __device__ int64_t block_bags(int U) const { return 4LL * rpw * U; }
  __host__ __device__ int chunks() const { return (nvec + 63) / 64; }
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

struct WGradTable {
  const int64_t* idx;      // [batch][L], an id < 0 is a pad
  const void*    weight;   // the table's rows, fp32 or bf16 bits
  const float*   dy;       // [batch] rows dy_ld apart: the table's slice of the embedding output gradient
  float*         gw;       // [batch] rows gw_ld apart, L floats each
  int32_t        dy_ld, gw_ld;
};
struct WGradArgs {
  WGradTable t[FFH_MAX_TABLES];
  uint16_t L[FFH_MAX_TABLES];      // bag size of table i (<= kBagMaxL)
  int64_t batch;
  int64_t nrb[2];        // bag blocks of the batch: [0] short bags (U = 4), [1] long bags (U = 2)
  int     ntables, D;
  int     shift;         // workgroups of table i = clamp((batch * L[i]) >> shift, 1, nrb)
  int     accumulate;
};
static_assert(sizeof(WGradArgs) <= 4096, "kernel arguments");

// v of every lane of a group of 1 << gsh lanes -> the group's sum, in every lane: level k pairs the lanes that differ in bit k.  Both partners
// form the same sum (the add commutes), so the group agrees bit for bit.  Called by whole waves only.
__device__ __forceinline__ float xlane(float v, int k) {
  const int x = __float_as_int(v);
  int y;
  switch (k) {
    case 0: y = __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, true); break;      // quad_perm [1, 0, 3, 2]
    case 1: y = __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, true); break;      // quad_perm [2, 3, 0, 1]
    case 2: y = __builtin_amdgcn_ds_swizzle(x, 0x101F); break;                       // bit mode: and 0x1f, or 0, xor 4
    case 3: y = __builtin_amdgcn_ds_swizzle(x, 0x201F); break;                       // ... xor 8
    case 4: y = __builtin_amdgcn_ds_swizzle(x, 0x401F); break;                       // ... xor 16
    default: y = __builtin_amdgcn_ds_bpermute((int)(((threadIdx.x & 63) ^ 32) << 2), x); break;      // the other half of the wave
  }
  return __int_as_float(y);
}
__device__ __forceinline__ float group_sum(float v, const int gsh) {
#pragma unroll
  for (int k = 0; k < 6; k++)
    if (k < gsh) v = v + xlane(v, k);      // (gsh is uniform over the workgroup)
  return v;
}

// the bags [first, first + step, ...) x bags_per_block of table t; U bags x JU slots in flight per lane-group.  The id of a slot is the same in the
// lanes that share a bag and differs between the bags of a wave, so the row loads and the multiply-adds are predicated (on the id, on the bag
// being inside the batch, on the lane having a vector there), not branched around: every lane reaches every butterfly.
template <int VEC, int CH, int U, int JU, class WT>
__device__ __forceinline__ void wgrad_bags(const WGradArgs& a, const int t, const int64_t first, const int64_t step) {
  using vec_t = typename RowVec<VEC, WT>::type;
  using dy_t = typename RowVec<VEC, float>::type;
  const WGradTable tw = a.t[t];
  const WT* const wt = reinterpret_cast<const WT*>(tw.weight);
  const int D = a.D, L = a.L[t];
  const bool accumulate = a.accumulate != 0;
  const DotLanes g(D, VEC, threadIdx.x & 63);
  const int wave = threadIdx.x >> 6;
  const int64_t bags_per_block = g.block_bags(U);
  bool has[CH];      // this lane's vector h of a row exists
#pragma unroll
  for (int h = 0; h < CH; h++) has[h] = g.c0 + h * g.G < g.nvec;

  for (int64_t base = first * bags_per_block; base < a.batch; base += step * bags_per_block) {
    const int64_t b0 = base + (int64_t)wave * g.rpw * U + g.rsub;
    bool ok[U];
    const int64_t* ids[U];
    float* out[U];
    float dy[U][CH][VEC];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t b = b0 + (int64_t)u * g.rpw;
      ok[u] = b < a.batch;
      ids[u] = tw.idx + b * L;      // (read where ok[u] only)
      out[u] = tw.gw + b * (int64_t)tw.gw_ld;
#pragma unroll
      for (int h = 0; h < CH; h++) {
        dy_t v = {};
        if (ok[u] && has[h]) v = *(reinterpret_cast<const dy_t*>(tw.dy + b * (int64_t)tw.dy_ld) + g.c0 + h * g.G);
#pragma unroll
        for (int e = 0; e < VEC; e++) dy[u][h][e] = reinterpret_cast<const float*>(&v)[e];
      }
    }
    // JN slots of every bag in flight, from slot j
    auto slots = [&](auto jn, const int j) {
      constexpr int JN = decltype(jn)::value;
      int64_t row[U][JN];
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int k = 0; k < JN; k++) row[u][k] = ok[u] ? ids[u][j + k] : -1;
      vec_t val[U][JN][CH];
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int k = 0; k < JN; k++)
#pragma unroll
          for (int h = 0; h < CH; h++)
            if (row[u][k] >= 0 && has[h]) val[u][k][h] = *(reinterpret_cast<const vec_t*>(wt + row[u][k] * (int64_t)D) + g.c0 + h * g.G);
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int k = 0; k < JN; k++) {
          float acc = 0.0f;
#pragma unroll
          for (int h = 0; h < CH; h++)      // ascending d
            if (row[u][k] >= 0 && has[h]) {
#pragma unroll
              for (int e = 0; e < VEC; e++) acc = fmaf(dy[u][h][e], row_elem<VEC, WT>(val[u][k][h], e), acc);
            }
          const float r = group_sum(acc, g.gsh);
          if (ok[u] && g.c0 == (k & (g.G - 1))) {
            float* const p = out[u] + j + k;
            *p = accumulate ? *p + r : r;
          }
        }
    };
    int j = 0;
    if constexpr (JU > 1)
      for (; j + JU <= L; j += JU) slots(std::integral_constant<int, JU>(), j);
    for (; j < L; j++) slots(std::integral_constant<int, 1>(), j);
  }
}

template <int VEC, int CH, class WT>
__global__ __launch_bounds__(256) void bag_wgrad_kernel(const WGradArgs a) {
  ffh_kernel_prio();
  // workgroup -> (table, first bag block of the table): block-uniform, the map of emb_fwd_bags_kernel
  int t = 0;
  int64_t first = blockIdx.x, w = 0;
  for (; t < a.ntables; t++) {
    const int L = a.L[t];
    w = bag_blocks(a.batch, L, a.shift, L >= kBagLong ? a.nrb[1] : a.nrb[0]);
    if (first < w) break;
    first -= w;
  }
  if (t >= a.ntables) return;
  if (a.L[t] >= kBagLong) wgrad_bags<VEC, CH, 2, 4, WT>(a, t, first, w);
  else wgrad_bags<VEC, CH, 4, 1, WT>(a, t, first, w);
}

template <int VEC, class WT>
void wgrad_launch_ch(int ch, unsigned grid, hipStream_t s, const WGradArgs& a) {
  if (ch <= 1) hipLaunchKernelGGL((bag_wgrad_kernel<VEC, 1, WT>), dim3(grid), dim3(256), 0, s, a);
  else if (ch == 2) hipLaunchKernelGGL((bag_wgrad_kernel<VEC, 2, WT>), dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((bag_wgrad_kernel<VEC, kMaxCH, WT>), dim3(grid), dim3(256), 0, s, a);
}

template <class WT>
int wgrad_launch(ffh_ctx* c, const ffh_emb_table* tables, float* const* gw, const int64_t* gw_ld, const int* in_dims, int nt, int D, int64_t batch,
                 int flags, ffh_stream s) {
  if (nt < 0 || nt > FFH_MAX_TABLES) return ffh_fail(c, FFH_ERR_BAD_ARG, "bag_weights_grad: ntables out of range");
  if (nt > 0 && (!tables || !gw || !gw_ld || !in_dims)) return ffh_fail(c, FFH_ERR_BAD_ARG, "bag_weights_grad: null tables, gw, gw_ld or in_dims");
  if (flags & ~FFH_BAG_WGRAD_ACCUMULATE) return ffh_fail(c, FFH_ERR_BAD_ARG, "bag_weights_grad: unknown flag");
  int rc = validate_tables(c, tables, nt, 1, D, batch, FFH_AGGR_MODE_SUM);
  if (rc) return rc;
  constexpr uintptr_t elem = sizeof(WT);
  for (int i = 0; i < nt; i++) {
    if (in_dims[i] < 1) return ffh_fail(c, FFH_ERR_BAD_ARG, "bag_weights_grad: in_dims[i] < 1");
    if (in_dims[i] > kBagMaxL) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "bag_weights_grad: in_dims[i] > FFH_BAGS_MAX_IN_DIM (65535)");
    if (batch > 0 && !gw[i]) return ffh_fail(c, FFH_ERR_BAD_ARG, "bag_weights_grad: gw[i] is null");
    if (gw_ld[i] < in_dims[i]) return ffh_fail(c, FFH_ERR_BAD_ARG, "bag_weights_grad: gw_ld[i] < in_dims[i]");
    if (((uintptr_t)gw[i] & 3) || ((uintptr_t)tables[i].io & 3) || ((uintptr_t)tables[i].idx & 7) || ((uintptr_t)tables[i].weight & (elem - 1)))
      return ffh_fail(c, FFH_ERR_BAD_ARG, "bag_weights_grad: a misaligned pointer");
    for (int k = 0; k < i; k++)
      if (gw[i] && gw[k] == gw[i]) return ffh_fail(c, FFH_ERR_BAD_ARG, "bag_weights_grad: two tables of one call share a destination (one call per table on a buffer)");
    if (gw_ld[i] > INT32_MAX || tables[i].ld > INT32_MAX)
      return ffh_fail(c, FFH_ERR_UNSUPPORTED, "bag_weights_grad: a leading dimension of 2^31 or more");
  }
  // the 16-byte form (bf16 rows: 8-byte row loads) where every table and every dY row allows it, the 4-byte form otherwise
  bool v4 = D % 4 == 0;
  for (int i = 0; i < nt; i++) v4 = v4 && ((uintptr_t)tables[i].weight & (4 * elem - 1)) == 0 && aligned16(tables[i].io) && tables[i].ld % 4 == 0;
  const int vec = v4 ? 4 : 1;
  const DotLanes g(D, vec);
  if (g.chunks() > kMaxCH)
    return ffh_fail(c, FFH_ERR_UNSUPPORTED, "bag_weights_grad: out_dim too large (1024 in the 16-byte form, 256 in the 4-byte form)");
  if (nt == 0 || batch == 0) return FFH_OK;
  WGradArgs a;
  memset(&a, 0, sizeof a);
  for (int i = 0; i < nt; i++) {
    a.t[i] = WGradTable{tables[i].idx, tables[i].weight, tables[i].io, gw[i], (int32_t)tables[i].ld, (int32_t)gw_ld[i]};
    a.L[i] = (uint16_t)in_dims[i];
  }
  a.batch = batch; a.ntables = nt; a.D = D;
  a.accumulate = (flags & FFH_BAG_WGRAD_ACCUMULATE) != 0;
  const int64_t bpb_short = g.block_bags(4), bpb_long = g.block_bags(2);      // wgrad_bags<.., U = 4 / 2, ..>
  a.nrb[0] = (batch + bpb_short - 1) / bpb_short;
  a.nrb[1] = (batch + bpb_long - 1) / bpb_long;
  // workgroups in proportion to the lookups: the smallest shift at which the tables' shares fit the cap
  int64_t total = 0;
  for (int sh = 0; sh < 63; sh++) {
    total = 0;
    for (int i = 0; i < nt; i++) total += bag_blocks(batch, in_dims[i], sh, a.nrb[in_dims[i] >= kBagLong ? 1 : 0]);
    a.shift = sh;
    if (total <= kGridCap) break;
  }
  if (vec == 4) wgrad_launch_ch<4, WT>(g.chunks(), (unsigned)total, as_stream(s), a);
  else wgrad_launch_ch<1, WT>(g.chunks(), (unsigned)total, as_stream(s), a);
  FFH_LAUNCH_CHECK(c, "bag_wgrad_kernel");
  return FFH_OK;
}

}  // namespace

extern "C" {

int ffh_bag_weights_grad_abi_version(void) { return FFH_BAG_WEIGHTS_GRAD_ABI_VERSION; }

int64_t ffh_bag_weights_grad_grid_cap(void) { return kGridCap; }

int ffh_bag_weights_grad(ffh_ctx* c, const ffh_emb_table* tables, float* const* gw, const int64_t* gw_ld, const int* in_dims, int nt, int D, int64_t batch,
                         int flags, ffh_stream s) {
  return wgrad_launch<float>(c, tables, gw, gw_ld, in_dims, nt, D, batch, flags, s);
}

int ffh_bag_weights_grad_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, float* const* gw, const int64_t* gw_ld, const int* in_dims, int nt, int D,
                              int64_t batch, int flags, ffh_stream s) {
  ffh_emb_table t[FFH_MAX_TABLES];
  const int rc = bf16_tables(c, tables, nt, t, nullptr);
  if (rc) return rc;
  return wgrad_launch<uint16_t>(c, nt > 0 ? t : nullptr, gw, gw_ld, in_dims, nt, D, batch, flags, s);
}

}  // extern "C"
