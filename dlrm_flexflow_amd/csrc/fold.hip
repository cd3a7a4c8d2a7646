// fold.hip -- small embedding tables folded out of the forward GEMM of the layer that reads them (include/ff_hip_fold.h).
//
// The first top layer of a `cat` DLRM multiplies [batch][in] by [out][in]; the column block of a table with R rows holds copies of at
// most R distinct rows, so its share of the product is (E W_t^T)[ids]: one small GEMM per table (fold_gemm_kernel, all tables in one
// launch), one gather-add of rows of the products per sample (fold_gather_add_kernel), and the big GEMM over the columns that are left
// with the gathered sum as an addend in its epilogue (linear_sk.hip's FOLD instantiation; fold_gemm_kernel where that does not serve).
//
// fold_gemm_kernel: C[r][n] = sum over the kept k of A[r][k] W[n][wcol0 + k], both operands k-contiguous, v_mfma_f32_16x16x4_f32 straight
// from global memory (the operands of the products are a few MB that live in L2; the big layers never come here).  One wave owns 32 rows
// x 64 columns: W is the MFMA's row operand, A its column operand, so a lane ends up with four consecutive columns of one row and stores
// 16 bytes.  Lane (c, q) loads 16 bytes at k = 16 j + 4 q of its rows; component e of both operands feeds MFMA e of the group -- any
// assignment of k to the MFMA's four k-slots is legal as long as both operands agree (the trick of linear_sk.hip's k-contiguous image).
// Order of the sum per element: segments in list order, groups of 16 ascending, e = 0..3, the MFMA's own order over q: fixed.
//
// The weight gradient of the same layer (ABI 2): dW[:, cols_t] = G_t^T E_t with G_t the segmented sum of dy over the table's rows -- the sum by
// fold_sum.hip's wide-row kernels behind embedding.hip's sort, or by embedding.hip's fused update on zeroed rows where those do not serve
// (ffh_fold_segment_sum), the products by fold_dw_product_kernel, the GEMM over the column tiles that are left by linear_sk.hip's KEPT
// instantiation (ffh_fold_linear_bwd_dw).
//
// The data gradient (ABI 3): the only reader of dX[:, cols_t] is table t's update, and sum_hits dX[b][cols_t] = G_t W[:, cols_t] -- the GEMM over the
// column tiles that are left by linear_sk.hip's KEPT data-gradient instantiations (ffh_fold_linear_bwd_dx), the tables' plain-SGD step as one dense
// product from the G the weight gradient has formed already (fold_table_update_kernel).
#include "fold_sum.h"
#include "linear_gemm.h"
#include "lr_state.h"

#include "../../include/ff_hip_fold.h"

using namespace ffh_gemm;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct FoldGemmGroup { const float* a; int64_t lda; int64_t wcol0; float* c; int64_t ldc; int rows; int tile0; };   // tile0: the group's first wave tile in the launch
struct FoldGemmArgs {
  FoldGemmGroup grp[FFH_FOLD_MAX_GROUPS];
  ffh_fold_seg  seg[FFH_FOLD_MAX_SEGS];
  const float*  w; int64_t ldw;
  const float*  bias;            // EPI: per-column bias or null
  const float*  addend; int64_t ldadd;   // EPI: addend[r][n] or null (one group)
  int ngroups, nseg, N, act, ntiles;
};
static_assert(sizeof(FoldGemmArgs) <= 4096, "kernel arguments");

template <bool EPI>
__global__ __launch_bounds__(256) void fold_gemm_kernel(const FoldGemmArgs g) {
  ffh_kernel_prio();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c = lane & 15, q = lane >> 4;
  const int wt = (int)blockIdx.x * 4 + wave;
  if (wt >= g.ntiles) return;
  int gi = 0;
  while (gi + 1 < g.ngroups && g.grp[gi + 1].tile0 <= wt) gi++;       // uniform
  const FoldGemmGroup G = g.grp[gi];
  const int ct = g.N / 64, local = wt - G.tile0;
  const int r0 = (local / ct) * 32, n0 = (local % ct) * 64;
  const float* ap[2];
  const float* wp[4];
#pragma unroll
  for (int mt = 0; mt < 2; mt++) {
    int r = r0 + 16 * mt + c;
    if (r > G.rows - 1) r = G.rows - 1;                                // rows behind the table: any valid row, never stored
    ap[mt] = G.a + (int64_t)r * G.lda + 4 * q;
  }
#pragma unroll
  for (int nt = 0; nt < 4; nt++) wp[nt] = g.w + (int64_t)(n0 + 16 * nt + c) * g.ldw + G.wcol0 + 4 * q;
  f32x4 acc[4][2];
#pragma unroll
  for (int nt = 0; nt < 4; nt++)
#pragma unroll
    for (int mt = 0; mt < 2; mt++) acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int si = 0; si < g.nseg; si++) {
    const int k0 = g.seg[si].k0, k1 = k0 + g.seg[si].len;
    for (int k = k0; k < k1; k += 16) {
      f32x4 a[2], b[4];
#pragma unroll
      for (int mt = 0; mt < 2; mt++) a[mt] = *reinterpret_cast<const f32x4*>(ap[mt] + k);
#pragma unroll
      for (int nt = 0; nt < 4; nt++) b[nt] = *reinterpret_cast<const f32x4*>(wp[nt] + k);
#pragma unroll
      for (int e = 0; e < 4; e++)
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
#pragma unroll
          for (int mt = 0; mt < 2; mt++) acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[nt][e], a[mt][e], acc[nt][mt], 0, 0, 0);
    }
  }
  // lane (c, q): columns n0 + 16 nt + 4 q + {0..3} of row r0 + 16 mt + c
#pragma unroll
  for (int mt = 0; mt < 2; mt++) {
    const int r = r0 + 16 * mt + c;
    if (r >= G.rows) continue;
#pragma unroll
    for (int nt = 0; nt < 4; nt++) {
      const int n = n0 + 16 * nt + 4 * q;
      f32x4 v = acc[nt][mt];
      if constexpr (EPI) {
        if (g.addend) v += *reinterpret_cast<const f32x4*>(g.addend + (int64_t)r * g.ldadd + n);
        if (g.bias) v += f32x4{g.bias[n], g.bias[n + 1], g.bias[n + 2], g.bias[n + 3]};
        if (g.act != FFH_AC_MODE_NONE) { v.x = act_apply(v.x, g.act); v.y = act_apply(v.y, g.act); v.z = act_apply(v.z, g.act); v.w = act_apply(v.w, g.act); }
      }
      *reinterpret_cast<f32x4*>(G.c + (int64_t)r * G.ldc + n) = v;
    }
  }
}

// fold_gather_add_kernel: one lane per 16 bytes of S.  The (table, position) pairs are walked four at a time: four ids, then four rows in flight, then
// the adds in list order.  The rows come out of L2 / the Infinity Cache (the products of all folded tables are a few tens of MB).
struct FoldGatherTable { const int64_t* idx; const float* p; };
struct FoldGatherArgs {
  FoldGatherTable t[FFH_MAX_TABLES];
  float* S; int64_t ldS;
  int64_t batch;
  int ntables, L, out;
};

__global__ __launch_bounds__(256) void fold_gather_add_kernel(const FoldGatherArgs g) {
  ffh_kernel_prio();
  const int nvec = g.out / 4;
  const int64_t total = g.batch * nvec;
  const int n = g.ntables * g.L;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / nvec;
    const int cv = (int)(i - b * nvec) * 4;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < n; j0 += 4) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int j = j0 + u;
        if (j < n) {        // uniform
          const int t = j / g.L, l = j - t * g.L;
          const int64_t id = g.t[t].idx[b * g.L + l];
          v[u] = *reinterpret_cast<const f32x4*>(g.t[t].p + id * g.out + cv);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (j0 + u < n) acc = (j0 + u == 0) ? v[u] : acc + v[u];
    }
    *reinterpret_cast<f32x4*>(g.S + b * g.ldS + cv) = acc;
  }
}

// fold_dw_product_kernel: dW[o][col0 + d] += sum over a chunk of rows r of G[r][o] E[r][d] -- both operands rows-are-k.  One wave owns 64 outputs x
// 64 columns of one chunk of FFH_FOLD_DW_CHUNK rows of one table; lane (c, q) loads 16 bytes of row k + q of either operand: ONE k-step of FOUR
// 16-wide tiles (tile t holds outputs / columns 4 c + t -- linear_sk.hip's rows-are-k image, read from global memory instead of LDS).  Rows behind
// the table's last contribute zeros (loaded from its last row, then cleared).  The next 16 rows are in flight while the MFMAs of these run.  The
// chunks of a table meet in dW by float atomics, through a per-wave LDS image so that one atomic instruction covers 256 contiguous bytes of one
// row of dW (the epilogue of the stream-K weight gradient, which writes the neighbouring columns under the same contract).
constexpr int FOLD_DW_EP_LD = 68;      // floats per row of the wave's epilogue image: 64 + 4 of padding
struct FoldDwGroup { const float* g; const float* e; int64_t lde; int64_t col0; int rows; int tile0; };   // tile0: the group's first wave tile in the launch
struct FoldDwArgs {
  FoldDwGroup grp[FFH_FOLD_MAX_GROUPS];
  float* dw; int64_t lddw;
  int ngroups, out, d, ntiles;
};
static_assert(sizeof(FoldDwArgs) <= 4096, "kernel arguments");

__global__ __launch_bounds__(256) void fold_dw_product_kernel(const FoldDwArgs g) {
  __shared__ __attribute__((aligned(16))) float ep_all[4][16 * FOLD_DW_EP_LD];
  ffh_kernel_prio();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c = lane & 15, q = lane >> 4;
  const int wt = (int)blockIdx.x * 4 + wave;
  if (wt >= g.ntiles) return;
  int gi = 0;
  while (gi + 1 < g.ngroups && g.grp[gi + 1].tile0 <= wt) gi++;       // uniform
  const FoldDwGroup G = g.grp[gi];
  const int ot = g.out / 64, dt = g.d / 64, local = wt - G.tile0;
  const int chunk = local / (ot * dt), rem = local - chunk * (ot * dt);
  const int o0 = (rem / dt) * 64, d0 = (rem % dt) * 64;
  const int rb = chunk * FFH_FOLD_DW_CHUNK;
  const int re = rb + FFH_FOLD_DW_CHUNK < G.rows ? rb + FFH_FOLD_DW_CHUNK : G.rows;      // rb < re <= G.rows
  const float* gp = G.g + o0 + 4 * c;
  const float* epn = G.e + d0 + 4 * c;
  f32x4 acc[4][4];
#pragma unroll
  for (int tm = 0; tm < 4; tm++)
#pragma unroll
    for (int tn = 0; tn < 4; tn++) acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 a[4], b[4], an[4], bn[4];
  auto load16 = [&](int k, f32x4* av, f32x4* bv) {      // rows k + 4 u + q, u = 0..3
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int r = k + 4 * u + q;
      const int rc = r < re ? r : re - 1;
      av[u] = *reinterpret_cast<const f32x4*>(gp + (int64_t)rc * g.out);
      bv[u] = *reinterpret_cast<const f32x4*>(epn + (int64_t)rc * G.lde);
      if (r >= re) av[u] = f32x4{0.f, 0.f, 0.f, 0.f};     // (a zero times whatever the valid row holds: finite tables, as everywhere)
    }
  };
  load16(rb, a, b);
  for (int k = rb; k < re; k += 16) {
    if (k + 16 < re) load16(k + 16, an, bn);      // uniform
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int tm = 0; tm < 4; tm++)
#pragma unroll
        for (int tn = 0; tn < 4; tn++) acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][tm], b[u][tn], acc[tm][tn], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < 4; u++) { a[u] = an[u]; b[u] = bn[u]; }
  }
  // lane (c, q) holds, for tm, tn, i in 0..3, output o0 + 16 q + 4 i + tm, column d0 + 4 c + tn: the layout of the stream-K weight gradient's wave
  float* const ep = ep_all[wave];
  float* crow = g.dw + (int64_t)o0 * g.lddw + G.col0 + d0 + lane;
#pragma unroll
  for (int p = 0; p < 4; p++) {            // outputs 16 p .. 16 p + 15 of the wave's result are held by the lanes with q == p
    if (q == p) {
#pragma unroll
      for (int tm = 0; tm < 4; tm++)
#pragma unroll
        for (int i = 0; i < 4; i++)
          *reinterpret_cast<f32x4*>(ep + (4 * i + tm) * FOLD_DW_EP_LD + 4 * c) = f32x4{acc[tm][0][i], acc[tm][1][i], acc[tm][2][i], acc[tm][3][i]};
    }
    __builtin_amdgcn_wave_barrier();       // the wave's own image: no workgroup barrier (a wave's ds operations complete in order)
#pragma unroll
    for (int r = 0; r < 16; r++) atomicAdd(crow + (int64_t)(16 * p + r) * g.lddw, ep[r * FOLD_DW_EP_LD + lane]);
    __builtin_amdgcn_wave_barrier();
  }
}

// fold_table_update_kernel (ABI 3): E[r][d] = fmaf(-lr, sum_o G[r][o] W[o][col0 + d], E[r][d]) -- G k-contiguous, W rows-are-k.  One wave owns 32 rows x 64
// columns of one table over the whole depth `out`: a 16-deep group is 16 bytes of G per lane (lane (c, q): o = 16 j + 4 q + {0..3} of rows r0 + 16 mt + c,
// fold_gemm_kernel's image) and four 16-byte loads of W (rows o = 16 j + 4 q + e, e = 0..3, columns d0 + 4 c + {0..3}: fold_dw_product_kernel's image, ONE
// depth step of FOUR 16-wide column tiles, tile tn holding columns 4 c + tn); component e of G meets row e of W in MFMA e.  W is the MFMA's row operand, so
// lane (c, q) ends up with columns d0 + 4 (4 q + i) + tn of row r0 + 16 mt + c: for every i four consecutive columns, 16 bytes of E read, updated and stored.
// The next group's operands are in flight while the MFMAs of this one run.  Order per element: j ascending, e = 0..3, the MFMA's own order over q; one fmaf.
// Rows behind the table's last: loaded from its last row, never stored.  Nothing is shared between waves: no LDS, no atomics.
struct FoldUpdGroup { const float* g; float* e; int64_t lde; int64_t col0; int rows; int tile0; };   // tile0: the group's first wave tile in the launch
struct FoldUpdArgs {
  FoldUpdGroup grp[FFH_FOLD_MAX_GROUPS];
  const float* w; int64_t ldw;
  const float* lr_ptr; float lr;      // the rate: *lr_ptr where given (include/ff_hip_lr.h), else lr
  int ngroups, out, d, ntiles;
};
static_assert(sizeof(FoldUpdArgs) <= 4096, "kernel arguments");

__global__ __launch_bounds__(256) void fold_table_update_kernel(const FoldUpdArgs g) {
  ffh_kernel_prio();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c = lane & 15, q = lane >> 4;
  const int wt = (int)blockIdx.x * 4 + wave;
  if (wt >= g.ntiles) return;
  int gi = 0;
  while (gi + 1 < g.ngroups && g.grp[gi + 1].tile0 <= wt) gi++;       // uniform
  const FoldUpdGroup G = g.grp[gi];
  const int dt = g.d / 64, local = wt - G.tile0;
  const int r0 = (local / dt) * 32, d0 = (local % dt) * 64;
  const float nlr = -(g.lr_ptr ? *g.lr_ptr : g.lr);
  const float* gp[2];
#pragma unroll
  for (int mt = 0; mt < 2; mt++) {
    int r = r0 + 16 * mt + c;
    if (r > G.rows - 1) r = G.rows - 1;                                // rows behind the table: any valid row, never stored
    gp[mt] = G.g + (int64_t)r * g.out + 4 * q;
  }
  const float* wp = g.w + (int64_t)(4 * q) * g.ldw + G.col0 + d0 + 4 * c;
  f32x4 acc[2][4];
#pragma unroll
  for (int mt = 0; mt < 2; mt++)
#pragma unroll
    for (int tn = 0; tn < 4; tn++) acc[mt][tn] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 a[2], b[4], an[2], bn[4];
  auto load16 = [&](int k, f32x4* av, f32x4* bv) {      // depth k .. k + 15
#pragma unroll
    for (int mt = 0; mt < 2; mt++) av[mt] = *reinterpret_cast<const f32x4*>(gp[mt] + k);
#pragma unroll
    for (int e = 0; e < 4; e++) bv[e] = *reinterpret_cast<const f32x4*>(wp + (int64_t)(k + e) * g.ldw);
  };
  load16(0, a, b);
  for (int k = 0; k < g.out; k += 16) {
    if (k + 16 < g.out) load16(k + 16, an, bn);         // uniform
#pragma unroll
    for (int e = 0; e < 4; e++)
#pragma unroll
      for (int tn = 0; tn < 4; tn++)
#pragma unroll
        for (int mt = 0; mt < 2; mt++) acc[mt][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[e][tn], a[mt][e], acc[mt][tn], 0, 0, 0);
#pragma unroll
    for (int mt = 0; mt < 2; mt++) a[mt] = an[mt];
#pragma unroll
    for (int e = 0; e < 4; e++) b[e] = bn[e];
  }
#pragma unroll
  for (int mt = 0; mt < 2; mt++) {
    const int r = r0 + 16 * mt + c;
    if (r >= G.rows) continue;
    float* erow = G.e + (int64_t)r * G.lde + d0 + 16 * q;
    f32x4 old[4];
#pragma unroll
    for (int i = 0; i < 4; i++) old[i] = *reinterpret_cast<const f32x4*>(erow + 4 * i);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      f32x4 v;
      v.x = fmaf(nlr, acc[mt][0][i], old[i].x); v.y = fmaf(nlr, acc[mt][1][i], old[i].y);
      v.z = fmaf(nlr, acc[mt][2][i], old[i].z); v.w = fmaf(nlr, acc[mt][3][i], old[i].w);
      *reinterpret_cast<f32x4*>(erow + 4 * i) = v;
    }
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int fold_table_update_launch(ffh_ctx* c, const ffh_fold_group* groups, int ngroups, const float* w, int64_t ldw, int d, int out, const float* lr_ptr, float lr,
                             ffh_stream s) {
  FFH_REQUIRE(c, groups && w && ngroups >= 1 && d > 0 && out > 0 && ldw >= d, "fold_table_update: bad arguments");
  if (ngroups > FFH_FOLD_MAX_GROUPS || d % 64 || out % FFH_FOLD_NTILE || !al16(w) || ldw % 4)
    return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_table_update: d and out_dim multiples of 64, at most 64 tables, aligned weight");
  FoldUpdArgs a{};
  int64_t tiles = 0;
  for (int i = 0; i < ngroups; i++) {
    const ffh_fold_group& gr = groups[i];
    FFH_REQUIRE(c, gr.e && gr.p && gr.rows >= 1 && gr.rows < (1LL << 31) && gr.lde >= d && gr.col0 >= 0 && gr.col0 + d <= ldw, "fold_table_update: bad group");
    if (!al16(gr.e) || !al16(gr.p) || gr.lde % 4 || gr.col0 % 4) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_table_update: group not aligned");
    a.grp[i] = FoldUpdGroup{gr.p, const_cast<float*>(gr.e), gr.lde, gr.col0, (int)gr.rows, (int)tiles};
    tiles += ((gr.rows + 31) / 32) * (d / 64);
    FFH_REQUIRE(c, tiles < (1LL << 30), "fold_table_update: too many rows");
  }
  a.w = w; a.ldw = ldw; a.lr_ptr = lr_ptr; a.lr = lr; a.ngroups = ngroups; a.out = out; a.d = d; a.ntiles = (int)tiles;
  hipLaunchKernelGGL(fold_table_update_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, as_stream(s), a);
  FFH_LAUNCH_CHECK(c, "fold_table_update_kernel");
  return FFH_OK;
}

// the checks ffh_fold_linear_bwd_dx and its plan query share; FFH_OK, or the error left in the ctx
int fold_dx_check(ffh_ctx* c, const float* x, int64_t ldx, const float* dx, int64_t lddx, const float* dy, int64_t lddy, const float* w, int in, int out,
                  int64_t batch, int flags, const int32_t* kept, int nkept) {
  FFH_REQUIRE(c, in > 0 && out > 0 && batch >= 0 && lddx >= in && lddy >= out, "fold_linear_bwd_dx: bad dims");
  FFH_REQUIRE(c, !(flags & ~(FFH_LINEAR_DX_OVERWRITE | FFH_LINEAR_DX_MASK_BY_X)), "fold_linear_bwd_dx: flags are DX_OVERWRITE and DX_MASK_BY_X");
  FFH_REQUIRE(c, !(flags & FFH_LINEAR_DX_MASK_BY_X) || (x && ldx >= in), "fold_linear_bwd_dx: the mask needs x");
  FFH_REQUIRE(c, batch == 0 || (dx && dy && w), "fold_linear_bwd_dx: null pointer");
  FFH_REQUIRE(c, batch < (1LL << 31), "fold_linear_bwd_dx: batch too large");
  FFH_REQUIRE(c, nkept >= 1 && kept, "fold_linear_bwd_dx: bad tile list");
  for (int i = 0; i < nkept; i++)
    FFH_REQUIRE(c, kept[i] >= 0 && ((int64_t)kept[i] + 1) * FFH_FOLD_DW_NTILE <= in && (i == 0 || kept[i] > kept[i - 1]), "fold_linear_bwd_dx: tiles must ascend inside [0, in_dim)");
  return FFH_OK;
}
GemmArgs fold_dx_gemm(const float* x, int64_t ldx, float* dx, int64_t lddx, const float* dy, int64_t lddy, const float* w, int in, int out, int64_t batch, int flags) {
  GemmArgs g{};      // as linear.hip states the data gradient of a layer whose dy is final
  g.A = dy; g.sAm = lddy; g.sAk = 1;
  g.B = w; g.sBn = 1; g.sBk = in;
  g.C = dx; g.ldc = lddx;
  g.M = (int)batch; g.N = in; g.K = out;
  g.epi = (flags & FFH_LINEAR_DX_OVERWRITE) ? EPI_STORE : EPI_ADD; g.act = FFH_AC_MODE_NONE;
  if (flags & FFH_LINEAR_DX_MASK_BY_X) { g.mask = x; g.ldmask = ldx; }
  return g;
}

// the checks ffh_fold_linear_bwd_dw and its plan query share; FFH_OK, or the error left in the ctx
int fold_dw_check(ffh_ctx* c, const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* dw, int in, int out, int64_t batch,
                  const int32_t* kept, int nkept) {
  FFH_REQUIRE(c, in > 0 && out > 0 && batch >= 0 && ldx >= in && lddy >= out, "fold_linear_bwd_dw: bad dims");
  FFH_REQUIRE(c, batch == 0 || (x && dy && dw), "fold_linear_bwd_dw: null pointer");
  FFH_REQUIRE(c, batch < (1LL << 31), "fold_linear_bwd_dw: batch too large");
  FFH_REQUIRE(c, nkept >= 1 && kept, "fold_linear_bwd_dw: bad tile list");
  for (int i = 0; i < nkept; i++)
    FFH_REQUIRE(c, kept[i] >= 0 && ((int64_t)kept[i] + 1) * FFH_FOLD_DW_NTILE <= in && (i == 0 || kept[i] > kept[i - 1]), "fold_linear_bwd_dw: tiles must ascend inside [0, in_dim)");
  return FFH_OK;
}
GemmArgs fold_dw_gemm(const float* x, int64_t ldx, const float* dy, int64_t lddy, float* dw, float* db, int in, int out, int64_t batch) {
  GemmArgs g{};      // as linear.hip states the weight gradient of a layer whose dy is final
  g.A = dy; g.sAm = 1; g.sAk = lddy;
  g.B = x; g.sBn = 1; g.sBk = ldx;
  g.C = dw; g.ldc = in;
  g.M = out; g.N = in; g.K = (int)batch;
  g.epi = EPI_ATOMIC; g.act = FFH_AC_MODE_NONE;
  g.db = db;
  return g;
}

// the checks ffh_fold_linear_fwd and its plan query share; FFH_OK, or the error left in the ctx
int fold_fwd_check(ffh_ctx* c, const float* x, int64_t ldx, const float* y, int64_t ldy, const float* w, int in, int out, int64_t batch,
                   const ffh_fold_seg* keep, int nkeep, const float* addend, int64_t ldadd) {
  FFH_REQUIRE(c, in > 0 && out > 0 && batch >= 0 && ldx >= in && ldy >= out, "fold_linear_fwd: bad dims");
  FFH_REQUIRE(c, batch == 0 || (x && y && w), "fold_linear_fwd: null pointer");
  FFH_REQUIRE(c, batch < (1LL << 31), "fold_linear_fwd: batch too large");
  FFH_REQUIRE(c, nkeep >= 0 && (nkeep == 0 || keep), "fold_linear_fwd: bad segment list");
  FFH_REQUIRE(c, !addend || ldadd >= out, "fold_linear_fwd: bad addend");
  int prev = 0;
  for (int i = 0; i < nkeep; i++) {
    FFH_REQUIRE(c, keep[i].k0 >= prev && keep[i].len > 0 && (int64_t)keep[i].k0 + keep[i].len <= in, "fold_linear_fwd: segments must ascend inside [0, in_dim)");
    prev = keep[i].k0 + keep[i].len;
  }
  return FFH_OK;
}
bool fold_fwd_served(const ffh_ctx* c, const float* x, int64_t ldx, const float* y, int64_t ldy, const float* w, int in, int out,
                     const ffh_fold_seg* keep, int nkeep, const float* addend, int64_t ldadd) {
  if (c->math_mode != FFH_MATH_DEFAULT) return false;
  if (in % FFH_FOLD_KTILE || out % FFH_FOLD_NTILE || nkeep > FFH_FOLD_MAX_SEGS) return false;
  if (!al16(x) || !al16(y) || !al16(w) || ldx % 4 || ldy % 4 || (addend && (!al16(addend) || ldadd % 4))) return false;
  for (int i = 0; i < nkeep; i++)
    if (keep[i].k0 % FFH_FOLD_KTILE || keep[i].len % FFH_FOLD_KTILE) return false;
  return true;
}
// the kept k-tiles as the persistent kernel takes them; false: not whole 64-deep k-tiles / too deep
bool fold_keep_mask(int in, const ffh_fold_seg* keep, int nkeep, unsigned long long mask[2], int* nk_kept) {
  mask[0] = mask[1] = 0;
  *nk_kept = 0;
  if (in % 64 || in > 128 * 64) return false;
  const ffh_fold_seg all{0, in};
  if (nkeep == 0) { keep = &all; nkeep = 1; }
  for (int i = 0; i < nkeep; i++) {
    if (keep[i].k0 % 64 || keep[i].len % 64) return false;
    for (int kt = keep[i].k0 / 64; kt < (keep[i].k0 + keep[i].len) / 64; kt++) { mask[kt >> 6] |= 1ull << (kt & 63); (*nk_kept)++; }
  }
  return *nk_kept > 0;
}
GemmArgs fold_fwd_gemm(const float* x, int64_t ldx, float* y, int64_t ldy, const float* w, const float* bias, int in, int out, int64_t batch, int act) {
  GemmArgs g{};
  g.A = x; g.sAm = ldx; g.sAk = 1;
  g.B = w; g.sBn = in; g.sBk = 1;
  g.C = y; g.ldc = ldy; g.bias = bias;
  g.M = (int)batch; g.N = out; g.K = in;
  g.epi = EPI_STORE; g.act = act;
  return g;
}

}  // namespace

extern "C" {

int ffh_fold_abi_version(void) { return FFH_FOLD_ABI_VERSION; }

int ffh_fold_product(ffh_ctx* c, const ffh_fold_group* groups, int ngroups, const float* w, int64_t ldw, int d, int out, ffh_stream s) {
  FFH_REQUIRE(c, groups && w && ngroups >= 1 && d > 0 && out > 0 && ldw >= d, "fold_product: bad arguments");
  if (ngroups > FFH_FOLD_MAX_GROUPS || d % FFH_FOLD_KTILE || out % FFH_FOLD_NTILE || !al16(w) || ldw % 4)
    return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_product: d a multiple of 16, out_dim a multiple of 64, at most 64 tables, aligned weight");
  FoldGemmArgs a{};
  int64_t tiles = 0;
  for (int i = 0; i < ngroups; i++) {
    const ffh_fold_group& gr = groups[i];
    FFH_REQUIRE(c, gr.e && gr.p && gr.rows >= 1 && gr.rows < (1LL << 31) && gr.lde >= d && gr.col0 >= 0 && gr.col0 + d <= ldw, "fold_product: bad group");
    if (!al16(gr.e) || !al16(gr.p) || gr.lde % 4 || gr.col0 % FFH_FOLD_KTILE) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_product: group not aligned");
    a.grp[i] = FoldGemmGroup{gr.e, gr.lde, gr.col0, gr.p, (int64_t)out, (int)gr.rows, (int)tiles};
    tiles += ((gr.rows + 31) / 32) * (out / 64);
    FFH_REQUIRE(c, tiles < (1LL << 30), "fold_product: too many rows");
  }
  a.seg[0] = ffh_fold_seg{0, d};
  a.w = w; a.ldw = ldw; a.ngroups = ngroups; a.nseg = 1; a.N = out; a.act = FFH_AC_MODE_NONE; a.ntiles = (int)tiles;
  hipLaunchKernelGGL(fold_gemm_kernel<false>, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, as_stream(s), a);
  FFH_LAUNCH_CHECK(c, "fold_gemm_kernel (products)");
  return FFH_OK;
}

int ffh_fold_gather_add(ffh_ctx* c, const ffh_emb_table* tables, int ntables, int in_dim, int out, int64_t batch, int aggr, float* S, int64_t ldS,
                        ffh_stream s) {
  FFH_REQUIRE(c, tables && ntables >= 1 && in_dim >= 1 && out > 0 && batch >= 0 && S && ldS >= out, "fold_gather_add: bad arguments");
  if (aggr != FFH_AGGR_MODE_SUM) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_gather_add: sum aggregation only");
  if (ntables > FFH_MAX_TABLES || out % 4 || ldS % 4 || !al16(S)) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_gather_add: out_dim and ldS multiples of 4, aligned S, at most 64 tables");
  FoldGatherArgs a{};
  for (int t = 0; t < ntables; t++) {
    FFH_REQUIRE(c, tables[t].idx && tables[t].weight && tables[t].num_entries >= 1, "fold_gather_add: bad table");
    if (!al16(tables[t].weight)) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_gather_add: product not aligned");
    a.t[t] = FoldGatherTable{tables[t].idx, tables[t].weight};
  }
  if (batch == 0) return FFH_OK;
  a.S = S; a.ldS = ldS; a.batch = batch; a.ntables = ntables; a.L = in_dim; a.out = out;
  hipLaunchKernelGGL(fold_gather_add_kernel, dim3(ffh_grid(batch * (out / 4), 256, 4096)), dim3(256), 0, as_stream(s), a);
  FFH_LAUNCH_CHECK(c, "fold_gather_add_kernel");
  return FFH_OK;
}

int ffh_fold_linear_fwd_plan(ffh_ctx* c, const float* x, int64_t ldx, const float* y, int64_t ldy, const float* w, const float* bias, int in, int out,
                             int64_t batch, const ffh_fold_seg* keep, int nkeep, const float* addend, int64_t ldadd) {
  const int rc = fold_fwd_check(c, x, ldx, y, ldy, w, in, out, batch, keep, nkeep, addend, ldadd);
  if (rc != FFH_OK) return rc;
  if (!fold_fwd_served(c, x, ldx, y, ldy, w, in, out, keep, nkeep, addend, ldadd)) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_linear_fwd: shape / alignment / math mode not served");
  const GemmArgs g = fold_fwd_gemm(x, ldx, const_cast<float*>(y), ldy, w, bias, in, out, batch, FFH_AC_MODE_NONE);
  unsigned long long mask[2]; int nk = 0;
  if (batch > 0 && fold_keep_mask(in, keep, nkeep, mask, &nk) && launch_gemm_sk_fold(c, g, mask, nk, addend, ldadd, true, nullptr, "") == 1) return 2;
  return (batch > 0 && gemm_sk_serves(c, g, SK_FORM_FWD)) ? 0 : 1;
}

int ffh_fold_linear_fwd(ffh_ctx* c, const float* x, int64_t ldx, float* y, int64_t ldy, const float* w, const float* bias, int in, int out, int64_t batch,
                        int act, const ffh_fold_seg* keep, int nkeep, const float* addend, int64_t ldadd, ffh_stream s) {
  if (nkeep == 0 && !addend) return ffh_linear_fwd(c, x, ldx, y, ldy, w, bias, in, out, batch, act, s);
  const int rc = fold_fwd_check(c, x, ldx, y, ldy, w, in, out, batch, keep, nkeep, addend, ldadd);
  if (rc != FFH_OK) return rc;
  if (act != FFH_AC_MODE_NONE && act != FFH_AC_MODE_RELU && act != FFH_AC_MODE_SIGMOID && act != FFH_AC_MODE_GELU)
    return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_linear_fwd: activation not supported (NONE, RELU, SIGMOID, GELU)");
  if (!fold_fwd_served(c, x, ldx, y, ldy, w, in, out, keep, nkeep, addend, ldadd)) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_linear_fwd: shape / alignment / math mode not served");
  ffh_route_clear(c);
  if (batch == 0) return FFH_OK;
  const GemmArgs g = fold_fwd_gemm(x, ldx, y, ldy, w, bias, in, out, batch, act);
  unsigned long long mask[2]; int nk = 0;
  if (fold_keep_mask(in, keep, nkeep, mask, &nk) && (!bias || al16(bias))) {
    const int r = launch_gemm_sk_fold(c, g, mask, nk, addend, ldadd, false, s, "fold_linear_fwd gemm");
    if (r != 0) return r < 0 ? r : FFH_OK;
  }
  FoldGemmArgs a{};
  a.grp[0] = FoldGemmGroup{x, ldx, 0, y, ldy, (int)batch, 0};
  if (nkeep == 0) { a.seg[0] = ffh_fold_seg{0, in}; a.nseg = 1; }
  else { for (int i = 0; i < nkeep; i++) a.seg[i] = keep[i]; a.nseg = nkeep; }
  const int64_t tiles = ((batch + 31) / 32) * (out / 64);
  FFH_REQUIRE(c, tiles < (1LL << 30), "fold_linear_fwd: too many tiles");
  a.w = w; a.ldw = in; a.bias = bias; a.addend = addend; a.ldadd = ldadd; a.ngroups = 1; a.N = out; a.act = act; a.ntiles = (int)tiles;
  hipLaunchKernelGGL(fold_gemm_kernel<true>, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, as_stream(s), a);
  FFH_LAUNCH_CHECK(c, "fold_gemm_kernel (forward)");
  ffh_route_add(c, "fold_linear_fwd gemm|mfma_32x64x16");
  return FFH_OK;
}

// G_t = the segmented sum of dy over the hits of every row, in the fused table update's canonical order.  Wide aligned rows: that update's sort run to
// completion + fold_sum.hip's two launches.  Anything else: the fused table update itself on zeroed rows with lr = -1 (w = fmaf(1, sum, 0) = sum), so
// the sort, the ordered reduction and their summation order are embedding.hip's, launch for launch
int ffh_fold_segment_sum(ffh_ctx* c, const ffh_emb_table* tables, int ntables, int in_dim, int width, int64_t batch, ffh_stream s) {
  FFH_REQUIRE(c, tables && ntables >= 1 && in_dim >= 1 && width > 0 && batch >= 0, "fold_segment_sum: bad arguments");
  if (ntables > FFH_MAX_TABLES || batch * in_dim >= (1LL << 31)) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_segment_sum: at most 64 tables, batch * in_dim < 2^31");
  for (int t = 0; t < ntables; t++)
    FFH_REQUIRE(c, tables[t].weight && tables[t].num_entries >= 1 && (batch == 0 || (tables[t].idx && tables[t].io && tables[t].ld >= width)), "fold_segment_sum: bad table");
  if (batch > 0 && (!c->ws || c->ws_bytes < ffh_embedding_bwd_workspace_bytes(ntables, in_dim, width, batch) || ((uintptr_t)c->ws & 15)))
    return ffh_fail(c, FFH_ERR_WORKSPACE, "fold_segment_sum: workspace too small (ffh_embedding_bwd_workspace_bytes) or not 16-byte aligned");
  if (batch > 0) {      // wide aligned rows: fold_sum.hip, which writes every row of G itself
    const int wide = ffh_emb::fold_sum_wide(c, tables, ntables, in_dim, width, batch, s);
    if (wide != 0) return wide < 0 ? wide : FFH_OK;
  }
  for (int t = 0; t < ntables;) {      // tables that lie back to back (the usual case: one buffer) are cleared by one memset
    char* p0 = (char*)tables[t].weight;
    size_t bytes = 0;
    for (; t < ntables && (char*)tables[t].weight == p0 + bytes; t++) bytes += (size_t)tables[t].num_entries * (size_t)width * 4;
    const int rc = ffh_zero(c, p0, bytes, s);
    if (rc != FFH_OK) return rc;
  }
  if (batch == 0) return FFH_OK;
  return ffh_embedding_bwd_sgd_fused_multi(c, tables, ntables, in_dim, width, batch, FFH_AGGR_MODE_SUM, -1.0f, s);
}

int ffh_fold_dw_product(ffh_ctx* c, const ffh_fold_group* groups, int ngroups, float* dw, int64_t lddw, int d, int out, ffh_stream s) {
  FFH_REQUIRE(c, groups && dw && ngroups >= 1 && d > 0 && out > 0 && lddw >= d, "fold_dw_product: bad arguments");
  if (ngroups > FFH_FOLD_MAX_GROUPS || d % 64 || out % FFH_FOLD_NTILE) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_dw_product: d and out_dim multiples of 64, at most 64 tables");
  FoldDwArgs a{};
  int64_t tiles = 0;
  for (int i = 0; i < ngroups; i++) {
    const ffh_fold_group& gr = groups[i];
    FFH_REQUIRE(c, gr.e && gr.p && gr.rows >= 1 && gr.rows < (1LL << 31) && gr.lde >= d && gr.col0 >= 0 && gr.col0 + d <= lddw, "fold_dw_product: bad group");
    if (!al16(gr.e) || !al16(gr.p) || gr.lde % 4) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_dw_product: group not aligned");
    a.grp[i] = FoldDwGroup{gr.p, gr.e, gr.lde, gr.col0, (int)gr.rows, (int)tiles};
    tiles += ((gr.rows + FFH_FOLD_DW_CHUNK - 1) / FFH_FOLD_DW_CHUNK) * (out / 64) * (d / 64);
    FFH_REQUIRE(c, tiles < (1LL << 30), "fold_dw_product: too many rows");
  }
  a.dw = dw; a.lddw = lddw; a.ngroups = ngroups; a.out = out; a.d = d; a.ntiles = (int)tiles;
  hipLaunchKernelGGL(fold_dw_product_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, as_stream(s), a);
  FFH_LAUNCH_CHECK(c, "fold_dw_product_kernel");
  return FFH_OK;
}

int ffh_fold_linear_bwd_dw_plan(ffh_ctx* c, const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* dw, const float* db, int in, int out,
                                int64_t batch, const int32_t* kept, int nkept) {
  const int rc = fold_dw_check(c, x, ldx, dy, lddy, dw, in, out, batch, kept, nkept);
  if (rc != FFH_OK) return rc;
  if (batch == 0 || c->math_mode != FFH_MATH_DEFAULT) return 0;
  const GemmArgs g = fold_dw_gemm(x, ldx, dy, lddy, const_cast<float*>(dw), const_cast<float*>(db), in, out, batch);
  if (!gemm_sk_serves(c, g, SK_FORM_DW)) return 0;      // the whole layer does not run the stream-K form: leave it where it is
  return launch_gemm_sk_kept(c, g, kept, nkept, true, nullptr, "") == 1 ? 1 : 0;
}

int ffh_fold_linear_bwd_dw(ffh_ctx* c, const float* x, int64_t ldx, const float* dy, int64_t lddy, float* dw, float* db, int in, int out, int64_t batch,
                           const int32_t* kept, int nkept, ffh_stream s) {
  const int rc = fold_dw_check(c, x, ldx, dy, lddy, dw, in, out, batch, kept, nkept);
  if (rc != FFH_OK) return rc;
  ffh_route_clear(c);
  if (batch == 0 || c->math_mode != FFH_MATH_DEFAULT) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_linear_bwd_dw: empty batch / math mode not served");
  const GemmArgs g = fold_dw_gemm(x, ldx, dy, lddy, dw, db, in, out, batch);
  if (!gemm_sk_serves(c, g, SK_FORM_DW)) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_linear_bwd_dw: the layer's weight gradient does not run the stream-K form");
  const int r = launch_gemm_sk_kept(c, g, kept, nkept, false, s, "fold_linear_bwd_dw gemm");
  if (r < 0) return r;
  if (r == 0) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_linear_bwd_dw: too few kept tiles for the stream-K form, deterministic mode, or a bias gradient without tile 0");
  return FFH_OK;
}

int ffh_fold_linear_bwd_dx_plan(ffh_ctx* c, const float* x, int64_t ldx, const float* dx, int64_t lddx, const float* dy, int64_t lddy, const float* w, int in,
                                int out, int64_t batch, int flags, const int32_t* kept, int nkept, const float* colsum) {
  const int rc = fold_dx_check(c, x, ldx, dx, lddx, dy, lddy, w, in, out, batch, flags, kept, nkept);
  if (rc != FFH_OK) return rc;
  if (batch == 0 || c->math_mode != FFH_MATH_DEFAULT) return 0;
  const GemmArgs g = fold_dx_gemm(x, ldx, const_cast<float*>(dx), lddx, dy, lddy, w, in, out, batch, flags);
  return launch_gemm_sk_kept_dx(c, g, kept, nkept, const_cast<float*>(colsum), true, nullptr, "") == 1 ? 1 : 0;
}

int ffh_fold_linear_bwd_dx(ffh_ctx* c, const float* x, int64_t ldx, float* dx, int64_t lddx, const float* dy, int64_t lddy, const float* w, int in, int out,
                           int64_t batch, int flags, const int32_t* kept, int nkept, float* colsum, ffh_event record_behind, ffh_stream s) {
  const int rc = fold_dx_check(c, x, ldx, dx, lddx, dy, lddy, w, in, out, batch, flags, kept, nkept);
  if (rc != FFH_OK) return rc;
  ffh_route_clear(c);
  if (batch == 0 || c->math_mode != FFH_MATH_DEFAULT) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_linear_bwd_dx: empty batch / math mode not served");
  const GemmArgs g = fold_dx_gemm(x, ldx, dx, lddx, dy, lddy, w, in, out, batch, flags);
  const int r = launch_gemm_sk_kept_dx(c, g, kept, nkept, colsum, false, s, "fold_linear_bwd_dx gemm");
  if (r < 0) return r;
  if (r == 0)
    return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_linear_bwd_dx: the layer's data gradient does not run whole tiles on the persistent kernel, too few kept tiles, "
                                            "deterministic mode, or column sums without tile 0 / without DX_OVERWRITE");
  if (record_behind) FFH_HIP_TRY(c, hipEventRecord((hipEvent_t)record_behind, as_stream(s)));
  return FFH_OK;
}

int ffh_fold_table_update(ffh_ctx* c, const ffh_fold_group* groups, int ngroups, const float* w, int64_t ldw, int d, int out, float lr, ffh_stream s) {
  return fold_table_update_launch(c, groups, ngroups, w, ldw, d, out, nullptr, lr, s);
}

int ffh_fold_table_update_lr(ffh_ctx* c, const ffh_fold_group* groups, int ngroups, const float* w, int64_t ldw, int d, int out, const ffh_lr_state* block,
                             ffh_stream s) {
  FFH_REQUIRE(c, block, "fold_table_update_lr: null rate block");
  return fold_table_update_launch(c, groups, ngroups, w, ldw, d, out, ffh_lr_rate_ptr(block, false), 0.0f, s);
}

}  // extern "C"
