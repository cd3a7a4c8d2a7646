// linear_sk.hip -- the launches of the persistent fp32 GEMM kernel (linear_sk_kernel.h): which layers it serves, how the work is dealt, one launch per form.
#include "linear_sk_kernel.h"


namespace ffh_gemm {

namespace {
struct SkPlan { int64_t lda, ldb, a_bytes, b_bytes; int G; bool split; int tmw; };
bool sk_plan(const ffh_ctx* c, const GemmArgs& g, int form, SkPlan& p) {
  static const int off = FFH_LAB_INT("FFH_GEMM_NO_SK", 0);   // A/B switch (tools/ab.sh)
  if (off) return false;
  {
    // The backward GEMMs of a layer with fewer than 256 x 256 weights stay with the register-staged kernels: their workgroups
    // (33-37 KB of LDS, 100-160 registers) fit on a CU beside a persistent one, a second persistent workgroup does not (registers).  In
    // the DLRM step that layer is the bottom MLP's last one, whose backward is launched while the first top layer's stream-K weight
    // gradient holds a workgroup on every CU: as a persistent kernel it waited ~1.7 ms for CUs and the rest of the bottom MLP's
    // backward behind it (Terabyte step 8.07-8.10 -> 8.01-8.03 ms; at 140 K the two 512 x 256 layers move too: 8.13-8.15).
    // FFH_SK_MIN_WEIGHTS / _BWD: A/B switches (all forms / the two backward forms).
    static const int64_t min_w = FFH_LAB_I64("FFH_SK_MIN_WEIGHTS", 0);
    static const int64_t min_wb = FFH_LAB_I64("FFH_SK_MIN_WEIGHTS_BWD", 65536);
    const int64_t nw = form == SK_FORM_DW ? (int64_t)g.M * g.N : (int64_t)g.N * g.K;
    if (nw < min_w || (form != SK_FORM_FWD && nw < min_wb)) return false;
  }
  if (g.M % SK_BM || g.N % SK_BN || g.K % SK_BK || g.M <= 0 || g.N <= 0 || g.K <= 0) return false;      // (64-row tiles: M a multiple of 128 as well -- every other layer has it)
  const bool akr = form == SK_FORM_DW, bkr = form != SK_FORM_FWD;
  p.lda = akr ? g.sAk : g.sAm; p.ldb = bkr ? g.sBk : g.sBn;
  if ((akr ? g.sAm : g.sAk) != 1 || (bkr ? g.sBn : g.sBk) != 1) return false;
  if (!sk_aligned(g.A, p.lda) || !sk_aligned(g.B, p.ldb) || (!g.colmap && !sk_aligned(g.C, g.ldc))) return false;
  if (g.mask && !sk_aligned(g.mask, g.ldmask)) return false;
  if (g.bias && ((uintptr_t)g.bias & 15)) return false;
  if (g.act_y || g.fuse || g.splitk > 1) return false;  // masking-while-loading forms stay with linear.hip
  if (g.colmap && (form != SK_FORM_DX || g.epi != EPI_STORE || g.mask)) return false;     // the column map: plain stored data gradients only
  p.a_bytes = ((akr ? (int64_t)(g.K - 1) : (int64_t)(g.M - 1)) * p.lda + (akr ? g.M : g.K)) * 4;
  p.b_bytes = ((bkr ? (int64_t)(g.K - 1) : (int64_t)(g.N - 1)) * p.ldb + (bkr ? g.N : g.K)) * 4;
  if (p.a_bytes >= (1LL << 32) || p.b_bytes >= (1LL << 32)) return false;  // 32-bit buffer offsets
  p.G = c->num_cus & ~7;
  if (form == SK_FORM_DW && c->dw_cu_reserve > 0 && p.G - c->dw_cu_reserve >= 64) p.G -= c->dw_cu_reserve;     // ffh_ctx_set_dw_cu_reserve
  if (p.G < 8) return false;
  const int64_t ntiles = (int64_t)(g.M / SK_BM) * (g.N / SK_BN), nk = g.K / SK_BK;
  if (ntiles * nk >= (1LL << 31)) return false;
  p.tmw = 4;
  if (form == SK_FORM_DW) {
    if (c->deterministic || g.epi != EPI_ATOMIC) return false;     // its partial tiles meet by atomics
    static const int dw_min_it = FFH_LAB_INT("FFH_SK_DW_MIN_IT", 8);       // A/B switch
    if (ntiles * nk < (int64_t)dw_min_it * p.G) return false;      // at least eight k-tiles per workgroup (with four the split-K kernels of linear.hip win:
                                                                   // 8192 x 512 -> 256: 32.3 vs 37.0 us; with eight this one does: 4096 x 1024 -> 512: 48.7 vs 52.5)
  } else {
    if (g.epi != EPI_STORE && g.epi != EPI_ADD) return false;
    // whole tiles when they fill whole rounds of workgroups (or nearly: a split costs a partial tile's round trip through memory);
    // otherwise stream-K with the fix-up of the kernel's SPLIT form when every workgroup still gets >= 8 k-tiles
    static const int no_split = FFH_LAB_INT("FFH_SK_NO_SPLIT", 0);     // A/B switch (tools/ab.sh)
    const int64_t rounds = (ntiles + p.G - 1) / p.G;
    const int64_t idle_it = (rounds * p.G - ntiles) * nk / p.G;      // k-tile iterations per workgroup the last round wastes
    // less than one round of 128-row tiles, one (nearly) full round of 64-row tiles: those, whole, with the full reduction each
    // (1024 -> 512 forward at 4096 samples: 128 tiles / 256)
    static const int no_t64 = FFH_LAB_INT("FFH_SK_NO_T64", 0);        // A/B switch
    p.tmw = 4;
    if (!no_t64 && ntiles < p.G && g.M % 64 == 0 && (g.epi == EPI_STORE || g.epi == EPI_ADD) && nk >= 8) {
      const int64_t nt64 = (int64_t)(g.M / 64) * (g.N / SK_BN);
      if (nt64 <= p.G && nt64 * 100 >= (int64_t)p.G * 80) { p.tmw = 2; p.split = false; return true; }
    }
    p.split = !no_split && idle_it >= 2 && ntiles * nk >= 8LL * p.G && g.epi == EPI_STORE;    // (four k-tiles per workgroup: 8192 x 512 -> 256 forward 33.3 us split, 27.8 on the LDS-DMA kernel)
    if (!p.split) {
      if (ntiles < p.G) return false;
      if (ntiles * 100 < rounds * p.G * 80) return false;          // whole tiles only: the last round must be nearly full
    }
  }
  return true;
}

// the partial-tile slots of the SPLIT form for launches on stream s: ctx-owned scratch reserved by ffh_ctx_reserve_scratch(ctx, s)
// (runtime.hip) -- a compute entry point never allocates.  No set for this stream: the form is not offered.
bool sk_slots_for(ffh_ctx* c, hipStream_t s, float** slots, unsigned** cnt) {
  for (int i = 0; i < c->nscratch; i++)
    if (c->scratch[i].stream == (void*)s && c->scratch[i].sk_slots) { *slots = c->scratch[i].sk_slots; *cnt = c->scratch[i].sk_cnt; return true; }
  return false;
}
}  // namespace

bool gemm_sk_serves(const ffh_ctx* c, const GemmArgs& g, int form) { SkPlan p; return sk_plan(c, g, form, p); }

// 1: launched; 0: not this kernel's shape (nothing launched); < 0: error
int launch_gemm_sk(ffh_ctx* c, const GemmArgs& g, int form, ffh_stream s, const char* name) {
  SkPlan p{};
  if (!sk_plan(c, g, form, p)) return 0;
  float* slots = nullptr; unsigned* flags = nullptr;
  if (p.split && !sk_slots_for(c, as_stream(s), &slots, &flags)) {
    // no scratch reserved for this stream (ffh_ctx_reserve_scratch): the whole-tile form where it serves, else not this kernel's launch --
    // said in the route, so that a caller who launches on a stream of its own sees why a slower form ran
    p.split = false;
    { char tok[96]; snprintf(tok, sizeof tok, "%s|no_scratch_on_this_stream", name); ffh_route_add(c, tok); }
    const int64_t ntiles = (int64_t)(g.M / SK_BM) * (g.N / SK_BN), rounds = (ntiles + p.G - 1) / p.G;
    if (ntiles < p.G || ntiles * 100 < rounds * p.G * 80) return 0;
  }
  const int64_t lda = p.lda, ldb = p.ldb, a_bytes = p.a_bytes, b_bytes = p.b_bytes;
  const int G = p.G;
  SkArgs a{};
  a.A = g.A; a.B = g.B; a.C = g.C; a.bias = g.bias; a.mask = g.mask; a.db = g.db; a.colmap = g.colmap; a.colsum = (form == SK_FORM_DX && g.epi == EPI_STORE && !g.colmap) ? g.colsum : nullptr;
  a.lda = lda; a.ldb = ldb; a.ldc = g.ldc; a.ldmask = g.ldmask;
  a.M = g.M; a.N = g.N; a.K = g.K; a.act = g.act;
  a.a_bytes = (unsigned)a_bytes; a.b_bytes = (unsigned)b_bytes;
  a.bias_bytes = g.bias ? (unsigned)g.N * 4u : 0u;
  a.mask_bytes = g.mask ? 1u : 0u;
  if (p.split) { a.sk_slots = slots; a.sk_cnt = flags; }
  // The kernels need more than 64 KB of dynamic LDS; hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute of the
  // function, and one process may hold a ctx per device (ffh_ctx_default): set once per (kernel, device).  A launch that still
  // fails (attribute refused, no such resources) is not an error of the call: 0 = "not served", linear.hip's kernels take the layer.
#define FFH_SK_LAUNCH(AKR, BKR, EPI, LDSB, ...)                                                                  \
  {                                                                                                              \
    auto kern = gemm_sk_kernel<AKR, BKR, EPI, ##__VA_ARGS__>;                                                    \
    static std::atomic<signed char> ok[64];      /* 0: not tried on this device, 1: set, -1: refused */          \
    const int dev = c->device & 63;                                                                              \
    if (ok[dev].load(std::memory_order_acquire) == 0) ok[dev].store(sk_set_lds(kern, LDSB) ? 1 : -1, std::memory_order_release); \
    if (ok[dev].load(std::memory_order_acquire) < 0) return 0;                                                   \
    hipLaunchKernelGGL(kern, dim3((unsigned)G), dim3(256), LDSB, as_stream(s), a);                               \
  }
  constexpr int BCW = 64;      // SPLIT: the arrival broadcast word behind the operand images
  constexpr int KC64 = sk_lds_kc_a(2);
  if (form == SK_FORM_FWD && p.tmw == 2) FFH_SK_LAUNCH(false, false, SK_EPI_FWD, KC64 + SK_LDS_KC, false, false, 2)
  else if (form == SK_FORM_DX && p.tmw == 2 && g.colmap) FFH_SK_LAUNCH(false, true, SK_EPI_DX_CMAP, KC64 + SK_LDS_KR, false, false, 2)
  else if (form == SK_FORM_DX && p.tmw == 2 && g.epi == EPI_STORE) FFH_SK_LAUNCH(false, true, SK_EPI_DX_STORE, KC64 + SK_LDS_KR, false, false, 2)
  else if (form == SK_FORM_DX && p.tmw == 2) FFH_SK_LAUNCH(false, true, SK_EPI_DX_ADD, KC64 + SK_LDS_KR, false, false, 2)
  else if (form == SK_FORM_FWD && p.split) FFH_SK_LAUNCH(false, false, SK_EPI_FWD, 2 * SK_LDS_KC + BCW, false, true)
  else if (form == SK_FORM_DX && p.split && g.colmap) FFH_SK_LAUNCH(false, true, SK_EPI_DX_CMAP, SK_LDS_KC + SK_LDS_KR + BCW, false, true)
  else if (form == SK_FORM_DX && p.split) FFH_SK_LAUNCH(false, true, SK_EPI_DX_STORE, SK_LDS_KC + SK_LDS_KR + BCW, false, true)
  else if (form == SK_FORM_FWD) FFH_SK_LAUNCH(false, false, SK_EPI_FWD, 2 * SK_LDS_KC)
  else if (form == SK_FORM_DW && g.db) FFH_SK_LAUNCH(true, true, SK_EPI_DW_ATOMIC, 2 * SK_LDS_KR + 4 * SK_EP_WAVE, true)
  else if (form == SK_FORM_DW) FFH_SK_LAUNCH(true, true, SK_EPI_DW_ATOMIC, 2 * SK_LDS_KR + 4 * SK_EP_WAVE)
  else if (g.colmap) FFH_SK_LAUNCH(false, true, SK_EPI_DX_CMAP, SK_LDS_KC + SK_LDS_KR)
  else if (g.epi == EPI_STORE) FFH_SK_LAUNCH(false, true, SK_EPI_DX_STORE, SK_LDS_KC + SK_LDS_KR)
  else FFH_SK_LAUNCH(false, true, SK_EPI_DX_ADD, SK_LDS_KC + SK_LDS_KR)
#undef FFH_SK_LAUNCH
  {
    // a launch the device refuses for its CONFIGURATION enqueued nothing: "not served", the caller falls through to linear.hip.  Anything
    // else (a sticky fault of earlier work surfacing here) is the caller's to see
    const hipError_t e = hipGetLastError();
    if (e == hipErrorInvalidValue || e == hipErrorInvalidConfiguration || e == hipErrorLaunchOutOfResources || e == hipErrorSharedObjectInitFailed) return 0;
    if (e != hipSuccess) return ffh_fail_hip(c, e, name);
  }
  { char tok[96]; snprintf(tok, sizeof tok, "%s|sk_%dx128x64%s%s%s|wgs=%d", name, 32 * p.tmw, g.colmap ? "|colmap" : "", p.split ? "|streamk" : "", a.colsum ? "|colsum" : "", G); ffh_route_add(c, tok); }
  return 1;
}

bool gemm_sk_fold_plan(const ffh_ctx* c, const GemmArgs& g, int nk_kept, SkFoldPlan& fp) {
  if (g.K % SK_BK || g.K > 128 * SK_BK || nk_kept < 1 || nk_kept > g.K / SK_BK) return false;
  GemmArgs gk = g;
  gk.K = nk_kept * SK_BK;
  SkPlan p{};
  if (!sk_plan(c, gk, SK_FORM_FWD, p) || p.split || p.tmw != 4) return false;
  fp.lda = p.lda; fp.ldb = p.ldb; fp.G = p.G;
  fp.a_bytes = ((int64_t)(g.M - 1) * p.lda + g.K) * 4; fp.b_bytes = ((int64_t)(g.N - 1) * p.ldb + g.K) * 4;      // the operands over the whole depth: the kept k-tiles lie anywhere in it
  return fp.a_bytes < (1LL << 32) && fp.b_bytes < (1LL << 32);
}

// The forward form over kept k-tiles (+ addend): g describes the WHOLE layer (K = in_dim); keep / nk_kept as in SkArgsFold.  Served where the
// plain forward of a layer of depth 64 nk_kept would run whole tiles on 128-row tiles.  dry: decide only.  1: launched (dry: would be),
// 0: not this kernel's shape (nothing launched), < 0: error
int launch_gemm_sk_fold(ffh_ctx* c, const GemmArgs& g, const unsigned long long keep[2], int nk_kept, const float* addend, int64_t ldadd, bool dry,
                        ffh_stream s, const char* name) {
  if (addend && !sk_aligned(addend, ldadd)) return 0;
  SkFoldPlan p{};
  if (!gemm_sk_fold_plan(c, g, nk_kept, p)) return 0;
  if (dry) return 1;
  SkArgsFold a{};
  a.A = g.A; a.B = g.B; a.C = g.C; a.bias = g.bias;
  a.lda = p.lda; a.ldb = p.ldb; a.ldc = g.ldc;
  a.M = g.M; a.N = g.N; a.K = g.K; a.act = g.act;
  a.a_bytes = (unsigned)p.a_bytes; a.b_bytes = (unsigned)p.b_bytes;
  a.bias_bytes = g.bias ? (unsigned)g.N * 4u : 0u;
  a.keep[0] = keep[0]; a.keep[1] = keep[1]; a.nk_kept = (unsigned)nk_kept; a.addend = addend; a.ldadd = ldadd;
  {
    auto kern = gemm_sk_kernel<false, false, SK_EPI_FWD, false, false, 4, true>;
    constexpr int LDSB = 2 * SK_LDS_KC;
    static std::atomic<signed char> ok[64];      // as in launch_gemm_sk: the LDS attribute once per (kernel, device)
    const int dev = c->device & 63;
    if (ok[dev].load(std::memory_order_acquire) == 0) ok[dev].store(sk_set_lds(kern, LDSB) ? 1 : -1, std::memory_order_release);
    if (ok[dev].load(std::memory_order_acquire) < 0) return 0;
    hipLaunchKernelGGL(kern, dim3((unsigned)p.G), dim3(256), LDSB, as_stream(s), a);
    const hipError_t e = hipGetLastError();
    if (e == hipErrorInvalidValue || e == hipErrorInvalidConfiguration || e == hipErrorLaunchOutOfResources || e == hipErrorSharedObjectInitFailed) return 0;
    if (e != hipSuccess) return ffh_fail_hip(c, e, name);
  }
  { char tok[96]; snprintf(tok, sizeof tok, "%s|sk_128x128x64|kept=%d/%d%s|wgs=%d", name, nk_kept, g.K / SK_BK, addend ? "|addend" : "", p.G); ffh_route_add(c, tok); }
  return 1;
}

// The weight-gradient form over kept 128-column tiles of dW (include/ff_hip_fold.h): g describes the WHOLE layer's weight gradient (M = out_dim,
// N = in_dim, K = batch, db as launch_gemm_sk takes it); tiles: nkept ascending indices below N / 128.  Served where the stream-K weight gradient
// of a layer of nkept column tiles would run (sk_plan: nkept tiles * nk >= 8 workgroups' worth, not in deterministic mode).  dry: decide only.
// 1: launched (dry: would be), 0: not this kernel's shape (nothing launched), < 0: error
int launch_gemm_sk_kept(ffh_ctx* c, const GemmArgs& g, const int* tiles, int nkept, bool dry, ffh_stream s, const char* name) {
  if (g.N % SK_BN || g.N / SK_BN > 128 || nkept < 1 || nkept > g.N / SK_BN) return 0;
  for (int i = 0; i < nkept; i++)
    if (tiles[i] < 0 || tiles[i] >= g.N / SK_BN || (i > 0 && tiles[i] <= tiles[i - 1])) return 0;
  if (g.db && tiles[0] != 0) return 0;            // the bias gradient rides on the column tiles at n0 == 0
  GemmArgs gk = g;
  gk.N = nkept * SK_BN;
  SkPlan p{};
  if (!sk_plan(c, gk, SK_FORM_DW, p)) return 0;
  const int64_t b_bytes = ((int64_t)(g.K - 1) * p.ldb + g.N) * 4;      // x over the whole width: the kept tiles lie anywhere in it
  if (b_bytes >= (1LL << 32)) return 0;
  if (dry) return 1;
  SkArgsKept a{};
  a.A = g.A; a.B = g.B; a.C = g.C; a.db = g.db;
  a.lda = p.lda; a.ldb = p.ldb; a.ldc = g.ldc;
  a.M = g.M; a.N = g.N; a.K = g.K; a.act = g.act;
  a.a_bytes = (unsigned)p.a_bytes; a.b_bytes = (unsigned)b_bytes;
  a.nkept = (unsigned)nkept;
  for (int i = 0; i < nkept; i++) a.tile[i] = (unsigned short)tiles[i];
  constexpr int LDSB = 2 * SK_LDS_KR + 4 * SK_EP_WAVE;
#define FFH_SK_KEPT_LAUNCH(DBV)                                                                                  \
  {                                                                                                              \
    auto kern = gemm_sk_kernel<true, true, SK_EPI_DW_ATOMIC, DBV, false, 4, false, true>;                        \
    static std::atomic<signed char> ok[64];      /* as in launch_gemm_sk: the LDS attribute once per (kernel, device) */ \
    const int dev = c->device & 63;                                                                              \
    if (ok[dev].load(std::memory_order_acquire) == 0) ok[dev].store(sk_set_lds(kern, LDSB) ? 1 : -1, std::memory_order_release); \
    if (ok[dev].load(std::memory_order_acquire) < 0) return 0;                                                   \
    hipLaunchKernelGGL(kern, dim3((unsigned)p.G), dim3(256), LDSB, as_stream(s), a);                             \
  }
  if (g.db) FFH_SK_KEPT_LAUNCH(true)
  else FFH_SK_KEPT_LAUNCH(false)
#undef FFH_SK_KEPT_LAUNCH
  {
    const hipError_t e = hipGetLastError();
    if (e == hipErrorInvalidValue || e == hipErrorInvalidConfiguration || e == hipErrorLaunchOutOfResources || e == hipErrorSharedObjectInitFailed) return 0;
    if (e != hipSuccess) return ffh_fail_hip(c, e, name);
  }
  { char tok[96]; snprintf(tok, sizeof tok, "%s|sk_128x128x64|kept=%d/%d%s|wgs=%d", name, nkept, g.N / SK_BN, g.db ? "|db" : "", p.G); ffh_route_add(c, tok); }
  return 1;
}

// The data-gradient form over kept 128-column tiles of dX (include/ff_hip_fold.h): g describes the WHOLE layer's data gradient (M = batch, N = in_dim,
// K = out_dim, epi, mask as launch_gemm_sk takes them; g.colsum is ignored: `colsum` is this call's own argument, [in_dim], store epilogue only).
// Served where the whole layer runs whole 128-row tiles (sk_plan: not the stream-K split, not the 64-row tiles) and the kept tiles still fill whole
// rounds of workgroups by the rule sk_plan holds whole tiles to (at least one round, the last one 80 % full); never in deterministic mode (colsum
// meets by atomics; the host keeps that mode on the plain call).  dry: decide only.  1: launched (dry: would be), 0: not served (nothing launched), < 0: error
int launch_gemm_sk_kept_dx(ffh_ctx* c, const GemmArgs& g, const int* tiles, int nkept, float* colsum, bool dry, ffh_stream s, const char* name) {
  if (g.N % SK_BN || g.N / SK_BN > 128 || nkept < 1 || nkept > g.N / SK_BN) return 0;
  for (int i = 0; i < nkept; i++)
    if (tiles[i] < 0 || tiles[i] >= g.N / SK_BN || (i > 0 && tiles[i] <= tiles[i - 1])) return 0;
  if (colsum && (tiles[0] != 0 || g.epi != EPI_STORE)) return 0;      // the bias gradient of the layer below rides on the column tile at n0 == 0
  if (c->deterministic || g.colmap) return 0;
  SkPlan p{};
  if (!sk_plan(c, g, SK_FORM_DX, p) || p.split || p.tmw != 4) return 0;
  const int64_t ntk = (int64_t)(g.M / SK_BM) * nkept, rounds = (ntk + p.G - 1) / p.G;
  if (ntk < p.G || ntk * 100 < rounds * p.G * 80) return 0;
  if (dry) return 1;
  SkArgsKept a{};
  a.A = g.A; a.B = g.B; a.C = g.C; a.mask = g.mask; a.colsum = colsum;
  a.lda = p.lda; a.ldb = p.ldb; a.ldc = g.ldc; a.ldmask = g.ldmask;
  a.M = g.M; a.N = g.N; a.K = g.K; a.act = g.act;
  a.a_bytes = (unsigned)p.a_bytes; a.b_bytes = (unsigned)p.b_bytes;      // w over the whole width: the kept tiles lie anywhere in it
  a.mask_bytes = g.mask ? 1u : 0u;
  a.nkept = (unsigned)nkept;
  for (int i = 0; i < nkept; i++) a.tile[i] = (unsigned short)tiles[i];
  constexpr int LDSB = SK_LDS_KC + SK_LDS_KR;
#define FFH_SK_KEPT_DX_LAUNCH(EPI)                                                                               \
  {                                                                                                              \
    auto kern = gemm_sk_kernel<false, true, EPI, false, false, 4, false, true>;                                  \
    static std::atomic<signed char> ok[64];      /* as in launch_gemm_sk: the LDS attribute once per (kernel, device) */ \
    const int dev = c->device & 63;                                                                              \
    if (ok[dev].load(std::memory_order_acquire) == 0) ok[dev].store(sk_set_lds(kern, LDSB) ? 1 : -1, std::memory_order_release); \
    if (ok[dev].load(std::memory_order_acquire) < 0) return 0;                                                   \
    hipLaunchKernelGGL(kern, dim3((unsigned)p.G), dim3(256), LDSB, as_stream(s), a);                             \
  }
  if (g.epi == EPI_STORE) FFH_SK_KEPT_DX_LAUNCH(SK_EPI_DX_STORE)
  else FFH_SK_KEPT_DX_LAUNCH(SK_EPI_DX_ADD)
#undef FFH_SK_KEPT_DX_LAUNCH
  {
    const hipError_t e = hipGetLastError();
    if (e == hipErrorInvalidValue || e == hipErrorInvalidConfiguration || e == hipErrorLaunchOutOfResources || e == hipErrorSharedObjectInitFailed) return 0;
    if (e != hipSuccess) return ffh_fail_hip(c, e, name);
  }
  { char tok[96]; snprintf(tok, sizeof tok, "%s|sk_128x128x64|kept=%d/%d%s|wgs=%d", name, nkept, g.N / SK_BN, colsum ? "|colsum" : "", p.G); ffh_route_add(c, tok); }
  return 1;
}

}  // namespace ffh_gemm
