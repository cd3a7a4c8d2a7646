// linear_sk_gather.hip -- the GATHER form of the persistent fp32 GEMM kernel (linear_sk_kernel.h): the first top layer's forward over the kept k-tiles
// with the folded tables' share gathered in the epilogue (include/ffh_fused_gather.h, ffh_fused_gather_linear_fwd).  A translation unit of its own: built
// without the packed fp32 instructions (build.py), which the other instantiations' listing must not notice.
#include "linear_sk_kernel.h"

namespace ffh_gemm {

// g describes the WHOLE layer (K = in_dim); keep / nk_kept as in SkArgsFold.  Served where launch_gemm_sk_fold serves the layer.  dry: decide only.
// 1: launched (dry: would be), 0: not this kernel's shape (nothing launched), < 0: error
int launch_gemm_sk_fold_gather(ffh_ctx* c, const GemmArgs& g, const unsigned long long keep[2], int nk_kept, const FoldGatherList& gl, bool dry, ffh_stream s,
                               const char* name) {
  if (gl.ntables < 1 || gl.ntables > FFH_FUSED_GATHER_MAX_TABLES || gl.L < 1 || gl.L > FFH_FUSED_GATHER_MAX_BAG || gl.ntables * gl.L > FFH_FUSED_GATHER_MAX_TERMS) return 0;
  if (gl.ldp % 4) return 0;
  for (int t = 0; t < gl.ntables; t++)
    if (!gl.idx[t] || !gl.p[t] || ((uintptr_t)gl.p[t] & 15)) return 0;
  SkFoldPlan p{};
  if (!gemm_sk_fold_plan(c, g, nk_kept, p)) return 0;
  if (dry) return 1;
  SkArgsGather a{};
  a.A = g.A; a.B = g.B; a.C = g.C; a.bias = g.bias;
  a.lda = p.lda; a.ldb = p.ldb; a.ldc = g.ldc;
  a.M = g.M; a.N = g.N; a.K = g.K; a.act = g.act;
  a.a_bytes = (unsigned)p.a_bytes; a.b_bytes = (unsigned)p.b_bytes;
  a.bias_bytes = g.bias ? (unsigned)g.N * 4u : 0u;
  a.keep[0] = keep[0]; a.keep[1] = keep[1]; a.nk_kept = (unsigned)nk_kept;
  a.gl = gl;
  {
    auto kern = gemm_sk_kernel<false, false, SK_EPI_FWD, false, false, 4, true, false, true>;
    constexpr int LDS_MAX = 2 * SK_LDS_KC + 2 * FFH_FUSED_GATHER_MAX_TERMS * 128 * 8;      // the operand images + two images of a tile's ids
    static_assert(LDS_MAX <= 160 * 1024, "LDS of a gfx950 CU");
    const int ldsb = 2 * SK_LDS_KC + 2 * gl.ntables * gl.L * 128 * 8;
    static std::atomic<signed char> ok[64];      // as in launch_gemm_sk: the LDS attribute once per (kernel, device)
    const int dev = c->device & 63;
    if (ok[dev].load(std::memory_order_acquire) == 0) ok[dev].store(sk_set_lds(kern, LDS_MAX) ? 1 : -1, std::memory_order_release);
    if (ok[dev].load(std::memory_order_acquire) < 0) return 0;
    hipLaunchKernelGGL(kern, dim3((unsigned)p.G), dim3(256), ldsb, as_stream(s), a);
    const hipError_t e = hipGetLastError();
    if (e == hipErrorInvalidValue || e == hipErrorInvalidConfiguration || e == hipErrorLaunchOutOfResources || e == hipErrorSharedObjectInitFailed) return 0;
    if (e != hipSuccess) return ffh_fail_hip(c, e, name);
  }
  { char tok[112]; snprintf(tok, sizeof tok, "%s|sk_128x128x64|kept=%d/%d|gather=%dx%d|wgs=%d", name, nk_kept, g.K / SK_BK, gl.ntables, gl.L, p.G); ffh_route_add(c, tok); }
  return 1;
}

}  // namespace ffh_gemm
