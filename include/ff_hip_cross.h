/* ff_hip_cross.h -- optional extension of the kernel C-ABI (include/ff_hip.h): the elementwise combine of the DCNv2 low-rank cross
 * network (torchrec's LowRankCrossNet, the interaction of MLPerf DLRM-DCNv2).
 *
 * A library may export this list or not; include/ff_hip.h and its symbol list are unchanged by it.  libffhip.so exports it,
 * the CPU oracle does not.  Callers load it separately (host/backend: KernelApi::cross, null when absent; capi.cross_api(lib)).
 *
 * One cross layer is   u = V x_l,   v = W u + b,   x_{l+1} = x_0 (.) v + x_l.   The two products are ordinary Linear layers
 * (ffh_linear_*); the third line and its backward are the two entries below: memory-bound passes over [batch][dim] operands that each
 * carry a row stride of their own (tensors of the host layer have pad columns, and slices of a wider buffer).
 *
 * CONTRACT (fmul_rn / fadd_rn: the IEEE-754 binary32 product / sum, rounded to nearest even, subnormals kept, each rounded on its
 * own -- never contracted into a fused multiply-add; a float32 numpy expression computes the same bits, NaN payloads aside)
 *   ffh_cross_fwd    y[i][j]  = fadd_rn(fmul_rn(x0[i][j], v[i][j]), xl[i][j])                  i in [0, batch), j in [0, dim)
 *   ffh_cross_bwd    dv[i][j] = fmul_rn(dy[i][j], x0[i][j])                                     always stored
 *                    g0       = fmul_rn(dy[i][j], v[i][j])
 *                    dx0[i][j] = g0 (FFH_CROSS_STORE) | fadd_rn(dx0[i][j], g0) (FFH_CROSS_ADD) | untouched (FFH_CROSS_SKIP)
 *                    dxl[i][j] = dy[i][j] (STORE)     | fadd_rn(dxl[i][j], dy[i][j]) (ADD)     | untouched (SKIP)
 *                    dx0 == dxl (layer 0, where x_l IS x_0): ONE write under mode_x0,  g = fadd_rn(g0, dy[i][j]),
 *                    dx0[i][j] = g (STORE) | fadd_rn(dx0[i][j], g) (ADD); mode_xl must equal mode_x0 and neither may be SKIP,
 *                    else FFH_ERR_BAD_ARG.
 *   Aliasing: the inputs of one call may be the same buffer (x0 == xl in the forward of layer 0).  A destination may not overlap an
 *   input or another destination, except dx0 == dxl as stated; dx0 and dxl that overlap without being equal are the caller's error.
 *   A SKIP destination may be NULL.  Nothing outside the [batch][dim] elements of a destination is written (pad columns and rows
 *   behind `batch` stay as they are), nothing outside those elements of an input is read.
 *   Requires batch >= 0, dim >= 1, every ld >= dim, 4-byte aligned pointers; batch == 0 launches nothing.
 *   A launch moves 16 bytes per lane when dim, every ld and every base address are multiples of 16 bytes, and 4 bytes per lane
 *   otherwise: one choice for the whole launch.  No atomics (results are bit-identical from run to run), no allocation, no
 *   environment variable; one launch on the caller's stream, with arguments that do not change from step to step (capturable).
 *   Bytes moved: forward 16 batch dim; backward (12 + 8 [dx0 not SKIP] + 4 [dx0 ADD] + 4 [dxl not SKIP] + 4 [dxl ADD]) batch dim,
 *   with dx0 == dxl counted once under mode_x0: 12 ... 32 batch dim.
 */
#ifndef FF_HIP_CROSS_H_
#define FF_HIP_CROSS_H_

#include "ff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_CROSS_ABI_VERSION 1

#define FFH_CROSS_SKIP  0
#define FFH_CROSS_STORE 1
#define FFH_CROSS_ADD   2

int ffh_cross_abi_version(void);

int ffh_cross_fwd(ffh_ctx* ctx, float* y, int64_t ldy, const float* x0, int64_t ldx0, const float* v, int64_t ldv, const float* xl, int64_t ldxl,
                  int64_t batch, int64_t dim, ffh_stream stream);

int ffh_cross_bwd(ffh_ctx* ctx, const float* dy, int64_t lddy, const float* x0, int64_t ldx0, const float* v, int64_t ldv, float* dv, int64_t lddv,
                  float* dx0, int64_t lddx0, int mode_x0, float* dxl, int64_t lddxl, int mode_xl, int64_t batch, int64_t dim, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_CROSS_API_LIST(X) \
  X(ffh_cross_abi_version) X(ffh_cross_fwd) X(ffh_cross_bwd)

#endif /* FF_HIP_CROSS_H_ */
