/* ffh_q8_linear.h -- optional extension of the kernel C-ABI (include/ff_hip.h): Linear layers on the int8 matrix pipe for held-out evaluation
 * (csrc/linear_q8.hip; --eval-mlp-dtype int8, the counterpart of Facebook DLRM's --quantize-mlp-with-bit 8).
 *
 * A library may export this list or not; include/ff_hip.h and its symbol list are unchanged by it.  libffhip.so exports it, the CPU oracle does
 * not.  Callers load it separately (host/backend: KernelApi::q8_linear, null when absent; capi.q8_linear_api(lib)).  The header is named
 * ffh_q8_linear.h and capi defines no Q8_LINEAR_HEADER_PATH (callers use capi.EXTENSIONS["q8_linear"].header_path), for the reason
 * include/ffh_dot_wide.h gives.
 *
 * THE RULE -- fp32 where it is not integer, every fp32 operation rounded on its own (no fused multiply-add).  For a row v of length K (a weight
 * row W[o][:] or an activation row x[b][:]):
 *     a     = max_k |v[k]|
 *     scale = a / 127.0f
 *     inv   = a > 0 ? 127.0f / a : 0.0f
 *     q[k]  = (int8) rint(v[k] * inv)            round half to even; in [-127, 127]
 * Symmetric; per output channel for weights, per sample (dynamic) for activations.  A row of zeros has scale 0 and codes 0.
 *     acc[b][o] = sum_k qx[b][k] * qw[o][k]      int32, exact: |acc| <= 127^2 K < 2^31 for K <= FFH_Q8_LINEAR_MAX_IN
 *     y[b][o]   = act((float)acc * (sx[b] * sw[o]) + bias[o])
 * (float)acc is round-to-nearest-even; the scale product first, then the multiply, then the add; act as ffh_linear_fwd takes it (FFH_AC_MODE_NONE,
 * _RELU, _SIGMOID = 1 / (1 + expf(-v)), _GELU in the tanh form).  Non-finite input is outside the contract.
 * dlrm_flexflow_amd.ffmodel.q8_linear_quantize_reference / q8_linear_reference restate the rule in numpy.
 *
 * THE IMAGE -- int8 codes [rows][ldq], ldq = ffh_q8_linear_ldq(in_dim) = in_dim rounded up to FFH_Q8_LINEAR_KSTEP (64): the quantizers write
 * zero codes into the columns in_dim .. ldq, so the GEMM's main loop has no tail.  An image starts 16-byte aligned.
 *
 * ENTRIES.  A bad argument (a null pointer where one is needed, a negative count, a leading dimension below the width, an image that is not
 * 16-byte aligned, in_dim > FFH_Q8_LINEAR_MAX_IN, an unknown activation) is FFH_ERR_BAD_ARG: nothing is launched, nothing is written.
 * A count of 0 rows is FFH_OK.  No allocation, no environment variable, no atomics, no split of K: one launch on the caller's stream with
 * arguments that do not change from call to call (capturable), results bit-identical from run to run and independent of the grid.
 *   ffh_q8_linear_quantize_weights   every matrix of the list in ONE grid-capped (ffh_q8_linear_quantize_max_workgroups()), grid-stride launch:
 *                                    src [rows][in_dim] floats with leading dimension ld >= in_dim  ->  codes [rows][ldq], scales [rows].
 *                                    1 <= nlayers <= FFH_Q8_LINEAR_MAX_LAYERS.  A lane group (a power of two of lanes, 16 columns per lane and
 *                                    trip) owns a row; its absmax is a butterfly over the group.
 *   ffh_q8_linear_quantize_rows      the same kernel on one matrix: the activations x [batch][in_dim], ldx >= in_dim -> xq [batch][ldq], sx [batch].
 *   ffh_q8_linear_fwd                y [batch][out_dim] floats, ldy >= out_dim, from the two images and their scales; bias may be null.  Any
 *                                    batch >= 1, in_dim >= 1, out_dim >= 1; edge tiles are masked in the epilogue only (the loads of rows past
 *                                    the edge are clamped to the last row).  16-byte stores where ldy % 4 == 0 and y is 16-byte aligned, dword
 *                                    stores otherwise.  Nothing outside y[b][0 .. out_dim) is written.
 *     TILES: a 4-wave workgroup owns 128 x 128 of y where that gives at least FFH_Q8_LINEAR_BIG_TILES workgroups
 *            (ceil(batch / 128) * ceil(out_dim / 128)), else 64 x 64: a choice by shape alone.
 */
#ifndef FFH_Q8_LINEAR_H_
#define FFH_Q8_LINEAR_H_

#include "ff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_Q8_LINEAR_ABI_VERSION 1

#define FFH_Q8_LINEAR_MIN_DIM 64         /* the host layer gives a Linear an image where in_channels and out_channels are at least this */
#define FFH_Q8_LINEAR_KSTEP 64           /* bytes of a row per step of the GEMM's main loop: the image's K is padded to a multiple of it */
#define FFH_Q8_LINEAR_MAX_IN 133144      /* 127 * 127 * 133144 = 2147479576 < 2^31 */
#define FFH_Q8_LINEAR_MAX_LAYERS 32      /* matrices of one ffh_q8_linear_quantize_weights call */
#define FFH_Q8_LINEAR_BIG_TILES 256      /* 128 x 128 tiles from this many workgroups on */

typedef struct ffh_q8_linear_rows {
  const float* src;      /* [rows][in_dim], leading dimension ld */
  int64_t ld;
  int8_t* codes;         /* [rows][ffh_q8_linear_ldq(in_dim)] */
  float* scales;         /* [rows] */
  int64_t rows;
  int32_t in_dim;
  int32_t reserved_;
} ffh_q8_linear_rows;

int     ffh_q8_linear_abi_version(void);
int64_t ffh_q8_linear_ldq(int in_dim);                       /* 0 for in_dim < 1 or > FFH_Q8_LINEAR_MAX_IN */
int     ffh_q8_linear_quantize_max_workgroups(void);          /* the quantizers' grid cap */

int ffh_q8_linear_quantize_weights(ffh_ctx* ctx, const ffh_q8_linear_rows* layers, int nlayers, ffh_stream stream);

int ffh_q8_linear_quantize_rows(ffh_ctx* ctx, const float* x, int64_t ldx, int8_t* xq, float* sx, int64_t batch, int in_dim, ffh_stream stream);

int ffh_q8_linear_fwd(ffh_ctx* ctx, const int8_t* xq, const int8_t* wq, const float* sx, const float* sw, const float* bias, float* y, int64_t ldy,
                      int64_t batch, int in_dim, int out_dim, int activation, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_Q8_LINEAR_API_LIST(X) \
  X(ffh_q8_linear_abi_version) X(ffh_q8_linear_ldq) X(ffh_q8_linear_quantize_max_workgroups) X(ffh_q8_linear_quantize_weights) \
  X(ffh_q8_linear_quantize_rows) X(ffh_q8_linear_fwd)

#endif /* FFH_Q8_LINEAR_H_ */
