/* ff_hip_ctr.h -- optional extension of the kernel C-ABI (include/ff_hip.h): the click-through-rate (CTR) loss and evaluation.
 *
 * A library may export this list or not; include/ff_hip.h and its symbol list are unchanged by it.  libffhip.so exports
 * it, the CPU oracle does not.  Callers load it separately (host/backend: KernelApi::ctr, null when absent;
 * capi.ctr_api(lib)).  The reference has neither this loss nor an AUC: the contract below is this build's own, pinned by
 * torch.nn.functional.binary_cross_entropy and float64 numpy in the tests.
 *
 * CONTRACT
 *   p      the output of a final Linear with FFH_AC_MODE_SIGMOID (a probability), y the label in [0, 1].
 *   loss   per element  -( y * max(log(p), -100) + (1 - y) * max(log(1 - p), -100) ).  The clamp at -100 is torch's
 *          binary_cross_entropy convention; it keeps p == 0 and p == 1 finite.
 *   dz     the gradient is taken with respect to the layer's PRE-ACTIVATION:  dz = (p - y) * scale, one subtraction and one
 *          multiplication in fp32 (no fused multiply-add), scale = 1 / global batch for the mean form.  The sigmoid derivative
 *          is never applied: p (1 - p) cancels against the derivative of the loss.  dz is stored where the MSE path stores dy,
 *          and the layer's own backward then runs as with FFH_LINEAR_DY_PREMASKED.
 *   sums   the log-loss sum accumulates as the MSE sum of ffh_metrics_update does: fp32 partial sums per lane and per
 *          workgroup, one floating-point atomic per workgroup (so its last bits depend on the launch geometry).  Every
 *          COUNT of this header is an integer added with integer atomics: bit-reproducible under any launch geometry.
 *   bins   bin(p) = min(FFH_AUC_BINS - 1, (int)(p * FFH_AUC_BINS)).  FFH_AUC_BINS is a power of two, so p * FFH_AUC_BINS is
 *          exact in fp32 and host code reproduces every bin.
 *   AUC    from the two histograms in float64 by the trapezoid rule, a tie inside a bin counted half (ffh_auc_from_histograms).
 *          It differs from the exact pair-counting AUC by at most 0.5 * sum_k pos[k] * neg[k] / (P * N).
 */
#ifndef FF_HIP_CTR_H_
#define FF_HIP_CTR_H_

#include <math.h>

#include "ff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_CTR_ABI_VERSION 1

#define FFH_AUC_BINS 65536

/* metrics_flags bit of the entries below, beside bit0 accuracy, bit1 mse, bit2 rmse, bit3 mae of ffh_metrics_update */
#define FFH_METRIC_BCE 16

/* Evaluation metrics accumulated on the device (zero it with ffh_zero to start an evaluation).  Predictions that are NaN
 * are counted in `nan_predictions` and left out of everything else.  64-bit counts: wide enough for 2^40 samples. */
typedef struct ffh_ctr_eval {
  uint64_t samples;          /* predictions that are not NaN                                  */
  uint64_t positives;        /* of those: y >= 0.5                                            */
  uint64_t correct;          /* of those: (p >= 0.5) == (y >= 0.5)                            */
  uint64_t nan_predictions;
  float    logloss_sum;      /* sum of the per-sample loss (fp32, see "sums" above)           */
  float    pad_[3];
  uint64_t hist_pos[FFH_AUC_BINS];   /* bin(p) of the samples with y >= 0.5 */
  uint64_t hist_neg[FFH_AUC_BINS];   /* ... of the rest                     */
} ffh_ctr_eval;

int ffh_ctr_abi_version(void);

/* The stand-alone loss step: logit_grad[b][i] = dz, and into `perf` the accuracy / MSE / RMSE / MAE sums selected by
 * metrics_flags exactly as ffh_metrics_update accumulates them (its accuracy rule and its double count of train_all
 * included); with FFH_METRIC_BCE the log-loss sum (over all elements) is added to *bce_sum (device memory; may be NULL
 * without that flag). */
int ffh_bce_bwd_metrics(ffh_ctx* ctx, float* logit_grad, const float* prob, const float* label, ffh_perf_metrics* perf,
                        float* bce_sum, int64_t num_samples, int num_classes, float scale, int metrics_flags, ffh_stream s);

/* The last layer's backward with the loss step folded in: exactly
 *   ffh_bce_bwd_metrics(ctx, dy, y, label, perf, bce_sum, batch, out_dim, scale, metrics_flags, s)
 *   ffh_linear_bwd_ex(ctx, x, ..., FFH_AC_MODE_SIGMOID, flags | FFH_LINEAR_DY_PREMASKED, s, NULL)
 * as one launch.  `act` must be FFH_AC_MODE_SIGMOID (FFH_ERR_BAD_ARG otherwise).  Served shapes, and the rule that
 * FFH_ERR_UNSUPPORTED means nothing was launched and no buffer was touched (the caller then makes the two calls), are
 * those of ffh_linear_bwd_mse; dy and dX equal the two calls' bit for bit, dW / db / the sums up to the order of atomics. */
int ffh_linear_bwd_bce(ffh_ctx* ctx, const float* x, int64_t ldx, float* dx, int64_t lddx,
                       const float* y, int64_t ldy, float* dy, int64_t lddy,
                       const float* w, float* dw, float* db, int in_dim, int out_dim, int64_t batch, int act, int flags,
                       const float* label, float scale, ffh_perf_metrics* perf, float* bce_sum, int metrics_flags, ffh_stream s);

/* Evaluation metrics of one batch, no gradient: accumulates prob[0 .. num_samples) / label[...] into *eval (device memory). */
int ffh_ctr_eval_update(ffh_ctx* ctx, const float* prob, const float* label, ffh_ctr_eval* eval, int64_t num_samples, ffh_stream s);

#ifdef __cplusplus
}
#endif

/* bin of a prediction (not NaN): host code and device code share this statement */
static inline int ffh_auc_bin(float p) {
  const float t = p * (float)FFH_AUC_BINS;
  if (!(t > 0.0f)) return 0;
  return t >= (float)FFH_AUC_BINS ? FFH_AUC_BINS - 1 : (int)t;
}

/* Host side, plain C: AUC = sum_k pos[k] * (neg_below[k] + 0.5 * neg[k]) / (P * N) in float64; NaN when P == 0 or N == 0. */
static inline double ffh_auc_from_histograms(const uint64_t* pos, const uint64_t* neg, int bins) {
  double P = 0.0, N = 0.0, below = 0.0, acc = 0.0;
  for (int k = 0; k < bins; k++) {
    acc += (double)pos[k] * (below + 0.5 * (double)neg[k]);
    below += (double)neg[k];
    P += (double)pos[k];
    N += (double)neg[k];
  }
  if (P == 0.0 || N == 0.0) return NAN;
  return acc / (P * N);
}

#define FFH_CTR_API_LIST(X) \
  X(ffh_ctr_abi_version) X(ffh_bce_bwd_metrics) X(ffh_linear_bwd_bce) X(ffh_ctr_eval_update)

#endif /* FF_HIP_CTR_H_ */
