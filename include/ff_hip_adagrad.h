/* ff_hip_adagrad.h -- optional extension of the kernel C-ABI (include/ff_hip.h): Adagrad with torch.optim.Adagrad's element-wise rule
 * (the optimizer of the MLPerf DLRM-DCNv2 recipe), as one dense launch and as a row rule of the fused sorted-segments table update.
 *
 * A library may export this list or not; include/ff_hip.h and its symbol list are unchanged by it.  libffhip.so exports it,
 * the CPU oracle does not.  Callers load it separately (host/backend: KernelApi::adagrad, null when absent; capi.adagrad_api(lib)).
 *
 * THE RULE, per element in fp32 (fmul_rn / fadd_rn / fsub_rn / fdiv_rn / fsqrt_rn: the IEEE-754 binary32 operation, correctly rounded to
 * nearest even, subnormals kept, each rounded on its own -- never contracted into a fused multiply-add; one float32 numpy operation per
 * line computes the same bits, ffmodel.adagrad_reference):
 *   gt = g                                    (weight_decay == 0)
 *   gt = fadd_rn(g, fmul_rn(wd, w))           (weight_decay != 0)
 *   S  = fadd_rn(S, fmul_rn(gt, gt))
 *   d  = fadd_rn(fsqrt_rn(S), eps)
 *   q  = fdiv_rn(gt, d)
 *   w  = fsub_rn(w, fmul_rn(lr, q))
 * No lr_decay.  S has the shape of w, is fp32 and starts at the caller's initial accumulator value.  With weight_decay == 0 an element
 * whose g is +0 keeps w and S bit for bit (S + 0 = S; q = 0 / d = 0 where d > 0; w - 0 = w, -0.0 included): updating only the rows a batch
 * touched IS the dense sweep.  d == 0 (S == 0 with eps <= 0) gives 0 / 0: the caller's error.
 *
 * DENSE
 *   ffh_adagrad_update      the rule over w[0 .. n), g, S with `lr` a launch argument
 *   ffh_adagrad_update_lr   the same with lr read from a learning-rate state block in device memory (include/ff_hip_lr.h): the step's
 *                           rate, the one plain SGD reads (ffh_lr_rate_ptr(block, false)); the launch arguments do not change from step
 *                           to step (capturable)
 *   flags: FFH_OPT_ZERO_GRAD (g is cleared behind its read) or 0; anything else FFH_ERR_BAD_ARG.  n == 0 launches nothing; null w, g or S
 *   with n > 0: FFH_ERR_BAD_ARG.  One launch: 16 bytes per lane where n % 4 == 0 and w, g, S are 16-byte aligned, else 4 bytes per lane.
 *   The bf16 twin / three-plane image of a mirrored weight range (ffh_ctx_bf16_mirror_set / ffh_ctx_bf16x3_mirror_set) is refreshed in the
 *   same launch in the 16-byte form, by a conversion launch behind it otherwise -- as ffh_sgd_update_ex and ffh_adam_update do.
 *   Bytes moved: 20 n (w, S read and written, g read), 24 n with FFH_OPT_ZERO_GRAD.
 *
 * SPARSE: ffh_sparse_opt.kind == FFH_SPARSE_OPT_ADAGRAD is accepted by the sorted-segments entry points of a library with this extension:
 *   ffh_embedding_bwd_opt_fused_multi / _apply_multi (ff_hip.h), their _bf16 forms (ff_hip_bf16.h), their _lr and _bf16_lr forms
 *   (ff_hip_lr.h).  g of a touched row is its canonical gradient sum (FFH_EMB_CHUNK order, unchanged); the rule above runs on the row.
 *   State: ffh_emb_state.s0 = S [num_entries][out_dim] fp32; s1 is unused.  A missing s0 returns FFH_ERR_BAD_ARG (nothing is launched).
 *   Read from ffh_sparse_opt: lr, epsilon, weight_decay (the _lr forms ignore lr and read the block's rate, as for FFH_SPARSE_OPT_SGD).
 *   bf16 tables: the row is widened exactly, the rule runs in fp32 on fp32 S, then the one rounding of the plain bf16 update follows
 *   (stochastic or nearest, same keys and counter).  One state pointer per table: up to FFH_MAX_TABLES tables per call
 *   (FFH_BF16_MAX_STATEFUL_TABLES does not apply).
 */
#ifndef FF_HIP_ADAGRAD_H_
#define FF_HIP_ADAGRAD_H_

#include "ff_hip.h"
#include "ff_hip_lr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_ADAGRAD_ABI_VERSION 1

#define FFH_SPARSE_OPT_ADAGRAD 3      /* ffh_sparse_opt.kind, beside FFH_SPARSE_OPT_SGD / _SGD_MOMENTUM / _ADAM */

int ffh_adagrad_abi_version(void);

int ffh_adagrad_update(ffh_ctx* ctx, float* w, float* w_grad, float* S, int64_t count, float lr, float eps, float weight_decay, int flags,
                       ffh_stream stream);

int ffh_adagrad_update_lr(ffh_ctx* ctx, float* w, float* w_grad, float* S, int64_t count, const ffh_lr_state* block, float eps,
                          float weight_decay, int flags, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_ADAGRAD_API_LIST(X) \
  X(ffh_adagrad_abi_version) X(ffh_adagrad_update) X(ffh_adagrad_update_lr)

#endif /* FF_HIP_ADAGRAD_H_ */
