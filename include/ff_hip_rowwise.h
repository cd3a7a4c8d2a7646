/* ff_hip_rowwise.h -- optional extension of the kernel C-ABI (include/ff_hip.h): row-wise Adagrad for embedding tables -- ONE fp32 accumulator per
 * table row, the running sum of the row's mean squared gradient (what fbgemm calls EXACT_ROWWISE_ADAGRAD) -- as a row rule of the fused
 * sorted-segments table update.  There is no dense launch: MLPs keep the element-wise rule of include/ff_hip_adagrad.h.
 *
 * A library may export this list or not; include/ff_hip.h, include/ff_hip_adagrad.h and their symbol lists are unchanged by it.  libffhip.so
 * exports it, the CPU oracle does not.  Callers load it separately (host/backend: KernelApi::rowwise, null when absent; capi.rowwise_api(lib)).
 *
 * THE RULE, per touched row of width D, in fp32 (fmul_rn / fadd_rn / fsub_rn / fdiv_rn / fsqrt_rn: the IEEE-754 binary32 operation, correctly
 * rounded to nearest even, subnormals kept, each rounded on its own -- never contracted into a fused multiply-add; one float32 numpy operation
 * per line computes the same bits, ffmodel.rowwise_adagrad_reference).  g[0 .. D) is the row's canonical gradient sum, S the row's one float:
 *   gt[j] = g[j]                                  (weight_decay == 0)
 *   gt[j] = fadd_rn(g[j], fmul_rn(wd, w[j]))      (weight_decay != 0)
 *   t[j]  = fmul_rn(gt[j], gt[j])
 *   sum   = TREE(t)                               (below)
 *   ms    = fdiv_rn(sum, (float)D)
 *   S     = fadd_rn(S, ms)
 *   d     = fadd_rn(fsqrt_rn(S), eps)
 *   q[j]  = fdiv_rn(gt[j], d)
 *   w[j]  = fsub_rn(w[j], fmul_rn(lr, q[j]))
 * The last five statements are those of the element-wise rule (ff_hip_adagrad.h) on purpose: at D == 1, TREE(t) = t[0] and t[0] / 1.0f = t[0],
 * so the two rules give the same bits.  At any D the rule differs from fbgemm's only in how lr / d is folded (fbgemm multiplies g by the one
 * quotient lr / d; here g is divided by d, then multiplied by lr, as torch.optim.Adagrad does): a few ulps of w per step.
 *
 * THE SUM ORDER.  TREE is one fixed order, so the result depends neither on how many columns a lane holds, nor on how rows are laid over the
 * lanes of a wave, nor on the route a call takes:
 *   pad t with +0 to the next power of two P >= D;  for stride = 1, 2, 4, ..., P / 2:  t'[i] = fadd_rn(t[2 i], t[2 i + 1]) on the halved array.
 * Level k adds the two subtrees whose column indices differ in bit k.  Every t[j] >= +0, so x + (+0) = x bit for bit at every level: the padding
 * (and any further padding, to a larger power of two) never changes a bit.  A NaN or infinite gradient makes S NaN / infinite, as in the
 * element-wise rule.
 *
 * UNTOUCHED ROWS.  With weight_decay == 0 a row whose g is all +0 keeps w and S bit for bit: t = +0, TREE = +0, ms = +0 / D = +0, S + 0 = S;
 * q = +0 / d = +0 where d > 0; w - lr * (+0) = w - (+0) = w for lr >= 0, -0.0 included.  Updating only the rows a batch touched therefore IS the
 * sweep over the whole table, for the reason given in ff_hip_adagrad.h for its elements.  d == 0 (S == 0 with eps <= 0) gives 0 / 0: the
 * caller's error.  With weight_decay != 0 the rows that were not touched are NOT decayed: the stated divergence of every touched-rows rule
 * (ffh_sparse_opt).
 *
 * ffh_sparse_opt.kind == FFH_SPARSE_OPT_ROWWISE_ADAGRAD is accepted by the sorted-segments entry points of a library with this extension:
 *   ffh_embedding_bwd_opt_fused_multi / _apply_multi (ff_hip.h), their _bf16 forms (ff_hip_bf16.h), their _lr and _bf16_lr forms (ff_hip_lr.h).
 *   Kinds 4 .. 7 and anything above 8 stay FFH_ERR_BAD_ARG.
 *   State: ffh_emb_state.s0 = S, float[num_entries]; s1 is unused.  A missing s0 returns FFH_ERR_BAD_ARG (nothing is launched).  s0 needs no
 *   16-byte alignment (it is read and written one float per row).
 *   Read from ffh_sparse_opt: lr, epsilon, weight_decay (the _lr forms ignore lr and read the block's rate, as for FFH_SPARSE_OPT_SGD).
 *   bf16 tables: the row is widened exactly, the rule runs in fp32, then the one rounding of the plain bf16 update follows (stochastic or
 *   nearest, same keys and counter).  One state pointer per table: up to FFH_MAX_TABLES tables per call (FFH_BF16_MAX_STATEFUL_TABLES does not
 *   apply).
 *   Width: a row's gradient and weights stay in registers between the sum and the update, at most four vectors per lane: out_dim <= 1024 in the
 *   16-byte form (out_dim % 4 == 0, aligned tables and gradients), <= 256 otherwise; wider rows return FFH_ERR_UNSUPPORTED.
 *   Bytes moved per touched row, beside the gradient reads: 2 * 4 D + 8 (w read and written, S read and written), against 4 * 4 D element-wise.
 */
#ifndef FF_HIP_ROWWISE_H_
#define FF_HIP_ROWWISE_H_

#include "ff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_ROWWISE_ABI_VERSION 1

#define FFH_SPARSE_OPT_ROWWISE_ADAGRAD 8      /* ffh_sparse_opt.kind, beside FFH_SPARSE_OPT_SGD / _SGD_MOMENTUM / _ADAM / _ADAGRAD (3) */

int ffh_rowwise_abi_version(void);

#ifdef __cplusplus
}
#endif

#define FFH_ROWWISE_API_LIST(X) \
  X(ffh_rowwise_abi_version)

#endif /* FF_HIP_ROWWISE_H_ */
