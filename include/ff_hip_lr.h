/* ff_hip_lr.h -- optional extension of the kernel C-ABI (include/ff_hip.h): the learning-rate schedule, and optimizer entry
 * points that read their rate from a small state block in device memory instead of taking it as a launch argument.
 *
 * A library may export this list or not; include/ff_hip.h and its symbol list are unchanged by it.  libffhip.so exports it,
 * the CPU oracle does not.  Callers load it separately (host/backend: KernelApi::lr, null when absent; capi.lr_api(lib)).
 *
 * Why: a launch argument is baked into a captured hipGraph, so a rate that changes from step to step (a schedule, Adam's
 * alpha_t) cannot be replayed.  A rate read from device memory can: a one-lane kernel (ffh_lr_state_advance) enqueued behind
 * the step's last reader moves the block to the next step, and a replayed graph replays that launch too -- the way the update
 * counter of the bf16 tables (ff_hip_bf16.h) already works.
 *
 * The schedule (k: zero-based optimizer step; base: the optimizer's rate; W warm-up steps, S decay start step, N decay steps):
 *
 *     k < W                      base * ((double)(k+1) / W)
 *     N > 0 and S <= k < S+N     max(1e-7, base * r * r),  r = (double)(S+N-k) / N
 *     N > 0 and k >= S+N         the value at k = S+N-1
 *     otherwise                  base
 *
 * in double, rounded to float once by the caller ((float)ffh_lr_schedule_value(...)).  W = S = N = 0 returns `base` itself.
 * The schedule is stated ONCE, below, and compiled into the host model, the Python binding's pure function (through the host
 * model) and the device kernel alike.
 */
#ifndef FF_HIP_LR_H_
#define FF_HIP_LR_H_

#include "ff_hip.h"
#include "ff_hip_bf16.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_LR_ABI_VERSION 1

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FFH_LR_INLINE static __host__ __device__ inline
#else
#define FFH_LR_INLINE static inline
#endif

/* The rate of step k.  Only multiplies and divides of values that come out of integer arithmetic: there is no a*b+c anywhere
 * for a compiler to contract into a fused multiply-add (hipcc contracts by default), so host and device agree bit for bit. */
FFH_LR_INLINE double ffh_lr_schedule_value(int64_t k, double base, int64_t W, int64_t S, int64_t N) {
  if (k < W) return base * ((double)(k + 1) / (double)W);
  if (N > 0 && k >= S) {
    const int64_t kk = k < S + N ? k : S + N - 1;                 /* past the decay: the last decayed value is held */
    const double r = (double)(S + N - kk) / (double)N;
    const double v = base * r * r;
    return v > 1e-7 ? v : 1e-7;
  }
  return base;
}

/* Adam's step size [AdamOptimizer::next]: alpha_t = alpha_k * sqrt(1 - beta2^t) / (1 - beta1^t), t = k + 1, the products kept
 * as running doubles (one multiplication per step).  `one_minus_*` are computed by the caller from products it has already
 * STORED (or passed through ffh_lr_opaque), so that 1 - b*bt is never contracted into one fused operation. */
FFH_LR_INLINE double ffh_lr_opaque(double v) {
#if defined(__GNUC__) || defined(__clang__)
#if defined(__HIP_DEVICE_COMPILE__)
  __asm__ volatile("" : "+v"(v));
#else
  __asm__ volatile("" : "+m"(v));
#endif
#endif
  return v;
}

/* What a block was initialised with.  beta1 / beta2 are only used for alpha_t (set them to 0 for SGD: alpha_t is then the rate itself). */
typedef struct ffh_lr_schedule {
  double  base;            /* --lr for SGD, alpha for Adam */
  int64_t warmup_steps;    /* W */
  int64_t decay_start;     /* S */
  int64_t decay_steps;     /* N */
  double  beta1, beta2;    /* Adam's decay rates (as the doubles AdamOptimizer holds) */
} ffh_lr_schedule;

/* What ffh_lr_state_read returns: the values of the step the block stands at. */
typedef struct ffh_lr_values {
  int64_t k;               /* zero-based index of the next optimizer step */
  float   lr;              /* (float)ffh_lr_schedule_value(k, base, W, S, N): what SGD reads */
  float   alpha_t;         /* (float)(lr_k * sqrt(1 - beta2^(k+1)) / (1 - beta1^(k+1))) in double: what Adam reads */
  double  beta1_t, beta2_t;/* beta^(k+1), running products */
} ffh_lr_values;

typedef struct ffh_lr_state ffh_lr_state;       /* opaque, device memory, ffh_lr_state_bytes() bytes, 16-byte aligned */

int    ffh_lr_abi_version(void);
size_t ffh_lr_state_bytes(void);
/* Fills the block for step `first_step` (the running products by first_step + 1 multiplications, as that many advances give). */
int ffh_lr_state_init(ffh_ctx* ctx, ffh_lr_state* block, const ffh_lr_schedule* sched, int64_t first_step, ffh_stream stream);
/* One lane on `stream`: the values of step k + 1.  Enqueue it behind the last reader of step k on that reader's stream. */
int ffh_lr_state_advance(ffh_ctx* ctx, ffh_lr_state* block, ffh_stream stream);
/* Device -> host, synchronises `stream`. */
int ffh_lr_state_read(ffh_ctx* ctx, const ffh_lr_state* block, ffh_lr_values* host_out, ffh_stream stream);

/* ffh_sgd_update_ex / ffh_adam_update with lr / alpha_t read from `block` at run time (one wave-uniform load); everything else --
 * zero_grad, the bf16 twin and the three-plane image of the weights, the 4-wide and 1-wide forms -- is the scalar entry's. */
int ffh_sgd_update_ex_lr(ffh_ctx* ctx, float* w, float* g, float* v, int64_t n, const ffh_lr_state* block, float wd, float mom, int nesterov,
                         int flags, ffh_stream stream);
int ffh_adam_update_lr(ffh_ctx* ctx, float* w, float* g, float* m, float* v, int64_t n, const ffh_lr_state* block, float b1, float b2, float wd,
                       float eps, int flags, ffh_stream stream);

/* ffh_embedding_bwd_opt_{fused,apply}_multi with opt->lr ignored: FFH_SPARSE_OPT_SGD and _SGD_MOMENTUM read the block's lr,
 * FFH_SPARSE_OPT_ADAM its alpha_t.  Same kernels (small, lsd, buckets), same bits as the scalar entry given that value. */
int ffh_embedding_bwd_opt_fused_multi_lr(ffh_ctx* ctx, const ffh_emb_table* tables, const ffh_emb_state* states, int ntables, int in_dim,
                                         int out_dim, int64_t batch, int aggr, const ffh_sparse_opt* opt, const ffh_lr_state* block, ffh_stream stream);
int ffh_embedding_bwd_opt_apply_multi_lr(ffh_ctx* ctx, const ffh_emb_table* tables, const ffh_emb_state* states, int ntables, int in_dim,
                                         int out_dim, int64_t batch, int aggr, const ffh_sparse_opt* opt, const ffh_lr_state* block, ffh_stream stream);
/* The same on bf16 tables (ff_hip_bf16.h: ffh_embedding_bwd_opt_{fused,apply}_multi_bf16; kind == FFH_SPARSE_OPT_SGD gives the bits of the
 * bf16 SGD entries). */
int ffh_embedding_bwd_opt_fused_multi_bf16_lr(ffh_ctx* ctx, const ffh_emb_table_bf16* tables, const ffh_emb_state* states, int ntables, int in_dim,
                                              int out_dim, int64_t batch, int aggr, const ffh_sparse_opt* opt, const ffh_bf16_rounding* rounding,
                                              const ffh_lr_state* block, ffh_stream stream);
int ffh_embedding_bwd_opt_apply_multi_bf16_lr(ffh_ctx* ctx, const ffh_emb_table_bf16* tables, const ffh_emb_state* states, int ntables, int in_dim,
                                              int out_dim, int64_t batch, int aggr, const ffh_sparse_opt* opt, const ffh_bf16_rounding* rounding,
                                              const ffh_lr_state* block, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_LR_API_LIST(X) \
  X(ffh_lr_abi_version) X(ffh_lr_state_bytes) X(ffh_lr_state_init) X(ffh_lr_state_advance) X(ffh_lr_state_read) \
  X(ffh_sgd_update_ex_lr) X(ffh_adam_update_lr) X(ffh_embedding_bwd_opt_fused_multi_lr) X(ffh_embedding_bwd_opt_apply_multi_lr) \
  X(ffh_embedding_bwd_opt_fused_multi_bf16_lr) X(ffh_embedding_bwd_opt_apply_multi_bf16_lr)

#endif /* FF_HIP_LR_H_ */
