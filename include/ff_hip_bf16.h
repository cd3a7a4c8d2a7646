/* ff_hip_bf16.h -- optional extension of the kernel C-ABI (include/ff_hip.h): embedding tables stored in bf16.
 *
 * A library may export this list or not; include/ff_hip.h and its symbol list are unchanged by it.  libffhip.so exports
 * it, the CPU oracle does not.  Callers load it separately (host/backend: KernelApi::bf16, null when absent;
 * capi.bf16_api(lib)).
 *
 * The math stays fp32: the gather widens every stored element exactly and sums in the order of ffh_embedding_fwd_multi
 * (bit-identical to that entry on the widened fp32 table, SUM and AVG, twin / three-plane outputs included); the update
 * computes the row sums and w32 = fmaf(-lr, sum, (float)w16) exactly as ffh_embedding_bwd_sgd_fused_multi does on the
 * widened table, then rounds once to bf16 (include/ffh_bf16.h: nearest even, or stochastic with bits keyed by seed,
 * the update counter in device memory, global table index, global row and global column).
 * Version 2 adds momentum / weight-decay SGD and Adam on bf16 tables (ffh_embedding_bwd_opt_{fused,apply}_multi_bf16): the row gradient
 * is the canonical FFH_EMB_CHUNK-order sum, w is the widened (float)w16, and the state update and the fp32 result w32 are statement by
 * statement those of FFH_SPARSE_OPT_SGD_MOMENTUM / FFH_SPARSE_OPT_ADAM in ffh_embedding_bwd_opt_fused_multi on the widened table.  The state
 * stays fp32 (ffh_emb_state, [num_entries][out_dim]) and is bit-identical to what the fp32 entry leaves on the widened table; w32 is then
 * rounded once to bf16 with the key above.  kind == FFH_SPARSE_OPT_SGD gives the bits of ffh_embedding_bwd_sgd_*_multi_bf16.
 */
#ifndef FF_HIP_BF16_H_
#define FF_HIP_BF16_H_

#include "ff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_BF16_ABI_VERSION 2   /* 2: ffh_embedding_bwd_opt_fused_multi_bf16 / _apply_multi_bf16 (momentum / weight-decay SGD, Adam);
                                    1: gather, fused update (one call or sort + apply), uniform init, counter advance */

/* the stateful entries (momentum / Adam) take at most this many tables per call: their kernel arguments hold the tables, the state pointers
 * AND the rounding keys, which for 64 tables would pass the 4 KB of kernel arguments; more tables are refused with FFH_ERR_BAD_ARG
 * (split the call).  kind == FFH_SPARSE_OPT_SGD takes FFH_MAX_TABLES like the SGD entries. */
#define FFH_BF16_MAX_STATEFUL_TABLES 32

/* One bf16 table of a batched launch: ffh_emb_table with 16-bit weights and the table's place in the model. */
typedef struct ffh_emb_table_bf16 {
  const int64_t* idx;      /* [batch][in_dim] int64 row ids                                         */
  uint16_t*      weight;   /* [num_entries][out_dim] bf16 bit patterns                              */
  float*         io;       /* fwd: out [batch][ld] fp32; bwd: out_grad [batch][ld] fp32 (read)      */
  int64_t        num_entries;
  int64_t        ld;       /* leading dimension of `io` in floats (>= out_dim)                      */
  int32_t        table;    /* global table index in the model (stochastic-rounding key)             */
  int32_t        col0;     /* global column of this slice's column 0 (column-sharded tables; else 0) */
} ffh_emb_table_bf16;

/* How the update rounds: FFH_BF16_ROUND_STOCHASTIC (0) or FFH_BF16_ROUND_NEAREST (1) (include/ffh_bf16.h).  `counter`:
 * one uint64 in device memory, the update number the stochastic bits are keyed by; read by the update kernels, advanced
 * by ffh_bf16_counter_advance (enqueue it once per training step behind the apply; a captured graph replays it too). */
typedef struct ffh_bf16_rounding {
  int32_t         mode;
  int32_t         reserved_;
  uint64_t        seed;
  const uint64_t* counter;  /* may be null for FFH_BF16_ROUND_NEAREST */
} ffh_bf16_rounding;

int ffh_bf16_abi_version(void);

/* Gather + bag-sum from bf16 tables into fp32 outputs (ffh_embedding_fwd_multi semantics). */
int ffh_embedding_fwd_multi_bf16(ffh_ctx* ctx, const ffh_emb_table_bf16* tables, int ntables, int in_dim, int out_dim,
                                 int64_t batch, int aggr, ffh_stream stream);
/* Fused backward + plain SGD on bf16 tables (ffh_embedding_bwd_sgd_fused_multi semantics, then one rounding). */
int ffh_embedding_bwd_sgd_fused_multi_bf16(ffh_ctx* ctx, const ffh_emb_table_bf16* tables, int ntables, int in_dim, int out_dim,
                                           int64_t batch, int aggr, float lr, const ffh_bf16_rounding* rounding, ffh_stream stream);
/* The same in two phases (ffh_embedding_bwd_sort_multi / ffh_embedding_bwd_sgd_apply_multi: one apply per sort). */
int ffh_embedding_bwd_sort_multi_bf16(ffh_ctx* ctx, const ffh_emb_table_bf16* tables, int ntables, int in_dim, int out_dim,
                                      int64_t batch, ffh_stream stream);
int ffh_embedding_bwd_sgd_apply_multi_bf16(ffh_ctx* ctx, const ffh_emb_table_bf16* tables, int ntables, int in_dim, int out_dim,
                                           int64_t batch, int aggr, float lr, const ffh_bf16_rounding* rounding, ffh_stream stream);
/* Fused backward + the row rule `opt` (ffh_embedding_bwd_opt_fused_multi semantics on the widened table, fp32 state `states`, then one
 * rounding); the apply half behind ffh_embedding_bwd_sort_multi_bf16, with the same one-shot rule (one apply per sort). */
int ffh_embedding_bwd_opt_fused_multi_bf16(ffh_ctx* ctx, const ffh_emb_table_bf16* tables, const ffh_emb_state* states, int ntables, int in_dim,
                                           int out_dim, int64_t batch, int aggr, const ffh_sparse_opt* opt, const ffh_bf16_rounding* rounding,
                                           ffh_stream stream);
int ffh_embedding_bwd_opt_apply_multi_bf16(ffh_ctx* ctx, const ffh_emb_table_bf16* tables, const ffh_emb_state* states, int ntables, int in_dim,
                                           int out_dim, int64_t batch, int aggr, const ffh_sparse_opt* opt, const ffh_bf16_rounding* rounding,
                                           ffh_stream stream);
/* p[i] = ffh_bf16_rne(ffh_uniform(ffh_hash(seed, i), lo, hi)): the rounding of ffh_init_uniform's output. */
int ffh_init_uniform_bf16(ffh_ctx* ctx, uint16_t* p, int64_t n, uint64_t seed, float lo, float hi, ffh_stream stream);
/* *counter += 1, one lane, on `stream`. */
int ffh_bf16_counter_advance(ffh_ctx* ctx, uint64_t* counter, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_BF16_API_LIST(X) \
  X(ffh_bf16_abi_version) X(ffh_embedding_fwd_multi_bf16) X(ffh_embedding_bwd_sgd_fused_multi_bf16) \
  X(ffh_embedding_bwd_sort_multi_bf16) X(ffh_embedding_bwd_sgd_apply_multi_bf16) X(ffh_init_uniform_bf16) X(ffh_bf16_counter_advance) \
  X(ffh_embedding_bwd_opt_fused_multi_bf16) X(ffh_embedding_bwd_opt_apply_multi_bf16)

#endif /* FF_HIP_BF16_H_ */
