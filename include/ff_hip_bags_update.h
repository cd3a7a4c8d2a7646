/* ff_hip_bags_update.h -- optional extension of the kernel C-ABI (include/ff_hip.h): the fused table update (sort + segmented reduce + row
 * rule) of tables with a bag size PER TABLE, in one call.  The companion of include/ff_hip_bags.h (the ragged gather).
 *
 * A library may export this list or not; include/ff_hip.h, include/ff_hip_bags.h and their symbol lists are unchanged by it.  libffhip.so
 * exports it, the CPU oracle does not.  Callers load it separately (host/backend: KernelApi::bags_update, null when absent;
 * capi.bags_update_api(lib)).
 *
 * SEMANTICS.  tables[i].idx is [batch][in_dims[i]] int64.  For every table i the call leaves, bit for bit, the weights and the optimizer
 * state that the uniform fused entry leaves when called for that table alone with in_dim = in_dims[i]:
 *   opt == NULL                      ffh_embedding_bwd_sgd_fused_multi[_bf16]     at `lr`
 *   opt != NULL, lr_block == NULL    ffh_embedding_bwd_opt_fused_multi[_bf16]     (every ffh_sparse_opt kind; the rate is opt->lr, `lr` is ignored)
 *   opt != NULL, lr_block != NULL    ffh_embedding_bwd_opt_fused_multi[_bf16]_lr  (include/ff_hip_lr.h)
 * FFH_AGGR_MODE_AVG divides a table's gradient rows by its own in_dims[i].  A row that no id touches keeps its weights and state.  With all
 * in_dims equal the call equals the uniform multi-table call bit for bit.  Exactly one of `tables` (fp32 rows) and `tables_bf16` (bf16
 * rows, include/ff_hip_bf16.h; `rounding` is required then and ignored otherwise) is set.
 *
 * ROUTES (ffh_embedding_last_route).  "bags:small": every batch * in_dims[i] <= 2048 -- one launch, one workgroup per table.
 * "bags:lsd:passes=P": otherwise -- P histogram + scatter passes of the stable sort (a table runs only the passes its own row count needs)
 * and one apply launch, each over a flat grid in which table i has exactly ceil(batch * in_dims[i] / tile) workgroups.
 *
 * ARGUMENTS.  FFH_ERR_BAD_ARG: in_dims[i] < 1; a null in_dims with ntables > 0; both or neither table array; ntables < 0 or above
 * FFH_BAGS_UPDATE_MAX_TABLES (the kernel arguments hold 64 table descriptors, state pointers and 16-bit bag sizes in 3,936 of their 4,096
 * bytes; every offset is derived from the bag sizes inside the kernels, so a captured graph replays the launch without reading anything
 * the host rewrites); momentum / Adam on bf16 rows above FFH_BF16_MAX_STATEFUL_TABLES tables; an lr_block without opt; a missing
 * optimizer state for a rule that needs one; whatever the uniform entries refuse.  FFH_ERR_UNSUPPORTED: in_dims[i] > FFH_BAGS_MAX_IN_DIM;
 * batch * in_dims[i] >= 2^31.  FFH_ERR_WORKSPACE: the ctx's workspace is smaller than ffh_embedding_bwd_bags_workspace_bytes.  Nothing is
 * launched on an error.  Row ids are not checked.
 *
 * Like the uniform fused call, this one spoils a pending ffh_embedding_bwd_sort_multi note on the workspace it overwrites: a later
 * ffh_embedding_bwd_*_apply_multi on that note returns FFH_ERR_WORKSPACE.  The ragged two-call form (sort, then apply) of this entry is an
 * extension of its own, include/ff_hip_bags_sort.h, on this header's descriptor; this call spoils a pending ragged sort in the same way.
 */
#ifndef FF_HIP_BAGS_UPDATE_H_
#define FF_HIP_BAGS_UPDATE_H_

#include "ff_hip.h"
#include "ff_hip_bf16.h"
#include "ff_hip_lr.h"
#include "ff_hip_bags.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_BAGS_UPDATE_ABI_VERSION 1

#define FFH_BAGS_UPDATE_MAX_TABLES FFH_MAX_TABLES

typedef struct ffh_bags_update {
  const ffh_emb_table*      tables;       /* fp32 tables, or NULL                                      */
  const ffh_emb_table_bf16* tables_bf16;  /* bf16 tables, or NULL: exactly one of the two              */
  const int*                in_dims;      /* ids per sample, per table                                 */
  const ffh_emb_state*      states;       /* NULL for plain SGD                                        */
  int                       ntables;
  int                       out_dim;
  int64_t                   batch;
  int                       aggr;         /* FFH_AGGR_MODE_SUM / _AVG                                  */
  float                     lr;           /* the rate when opt is NULL                                 */
  const ffh_sparse_opt*     opt;          /* NULL: plain SGD at `lr`                                   */
  const ffh_bf16_rounding*  rounding;     /* bf16 tables only                                          */
  const ffh_lr_state*       lr_block;     /* NULL: the rate from opt / lr                              */
} ffh_bags_update;

int ffh_bags_update_abi_version(void);
/* the largest kernel-argument struct of the ragged kernels (<= 4096: a launch would fail otherwise) */
size_t ffh_bags_update_kernarg_bytes(void);

/* host arithmetic, no device needed: the workspace (ffh_ctx_set_workspace) the call below needs; 0 on a bad argument.  Grows with
 * sum over i of batch * in_dims[i]; with equal in_dims it equals ffh_embedding_bwd_workspace_bytes. */
size_t ffh_embedding_bwd_bags_workspace_bytes(const int* in_dims, int ntables, int out_dim, int64_t batch);

int ffh_embedding_bwd_fused_multi_bags(ffh_ctx* ctx, const ffh_bags_update* u, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_BAGS_UPDATE_API_LIST(X) \
  X(ffh_bags_update_abi_version) X(ffh_bags_update_kernarg_bytes) X(ffh_embedding_bwd_bags_workspace_bytes) X(ffh_embedding_bwd_fused_multi_bags)

#endif /* FF_HIP_BAGS_UPDATE_H_ */
