/* ff_hip_bags_sort.h -- optional extension of the kernel C-ABI (include/ff_hip.h): the two-call form of the ragged table update
 * (include/ff_hip_bags_update.h).  The stable sort of a table's (row id, position) list needs the ids only, so a caller that knows them early
 * (the DLRM step: at the gather) runs it off the critical path with ffh_embedding_bwd_sort_multi_bags and does the part that needs the output
 * gradients -- segmented reduce, folds, the row rule -- with ffh_embedding_bwd_apply_multi_bags when they exist.  The ragged companion of
 * ffh_embedding_bwd_sort_multi / ffh_embedding_bwd_*_apply_multi (include/ff_hip.h).
 *
 * A library may export this list or not; include/ff_hip.h, include/ff_hip_bags.h, include/ff_hip_bags_update.h and their symbol lists are
 * unchanged by it.  libffhip.so exports it, the CPU oracle does not.  Callers load it separately (host/backend: KernelApi::bags_sort, null
 * when absent; capi.bags_sort_api(lib)).
 *
 * SEMANTICS.  Both entries take the descriptor of ffh_embedding_bwd_fused_multi_bags.  Sort followed by apply launches what that call
 * launches, in the same order, on the same workspace layout (ffh_embedding_bwd_bags_workspace_bytes sizes both): the pair leaves the fused
 * call's bits, table by table -- weights and every state array, fp32 and bf16 rows in both rounding modes, every row rule, the scalar rate
 * and the rate block, SUM and AVG.
 *   sort    reads the table array that is set (its idx and num_entries), in_dims, ntables, out_dim and batch.  It does not read io / ld,
 *           weight, states, opt, rounding, lr, lr_block or aggr: a null `rounding` with bf16 tables is fine here.
 *   apply   reads every field, as the fused call does.
 *
 * ROUTES (ffh_embedding_last_route) are the fused call's, set by either entry.  "bags:small": the sort lives inside the apply kernel, so the
 * sort call launches nothing and only leaves its note.  "bags:lsd:passes=P": the sort call runs the P histogram + scatter passes (pass 0
 * clears the apply phase's level-1 slots and arrival counters), the apply call is the one apply launch.
 *
 * CONTRACT.  The apply CONSUMES what the sort left in the workspace, so the pair is one-shot: the ctx remembers its latest ragged sort (the
 * workspace, ntables, out_dim, batch, every bag size, every table's num_entries and idx pointer), the apply requires a matching note and
 * clears it.  The caller keeps
 *   - the same tables, ids and batch in both calls, and the ids unchanged until the apply has run;
 *   - nothing else on the workspace in between: a fused update (uniform or ragged), a uniform ffh_embedding_bwd_sort_multi[_bf16], a
 *     segmented sum of include/ff_hip_fold.h on this ctx spoil the note;
 *   - the order: the library orders nothing between the two calls, the caller's streams and events put the apply behind the sort;
 *   - a capture that records both replays them as a pair (the note is host state: a replay does not consult it).
 * The apply returns FFH_ERR_WORKSPACE, with nothing launched and nothing written, when there is no sort before it, on a second apply on one
 * sort, on another bag-size list (even one with the same sum), batch, out_dim, num_entries or idx pointer, when another workspace is
 * attached, and when a fused call or a uniform sort came in between.  A ragged note never satisfies a uniform ffh_embedding_bwd_*_apply_multi,
 * a uniform note never satisfies the ragged apply.
 *
 * ARGUMENTS.  Those of ffh_embedding_bwd_fused_multi_bags, with its codes, checked before the note; nothing is launched on an error.  The
 * sort checks only what it reads.
 */
#ifndef FF_HIP_BAGS_SORT_H_
#define FF_HIP_BAGS_SORT_H_

#include "ff_hip_bags_update.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_BAGS_SORT_ABI_VERSION 1

int ffh_bags_sort_abi_version(void);

int ffh_embedding_bwd_sort_multi_bags(ffh_ctx* ctx, const ffh_bags_update* u, ffh_stream stream);
int ffh_embedding_bwd_apply_multi_bags(ffh_ctx* ctx, const ffh_bags_update* u, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_BAGS_SORT_API_LIST(X) \
  X(ffh_bags_sort_abi_version) X(ffh_embedding_bwd_sort_multi_bags) X(ffh_embedding_bwd_apply_multi_bags)

#endif /* FF_HIP_BAGS_SORT_H_ */
