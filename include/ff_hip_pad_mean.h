/* ff_hip_pad_mean.h -- optional extension of the kernel C-ABI (include/ff_hip.h): MEAN pooling over variable-length embedding bags.  The pad
 * entries of include/ff_hip_pad.h pool with a sum and refuse FFH_AGGR_MODE_AVG; the entries here are their mean forms: the divisor of a bag is
 * the number of lookups that are there, not its slot count in_dims[i].  This is torch.nn.EmbeddingBag(mode="mean", padding_idx=...) with the
 * pad outside the table.
 *
 * A library may export this list or not; include/ff_hip_pad.h keeps its seven symbols and its ABI version, and none of its entries changes
 * what it does.  libffhip.so exports the list, the CPU oracle does not.  Callers load it separately (host/backend: KernelApi::pad_mean, null
 * when absent; capi.pad_mean_api(lib)).
 *
 * CONTRACT.  An id < 0 is a pad, as in include/ff_hip_pad.h.  Let count[t][b] be the number of ids >= 0 in bag b of table t.  `aggr`
 * (u->aggr) must be FFH_AGGR_MODE_AVG: FFH_AGGR_MODE_SUM gets FFH_ERR_BAD_ARG with a message that names the pad entry to call instead.
 * Nothing is launched on any error.
 *
 *   GATHER   out[b][d] = S * (1.0f / (float)max(count, 1)), where S is the pad gather's fp32 sum (ascending slots, from +0, no row read for
 *            a pad): one fp32 reciprocal and one fp32 multiply per element -- the operation and the place of the AVG epilogue of the
 *            existing gathers, with count in place of in_dims[i].  A bag of only pads gives a row of +0.  A bf16 twin
 *            (ffh_ctx_bf16_mirror_set) or a three-plane image (ffh_ctx_bf16x3_mirror_set) of the destination is kept from the scaled value,
 *            as the existing entries keep it.
 *   UPDATE   every gradient row is divided by (float)count[t][b], one correctly rounded fp32 division per element, as the row is loaded and
 *            before any sum -- the operation and the place of the AVG update of the existing entries, with count in place of in_dims[i].  A
 *            pad contributes nothing.  A row that only pads "touch" keeps its weights and its optimizer state bit for bit.  No row past
 *            num_entries - 1 is read or written.
 *
 * REFERENCES, BIT FOR BIT AND BY CONSTRUCTION.
 *   1. With no pad in the input, both mean entries equal ffh_embedding_fwd_multi_bags[_bf16] / ffh_embedding_bwd_fused_multi_bags with
 *      FFH_AGGR_MODE_AVG on the same tables (count = in_dims[i] everywhere).
 *   2. The mean gather equals the pad gather of include/ff_hip_pad.h in SUM mode, multiplied on the host in float32 by
 *      float32(1) / float32(max(count, 1)).
 *   3. The mean update on gradient rows G equals the pad update of include/ff_hip_pad.h in SUM mode on the host-prepared rows
 *      G'[t][b] = G[t][b] / float32(max(count[t][b], 1)) -- every ffh_sparse_opt kind and plain SGD, fp32 and bf16 rows, both rounding modes
 *      (the same ffh_bf16_rounding keys and counter), the scalar rate and the rate block, the fused call and the pair, both routes.  (A bag
 *      whose count is 0 has no entry that is summed, so its row of G is never loaded.)
 *
 * THE PAIR.  There is no sort entry here: the sort reads ids only, and ffh_embedding_bwd_sort_multi_bags_pad serves either apply.  A pad sort
 * note is consumed by exactly one of ffh_embedding_bwd_apply_multi_bags_pad and the mean apply below; ffh_embedding_bwd_sort_multi_bags
 * followed by the mean apply returns FFH_ERR_WORKSPACE and launches nothing.  The spoiling rules of include/ff_hip_bags_sort.h hold unchanged.
 *
 * WORKSPACE.  The mean update keeps one 16-bit count per (table, bag) in a region BEHIND the layout of ffh_embedding_bwd_bags_workspace_bytes
 * (in_dims[i] <= 65535, so 16 bits hold every count).  ffh_embedding_bwd_bags_pad_mean_workspace_bytes returns that size plus the region
 * (host arithmetic; 0 on a bad argument); the mean update entries return FFH_ERR_WORKSPACE on a smaller workspace.  The counts are written by
 * the mean apply and by the mean fused call -- never by the sort -- so a pending sort's lists and cleared slots are not touched, and the
 * existing query and layout do not change.
 *
 * ROUTES (ffh_embedding_last_route): "bags:small:pad:mean" and "bags:lsd:passes=P:pad:mean"; the passes are those of the pad form.
 *
 * LIMITS.  Those of the pad entries (include/ff_hip_pad.h).
 */
#ifndef FF_HIP_PAD_MEAN_H_
#define FF_HIP_PAD_MEAN_H_

#include "ff_hip_pad.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_PAD_MEAN_ABI_VERSION 1

int ffh_pad_mean_abi_version(void);

int ffh_embedding_fwd_multi_bags_pad_mean(ffh_ctx* ctx, const ffh_emb_table* tables, const int* in_dims, int ntables, int out_dim, int64_t batch,
                                          int aggr, ffh_stream stream);
int ffh_embedding_fwd_multi_bags_pad_mean_bf16(ffh_ctx* ctx, const ffh_emb_table_bf16* tables, const int* in_dims, int ntables, int out_dim,
                                               int64_t batch, int aggr, ffh_stream stream);

size_t ffh_embedding_bwd_bags_pad_mean_workspace_bytes(const int* in_dims, int ntables, int out_dim, int64_t batch);

int ffh_embedding_bwd_fused_multi_bags_pad_mean(ffh_ctx* ctx, const ffh_bags_update* u, ffh_stream stream);
int ffh_embedding_bwd_apply_multi_bags_pad_mean(ffh_ctx* ctx, const ffh_bags_update* u, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_PAD_MEAN_API_LIST(X) \
  X(ffh_pad_mean_abi_version) X(ffh_embedding_fwd_multi_bags_pad_mean) X(ffh_embedding_fwd_multi_bags_pad_mean_bf16) \
  X(ffh_embedding_bwd_bags_pad_mean_workspace_bytes) X(ffh_embedding_bwd_fused_multi_bags_pad_mean) \
  X(ffh_embedding_bwd_apply_multi_bags_pad_mean)

#endif /* FF_HIP_PAD_MEAN_H_ */
