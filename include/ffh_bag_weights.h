/* ffh_bag_weights.h -- optional extension of the kernel C-ABI (include/ff_hip.h): PER-SAMPLE WEIGHTS on embedding bags.  Every lookup carries a
 * float; a bag is the weighted sum of its rows, and a row's gradient is the weighted sum of its bags' gradients.  This is
 * torch.nn.EmbeddingBag(mode="sum", per_sample_weights=..., padding_idx=...) with the pad outside the table, torchrec's weighted features.  The
 * weights are data: no gradient with respect to them is formed.
 *
 * A library may export this list or not; include/ff_hip_pad.h, include/ff_hip_pad_mean.h and their symbol lists are unchanged by it, and none of
 * their entries changes what it does.  libffhip.so exports it, the CPU oracle does not.  Callers load it separately (host/backend:
 * KernelApi::bag_weights, null when absent; capi.bag_weights_api(lib)).  The header is named ffh_bag_weights.h and capi defines no
 * BAG_WEIGHTS_HEADER_PATH (callers use capi.EXTENSIONS["bag_weights"].header_path), for the reason include/ffh_dot_wide.h gives.
 *
 * The entries are weighted forms of the PAD RAGGED entries of include/ff_hip_pad.h: a bag size per table, an id < 0 is a pad, and a pad's weight
 * is never read.  Table i's weights are `weights[i]`, floats laid out [batch][in_dims[i]] like its ids.  SUM only: FFH_AGGR_MODE_AVG gets
 * FFH_ERR_BAD_ARG with a message that names the mean entry (include/ff_hip_pad_mean.h); weights with mean pooling are left out.
 *
 * CONTRACT.  Every product is rounded on its own (the file is compiled with contraction off): a multiply, then an add, never an fma.
 *   GATHER   acc = +0; for ascending slot j with idx[b][j] >= 0: acc = acc + w[b][j] * W[idx[b][j]][d].  A bf16 row is widened exactly first.  A
 *            bag of only pads gives +0.  No table row and no weight is read for a pad.  A bf16 twin (ffh_ctx_bf16_mirror_set) or a three-plane
 *            image (ffh_ctx_bf16x3_mirror_set) of the destination is kept as the pad gather keeps it (the same store epilogue).
 *   UPDATE   the gradient row of entry (b, j) is w[b][j] * G[b][d]: one multiply as the row is loaded and before any sum, at the place where the
 *            AVG update of the existing entries divides.  A pad contributes nothing.  A row that only pads "touch" keeps its weights and its
 *            optimizer state bit for bit.  No row past num_entries - 1 is read or written.
 *   Every ffh_sparse_opt kind and plain SGD, fp32 and bf16 rows, both rounding modes (the same ffh_bf16_rounding keys and counter), the scalar
 *   rate and the rate block, the fused call and the pair.
 *
 * REFERENCES, BIT FOR BIT AND BY CONSTRUCTION.
 *   1. With every weight 1.0f, both entries equal the pad entries of include/ff_hip_pad.h in SUM mode (1 * x = x).
 *   2. The weighted gather equals a float32 loop in slot order (ffmodel.weighted_bag_reference).
 *   3. The weighted update on (idx, w, G) equals the pad update on the EXPANDED problem: every bag of L slots becomes L bags of one slot
 *      (in_dims = 1, batch' = batch * L), the flat position b * L + j stays, and G'[b * L + j] = float32(w[b][j]) * G[b] is prepared on the
 *      host.  The flat positions, and so the sort order, the FFH_EMB_CHUNK cuts and the summation order, are the same.
 *
 * THE PAIR.  There is no sort entry here: the sort reads ids only, and ffh_embedding_bwd_sort_multi_bags_pad serves this apply too.  A pad sort's
 * note is consumed by exactly one apply -- the pad apply, the mean apply or the weighted apply; ffh_embedding_bwd_sort_multi_bags followed by the
 * weighted apply returns FFH_ERR_WORKSPACE and launches nothing.  The spoiling rules of include/ff_hip_bags_sort.h hold unchanged.
 *
 * ROUTES (ffh_embedding_last_route): "bags:small:pad:w" and "bags:lsd:passes=P:pad:w"; the passes are those of the pad form.
 *
 * ARGUMENTS, LIMITS.  Those of the pad entries, and nothing is launched on an error.  In addition: a null `weights`, or a null weights[i] with
 * batch > 0, is FFH_ERR_BAD_ARG; a weight pointer needs 4-byte alignment only (a misaligned one is FFH_ERR_BAD_ARG); in the update a gradient
 * leading dimension tables[i].ld >= 2^32 is FFH_ERR_UNSUPPORTED (the kernel arguments carry it in 32 bits beside the weight pointer).  The
 * workspace is ffh_embedding_bwd_bags_workspace_bytes, unchanged: the weights are read where they lie.
 *
 * Bytes moved per lookup: 12 + 4 D in the gather (id, weight, fp32 row) against the pad gather's 8 + 4 D.
 */
#ifndef FFH_BAG_WEIGHTS_H_
#define FFH_BAG_WEIGHTS_H_

#include "ff_hip_pad.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_BAG_WEIGHTS_ABI_VERSION 1

/* the descriptor of the ragged update (include/ff_hip_bags_update.h) and one weight pointer per table */
typedef struct ffh_bags_update_weighted {
  ffh_bags_update     u;
  const float* const* weights;      /* [u.ntables]: table i's [batch][in_dims[i]] floats */
} ffh_bags_update_weighted;

int ffh_bag_weights_abi_version(void);

int ffh_embedding_fwd_multi_bags_weighted(ffh_ctx* ctx, const ffh_emb_table* tables, const float* const* weights, const int* in_dims, int ntables,
                                          int out_dim, int64_t batch, int aggr, ffh_stream stream);
int ffh_embedding_fwd_multi_bags_weighted_bf16(ffh_ctx* ctx, const ffh_emb_table_bf16* tables, const float* const* weights, const int* in_dims,
                                               int ntables, int out_dim, int64_t batch, int aggr, ffh_stream stream);

int ffh_embedding_bwd_fused_multi_bags_weighted(ffh_ctx* ctx, const ffh_bags_update_weighted* u, ffh_stream stream);
/* the apply behind ffh_embedding_bwd_sort_multi_bags_pad */
int ffh_embedding_bwd_apply_multi_bags_weighted(ffh_ctx* ctx, const ffh_bags_update_weighted* u, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_BAG_WEIGHTS_API_LIST(X) \
  X(ffh_bag_weights_abi_version) X(ffh_embedding_fwd_multi_bags_weighted) X(ffh_embedding_fwd_multi_bags_weighted_bf16) \
  X(ffh_embedding_bwd_fused_multi_bags_weighted) X(ffh_embedding_bwd_apply_multi_bags_weighted)

#endif /* FFH_BAG_WEIGHTS_H_ */
