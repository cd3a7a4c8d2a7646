/* ff_hip_bags.h -- optional extension of the kernel C-ABI (include/ff_hip.h): the embedding gather with a bag size PER TABLE, in one launch
 * (multi-hot lookups; the MLPerf DLRM-DCNv2 pooling sizes run from 1 to 100 over 26 tables).
 *
 * A library may export this list or not; include/ff_hip.h, include/ff_hip_bf16.h and their symbol lists are unchanged by it.  libffhip.so
 * exports it, the CPU oracle does not.  Callers load it separately (host/backend: KernelApi::bags, null when absent; capi.bags_api(lib)).
 *
 * SEMANTICS.  Those of ffh_embedding_fwd_multi, per table: tables[i].idx is [batch][in_dims[i]] int64, and
 *   out[b][d] = sum over j = 0 .. in_dims[i] - 1, ascending, of W[idx[b][j]][d]      in fp32, starting from +0;
 * FFH_AGGR_MODE_AVG multiplies the sum by the table's own 1.0f / (float)in_dims[i].  The result of table i is bit for bit what
 * ffh_embedding_fwd gives for that table alone; with all in_dims equal the call equals ffh_embedding_fwd_multi bit for bit.  A bf16 twin
 * (ffh_ctx_bf16_mirror_set) or a three-plane image (ffh_ctx_bf16x3_mirror_set) of a destination is kept current under the conditions of
 * ffh_embedding_fwd_multi, with the same bits.  The _bf16 form reads bf16 tables (include/ff_hip_bf16.h) and equals the fp32 form on the
 * widened table.
 *
 * ARGUMENTS.  in_dims[i] >= 1, else FFH_ERR_BAD_ARG; in_dims[i] > FFH_BAGS_MAX_IN_DIM returns FFH_ERR_UNSUPPORTED (the kernel arguments
 * carry a bag size in 16 bits: 64 tables, their twin and image pointers and the bag sizes stay inside the 4 KB of kernel arguments, and a
 * captured graph replays the launch without reading anything the host rewrites).  A null in_dims with ntables > 0 and ntables >
 * FFH_MAX_TABLES return FFH_ERR_BAD_ARG.  Nothing is launched on an error.  Row ids are not checked (as in ffh_embedding_fwd_multi).
 *
 * The update's ragged form is an extension of its own, include/ff_hip_bags_update.h (ffh_embedding_bwd_fused_multi_bags): the sort and the
 * segmented reduction of ffh_embedding_bwd_* are laid out on one N = batch * in_dim per call.  Without that extension, call them once per bag size.
 */
#ifndef FF_HIP_BAGS_H_
#define FF_HIP_BAGS_H_

#include "ff_hip.h"
#include "ff_hip_bf16.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_BAGS_ABI_VERSION 1

#define FFH_BAGS_MAX_IN_DIM 65535

int ffh_bags_abi_version(void);
/* sizeof the kernel-argument struct of the ragged gather's kernel (<= 4096: the launch would fail otherwise) */
size_t ffh_bags_kernarg_bytes(void);

int ffh_embedding_fwd_multi_bags(ffh_ctx* ctx, const ffh_emb_table* tables, const int* in_dims, int ntables, int out_dim, int64_t batch,
                                 int aggr, ffh_stream stream);
int ffh_embedding_fwd_multi_bags_bf16(ffh_ctx* ctx, const ffh_emb_table_bf16* tables, const int* in_dims, int ntables, int out_dim,
                                      int64_t batch, int aggr, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_BAGS_API_LIST(X) \
  X(ffh_bags_abi_version) X(ffh_bags_kernarg_bytes) X(ffh_embedding_fwd_multi_bags) X(ffh_embedding_fwd_multi_bags_bf16)

#endif /* FF_HIP_BAGS_H_ */
