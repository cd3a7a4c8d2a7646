/* ff_hip_pad.h -- optional extension of the kernel C-ABI (include/ff_hip.h): variable-length embedding bags.  A bag stays a fixed
 * [batch][in_dims[i]] block of int64 ids (include/ff_hip_bags.h), and "no lookup" is a value of the id itself: FFH_EMB_PAD_ID.  A sample has
 * UP TO in_dims[i] lookups for table i, and sometimes none.  This is padding_idx semantics with the pad outside the table: no row is set
 * aside for it, the table and its optimizer state keep their shapes, and a captured step replays with the same grids.
 *
 * A library may export this list or not; include/ff_hip.h, include/ff_hip_bags.h, include/ff_hip_bags_update.h, include/ff_hip_bags_sort.h
 * and their symbol lists are unchanged by it, and none of their entries changes what it does.  libffhip.so exports it, the CPU oracle does
 * not.  Callers load it separately (host/backend: KernelApi::pad, null when absent; capi.pad_api(lib)).
 *
 * SEMANTICS.  FFH_EMB_PAD_ID is -1.  In the entries below an id < 0 is a pad (a host layer lets only -1 through); every other id is a row
 * of the table and is not checked, as in the ragged entries.
 *
 *   GATHER   out[b][d] = sum of W[idx[b][j]][d] over the j, ascending, whose id is not a pad, in fp32, starting from +0.  A bag of only pads
 *            gives a row of +0 (bit pattern 0).  No table row is read for a pad.  A bf16 twin (ffh_ctx_bf16_mirror_set) or a three-plane
 *            image (ffh_ctx_bf16x3_mirror_set) of the destination is kept current exactly as ffh_embedding_fwd_multi_bags keeps it.
 *   UPDATE   a pad contributes no gradient to any row.  A row that only pads "touch" keeps its weights and its optimizer state bit for
 *            bit.  No row past num_entries - 1 is read or written, and no extra row or state row is allocated anywhere.
 *
 * REFERENCE, BIT FOR BIT.  Take the table's R rows and append one all-zero row R; replace every pad by R; append one state row where the
 * rule has state.  ffh_embedding_fwd_multi_bags[_bf16] on that table gives the pad gather's output.  ffh_embedding_bwd_fused_multi_bags on
 * it leaves rows [0, R) of the weights and of every state array as the pad update leaves them -- every ffh_sparse_opt kind, fp32 and bf16
 * rows, both rounding modes (the same ffh_bf16_rounding keys and counter), the scalar rate and the rate block.  By construction:
 *   - x + (+0) = x bit for bit for every value an accumulator that started at +0 can hold (it never holds -0), so leaving a pad's add out
 *     equals adding the zero row;
 *   - the sort loads a pad as key R, the largest key, so the pads sort behind every real entry and the FFH_EMB_CHUNK cuts of the SORTED
 *     list (the canonical order of the segmented sum) over the real entries are those of the reference call; the apply phase drops the
 *     segment whose key is R in the level-0 reduce -- it leaves no partial row and no slot record, so neither fold ever sees it.
 * With no pad in the input the pad entries equal the ragged entries on the same table bit for bit.  A model of one bag size uses the same
 * entries with equal in_dims (the ragged headers promise that this equals the uniform call): there are no _pad forms of the uniform entries.
 *
 * MEAN POOLING (FFH_AGGR_MODE_AVG) is refused with FFH_ERR_UNSUPPORTED by every entry here that takes an aggregation mode, and nothing is
 * launched: a mean over the lookups that are there needs each bag's count of them in the gather's epilogue and in the apply phase.  The
 * mean forms that keep that count are an extension of their own, include/ff_hip_pad_mean.h.
 *
 * ROUTES (ffh_embedding_last_route): "bags:small:pad" and "bags:lsd:passes=P:pad", under the ragged update's rules.  The radix plan of a
 * table covers the bits of num_entries (the pad key) instead of those of num_entries - 1, so a table whose row count is a power of the
 * digit's base runs one more pass than it does without pads.
 *
 * THE PAIR.  ffh_embedding_bwd_sort_multi_bags_pad and ffh_embedding_bwd_apply_multi_bags_pad are the two-call form, under the contract
 * of include/ff_hip_bags_sort.h (one apply per sort, the same spoiling rules, FFH_ERR_WORKSPACE with nothing launched otherwise).  A pad
 * sort is followed by a pad apply: a pad sort followed by ffh_embedding_bwd_apply_multi_bags, or ffh_embedding_bwd_sort_multi_bags followed
 * by the pad apply, returns FFH_ERR_WORKSPACE and launches nothing.
 *
 * LIMITS.  Those of the ragged entries, plus num_entries <= 2^32 - 2: the sort keys are 32 bits and 0xFFFFFFFF is the reduce kernel's "no
 * key"; above that FFH_ERR_UNSUPPORTED.  The workspace is ffh_embedding_bwd_bags_workspace_bytes, unchanged.
 *
 * ffh_pad_mask_indices makes synthetic pads: idx[i] becomes FFH_EMB_PAD_ID unless ffh_u24(ffh_hash(seed, first + i)) < fill -- the
 * counter-based stream of include/ffh_rng.h that ffh_init_uniform draws from, so a host restates it exactly.  fill >= 1 changes nothing,
 * fill <= 0 pads every slot.  `first` is the global index of idx[0] in its stream, so a rank that holds a slice of the data masks it as
 * the whole would be masked.
 */
#ifndef FF_HIP_PAD_H_
#define FF_HIP_PAD_H_

#include "ff_hip_bags_sort.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_PAD_ABI_VERSION 1

#define FFH_EMB_PAD_ID (-1)

int ffh_pad_abi_version(void);

int ffh_embedding_fwd_multi_bags_pad(ffh_ctx* ctx, const ffh_emb_table* tables, const int* in_dims, int ntables, int out_dim, int64_t batch,
                                     int aggr, ffh_stream stream);
int ffh_embedding_fwd_multi_bags_pad_bf16(ffh_ctx* ctx, const ffh_emb_table_bf16* tables, const int* in_dims, int ntables, int out_dim,
                                          int64_t batch, int aggr, ffh_stream stream);

int ffh_embedding_bwd_fused_multi_bags_pad(ffh_ctx* ctx, const ffh_bags_update* u, ffh_stream stream);
int ffh_embedding_bwd_sort_multi_bags_pad(ffh_ctx* ctx, const ffh_bags_update* u, ffh_stream stream);
int ffh_embedding_bwd_apply_multi_bags_pad(ffh_ctx* ctx, const ffh_bags_update* u, ffh_stream stream);

int ffh_pad_mask_indices(ffh_ctx* ctx, int64_t* idx, int64_t count, uint64_t seed, int64_t first, float fill, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_PAD_API_LIST(X) \
  X(ffh_pad_abi_version) X(ffh_embedding_fwd_multi_bags_pad) X(ffh_embedding_fwd_multi_bags_pad_bf16) \
  X(ffh_embedding_bwd_fused_multi_bags_pad) X(ffh_embedding_bwd_sort_multi_bags_pad) X(ffh_embedding_bwd_apply_multi_bags_pad) \
  X(ffh_pad_mask_indices)

#endif /* FF_HIP_PAD_H_ */
