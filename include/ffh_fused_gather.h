/* ffh_fused_gather.h -- optional extension of the kernel C-ABI (include/ff_hip.h) on top of the fold extension (include/ff_hip_fold.h): the gather-add
 * of the folded tables' products inside the epilogue of the first top layer's forward GEMM (csrc/linear_sk_gather.hip; DESIGN section 18, "The gather in
 * the epilogue").
 *
 * A library may export this list or not; include/ff_hip_fold.h, its symbol list and its ABI version are unchanged by it.  libffhip.so exports it, the
 * CPU oracle does not.  Callers load it separately (host/backend: KernelApi::fused_gather, null when absent: the host layer then keeps the gather-add
 * pass; capi.fused_gather_api(lib)).  An extension and a version of its own rather than fold ABI 4, and a header named ffh_fused_gather.h with no
 * FUSED_GATHER_HEADER_PATH in capi (callers use capi.EXTENSIONS["fused_gather"].header_path), for the reason include/ffh_dot_wide.h gives:
 * tests/test_extension_loader_cpu.py pins the fold header to ABI 3 and its thirteen entries, and the include/ff_hip_*.h files with an _API_LIST
 * and the capi.*_HEADER_PATH names to the fifteen extensions that came first.
 */
#ifndef FFH_FUSED_GATHER_H_
#define FFH_FUSED_GATHER_H_

#include "ff_hip_fold.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_FUSED_GATHER_ABI_VERSION 1

#define FFH_FUSED_GATHER_MAX_TABLES 16   /* tables per ffh_fused_gather_linear_fwd call                            */
#define FFH_FUSED_GATHER_MAX_BAG     4   /* ... ids per sample and table                                          */
#define FFH_FUSED_GATHER_MAX_TERMS  32   /* ... tables x ids (two images of a tile's ids live in LDS)             */

int ffh_fused_gather_abi_version(void);

/* ffh_fold_gather_add + ffh_fold_linear_fwd(addend = S) as ONE launch that never writes S: the persistent kernel's epilogue forms
 *     s = ((P_t0[id_t0[b][0]] + ...) + ...)        tables in list order, then l < bag, starting from the first term: ffh_fold_gather_add's order
 * for the 128 rows of its output tile, 16 bytes of a row per lane, and stores act((acc + s) + bias) -- the expression and the order of the two-call
 * form, hence ITS BITS.  `tables` / ntables / bag / aggr as ffh_fold_gather_add takes tables / ntables / in_dim / aggr (idx = [batch][bag] int64 ids,
 * weight = P_t, [num_entries][out_dim] contiguous; ids are not checked on the device); the rest as ffh_fold_linear_fwd.  The workgroup that owns a tile
 * reads the tile's ids once, into LDS, one tile ahead; the row pieces come out of L2 / the Infinity Cache, two terms of 16 rows in flight per lane.
 * No atomics, no arrival order, plain stores.
 * Served only where ffh_fold_linear_fwd_plan answers 2 for the layer (whole 128 x 128 tiles on the persistent kernel), aggr == FFH_AGGR_MODE_SUM,
 * ntables <= FFH_FUSED_GATHER_MAX_TABLES, bag <= FFH_FUSED_GATHER_MAX_BAG, ntables * bag <= FFH_FUSED_GATHER_MAX_TERMS, 16-byte aligned P_t and bias.
 * Anything else: FFH_ERR_UNSUPPORTED, nothing launched, y untouched.  ffh_linear_last_route: "fold_linear_fwd_gather gemm|sk_128x128x64|kept=a/b|gather=TxL|wgs=G". */
int ffh_fused_gather_linear_fwd(ffh_ctx* ctx, const ffh_emb_table* tables, int ntables, int bag, int aggr, const float* x, int64_t ldx, float* y, int64_t ldy,
                               const float* w, const float* bias, int in_dim, int out_dim, int64_t batch, int activation, const ffh_fold_seg* keep, int nkeep,
                               ffh_stream s);

/* Whether the call above would be served for these arguments (nothing is launched): 1 = yes; FFH_ERR_UNSUPPORTED = no; another negative: bad arguments. */
int ffh_fused_gather_linear_fwd_plan(ffh_ctx* ctx, const ffh_emb_table* tables, int ntables, int bag, int aggr, const float* x, int64_t ldx, const float* y,
                                    int64_t ldy, const float* w, const float* bias, int in_dim, int out_dim, int64_t batch, int activation,
                                    const ffh_fold_seg* keep, int nkeep);

#ifdef __cplusplus
}
#endif

#define FFH_FUSED_GATHER_API_LIST(X) X(ffh_fused_gather_abi_version) X(ffh_fused_gather_linear_fwd) X(ffh_fused_gather_linear_fwd_plan)

#endif /* FFH_FUSED_GATHER_H_ */
