/* ff_hip_fold.h -- optional extension of the kernel C-ABI (include/ff_hip.h): small embedding tables folded out of the forward
 * GEMM of the Linear layer that reads their rows through a Concat.
 *
 * A library may export this list or not; include/ff_hip.h and its symbol list are unchanged by it.  libffhip.so exports it,
 * the CPU oracle does not.  Callers load it separately (host/backend: KernelApi::fold, null when absent).
 *
 * Why: the layer's input row of sample b is [ ... | E_t[id_t(b)] | ... ].  For a table of R_t rows the batch's column block X_t holds
 * copies of at most R_t distinct rows, so
 *
 *     X_t W_t^T = (E_t W_t^T)[id_t]            W_t: the [out][D] column block of the layer's [out][in] weight that faces table t
 *
 * The product P_t = E_t W_t^T costs R_t D out multiply-adds instead of batch D out; the batch then needs one row of every P_t:
 *
 *     S[b][:] = sum_t sum_{l < L} P_t[id_t[b][l]][:]                       (ffh_fold_gather_add)
 *     y = act((X_kept W_kept^T + S) + bias)                                (ffh_fold_linear_fwd: the GEMM over the columns that stay)
 *
 * SUMMATION ORDERS (all fixed: the same bits on every run, eager or replayed, beside whatever else runs)
 *   ffh_fold_product     one fp32 chain per element: groups j of 16 columns ascending, in a group four MFMAs e = 0..3, MFMA e adding k = 16 j + 4 q + e, q = 0..3
 *   ffh_fold_gather_add  tables in list order, then l ascending, starting from the first term (no atomics)
 *   ffh_fold_linear_fwd  the kept segments in list order, k inside a segment in the GEMM kernel's own fixed order; then + S, then + bias
 * Every kernel meets the project's bound |error| <= 1e-5 * sum_k |a_k b_k| + 1e-6 against the unfolded formula in float64, the term
 * mass taken over the full-width sum.
 *
 * No allocation, no host synchronisation, no environment variable, no arrival counters: every entry is a fixed number of launches on the
 * caller's stream with arguments that do not change from step to step (capturable into a hipGraph).  Entries return FFH_OK or a
 * negative FFH_ERR_*; FFH_ERR_UNSUPPORTED means nothing was launched.
 */
#ifndef FF_HIP_FOLD_H_
#define FF_HIP_FOLD_H_

#include "ff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_FOLD_ABI_VERSION 1

#define FFH_FOLD_KTILE      16    /* granularity of every reduction-depth segment and of D, in floats          */
#define FFH_FOLD_NTILE      64    /* out_dim of the folded layer is a multiple of this                           */
#define FFH_FOLD_MAX_GROUPS 64    /* tables per ffh_fold_product launch (= FFH_MAX_TABLES)                       */
#define FFH_FOLD_MAX_SEGS   32    /* kept segments per ffh_fold_linear_fwd call                                  */

/* one table of ffh_fold_product */
typedef struct ffh_fold_group {
  const float* e;        /* [rows][lde] fp32 table rows, 16-byte aligned                                   */
  int64_t      lde;      /* floats between rows of e, a multiple of 4                                      */
  int64_t      col0;     /* first column of W_t inside the layer's weight: a multiple of FFH_FOLD_KTILE    */
  float*       p;        /* [rows][out_dim] result, rows contiguous, 16-byte aligned                       */
  int64_t      rows;     /* R_t >= 1                                                                       */
} ffh_fold_group;

/* a run of reduction-depth columns [k0, k0 + len) the GEMM keeps: both multiples of FFH_FOLD_KTILE, segments ascending and disjoint */
typedef struct ffh_fold_seg { int32_t k0, len; } ffh_fold_seg;

int ffh_fold_abi_version(void);

/* P_t = E_t W_t^T for ngroups tables in ONE launch.  w is the layer's [out_dim][ldw] weight (16-byte aligned, ldw % 4 == 0); W_t is
 * its columns [col0, col0 + d).  d % FFH_FOLD_KTILE == 0, out_dim % FFH_FOLD_NTILE == 0, 1 <= ngroups <= FFH_FOLD_MAX_GROUPS;
 * anything else: FFH_ERR_UNSUPPORTED. */
int ffh_fold_product(ffh_ctx* ctx, const ffh_fold_group* groups, int ngroups, const float* w, int64_t ldw, int d, int out_dim, ffh_stream s);

/* S[b][0 .. out_dim) = sum over tables t (in list order), then l < in_dim, of P_t[idx_t[b][l]][:].  `tables` has the layout
 * ffh_embedding_fwd_multi takes: idx = [batch][in_dim] int64 ids, weight = P_t ([num_entries][out_dim] contiguous), num_entries = R_t;
 * io and ld are ignored.  Ids are not checked on the device, as in the gather.  aggr must be FFH_AGGR_MODE_SUM, out_dim % 4 == 0,
 * ldS % 4 == 0, 16-byte aligned P_t and S, 1 <= ntables <= FFH_MAX_TABLES; anything else: FFH_ERR_UNSUPPORTED. */
int ffh_fold_gather_add(ffh_ctx* ctx, const ffh_emb_table* tables, int ntables, int in_dim, int out_dim, int64_t batch, int aggr,
                        float* S, int64_t ldS, ffh_stream s);

/* ffh_linear_fwd over the kept reduction-depth segments only, with an optional addend read in the epilogue:
 *     y[b][o] = act((sum_{k in keep} x[b][k] w[o][k] + addend[b][o]) + bias[o])
 * nkeep == 0 means "keep all of [0, in_dim)"; with addend == NULL as well the call IS ffh_linear_fwd (the same launches, the same bits).
 * w is [out_dim][in_dim] (the whole layer's weight), x and y as in ffh_linear_fwd.  Served: in_dim and every segment multiples of
 * FFH_FOLD_KTILE, out_dim % FFH_FOLD_NTILE == 0, x / w / y / addend 16-byte aligned with leading dimensions that are multiples of 4,
 * nkeep <= FFH_FOLD_MAX_SEGS, exact fp32 math mode; anything else: FFH_ERR_UNSUPPORTED.  Big aligned layers (segments of whole 64-deep
 * k-tiles, in_dim <= 8192, the shapes the persistent forward kernel of ffh_linear_fwd takes) run on that kernel with the skipped
 * k-tiles left out of its operand stream; the rest on a plain MFMA kernel. */
int ffh_fold_linear_fwd(ffh_ctx* ctx, const float* x, int64_t ldx, float* y, int64_t ldy, const float* w, const float* bias,
                        int in_dim, int out_dim, int64_t batch, int activation, const ffh_fold_seg* keep, int nkeep,
                        const float* addend, int64_t ldadd, ffh_stream s);

/* Which kernel the call above would launch for these arguments (nothing is launched): 2 = the persistent kernel; 1 = the plain kernel
 * and ffh_linear_fwd of the whole layer would not run on the persistent kernel either; 0 = the plain kernel where the whole layer runs on
 * the persistent one (folding would lose more than it saves); FFH_ERR_UNSUPPORTED as above. */
int ffh_fold_linear_fwd_plan(ffh_ctx* ctx, const float* x, int64_t ldx, const float* y, int64_t ldy, const float* w, const float* bias,
                             int in_dim, int out_dim, int64_t batch, const ffh_fold_seg* keep, int nkeep, const float* addend, int64_t ldadd);

#ifdef __cplusplus
}
#endif

#define FFH_FOLD_API_LIST(X) \
  X(ffh_fold_abi_version) X(ffh_fold_product) X(ffh_fold_gather_add) X(ffh_fold_linear_fwd) X(ffh_fold_linear_fwd_plan)

#endif /* FF_HIP_FOLD_H_ */
