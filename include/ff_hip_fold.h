/* ff_hip_fold.h -- optional extension of the kernel C-ABI (include/ff_hip.h): small embedding tables folded out of the forward
 * GEMM, (ABI 2, further down) out of the weight-gradient GEMM, and (ABI 3, at the end) out of the data-gradient GEMM, of the Linear
 * layer that reads their rows through a Concat.
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

#define FFH_FOLD_ABI_VERSION 3

#define FFH_FOLD_KTILE      16    /* granularity of every reduction-depth segment and of D, in floats          */
#define FFH_FOLD_NTILE      64    /* out_dim of the folded layer is a multiple of this                           */
#define FFH_FOLD_MAX_GROUPS 64    /* tables per ffh_fold_product launch (= FFH_MAX_TABLES)                       */
#define FFH_FOLD_MAX_SEGS   32    /* kept segments per ffh_fold_linear_fwd call                                  */
#define FFH_FOLD_DW_NTILE   128   /* width of a column tile of dW in ffh_fold_linear_bwd_dw                      */
#define FFH_FOLD_DW_CHUNK   256   /* rows of a table per partial product of ffh_fold_dw_product                  */

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

/* ---- the weight gradient of the same layer (ABI 2) --------------------------------------------------------------------------------------
 * The column block of dW that faces a folded table is dy^T X_t, and X_t holds copies of the table's rows:
 *
 *     dW[:, cols_t] = dy^T X_t = G_t^T E_t,      G_t[r][:] = sum over the hits (b, l) of row r, id_t[b][l] == r, of dy[b][:]      (G_t: [R_t][out_dim])
 *
 * ffh_fold_segment_sum forms G, ffh_fold_dw_product adds G_t^T E_t into dW, ffh_fold_linear_bwd_dw is the layer's weight gradient over the column
 * tiles that are left.  dy is FINAL in all three (the activation derivative applied by whoever produced it, FFH_LINEAR_DY_PREMASKED's meaning).
 * Orders: G in the canonical order of the fused table update (below); the other two add partial sums into dW by float atomics, as the weight
 * gradient of ffh_linear_bwd does on this shape: not the same bits from run to run.  Each meets the bound above against float64. */

/* G_t[r][0 .. width) = sum over the hits of row r of dy[b][0 .. width); rows not hit: exactly 0.  `tables` as ffh_embedding_bwd_sgd_fused_multi takes
 * them: idx = [batch][in_dim] ids, weight = G_t ([num_entries][width] contiguous, overwritten), num_entries = R_t, io = dy, ld = its leading dimension.
 * THE ORDER OF THE SUM IS THE CONTRACT: the one include/ff_hip.h documents for the fused table update ("Canonical (deterministic) summation order":
 * hits sorted by (row, position), added left to right inside blocks of 32, the blocks' partials inside blocks of 1024, then those): the same bits on
 * every run and stream, whichever of the two forms below produces them.  The entry zeroes G, then
 *   wide rows (fp32 dy, width % 256 == 0, dy and every G_t 16-byte aligned, ld % 4 == 0): the update's index-only LSD sort run to completion (no bucket
 *     form, no one-launch form), then two launches of their own (csrc/fold_sum.hip): one workgroup per (table, 1024-block of the sorted list, 256
 *     columns) adds the runs of its 32-blocks and their partials in list order and stores every row that lies inside the block; a second, small launch
 *     adds the rows that cross 1024-block boundaries, block by block.  No arrival counters, no atomics; plain stores only.
 *   every other call: that update's own sort and ordered reduction with lr = -1, w = fmaf(1, sum, 0), launch for launch.
 * ffh_embedding_last_route(ctx) names the form: "fold_sum:wide|slice=256|lsd:passes=P", or the update's own token.  Needs
 * ffh_embedding_bwd_workspace_bytes(ntables, in_dim, width, batch) of workspace attached to ctx, and spoils a pending ffh_embedding_bwd_sort_multi
 * note on that workspace like any fused update: give it a ctx and a workspace of its own beside a table update in flight.  Width limits as the update's. */
int ffh_fold_segment_sum(ffh_ctx* ctx, const ffh_emb_table* tables, int ntables, int in_dim, int width, int64_t batch, ffh_stream s);

/* dw[o][col0_t + j] += sum_r G_t[r][o] E_t[r][j], j < d, for ngroups tables in ONE launch.  groups[t]: e = E_t, lde, col0 = col0_t, p = G_t ([rows][out_dim]
 * contiguous, read), rows = R_t.  dw is the layer's [out_dim][lddw] weight gradient, pre-zeroed or accumulating: the entry ADDS.  The rows of a table are
 * cut into chunks of FFH_FOLD_DW_CHUNK whose partial products meet in dw by float atomics.  d % 64 == 0, out_dim % FFH_FOLD_NTILE == 0, 16-byte aligned e
 * and p, lde % 4 == 0, 1 <= ngroups <= FFH_FOLD_MAX_GROUPS; anything else: FFH_ERR_UNSUPPORTED. */
int ffh_fold_dw_product(ffh_ctx* ctx, const ffh_fold_group* groups, int ngroups, float* dw, int64_t lddw, int d, int out_dim, ffh_stream s);

/* The weight gradient of ffh_linear_bwd over the KEPT column tiles only:
 *     dw[o][k] += sum_b dy[b][o] x[b][k]   for k in the tiles [FFH_FOLD_DW_NTILE kept[i], FFH_FOLD_DW_NTILE (kept[i] + 1)), i < nkept (ascending);
 *     db[o]    += sum_b dy[b][o]           when db != NULL, which needs kept[0] == 0 (the bias gradient rides on the first column of tiles)
 * dw is [out_dim][in_dim] contiguous.  Every other column of dw is left as it is.  Served only on the stream-K weight-gradient kernel, and only where
 * the whole layer's weight gradient runs on it too: exact fp32 math mode, not the deterministic mode, out_dim and in_dim multiples of 128, batch a
 * multiple of 64, aligned operands, and nkept column tiles that still fill the chip (nkept * (out_dim / 128) * (batch / 64) >= 8 per workgroup).
 * Anything else: FFH_ERR_UNSUPPORTED, nothing launched, nothing written.  ffh_linear_last_route names the form: "...|kept=a/b|...". */
int ffh_fold_linear_bwd_dw(ffh_ctx* ctx, const float* x, int64_t ldx, const float* dy, int64_t lddy, float* dw, float* db, int in_dim, int out_dim,
                           int64_t batch, const int32_t* kept, int nkept, ffh_stream s);

/* Whether the call above would be served for these arguments (nothing is launched): 1 = yes; 0 = no (it would return FFH_ERR_UNSUPPORTED);
 * negative: bad arguments. */
int ffh_fold_linear_bwd_dw_plan(ffh_ctx* ctx, const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* dw, const float* db, int in_dim,
                                int out_dim, int64_t batch, const int32_t* kept, int nkept);

/* ---- the data gradient of the same layer (ABI 3) -------------------------------------------------------------------------------------------
 * The only reader of dx[:, cols_t] of a folded table is that table's update, which sums those rows per table row:
 *
 *     dE_t[r] = sum over the hits (b, l) of r of dx[b][cols_t] = sum_hits dy[b] W[:, cols_t] = G_t[r] W[:, cols_t]       (G_t as above)
 *
 * ffh_fold_linear_bwd_dx is the layer's data gradient over the column tiles that are left; ffh_fold_table_update applies G_t W[:, cols_t] to the
 * tables as one dense product.  The rows of dx that face a folded table are then NOT PRODUCED: whoever reads the gradient of such a table's output
 * (a caller's own probe of the embedding output gradient) finds what the buffer held before.
 * Orders: the kept columns of dx are those of ffh_linear_bwd_ex(FFH_LINEAR_ONLY_DX) bit for bit (the same kernel, the same k order, whole tiles).
 * ffh_fold_table_update: one fp32 chain per element, the order of ffh_fold_product over the depth o (groups j of 16 ascending, in a group four MFMAs
 * e = 0..3, MFMA e adding o = 16 j + 4 q + e, q = 0..3), then ONE fmaf(-lr, sum, E): no atomics, no split over o.  With the canonical order of G
 * (ffh_fold_segment_sum) the tables' bits are the same from run to run and from stream to stream.  Bound: 1e-5 lr (term mass of the unfolded
 * sum over hits and o) + 2 ulp(E) against float64. */

/* The data gradient of ffh_linear_bwd_ex(..., FFH_LINEAR_ONLY_DX ...) of a layer whose dy is FINAL, over the KEPT column tiles only:
 *     dx[b][k] (+)= mask(sum_o dy[b][o] w[o][k])   for k in the tiles [FFH_FOLD_DW_NTILE kept[i], FFH_FOLD_DW_NTILE (kept[i] + 1)), i < nkept (ascending)
 * flags: FFH_LINEAR_DX_OVERWRITE (store; otherwise add to what dx holds) and FFH_LINEAR_DX_MASK_BY_X (dx = x > 0 ? v : 0, x the layer's input);
 * x may be NULL without the mask.  w is [out_dim][in_dim] contiguous.  Every other column of dx is left as it is.
 * colsum (or NULL): [in_dim] floats; colsum[k] += sum_b dx[b][k] as stored, for the kept k -- the bias gradient of the layer below, which rides on the
 *   tile at column 0: needs kept[0] == 0 and FFH_LINEAR_DX_OVERWRITE.  When the call returns FFH_OK the sums have been added.
 * record_behind (or NULL): recorded on `s` behind the kernel.
 * Both are THIS call's arguments: the entry neither reads nor clears what ffh_linear_bwd_set_dx_colsum / ffh_event_record_with_next_linear_bwd armed.
 * Served only where the whole layer's ONLY_DX call runs the persistent kernel on whole 128 x 128 tiles and the kept tiles still fill whole rounds of
 * workgroups by that kernel's own rule (at least one round, the last one 80 % full); exact fp32 math mode, not the deterministic mode.  Anything else:
 * FFH_ERR_UNSUPPORTED, nothing launched, nothing written, nothing recorded.  ffh_linear_last_route: "fold_linear_bwd_dx gemm|sk_128x128x64|kept=a/b|...". */
int ffh_fold_linear_bwd_dx(ffh_ctx* ctx, const float* x, int64_t ldx, float* dx, int64_t lddx, const float* dy, int64_t lddy, const float* w, int in_dim,
                           int out_dim, int64_t batch, int flags, const int32_t* kept, int nkept, float* colsum, ffh_event record_behind, ffh_stream s);

/* Whether the call above would be served for these arguments (nothing is launched): 1 = yes; 0 = no; negative: bad arguments. */
int ffh_fold_linear_bwd_dx_plan(ffh_ctx* ctx, const float* x, int64_t ldx, const float* dx, int64_t lddx, const float* dy, int64_t lddy, const float* w,
                                int in_dim, int out_dim, int64_t batch, int flags, const int32_t* kept, int nkept, const float* colsum);

/* E_t[r][j] = fmaf(-lr, sum_o G_t[r][o] w[o][col0_t + j], E_t[r][j]), j < d, for ngroups tables in ONE launch: plain SGD on the folded tables (no
 * state, no weight decay).  groups[t]: e = E_t (WRITTEN here, unlike the other entries), lde, col0 = col0_t, p = G_t ([rows][out_dim] contiguous, read),
 * rows = R_t.  w is the layer's [out_dim][ldw] weight.  A row nobody hit has G = 0 and keeps its bits.  Order: see above.  d % 64 == 0,
 * out_dim % FFH_FOLD_NTILE == 0, 16-byte aligned e, p and w, lde % 4 == 0, ldw % 4 == 0, col0 % 4 == 0, 1 <= ngroups <= FFH_FOLD_MAX_GROUPS;
 * anything else: FFH_ERR_UNSUPPORTED. */
int ffh_fold_table_update(ffh_ctx* ctx, const ffh_fold_group* groups, int ngroups, const float* w, int64_t ldw, int d, int out_dim, float lr, ffh_stream s);
/* ... with the rate read from `block` at run time (include/ff_hip_lr.h: the lr of ffh_lr_state, one uniform 4-byte load): the same bits as the
 * entry above given that value. */
struct ffh_lr_state;
int ffh_fold_table_update_lr(ffh_ctx* ctx, const ffh_fold_group* groups, int ngroups, const float* w, int64_t ldw, int d, int out_dim,
                             const struct ffh_lr_state* block, ffh_stream s);

#ifdef __cplusplus
}
#endif

#define FFH_FOLD_API_LIST(X) \
  X(ffh_fold_abi_version) X(ffh_fold_product) X(ffh_fold_gather_add) X(ffh_fold_linear_fwd) X(ffh_fold_linear_fwd_plan) \
  X(ffh_fold_segment_sum) X(ffh_fold_dw_product) X(ffh_fold_linear_bwd_dw) X(ffh_fold_linear_bwd_dw_plan) \
  X(ffh_fold_linear_bwd_dx) X(ffh_fold_linear_bwd_dx_plan) X(ffh_fold_table_update) X(ffh_fold_table_update_lr)

#endif /* FF_HIP_FOLD_H_ */
