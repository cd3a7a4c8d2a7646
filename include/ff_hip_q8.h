/* ff_hip_q8.h -- optional extension of the kernel C-ABI (include/ff_hip.h): embedding tables stored as 8-bit rows, each with its own
 * scale and bias (fbgemm's "fused 8-bit row-wise" format), for held-out evaluation: a quantizer fp32 / bf16 table -> rows, and the gather
 * (one bag size, or a bag size per table) that reads such rows.
 *
 * A library may export this list or not; include/ff_hip.h, include/ff_hip_bags.h and their symbol lists are unchanged by it.  libffhip.so
 * exports it, the CPU oracle does not.  Callers load it separately (capi.q8_api(lib)).
 *
 * ROW FORMAT.  A row of a table of width D (D % 4 == 0) is row_bytes bytes, row_bytes >= D + 8 and row_bytes % 4 == 0:
 *   bytes [0, D)        the D uint8 codes
 *   bytes [D, D + 4)    fp32 scale
 *   bytes [D + 4, D + 8) fp32 bias
 *   bytes [D + 8, row_bytes)  zero
 * row_bytes = D + 8 is fbgemm's layout and the default (the library's row-size function returns it).
 *
 * THE RULE, fp32 throughout, every operation rounded on its own (no fma); a bf16 source is widened exactly first:
 *   mn = min(x) + 0.0f      (a zero minimum is +0)        mx = max(x)         range = mx - mn
 *   scale = range / 255.0f        bias = mn               inv = 255.0f / (range + 1e-8f)
 *   code[d] = (uint8) rint((x[d] - mn) * inv)             round half to even; in [0, 255]
 *   w[d] = (float)code[d] * scale + bias                  a multiply, then an add: two roundings
 * A row with a non-finite value, or whose mx - mn overflows, is outside the contract: its codes are unspecified, nothing else is
 * affected.  dlrm_flexflow_amd.ffmodel.q8_quantize_reference / q8_dequantize_reference restate the rule in numpy.
 *
 * GATHER.  The semantics of ffh_embedding_fwd_multi (ffh_embedding_fwd_multi_bags), with W[row][d] replaced by w[d] of that row: the
 * accumulator starts at +0, acc = acc + w over ascending j, FFH_AGGR_MODE_AVG multiplies by the table's own 1.0f / (float)L.  The output
 * is bit for bit what the fp32 gather gives on the dequantized table, and a registered bf16 twin or three-plane image of a destination
 * is kept current with the same bits.
 *
 * ERRORS, as in the fp32 entries; nothing is launched on an error.  FFH_ERR_BAD_ARG: a null pointer, ntables > FFH_MAX_TABLES,
 * in_dims[i] < 1, a bad aggr, row_bytes < out_dim + 8, row_bytes % 4 != 0.  FFH_ERR_UNSUPPORTED: the 16-byte output form does not apply
 * (out_dim % 4 != 0, io not 16-byte aligned, ld % 4 != 0, rows not 4-byte aligned; there is no scalar form), in_dims[i] >
 * FFH_BAGS_MAX_IN_DIM, row_bytes >= 2^32.  Row ids are not checked.
 *
 * QUANTIZER.  One launch for all tables of a call: one grid-capped, grid-stride pass.  A lane takes E = 16 elements of a row where
 * out_dim % 16 == 0 (16-byte loads, a 16-byte store of codes), else E = 4.  A 256-thread workgroup takes 4 * (64 / P) rows of ONE table
 * per trip, P = the least power of two >= min(out_dim / E, 64) (the lanes that share a row), so table i
 * has ceil(num_entries_i / that) trips; the grid is the sum of trips, capped at the library's maximum of workgroups.
 */
#ifndef FF_HIP_Q8_H_
#define FF_HIP_Q8_H_

#include "ff_hip.h"
#include "ff_hip_bags.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_Q8_ABI_VERSION 1

/* one table of a gather: `rows` holds num_entries rows of row_bytes bytes; idx, io, ld as in ffh_emb_table */
typedef struct ffh_emb_table_q8 {
  const int64_t* idx;
  const uint8_t* rows;
  float*         io;
  int64_t        num_entries;
  int64_t        ld;
  int64_t        row_bytes;
} ffh_emb_table_q8;

/* one table of a quantizer call: weight is [num_entries][out_dim] fp32 (bf16 == 0) or bf16 bits (bf16 == 1), 16-byte aligned (bf16: 8) */
typedef struct ffh_q8_source {
  const void* weight;
  uint8_t*    rows;
  int64_t     num_entries;
  int64_t     row_bytes;
  int32_t     bf16;
  int32_t     reserved_;
} ffh_q8_source;

int    ffh_q8_abi_version(void);
size_t ffh_q8_row_bytes(int out_dim);                 /* out_dim + 8 */
int    ffh_q8_quantize_max_workgroups(void);          /* the quantizer's grid cap */

int ffh_embedding_quantize_q8(ffh_ctx* ctx, const ffh_q8_source* src, int ntables, int out_dim, ffh_stream stream);
int ffh_embedding_fwd_multi_q8(ffh_ctx* ctx, const ffh_emb_table_q8* tables, int ntables, int in_dim, int out_dim, int64_t batch, int aggr,
                               ffh_stream stream);
int ffh_embedding_fwd_multi_bags_q8(ffh_ctx* ctx, const ffh_emb_table_q8* tables, const int* in_dims, int ntables, int out_dim,
                                    int64_t batch, int aggr, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_Q8_API_LIST(X) \
  X(ffh_q8_abi_version) X(ffh_q8_row_bytes) X(ffh_q8_quantize_max_workgroups) X(ffh_embedding_quantize_q8) \
  X(ffh_embedding_fwd_multi_q8) X(ffh_embedding_fwd_multi_bags_q8)

#endif /* FF_HIP_Q8_H_ */
