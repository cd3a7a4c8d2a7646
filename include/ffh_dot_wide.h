/* ffh_dot_wide.h -- optional extension of the kernel C-ABI (include/ff_hip.h): the pairwise-dot feature interaction for up to 128 feature
 * vectors, one launch each way (csrc/interaction_wide.hip).
 *
 * A library may export this list or not; include/ff_hip.h and its symbol list are unchanged by it, and ffh_dot_interaction_fwd / _bwd keep
 * refusing nrows > 32.  libffhip.so exports it, the CPU oracle does not.  Callers load it separately (host/backend: KernelApi::dot_wide, null
 * when absent; capi.dot_wide_api(lib)).  The header is named ffh_dot_wide.h, beside ffh_rng.h / ffh_perm.h / ffh_bf16.h and not ff_hip_dot_wide.h,
 * and capi defines no DOT_WIDE_HEADER_PATH (callers use capi.EXTENSIONS["dot_wide"].header_path): tests/test_extension_loader_cpu.py pins the
 * include/ff_hip_*.h files with an _API_LIST and the capi.*_HEADER_PATH names to the fifteen extensions that came before this one.
 *
 * CONTRACT -- the one of ffh_dot_interaction_fwd / _bwd with 128 in place of 32.  z: [batch][nrows][d] floats, sample stride ldz >= nrows * d
 * (row 0 is the bottom-MLP output, rows 1.. the embedding outputs), 2 <= nrows <= 128, d >= 1.
 *   ffh_dot_interaction_wide_fwd   out[b][0 .. d)                 = z[b][0][:]                            (bit for bit)
 *                                  out[b][d + i (i - 1) / 2 + j]  = <z[b][i], z[b][j]>   for i > j        ldo >= d + nrows (nrows - 1) / 2
 *   ffh_dot_interaction_wide_bwd   dz[b][i][:] = sum_{j != i} g(i, j) z[b][j][:],  g(i, j) = out_grad[b][d + pair(max(i, j), min(i, j))],
 *                                  dz[b][0][:] += out_grad[b][0 .. d);   z_grad = dz (FFH_DOT_BWD_OVERWRITE) or z_grad + dz (flags 0).
 *                                  ldg >= d + nrows (nrows - 1) / 2, ldzg >= nrows * d; any other flag bit is refused.
 *   Exact fp32 on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32), no atomics: results are bit-identical from run to run and do not depend on
 *   the batch or on the grid.  |got - exact| <= (k + 2) 2^-23 sum|terms| with k the number of terms.  Sample offsets are 64-bit.
 *   Nothing outside the stated elements of out / z_grad is written; z and out_grad are only read.  A bad argument is FFH_ERR_BAD_ARG: nothing
 *   is launched, nothing is written.  batch == 0 is FFH_OK.  No allocation, no environment variable; one launch on the caller's stream with
 *   arguments that do not change from step to step (capturable).
 *   FORM: one choice for the whole launch -- 16-byte accesses (forward: the sample goes global -> LDS by LDS-DMA) where d % 4 == 0, the leading
 *   dimensions of z (and z_grad) are multiples of 4 and their bases 16-byte aligned; 4-byte accesses otherwise.  The forward's pass-through
 *   columns take 16-byte stores where, in addition, ldo % 4 == 0 and out is 16-byte aligned.  out_grad needs no alignment.
 *   GRID: one 4-wave workgroup owns a sample and walks the batch with the grid as its stride;
 *     workgroups = min(batch, compute units * FFH_DOT_WIDE_FWD_PER_CU(nrows))   forward  (two images of 32 ceil(nrows / 32) rows x 512 bytes)
 *     workgroups = min(batch, compute units * FFH_DOT_WIDE_BWD_PER_CU(nrows))   backward (S = G + G^T and the pair table)
 *   Bytes moved per sample: 4 (nrows d + d + nrows (nrows - 1) / 2) forward, that plus 4 nrows d (8 nrows d accumulating) backward.
 */
#ifndef FFH_DOT_WIDE_H_
#define FFH_DOT_WIDE_H_

#include "ff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_DOT_WIDE_ABI_VERSION 1

#define FFH_DOT_WIDE_MAX_ROWS 128
#define FFH_DOT_WIDE_FWD_PER_CU(nrows) ((nrows) <= 64 ? 2 : 1)
#define FFH_DOT_WIDE_BWD_PER_CU(nrows) ((nrows) <= 96 ? 2 : 1)

int ffh_dot_wide_abi_version(void);

int ffh_dot_interaction_wide_fwd(ffh_ctx* ctx, const float* z, int64_t ldz, float* out, int64_t ldo, int64_t batch, int nrows, int d,
                                 ffh_stream stream);

int ffh_dot_interaction_wide_bwd(ffh_ctx* ctx, const float* z, int64_t ldz, const float* out_grad, int64_t ldg, float* z_grad, int64_t ldzg,
                                 int64_t batch, int nrows, int d, int flags, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_DOT_WIDE_API_LIST(X) \
  X(ffh_dot_wide_abi_version) X(ffh_dot_interaction_wide_fwd) X(ffh_dot_interaction_wide_bwd)

#endif /* FFH_DOT_WIDE_H_ */
