/* ff_hip_data.h -- optional extension of the kernel C-ABI (include/ff_hip.h): loading one training batch of a device-resident data
 * set in shuffled order.
 *
 * A library may export this list or not; include/ff_hip.h and its symbol list are unchanged by it.  libffhip.so exports it,
 * the CPU oracle does not.  Callers load it separately (host/backend: KernelApi::data, null when absent; capi.data_api(lib)).
 *
 * Why: in file order a batch is a contiguous block of every array of the data set, and loading it is a handful of device-to-device
 * copies (one per table, one for the dense features, one for the labels).  In shuffled order its rows are scattered, so the whole
 * batch is ONE gather launch.  The order is the stateless function of include/ffh_perm.h: there is no permutation array and no
 * device-side state, and the launch arguments (epoch, step) say all there is to say.  The batch is loaded outside a captured step,
 * so arguments that change every step are no obstacle.
 *
 * CONTRACT (the order and the stripe rule are stated in include/ffh_perm.h)
 *   For every slot i in [0, local_batch):  p = ffh_perm_index(seed, epoch, step * local_batch + i, n_local), once per slot.
 *   A segment copies rows of `row_bytes` bytes from `src` to `dst`, both row-major without padding:
 *     FFH_GATHER_LOCAL_ROWS    dst row i               <- src row p                          (i in [0, local_batch))
 *                              dense features and labels: `src` holds this rank's n_local rows (and may hold more behind them)
 *     FFH_GATHER_GLOBAL_ROWS   dst row r * local_batch + i  <- src row ffh_perm_global_sample(p, local_batch, world, r)
 *                              for every r in [0, world): ids, whose owner serves the global batch; `src` holds at least
 *                              n_local * world rows
 *   A segment whose `dst` is NULL is skipped (a table this rank does not hold).  Nothing outside the destination rows is written,
 *   nothing outside the first n_local (local) / n_local * world (global) source rows is read.
 *   row_bytes is a positive multiple of 4; `src` and `dst` are 4-byte aligned.  A row moves in units of 16, 8 or 4 bytes: the widest
 *   that divides row_bytes and both base addresses.
 *   Requires 0 <= rank < world, local_batch >= 1, n_local a positive multiple of local_batch, (step + 1) * local_batch <= n_local.
 *   `rank` names the caller's stripe and is checked; the addressing does not need it, because a LOCAL segment's `src` already is
 *   that rank's stripe.
 *   The entry does not allocate, reads no environment variable and launches on the caller's stream: up to
 *   FFH_GATHER_MAX_SEGMENTS segments travel in the kernel arguments of one launch, a longer list takes one launch per
 *   FFH_GATHER_MAX_SEGMENTS segments.
 */
#ifndef FF_HIP_DATA_H_
#define FF_HIP_DATA_H_

#include "ff_hip.h"
#include "ffh_perm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_DATA_ABI_VERSION 1

#define FFH_GATHER_LOCAL_ROWS  0
#define FFH_GATHER_GLOBAL_ROWS 1
#define FFH_GATHER_MAX_SEGMENTS 64

typedef struct ffh_gather_segment {
  const void* src;
  void*       dst;         /* NULL: skipped */
  int32_t     row_bytes;   /* 8 * bag for ids, 4 * dense_dim for the dense features, 4 for labels */
  int32_t     kind;        /* FFH_GATHER_LOCAL_ROWS | FFH_GATHER_GLOBAL_ROWS */
} ffh_gather_segment;

typedef struct ffh_batch_order {
  uint64_t seed;
  int64_t  epoch;
  int64_t  step;           /* zero-based batch of the epoch */
  int64_t  local_batch;    /* Bl */
  int64_t  n_local;        /* training rows of one rank's stripe: (training batches) * Bl */
  int32_t  world, rank;
} ffh_batch_order;

int ffh_data_abi_version(void);

/* Fills the training batch `order` names: every segment, one launch (see the contract above).  `segments` is host memory and is
 * consumed before the call returns. */
int ffh_batch_gather(ffh_ctx* ctx, const ffh_gather_segment* segments, int nsegments, const ffh_batch_order* order, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_DATA_API_LIST(X) \
  X(ffh_data_abi_version) X(ffh_batch_gather)

#endif /* FF_HIP_DATA_H_ */
