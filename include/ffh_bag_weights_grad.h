/* ffh_bag_weights_grad.h -- optional extension of the kernel C-ABI (include/ff_hip.h): THE GRADIENT OF PER-SAMPLE BAG WEIGHTS.  Where the weights of
 * include/ffh_bag_weights.h are computed by the model (torchrec's PositionWeightedModule, feature gating, any small layer whose output scales the
 * lookups) they need a gradient, as torch.nn.EmbeddingBag(mode="sum", per_sample_weights=...) gives them one:
 *     gw[b][l] = sum over d of dY[b][d] * W[idx[b][l]][d]
 * for every lookup: the dot product of the bag's incoming gradient row with the table row that was looked up.  The per-sample weight itself does
 * NOT enter: d out / d w[b][l] is the unweighted row.
 *
 * A library may export this list or not; no other header, list or entry changes with it.  libffhip.so exports it, the CPU oracle does not.  Callers
 * load it separately (host/backend: KernelApi::bag_weights_grad, null when absent; capi.bag_weights_grad_api(lib)).  The header is named
 * ffh_bag_weights_grad.h and capi defines no BAG_WEIGHTS_GRAD_HEADER_PATH (callers use capi.EXTENSIONS["bag_weights_grad"].header_path), for the
 * reason include/ffh_dot_wide.h gives.
 *
 * THE CALL.  One launch for a group of <= FFH_MAX_TABLES tables of one width out_dim = D.  The table list has the shape of the weighted pad
 * gather's: tables[i].idx the ids [batch][in_dims[i]] with the pad id -1 (any id < 0), tables[i].weight the table (fp32 rows; the _bf16 entry: bf16
 * rows, widened exactly), tables[i].io the table's slice of the embedding output GRADIENT dY_i, [batch] rows tables[i].ld floats apart (read only).
 * The destination of table i is gw[i], [batch] rows gw_ld[i] floats apart, in_dims[i] floats each.
 *
 * CONTRACT.
 *   * a pad gives +0, and no table row is read for it;
 *   * flags & FFH_BAG_WGRAD_ACCUMULATE: gw[i][b][l] = gw[i][b][l] + dot (a pad adds +0); otherwise the dot is stored.  Nothing outside the
 *     [batch][in_dims[i]] elements of each destination is written.  THE DESTINATIONS OF ONE CALL MUST NOT OVERLAP: different workgroups would
 *     read, add and write the same element without atomics.  Tables that add into one buffer take one call each, in stream order.  gw[i] == gw[j] is FFH_ERR_BAD_ARG; other overlaps are not checked;
 *   * THE SUMMATION ORDER is fixed.  A row is cut into vectors of V elements (V = 4, or 1 in the 4-byte form below); a group of G lanes shares a
 *     row, G the smallest power of two >= min(D / V, 64).  Lane c of the group takes vectors c, c + G, c + 2 G, ... and adds its products over
 *     ascending d: acc = +0, then acc = fmaf(dY[b][d], W[id][d], acc).  A lane without a vector keeps +0.  The G lanes are then combined in a
 *     butterfly whose level k = 0, 1, ... pairs the lanes that differ in bit k: v = v + v_partner (both partners form the same sum).  So the result
 *     does not depend on the batch, the grid, the other tables of the call or the bag's position in it, and is bit-identical from run to run.  No
 *     atomics;
 *   * the error of one element is at most (D + 2) * 2^-23 * sum over d of |dY[b][d] * W[id][d]|;
 *   * rows that need more than 64 lanes are looped over by the group as said above; every lane keeps its part of the dY row in registers, which
 *     bounds the row: D <= 1024 in the 16-byte form, D <= 256 in the 4-byte form.  Wider is FFH_ERR_UNSUPPORTED;
 *   * THE 4-BYTE FORM.  The 16-byte form (16-byte loads of an fp32 row and of dY, 8-byte loads of a bf16 row) needs D % 4 == 0, every
 *     tables[i].ld % 4 == 0, every dY pointer and fp32 table 16-byte aligned and every bf16 table 8-byte aligned.  Any other call takes the 4-byte
 *     form: V = 1, the same kernel with scalar loads.  Nothing is refused for its alignment beyond the natural one;
 *   * tables[i].ld or gw_ld[i] >= 2^31 is FFH_ERR_UNSUPPORTED (the kernel arguments carry them in 32 bits), as is in_dims[i] > FFH_BAGS_MAX_IN_DIM;
 *   * a bad argument (null list or pointer with batch > 0, ntables outside [0, FFH_MAX_TABLES], D < 1, batch < 0, in_dims[i] < 1, ld < D,
 *     gw_ld[i] < in_dims[i], num_entries < 1, an unknown flag, a misaligned pointer) is FFH_ERR_BAD_ARG, and nothing is launched;
 *   * batch == 0 or ntables == 0 is FFH_OK;
 *   * no allocation, no workspace, no environment variable; the launch arguments do not change from step to step, so a step stays capturable.
 *
 * GEOMETRY.  A lane group owns one bag (table, b) at a time: it loads dY_i[b] into registers once and walks the bag's slots, U bags x JU slots in
 * flight per group: 4 x 1 for bags of fewer than 4 slots, 2 x 4 for longer ones (the two shapes of the ragged gather).  A 256-thread workgroup
 * takes 4 * (64 / G) * U bags per trip; workgroups are handed out in proportion to each table's lookups over one flat grid of at most
 * ffh_bag_weights_grad_grid_cap() workgroups, and a table's workgroups walk its batch with a stride.
 *
 * Bytes moved per lookup: 8 (id) + row bytes + 4 (result; 8 when accumulating), and one dY row of 4 D bytes per bag.
 */
#ifndef FFH_BAG_WEIGHTS_GRAD_H_
#define FFH_BAG_WEIGHTS_GRAD_H_

#include "ff_hip_bf16.h"
#include "ff_hip_bags.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFH_BAG_WEIGHTS_GRAD_ABI_VERSION 1

#define FFH_BAG_WGRAD_ACCUMULATE 1      /* add into gw instead of storing */

int ffh_bag_weights_grad_abi_version(void);
/* the most workgroups a launch takes */
int64_t ffh_bag_weights_grad_grid_cap(void);

int ffh_bag_weights_grad(ffh_ctx* ctx, const ffh_emb_table* tables, float* const* gw, const int64_t* gw_ld, const int* in_dims, int ntables, int out_dim,
                         int64_t batch, int flags, ffh_stream stream);
int ffh_bag_weights_grad_bf16(ffh_ctx* ctx, const ffh_emb_table_bf16* tables, float* const* gw, const int64_t* gw_ld, const int* in_dims, int ntables,
                              int out_dim, int64_t batch, int flags, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_BAG_WEIGHTS_GRAD_API_LIST(X) \
  X(ffh_bag_weights_grad_abi_version) X(ffh_bag_weights_grad_grid_cap) X(ffh_bag_weights_grad) X(ffh_bag_weights_grad_bf16)

#endif /* FFH_BAG_WEIGHTS_GRAD_H_ */
