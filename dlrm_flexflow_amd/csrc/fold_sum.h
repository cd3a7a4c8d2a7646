// fold_sum.h -- what fold_sum.hip (the wide-row segmented sum of include/ff_hip_fold.h) takes from embedding.hip: the FULLY sorted (row, position)
// list of every table in the ctx workspace, and the level-1 partial area of that workspace's layout.
#pragma once
#include "ffh_common.h"

namespace ffh_emb {

struct FullSort {
  const uint2* kp[FFH_MAX_TABLES];   // table t's N = batch * in_dim entries {row id, position}, sorted by (row, position)
  float*       partial0;             // [ntables][2 * ceil(N / FFH_EMB_CHUNK)][out_dim] floats of the workspace, free for the caller
  float*       partial1;             // [ntables][2 * ceil(N / FFH_EMB_CHUNK1)][out_dim] floats of the workspace, free for the caller
  int          passes;               // LSD passes the longest table took
};

// The index-only stable LSD passes of the fused table update (emb_sort.h) with the bucket form off, at any N: launches only, on `s`, into c's
// workspace (ffh_embedding_bwd_workspace_bytes, checked by the caller).  Spoils a pending ffh_embedding_bwd_sort_multi note on that workspace.
__attribute__((visibility("hidden"))) int emb_sort_full(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int D, int64_t batch, ffh_stream s, FullSort* out);

// fold_sum.hip: the sum itself behind that sort.  1: launched (the route note of c says so); 0: not served (width not a multiple of 256, dy or G not
// 16-byte aligned, ld % 4), nothing launched; < 0: error.  Writes every row of every G_t (rows not hit: zeros); arguments checked by the caller.
__attribute__((visibility("hidden"))) int fold_sum_wide(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int width, int64_t batch, ffh_stream s);

}  // namespace ffh_emb
