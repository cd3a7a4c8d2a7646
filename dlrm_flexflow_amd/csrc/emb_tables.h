// emb_tables.h -- host-side checks on a call's table list that the gather (embedding_fwd.hip)
// and the table update (embedding.hip) share.  Internal: no kernel, nothing exported.
#pragma once
#include "emb_row_rules.h"
#include "../../include/ff_hip_bags.h"

#include <cstdint>
#include <cstring>

namespace ffh_emb {

constexpr int kBagMaxL = 65535;    // a bag size travels in 16 bits of the kernel arguments (BagArgs::L, BagsGeo::L)
static_assert(kBagMaxL == FFH_BAGS_MAX_IN_DIM, "include/ff_hip_bags.h");

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline int validate_tables(ffh_ctx* c, const ffh_emb_table* t, int nt, int L, int D, int64_t batch, int aggr) {
  if (nt < 0 || nt > FFH_MAX_TABLES) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding: ntables out of range");
  if (L <= 0 || D <= 0 || batch < 0) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding: bad dims");
  if (aggr != FFH_AGGR_MODE_SUM && aggr != FFH_AGGR_MODE_AVG) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding: aggr must be SUM or AVG");
  for (int i = 0; i < nt; i++) {
    if (batch > 0 && (!t[i].idx || !t[i].weight || !t[i].io)) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding: null pointer");
    if (t[i].ld < D || t[i].num_entries <= 0) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding: ld < out_dim or num_entries <= 0");
  }
  return FFH_OK;
}

// fp32 tables: every table row and every io row can be read and written 16 bytes at a time
inline bool can_vec4(const ffh_emb_table* t, int nt, int D) {
  if (D % 4) return false;
  for (int i = 0; i < nt; i++)
    if (!aligned16(t[i].weight) || !aligned16(t[i].io) || (t[i].ld % 4)) return false;
  return true;
}

// bf16 tables as ffh_emb_table (the weight pointer carries the bf16 bits; the kernels read it through WT) and, for the update, their keys
inline int bf16_tables(ffh_ctx* c, const ffh_emb_table_bf16* in, int nt, ffh_emb_table* out, Bf16Keys* keys) {
  if (nt < 0 || nt > FFH_MAX_TABLES) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bf16: ntables out of range");
  if (nt > 0 && !in) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bf16: null tables");
  for (int i = 0; i < nt; i++) {
    if (in[i].table < 0 || in[i].col0 < 0) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bf16: negative table index or col0");
    out[i] = ffh_emb_table{in[i].idx, reinterpret_cast<float*>(in[i].weight), in[i].io, in[i].num_entries, in[i].ld};
    if (keys) { keys->table[i] = in[i].table; keys->col0[i] = in[i].col0; }
  }
  return FFH_OK;
}

}  // namespace ffh_emb
