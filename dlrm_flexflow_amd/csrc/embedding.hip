// embedding.hip -- the fused table update (backward + sparse optimizer step), the reference's
// dense atomic backward and the bf16 tables' helpers, hand-written for gfx950.
//
// The update never materialises the dense [R][D] gradient: row ids are radix-sorted per table
// with LDS histograms and wave-ballot ranking, duplicate rows are reduced in registers by the
// lane-group that owns the run, and each touched row is read-modified-written exactly once.
// What is here (host code but for four small kernels):
//   * the plan of a call, for both updates: radix_plan, fill_passes, sort_per_thread, reduce_tile,
//     ws_layout (bwd_layout, bags_layout), UpdatePlan, set_rule_args, set_ws_slots;
//   * emb_bwd_phases: the update with one bag size; emb_sort_full: its sort alone (fold_sum.hip);
//   * emb_bwd_bags: the update with a bag size per table (include/ff_hip_bags_update.h), whole or in its two phases (include/ff_hip_bags_sort.h),
//     and its pad form, in which an id < 0 is no lookup (include/ff_hip_pad.h);
//   * emb_bwd_dense_kernel, emb_localize_kernel, the bf16 init / counter kernels; every entry.
// What is where:
//   * the gather: embedding_fwd.hip; checks on a table list shared with it: emb_tables.h;
//   * the sort kernels: emb_sort.h; the apply kernels and row rules: emb_reduce.h, emb_row_rules.h,
//     compiled per weight type in embedding_update_f32.hip / _bf16.hip;
//   * the ragged update's kernels: emb_bags_update.h, in embedding_update_bags_f32.hip / _bf16.hip.
#include "emb_tables.h"
#include "emb_reduce.h"
#include "fold_sum.h"
#include "lr_state.h"
#include "../../include/ff_hip_bags_update.h"
#include "../../include/ff_hip_bags_sort.h"
#include "emb_bags_update.h"
#include "../../include/ff_hip_pad_mean.h"

namespace {

using namespace ffh_emb;

// ---------------------------------------------------------------------------
// reference-parity dense backward: fp32 atomics into the full-table gradient.
// One dword per lane, lanes contiguous along the row: each atomic wave-instruction is
// 256 contiguous bytes, the shape the memory-side atomic units run at full rate.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void emb_bwd_dense_kernel(const int64_t* __restrict__ idx, const float* __restrict__ g,
                                                            float* __restrict__ wg, int L, int D, int64_t batch,
                                                            int64_t gld, int avg) {
  ffh_kernel_prio();
  const int64_t total = batch * D;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t b = i / D;
    const int off = (int)(i - b * D);
    float gr = g[b * gld + off];
    if (avg) gr = gr / (float)L;
    for (int j = 0; j < L; j++) {
      const int64_t row = idx[b * L + j];
      atomicAdd(wg + row * (int64_t)D + off, gr);
    }
  }
}

// ---- The plan of an update call, one bag size or one per table: radix digits, tile sizes, workspace. ----
// bits that hold every row id of a table of `rows` rows (at least 1)
inline int bit_length(int64_t rows) {
  int tb = 1;
  while (tb < 32 && ((rows - 1) >> tb) != 0) tb++;
  return tb;
}

inline int64_t max_rows(const ffh_emb_table* tables, int nt) {
  int64_t maxR = 1;
  for (int i = 0; i < nt; i++) maxR = tables[i].num_entries > maxR ? tables[i].num_entries : maxR;
  return maxR;
}

// digits of <= kMaxRadixBits bits covering the ids of the largest table: `passes` stable passes of `rb` bits each
struct RadixPlan { int bits, passes, rb; };
inline RadixPlan radix_plan(int64_t maxR) {
  const int bits = bit_length(maxR), passes = (bits + kMaxRadixBits - 1) / kMaxRadixBits;
  return RadixPlan{bits, passes, (bits + passes - 1) / passes};
}
// a table only runs the passes its own ids need; its sorted list ends in key buffer parity[i]
// (more_keys = 1: the pad form, whose largest key is num_entries itself)
inline void fill_passes(const ffh_emb_table* tables, int nt, int rb, uint8_t* npass, uint8_t* parity = nullptr, int more_keys = 0) {
  for (int i = 0; i < nt; i++) {
    const int np = (bit_length(tables[i].num_entries + more_keys) + rb - 1) / rb;
    npass[i] = (uint8_t)np;
    if (parity) parity[i] = (uint8_t)(np & 1);
  }
}

// Tile choices, from the call's lookups over all tables and those of its largest table (one bag size: nt * N and N).
// entries per thread of the sort kernels: enough workgroups to cover the chip, tiles as large as that allows
inline int sort_per_thread(int64_t total, int64_t maxN) {
  const int64_t want = total / (512LL * kSortThreads);
  int e = 1;
  while (e * 2 <= want && e < kSortMaxPerThread) e *= 2;
  // every scatter workgroup walks the table's [tiles][radix] histogram matrix: keep <= 32 tiles per table
  while ((maxN + (int64_t)kSortThreads * e - 1) / ((int64_t)kSortThreads * e) > 32 && e < kSortMaxPerThread) e *= 2;
  return e;
}
inline int reduce_tile(int64_t total) {
  const int64_t want = total / 1024;
  int t = 128;
  while (t * 2 <= want && t < kRedTile) t *= 2;
  return t;
}

// The workspace of a call, byte offsets.  Sized by four totals over the tables: sorted entries (`keys`), sort tiles, FFH_EMB_CHUNK blocks
// (ch0: two level-0 slots each) and FFH_EMB_CHUNK1 blocks (ch1: two level-1 slots and an arrival counter each, one more counter per table).
struct WsLayout { size_t kp_a, kp_b, hist, partial, meta, partial1, meta1, arrive, bstart, total; };
inline void ws_layout(WsLayout& l, size_t keys, size_t sort_tiles, size_t ch0, size_t ch1, int nt, int D) {
  const size_t arr = align_up(keys * sizeof(uint2), 256);
  size_t o = 0;
  l.kp_a = o; o += arr;
  l.kp_b = o; o += arr;
  l.hist = o; o += align_up(sort_tiles * kMaxRadix * sizeof(uint32_t), 256);
  l.partial = o; o += align_up(2 * ch0 * (size_t)D * sizeof(float), 256);
  l.meta = o; o += align_up(2 * ch0 * sizeof(uint2), 256);
  l.partial1 = o; o += align_up(2 * ch1 * (size_t)D * sizeof(float), 256);
  l.meta1 = o; o += align_up(2 * ch1 * sizeof(uint2), 256);
  l.arrive = o; o += align_up((ch1 + (size_t)nt) * sizeof(uint32_t), 256);
  // the bucket form's bucket starts (its nextkey array lives in `hist`, free by then); no ragged kernel uses them yet
  l.bstart = o; o += align_up((size_t)nt * (kMaxRadix + 1) * sizeof(uint32_t), 256);
  l.total = o;
}

// one bag size: every table has N = batch * L entries, nblk sort tiles of 256 * E entries, nchunks / nchunks1 blocks
struct BwdLayout : WsLayout { int E, nblk, nchunks, nchunks1; };
inline BwdLayout bwd_layout(int nt, int L, int D, int64_t batch) {
  BwdLayout l;
  const int64_t N = batch * L;
  l.E = sort_per_thread(nt * N, N);
  const int sort_tile = kSortThreads * l.E;
  l.nblk = (int)((N + sort_tile - 1) / sort_tile);
  l.nchunks = (int)((N + FFH_EMB_CHUNK - 1) / FFH_EMB_CHUNK);
  l.nchunks1 = (int)((N + FFH_EMB_CHUNK1 - 1) / FFH_EMB_CHUNK1);
  ws_layout(l, (size_t)nt * (size_t)N, (size_t)nt * (size_t)l.nblk, (size_t)nt * (size_t)l.nchunks, (size_t)nt * (size_t)l.nchunks1, nt, D);
  return l;
}

// a bag size per table: every table's share sized by its own N_t = batch * L_t (with equal bag sizes: bwd_layout's bytes)
struct BagsLayout : WsLayout {
  BagsGeo g;           // (sort_sh and red_sh set: the tiles the call runs with)
  BagsAt tot;          // totals over the tables; tot.sblk0 = sort tiles, tot.local = reduce tiles
  int64_t maxN;
  int E;
};

inline int log2_of(int v) { int s = 0; while ((1 << s) < v) s++; return s; }

// in_dims checked by the caller: 1 .. kBagMaxL, batch * in_dims[i] < 2^31
inline BagsLayout bags_layout(const int* in_dims, int nt, int D, int64_t batch) {
  BagsLayout l;
  memset(&l, 0, sizeof l);
  int64_t total = 0;
  for (int i = 0; i < nt; i++) {
    l.g.L[i] = (uint16_t)in_dims[i];
    const int64_t N = batch * in_dims[i];
    total += N;
    l.maxN = N > l.maxN ? N : l.maxN;
  }
  l.g.batch = batch; l.g.nt = nt;
  l.E = sort_per_thread(total, l.maxN);
  l.g.sort_sh = log2_of(kSortThreads * l.E);
  l.g.red_sh = log2_of(reduce_tile(total));
  bags_locate(l.g, l.g.red_sh, INT64_MAX, &l.tot);
  ws_layout(l, (size_t)l.tot.key0, (size_t)l.tot.sblk0, (size_t)l.tot.ch0, (size_t)l.tot.ch1, nt, D);
  return l;
}

}  // namespace

// row-wise sharded table: global id -> local id, rows held elsewhere -> the zero row behind the local slice
__global__ __launch_bounds__(256) void emb_localize_kernel(const int64_t* __restrict__ idx, int64_t* __restrict__ local, int64_t n,
                                                           int64_t row_begin, int64_t rows_local) {
  ffh_kernel_prio();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = idx[i] - row_begin;
    local[i] = (r >= 0 && r < rows_local) ? r : rows_local;
  }
}

extern "C" {

int ffh_embedding_bwd_dense(ffh_ctx* c, const int64_t* idx, const float* g, float* wg, int L, int D, int64_t batch,
                            int64_t num_entries, int64_t gld, int aggr, ffh_stream s) {
  ffh_emb_table t{idx, wg, const_cast<float*>(g), num_entries, gld};
  int rc = validate_tables(c, &t, 1, L, D, batch, aggr);
  if (rc) return rc;
  if (batch == 0) return FFH_OK;
  hipLaunchKernelGGL(emb_bwd_dense_kernel, dim3(ffh_grid(batch * D, 256, 4096)), dim3(256), 0, as_stream(s),
                     idx, g, wg, L, D, batch, gld, aggr == FFH_AGGR_MODE_AVG ? 1 : 0);
  FFH_LAUNCH_CHECK(c, "emb_bwd_dense_kernel");
  return FFH_OK;
}

int ffh_embedding_localize_rows(ffh_ctx* c, const int64_t* idx, int64_t* local, int64_t n, int64_t row_begin, int64_t rows_local, ffh_stream s) {
  FFH_REQUIRE(c, n >= 0 && row_begin >= 0 && rows_local >= 0 && ((idx && local) || n == 0), "embedding_localize_rows: bad args");
  if (n == 0) return FFH_OK;
  hipLaunchKernelGGL(emb_localize_kernel, dim3(ffh_grid(n, 256)), dim3(256), 0, as_stream(s), idx, local, n, row_begin, rows_local);
  FFH_LAUNCH_CHECK(c, "embedding_localize_rows");
  return FFH_OK;
}

size_t ffh_embedding_bwd_workspace_bytes(int nt, int L, int D, int64_t batch) {
  if (nt <= 0 || L <= 0 || D <= 0 || batch <= 0) return 0;
  return bwd_layout(nt, L, D, batch).total;
}

}  // extern "C"

// The fused update in two phases: the stable sort of (row id, position) needs the indices only, so a caller that knows them
// early (the DLRM step: at the gather) can run it off the critical path (ffh_embedding_bwd_sort_multi) and do the part that
// needs the output gradients -- segmented reduce, folds, the SGD step -- when they exist (ffh_embedding_bwd_sgd_apply_multi).
// Same launches in the same order on the same workspace: the fused entry is both phases back to back.
// `opt` / `states`: the row rule (ffh_sparse_opt) and the per-table optimizer state it updates; null opt = plain SGD with `lr`
// `b16`: bf16 tables (ff_hip_bf16.h; `tables[i].weight` holds bf16 bits): the rule on uint16_t weight rows (emb_row_rules.h)
struct Bf16Cfg { const ffh_bf16_rounding* r; Bf16Keys keys; };
// the update kernels' translation units, by weight type (emb_reduce.h: the launch table)
typedef bool (*UpdateOfFn)(const UpdateLaunch&);
static constexpr UpdateOfFn kUpdateOf[2] = {emb_update_launch_f32, emb_update_launch_bf16};

// The row rule of an update call: its parameters (OptP), its kind and the argument checks that go with them.  Shared by the uniform entries
// (emb_bwd_phases) and the ragged one (emb_bwd_bags).
struct UpdatePlan { OptP op; int kind; RowRule rule; bool v4; int64_t maxR; };
static int emb_update_rule(ffh_ctx* c, int nt, int D, int64_t batch, float lr, const bool do_apply, const ffh_sparse_opt* opt, const ffh_emb_state* states,
                           const Bf16Cfg* b16, const ffh_lr_state* lr_block, UpdatePlan* plan) {
  OptP op{};
  op.lr = lr;
  if (b16 && do_apply) {
    const ffh_bf16_rounding* r = b16->r;
    if (!r) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_bf16: null ffh_bf16_rounding");
    if (r->mode != FFH_BF16_ROUND_STOCHASTIC && r->mode != FFH_BF16_ROUND_NEAREST) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_bf16: unknown rounding mode");
    if (r->mode == FFH_BF16_ROUND_STOCHASTIC && !r->counter) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_bf16: stochastic rounding needs the update counter");
    op.sr_mode = r->mode; op.sr_seed = r->seed; op.sr_counter = r->counter;
  }
  // (round 6) the rows of a table above 64 MB are read and written back NONTEMPORAL by the plain-SGD apply step: a row of such a table is touched once
  // per launch and must not evict the small tables' rows from L2 / Infinity Cache (as in the gather): 26 tables x 32768 lookups 198.0 -> 188.2 us
  // = 0.83 -> 0.875 of 8 TB/s, interleaved on one box; same bits
  op.nt_rows = (int64_t)FFH_LAB_INT("FFH_EMB_APPLY_NT_MB", 64) * (int64_t)(1 << 20) / ((int64_t)D * (b16 ? 2 : 4));      // (bytes, not rows)
  int kind = FFH_SPARSE_OPT_SGD;
  RowRule rule = RowRule::Sgd;
  if (opt && do_apply) {
    kind = opt->kind;
    if (!row_rule_of(kind, &rule)) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt: unknown ffh_sparse_opt.kind");
    if (b16 && (kind == FFH_SPARSE_OPT_SGD_MOMENTUM || kind == FFH_SPARSE_OPT_ADAM) && nt > FFH_BF16_MAX_STATEFUL_TABLES)      // (Adagrad: one state pointer, the Bf16Keys layout)
      return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_multi_bf16: momentum / Adam take at most FFH_BF16_MAX_STATEFUL_TABLES (32) tables per call");
    op.lr = opt->lr; op.wd = opt->weight_decay; op.mom = opt->momentum; op.nesterov = opt->nesterov ? 1 : 0;
    op.b1 = opt->beta1; op.b2 = opt->beta2; op.eps = opt->epsilon; op.omb1 = 1.0f - opt->beta1; op.omb2 = 1.0f - opt->beta2;
    if (kind == FFH_SPARSE_OPT_SGD && (op.wd != 0.0f || op.mom != 0.0f)) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt: FFH_SPARSE_OPT_SGD takes no weight decay / momentum (use FFH_SPARSE_OPT_SGD_MOMENTUM)");
    if (lr_block) { op.lr = 0.0f; opt_set_lr_src(op, ffh_lr_rate_ptr(lr_block, kind == FFH_SPARSE_OPT_ADAM)); }      // (include/ff_hip_lr.h: opt->lr is ignored)
    const bool need0 = kind == FFH_SPARSE_OPT_ADAM || kind == FFH_SPARSE_OPT_ADAGRAD || kind == FFH_SPARSE_OPT_ROWWISE_ADAGRAD || (kind == FFH_SPARSE_OPT_SGD_MOMENTUM && op.mom > 0.0f);
    for (int i = 0; i < nt && batch > 0; i++) {
      if (need0 && (!states || !states[i].s0)) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt: optimizer state (s0) missing");
      if (kind == FFH_SPARSE_OPT_ADAM && !states[i].s1) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt: optimizer state (s1) missing");
    }
  }
  plan->op = op; plan->kind = kind; plan->rule = rule;
  return FFH_OK;
}
// ... and what depends on the tables: the largest row count and whether every row and state row takes the 16-byte form
static int emb_update_form(ffh_ctx* c, const ffh_emb_table* tables, int nt, int D, const ffh_emb_state* states, UpdatePlan* plan) {
  const int kind = plan->kind;
  const int64_t maxR = max_rows(tables, nt);
  if (maxR > (1LL << 32)) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_sgd_fused: num_entries > 2^32");
  bool v4 = can_vec4(tables, nt, D);
  for (int i = 0; i < nt && v4 && kind != FFH_SPARSE_OPT_SGD && kind != FFH_SPARSE_OPT_ROWWISE_ADAGRAD; i++)      // (row-wise: s0 is one float per row, never read as a vector)
    v4 = (!states[i].s0 || aligned16(states[i].s0)) && (kind == FFH_SPARSE_OPT_ADAGRAD || !states[i].s1 || aligned16(states[i].s1));      // (Adagrad: s1 is unused)
  const int nvec = v4 ? D / 4 : D;
  if ((nvec + 63) / 64 > kMaxChunks * 64) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_sgd_fused: out_dim too large");
  if (kind == FFH_SPARSE_OPT_ROWWISE_ADAGRAD && (nvec + 63) / 64 > kMaxChunks)      // (apply_row_rowwise keeps the row in registers)
    return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_opt: FFH_SPARSE_OPT_ROWWISE_ADAGRAD takes out_dim <= 1024 (16-byte form) / 256 (include/ff_hip_rowwise.h)");
  plan->v4 = v4; plan->maxR = maxR;
  return FFH_OK;
}

// the bf16 keys into a kernel's arguments: beside the s0 / s1 pointers already set (Adam: s1 moves into Bf16AdamKeys)
// (`keys` and `adam` are the same union of the arguments)
static void set_bf16_keys(Bf16Keys& keys, Bf16AdamKeys& adam, const Bf16Cfg& b16, const ffh_emb_state* states, int nt, int kind) {
  if (kind != FFH_SPARSE_OPT_ADAM) { keys = b16.keys; return; }
  Bf16AdamKeys k;
  memset(&k, 0, sizeof k);
  for (int i = 0; i < nt; i++) { k.s1[i] = states[i].s1; k.table[i] = b16.keys.table[i]; k.col0[i] = b16.keys.col0[i]; }
  adam = k;
}
// the rule-related fields of a kernel's arguments (SmallArgs, RedArgs, BagsSmallArgs, BagsRedArgs) ...
template <class Args>
static void set_rule_args(Args& a, const UpdatePlan& plan, const ffh_emb_state* states, int nt, const Bf16Cfg* b16) {
  a.op = plan.op;
  for (int i = 0; i < nt && plan.kind != FFH_SPARSE_OPT_SGD; i++) { a.s0[i] = states[i].s0; a.s1[i] = states[i].s1; }
  if (b16) set_bf16_keys(a.b16, a.b16a, *b16, states, nt, plan.kind);
}
// ... and its level-0 / level-1 slots in the workspace
template <class Args>
static void set_ws_slots(Args& a, char* ws, const WsLayout& lay) {
  a.partial = (float*)(ws + lay.partial); a.meta = (uint2*)(ws + lay.meta);
  a.partial1 = (float*)(ws + lay.partial1); a.meta1 = (uint2*)(ws + lay.meta1);
}

// A call that overwrites the ctx's workspace spoils the ragged sort waiting there (include/ff_hip_bags_sort.h: the note of emb_bwd_bags)
static inline void spoil_bags_sort_note(ffh_ctx* c) {
  if (c->emb_bags_sorted.ws == c->ws) c->emb_bags_sorted.ws = nullptr;
}

// The sort of a call with one bag size, on its workspace.  Set for the LSD form (no bucket digit), every table running its own passes,
// and to clear the apply phase's level-1 slots and arrival counters in pass 0.
struct SortSetup { SortArgs sa; uint2* kbuf[2]; dim3 grid; };
static void sort_setup(SortSetup& st, const ffh_emb_table* tables, int nt, int64_t N, const BwdLayout& lay, char* ws, int rb, uint8_t* parity) {
  SortArgs& sa = st.sa;
  memset(&sa, 0, sizeof sa);
  for (int i = 0; i < nt; i++) sa.idx[i] = tables[i].idx;
  fill_passes(tables, nt, rb, sa.npass, parity);
  sa.bstart = (uint32_t*)(ws + lay.bstart);
  sa.hist = (uint32_t*)(ws + lay.hist);
  sa.N = N; sa.nblk = lay.nblk; sa.bits = rb;
  sa.clear[0] = (uint32_t*)(ws + lay.meta1); sa.nclear[0] = 4 * lay.nchunks1;     // uint2 slots, two per 1024-block
  sa.clear[1] = (uint32_t*)(ws + lay.arrive); sa.nclear[1] = lay.nchunks1 + 1;
  st.kbuf[0] = (uint2*)(ws + lay.kp_a); st.kbuf[1] = (uint2*)(ws + lay.kp_b);
  st.grid = dim3((unsigned)lay.nblk, (unsigned)nt);
}
// the stable passes of the sort, one digit of rb bits each: pass p reads buffer p % 2 (pass 0: the int64 ids) and writes buffer (p + 1) % 2
static void launch_sort_passes(SortSetup& st, int passes, int rb, int E, ffh_stream s) {
  SortArgs& sa = st.sa;
  const dim3 sgrid = st.grid;
  for (int p = 0; p < passes; p++) {
    sa.shift = p * rb;
    sa.pass = p;
    sa.src = st.kbuf[p & 1];
    sa.dst = st.kbuf[(p + 1) & 1];
#define FFH_SORT_PASS(FIRSTV, EV)                                                                              \
    hipLaunchKernelGGL((radix_hist_kernel<FIRSTV, EV>), sgrid, dim3(kSortThreads), 0, as_stream(s), sa);      \
    hipLaunchKernelGGL((radix_scatter_kernel<FIRSTV, EV>), sgrid, dim3(kSortThreads), 0, as_stream(s), sa);
    if (p == 0) {
      switch (E) { case 1: FFH_SORT_PASS(true, 1) break; case 2: FFH_SORT_PASS(true, 2) break; case 4: FFH_SORT_PASS(true, 4) break; default: FFH_SORT_PASS(true, 8) break; }
    } else {
      switch (E) { case 1: FFH_SORT_PASS(false, 1) break; case 2: FFH_SORT_PASS(false, 2) break; case 4: FFH_SORT_PASS(false, 4) break; default: FFH_SORT_PASS(false, 8) break; }
    }
#undef FFH_SORT_PASS
  }
}

static int emb_bwd_phases(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int D, int64_t batch,
                          int aggr, float lr, ffh_stream s, const bool do_sort, const bool do_apply,
                          const ffh_sparse_opt* opt = nullptr, const ffh_emb_state* states = nullptr, const Bf16Cfg* b16 = nullptr,
                          const ffh_lr_state* lr_block = nullptr) {
  int rc = validate_tables(c, tables, nt, L, D, batch, aggr);
  if (rc) return rc;
  UpdatePlan plan;
  rc = emb_update_rule(c, nt, D, batch, lr, do_apply, opt, states, b16, lr_block, &plan);
  if (rc) return rc;
  if (nt == 0 || batch == 0) return FFH_OK;
  const int64_t N = batch * L;
  if (N >= (1LL << 31)) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_sgd_fused: batch*in_dim >= 2^31");
  rc = emb_update_form(c, tables, nt, D, states, &plan);
  if (rc) return rc;
  const BwdLayout lay = bwd_layout(nt, L, D, batch);
  if (!c->ws || c->ws_bytes < lay.total) return ffh_fail(c, FFH_ERR_WORKSPACE, "embedding_bwd_sgd_fused: workspace too small (ffh_embedding_bwd_workspace_bytes)");
  char* ws = (char*)c->ws;
  if (!aligned16(ws)) return ffh_fail(c, FFH_ERR_WORKSPACE, "embedding_bwd_sgd_fused: workspace must be 16-byte aligned");
  // The apply phase CONSUMES what the sort phase left in the workspace: besides the sorted list, the arrival counters and level-1
  // slots that only the sort's first histogram pass clears -- a second apply on the same sort would find them used (no workgroup
  // would be "last", rows whose runs cross tiles would silently miss their update).  The two-call form is therefore one-shot: the
  // sort notes (workspace, shape) in the ctx, the apply requires and clears that note; the fused call needs no note but spoils one
  // that sits on the workspace it overwrites.
  const int64_t sig[4] = {nt, L, D, batch};
  if (do_sort) spoil_bags_sort_note(c);      // (a ragged note never satisfies a uniform apply, and the reverse: emb_bwd_bags)
  if (do_sort && do_apply) {
    if (c->emb_sorted_ws == c->ws) c->emb_sorted_ws = nullptr;
  } else if (do_sort) {
    c->emb_sorted_ws = c->ws;
    memcpy(c->emb_sorted_sig, sig, sizeof sig);
  } else {
    if (c->emb_sorted_ws != c->ws || memcmp(c->emb_sorted_sig, sig, sizeof sig) != 0)
      return ffh_fail(c, FFH_ERR_WORKSPACE, "embedding_bwd_sgd_apply_multi: no fresh ffh_embedding_bwd_sort_multi of the same tables / batch on this ctx's "
                                           "workspace (the apply phase consumes the sort: one apply per sort)");
    c->emb_sorted_ws = nullptr;
  }
  // radix plan: digits of <= 9 bits covering bit_length(maxR-1); a table only runs the passes its own ids need
  RadixPlan rp = radix_plan(plan.maxR);
  const int avg = aggr == FFH_AGGR_MODE_AVG ? 1 : 0;

  if (N <= kSmallMax) {
    // small-batch path: one launch, one workgroup per table (see emb_sgd_small_kernel): the sort lives inside it
    snprintf(c->emb_route, sizeof c->emb_route, "small");
    if (!do_apply) return FFH_OK;
    SmallArgs sm;
    memset(&sm, 0, sizeof sm);
    for (int i = 0; i < nt; i++) sm.t[i] = tables[i];
    fill_passes(tables, nt, rp.rb, sm.npass);
    sm.kp = (uint2*)(ws + lay.kp_a);
    set_ws_slots(sm, ws, lay);
    sm.N = N; sm.nch0 = lay.nchunks; sm.nch1 = lay.nchunks1; sm.rb = rp.rb; sm.L = L; sm.D = D; sm.avg = avg;
    set_rule_args(sm, plan, states, nt, b16);
    int tile = (int)((N + kSmallRedParts - 1) / kSmallRedParts);          // one tile per 256-thread team
    tile = (tile + FFH_EMB_CHUNK - 1) / FFH_EMB_CHUNK * FFH_EMB_CHUNK;
    sm.tile = tile < FFH_EMB_CHUNK ? FFH_EMB_CHUNK : tile;
    if (!kUpdateOf[b16 ? 1 : 0](UpdateLaunch{plan.rule, plan.v4, lr_block != nullptr, false, &sm, nullptr, dim3(nt), as_stream(s)}))
      return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd: no small-batch kernel for this rule / weight type");
    FFH_LAUNCH_CHECK(c, "emb_sgd_small_kernel");
    return FFH_OK;
  }
  // bucket form (msd_window): one pass on the top digit, the rest inside the apply launch.  Where the LSD form would need >= 2 passes
  // and a bucket averages <= 128 entries (N <= 64 K at 512 buckets); the digit: ~32 entries per bucket, 4 .. 9 bits
  static const int msd_env = FFH_LAB_INT("FFH_EMB_MSD", 1);          // A/B switch: 0 = never, 1 = by shape, 2 = wherever it is valid
  static const int msd_max_tables = FFH_LAB_INT("FFH_EMB_MSD_MAX_TABLES", FFH_MAX_TABLES);      // (first rule: <= 8 tables; at 26 tables x 32768 lookups the form takes 196 instead of 238 us)
  int mb = 4;
  while (mb < kMaxRadixBits && (N >> (mb + 1)) >= 32) mb++;
  const bool msd = msd_env != 0 && rp.bits > kMaxRadixBits && N <= 65536 && (N >> mb) <= 128 && (msd_env == 2 || nt <= msd_max_tables) &&
                   (size_t)lay.nblk * kMaxRadix >= (size_t)lay.nchunks1;
  if (msd) { rp.passes = 1; rp.rb = mb; }
  if (msd) snprintf(c->emb_route, sizeof c->emb_route, "buckets:bits=%d", rp.rb); else snprintf(c->emb_route, sizeof c->emb_route, "lsd:passes=%d", rp.passes);

  SortSetup st;
  RedArgs ra;
  memset(&ra, 0, sizeof ra);
  sort_setup(st, tables, nt, N, lay, ws, rp.rb, ra.parity);
  if (msd) {      // the bucket form: one pass for every table, on its top digit -- in place of the LSD passes sort_setup filled in
    st.sa.msd = 1;
    for (int i = 0; i < nt; i++) {
      const int tb = bit_length(tables[i].num_entries);
      st.sa.npass[i] = ra.parity[i] = 1;
      st.sa.shift_t[i] = ra.shift_t[i] = (uint8_t)(tb > rp.rb ? tb - rp.rb : 0);
    }
  }
  ra.bstart = st.sa.bstart; ra.nextkey = (uint32_t*)(ws + lay.hist); ra.radix = 1 << rp.rb;
  if (do_sort) launch_sort_passes(st, rp.passes, rp.rb, lay.E, s);
  FFH_LAUNCH_CHECK(c, "radix sort");
  if (!do_apply) return FFH_OK;

  for (int i = 0; i < nt; i++) ra.t[i] = tables[i];
  ra.kp[0] = st.kbuf[0]; ra.kp[1] = st.kbuf[1];
  ra.tile = reduce_tile(nt * N);
  {
    static const int msd_tile = FFH_LAB_INT("FFH_EMB_MSD_TILE", 0);      // A/B switch: the bucket form's tile
    if (msd && msd_tile >= 128 && msd_tile <= kRedTile && (msd_tile & (msd_tile - 1)) == 0) ra.tile = msd_tile;
  }
  set_ws_slots(ra, ws, lay);
  ra.arrive = (uint32_t*)(ws + lay.arrive);
  ra.N = N; ra.nchunks = lay.nchunks; ra.nchunks1 = lay.nchunks1; ra.L = L; ra.D = D; ra.avg = avg;
  set_rule_args(ra, plan, states, nt, b16);
  // segmented sums + both folds (32-block partials -> 1024-block partials -> row totals) + the SGD step: one launch
  dim3 rgrid((unsigned)((N + ra.tile - 1) / ra.tile), (unsigned)nt);
  if (!kUpdateOf[b16 ? 1 : 0](UpdateLaunch{plan.rule, plan.v4, lr_block != nullptr, msd, nullptr, &ra, rgrid, as_stream(s)}))
    return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd: no reduce kernel for this rule / weight type");
  FFH_LAUNCH_CHECK(c, "emb_sgd_reduce/fold");
  return FFH_OK;
}

extern "C" {

int ffh_embedding_bwd_sgd_fused_multi(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int D, int64_t batch,
                                      int aggr, float lr, ffh_stream s) {
  return emb_bwd_phases(c, tables, nt, L, D, batch, aggr, lr, s, true, true);
}

int ffh_embedding_bwd_sort_multi(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int D, int64_t batch, ffh_stream s) {
  return emb_bwd_phases(c, tables, nt, L, D, batch, FFH_AGGR_MODE_SUM, 0.0f, s, true, false);
}

int ffh_embedding_bwd_sgd_apply_multi(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int D, int64_t batch,
                                      int aggr, float lr, ffh_stream s) {
  return emb_bwd_phases(c, tables, nt, L, D, batch, aggr, lr, s, false, true);
}

int ffh_embedding_bwd_opt_fused_multi(ffh_ctx* c, const ffh_emb_table* tables, const ffh_emb_state* states, int nt, int L, int D, int64_t batch,
                                      int aggr, const ffh_sparse_opt* opt, ffh_stream s) {
  if (!opt) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_fused_multi: null ffh_sparse_opt");
  return emb_bwd_phases(c, tables, nt, L, D, batch, aggr, opt->lr, s, true, true, opt, states);
}

int ffh_embedding_bwd_opt_apply_multi(ffh_ctx* c, const ffh_emb_table* tables, const ffh_emb_state* states, int nt, int L, int D, int64_t batch,
                                      int aggr, const ffh_sparse_opt* opt, ffh_stream s) {
  if (!opt) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_apply_multi: null ffh_sparse_opt");
  return emb_bwd_phases(c, tables, nt, L, D, batch, aggr, opt->lr, s, false, true, opt, states);
}

// include/ff_hip_lr.h: the row rule's rate read from a state block in device memory
int ffh_embedding_bwd_opt_fused_multi_lr(ffh_ctx* c, const ffh_emb_table* tables, const ffh_emb_state* states, int nt, int L, int D, int64_t batch,
                                         int aggr, const ffh_sparse_opt* opt, const ffh_lr_state* block, ffh_stream s) {
  if (!opt || !block) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_fused_multi_lr: null ffh_sparse_opt or ffh_lr_state");
  return emb_bwd_phases(c, tables, nt, L, D, batch, aggr, 0.0f, s, true, true, opt, states, nullptr, block);
}

int ffh_embedding_bwd_opt_apply_multi_lr(ffh_ctx* c, const ffh_emb_table* tables, const ffh_emb_state* states, int nt, int L, int D, int64_t batch,
                                         int aggr, const ffh_sparse_opt* opt, const ffh_lr_state* block, ffh_stream s) {
  if (!opt || !block) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_apply_multi_lr: null ffh_sparse_opt or ffh_lr_state");
  return emb_bwd_phases(c, tables, nt, L, D, batch, aggr, 0.0f, s, false, true, opt, states, nullptr, block);
}

int ffh_embedding_bwd_sgd_fused(ffh_ctx* c, const int64_t* idx, const float* g, float* weight, int L, int D, int64_t batch,
                                int64_t num_entries, int64_t gld, int aggr, float lr, ffh_stream s) {
  ffh_emb_table t{idx, weight, const_cast<float*>(g), num_entries, gld};
  return ffh_embedding_bwd_sgd_fused_multi(c, &t, 1, L, D, batch, aggr, lr, s);
}

}  // extern "C"

// fold_sum.h: the sort alone, complete (no bucket form, no one-launch form), for a caller that reduces the list itself.  Every table runs
// the passes its own ids need; its result lies in buffer (passes % 2).
int ffh_emb::emb_sort_full(ffh_ctx* c, const ffh_emb_table* tables, int nt, int L, int D, int64_t batch, ffh_stream s, FullSort* out) {
  const int64_t N = batch * L;
  const BwdLayout lay = bwd_layout(nt, L, D, batch);
  char* ws = (char*)c->ws;
  if (c->emb_sorted_ws == c->ws) c->emb_sorted_ws = nullptr;
  spoil_bags_sort_note(c);
  const int64_t maxR = max_rows(tables, nt);
  if (maxR > (1LL << 32)) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "fold_segment_sum: num_entries > 2^32");
  const RadixPlan rp = radix_plan(maxR);
  SortSetup st;
  uint8_t parity[FFH_MAX_TABLES];
  sort_setup(st, tables, nt, N, lay, ws, rp.rb, parity);
  st.sa.nclear[0] = st.sa.nclear[1] = 0;      // (this caller has no counters to clear)
  for (int i = 0; i < nt; i++) out->kp[i] = st.kbuf[parity[i]] + (int64_t)i * N;
  launch_sort_passes(st, rp.passes, rp.rb, lay.E, s);
  FFH_LAUNCH_CHECK(c, "radix sort");
  out->partial0 = (float*)(ws + lay.partial);
  out->partial1 = (float*)(ws + lay.partial1);
  out->passes = rp.passes;
  return FFH_OK;
}

// ---------------------------------------------------------------------------
// bf16 tables (include/ff_hip_bf16.h): the fp32 launchers with 16-bit weight rows, the numerics of include/ffh_bf16.h
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void init_uniform_bf16_kernel(uint16_t* __restrict__ p, int64_t n, uint64_t seed, float lo, float hi) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    p[i] = ffh_bf16_rne(ffh_uniform(ffh_hash(seed, (uint64_t)i), lo, hi));
}

__global__ void bf16_counter_advance_kernel(uint64_t* counter) { *counter = *counter + 1; }

static int emb_bwd_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, int nt, int L, int D, int64_t batch, int aggr, float lr,
                        const ffh_bf16_rounding* r, ffh_stream s, bool do_sort, bool do_apply,
                        const ffh_sparse_opt* opt = nullptr, const ffh_emb_state* states = nullptr, const ffh_lr_state* lr_block = nullptr) {
  ffh_emb_table t[FFH_MAX_TABLES];
  Bf16Cfg cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.r = r;
  const int rc = bf16_tables(c, tables, nt, t, &cfg.keys);
  if (rc) return rc;
  return emb_bwd_phases(c, t, nt, L, D, batch, aggr, lr, s, do_sort, do_apply, opt, states, &cfg, lr_block);
}

extern "C" {

int ffh_bf16_abi_version(void) { return FFH_BF16_ABI_VERSION; }

int ffh_embedding_bwd_sgd_fused_multi_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, int nt, int L, int D, int64_t batch,
                                           int aggr, float lr, const ffh_bf16_rounding* r, ffh_stream s) {
  return emb_bwd_bf16(c, tables, nt, L, D, batch, aggr, lr, r, s, true, true);
}

int ffh_embedding_bwd_sort_multi_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, int nt, int L, int D, int64_t batch, ffh_stream s) {
  return emb_bwd_bf16(c, tables, nt, L, D, batch, FFH_AGGR_MODE_SUM, 0.0f, nullptr, s, true, false);
}

int ffh_embedding_bwd_sgd_apply_multi_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, int nt, int L, int D, int64_t batch,
                                           int aggr, float lr, const ffh_bf16_rounding* r, ffh_stream s) {
  return emb_bwd_bf16(c, tables, nt, L, D, batch, aggr, lr, r, s, false, true);
}

int ffh_embedding_bwd_opt_fused_multi_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, const ffh_emb_state* states, int nt, int L, int D,
                                           int64_t batch, int aggr, const ffh_sparse_opt* opt, const ffh_bf16_rounding* r, ffh_stream s) {
  if (!opt) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_fused_multi_bf16: null ffh_sparse_opt");
  return emb_bwd_bf16(c, tables, nt, L, D, batch, aggr, opt->lr, r, s, true, true, opt, states);
}

int ffh_embedding_bwd_opt_apply_multi_bf16(ffh_ctx* c, const ffh_emb_table_bf16* tables, const ffh_emb_state* states, int nt, int L, int D,
                                           int64_t batch, int aggr, const ffh_sparse_opt* opt, const ffh_bf16_rounding* r, ffh_stream s) {
  if (!opt) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_apply_multi_bf16: null ffh_sparse_opt");
  return emb_bwd_bf16(c, tables, nt, L, D, batch, aggr, opt->lr, r, s, false, true, opt, states);
}

int ffh_embedding_bwd_opt_fused_multi_bf16_lr(ffh_ctx* c, const ffh_emb_table_bf16* tables, const ffh_emb_state* states, int nt, int L, int D,
                                              int64_t batch, int aggr, const ffh_sparse_opt* opt, const ffh_bf16_rounding* r, const ffh_lr_state* block,
                                              ffh_stream s) {
  if (!opt || !block) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_fused_multi_bf16_lr: null ffh_sparse_opt or ffh_lr_state");
  return emb_bwd_bf16(c, tables, nt, L, D, batch, aggr, 0.0f, r, s, true, true, opt, states, block);
}

int ffh_embedding_bwd_opt_apply_multi_bf16_lr(ffh_ctx* c, const ffh_emb_table_bf16* tables, const ffh_emb_state* states, int nt, int L, int D,
                                              int64_t batch, int aggr, const ffh_sparse_opt* opt, const ffh_bf16_rounding* r, const ffh_lr_state* block,
                                              ffh_stream s) {
  if (!opt || !block) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_opt_apply_multi_bf16_lr: null ffh_sparse_opt or ffh_lr_state");
  return emb_bwd_bf16(c, tables, nt, L, D, batch, aggr, 0.0f, r, s, false, true, opt, states, block);
}

int ffh_init_uniform_bf16(ffh_ctx* c, uint16_t* p, int64_t n, uint64_t seed, float lo, float hi, ffh_stream s) {
  FFH_REQUIRE(c, n >= 0 && (p || n == 0), "init_uniform_bf16: bad args");
  if (n == 0) return FFH_OK;
  hipLaunchKernelGGL(init_uniform_bf16_kernel, dim3(ffh_grid(n, 256, 8192)), dim3(256), 0, as_stream(s), p, n, seed, lo, hi);
  FFH_LAUNCH_CHECK(c, "init_uniform_bf16");
  return FFH_OK;
}

int ffh_bf16_counter_advance(ffh_ctx* c, uint64_t* counter, ffh_stream s) {
  FFH_REQUIRE(c, counter != nullptr, "bf16_counter_advance: null counter");
  hipLaunchKernelGGL(bf16_counter_advance_kernel, dim3(1), dim3(1), 0, as_stream(s), counter);
  FFH_LAUNCH_CHECK(c, "bf16_counter_advance");
  return FFH_OK;
}

int ffh_rowwise_abi_version(void) { return FFH_ROWWISE_ABI_VERSION; }      // include/ff_hip_rowwise.h: the row rule lives in this file

}  // extern "C"

// ---------------------------------------------------------------------------
// include/ff_hip_bags_update.h: the fused update with a bag size per table.  One call, the kernels of emb_bags_update.h.
// ---------------------------------------------------------------------------
namespace {

// FFH_OK, or the code the entry returns for these bag sizes (no message: the callers add their own)
inline int bags_dims_check(const int* in_dims, int nt, int64_t batch) {
  if (nt < 0 || nt > FFH_BAGS_UPDATE_MAX_TABLES || (nt > 0 && !in_dims) || batch < 0) return FFH_ERR_BAD_ARG;
  for (int i = 0; i < nt; i++)
    if (in_dims[i] < 1) return FFH_ERR_BAD_ARG;
  for (int i = 0; i < nt; i++) {
    if (in_dims[i] > kBagMaxL) return FFH_ERR_UNSUPPORTED;
    if (batch * (int64_t)in_dims[i] >= (1LL << 31)) return FFH_ERR_UNSUPPORTED;
  }
  return FFH_OK;
}

typedef bool (*BagsUpdateOfFn)(const BagsUpdateLaunch&);
constexpr BagsUpdateOfFn kBagsUpdateOf[3][2] = {{emb_bags_update_launch_f32, emb_bags_update_launch_bf16},      // [BagsForm][bf16 rows]
                                                {emb_pad_update_launch_f32, emb_pad_update_launch_bf16},
                                                {emb_padmean_update_launch_f32, emb_padmean_update_launch_bf16}};
// the form of a ragged update call: plain, the pad form (include/ff_hip_pad.h) or the pad form with a mean over the lookups that are there
// (include/ff_hip_pad_mean.h)
enum BagsForm { kBagsPlain = 0, kBagsPad = 1, kBagsPadMean = 2 };

// The mean form's counts: one uint16 per (table, bag), [table][batch], in a region behind the ragged layout -- the sort phase, which sizes and
// writes only that layout, never touches it.
inline size_t padmean_cnt_offset(const BagsLayout& lay) { return (lay.total + 15) & ~(size_t)15; }
inline size_t padmean_total(const BagsLayout& lay, int nt, int64_t batch) { return padmean_cnt_offset(lay) + (((size_t)nt * (size_t)batch * 2 + 15) & ~(size_t)15); }

// the sort phase alone reads idx and num_entries only (include/ff_hip_bags_sort.h): validate_tables without the weight / io / ld checks
inline int validate_sort_tables(ffh_ctx* c, const ffh_emb_table* t, int nt, int D, int64_t batch) {
  if (D <= 0) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding: bad dims");
  for (int i = 0; i < nt; i++) {
    if (batch > 0 && !t[i].idx) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding: null pointer");
    if (t[i].num_entries <= 0) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding: ld < out_dim or num_entries <= 0");
  }
  return FFH_OK;
}

// The ragged update in the two phases of emb_bwd_phases: do_sort && do_apply is the fused entry, do_sort alone and do_apply alone are the pair of
// include/ff_hip_bags_sort.h.  Same launches in the same order on the same workspace.
// `pad` (include/ff_hip_pad.h): an id < 0 is no lookup.  Pass 0 of the sort loads it as key num_entries, so the radix plan covers one more key
// per table, and the apply kernels drop that key's segment; the layout, the grids and the workspace are those of the call without pads.
// kBagsPadMean (include/ff_hip_pad_mean.h; apply and fused only -- the sort is the pad form's): the apply phase first counts every bag's real
// lookups into the region behind the layout (one small launch), and its kernels divide each gradient row by its bag's count.
int emb_bwd_bags(ffh_ctx* c, const ffh_emb_table* tables, const int* in_dims, int nt, int D, int64_t batch, int aggr, float lr, ffh_stream s,
                 const bool do_sort, const bool do_apply,
                 const ffh_sparse_opt* opt, const ffh_emb_state* states, const Bf16Cfg* b16, const ffh_lr_state* lr_block, const BagsForm form) {
  const bool pad = form != kBagsPlain, mean = form == kBagsPadMean;
  int rc = bags_dims_check(in_dims, nt, batch);
  if (rc == FFH_ERR_BAD_ARG) return ffh_fail(c, rc, "embedding_bwd_fused_multi_bags: ntables out of range, null in_dims or in_dims[i] < 1");
  if (rc) return ffh_fail(c, rc, "embedding_bwd_fused_multi_bags: in_dims[i] > FFH_BAGS_MAX_IN_DIM (65535) or batch*in_dims[i] >= 2^31");
  rc = do_apply ? validate_tables(c, tables, nt, 1, D, batch, aggr) : validate_sort_tables(c, tables, nt, D, batch);
  if (rc) return rc;
  if (pad && !mean && aggr == FFH_AGGR_MODE_AVG)      // (a mean over the lookups that are there needs each bag's count in the apply phase: include/ff_hip_pad_mean.h)
    return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_fused_multi_bags_pad: FFH_AGGR_MODE_AVG is not supported with pad ids");
  if (mean && aggr != FFH_AGGR_MODE_AVG)
    return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_fused_multi_bags_pad_mean: aggr must be FFH_AGGR_MODE_AVG (for a sum call ffh_embedding_bwd_fused_multi_bags_pad / "
                                        "ffh_embedding_bwd_apply_multi_bags_pad)");
  UpdatePlan plan;
  rc = emb_update_rule(c, nt, D, batch, lr, do_apply, opt, states, b16, lr_block, &plan);
  if (rc) return rc;
  if (nt == 0 || batch == 0) return FFH_OK;
  rc = emb_update_form(c, tables, nt, D, states, &plan);      // (the sort phase: the plain rule, no state is looked at; it keeps maxR)
  if (rc) return rc;
  if (pad && plan.maxR > 0xFFFFFFFELL)      // (the pad key is num_entries; 0xFFFFFFFF is the reduce kernel's "no key")
    return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_fused_multi_bags_pad: num_entries > 2^32 - 2");
  const BagsLayout lay = bags_layout(in_dims, nt, D, batch);
  if (!c->ws || c->ws_bytes < lay.total) return ffh_fail(c, FFH_ERR_WORKSPACE, "embedding_bwd_fused_multi_bags: workspace too small (ffh_embedding_bwd_bags_workspace_bytes)");
  if (mean && c->ws_bytes < padmean_total(lay, nt, batch))
    return ffh_fail(c, FFH_ERR_WORKSPACE, "embedding_bwd_fused_multi_bags_pad_mean: workspace too small (ffh_embedding_bwd_bags_pad_mean_workspace_bytes)");
  char* ws = (char*)c->ws;
  if (!aligned16(ws)) return ffh_fail(c, FFH_ERR_WORKSPACE, "embedding_bwd_fused_multi_bags: workspace must be 16-byte aligned");
  // One-shot, as in emb_bwd_phases: the apply phase consumes the sorted lists, the level-1 slots and the arrival counters that only the sort's
  // pass 0 clears.  The sort notes the workspace and everything the layout and the lists depend on; the apply requires that note and clears it.
  // Either phase overwrites what a uniform sort left on this workspace, and a uniform fused call or sort spoils this note (spoil_bags_sort_note):
  // a note of one kind never serves the other kind's apply.
  if (do_sort) {
    if (c->emb_sorted_ws == c->ws) c->emb_sorted_ws = nullptr;      // (as the uniform fused call: a pending sort on this workspace is overwritten)
    spoil_bags_sort_note(c);
  }
  if (do_sort != do_apply) {
    ffh_ctx::bags_sort_note note;
    memset(&note, 0, sizeof note);
    note.ws = c->ws; note.nt = nt; note.D = D; note.batch = batch; note.pad = pad ? 1 : 0;      // (a pad sort serves a pad apply only, and the reverse)
    for (int i = 0; i < nt; i++) { note.rows[i] = tables[i].num_entries; note.idx[i] = tables[i].idx; note.L[i] = (uint16_t)in_dims[i]; }
    if (do_sort) {
      c->emb_bags_sorted = note;
    } else {
      if (memcmp(&c->emb_bags_sorted, &note, sizeof note) != 0)
        return ffh_fail(c, FFH_ERR_WORKSPACE, "embedding_bwd_apply_multi_bags: no fresh ffh_embedding_bwd_sort_multi_bags of the same tables / bag sizes / batch on this "
                                             "ctx's workspace (the apply phase consumes the sort: one apply per sort)");
      c->emb_bags_sorted.ws = nullptr;
    }
  }
  const int more_keys = pad ? 1 : 0;
  const RadixPlan rp = radix_plan(plan.maxR + more_keys);
  const int avg = aggr == FFH_AGGR_MODE_AVG ? 1 : 0;
  uint16_t* const cnt = mean ? (uint16_t*)(ws + padmean_cnt_offset(lay)) : nullptr;
  auto count_bags = [&]() {      // (the mean form's apply phase, ahead of its kernels on the stream)
    BagsCountArgs ca;
    memset(&ca, 0, sizeof ca);
    for (int i = 0; i < nt; i++) { ca.idx[i] = tables[i].idx; ca.L[i] = (uint16_t)in_dims[i]; }
    ca.cnt = cnt; ca.batch = batch; ca.nt = nt;
    emb_padmean_count(ca, as_stream(s));
  };

  if (lay.maxN <= kSmallMax) {
    snprintf(c->emb_route, sizeof c->emb_route, mean ? "bags:small:pad:mean" : pad ? "bags:small:pad" : "bags:small");
    if (!do_apply) return FFH_OK;      // (the sort lives inside the one launch: the sort call only leaves the note)
    if (mean) count_bags();
    BagsSmallArgs sm;
    memset(&sm, 0, sizeof sm);
    for (int i = 0; i < nt; i++) sm.t[i] = tables[i];
    fill_passes(tables, nt, rp.rb, sm.npass, nullptr, more_keys);
    sm.kp = (uint2*)(ws + lay.kp_a);
    set_ws_slots(sm, ws, lay);
    sm.rb = rp.rb; sm.D = D; sm.avg = avg; sm.g = lay.g; sm.cnt = cnt;
    set_rule_args(sm, plan, states, nt, b16);
    if (!kBagsUpdateOf[form][b16 ? 1 : 0](BagsUpdateLaunch{plan.rule, plan.v4, lr_block != nullptr, &sm, nullptr, dim3((unsigned)nt), as_stream(s)}))
      return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_fused_multi_bags: no small-route kernel for this rule / weight type");
    FFH_LAUNCH_CHECK(c, "emb_bags_small_kernel");
    return FFH_OK;
  }

  snprintf(c->emb_route, sizeof c->emb_route, mean ? "bags:lsd:passes=%d:pad:mean" : pad ? "bags:lsd:passes=%d:pad" : "bags:lsd:passes=%d", rp.passes);
  BagsSortArgs sa;
  memset(&sa, 0, sizeof sa);
  BagsRedArgs ra;
  memset(&ra, 0, sizeof ra);
  for (int i = 0; i < nt; i++) { sa.idx[i] = tables[i].idx; ra.t[i] = tables[i]; sa.padkey[i] = (uint32_t)tables[i].num_entries; }
  fill_passes(tables, nt, rp.rb, sa.npass, ra.parity, more_keys);
  sa.hist = (uint32_t*)(ws + lay.hist);
  sa.bits = rp.rb; sa.g = lay.g;
  sa.clear[0] = (uint32_t*)(ws + lay.meta1); sa.nclear[0] = (int)(4 * lay.tot.ch1);      // uint2 slots, two per 1024-block
  sa.clear[1] = (uint32_t*)(ws + lay.arrive); sa.nclear[1] = (int)(lay.tot.ch1 + nt);
  uint2* kbuf[2] = {(uint2*)(ws + lay.kp_a), (uint2*)(ws + lay.kp_b)};
  const dim3 sgrid((unsigned)lay.tot.sblk0), rgrid((unsigned)lay.tot.local);      // the flat map: every table's own tiles
  for (int p = 0; do_sort && p < rp.passes; p++) {
    sa.shift = p * rp.rb; sa.pass = p;
    sa.src = kbuf[p & 1]; sa.dst = kbuf[(p + 1) & 1];
    if (!(pad && p == 0 ? emb_pad_sort_first_pass(sa, lay.E, sgrid, as_stream(s)) : emb_bags_sort_pass(sa, p == 0, lay.E, sgrid, as_stream(s)))) return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_fused_multi_bags: no sort kernel");
  }
  FFH_LAUNCH_CHECK(c, "bags radix sort");
  if (!do_apply) return FFH_OK;

  if (mean) count_bags();
  ra.kp[0] = kbuf[0]; ra.kp[1] = kbuf[1];
  set_ws_slots(ra, ws, lay);
  ra.arrive = (uint32_t*)(ws + lay.arrive);
  ra.D = D; ra.avg = avg; ra.g = lay.g; ra.cnt = cnt;
  set_rule_args(ra, plan, states, nt, b16);
  if (!kBagsUpdateOf[form][b16 ? 1 : 0](BagsUpdateLaunch{plan.rule, plan.v4, lr_block != nullptr, nullptr, &ra, rgrid, as_stream(s)}))
    return ffh_fail(c, FFH_ERR_UNSUPPORTED, "embedding_bwd_fused_multi_bags: no reduce kernel for this rule / weight type");
  FFH_LAUNCH_CHECK(c, "emb_bags_reduce/fold");
  return FFH_OK;
}

}  // namespace

extern "C" {

int ffh_bags_update_abi_version(void) { return FFH_BAGS_UPDATE_ABI_VERSION; }
size_t ffh_bags_update_kernarg_bytes(void) { return kBagsKernargBytes; }

size_t ffh_embedding_bwd_bags_workspace_bytes(const int* in_dims, int nt, int D, int64_t batch) {
  if (nt <= 0 || D <= 0 || batch <= 0 || bags_dims_check(in_dims, nt, batch) != FFH_OK) return 0;
  return bags_layout(in_dims, nt, D, batch).total;
}

// the descriptor of the three ragged entries: the fused call (do_sort && do_apply) and the pair of include/ff_hip_bags_sort.h.  The sort phase
// takes the fields it reads (tables, in_dims, ntables, out_dim, batch) and nothing else.
static int emb_bwd_bags_desc(ffh_ctx* c, const ffh_bags_update* u, ffh_stream s, const bool do_sort, const bool do_apply, const BagsForm pad = kBagsPlain) {
  if (!u) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_fused_multi_bags: null descriptor");
  if ((u->tables != nullptr) == (u->tables_bf16 != nullptr)) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_fused_multi_bags: exactly one of tables / tables_bf16");
  if (do_apply && u->lr_block && !u->opt) return ffh_fail(c, FFH_ERR_BAD_ARG, "embedding_bwd_fused_multi_bags: lr_block needs opt");
  const int aggr = do_apply ? u->aggr : FFH_AGGR_MODE_SUM;
  const float lr = do_apply ? u->lr : 0.0f;
  const ffh_sparse_opt* opt = do_apply ? u->opt : nullptr;
  const ffh_emb_state* states = do_apply ? u->states : nullptr;
  const ffh_lr_state* lr_block = do_apply ? u->lr_block : nullptr;
  if (u->tables) return emb_bwd_bags(c, u->tables, u->in_dims, u->ntables, u->out_dim, u->batch, aggr, lr, s, do_sort, do_apply, opt, states, nullptr, lr_block, pad);
  ffh_emb_table t[FFH_MAX_TABLES];
  Bf16Cfg cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.r = do_apply ? u->rounding : nullptr;
  const int rc = bf16_tables(c, u->tables_bf16, u->ntables, t, &cfg.keys);
  if (rc) return rc;
  return emb_bwd_bags(c, t, u->in_dims, u->ntables, u->out_dim, u->batch, aggr, lr, s, do_sort, do_apply, opt, states, &cfg, lr_block, pad);
}

int ffh_embedding_bwd_fused_multi_bags(ffh_ctx* c, const ffh_bags_update* u, ffh_stream s) { return emb_bwd_bags_desc(c, u, s, true, true); }

// include/ff_hip_bags_sort.h
int ffh_bags_sort_abi_version(void) { return FFH_BAGS_SORT_ABI_VERSION; }
int ffh_embedding_bwd_sort_multi_bags(ffh_ctx* c, const ffh_bags_update* u, ffh_stream s) { return emb_bwd_bags_desc(c, u, s, true, false); }
int ffh_embedding_bwd_apply_multi_bags(ffh_ctx* c, const ffh_bags_update* u, ffh_stream s) { return emb_bwd_bags_desc(c, u, s, false, true); }

// include/ff_hip_pad.h: the three entries above with an id < 0 as no lookup
int ffh_embedding_bwd_fused_multi_bags_pad(ffh_ctx* c, const ffh_bags_update* u, ffh_stream s) { return emb_bwd_bags_desc(c, u, s, true, true, kBagsPad); }
int ffh_embedding_bwd_sort_multi_bags_pad(ffh_ctx* c, const ffh_bags_update* u, ffh_stream s) { return emb_bwd_bags_desc(c, u, s, true, false, kBagsPad); }
int ffh_embedding_bwd_apply_multi_bags_pad(ffh_ctx* c, const ffh_bags_update* u, ffh_stream s) { return emb_bwd_bags_desc(c, u, s, false, true, kBagsPad); }

// include/ff_hip_pad_mean.h: the fused call and the apply with a mean over the lookups that are there (the sort is the pad sort above)
size_t ffh_embedding_bwd_bags_pad_mean_workspace_bytes(const int* in_dims, int nt, int D, int64_t batch) {
  if (nt <= 0 || D <= 0 || batch <= 0 || bags_dims_check(in_dims, nt, batch) != FFH_OK) return 0;
  return padmean_total(bags_layout(in_dims, nt, D, batch), nt, batch);
}
int ffh_embedding_bwd_fused_multi_bags_pad_mean(ffh_ctx* c, const ffh_bags_update* u, ffh_stream s) { return emb_bwd_bags_desc(c, u, s, true, true, kBagsPadMean); }
int ffh_embedding_bwd_apply_multi_bags_pad_mean(ffh_ctx* c, const ffh_bags_update* u, ffh_stream s) { return emb_bwd_bags_desc(c, u, s, false, true, kBagsPadMean); }

}  // extern "C"
