// model_exchange.cc -- the embedding group (gather, exchange, fused update) and the MLP gradients' all-reduce
// (one of the translation units of the host shim: model_internal.h lists them)
#include "model_internal.h"

#include <map>
#include <tuple>

// =============================================================================================
// embedding group: batched gather (+ exchange) and batched fused update
// =============================================================================================
// launches one batched kernel per distinct shard width (all table-wise tables share one; column blocks of
// giant tables another) and, where the tables' bag sizes differ, per bag size (the gather: one ragged launch where the
// library has it; the fused update: one ragged call where the library has it and the flag allows it); FWD: gather, else fused
// backward + SGD
void launch_shard_groups(const FFModel* ff, ShardLaunch what, ffh_stream s, ffh_ctx* cx, const std::vector<const int64_t*>* idx_override, bool all_tables) {
  const bool fwd = what == kGather;
  ffh_sparse_opt rule;
  const bool ruled = !fwd && ff->sparse_rule(rule);     // momentum / wd SGD, Adam on the touched rows (the sort-only calls read none of it)
  // the rate from device memory (include/ff_hip_lr.h): the opt entries with the table update's own block; kind FFH_SPARSE_OPT_SGD = the plain update's bits
  const ffh_lr_state* lrb = ff->lr_route == FFModel::kLrDevice ? ff->lr_block[1] : nullptr;
  const KernelApiLr* lra = ff->api->lr;
  const int aggr = (int)ff->embeddings[0]->aggr;
  // by shard width, then storage (bf16 tables: include/ff_hip_bf16.h, keyed by global table index and global column), then bag size.  The uniform
  // update entries take one bag size per call, so their groups are split by bag size; a model of mixed bag sizes keeps a group whole (key 0) for the
  // gather where the library has the one-launch ragged gather (include/ff_hip_bags.h) and --no-ragged-gather is not given, and for the fused update
  // where it has the ragged update (include/ff_hip_bags_update.h) and --ragged-update allows it, and for the sort-only / apply-only pair where the
  // ragged early sort is on (include/ff_hip_bags_sort.h, FFModel::ragged_early_sort_on).
  // --embedding-padding (include/ff_hip_pad.h): an id may be -1, which only the pad forms of the ragged entries take -- every chunk of every group
  // goes through them, whether or not its bag sizes differ (compile() has refused every configuration in which one of the three is off).
  const bool ragged = fwd ? ff->ragged_gather_on() : (what == kFusedUpdate ? ff->ragged_update_on() : ff->ragged_early_sort_on());
  const bool pad = ff->config.embedding_padding;
  const KernelApiPad* pda = ff->api->pad;
  // ... and a padded table that pools with AGGR_MODE_AVG takes their mean forms (include/ff_hip_pad_mean.h; compile() has checked that the library has
  // them): the gather, the fused update and the apply.  The early sort stays the pad sort, which serves either apply.
  const bool pad_mean = pad && aggr == FFH_AGGR_MODE_AVG;
  const KernelApiPadMean* pma = ff->api->pad_mean;
  struct Group { std::vector<ffh_emb_table> t; std::vector<ffh_emb_table_bf16> t16; std::vector<ffh_emb_state> st; std::vector<int> bag;
                 std::vector<ffh_emb_table_q8> tq; std::vector<int> bagq; };      // tq, bagq: the tables an evaluation gathers from their 8-bit row images
  // --eval-embedding-dtype int8: the gather of eval_batch() reads the images (include/ff_hip_q8.h), in the same groups.  eval_batch() has made stale images
  // again before it issued this forward pass (on the calling thread: this function may run on a launch worker, and reads the images' addresses only)
  const bool q8 = fwd && ff->evaluating && ff->q8_on() && !idx_override && !all_tables;
  std::map<std::tuple<int, bool, int>, Group> groups;
  size_t owned_i = 0;
  for (const FFModel::EmbShard& sh : ff->shards) {
    if (sh.owner != ff->rank) continue;
    const Embedding* e = sh.e;
    ffh_emb_table t;
    t.idx = (const int64_t*)e->inputs[0].impl->ptr;
    if (idx_override && owned_i < idx_override->size()) t.idx = (*idx_override)[owned_i];
    owned_i++;
    if (!fwd && !all_tables && ff->fold_dx_table(e)) continue;      // its update is FFModel::fold_table_update (its rows of the data gradient are not produced)
    t.weight = (float*)e->weights[0].impl->ptr;      // column-sharded: the local [R][cols] slice
    t.num_entries = e->num_entries;
    if (!ff->exchange) {
      t.io = fwd ? (float*)e->outputs[0].impl->ptr : e->outputs[0].impl->grad;
      t.ld = fwd ? e->outputs[0].impl->ld : e->outputs[0].impl->grad_ld;
    } else {
      t.io = (fwd ? ff->xsend : ff->grecv) + sh.off;
      t.ld = ff->rank_width[ff->rank];
    }
    const int bag = e->inputs[0].adim[0];
    Group& g = groups[std::make_tuple(sh.cols, e->bf16_weights(), ragged ? 0 : bag)];
    if (q8 && e->q8_rows) {
      g.tq.push_back(ffh_emb_table_q8{t.idx, e->q8_rows, t.io, t.num_entries, t.ld, e->q8_row_bytes});
      g.bagq.push_back(bag);
      continue;
    }
    if (e->bf16_weights()) g.t16.push_back(ffh_emb_table_bf16{t.idx, (uint16_t*)t.weight, t.io, t.num_entries, t.ld, e->table_index, sh.col0});
    else g.t.push_back(t);
    g.st.push_back(ffh_emb_state{e->opt_state[0], e->opt_state[1]});
    g.bag.push_back(bag);
  }
  const int64_t B = ff->config.batchSize;
  for (auto& kv : groups) {
    const int D = std::get<0>(kv.first);
    const Group& g = kv.second;
    // tables [b, b + n) of the group in one ragged launch: where their bag sizes differ (else the call stays the uniform one)
    auto differ = [&](size_t b, int n) {
      if (pad) return true;
      for (int i = 1; i < n; i++) if (g.bag[b + i] != g.bag[b]) return true;
      return false;
    };
    // the ragged update of tables [b, b + n), fused or one call of the pair (`what`): every rule and both rates through the one descriptor
    auto ragged_update = [&](const ffh_emb_table* t32, const ffh_emb_table_bf16* t16, const ffh_emb_state* st, const ffh_bf16_rounding* rnd, size_t b, int n) {
      ffh_bags_update u;
      u.tables = t32; u.tables_bf16 = t16; u.in_dims = g.bag.data() + b; u.states = st;
      u.ntables = n; u.out_dim = D; u.batch = B; u.aggr = aggr; u.lr = rule.lr;
      u.opt = (ruled || lrb) ? &rule : nullptr;
      u.rounding = rnd; u.lr_block = lrb;
      if (what == kSortOnly) {
        if (pad) ff->check(pda->ffh_embedding_bwd_sort_multi_bags_pad(cx, &u, s), "embedding_bwd_sort_multi_bags_pad");
        else ff->check(ff->api->bags_sort->ffh_embedding_bwd_sort_multi_bags(cx, &u, s), "embedding_bwd_sort_multi_bags");
        ff->n_early_sorts++; ff->n_ragged_early_sorts++;
        return;
      }
      if (pad_mean) {
        if (what == kApplyOnly) ff->check(pma->ffh_embedding_bwd_apply_multi_bags_pad_mean(cx, &u, s), "embedding_bwd_apply_multi_bags_pad_mean");
        else ff->check(pma->ffh_embedding_bwd_fused_multi_bags_pad_mean(cx, &u, s), "embedding_bwd_fused_multi_bags_pad_mean");
        ff->n_pad_mean_updates++;
        return;
      }
      if (pad) {
        if (what == kApplyOnly) ff->check(pda->ffh_embedding_bwd_apply_multi_bags_pad(cx, &u, s), "embedding_bwd_apply_multi_bags_pad");
        else ff->check(pda->ffh_embedding_bwd_fused_multi_bags_pad(cx, &u, s), "embedding_bwd_fused_multi_bags_pad");
        ff->n_pad_updates++;
        return;
      }
      if (what == kApplyOnly) ff->check(ff->api->bags_sort->ffh_embedding_bwd_apply_multi_bags(cx, &u, s), "embedding_bwd_apply_multi_bags");
      else ff->check(ff->api->bags_update->ffh_embedding_bwd_fused_multi_bags(cx, &u, s), "embedding_bwd_fused_multi_bags");
      ff->n_ragged_updates++;
    };
    for (size_t b = 0; b < g.tq.size(); b += FFH_MAX_TABLES) {      // (evaluation with --eval-embedding-dtype int8 only)
      const int n = (int)std::min<size_t>(FFH_MAX_TABLES, g.tq.size() - b);
      bool mixed = false;
      for (int i = 1; i < n; i++) mixed = mixed || g.bagq[b + i] != g.bagq[b];
      if (ragged && mixed) ff->check(ff->api->q8->ffh_embedding_fwd_multi_bags_q8(cx, g.tq.data() + b, g.bagq.data() + b, n, D, B, aggr, s), "embedding_fwd_multi_bags_q8");
      else ff->check(ff->api->q8->ffh_embedding_fwd_multi_q8(cx, g.tq.data() + b, n, g.bagq[b], D, B, aggr, s), "embedding_fwd_multi_q8");
      ff->n_q8_gathers++;
    }
    if (std::get<1>(kv.first)) {
      const KernelApiBf16* b16 = ff->api->bf16;
      const ffh_bf16_rounding rnd = ff->bf16_rounding();
      const size_t per = ff->bf16_tables_per_launch();       // momentum / Adam: FFH_BF16_MAX_STATEFUL_TABLES (the sort of an early-sorted group matches it)
      for (size_t b = 0; b < g.t16.size(); b += per) {
        const int n = (int)std::min<size_t>(per, g.t16.size() - b);
        const ffh_emb_table_bf16* tb = g.t16.data() + b;
        const ffh_emb_state* st = g.st.data() + b;
        const int L = g.bag[b];       // a uniform call's bag size is its own tables' (a whole group of mixed sizes holds several)
        switch (what) {
          case kGather:
            if (pad_mean) {
              ff->check(pma->ffh_embedding_fwd_multi_bags_pad_mean_bf16(cx, tb, g.bag.data() + b, n, D, B, aggr, s), "embedding_fwd_multi_bags_pad_mean_bf16");
              ff->n_pad_mean_gathers++;
            } else if (pad) {
              ff->check(pda->ffh_embedding_fwd_multi_bags_pad_bf16(cx, tb, g.bag.data() + b, n, D, B, aggr, s), "embedding_fwd_multi_bags_pad_bf16");
              ff->n_pad_gathers++;
            } else if (ragged && differ(b, n)) {
              ff->check(ff->api->bags->ffh_embedding_fwd_multi_bags_bf16(cx, tb, g.bag.data() + b, n, D, B, aggr, s), "embedding_fwd_multi_bags_bf16");
              ff->n_ragged_gathers++;
            } else ff->check(b16->ffh_embedding_fwd_multi_bf16(cx, tb, n, g.bag[b], D, B, aggr, s), "embedding_fwd_multi_bf16");
            break;
          case kFusedUpdate:
            if (ragged && differ(b, n)) ragged_update(nullptr, tb, st, &rnd, b, n);
            else if (lrb) ff->check(lra->ffh_embedding_bwd_opt_fused_multi_bf16_lr(cx, tb, st, n, L, D, B, aggr, &rule, &rnd, lrb, s), "embedding_bwd_opt_fused_multi_bf16_lr");
            else if (ruled) ff->check(b16->ffh_embedding_bwd_opt_fused_multi_bf16(cx, tb, st, n, L, D, B, aggr, &rule, &rnd, s), "embedding_bwd_opt_fused_multi_bf16");
            else ff->check(b16->ffh_embedding_bwd_sgd_fused_multi_bf16(cx, tb, n, L, D, B, aggr, rule.lr, &rnd, s), "embedding_bwd_sgd_fused_multi_bf16");
            break;
          case kSortOnly:
            if (ragged && differ(b, n)) { ragged_update(nullptr, tb, st, &rnd, b, n); break; }
            ff->check(b16->ffh_embedding_bwd_sort_multi_bf16(cx, tb, n, L, D, B, s), "embedding_bwd_sort_multi_bf16"); ff->n_early_sorts++; break;
          case kApplyOnly:
            if (ragged && differ(b, n)) ragged_update(nullptr, tb, st, &rnd, b, n);
            else if (lrb) ff->check(lra->ffh_embedding_bwd_opt_apply_multi_bf16_lr(cx, tb, st, n, L, D, B, aggr, &rule, &rnd, lrb, s), "embedding_bwd_opt_apply_multi_bf16_lr");
            else if (ruled) ff->check(b16->ffh_embedding_bwd_opt_apply_multi_bf16(cx, tb, st, n, L, D, B, aggr, &rule, &rnd, s), "embedding_bwd_opt_apply_multi_bf16");
            else ff->check(b16->ffh_embedding_bwd_sgd_apply_multi_bf16(cx, tb, n, L, D, B, aggr, rule.lr, &rnd, s), "embedding_bwd_sgd_apply_multi_bf16");
            break;
        }
      }
      continue;
    }
    const std::vector<ffh_emb_table>& tabs = g.t;
    const std::vector<ffh_emb_state>& sts = g.st;
    for (size_t b = 0; b < tabs.size(); b += FFH_MAX_TABLES) {
      const int n = (int)std::min<size_t>(FFH_MAX_TABLES, tabs.size() - b);
      const int L = g.bag[b];
      switch (what) {
        case kGather:
          if (pad_mean) {
            ff->check(pma->ffh_embedding_fwd_multi_bags_pad_mean(cx, tabs.data() + b, g.bag.data() + b, n, D, B, aggr, s), "embedding_fwd_multi_bags_pad_mean");
            ff->n_pad_mean_gathers++;
          } else if (pad) {
            ff->check(pda->ffh_embedding_fwd_multi_bags_pad(cx, tabs.data() + b, g.bag.data() + b, n, D, B, aggr, s), "embedding_fwd_multi_bags_pad");
            ff->n_pad_gathers++;
          } else if (ragged && differ(b, n)) {
            ff->check(ff->api->bags->ffh_embedding_fwd_multi_bags(cx, tabs.data() + b, g.bag.data() + b, n, D, B, aggr, s), "embedding_fwd_multi_bags");
            ff->n_ragged_gathers++;
          } else ff->check(ff->api->ffh_embedding_fwd_multi(cx, tabs.data() + b, n, g.bag[b], D, B, aggr, s), "embedding_fwd_multi");
          break;
        case kFusedUpdate:
          if (ragged && differ(b, n)) ragged_update(tabs.data() + b, nullptr, sts.data() + b, nullptr, b, n);
          else if (lrb) ff->check(lra->ffh_embedding_bwd_opt_fused_multi_lr(cx, tabs.data() + b, sts.data() + b, n, L, D, B, aggr, &rule, lrb, s), "embedding_bwd_opt_fused_multi_lr");
          else if (ruled) ff->check(ff->api->ffh_embedding_bwd_opt_fused_multi(cx, tabs.data() + b, sts.data() + b, n, L, D, B, aggr, &rule, s), "embedding_bwd_opt_fused_multi");
          else ff->check(ff->api->ffh_embedding_bwd_sgd_fused_multi(cx, tabs.data() + b, n, L, D, B, aggr, rule.lr, s), "embedding_bwd_sgd_fused_multi");
          break;
        case kSortOnly:
          if (ragged && differ(b, n)) { ragged_update(tabs.data() + b, nullptr, sts.data() + b, nullptr, b, n); break; }
          ff->check(ff->api->ffh_embedding_bwd_sort_multi(cx, tabs.data() + b, n, L, D, B, s), "embedding_bwd_sort_multi"); ff->n_early_sorts++; break;
        case kApplyOnly:
          if (ragged && differ(b, n)) ragged_update(tabs.data() + b, nullptr, sts.data() + b, nullptr, b, n);
          else if (lrb) ff->check(lra->ffh_embedding_bwd_opt_apply_multi_lr(cx, tabs.data() + b, sts.data() + b, n, L, D, B, aggr, &rule, lrb, s), "embedding_bwd_opt_apply_multi_lr");
          else if (ruled) ff->check(ff->api->ffh_embedding_bwd_opt_apply_multi(cx, tabs.data() + b, sts.data() + b, n, L, D, B, aggr, &rule, s), "embedding_bwd_opt_apply_multi");
          else ff->check(ff->api->ffh_embedding_bwd_sgd_apply_multi(cx, tabs.data() + b, n, L, D, B, aggr, rule.lr, s), "embedding_bwd_sgd_apply_multi");
          break;
      }
    }
  }
}

// =============================================================================================
// --eval-embedding-dtype int8 (include/ff_hip_q8.h)
// =============================================================================================
// where this rank's gather of shard `sh` writes (launch_shard_groups, kGather)
static void gather_dest(const FFModel* ff, const FFModel::EmbShard& sh, float** io, int64_t* ld) {
  if (!ff->exchange) { *io = (float*)sh.e->outputs[0].impl->ptr; *ld = sh.e->outputs[0].impl->ld; }
  else { *io = ff->xsend + sh.off; *ld = ff->rank_width[ff->rank]; }
}

// Where allocate() will put a table's gathered rows, from the layer structure alone (its step 4): a table whose output is read only by one feature-axis
// Concat writes straight into the Concat's buffer, at the column where its input starts, with the Concat's width as leading dimension; any other table
// owns rows of its own width.  Through the exchange buffers a rank's tables lie side by side, each at a multiple of the (checked) table widths.  Buffers
// start 16-byte aligned, so the 16-byte form holds iff that column and that width are multiples of 4 floats.
void FFModel::q8_check_destinations() const {
  if (exchange) return;
  std::map<const TensorImpl*, int> consumers;
  for (const Op* op : layers)
    for (int i = 0; i < op->numInputs; i++) consumers[op->inputs[i].impl]++;
  std::set<const TensorImpl*> placed;
  for (const Op* op : layers) {
    const Concat* c = dynamic_cast<const Concat*>(op);
    if (!c || c->axis != 0) continue;
    int64_t width = 0;
    for (int i = 0; i < c->numInputs; i++) width += c->inputs[i].adim[0];
    int64_t off = 0;
    for (int i = 0; i < c->numInputs; i++) {
      const Tensor& in = c->inputs[i];
      if (in.owner_op && in.owner_op->op_type == OP_EMBEDDING && consumers[in.impl] == 1 && placed.insert(in.impl).second && (off % 4 || width % 4))
        die("--eval-embedding-dtype int8: the gather of %s writes columns %lld.. of a %lld-column Concat, rows that are not 16-byte aligned, and the 8-bit "
            "gather has no scalar form: make the widths in front of it and the Concat's width multiples of 4 (--arch-mlp-bot, --arch-sparse-feature-size), or "
            "drop --eval-embedding-dtype int8", in.owner_op->name, (long long)off, (long long)width);
      off += in.adim[0];
    }
  }
}

void FFModel::q8_allocate() {
  q8_bytes = q8_table_bytes = 0;
  q8_folded = 0;
  for (const EmbShard& sh : shards) {
    if (sh.owner != rank) continue;
    Embedding* e = sh.e;
    if (std::find(fold.tables.begin(), fold.tables.end(), e) != fold.tables.end()) { q8_folded++; continue; }      // read as products of the fp32 table: its path is kept
    float* io; int64_t ld;
    gather_dest(this, sh, &io, &ld);
    if (((uintptr_t)io & 15) || ld % 4)
      die("--eval-embedding-dtype int8: the gather of %s writes rows that are not 16-byte aligned (leading dimension %lld floats), which q8_check_destinations() "
          "did not foresee: drop --eval-embedding-dtype int8", e->name, (long long)ld);
  }
  for (const EmbShard& sh : shards) {
    if (sh.owner != rank) continue;
    Embedding* e = sh.e;
    if (std::find(fold.tables.begin(), fold.tables.end(), e) != fold.tables.end()) continue;
    e->q8_row_bytes = (int64_t)api->q8->ffh_q8_row_bytes(e->out_channels);
    const size_t bytes = (size_t)e->num_entries * (size_t)e->q8_row_bytes;
    e->q8_rows = (uint8_t*)dmalloc(bytes);
    q8_bytes += bytes;
    q8_table_bytes += (size_t)e->num_entries * e->out_channels * (e->bf16_weights() ? 2 : 4);
  }
  q8_stale = true;
}

void FFModel::q8_quantize(ffh_stream s, ffh_ctx* cx) const {
  std::map<std::pair<int, bool>, std::vector<ffh_q8_source>> groups;      // by width and storage
  for (const EmbShard& sh : shards) {
    const Embedding* e = sh.e;
    if (sh.owner != rank || !e->q8_rows) continue;
    groups[{e->out_channels, e->bf16_weights()}].push_back(ffh_q8_source{e->weights[0].impl->ptr, e->q8_rows, e->num_entries, e->q8_row_bytes, e->bf16_weights() ? 1 : 0, 0});
  }
  for (const auto& kv : groups)
    for (size_t b = 0; b < kv.second.size(); b += FFH_MAX_TABLES) {
      const int n = (int)std::min<size_t>(FFH_MAX_TABLES, kv.second.size() - b);
      check(api->q8->ffh_embedding_quantize_q8(cx, kv.second.data() + b, n, kv.first.first, s), "embedding_quantize_q8");
      n_q8_quantize++;
    }
  q8_stale = false;
}

std::string FFModel::q8_line() const {
  int64_t rb = 0;
  for (const Embedding* e : embeddings) if (e->q8_rows) { rb = e->q8_row_bytes; break; }
  char buf[200];
  snprintf(buf, sizeof buf, "int8 rows (row_bytes %lld), %zu bytes beside %zu bytes of tables, %d folded tables keep fp32", (long long)rb, q8_bytes, q8_table_bytes, q8_folded);
  return buf;
}

bool FFModel::ragged_gather_on() const { return bags_path() && config.ragged_gather && api->bags; }
// how a model of mixed bag sizes gathers (the driver prints it): the launches of one gather over this rank's tables
std::string FFModel::bag_gather_line() const {
  std::set<std::tuple<int, bool, int>> keys;
  for (const EmbShard& sh : shards)
    if (sh.owner == rank) keys.insert(std::make_tuple(sh.cols, sh.e->bf16_weights(), ragged_gather_on() ? 0 : sh.e->inputs[0].adim[0]));
  char buf[160];
  if (!mixed_bags) { snprintf(buf, sizeof buf, "one bag size, %zu launch%s", keys.size(), keys.size() == 1 ? "" : "es"); return buf; }
  if (ragged_gather_on()) snprintf(buf, sizeof buf, "ragged, one launch per group (%zu launch%s)", keys.size(), keys.size() == 1 ? "" : "es");
  else snprintf(buf, sizeof buf, "per bag size, %zu launches%s", keys.size(), !api->bags ? " (the kernel library has no ragged gather)" : " (--no-ragged-gather)");
  return buf;
}

bool FFModel::ragged_update_on() const { return bags_path() && config.ragged_update && api->bags_update; }
// a model of mixed bag sizes may sort behind the gather (early_sort_possible): asked for by --early-sort (never by shape: that default is unmeasured),
// with the ragged update on and a library that has its two-call form (include/ff_hip_bags_sort.h)
bool FFModel::ragged_early_sort_on() const { return config.early_sort > 0 && ragged_update_on() && api->bags_sort; }
// how a model of mixed bag sizes updates its tables (the driver prints it): the calls of one fused update over this rank's tables
std::string FFModel::bag_update_line() const {
  const bool on = ragged_update_on();
  std::map<std::tuple<int, bool, int>, std::vector<int>> keys;      // the groups of launch_shard_groups, each with its tables' bag sizes in order
  for (const EmbShard& sh : shards)
    if (sh.owner == rank) keys[std::make_tuple(sh.cols, sh.e->bf16_weights(), on ? 0 : sh.e->inputs[0].adim[0])].push_back(sh.e->inputs[0].adim[0]);
  size_t calls = 0, uniform = 0;      // (a chunk of a whole group whose bag sizes are equal makes the uniform call)
  for (const auto& kv : keys) {
    const std::vector<int>& bag = kv.second;
    const size_t per = std::get<1>(kv.first) ? bf16_tables_per_launch() : (size_t)FFH_MAX_TABLES;
    for (size_t b = 0; b < bag.size(); b += per, calls++)
      uniform += std::all_of(bag.begin() + b, bag.begin() + std::min(bag.size(), b + per), [&](int L) { return L == bag[b]; });
  }
  char buf[160];
  if (on && uniform) snprintf(buf, sizeof buf, "ragged, %zu call%s per step (%zu of them over one bag size)", calls, calls == 1 ? "" : "s", uniform);
  else if (on) snprintf(buf, sizeof buf, "ragged, %zu call%s per step", calls, calls == 1 ? "" : "s");
  else snprintf(buf, sizeof buf, "per bag size, %zu call%s per step%s", calls, calls == 1 ? "" : "s", !api->bags_update ? " (the kernel library has no ragged update)" : " (--no-ragged-update)");
  // the sort of the one ragged call leaves the chain behind the gradients (ffh_embedding_bwd_sort_multi_bags behind the gather)
  if (on && ragged_early_sort_on() && early_sort_possible(1)) snprintf(buf + strlen(buf), sizeof buf - strlen(buf), ", sorted behind the gather");
  return buf;
}

// bf16 tables: the rounding of this model's table update.  The stochastic bits' seed is ffh_hash(FFConfig::seed, kBf16SeedSalt) --
// the one place it is derived -- and the update number comes from the counter in device memory
static constexpr uint64_t kBf16SeedSalt = 0xBF16;
ffh_bf16_rounding FFModel::bf16_rounding() const {
  ffh_bf16_rounding r;
  r.mode = config.embedding_rounding;
  r.reserved_ = 0;
  r.seed = ffh_hash(config.seed, kBf16SeedSalt);
  r.counter = bf16_counter;
  return r;
}
// once per step behind the step's last bf16 table update, on its stream (a captured step replays it too)
void FFModel::advance_bf16_counter(ffh_stream s, ffh_ctx* cx) const {
  if (bf16_counter) check(api->bf16->ffh_bf16_counter_advance(cx, bf16_counter, s), "bf16_counter_advance");
}
// tables per bf16 launch: the stateful bf16 entries take at most FFH_BF16_MAX_STATEFUL_TABLES (include/ff_hip_bf16.h)
size_t FFModel::bf16_tables_per_launch() const {
  ffh_sparse_opt rule;
  bool any16 = false;
  for (const Embedding* e : embeddings) any16 = any16 || e->bf16_weights();
  // (Adagrad has one state pointer per table and rides the plain update's layout: include/ff_hip_adagrad.h)
  return any16 && fused_embedding_update() && sparse_rule(rule) && rule.kind != FFH_SPARSE_OPT_ADAGRAD && rule.kind != FFH_SPARSE_OPT_ROWWISE_ADAGRAD ? FFH_BF16_MAX_STATEFUL_TABLES : FFH_MAX_TABLES;
}
uint64_t FFModel::read_bf16_counter() const {
  if (!bf16_counter) return 0;
  if (dw_worker) dw_worker->drain();
  if (side_worker) side_worker->drain();
  check(api->ffh_stream_sync(ctx, side_stream), "bf16 counter sync");
  check(api->ffh_stream_sync(ctx, stream), "bf16 counter sync");
  uint64_t v = 0;
  check(api->ffh_memcpy_d2h(ctx, &v, bf16_counter, sizeof v, stream), "bf16 counter");
  check(api->ffh_stream_sync(ctx, stream), "bf16 counter sync");
  return v;
}

// the batched gather (fwd) or fused update kernels of this rank's shards alone, no exchange: what bench.py times as the
// roofline kernels of a multi-rank job
void FFModel::embedding_kernels_only(bool fwd, ffh_stream s, const std::vector<const int64_t*>* idx_override) const {
  if (embeddings.empty() || (!fwd && !fused_embedding_update())) return;
  launch_shard_groups(this, fwd ? kGather : kFusedUpdate, s, ctx, idx_override, true);      // (a roofline probe: every table, dx-folded or not)
  if (!fwd) q8_stale = true;      // (the probe's update writes the tables)
  if (!fwd) advance_bf16_counter(s, ctx);
}

// The sort of the fused update reads only the sparse ids, which are final when the gather starts: issued behind the gather on
// the side stream it runs beside the top MLP's forward instead of between the gradients and the next gather (what Legion's
// region dependences would give an index-only task).  The sorted list waits in the ctx workspace, so this is only done when
// nothing else writes the workspace between a step's gather and its update: one launch group (one shard width, <=
// FFH_MAX_TABLES shards), no row-wise sharded table (its own fused call), launches issued inline.
bool FFModel::early_sort_possible(int where) const {
  if (!config.early_sort || !config.overlap_embedding || !fused_embedding_update() || config.profiling) return false;
  if (config.computationMode != COMP_MODE_TRAINING || use_workers() || evaluating) return false;      // (eval_batch(): no update follows)
  // by shape (round 4, profiles/r04_ab_schedule.txt): behind the exchange the whole update sits between the backward all-to-all and
  // the next gather, so the sort leaves that chain; on one GPU it pays at small per-GPU batches (4096 samples: 1.178 vs 1.191 ms)
  // and costs at large ones, where it runs beside the top MLP's first forward GEMM (32768: 7.76-7.79 vs 7.71-7.73; 8192, MLPerf
  // shape: 1.236-1.239 vs 1.227-1.233)
  // (round 6) in the two bf16-pipe math modes the GEMMs the update used to hide under are 1.5-4x shorter and the sort sits on the step's
  // critical chain [sort -> apply -> gather] at every batch: early there (32768 samples: split mode 5.21-5.27 vs 5.28-5.31 ms, tensor-op 1.949-1.960 vs 1.969-1.972)
  const bool exact_gemms = !config.allow_tensor_op_math_conversion && !config.fp32_split_bf16x3;
  const int mode = config.early_sort > 0 ? config.early_sort : ((!exchange && local_batch >= 8192 && exact_gemms) ? early_sort_big_batch_mode : 1);
  if (mode != where) return false;
  if (config.embedding_padding && !ragged_early_sort_on()) return false;      // (the uniform sort takes no pad id: only the pad pair sorts early, on --early-sort)
  int n = 0, cols = -1, bag = -1;
  for (const EmbShard& sh : shards) {
    if (sh.owner != rank) continue;
    if (cols >= 0 && sh.cols != cols) return false;
    // one sort note per ctx: a model of mixed bag sizes sorts in front of its apply, unless its one group has the ragged pair (ragged_early_sort_on)
    if (bag >= 0 && sh.e->inputs[0].adim[0] != bag && !ragged_early_sort_on()) return false;
    cols = sh.cols;
    bag = sh.e->inputs[0].adim[0];
    n++;
  }
  for (const Embedding* e : embeddings)
    if (e->row_sharded) return false;
  return n > 0 && (size_t)n <= bf16_tables_per_launch();
}

void FFModel::probe_record(int which, ffh_stream s, ffh_ctx* cx) const {
  if (!probe_events_on) return;
  if (!probe_ev[which]) check(api->ffh_event_create(ctx, &probe_ev[which]), "probe event");
  check(api->ffh_event_record(cx, probe_ev[which], s), "probe event");
}

void FFModel::embedding_group_forward(ffh_stream s, ffh_ctx* on_ctx) const {
  if (embeddings.empty()) return;
  launch_shard_groups(this, kGather, s, on_ctx ? on_ctx : ctx);
  ffh_ctx* cx = on_ctx ? on_ctx : ctx;
  if (exchange) {
    // each owner gathered its tables / column blocks for the global batch; rows go to the rank that owns the sample
    probe_record(4, s, cx);
    if (!shards.empty() && config.comm.alltoall_f32(config.comm.user, xsend, fwd_send_counts.data(), xrecv, fwd_recv_counts.data(), s) != 0)
      die("alltoall (embedding forward) failed");
    probe_record(5, s, cx);
  }
  // data-parallel (replicated) tables: this rank's samples from this rank's copy, straight into the outputs; one launch
  {
    std::vector<ffh_emb_table> tabs;
    const int Lr = embeddings[0]->inputs[0].adim[0];
    for (const Embedding* e : embeddings) {
      if (!e->replicated) continue;
      ffh_emb_table t;
      t.idx = (const int64_t*)e->inputs[0].impl->ptr + (int64_t)rank * local_batch * Lr;   // every rank holds the ids of the global batch
      t.weight = (float*)e->weights[0].impl->ptr;
      t.num_entries = e->num_entries;
      t.io = (float*)e->outputs[0].impl->ptr;
      t.ld = e->outputs[0].impl->ld;
      tabs.push_back(t);
    }
    for (size_t b = 0; b < tabs.size(); b += FFH_MAX_TABLES) {
      const int n = (int)std::min<size_t>(FFH_MAX_TABLES, tabs.size() - b);
      check(api->ffh_embedding_fwd_multi(cx, tabs.data() + b, n, Lr, embeddings[0]->out_channels, local_batch, (int)embeddings[0]->aggr, s),
            "embedding_fwd_multi (data-parallel tables)");
    }
  }
  // row-wise sharded tables: partial bag sums of the GLOBAL batch over the rows held here (rows held elsewhere read the
  // zero row), then the ranks' partials are added and every rank keeps its own samples
  for (const Embedding* e : embeddings) {
    if (!e->row_sharded) continue;
    const int L = e->inputs[0].adim[0], D = e->out_channels;
    check(api->ffh_embedding_localize_rows(cx, (const int64_t*)e->inputs[0].impl->ptr, e->local_idx, (int64_t)config.batchSize * L,
                                           e->row_begin, e->rows_local, s), "embedding_localize_rows");
    check(api->ffh_embedding_fwd(cx, e->local_idx, e->partial, (const float*)e->weights[0].impl->ptr, L, D, config.batchSize,
                                 e->rows_local + 1, D, (int)e->aggr, s), e->name);
    if (config.comm.reduce_scatter_sum_f32(config.comm.user, e->partial, (float*)e->outputs[0].impl->ptr, local_batch * D, s) != 0)
      die("reduce-scatter (row-sharded embedding forward) failed");
  }
}

// Gradient of the data-parallel tables: G[row] += sum of this rank's gradient rows that looked the row up.  The reference
// scatter-adds with atomics; these are the SMALL tables (3 ... a few thousand rows), where a rank's samples pile hundreds of
// adds onto one address and atomics serialise.  The fused sparse kernels already compute exactly these segmented sums
// (sort + reduce, W[row] -= lr * sum): pointed at the zeroed slab gradient with lr = -1 they leave G = 0 + sum -- no
// atomics, a fixed order.  They need the scratch workspace, which the side-stream update of the owned tables may be using:
// this call brings its own (workspace pointers are read at launch time, so switching between launches is safe).
void FFModel::replicated_embedding_grads() const {
  if (!repl_workspace) return;
  std::vector<ffh_emb_table> tabs;
  const int L = embeddings[0]->inputs[0].adim[0], D = embeddings[0]->out_channels;
  for (const Embedding* e : embeddings) {
    if (!e->replicated) continue;
    ffh_emb_table t;
    t.idx = (const int64_t*)e->inputs[0].impl->ptr + (int64_t)rank * local_batch * L;
    t.weight = e->weights[0].impl->grad;
    t.num_entries = e->num_entries;
    t.io = e->outputs[0].impl->grad;
    t.ld = e->outputs[0].impl->grad_ld;
    tabs.push_back(t);
  }
  check(api->ffh_ctx_set_workspace(ctx, repl_workspace, repl_workspace_bytes), "set workspace");
  for (size_t b = 0; b < tabs.size(); b += FFH_MAX_TABLES) {
    const int n = (int)std::min<size_t>(FFH_MAX_TABLES, tabs.size() - b);
    check(api->ffh_embedding_bwd_sgd_fused_multi(ctx, tabs.data() + b, n, L, D, local_batch, (int)embeddings[0]->aggr, -1.0f, stream),
          "embedding gradient (data-parallel tables)");
  }
  check(api->ffh_ctx_set_workspace(ctx, workspace, workspace_bytes), "set workspace");
}

void FFModel::embedding_group_update(ffh_stream s, ffh_ctx* on_ctx, bool advance_rate) const {
  if (embeddings.empty()) return;
  if (exchange) {
    // gradients of the rows go back to the owners (transposed exchange)
    probe_record(6, s, on_ctx ? on_ctx : ctx);
    if (!shards.empty() && config.comm.alltoall_f32(config.comm.user, gsend, fwd_recv_counts.data(), grecv, fwd_send_counts.data(), s) != 0)
      die("alltoall (embedding backward) failed");
    probe_record(7, s, on_ctx ? on_ctx : ctx);
    bwd_alltoall_issued = true;
  }
  launch_shard_groups(this, emb_sorted_early ? kApplyOnly : kFusedUpdate, s, on_ctx ? on_ctx : ctx);
  emb_sorted_early = false;
  // row-wise sharded tables: every rank needs the gradient rows of the global batch; the fused update then touches the
  // rows held here, and whatever the other ranks' rows piled onto the zero row is wiped
  ffh_ctx* cx = on_ctx ? on_ctx : ctx;
  ffh_sparse_opt rule;
  const bool ruled = sparse_rule(rule);
  for (const Embedding* e : embeddings) {
    if (!e->row_sharded) continue;
    const int L = e->inputs[0].adim[0], D = e->out_channels;
    if (config.comm.allgather_f32(config.comm.user, e->outputs[0].impl->grad, e->gfull, local_batch * D, s) != 0)
      die("all-gather (row-sharded embedding backward) failed");
    float* w = (float*)e->weights[0].impl->ptr;
    if (ruled) {
      const ffh_emb_table t{e->local_idx, w, e->gfull, e->rows_local + 1, D};
      const ffh_emb_state st{e->opt_state[0], e->opt_state[1]};
      check(api->ffh_embedding_bwd_opt_fused_multi(cx, &t, &st, 1, L, D, config.batchSize, (int)e->aggr, &rule, s), e->name);
    } else {
      check(api->ffh_embedding_bwd_sgd_fused(cx, e->local_idx, e->gfull, w, L, D, config.batchSize, e->rows_local + 1, D, (int)e->aggr, rule.lr, s), e->name);
    }
    check(api->ffh_zero(cx, w + e->rows_local * (int64_t)D, (size_t)D * 4, s), "zero row");   // (its optimizer state is never read for a row of the block)
  }
  advance_bf16_counter(s, cx);
  if (advance_rate) advance_lr(1, s, cx);      // behind this step's last reader of the table update's block, on its stream
}

// The reference's own table update on the rank(s) that hold a table, for optimizers the fused update does not cover (default for
// momentum / weight-decay SGD and Adam): Op::zero_grad [ref: src/runtime/model.cc:466-490] (zero_gradients()), embed_backward
// [ref: src/ops/embedding.cu:192-217] into the owner-local dense gradient, then the optimizer's dense sweep with its dense per-table
// state [ref: src/runtime/optimizer.cc:93-189,256-330].  Multi-rank: the rows' gradients first travel back to the owners (the
// transposed all-to-all / the all-gather of a row-sharded table); a table has ONE holder per element, so nothing is all-reduced.
void FFModel::embedding_dense_update() const {
  if (embeddings.empty()) return;
  const int aggr = (int)embeddings[0]->aggr;
  if (exchange) {
    if (!shards.empty() && config.comm.alltoall_f32(config.comm.user, gsend, fwd_recv_counts.data(), grecv, fwd_send_counts.data(), stream) != 0)
      die("alltoall (embedding backward) failed");
    for (const EmbShard& sh : shards) {
      if (sh.owner != rank) continue;
      const Embedding* e = sh.e;
      const int L = e->inputs[0].adim[0];
      check(api->ffh_embedding_bwd_dense(ctx, (const int64_t*)e->inputs[0].impl->ptr, grecv + sh.off, e->weights[0].impl->grad, L, sh.cols,
                                         config.batchSize, e->num_entries, rank_width[rank], aggr, stream), e->name);
    }
    for (const Embedding* e : embeddings) {
      if (!e->row_sharded) continue;
      const int D = e->out_channels, L = e->inputs[0].adim[0];
      if (config.comm.allgather_f32(config.comm.user, e->outputs[0].impl->grad, e->gfull, local_batch * D, stream) != 0)
        die("all-gather (row-sharded embedding backward) failed");
      check(api->ffh_embedding_bwd_dense(ctx, e->local_idx, e->gfull, e->weights[0].impl->grad, L, D, config.batchSize, e->rows_local + 1, D, aggr, stream), e->name);
    }
  }
  for (Embedding* e : embeddings)
    if (e->held_here(rank) && !e->replicated) optimizer->update(&e->weights[0]);
}

// ---- bucketed all-reduce of the MLP gradients (allocate step 5b) ----------------------------------------------------------------
// The sum of a gradient range over the ranks.  Ring: the transport's all-reduce (ncclAllReduce: 2 (N - 1) / N of the bytes over ONE link per
// hop).  Direct (--direct-allreduce; SURVEY section 5: "prefer direct (fully-connected) algorithms"): xGMI connects every pair of GPUs, so
//   1. all-to-all: rank r receives slice r of the range from every rank (every link carries 1 / N of the range, all at once),
//   2. ffh_sum_slices_f32: the N copies added in RANK order -- the same fp32 chain on whichever rank owns the slice: every rank ends up with
//      the same bits, and a run gives the same bits as the next,
//   3. all-gather of the sums (again 1 / N per link), copied back into the range.
// Both collectives go to the buckets' channel where the transport has one.  [ref: one ncclAllReduce per parameter,
// src/runtime/optimizer_kernel.cu:170-171]
int FFModel::allreduce_grads(float* buf, int64_t count, ffh_stream s, bool bucket) const {
  const int G = world_size;
  auto ring = [&]() -> int {
    auto fn = (bucket && config.comm.allreduce_bucket_sum_f32) ? config.comm.allreduce_bucket_sum_f32 : config.comm.allreduce_sum_f32;
    return fn(config.comm.user, buf, count, s);
  };
  auto a2a = config.comm.alltoall_bucket_f32 ? config.comm.alltoall_bucket_f32 : config.comm.alltoall_f32;
  auto gather = config.comm.allgather_bucket_f32 ? config.comm.allgather_bucket_f32 : config.comm.allgather_f32;
  if (!config.direct_allreduce || !gather || !a2a || count <= 0) return ring();      // (one forced rank: the same three calls on one slice -- the functional run)
  const int64_t slice = (((count + G - 1) / G) + 3) / 4 * 4;
  if ((size_t)(2 * slice * G) > ar_scratch_floats) return ring();
  // (the count arrays live as long as the model: a transport may key its own bookkeeping on their addresses, as TorchComm does)
  auto& plan = direct_plans[count];
  if (plan.empty()) {
    plan.resize(2 * (size_t)G);
    for (int p = 0; p < G; p++) plan[p] = std::max<int64_t>(0, std::min<int64_t>(slice, count - (int64_t)p * slice));
    for (int q = 0; q < G; q++) plan[G + q] = plan[rank];
  }
  const int64_t* sc = plan.data();
  const int64_t* rc = plan.data() + G;
  const int64_t mine = sc[rank];
  float* r1 = ar_scratch;                    // [G][mine]: slice `rank` as every rank holds it
  float* r2 = ar_scratch + (size_t)slice * G;   // [G][slice]: the sums
  if (a2a(config.comm.user, buf, sc, r1, rc, s) != 0) return 1;
  if (api->ffh_sum_slices_f32(ctx, r1, r1, G, mine, mine, s) != FFH_OK) return 1;
  if (gather(config.comm.user, r1, r2, slice, s) != 0) return 1;
  if (api->ffh_memcpy_d2d(ctx, buf, r2, (size_t)count * 4, s) != FFH_OK) return 1;
  n_direct_allreduces++;
  return 0;
}

bool FFModel::bucketed_now() const {
  if (!exchange || grad_buckets.empty() || use_workers() || config.profiling) return false;
  if (config.bucket_allreduce == 0) return false;
  if (config.bucket_allreduce == 1) return true;
  // by default: where the transport only enqueues (a host-blocking one would stall the launches of the rest of the backward) and the
  // slab makes at least two buckets -- a single one cannot start before the last weight gradient anyway, and its detour over the
  // bucket stream costs two event hops (Kaggle shape, one forced rank: 0.209 vs 0.198 ms)
  return config.comm.nonblocking != 0 && grad_buckets.size() >= 2;
}
int FFModel::big_dw_chunks_now() const {
  if (!bucketed_now()) return 1;
  int n = 0;
  for (const GradBucket& b : grad_buckets) n += b.chunk_layer >= 0;
  return n > 1 ? n : 1;
}
// Issues every bucket whose layers (indices > next_layer) have all issued their backward.  The bucket's stream waits for what the
// compute stream and the weight-gradient streams hold at this point -- the layers' dW / db launches among it -- then runs the sum.
// While a capture is open (--capture-exchange) the sum goes on the capturing stream itself: with RCCL work on a stream that joined
// the capture through an event hipStreamEndCapture recurses (profiles/r04_capture_exchange_endcapture_backtrace.txt).
bool FFModel::buckets_held() const {
  return !config.comm.bucket_channel_own && !shards.empty() && !embeddings.empty() && fused_embedding_update() && !bwd_alltoall_issued;
}
void FFModel::issue_grad_buckets(int next_layer) {
  // A transport that serves the buckets on the SAME channel as the all-to-alls (ffcomm.bucket_channel_own == 0: one RCCL communicator runs its
  // collectives in issue order, whatever streams they are on): nothing goes out before this step's backward all-to-all has been enqueued --
  // otherwise the exchange of the embedding gradients, the table update and the next gather behind it would wait for the biggest layer's
  // weight-gradient GEMM and its all-reduce (round-5 advisor).  The held buckets follow at the next layer boundary.
  if (buckets_held()) return;
  for (size_t k = 0; k < grad_buckets.size(); k++) {
    GradBucket& b = grad_buckets[k];
    if (b.issued || b.lowest_layer <= next_layer) continue;
    issue_one_bucket(k, true);
  }
}
void FFModel::issue_one_bucket(size_t k, bool wait_main) {
  GradBucket& b = grad_buckets[k];
  const bool inline_now = capturing_trace >= 0 || config.capture_exchange;
  ffh_stream s = inline_now ? stream : ar_stream;
  if (dw_worker) dw_worker->drain();
  if (!inline_now && wait_main) {
    check(api->ffh_event_record(ctx, b.ready, stream), "bucket ready");
    check(api->ffh_stream_wait_event(ctx, s, b.ready), "bucket ready");
  }
  // (the weight-gradient streams: joined where this step has used them so far -- a bucket whose layers kept everything on `stream`
  //  waits for nothing extra; inline, `stream` itself takes the waits)
  if (dw_forked && dw1_used) { check(api->ffh_event_record(ctx, b.ready_dw, dw_stream), "bucket ready"); check(api->ffh_stream_wait_event(ctx, s, b.ready_dw), "bucket ready"); }
  if (k < 8) probe_record(14 + 2 * (int)k, s, ctx);
  if (allreduce_grads(mlp_grads + b.off, (int64_t)b.count, s, true) != 0) die("allreduce (bucket) failed");
  if (k < 8) probe_record(15 + 2 * (int)k, s, ctx);
  if (!inline_now) check(api->ffh_event_record(ctx, b.done, s), "bucket done");
  b.issued = true;
  b.inline_issued = inline_now;
  n_bucket_allreduces++;
}
