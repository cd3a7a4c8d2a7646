// model_step.cc -- the training step
// (one of the translation units of the host shim: model_internal.h lists them)
#include "model_internal.h"

// =============================================================================================
// the training step [ref: src/runtime/model.cc:1410-1477, examples/cpp/DLRM/dlrm.cc:166-182]
// =============================================================================================
void FFModel::reset_metrics() {
  if (replaying_trace >= 0) return;
  check(api->ffh_zero(ctx, d_perf, sizeof(ffh_perf_metrics), stream), "reset_metrics");
  if (d_bce_sum) check(api->ffh_zero(ctx, d_bce_sum, sizeof(float), stream), "reset_metrics");
}

// tensor-op mode: the weights' bf16 twin after a host write / (re)initialisation.  Called where a step STARTS -- from begin_trace()
// ahead of a capture or a replay (a replayed forward() returns at once, and a conversion captured into the graph would run on
// every replay) and from forward() for eager steps: the captured GEMMs of a replayed step never read a stale twin.
void FFModel::refresh_weight_twin() const {
  if (!w_twin || !w_twin_dirty) return;
  if (config.fp32_split_bf16x3 && !config.allow_tensor_op_math_conversion) check(api->ffh_convert_f32_to_bf16x3(ctx, mlp_weights, 1, (int64_t)mlp_count, (int64_t)mlp_count, stream), "weight image");
  else check(api->ffh_convert_f32_to_bf16(ctx, w_twin, mlp_weights, (int64_t)mlp_count, stream), "weight twin");
  w_twin_dirty = false;
}
int64_t FFModel::weight_mirror_stale_bytes() {
  if (!w_twin) return -1;
  if (w_twin_dirty) return -2;
  sync();
  const bool x3 = config.fp32_split_bf16x3 && !config.allow_tensor_op_math_conversion;
  const size_t bytes = x3 ? FFH_BF16X3_IMAGE_BYTES((size_t)mlp_count * 4) : (size_t)mlp_count * 2;
  std::vector<char> kept(bytes), fresh(bytes);
  check(api->ffh_memcpy_d2h(ctx, kept.data(), w_twin, bytes, stream), "weight mirror d2h");
  w_twin_dirty = true;
  refresh_weight_twin();
  check(api->ffh_memcpy_d2h(ctx, fresh.data(), w_twin, bytes, stream), "weight mirror d2h");
  check(api->ffh_stream_sync(ctx, stream), "weight mirror sync");
  int64_t n = 0;
  for (size_t i = 0; i < bytes; i++) n += kept[i] != fresh[i];
  return n;
}
void FFModel::note_weight_write(const void* p) const {
  // --eval-embedding-dtype int8: every host-side write of a tensor (initializers, set(), the checkpoint loader) passes here.  Only a write of a table
  // that has an image leaves the images behind: set() on an input or a label between eval_batch() calls must not cost a quantizer pass per batch
  // (before compile() has allocated the images they are stale anyway)
  for (const Embedding* e : embeddings)
    if (e->q8_rows && e->weights[0].impl && p == e->weights[0].impl->ptr) { q8_stale = true; break; }
  if (w_twin && (const char*)p >= (const char*)mlp_weights && (const char*)p < (const char*)(mlp_weights + mlp_count)) w_twin_dirty = true;
}

void FFModel::forward(int _seq_length) {
  if (replaying_trace >= 0) return;
  seq_length = _seq_length;
  if (capturing_trace < 0) refresh_weight_twin();      // (a capture: begin_trace() did it on the stream, outside the graph)
  emb_forward_issued = emb_forward_joined = false;
  fold_w_recorded = fold_on_side = false;
  // gather (+ all-to-all) go to the side stream beside the bottom MLP: the fork point is here (inputs ready)
  if (config.overlap_embedding && !embeddings.empty()) {
    // The side stream already runs behind everything it depends on from earlier steps (the table update is on it);
    // what it must additionally see is a batch that was copied in on `stream`.  No new batch (the reference reuses
    // the warm-up batch for random input), no event: each record / wait is a barrier packet on the critical stream.
    // Exception: data-parallel (replicated) tables live in the dense parameter slab, which the optimizer of the step before
    // wrote on `stream` (all-reduce + SGD / Adam in update()): their gather must always be ordered behind it.
    // ... and so must the gather of EVERY table when the tables are updated by the dense path, which runs on `stream` in update().
    fork_recorded = inputs_dirty || capturing_trace >= 0 || use_workers() || repl_workspace != nullptr || !fused_embedding_update();
    if (fork_recorded) check(api->ffh_event_record(ctx, ev_fork, stream), "fork");
    inputs_dirty = false;
    // start the gather right now unless a host-side collective would stall THIS thread's launches
    // folded tables: their products read the weights the optimizer of the step before wrote on `stream`.  The gather deliberately does
    // not wait for that launch (fork_recorded above), so the products get a dependency of their own
    if (fold.layer && !use_workers()) {
      check(api->ffh_event_record(ctx, ev_fold_w, stream), "fold: weights ready");
      fold_w_recorded = true;
    }
    if (!exchange || config.comm.nonblocking || use_workers()) issue_embedding_forward_on_side_stream();
  }
  for (Op* op : layers) {
    if (!config.profiling) { op->forward(*this); continue; }
    if (op->op_type == OP_EMBEDDING && emb_forward_issued) continue;      // the first table launched the whole group
    profiled(op, true, [&] { op->forward(*this); });
  }
  if (emb_forward_issued && !emb_forward_joined) join_embedding_forward();
}

// One op between two events on `stream`, waited for and printed in the reference's formats
// [ref: src/ops/linear.cu:525-546,761; src/ops/concat.cu:282-297,400-412; src/ops/batch_matmul.cu:303-318,476-494].
void FFModel::profiled(const Op* op, bool fwd, const std::function<void()>& fn) const {
  ffh_event e0, e1;
  check(api->ffh_event_create(ctx, &e0), "event");
  check(api->ffh_event_create(ctx, &e1), "event");
  check(api->ffh_event_record(ctx, e0, stream), "event");
  fn();
  check(api->ffh_event_record(ctx, e1, stream), "event");
  check(api->ffh_event_sync(ctx, e1), "event");
  float ms = 0.0f;
  check(api->ffh_event_elapsed_ms(ctx, e0, e1, &ms), "event");
  api->ffh_event_destroy(ctx, e0);
  api->ffh_event_destroy(ctx, e1);
  const char* dir = fwd ? "forward" : "backward";
  switch (op->op_type) {
    case OP_LINEAR:
      if (fwd) printf("%s [Linear] forward time = %.2lfms\n", op->name, (double)ms);
      else printf("Linear backward time = %.2lfms\n", (double)ms);
      break;
    case OP_BATCHMATMUL: printf("BatchMatmul %s time = %.2lfms\n", dir, (double)ms); break;
    case OP_EMBEDDING:   // the reference dumps tensors here (src/ops/embedding.cu:266-271); one launch serves every table
      printf("[Embedding x%zu] %s time = %.4f ms\n", embeddings.size(), dir, ms);
      break;
    default: printf("[%s] %s time = %.4f ms\n", op->name, dir, ms); break;   // Concat's format (its backward also says "forward" in the reference, :412)
  }
}

void FFModel::issue_embedding_forward_on_side_stream() const {
  if (use_workers()) {
    const FFModel* self = this;
    side_worker->post([self](ffh_ctx* wc) {
      self->check(self->api->ffh_stream_wait_event(wc, self->side_stream, self->ev_fork), "fork");
      self->embedding_group_forward(self->side_stream, wc);
      self->check(self->api->ffh_event_record(wc, self->ev_join, self->side_stream), "join");
    });
  } else {
    if (fork_recorded) check(api->ffh_stream_wait_event(ctx, side_stream, ev_fork), "fork");
    probe_record(0, side_stream, ctx);
    embedding_group_forward(side_stream);
    probe_record(1, side_stream, ctx);
    check(api->ffh_event_record(ctx, ev_join, side_stream), "join");
    if (fold.layer && fold_w_recorded) {
      // behind the gather: this stream already stands behind the table update of the step before (it ran here), ev_fold_w adds the
      // optimizer.  The bottom MLP's forward is the window; what sticks out of it the first top layer waits for (ev_fold_done)
      check(api->ffh_stream_wait_event(ctx, side_stream, ev_fold_w), "fold: weights ready");
      fold_products_and_sum(side_stream, ctx);
      check(api->ffh_event_record(ctx, ev_fold_done, side_stream), "fold: sum ready");
      fold_on_side = true;
    }
    if (early_sort_possible(1)) {       // behind the join: nothing waits for it until this step's update
      launch_shard_groups(this, kSortOnly, side_stream, ctx);
      emb_sorted_early = true;
    }
  }
  emb_forward_issued = true;
  emb_forward_joined = false;
}

void FFModel::fold_products_and_sum(ffh_stream s, ffh_ctx* cx) const {
  const Linear* li = fold.layer;
  const Embedding* e0 = fold.tables[0];
  check(api->fold->ffh_fold_product(cx, fold.groups.data(), (int)fold.groups.size(), (const float*)li->weights[0].impl->ptr, li->in_padded, e0->out_channels,
                                    li->out_channels, s), "fold_product");
  check(api->fold->ffh_fold_gather_add(cx, fold.gather.data(), (int)fold.gather.size(), e0->inputs[0].adim[0], li->out_channels, local_batch, FFH_AGGR_MODE_SUM,
                                       fold.S, li->out_channels, s), "fold_gather_add");
}

// The weight gradient of the layer the tables are folded out of, on `dws` (which stands behind "dy is ready"): G_t = the segmented sum of dy over
// table t's rows, the layer's weight-gradient GEMM over the column tiles that are left (with the bias gradient), dW[:, cols_t] += G_t^T E_t.
// The same launches with the same arguments every step: a captured step holds them as they are.
// `gemm_stream` is `dws`, or the compute stream (fold_dw_on_compute): the GEMM reads x and dy, which are final there, and adds into columns of dW the
// products do not touch, so nothing but stream order ever held it behind the sum.  Inside backward() it is then put off until the layers below have
// issued their backward: right behind the data gradient it keeps the segmented sum from finishing (the sum crawls beside a persistent GEMM, and the
// products, the dense table update and the optimizer wait for it) and only swaps places with the bottom MLP's data gradients.
void FFModel::fold_weight_gradient(const Linear* li, float* dbp, ffh_stream dws, ffh_stream gemm_stream) const {
  const Tensor& y = li->outputs[0];
  const Embedding* e0 = fold.dw_tables[0];
  const int64_t b = local_rows(y, this);
  const int out = li->out_channels, ng = (int)fold.dw_groups.size();
  if (api->fold->ffh_fold_segment_sum(fold.sum_ctx, fold.dw_sum.data(), ng, e0->inputs[0].adim[0], out, b, dws) != FFH_OK)
    die("%s: fold_segment_sum failed: %s", li->name, api->ffh_last_error_string(fold.sum_ctx));
  // The products in FRONT of the GEMM (both only add into dW, disjoint columns): they read the tables' rows, which this step's table update
  // overwrites on the side stream as soon as the data gradients are complete -- long before the GEMM ends.  The update waits for ev_fold_e_read.
  check(api->fold->ffh_fold_dw_product(ctx, fold.dw_groups.data(), ng, li->weights[0].impl->grad, li->in_padded, e0->out_channels, out, dws), "fold_dw_product");
  // (--serial-dw as well: "gradients ready" is recorded behind the data-gradient kernel, in front of these launches)
  check(api->ffh_event_record(ctx, ev_fold_e_read, dws), "fold: table rows read");
  fold_e_read_recorded = true;
  // (dbp: null where the layer above has produced this layer's bias gradient already -- Linear::backward_part consumed db_from_upper)
  if (gemm_stream != dws && fold_dw_defer) { fold_dw_pending = li; fold_dw_pending_db = dbp; return; }      // backward() issues it behind the layers below
  fold_kept_dw_gemm(li, dbp, gemm_stream, gemm_stream != dws);
}
void FFModel::fold_kept_dw_gemm(const Linear* li, float* dbp, ffh_stream s, bool off_dw_stream) const {
  const Tensor &x = li->inputs[0], &y = li->outputs[0];
  check(api->fold->ffh_fold_linear_bwd_dw(ctx, (const float*)x.impl->ptr, x.impl->ld, y.impl->grad, y.impl->grad_ld, li->weights[0].impl->grad, dbp, li->in_padded, li->out_channels,
                                          local_rows(y, this), fold.dw_kept.data(), (int)fold.dw_kept.size(), s), li->name);
  if (off_dw_stream) {
    // off the weight-gradient stream, neither ev_z_free nor ev_dw_done says that this reader of the Concat output is done: an event of its own for the
    // next gather (update() makes the side stream wait for it; in a captured step that wait is the graph edge)
    check(api->ffh_event_record(ctx, ev_fold_x_read, s), "fold: layer input read");
    fold_x_read_recorded = true;
    n_fold_dw_on_compute++;
  }
}
bool FFModel::fold_schedule_route() const {
  return fold.layer && !fold.dw_tables.empty() && fold.layer->forks_dw(*this) && config.overlap_embedding && !use_workers() && !config.profiling;
}
bool FFModel::fold_dw_on_compute() const { return fold_schedule_route() && !config.fold_dw_behind_sum; }
bool FFModel::fold_update_early() const { return fold_schedule_route() && fold.dx && !config.fold_update_behind_products; }

// The plain-SGD step of the dx-folded tables as one dense product (include/ff_hip_fold.h, ABI 3): E_t[r] = fmaf(-lr, G_t[r] W[:, cols_t], E_t[r]).  The rate
// as the sparse update of the other tables takes it: from the table update's block in device memory, or the optimizer's scalar.
void FFModel::fold_table_update(ffh_stream s, ffh_ctx* cx) const {
  const Linear* li = fold.layer;
  const Embedding* e0 = fold.dw_tables[0];
  const int ng = (int)fold.dw_groups.size();
  const float* w = (const float*)li->weights[0].impl->ptr;
  if (lr_route == kLrDevice) {
    check(api->fold->ffh_fold_table_update_lr(cx, fold.dw_groups.data(), ng, w, li->in_padded, e0->out_channels, li->out_channels, lr_block[1], s), "fold_table_update_lr");
  } else {
    ffh_sparse_opt rule;
    sparse_rule(rule);      // (plain SGD: plan_fold_dx)
    check(api->fold->ffh_fold_table_update(cx, fold.dw_groups.data(), ng, w, li->in_padded, e0->out_channels, li->out_channels, rule.lr, s), "fold_table_update");
  }
}
bool FFModel::fold_dx_table(const Embedding* e) const {
  if (!fold.dx) return false;
  for (const Embedding* t : fold.dw_tables) if (t == e) return true;
  return false;
}

// forward() of the layer the tables are folded out of.  The gather has been joined (the Concat below comes first), so `stream` stands behind
// this step's tables either way: the sum is waited for where the side stream computed it, and computed right here otherwise
void FFModel::fold_linear_forward(const Linear* li) const {
  if (fold_on_side) check(api->ffh_stream_wait_event(ctx, stream, ev_fold_done), "fold: sum ready");
  else fold_products_and_sum(stream, ctx);
  const Tensor& x = li->inputs[0];
  const Tensor& y = li->outputs[0];
  check(api->fold->ffh_fold_linear_fwd(ctx, (const float*)x.impl->ptr, x.impl->ld, (float*)y.impl->ptr, y.impl->ld, (const float*)li->weights[0].impl->ptr,
                                       li->use_bias ? (const float*)li->weights[1].impl->ptr : nullptr, li->in_padded, li->out_channels, local_rows(y, this),
                                       (int)li->activation, fold.keep.data(), (int)fold.keep.size(), fold.S, li->out_channels, stream), li->name);
}

void FFModel::join_embedding_forward() const {
  if (side_worker) side_worker->drain();   // the record of ev_join must have been issued before we wait on it
  probe_record(10, stream, ctx);           // bench probes: what the compute stream waits here is the EXPOSED part of gather + exchange
  check(api->ffh_stream_wait_event(ctx, stream, ev_join), "join");
  probe_record(11, stream, ctx);
  emb_forward_joined = true;
}

void FFModel::issue_embedding_update_on_side_stream() const {
  if (use_workers()) {
    const FFModel* self = this;
    side_worker->post([self](ffh_ctx* wc) {
      self->check(self->api->ffh_stream_wait_event(wc, self->side_stream, self->ev_grad_ready), "event");
      self->embedding_group_update(self->side_stream, wc);
      self->check(self->api->ffh_event_record(wc, self->ev_update_done, self->side_stream), "event");
    });
  } else {
    check(api->ffh_stream_wait_event(ctx, side_stream, ev_grad_ready), "event");
    if (fold_update_early()) {
      // The sparse update of the tables that are left needs the kept data gradient only: with dx folding it writes no table of fold.dw_groups (launch_shard_groups
      // skips them), and those are the only rows the products G_t^T E_t read, so it does not wait for ev_fold_e_read.  It runs on the model's ctx and workspace
      // while the segmented sum may still run on fold.sum_ctx and its own.  The dense update of the folded tables follows it, behind ev_fold_e_read as before; the
      // rate block both read advances behind the second reader.
      if (!fold_e_read_recorded) die("fold: the dx-folded tables' update without this step's segmented sum");
      probe_record(2, side_stream, ctx);
      embedding_group_update(side_stream, nullptr, false);
      check(api->ffh_stream_wait_event(ctx, side_stream, ev_fold_e_read), "fold: table rows read");
      fold_table_update(side_stream, ctx);
      check(api->ffh_event_record(ctx, ev_fold_w_read, side_stream), "fold: weights read");
      fold_w_read_recorded = true;
      advance_lr(1, side_stream, ctx);
      probe_record(3, side_stream, ctx);
      check(api->ffh_event_record(ctx, ev_update_done, side_stream), "event");
      n_fold_update_early++;
      return;
    }
    if (fold_e_read_recorded) check(api->ffh_stream_wait_event(ctx, side_stream, ev_fold_e_read), "fold: table rows read");      // (fold_weight_gradient)
    probe_record(2, side_stream, ctx);
    if (fold.dx) {
      // the dx-folded tables first: E_t -= lr G_t W[:, cols_t].  Behind ev_fold_e_read the products G_t^T E_t have read E_t and (the same stream, in front
      // of them) the segmented sum has completed G.  It reads W, which the slab optimizer rewrites on `stream`: update() waits for ev_fold_w_read
      if (!fold_e_read_recorded) die("fold: the dx-folded tables' update without this step's segmented sum");
      fold_table_update(side_stream, ctx);
      check(api->ffh_event_record(ctx, ev_fold_w_read, side_stream), "fold: weights read");
      fold_w_read_recorded = true;
    }
    embedding_group_update(side_stream);
    probe_record(3, side_stream, ctx);
    check(api->ffh_event_record(ctx, ev_update_done, side_stream), "event");
  }
}

// Writers of the model inputs on `stream` (the data loader's next batch) go behind the side-stream table update of the
// step before, which still sorts and reads the sparse ids.
void FFModel::order_input_writes_behind_update() const {
  if (embeddings.empty() || !config.overlap_embedding || !fused_embedding_update()) return;
  if (side_worker) side_worker->drain();       // the record of ev_update_done must have been issued
  check(api->ffh_stream_wait_event(ctx, stream, ev_update_done), "inputs behind the table update");
}

void FFModel::zero_gradients() {
  if (replaying_trace >= 0) return;
  // Op::zero_grad for every layer [ref: src/runtime/model.cc:466-490]: two slabs instead of ~34 tasks.
  // Embedding tables have no dense gradient on the fused path (nothing to zero: SURVEY fact 1).
  // activation gradients with a single producer are stored, not accumulated: nothing to clear (0 + x == x)
  if (need_zero_act_grads) check(api->ffh_zero(ctx, act_grad_slab, act_grad_bytes, stream), "zero_gradients");
  if (!mlp_grads_clean) check(api->ffh_zero(ctx, mlp_grads, mlp_count * 4, stream), "zero_gradients");
  if (exchange && gsend && need_zero_gsend) {
    size_t n = 0;
    for (int64_t c : fwd_recv_counts) n += (size_t)c;
    check(api->ffh_zero(ctx, gsend, n * 4, stream), "zero_gradients");
  }
  if (!fused_embedding_update())
    for (Embedding* e : embeddings)
      if (e->held_here(rank) && !e->replicated)
        check(api->ffh_zero(ctx, e->weights[0].impl->grad, e->weights[0].impl->bytes + (e->row_sharded ? (size_t)e->out_channels * 4 : 0), stream), "zero_gradients");
}

void FFModel::compute_metrics() {
  if (replaying_trace >= 0) return;
  const Tensor& fin = layers.back()->outputs[0];
  check(api->ffh_metrics_update(ctx, (const float*)fin.impl->ptr, (const float*)label_tensor.impl->ptr, d_perf,
                                local_rows(fin, this), fin.adim[0], metrics_flags, stream), "compute_metrics");
}

void FFModel::backward(int _seq_length) {
  q8_stale = true;               // the table update may start from here (a replayed step: the graph holds it)
  if (replaying_trace >= 0) return;
  seq_length = _seq_length;
  if (config.computationMode != COMP_MODE_TRAINING) die("backward() in inference mode");
  // compute_metrics() + loss backward [ref: src/runtime/model.cc:1443-1452; src/loss_functions/loss_functions.cu:141-170,196-237]
  // in one launch; scale_factor = 1 / global batch
  const Tensor& fin = layers.back()->outputs[0];
  const bool bce = loss_type == LOSS_BINARY_CROSSENTROPY;      // mean over the global batch, dz at the pre-activation (include/ff_hip_ctr.h)
  const float scale = (bce || loss_type == LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE) ? 1.0f / (float)fin.adim[fin.numDim - 1] : 1.0f;
  if (fin.impl->grad_ld != fin.adim[0] || fin.impl->ld != fin.adim[0]) die("final layer output must be contiguous");
  dw_forked = false;
  fold_e_read_recorded = false;
  fold_w_read_recorded = false;
  fold_x_read_recorded = false;
  fold_dw_pending = nullptr;
  fold_dw_defer = true;      // (a layer's backward() called on its own -- time_kernel(7) -- issues the GEMM at once)
  fold_dx_event = nullptr;
  opt_next_done = false;
  // the click-probability layer (out = 1): loss step + metrics + the layer's whole backward in ONE launch; any other last
  // layer: the loss kernel, then the layer's own backward
  int first = (int)layers.size() - 1;
  emb_update_pending = false;
  mlp_grads_clean = false;
  Linear* last = (config.fuse_loss && !config.profiling) ? dynamic_cast<Linear*>(layers.back()) : nullptr;   // --profiling: the loss kernel and every layer on their own
  int rc = FFH_ERR_UNSUPPORTED;
  if (last) {
    const Tensor& x = last->inputs[0];
    const int flags = (last->dx_overwrite ? FFH_LINEAR_DX_OVERWRITE : 0) | (last->dx_mask_by_x ? FFH_LINEAR_DX_MASK_BY_X : 0);
    if (bce)
      rc = api->ctr->ffh_linear_bwd_bce(ctx, (const float*)x.impl->ptr, x.impl->ld, last->discard_input_grad ? nullptr : x.impl->grad, x.impl->grad_ld,
                                        (const float*)fin.impl->ptr, fin.impl->ld, fin.impl->grad, fin.impl->grad_ld,
                                        (const float*)last->weights[0].impl->ptr, last->weights[0].impl->grad,
                                        last->use_bias ? last->weights[1].impl->grad : nullptr, last->in_channels, last->out_channels,
                                        local_rows(fin, this), (int)last->activation, flags, (const float*)label_tensor.impl->ptr, scale, d_perf,
                                        d_bce_sum, metrics_flags, stream);
    else
    rc = api->ffh_linear_bwd_mse(ctx, (const float*)x.impl->ptr, x.impl->ld, last->discard_input_grad ? nullptr : x.impl->grad, x.impl->grad_ld,
                                 (const float*)fin.impl->ptr, fin.impl->ld, fin.impl->grad, fin.impl->grad_ld,
                                 (const float*)last->weights[0].impl->ptr, last->weights[0].impl->grad,
                                 last->use_bias ? last->weights[1].impl->grad : nullptr, last->in_channels, last->out_channels,
                                 local_rows(fin, this), (int)last->activation, flags, (const float*)label_tensor.impl->ptr, scale, d_perf,
                                 metrics_flags, stream);
    if (rc == FFH_OK) n_fused_loss_calls++;
    if (rc == FFH_OK) first--;                          // the last layer is done
    else if (rc != FFH_ERR_UNSUPPORTED) check(rc, "loss + last layer backward");
  }
  if (rc != FFH_OK && bce)      // the two-call route: the final layer then runs with FFH_LINEAR_DY_PREMASKED (compile() set dy_premasked)
    check(api->ctr->ffh_bce_bwd_metrics(ctx, fin.impl->grad, (const float*)fin.impl->ptr, (const float*)label_tensor.impl->ptr, d_perf, d_bce_sum,
                                        local_rows(fin, this), fin.adim[0], scale, metrics_flags, stream), "metrics + loss backward (bce)");
  else if (rc != FFH_OK)
    check(api->ffh_mse_bwd_metrics(ctx, fin.impl->grad, (const float*)fin.impl->ptr, (const float*)label_tensor.impl->ptr, d_perf,
                                   local_rows(fin, this), fin.adim[0], scale, metrics_flags, stream), "metrics + loss backward");
  grad_ready_attached = false;
  z_free_recorded = false;
  auto mark_z_free = [&](int l) {     // behind the last reader of the gather's destination among the forked weight-gradient GEMMs
    if (l == z_reader_layer && dw_forked && !dw_worker && capturing_trace < 0) {
      check(api->ffh_event_record(ctx, ev_z_free, dw_stream), "z free");
      z_free_recorded = true;
    }
  };
  bwd_alltoall_issued = false;
  for (GradBucket& b : grad_buckets) b.issued = b.inline_issued = false;
  const int dw_chunks = big_dw_chunks_now();
  // the biggest layer with the bucketed all-reduce: data gradient, then its weight gradient in row blocks, a bucket behind each
  auto chunked_big_backward = [&](Linear* up, int l) {
    // (dy is final here: the weight-gradient stream forks in FRONT of the data gradient, as the library's own fork does, and the GEMMs of
    //  the row blocks run beside it)
    ffh_event ev = layer_events[l];
    check(api->ffh_event_record(ctx, ev, stream), "event");
    check(api->ffh_stream_wait_event(ctx, dw_stream, ev), "event");
    up->backward_part(*this, 1);
    const int per = up->out_channels / dw_chunks;
    for (size_t k = 0; k < grad_buckets.size(); k++) {
      GradBucket& b = grad_buckets[k];
      if (b.chunk_layer != l) continue;
      up->backward_dw_rows(*this, b.chunk_index * per, per);
      if (!buckets_held()) issue_one_bucket(k, false);      // (held: issue_grad_buckets sends it once the backward all-to-all is enqueued)
    }
    up->db_from_upper = false;
  };
  for (int l = first; l >= 0; l--) {
    if (bucketed_now()) issue_grad_buckets(l);     // the buckets every layer above l has completed
    if (l == grad_attach_layer) {
      // (the dx-folded layer takes the event as an argument of its data-gradient call: nothing armed in the ctx)
      if (fold.dx && layers[l] == fold.layer) fold_dx_event = ev_grad_ready;
      else check(api->ffh_event_record_with_next_linear_bwd(ctx, ev_grad_ready), "attach event");
      grad_ready_attached = true;
    }
    Linear* up = layers[l]->op_type == OP_LINEAR ? static_cast<Linear*>(layers[l]) : nullptr;
    if (up && up->dx_map && !use_workers()) {
      const bool attach = l == scatter_attach_layer;
      check(api->ffh_linear_bwd_set_dx_scatter(ctx, up->dx_map, up->in_channels, attach ? ev_grad_ready : nullptr), "dx scatter");
      if (dw_chunks > 1 && l == big_dw_layer) { chunked_big_backward(up, l); mark_z_free(l); }
      else { up->backward(*this); mark_z_free(l); }
      if (api->ffh_linear_dx_scatter_used(ctx)) {
        up->dx_map_concat->bwd_done = true;                    // its pack kernel is not needed this step
        if (attach) grad_ready_attached = true;
      }
      continue;
    }
    if (config.profiling) {
      if (layers[l]->op_type == OP_EMBEDDING && static_cast<Embedding*>(layers[l])->table_index != (int)embeddings.size() - 1) continue;
      profiled(layers[l], false, [&] {
        layers[l]->backward(*this);
        // the fused sparse update of the tables is the embedding group's backward here (it runs in update() otherwise)
        if (layers[l]->op_type == OP_EMBEDDING && fused_embedding_update()) embedding_group_update(stream);
      });
      continue;
    }
    if (up && !up->chain_bwd.empty() && mlp_chain_usable(local_rows(up->outputs[0], this), false)) {
      // the chain this layer tops: one call for all its members (their indices are l - n + 1 .. l)
      const int n = (int)up->chain_bwd.size();
      const int crc = run_chain_bwd(up);
      if (crc == FFH_OK) {
        // a lower member completes the embedding output gradients: "gradients ready" behind the whole call (the chain's weight-gradient
        // kernel still reads the buffer the next gather overwrites).  (l itself: attached above, recorded by the call.)
        if (grad_attach_layer > l - n && grad_attach_layer < l && !grad_ready_attached) {
          check(api->ffh_event_record(ctx, ev_grad_ready, stream), "event");
          grad_ready_attached = true;
        }
        for (int k = 0; k < n; k++) mark_z_free(l - k);
        l -= n - 1;
        continue;
      }
      if (crc != FFH_ERR_UNSUPPORTED) check(crc, up->name);
      up->chain_bwd.clear();                                   // not a chain the library serves: the per-layer calls from now on
    }
    if (up && up->pair_lower && !use_workers() && l != grad_attach_layer && l >= 1 && layers[l - 1] == up->pair_lower) {
      const int prc = up->backward_pair(*this);
      if (prc == FFH_OK) { l--; continue; }                   // the lower layer is done as well
      if (prc != FFH_ERR_UNSUPPORTED) check(prc, up->name);
      up->pair_lower = nullptr;                                // not a shape the pair launch serves: the ordinary calls from now on
    }
    if (up && dw_chunks > 1 && l == big_dw_layer) { chunked_big_backward(up, l); mark_z_free(l); continue; }
    layers[l]->backward(*this);
    mark_z_free(l);
  }
  fold_dw_defer = false;
  if (fold_dw_pending) {
    // the fold layer's kept-tile weight-gradient GEMM, behind the backward of the layers below it on `stream` (fold_dw_on_compute)
    fold_kept_dw_gemm(fold_dw_pending, fold_dw_pending_db, stream, true);
    fold_dw_pending = nullptr;
  }
  if (emb_update_pending) {
    // exchange of the row gradients + fused sparse update on the side stream, beside the bottom-MLP backward
    issue_embedding_update_on_side_stream();
    emb_update_pending = false;
  }
  // what is left (a shared channel: the buckets held until the exchange above was enqueued; a model whose backward all-to-all runs in update():
  // released here all the same -- update() waits for every bucket)
  if (bucketed_now()) { bwd_alltoall_issued = true; issue_grad_buckets(-1); }
}

void FFModel::update() {
  n_update_calls++;              // (a replayed step counts: its update is in the graph)
  q8_stale = true;               // ... and so the 8-bit row images of the tables are behind (--eval-embedding-dtype int8)
  if (replaying_trace >= 0) return;
  optimizer->next();
  opt_next_done = true;
  SGDOptimizer* sgd = dynamic_cast<SGDOptimizer*>(optimizer);
  AdamOptimizer* adam = dynamic_cast<AdamOptimizer*>(optimizer);
  AdagradOptimizer* adagrad = dynamic_cast<AdagradOptimizer*>(optimizer);
  if (!sgd && !adam && !adagrad) die("update(): unknown optimizer");
  // every rank must issue its collectives in the same order: the side thread's all-to-all (backward) first
  if (side_worker) side_worker->drain();
  if (dw_forked && !dw_worker && !api->ffh_second_stream_used(ctx, 1) && !dw_stream_used_directly) { dw_forked = false; dw1_used = false; }   // the library kept everything on `stream`
  dw_stream_used_directly = false;
  if (dw_forked) {   // the weight-gradient GEMMs ran on their own stream: join before the gradients are consumed
    if (dw_worker) { dw_worker->drain(); dw1_used = true; }
    if (dw1_used) {
      check(api->ffh_event_record(ctx, ev_dw_done, dw_stream), "join dw");
      check(api->ffh_stream_wait_event(ctx, stream, ev_dw_done), "join dw");
    }
    // the next gather (side stream) overwrites embedding outputs that alias the Concat output -- the x operand of the first
    // top-MLP layer, which a forked dW GEMM may still be reading: write-after-read across streams
    if (config.overlap_embedding && !embeddings.empty() && !use_workers()) {
      if (z_free_recorded) check(api->ffh_stream_wait_event(ctx, side_stream, ev_z_free), "join dw (embedding stream)");
      else {
        if (dw1_used) check(api->ffh_stream_wait_event(ctx, side_stream, ev_dw_done), "join dw (embedding stream)");
      }
    }
    dw1_used = false;
    dw_forked = false;
  }
  // ... and the kept-tile weight-gradient GEMM of the fold layer reads that buffer on `stream` (fold_dw_on_compute), where neither event above stands behind it
  if (fold_x_read_recorded) { check(api->ffh_stream_wait_event(ctx, side_stream, ev_fold_x_read), "fold: layer input read (embedding stream)"); fold_x_read_recorded = false; }
  // data-parallel MLP gradients: ONE bucket [ref: one ncclAllReduce per tensor, src/runtime/optimizer_kernel.cu:170-171].
  // No 1/world_size: the loss already divides by the global batch.
  if (exchange && mlp_count) {
    bool any_issued = false;
    for (const GradBucket& b : grad_buckets) any_issued = any_issued || b.issued;
    if (any_issued) {
      // the buckets went out from backward() on ar_stream: the optimizer waits for them here (what `stream` stands at these waits is
      // the EXPOSED part of the all-reduce: probe pair 12 / 13), then what no bucket covers is reduced as before
      for (const GradBucket& b : grad_buckets) if (!b.issued) die("update(): a gradient bucket was not issued");
      probe_record(12, stream, ctx);
      for (const GradBucket& b : grad_buckets) if (!b.inline_issued) check(api->ffh_stream_wait_event(ctx, stream, b.done), "join all-reduce bucket");
      probe_record(13, stream, ctx);
      probe_record(8, stream, ctx);
      for (auto& r : grad_rest)
        if (allreduce_grads(mlp_grads + r.first, (int64_t)r.second, stream, false) != 0) die("allreduce failed");
      probe_record(9, stream, ctx);
    } else {
      probe_record(8, stream, ctx);
      if (allreduce_grads(mlp_grads, (int64_t)mlp_count, stream, false) != 0) die("allreduce failed");
      probe_record(9, stream, ctx);
    }
  }
  // the dx-folded tables' update (side stream, issued from backward()) reads the first top layer's weight: the optimizer goes behind it
  if (fold_w_read_recorded) { check(api->ffh_stream_wait_event(ctx, stream, ev_fold_w_read), "fold: weights read"); fold_w_read_recorded = false; }
  // one launch over the whole MLP slab; it also clears the gradients it consumed, so the next zero_gradients()
  // has nothing to sweep [ref: one update task per parameter, src/runtime/optimizer.cc:93-189,256-330]
  const size_t opt_count = mlp_count;
  const ffh_lr_state* lrb = lr_route == kLrDevice ? lr_block[0] : nullptr;     // the rate from device memory (include/ff_hip_lr.h)
  if (adam) {
    if (mlp_count && lrb) {
      check(api->lr->ffh_adam_update_lr(ctx, mlp_weights, mlp_grads, adam->mlp_m, adam->mlp_v, (int64_t)opt_count, lrb, (float)adam->beta1,
                                        (float)adam->beta2, (float)adam->weight_decay, (float)adam->epsilon, FFH_OPT_ZERO_GRAD, stream),
            "adam_update_lr (MLP slab)");
      mlp_grads_clean = true;
    } else if (mlp_count) {
      check(api->ffh_adam_update(ctx, mlp_weights, mlp_grads, adam->mlp_m, adam->mlp_v, (int64_t)opt_count, (float)adam->alpha_t,
                                 (float)adam->beta1, (float)adam->beta2, (float)adam->weight_decay, (float)adam->epsilon,
                                 FFH_OPT_ZERO_GRAD, stream), "adam_update (MLP slab)");
      mlp_grads_clean = true;
    }
  } else if (adagrad) {
    if (mlp_count && lrb) {
      check(api->adagrad->ffh_adagrad_update_lr(ctx, mlp_weights, mlp_grads, adagrad->mlp_s, (int64_t)opt_count, lrb, (float)adagrad->epsilon,
                                                (float)adagrad->weight_decay, FFH_OPT_ZERO_GRAD, stream), "adagrad_update_lr (MLP slab)");
      mlp_grads_clean = true;
    } else if (mlp_count) {
      check(api->adagrad->ffh_adagrad_update(ctx, mlp_weights, mlp_grads, adagrad->mlp_s, (int64_t)opt_count, (float)adagrad->lr, (float)adagrad->epsilon,
                                             (float)adagrad->weight_decay, FFH_OPT_ZERO_GRAD, stream), "adagrad_update (MLP slab)");
      mlp_grads_clean = true;
    }
  } else if (sgd->momentum > 0.0) {
    for (const Parameter& p : parameters)
      if (in_dense_slab(p)) sgd->update(&p);
  } else if (mlp_count && lrb) {
    check(api->lr->ffh_sgd_update_ex_lr(ctx, mlp_weights, mlp_grads, nullptr, (int64_t)opt_count, lrb, (float)sgd->weight_decay, 0.0f, 0, FFH_OPT_ZERO_GRAD,
                                        stream), "sgd_update_ex_lr (MLP slab)");
    mlp_grads_clean = true;
  } else if (mlp_count) {
    check(api->ffh_sgd_update_ex(ctx, mlp_weights, mlp_grads, nullptr, (int64_t)opt_count, (float)sgd->lr, (float)sgd->weight_decay, 0.0f,
                                 0, FFH_OPT_ZERO_GRAD, stream), "sgd_update (MLP slab)");
    mlp_grads_clean = true;
  }
  if (fused_embedding_update()) {
    if (config.overlap_embedding) {
      // launched in backward() on the side stream.  Its only consumer, the next gather, runs on that same stream, and
      // every host read of a table syncs both streams -- so `stream` joins it only where a capture must close the fork
      if (!embeddings.empty() && (capturing_trace >= 0 || use_workers()))
        check(api->ffh_stream_wait_event(ctx, stream, ev_update_done), "join update");
    } else if (!config.profiling) {     // (--profiling: timed as the embedding group's backward)
      embedding_group_update(stream);
    }
  } else {
    embedding_dense_update();
  }
  // the schedule moves on: the dense optimizer's block behind its reader on `stream` (captured with the step, so a replay advances it too);
  // the host route writes the next step's rate into the optimizer object (the table update of that step is issued before its update())
  advance_lr(0, stream, ctx);
  if (lr_route == kLrHost) lr_host_set(++lr_host_steps);
}

bool FFModel::trace_replays(int trace_id) const {
  if (!config.enable_graph) return false;
  auto it = trace_tune.find(trace_id);
  return !(trace_adaptive() && it != trace_tune.end() && it->second.decided == 2);
}

// Adaptive replay (FFConfig::trace_mode 0, one GPU): calls 0-4 of a trace run eagerly -- the first two unmeasured (one-off costs of a first
// launch: code-object loads, hipFuncSetAttribute, a fall-back path taken once; a cold sample biased the choice towards the replay: round-5
// advisor), events behind calls 2 and 4 --, call 5 captures, calls 6-8 replay with events behind 6 and 8; the tenth call compares the spacing
// of the events (eager steps 3-4 against replays 7-8: what a step takes end to end, host gaps included) and keeps the faster form for good.
void FFModel::begin_trace(int trace_id) {
  if (!config.enable_graph) return;
  if (trace_adaptive()) {
    TraceTune& t = trace_tune[trace_id];
    if (t.decided == 2 || (t.decided == 0 && t.calls < 5)) return;      // an eager step
    if (t.decided == 0 && t.calls == 9) {
      check(api->ffh_event_sync(ctx, t.ev[3]), "trace timing");
      check(api->ffh_event_elapsed_ms(ctx, t.ev[0], t.ev[1], &t.eager_ms), "trace timing");
      check(api->ffh_event_elapsed_ms(ctx, t.ev[2], t.ev[3], &t.graph_ms), "trace timing");
      t.decided = t.graph_ms <= 1.02f * t.eager_ms ? 1 : 2;
      for (ffh_event& e : t.ev) { api->ffh_event_destroy(ctx, e); e = nullptr; }
      if (config.profiling || getenv("FFM_TRACE_VERBOSE"))
        fprintf(stderr, "[DLRM] trace %d: eager %.1f us / step, hipGraph replay %.1f us / step -> %s\n", trace_id, t.eager_ms * 500.f, t.graph_ms * 500.f,
                t.decided == 1 ? "replay" : "eager");
      if (t.decided == 2) return;
    }
  }
  refresh_weight_twin();                  // ahead of the capture / the replay, on `stream`
  auto it = graphs.find(trace_id);
  if (it != graphs.end()) { replaying_trace = trace_id; return; }
  if (dw_worker) dw_worker->drain();      // stream capture is thread-local: everything is issued inline while capturing
  if (side_worker) side_worker->drain();
  int rc = api->ffh_graph_begin_capture(ctx, stream);
  if (rc == FFH_ERR_UNSUPPORTED) { config.enable_graph = false; return; }   // backend without graphs: run eagerly
  check(rc, "begin_trace");
  capturing_trace = trace_id;
}

void FFModel::end_trace(int trace_id) {
  if (!config.enable_graph) return;
  TraceTune* tune = nullptr;
  if (trace_adaptive()) {
    TraceTune& t = trace_tune[trace_id];
    if (t.decided == 2) return;
    if (t.decided == 0) {
      auto mark = [&](int k) {
        if (!t.ev[k]) check(api->ffh_event_create(ctx, &t.ev[k]), "event create");
        check(api->ffh_event_record(ctx, t.ev[k], stream), "trace timing");
      };
      if (t.calls < 5) {               // the eager steps: events behind the third and the fifth
        if (t.calls == 2) mark(0);
        if (t.calls == 4) mark(1);
        t.calls++;
        return;
      }
      tune = &t;
    }
  }
  struct TuneMark {                    // behind the graph launch below (calls 6 and 8: two replays apart)
    FFModel* ff; TraceTune* t;
    ~TuneMark() {
      if (!t) return;
      const int k = t->calls == 6 ? 2 : (t->calls == 8 ? 3 : -1);
      if (k >= 0) {
        if (!t->ev[k]) ff->check(ff->api->ffh_event_create(ff->ctx, &t->ev[k]), "event create");
        ff->check(ff->api->ffh_event_record(ff->ctx, t->ev[k], ff->stream), "trace timing");
      }
      t->calls++;
    }
  } tune_mark{this, tune};
  if (capturing_trace == trace_id) {
    ffh_graph g = nullptr;
    check(api->ffh_graph_end_capture(ctx, stream, &g), "end_trace");
    graphs[trace_id] = g;
    capturing_trace = -1;
    check(api->ffh_graph_launch(ctx, g, stream), "graph launch");   // the captured iteration has not run yet
    return;
  }
  if (replaying_trace == trace_id) {
    check(api->ffh_graph_launch(ctx, graphs[trace_id], stream), "graph launch");
    n_graph_replays++;
    replaying_trace = -1;
  }
}

void FFModel::sync() {
  if (dw_worker) dw_worker->drain();
  if (side_worker) side_worker->drain();
  check(api->ffh_stream_sync(ctx, stream), "sync");
  check(api->ffh_stream_sync(ctx, side_stream), "sync");
  check(api->ffh_stream_sync(ctx, dw_stream), "sync");
  check(api->ffh_stream_sync(ctx, ar_stream), "sync");
}

PerfMetrics FFModel::get_perf_metrics() {
  sync();
  ffh_perf_metrics h;
  check(api->ffh_memcpy_d2h(ctx, &h, d_perf, sizeof h, stream), "metrics d2h");
  check(api->ffh_stream_sync(ctx, stream), "sync");
  PerfMetrics p;
  p.train_all = h.train_all; p.train_correct = h.train_correct; p.cce_loss = h.cce_loss;
  p.sparse_cce_loss = h.sparse_cce_loss; p.mse_loss = h.mse_loss; p.rmse_loss = h.rmse_loss; p.mae_loss = h.mae_loss;
  if (d_bce_sum) {
    check(api->ffh_memcpy_d2h(ctx, &p.bce_loss, d_bce_sum, sizeof(float), stream), "metrics d2h");
    check(api->ffh_stream_sync(ctx, stream), "sync");
  }
  return p;
}

// =============================================================================================
// held-out evaluation (include/ff_hip_ctr.h)
// =============================================================================================
void FFModel::reset_eval_metrics() {
  if (!api->ctr) die("reset_eval_metrics(): %s is a kernel library without the CTR extension (include/ff_hip_ctr.h)", api->path.c_str());
  if (capturing_trace >= 0 || replaying_trace >= 0) die("reset_eval_metrics() inside begin_trace / end_trace");
  if (!d_eval) d_eval = (ffh_ctr_eval*)dmalloc(sizeof(ffh_ctr_eval));
  check(api->ffh_zero(ctx, d_eval, sizeof(ffh_ctr_eval), stream), "reset_eval_metrics");
}

void FFModel::eval_batch() {
  if (!compiled) die("eval_batch() before compile()");
  if (capturing_trace >= 0 || replaying_trace >= 0) die("eval_batch() inside begin_trace / end_trace: evaluate between steps");
  const Linear* last = dynamic_cast<const Linear*>(layers.back());
  if (!last || last->activation != AC_MODE_SIGMOID || last->out_channels != 1)
    die("eval_batch(): the final operator must be a Linear with sigmoid activation and one output column (--sigmoid-top)");
  if (!d_eval) reset_eval_metrics();
  // The forward pass as a training step issues it, with two differences: the side-stream gather is always ordered behind `stream` (the
  // batch was just written there, and a replayed step joins its table update into `stream`), and no early sort is issued (it would
  // leave a sorted list of THESE ids in the workspace for the next training step's apply phase).  Nothing else a step carries across its
  // boundary is touched: gradients, the optimizer's step count, the bf16 rounding counter, the captured graphs.
  // --eval-embedding-dtype int8: images that a step, a set() or a load has left behind their tables are made again here, on the calling thread.  sync()
  // drains the launch workers and every stream, so `stream` stands behind the last write of every table; the gather (this stream, or the side stream
  // behind the fork event that inputs_dirty makes forward() record) stands behind the quantizer.  Once per evaluation after training, not per batch.
  if (q8_on() && q8_stale && !embeddings.empty()) {
    sync();
    q8_quantize(stream, ctx);
  }
  evaluating = true;
  inputs_dirty = true;
  forward();
  evaluating = false;
  inputs_dirty = true;     // the next training step's gather: behind whatever writes its batch (and behind this pass's readers)
  const Tensor& fin = layers.back()->outputs[0];
  check(api->ctr->ffh_ctr_eval_update(ctx, (const float*)fin.impl->ptr, (const float*)label_tensor.impl->ptr, d_eval, local_rows(fin, this), stream),
        "eval_batch");
}

// Counts and histograms are summed over the ranks EXACTLY through ffcomm's fp32 all-reduce: every 64-bit count travels as four 16-bit
// pieces, each below 2^16, so a sum over up to 8 ranks stays below 2^19 and is exact in fp32; the pieces are re-assembled in integers.
EvalMetrics FFModel::get_eval_metrics(bool with_histograms) {
  if (!d_eval) reset_eval_metrics();
  sync();
  std::vector<uint64_t> h(sizeof(ffh_ctr_eval) / 8);
  check(api->ffh_memcpy_d2h(ctx, h.data(), d_eval, sizeof(ffh_ctr_eval), stream), "eval metrics d2h");
  check(api->ffh_stream_sync(ctx, stream), "sync");
  ffh_ctr_eval* e = reinterpret_cast<ffh_ctr_eval*>(h.data());
  double logloss = (double)e->logloss_sum;
  if (exchange && world_size > 1) {
    if (world_size > 8) die("get_eval_metrics(): the exact count exchange is sized for up to 8 ranks");
    float ll = e->logloss_sum;
    e->logloss_sum = 0.0f; e->pad_[0] = e->pad_[1] = e->pad_[2] = 0.0f;
    const size_t nw = h.size(), nf = nw * 4 + 1;
    float* d = (float*)dmalloc(nf * sizeof(float));
    std::vector<float> f(nf);
    for (size_t i = 0; i < nw; i++)
      for (int k = 0; k < 4; k++) f[i * 4 + k] = (float)((h[i] >> (16 * k)) & 0xffffULL);
    f[nf - 1] = ll;
    check(api->ffh_memcpy_h2d(ctx, d, f.data(), nf * sizeof(float), stream), "eval metrics h2d");
    if (config.comm.allreduce_sum_f32(config.comm.user, d, (int64_t)nf, stream) != 0) die("allreduce (evaluation metrics) failed");
    check(api->ffh_memcpy_d2h(ctx, f.data(), d, nf * sizeof(float), stream), "eval metrics d2h");
    check(api->ffh_stream_sync(ctx, stream), "sync");
    api->ffh_free(ctx, d);
    for (size_t i = 0; i < nw; i++) {
      uint64_t v = 0;
      for (int k = 0; k < 4; k++) v += (uint64_t)f[i * 4 + k] << (16 * k);
      h[i] = v;
    }
    logloss = (double)f[nf - 1];
  }
  EvalMetrics m;
  m.samples = e->samples; m.positives = e->positives; m.correct = e->correct; m.nan_predictions = e->nan_predictions;
  m.logloss_sum = logloss;
  m.auc = ffh_auc_from_histograms(e->hist_pos, e->hist_neg, FFH_AUC_BINS);
  if (with_histograms) {
    m.hist_pos.assign(e->hist_pos, e->hist_pos + FFH_AUC_BINS);
    m.hist_neg.assign(e->hist_neg, e->hist_neg + FFH_AUC_BINS);
  }
  return m;
}

// =============================================================================================
// learning-rate schedule (include/ff_hip_lr.h)
// =============================================================================================
void FFModel::lr_choose_route() {
  const int64_t W = config.lr_warmup_steps, S = config.lr_decay_start_step, N = config.lr_num_decay_steps;
  if (W < 0) die("--lr-num-warmup-steps %lld: must be >= 0", (long long)W);
  if (S < 0) die("--lr-decay-start-step %lld: must be >= 0", (long long)S);
  if (N < 0) die("--lr-num-decay-steps %lld: must be >= 0", (long long)N);
  if (N > 0 && S < W)
    die("--lr-decay-start-step %lld lies inside the warm-up of %lld steps: raise --lr-decay-start-step to at least --lr-num-warmup-steps (or lower that)",
        (long long)S, (long long)W);
  if (config.device_lr && config.host_lr_schedule) die("--device-lr and --host-lr-schedule exclude each other: drop one");
  const bool scheduled = W > 0 || N > 0;
  SGDOptimizer* sgd = dynamic_cast<SGDOptimizer*>(optimizer);
  AdamOptimizer* adam = dynamic_cast<AdamOptimizer*>(optimizer);
  AdagradOptimizer* adagrad = dynamic_cast<AdagradOptimizer*>(optimizer);
  lr_base = sgd ? sgd->lr : (adam ? adam->alpha : (adagrad ? adagrad->lr : 0.0));
  lr_route = kLrOff;
  lr_route_why = "constant rate";
  if (config.device_lr && !api->lr)
    die("--device-lr: %s (%s) is a kernel library without the learning-rate extension (include/ff_hip_lr.h); drop --device-lr (a schedule then runs "
        "on the host route)", api->path.c_str(), api->ffh_backend_name());
  if (!scheduled && !config.device_lr) return;
  if (config.computationMode != COMP_MODE_TRAINING) return;
  // the device route needs an _lr form of every optimizer launch this model issues
  const char* no = nullptr;
  if (config.host_lr_schedule) no = "--host-lr-schedule";
  else if (!api->lr) no = "the kernel library has no learning-rate extension";
  else if (!sgd && !adam && !adagrad) no = "unknown optimizer";
  else if (!embeddings.empty() && !fused_embedding_update()) no = "the tables take the owner-local dense update";
  else if (config.profiling) no = "--profiling times the table update as the embedding group's backward";
  else {
    for (const Embedding* e : embeddings)
      if (e->row_sharded) no = "a table is row-sharded";
  }
  if (!no) { lr_route = kLrDevice; lr_route_why = config.device_lr ? "--device-lr" : "every optimizer launch has an _lr form"; return; }
  if (config.device_lr && !scheduled) {      // nothing to schedule: the scalar launches of before
    lr_route_why = std::string("constant rate; --device-lr not possible: ") + no;
    return;
  }
  lr_route = kLrHost;
  lr_route_why = no;
}

void FFModel::lr_allocate() {
  if (lr_route == kLrHost) { lr_host_steps = 0; lr_host_set(0); return; }
  if (lr_route != kLrDevice) return;
  AdamOptimizer* adam = dynamic_cast<AdamOptimizer*>(optimizer);
  ffh_lr_schedule sc;
  memset(&sc, 0, sizeof sc);
  sc.base = lr_base; sc.warmup_steps = config.lr_warmup_steps; sc.decay_start = config.lr_decay_start_step; sc.decay_steps = config.lr_num_decay_steps;
  if (adam) { sc.beta1 = adam->beta1; sc.beta2 = adam->beta2; }
  for (int i = 0; i < 2; i++) {
    lr_block[i] = (ffh_lr_state*)dmalloc(api->lr->ffh_lr_state_bytes());
    check(api->lr->ffh_lr_state_init(ctx, lr_block[i], &sc, 0, stream), "lr_state_init");
  }
}

void FFModel::lr_host_set(int64_t k) {
  const double v = ffh_lr_schedule_value(k, lr_base, config.lr_warmup_steps, config.lr_decay_start_step, config.lr_num_decay_steps);
  if (SGDOptimizer* sgd = dynamic_cast<SGDOptimizer*>(optimizer)) sgd->lr = v;
  else if (AdamOptimizer* adam = dynamic_cast<AdamOptimizer*>(optimizer)) adam->alpha = v;
  else if (AdagradOptimizer* adagrad = dynamic_cast<AdagradOptimizer*>(optimizer)) adagrad->lr = v;
}

void FFModel::advance_lr(int which, ffh_stream s, ffh_ctx* cx) const {
  if (lr_route == kLrDevice) check(api->lr->ffh_lr_state_advance(cx, lr_block[which], s), "lr_state_advance");
}

int64_t FFModel::lr_steps() {
  if (lr_route == kLrHost) return lr_host_steps;
  if (lr_route != kLrDevice) return 0;
  sync();
  ffh_lr_values v;
  check(api->lr->ffh_lr_state_read(ctx, lr_block[0], &v, stream), "lr_state_read");
  return v.k;
}

double FFModel::current_lr() {
  if (lr_route == kLrDevice) {
    sync();
    ffh_lr_values v;
    check(api->lr->ffh_lr_state_read(ctx, lr_block[0], &v, stream), "lr_state_read");
    return (double)v.lr;
  }
  const int64_t k = lr_route == kLrHost ? lr_host_steps : 0;
  if (lr_route == kLrOff) {
    if (SGDOptimizer* sgd = dynamic_cast<SGDOptimizer*>(optimizer)) return (double)(float)sgd->lr;
    if (AdamOptimizer* adam = dynamic_cast<AdamOptimizer*>(optimizer)) return (double)(float)adam->alpha;
    if (AdagradOptimizer* adagrad = dynamic_cast<AdagradOptimizer*>(optimizer)) return (double)(float)adagrad->lr;
    return 0.0;
  }
  return (double)(float)ffh_lr_schedule_value(k, lr_base, config.lr_warmup_steps, config.lr_decay_start_step, config.lr_num_decay_steps);
}

std::string FFModel::lr_schedule_line() const {
  char buf[512];
  snprintf(buf, sizeof buf, "warmup W=%lld, decay start S=%lld, decay steps N=%lld, base %g, route=%s (%s)", (long long)config.lr_warmup_steps,
           (long long)config.lr_decay_start_step, (long long)config.lr_num_decay_steps, lr_base,
           lr_route == kLrDevice ? "device" : (lr_route == kLrHost ? "host" : "off"), lr_route_why.c_str());
  return buf;
}
