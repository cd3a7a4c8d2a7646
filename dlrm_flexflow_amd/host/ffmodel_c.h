/* ffmodel_c.h -- extern "C" face of the FFModel shim, in the style of the reference's
 * python/flexflow_c.h (opaque {void* impl} handles, [ref: python/flexflow_c.h:24-42,108-138,
 * 196-248,498-546]).  Python (bench.py, run_dlrm.py, tests) binds it with ctypes.
 * Errors abort the process with a message, as the reference's asserts do. */
#ifndef FFMODEL_C_H_
#define FFMODEL_C_H_
#include <stdbool.h>
#include <stdint.h>
#include "ffcomm.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FF_NEW_OPAQUE_TYPE(T) typedef struct T { void* impl; } T
FF_NEW_OPAQUE_TYPE(flexflow_config_t);
FF_NEW_OPAQUE_TYPE(flexflow_model_t);
FF_NEW_OPAQUE_TYPE(flexflow_tensor_t);
FF_NEW_OPAQUE_TYPE(flexflow_initializer_t);
FF_NEW_OPAQUE_TYPE(flexflow_sgd_optimizer_t);
FF_NEW_OPAQUE_TYPE(flexflow_adam_optimizer_t);
FF_NEW_OPAQUE_TYPE(flexflow_adagrad_optimizer_t);
FF_NEW_OPAQUE_TYPE(flexflow_dlrm_t);
#undef FF_NEW_OPAQUE_TYPE

typedef struct flexflow_perf_metrics_t {
  int train_all, train_correct;
  float cce_loss, sparse_cce_loss, mse_loss, rmse_loss, mae_loss;
} flexflow_perf_metrics_t;

/* Binary cross-entropy and held-out evaluation (include/ff_hip_ctr.h; this build's own, the reference has neither).
 * Constants for flexflow_model_compile: loss 150 (LOSS_BINARY_CROSSENTROPY, mean over the global batch; the final layer must be a dense
 * layer with sigmoid activation and one output column), metrics 2001 (METRICS_BINARY_CROSSENTROPY) and 2002 (METRICS_AUC). */
#define FLEXFLOW_LOSS_BINARY_CROSSENTROPY 150
#define FLEXFLOW_METRICS_BINARY_CROSSENTROPY 2001
#define FLEXFLOW_METRICS_AUC 2002
typedef struct flexflow_eval_metrics_t {
  uint64_t samples, positives, correct, nan_predictions;   /* global counts; NaN predictions are left out of everything else */
  double logloss_sum, auc;                                  /* auc: NaN without a positive or without a negative sample */
} flexflow_eval_metrics_t;

/* FFConfig */
flexflow_config_t flexflow_config_create(void);
void flexflow_config_destroy(flexflow_config_t);
void flexflow_config_parse_args(flexflow_config_t, char** argv, int argc);
void flexflow_config_set_comm(flexflow_config_t, const ffcomm* comm);
void flexflow_config_set_batch_size(flexflow_config_t, int);
int  flexflow_config_get_batch_size(flexflow_config_t);
void flexflow_config_set_backend(flexflow_config_t, const char* lib_path);
void flexflow_config_set_seed(flexflow_config_t, uint64_t);
void flexflow_config_set_device(flexflow_config_t, int);
void flexflow_config_set_enable_graph(flexflow_config_t, bool);
void flexflow_config_set_overlap_embedding(flexflow_config_t, bool);
void flexflow_config_set_dense_embedding_update(flexflow_config_t, bool);
/* --ragged-update / --no-ragged-update: tables of differing bag sizes are updated in one ragged call per group (include/ff_hip_bags_update.h) */
void flexflow_config_set_ragged_update(flexflow_config_t, bool);
/* --embedding-padding: the id -1 in a sparse input is "no lookup" (variable-length bags; include/ff_hip_pad.h) */
void flexflow_config_set_embedding_padding(flexflow_config_t, bool);
/* bf16 embedding tables (--embedding-dtype / --embedding-rounding): data_type 40 (DT_FLOAT, default) or 140 (DT_BF16);
 * mode 0 stochastic (default) or 1 nearest even (include/ffh_bf16.h).  Other values abort. */
void flexflow_config_set_embedding_dtype(flexflow_config_t, int data_type);
void flexflow_config_set_embedding_rounding(flexflow_config_t, int mode);
/* --eval-embedding-dtype: 0 fp32 (default), 1 int8: eval_batch() gathers from 8-bit row images of the tables (include/ff_hip_q8.h).  Other values abort. */
void flexflow_config_set_eval_embedding_dtype(flexflow_config_t, int int8);
/* learning-rate schedule (include/ff_hip_lr.h): warm-up steps W, decay start step S, decay steps N (all 0: the constant rate); device_lr: 1 = the rate lives
 * in device memory (--device-lr), -1 = force the host route (--host-lr-schedule), 0 = compile() chooses.  compile() refuses bad values, naming the flag. */
void flexflow_config_set_lr_schedule(flexflow_config_t, int64_t warmup_steps, int64_t decay_start_step, int64_t num_decay_steps, int device_lr);
/* the schedule itself, a pure function: the rate of zero-based step k as the float the kernels receive */
double flexflow_lr_schedule_value(int64_t k, double base, int64_t W, int64_t S, int64_t N);
/* --data-randomize total: ffh_perm_index of include/ffh_perm.h (position i of epoch `epoch` -> row of a stripe of n rows; i < n), and the
 * same for positions first .. first + count - 1 into out[count] */
uint64_t flexflow_shuffle_index(uint64_t seed, uint64_t epoch, uint64_t i, uint64_t n);
void flexflow_shuffle_indices(uint64_t seed, uint64_t epoch, uint64_t first, uint64_t count, uint64_t n, uint64_t* out);

/* FFModel */
flexflow_model_t flexflow_model_create(flexflow_config_t);
void flexflow_model_destroy(flexflow_model_t);
flexflow_tensor_t flexflow_tensor_create(flexflow_model_t, int num_dims, const int* dims, int data_type, bool create_grad);
flexflow_tensor_t flexflow_model_add_dense(flexflow_model_t, flexflow_tensor_t input, int out_dim, int activation, bool use_bias,
                                           flexflow_initializer_t kernel_init, flexflow_initializer_t bias_init, const char* name);
flexflow_tensor_t flexflow_model_add_embedding(flexflow_model_t, flexflow_tensor_t input, int num_entries, int out_dim, int aggr,
                                               flexflow_initializer_t kernel_init, const char* name);
flexflow_tensor_t flexflow_model_add_concat(flexflow_model_t, int n, const flexflow_tensor_t* inputs, int axis, const char* name);
flexflow_tensor_t flexflow_model_add_flat(flexflow_model_t, flexflow_tensor_t input, const char* name);
flexflow_tensor_t flexflow_model_add_dot_interaction(flexflow_model_t, flexflow_tensor_t input, int d, const char* name);   /* [batch][c*d] -> [batch][d + c(c-1)/2] */
flexflow_tensor_t flexflow_model_add_cross_combine(flexflow_model_t, flexflow_tensor_t x0, flexflow_tensor_t v, flexflow_tensor_t xl, const char* name);   /* x0 (.) v + xl, all [batch][D] (include/ff_hip_cross.h) */
flexflow_tensor_t flexflow_model_add_cross_net(flexflow_model_t, flexflow_tensor_t x0, int num_layers, int low_rank, const char* name);   /* DCNv2 low-rank cross network: 3 ops per layer */
flexflow_tensor_t flexflow_model_add_tril(flexflow_model_t, flexflow_tensor_t input, const char* name);   /* strict lower triangle of [batch][n][n] */
flexflow_tensor_t flexflow_model_add_transpose(flexflow_model_t, flexflow_tensor_t input, int n, const int* perm, const char* name);
flexflow_tensor_t flexflow_model_add_reshape(flexflow_model_t, flexflow_tensor_t input, int n, const int* shape, const char* name);
flexflow_tensor_t flexflow_model_add_batch_matmul(flexflow_model_t, flexflow_tensor_t a, flexflow_tensor_t b, int a_seq_length_dim, int b_seq_length_dim);
flexflow_initializer_t flexflow_zero_initializer_create(void);
flexflow_initializer_t flexflow_uniform_initializer_create(int seed, float min, float max);
flexflow_initializer_t flexflow_norm_initializer_create(int seed, float mean, float stddev);
flexflow_initializer_t flexflow_glorot_uniform_initializer_create(int seed);
flexflow_sgd_optimizer_t flexflow_sgd_optimizer_create(flexflow_model_t, double lr, double momentum, bool nesterov, double weight_decay);
void flexflow_model_set_sgd_optimizer(flexflow_model_t, flexflow_sgd_optimizer_t);
/* [ref: python/flexflow_c.h:398-400,572-588] */
flexflow_adam_optimizer_t flexflow_adam_optimizer_create(flexflow_model_t, double alpha, double beta1, double beta2, double weight_decay, double epsilon);
void flexflow_adam_optimizer_set_lr(flexflow_adam_optimizer_t, double lr);
void flexflow_model_set_adam_optimizer(flexflow_model_t, flexflow_adam_optimizer_t);
/* Adagrad, torch.optim.Adagrad's element-wise rule (include/ff_hip_adagrad.h; no reference class).  epsilon / initial_accumulator given as NaN: the
   config's --adagrad-eps / --adagrad-initial-accumulator */
/* FFModel::weight_mirror_stale_bytes: bytes of the weight slab's bf16 twin / three-plane image that a fresh conversion changes (0: current; -1: none kept) */
int64_t flexflow_model_weight_mirror_stale_bytes(flexflow_model_t);
void flexflow_config_set_adagrad(flexflow_config_t, double epsilon, double initial_accumulator);
flexflow_adagrad_optimizer_t flexflow_adagrad_optimizer_create(flexflow_model_t, double lr, double weight_decay, double epsilon, double initial_accumulator);
void flexflow_model_set_adagrad_optimizer(flexflow_model_t, flexflow_adagrad_optimizer_t);
/* row-wise Adagrad on the tables (include/ff_hip_rowwise.h): --adagrad-rowwise for the optimizers created afterwards / for this optimizer (before compile) */
void flexflow_config_set_adagrad_rowwise(flexflow_config_t, int on);
void flexflow_adagrad_optimizer_set_rowwise(flexflow_adagrad_optimizer_t, int on);
void flexflow_model_compile(flexflow_model_t, int loss_type, const int* metrics, int nb_metrics, int comp_mode);
void flexflow_model_init_layers(flexflow_model_t);
void flexflow_model_reset_metrics(flexflow_model_t);
void flexflow_model_forward(flexflow_model_t, int seq_length);
void flexflow_model_zero_gradients(flexflow_model_t);
void flexflow_model_backward(flexflow_model_t, int seq_length);
void flexflow_model_update(flexflow_model_t);
void flexflow_model_begin_trace(flexflow_model_t, int trace_id);
void flexflow_model_end_trace(flexflow_model_t, int trace_id);
void flexflow_model_sync(flexflow_model_t);
void flexflow_model_get_perf_metrics(flexflow_model_t, flexflow_perf_metrics_t* out);
float flexflow_perf_metrics_get_bce_loss(flexflow_model_t);   /* log-loss sum of the training batches since reset_metrics (synchronises) */
void flexflow_model_eval_batch(flexflow_model_t);             /* forward pass on the current inputs + evaluation metrics; no gradient, no update */
void flexflow_model_reset_eval_metrics(flexflow_model_t);
/* hist_pos / hist_neg: NULL, or flexflow_auc_bins() counters each (the raw histograms of the predictions, labels >= 0.5 / the rest) */
void flexflow_model_get_eval_metrics(flexflow_model_t, flexflow_eval_metrics_t* out, uint64_t* hist_pos, uint64_t* hist_neg);
int  flexflow_auc_bins(void);
double flexflow_auc_from_histograms(const uint64_t* hist_pos, const uint64_t* hist_neg, int bins);   /* ffh_auc_from_histograms */
flexflow_tensor_t flexflow_model_get_label_tensor(flexflow_model_t);
int  flexflow_model_get_num_layers(flexflow_model_t);
const char* flexflow_model_get_layer_name(flexflow_model_t, int layer);
int  flexflow_model_get_layer_num_weights(flexflow_model_t, int layer);
flexflow_tensor_t flexflow_model_get_parameter(flexflow_model_t, int layer, int index);   /* 0 kernel, 1 bias */
flexflow_tensor_t flexflow_model_get_layer_output(flexflow_model_t, int layer);
void* flexflow_model_get_stream(flexflow_model_t);
int  flexflow_model_uses_graph(flexflow_model_t);
double flexflow_model_get_current_lr(flexflow_model_t);   /* the scheduled rate of the next optimizer step (synchronises on the device route); counters "lr_steps", "lr_route", "graph_replays" */
const char* flexflow_model_get_backend_name(flexflow_model_t);   /* ffh_backend_name() of the kernel library the model loaded: "hip-gfx950" | "oracle-cpu" */
const char* flexflow_model_get_backend_path(flexflow_model_t);   /* ... and the file it was loaded from */
void flexflow_model_set_trace_mode(flexflow_model_t, int mode);   /* 0: replay a trace only where that is not slower than launching it (decided on its first calls); 1: always replay */
int  flexflow_model_trace_replays(flexflow_model_t, int trace_id);   /* 0 once the adaptive mode has settled on eager launches for this trace */
int64_t flexflow_model_get_counter(flexflow_model_t, const char* name);   /* diagnostics for tests: "mlp_chain_fwd_calls", "mlp_chain_bwd_calls", "fused_loss_calls",
                                                                            "bf16_updates" (the bf16 tables' update counter, synchronises); -1: unknown */

/* Checkpoint save / exact resume (host/checkpoint.cc).  Both return 0, or print "FATAL: ..." and abort like compile(); both synchronise
 * and are called between steps.  save writes dir/rank-R-of-N.ffck; load writes the epochs the file had completed into *epochs_done (may be NULL). */
int flexflow_model_save_checkpoint(flexflow_model_t, const char* dir, int64_t epochs_done);
int flexflow_model_load_checkpoint(flexflow_model_t, const char* dir, int64_t* epochs_done);
/* the fold (wrapping sum) of every checkpoint record's digest (include/ff_hip_digest.h): equal for two models iff a checkpoint of one would equal a
 * checkpoint of the other record by record (up to a 2^-64 collision); on the device where the kernel library has the extension; synchronises */
uint64_t flexflow_model_state_digest(flexflow_model_t);
/* ffh_state_digest_host of include/ff_hip_digest.h on host memory: the definition as the host layer compiles it */
uint64_t flexflow_state_digest_host(const void* base, int64_t rows, int64_t row_bytes, int64_t ld_bytes, uint64_t seed, uint64_t index_base);
uint64_t flexflow_digest_record_seed(uint64_t ordinal);   /* ffh_digest_record_seed: the digest seed of a checkpoint's record */

/* Tensor / Parameter host<->device [ref: flexflow_parameter_set_weights_float, python/flexflow_c.h:498-546] */
int  flexflow_tensor_get_num_dims(flexflow_tensor_t);
void flexflow_tensor_get_dims(flexflow_tensor_t, int* dims);            /* natural order: dims[0] = batch */
int64_t flexflow_tensor_get_local_rows(flexflow_tensor_t);
bool flexflow_tensor_is_local(flexflow_tensor_t);                       /* false: table owned by another rank */
void* flexflow_tensor_get_device_ptr(flexflow_tensor_t);                /* address of element (0, 0) in the backend's memory (tests / tools: on-device
                                                                           comparisons of tables too large to copy out); NULL when not local.
                                                                           A bf16 table (data type 140): it points at bf16 bit patterns */
int  flexflow_tensor_get_data_type(flexflow_tensor_t);                  /* 40 DT_FLOAT, 43 DT_INT64, 140 DT_BF16 (a bf16 embedding table), ... */
int64_t flexflow_tensor_get_ld(flexflow_tensor_t);                      /* elements between consecutive rows */
void flexflow_tensor_set_float(flexflow_tensor_t, flexflow_model_t, const int* dims, int num_dims, const float* data);
void flexflow_tensor_set_int64(flexflow_tensor_t, flexflow_model_t, const int* dims, int num_dims, const int64_t* data);
void flexflow_tensor_get_float(flexflow_tensor_t, flexflow_model_t, float* data);
void flexflow_tensor_get_int64(flexflow_tensor_t, flexflow_model_t, int64_t* data);
void flexflow_tensor_get_grad_float(flexflow_tensor_t, flexflow_model_t, float* data);
/* a bf16 table: _set_float rounds to nearest even, _get_float widens exactly; _set_bf16 / _get_bf16 copy the uint16 bit patterns */
void flexflow_tensor_set_bf16(flexflow_tensor_t, flexflow_model_t, const int* dims, int num_dims, const uint16_t* data);
void flexflow_tensor_get_bf16(flexflow_tensor_t, flexflow_model_t, uint16_t* data);

/* DLRM application (examples/cpp/DLRM) */
flexflow_dlrm_t flexflow_dlrm_create(int argc, char** argv, const ffcomm* comm);
void flexflow_dlrm_destroy(flexflow_dlrm_t);
flexflow_model_t flexflow_dlrm_get_model(flexflow_dlrm_t);
int  flexflow_dlrm_get_num_samples(flexflow_dlrm_t);
int  flexflow_dlrm_get_num_tables(flexflow_dlrm_t);
int  flexflow_dlrm_get_bag_size(flexflow_dlrm_t, int table);      /* ids per sample of table `table` (--embedding-bag-size, or its entry of --embedding-bag-sizes) */
const char* flexflow_dlrm_get_embedding_pooling(flexflow_dlrm_t);   /* --embedding-pooling: "sum" (the default) or "mean" (every table pools with AGGR_MODE_AVG) */
double flexflow_dlrm_get_bag_fill(flexflow_dlrm_t);             /* --synthetic-bag-fill: the share of a synthetic bag's slots that hold a lookup (with --embedding-padding; 1: all) */
int  flexflow_dlrm_get_start_epoch(flexflow_dlrm_t);   /* --load-checkpoint: the epochs the checkpoint had completed (0 without it) */
flexflow_tensor_t flexflow_dlrm_get_sparse_input(flexflow_dlrm_t, int table);
flexflow_tensor_t flexflow_dlrm_get_dense_input(flexflow_dlrm_t);
void flexflow_dlrm_warmup(flexflow_dlrm_t);
void flexflow_dlrm_train_steps(flexflow_dlrm_t, int steps, bool trace);
double flexflow_dlrm_run_epochs(flexflow_dlrm_t);
/* --eval-batches: evaluates the held-out batches as the driver does after an epoch (prints its EVAL line on rank 0); returns the wall time */
double flexflow_dlrm_evaluate(flexflow_dlrm_t, int epoch, flexflow_eval_metrics_t* out);
/* average device time (ms) of `iters` back-to-back launches, HIP events on the launch stream:
 * which = 0 embedding gather (all owned tables, one launch), 1 fused embedding backward + SGD,
 *         2 whole training step (forward, zero_gradients, backward, update; traced if enabled),
 *         12 the batch load alone (DataLoader::next_batch: the copies of file order, or the one gather launch of --data-randomize total) */
void flexflow_dlrm_probe_step(flexflow_dlrm_t, int iters, float* out_ms, int nout);   /* in-step event intervals, see ffmodel_c.cc; collective at world_size > 1 */
float flexflow_dlrm_time_kernel(flexflow_dlrm_t, int which, int iters);

#ifdef __cplusplus
}
#endif
#endif
