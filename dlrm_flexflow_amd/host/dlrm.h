// dlrm.h -- the examples/cpp/DLRM driver re-stated on the FFModel shim: same flags, same model
// topology, same warm-up + timed-epoch protocol, same "ELAPSED TIME ... THROUGHPUT" line.
// [ref: examples/cpp/DLRM/dlrm.h:24-89, examples/cpp/DLRM/dlrm.cc]
#pragma once

#include <string>
#include <vector>

#include "ffmodel.h"
#include "../../include/ff_hip_data.h"

#define MAX_NUM_EMB 1000

struct DLRMConfig {
  DLRMConfig(void);   // defaults of [ref: examples/cpp/DLRM/dlrm.h:25-36]
  int sparse_feature_size, sigmoid_bot, sigmoid_top, embedding_bag_size;
  std::vector<int> embedding_bag_sizes;   // --embedding-bag-sizes a-b-c-...: one bag size per table (not a reference flag; empty: embedding_bag_size for all)
  bool bag_size_given;                    // --embedding-bag-size was on the command line (refused beside --embedding-bag-sizes)
  int bag_of(size_t table) const { return embedding_bag_sizes.empty() ? embedding_bag_size : embedding_bag_sizes[table]; }
  float loss_threshold;
  std::vector<int> embedding_size, mlp_bot, mlp_top;
  std::string arch_interaction_op, dataset_path;
  int data_size;
  std::string optimizer;   // --optimizer sgd (default, the reference driver's) | sgd-momentum | adam | adagrad (not a reference flag)
  double synthetic_bag_fill = 1.0;   // --synthetic-bag-fill F, 0 < F <= 1 (with --embedding-padding): a synthetic slot holds a lookup with probability F (not a reference flag)
  bool bag_fill_given = false;
  bool mean_pooling = false;         // --embedding-pooling sum|mean: every table pools with AGGR_MODE_AVG instead of AGGR_MODE_SUM (not a reference flag)
  bool pooling_given = false;
  double zipf_alpha;   // > 0: synthetic ids follow a power law instead of the reference's uniform draw (not a reference flag)
  int dcn_num_layers, dcn_low_rank_dim;   // --arch-interaction-op dcn: --dcn-num-layers L (3), --dcn-low-rank-dim R (512) (not reference flags)
};

void parse_input_args(char** argv, int argc, DLRMConfig& config);

Tensor create_mlp(FFModel* model, const Tensor& input, std::vector<int> ln, int sigmoid_layer);
Tensor create_emb(FFModel* model, const Tensor& input, int input_dim, int output_dim, int idx, AggrMode aggr = AGGR_MODE_SUM);
Tensor interact_features(FFModel* model, const Tensor& x, const std::vector<Tensor>& ly, std::string interaction, int dcn_num_layers = 3,
                         int dcn_low_rank_dim = 512);

// Dataset (synthetic, or the reference's HDF5 Criteo file with --dataset) resident on the device (the reference keeps it in zero-copy host memory and
// gathers + copies H2D every batch, [ref: examples/cpp/DLRM/dlrm.cc:357-377, dlrm.cu:19-122]).
// Distributions of [ref: examples/cpp/DLRM/dlrm.cc:413-420] from the seeded counter RNG, with a
// per-table row count (the reference asserts all tables equal, :349-354 -- lifted).
class DataLoader {
 public:
  DataLoader(FFModel& ff, const DLRMConfig& dlrm, const std::vector<Tensor>& sparse_inputs, Tensor dense_input, Tensor label);
  ~DataLoader();
  // the next TRAINING batch (wraps at num_train).  --data-randomize total: batch next_index / B of epoch `epoch`'s order, one gather launch
  // (include/ff_hip_data.h); a wrap without reset() moves on to the next epoch's order
  void next_batch(FFModel& ff);
  void load_batch(FFModel& ff, int k);          // batch k of what was loaded into the model inputs, in file order; the training cursor does not move
  void shuffle() {}
  void reset(int64_t epoch_ = 0) { next_index = 0; epoch = epoch_; }
  int num_samples, next_index;
  int64_t epoch;                                // which order next_batch follows (--data-randomize total)
  int num_train;                                // num_samples minus the held-out tail (--eval-batches)

 private:
  void generate_random(FFModel& ff, const DLRMConfig& dlrm);
  void generate_zipf(FFModel& ff, int64_t* dst, int64_t n, uint64_t seed, int64_t rows, double alpha);
  void load_hdf5(FFModel& ff, const DLRMConfig& dlrm);      // --dataset: X_int / X_cat / y of the reference's Criteo file
  void gather_batch(FFModel& ff, int64_t step);             // --data-randomize total: batch `step` of epoch `epoch`'s order
  std::vector<ffh_gather_segment> segments;                 // ... its segments: one per table (null destination: not held by this rank), the dense features, the labels
  std::vector<Tensor> batch_sparse_inputs;
  Tensor batch_dense_input, batch_label;
  std::vector<int64_t*> full_sparse;   // per owned table: [num_samples][bags[t]]
  float *full_dense, *full_label;      // this rank's samples of every batch: [num_samples/world][...]
  std::vector<int> bags;               // bag size per table
  int dense_dim;
  FFModel* model;
};

// The whole application: what top_level_task builds [ref: examples/cpp/DLRM/dlrm.cc:77-195].
struct DLRMApp {
  FFConfig ffconfig;
  DLRMConfig dlrm;
  FFModel* ff;
  DataLoader* loader;
  Optimizer* optimizer = nullptr;
  std::vector<Tensor> sparse_inputs;
  Tensor dense_input;
  bool warmed_up;
  int start_epoch = 0;           // --load-checkpoint: the epochs the checkpoint had completed; run_epochs() goes on from there
  double save_checkpoint(int epochs_done);   // --save-checkpoint: every rank writes its file; returns the wall time in seconds (outside the timed region)
  DLRMApp(int argc, char** argv, const ffcomm* comm);
  ~DLRMApp();
  void warmup();                 // the reference's single warm-up iteration
  void train_steps(int n, bool trace);   // n x {forward, zero_gradients, backward, update}
  double run_epochs();           // the timed loop; returns elapsed seconds and prints the THROUGHPUT line
  // --eval-batches: the held-out tail through FFModel::eval_batch(), one "EVAL epoch E: ..." line on rank 0; returns its wall time in seconds.
  // The model inputs hold the training batch of the warm-up again afterwards (synthetic input is not reloaded per step).
  double evaluate(int epoch, EvalMetrics* out = nullptr);
};

int dlrm_main(int argc, char** argv, const ffcomm* comm);
