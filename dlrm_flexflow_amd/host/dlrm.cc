// dlrm.cc -- DLRM application on the FFModel shim [ref: examples/cpp/DLRM/dlrm.cc].
#include "dlrm.h"

#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
#include "hdf5_io.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>

#include "backend.h"
#include "../../include/ffh_rng.h"
#include "../../include/ffh_bf16.h"

namespace {
double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
void print_vector(const std::string& name, const std::vector<int>& v) {
  std::ostringstream out;
  for (size_t i = 0; i < v.size(); i++) out << v[i] << (i + 1 < v.size() ? " " : "");
  printf("[DLRM] %s: %s\n", name.c_str(), out.str().c_str());
}
}  // namespace

DLRMConfig::DLRMConfig(void)
    : sparse_feature_size(2), sigmoid_bot(-1), sigmoid_top(-1), embedding_bag_size(1), bag_size_given(false), loss_threshold(0.0f),
      arch_interaction_op("cat"), dataset_path(""), data_size(-1), optimizer("sgd"), zipf_alpha(0.0), dcn_num_layers(3), dcn_low_rank_dim(512) {
  embedding_size.push_back(4);
  mlp_bot.push_back(4); mlp_bot.push_back(2);
  mlp_top.push_back(8); mlp_top.push_back(2);
}

// [ref: examples/cpp/DLRM/dlrm.cc:197-260] -- identical flags
void parse_input_args(char** argv, int argc, DLRMConfig& config) {
  auto split = [](const char* s) {
    std::vector<int> v;
    std::stringstream ss((std::string(s)));
    std::string word;
    while (std::getline(ss, word, '-')) v.push_back(std::stoi(word));
    return v;
  };
  for (int i = 1; i < argc; i++) {
    // the DCNv2 flags (not reference flags) take "--flag value" and "--flag=value", as FFConfig::parse_args does
    {
      const char* eq = strncmp(argv[i], "--", 2) == 0 ? strchr(argv[i], '=') : nullptr;
      auto is = [&](const char* a) { return eq ? (strlen(a) == (size_t)(eq - argv[i]) && !strncmp(argv[i], a, (size_t)(eq - argv[i]))) : !strcmp(argv[i], a); };
      auto next = [&]() -> const char* {
        if (eq) return eq + 1;
        if (i + 1 >= argc) { fprintf(stderr, "FATAL: flag %s needs a value\n", argv[i]); abort(); }
        return argv[++i];
      };
      if (eq && is("--arch-interaction-op")) { config.arch_interaction_op = std::string(next()); continue; }
      if (eq && is("--optimizer")) { config.optimizer = std::string(next()); continue; }
      if (is("--embedding-bag-sizes")) { config.embedding_bag_sizes = split(next()); continue; }      // one per table, the format of --arch-embedding-size
      if (is("--synthetic-bag-fill")) {      // with --embedding-padding: the share of a synthetic bag's slots that hold a lookup, the rest are the pad id
        config.synthetic_bag_fill = atof(next());
        if (!(config.synthetic_bag_fill > 0.0 && config.synthetic_bag_fill <= 1.0)) {
          fprintf(stderr, "FATAL: --synthetic-bag-fill %g: must be in (0, 1]\n", config.synthetic_bag_fill);
          abort();
        }
        config.bag_fill_given = true;
        continue;
      }
      if (is("--embedding-pooling")) {      // how a bag's rows become one: the sum (the default, the reference's), or the mean
        const std::string v(next());
        if (v != "sum" && v != "mean") {
          fprintf(stderr, "FATAL: --embedding-pooling %s: 'sum' or 'mean'\n", v.c_str());
          abort();
        }
        config.mean_pooling = v == "mean";
        config.pooling_given = true;
        continue;
      }
      if (is("--dcn-num-layers")) { config.dcn_num_layers = atoi(next()); continue; }
      if (is("--dcn-low-rank-dim")) { config.dcn_low_rank_dim = atoi(next()); continue; }
    }
    if (!strcmp(argv[i], "--arch-sparse-feature-size")) { config.sparse_feature_size = atoi(argv[++i]); continue; }
    if (!strcmp(argv[i], "--arch-embedding-size")) { config.embedding_size = split(argv[++i]); continue; }
    if (!strcmp(argv[i], "--embedding-bag-size")) { config.embedding_bag_size = atoi(argv[++i]); config.bag_size_given = true; continue; }
    if (!strcmp(argv[i], "--arch-mlp-bot")) { config.mlp_bot = split(argv[++i]); continue; }
    if (!strcmp(argv[i], "--arch-mlp-top")) { config.mlp_top = split(argv[++i]); continue; }
    if (!strcmp(argv[i], "--loss-threshold")) { config.loss_threshold = (float)atof(argv[++i]); continue; }
    if (!strcmp(argv[i], "--sigmoid-top")) { config.sigmoid_top = atoi(argv[++i]); continue; }
    if (!strcmp(argv[i], "--sigmoid-bot")) { config.sigmoid_bot = atoi(argv[++i]); continue; }
    if (!strcmp(argv[i], "--arch-interaction-op")) { config.arch_interaction_op = std::string(argv[++i]); continue; }
    if (!strcmp(argv[i], "--optimizer") && i + 1 < argc) { config.optimizer = std::string(argv[++i]); continue; }
    if (!strcmp(argv[i], "--dataset")) { config.dataset_path = std::string(argv[++i]); continue; }
    if (!strcmp(argv[i], "--data-size")) { config.data_size = atoi(argv[++i]); continue; }
    if (!strcmp(argv[i], "--zipf-alpha")) { config.zipf_alpha = atof(argv[++i]); continue; }   // not a reference flag
  }
}

// [ref: examples/cpp/DLRM/dlrm.cc:26-39]: N(0, sqrt(2/(in+out))) weights, N(0, sqrt(2/out)) bias,
// ReLU everywhere except `sigmoid_layer`
Tensor create_mlp(FFModel* model, const Tensor& input, std::vector<int> ln, int sigmoid_layer) {
  Tensor t = input;
  for (int i = 0; i < (int)(ln.size() - 1); i++) {
    float std_dev = std::sqrt(2.0f / (ln[i + 1] + ln[i]));
    Initializer* weight_init = model->own(new NormInitializer(model->next_seed(), 0, std_dev));
    std_dev = std::sqrt(2.0f / ln[i + 1]);
    Initializer* bias_init = model->own(new NormInitializer(model->next_seed(), 0, std_dev));
    ActiMode activation = i == sigmoid_layer ? AC_MODE_SIGMOID : AC_MODE_RELU;
    t = model->dense(t, ln[i + 1], activation, true /*bias*/, NULL /*weight_sharing*/, weight_init, bias_init);
  }
  return t;
}

// [ref: examples/cpp/DLRM/dlrm.cc:41-47]: U(-sqrt(1/R), sqrt(1/R)), AGGR_MODE_SUM (`aggr`: --embedding-pooling mean gives AGGR_MODE_AVG)
Tensor create_emb(FFModel* model, const Tensor& input, int input_dim, int output_dim, int idx, AggrMode aggr) {
  (void)idx;
  float range = std::sqrt(1.0f / input_dim);
  Initializer* embed_init = model->own(new UniformInitializer(model->next_seed(), -range, range));
  return model->embedding(input, input_dim, output_dim, aggr, NULL /*weight_sharing*/, embed_init);
}

// [ref: examples/cpp/DLRM/dlrm.cc:49-65]: the reference implements "cat" and asserts on "dot" (a TODO).
// "dot" here is the composition the reference's own op tests spell out for the pairwise interaction
// [ref: tests/ops/test_harness.py:125-177]: cat -> reshape [B][C][D] -> transpose -> batch_matmul -> flat,
// concatenated with the bottom-MLP output: [x | vec(Z Z^T)], width D + C*C with C = 1 + #tables.
// "dot-tril" is MLPerf-DLRM's variant: only the strict lower triangle of Z Z^T is kept (C (C - 1) / 2 products: 351 of 729
// for 26 tables; width D + C (C - 1) / 2 = 479) -- through FFModel::dot_interaction, the whole interaction as one
// MFMA kernel each way (csrc/interaction.hip); "dot-tril-ops" spells the same thing as the operator chain with
// FFModel::tril (neither operator exists in the reference).
// "dcn" is MLPerf DLRM-DCNv2's interaction: torchrec's LowRankCrossNet on the concat (FFModel::cross_net).
Tensor interact_features(FFModel* model, const Tensor& x, const std::vector<Tensor>& ly, std::string interaction, int dcn_num_layers, int dcn_low_rank_dim) {
  std::vector<Tensor> inputs;
  inputs.push_back(x);
  for (size_t i = 0; i < ly.size(); i++) inputs.push_back(ly[i]);
  if (interaction == "cat") return model->concat((int)inputs.size(), inputs.data(), 1 /*axis*/);
  if (interaction == "dcn") return model->cross_net(model->concat((int)inputs.size(), inputs.data(), 1 /*axis*/), dcn_num_layers, dcn_low_rank_dim);
  if (interaction == "dot" || interaction == "dot-tril" || interaction == "dot-tril-ops") {
    const int batch = x.adim[1], d = x.adim[0], c = (int)inputs.size();
    for (const Tensor& t : inputs)
      if (t.adim[0] != d) {
        fprintf(stderr, "FATAL: --arch-interaction-op dot needs the bottom MLP output width (%d) to equal --arch-sparse-feature-size (%d)\n", d, t.adim[0]);
        abort();
      }
    Tensor cat = model->concat(c, inputs.data(), 1 /*axis*/);
    if (interaction == "dot-tril") return model->dot_interaction(cat, d);   // the chain below (with tril) as one launch each way
    Tensor z = model->reshape(cat, {batch, c, d});
    Tensor zt = model->transpose(z, {0, 2, 1});
    Tensor p = model->batch_matmul(z, zt);            // [batch][c][c]
    Tensor pf = interaction == "dot" ? model->flat(p) : model->tril(p);   // "dot-tril-ops": the operator chain, kept for parity tests
    Tensor both[2] = {x, pf};
    return model->concat(2, both, 1 /*axis*/);
  }
  fprintf(stderr, "FATAL: --arch-interaction-op %s: 'cat', 'dot', 'dot-tril' or 'dot-tril-ops', or 'dcn' (the DCNv2 low-rank cross network)\n", interaction.c_str());
  abort();
}

static void check_eval_batches(int eval_batches, int nb);

// =============================================================================================
DataLoader::DataLoader(FFModel& ff, const DLRMConfig& dlrm, const std::vector<Tensor>& sparse_inputs, Tensor dense_input, Tensor label)
    : num_samples(0), next_index(0), epoch(0), batch_sparse_inputs(sparse_inputs), batch_dense_input(dense_input), batch_label(label),
      full_dense(nullptr), full_label(nullptr), model(&ff) {
  num_train = 0;
  for (size_t t = 0; t < sparse_inputs.size(); t++) bags.push_back(dlrm.bag_of(t));
  dense_dim = dense_input.adim[0];
  full_sparse.assign(sparse_inputs.size(), nullptr);
  if (dlrm.dataset_path != "") load_hdf5(ff, dlrm);
  else generate_random(ff, dlrm);
  ff.check(ff.api->ffh_stream_sync(ff.ctx, ff.stream), "dataset sync");
  check_eval_batches(ff.config.eval_batches, num_samples / ff.config.batchSize);
  num_train = num_samples - ff.config.eval_batches * ff.config.batchSize;
  if (ff.config.data_randomize) {
    for (size_t t = 0; t < batch_sparse_inputs.size(); t++)
      segments.push_back({full_sparse[t], full_sparse[t] ? batch_sparse_inputs[t].impl->ptr : nullptr, 8 * bags[t], FFH_GATHER_GLOBAL_ROWS});
    segments.push_back({full_dense, batch_dense_input.impl->ptr, 4 * dense_dim, FFH_GATHER_LOCAL_ROWS});
    segments.push_back({full_label, batch_label.impl->ptr, 4, FFH_GATHER_LOCAL_ROWS});
  }
}

// samples of the synthetic data set [ref: dlrm.cc:272-276], whole batches
static int random_num_samples(const FFConfig& cfg, const DLRMConfig& dlrm, int world_size) {
  int n = dlrm.data_size > 0 ? dlrm.data_size : 256 * 4 * std::max(1, world_size) * cfg.numNodes;
  const int B = cfg.batchSize;
  if (n < B) n = B;
  return n / B * B;
}

static void check_eval_batches(int eval_batches, int nb) {
  if (eval_batches < nb) return;
  fprintf(stderr, "FATAL: --eval-batches %d: only %d batches were loaded, and at least one must be left to train on (load more with --data-size, or hold out fewer)\n",
          eval_batches, nb);
  abort();
}

void DataLoader::generate_random(FFModel& ff, const DLRMConfig& dlrm) {
  const bool chatty = ff.world_size <= 1 || ff.rank == 0;
  if (chatty) printf("[DLRM] Use random dataset...\n");
  num_samples = random_num_samples(ff.config, dlrm, ff.world_size);
  const int B = ff.config.batchSize;
  if (chatty) printf("[DLRM] Number of random samples = %d\n", num_samples);
  const uint64_t s0 = ff.config.seed * 1000003ULL;
  const int nb = num_samples / B;
  const int64_t Bl = ff.local_batch;
  // sparse ids: owner of table t keeps ids of every sample (it gathers for the global batch)
  for (size_t t = 0; t < batch_sparse_inputs.size(); t++) {
    if (!batch_sparse_inputs[t].impl->ptr) continue;          // this rank neither owns the table nor holds a column block of it
    const int64_t n = (int64_t)num_samples * bags[t];
    full_sparse[t] = (int64_t*)ff.dmalloc((size_t)n * sizeof(int64_t));
    if (dlrm.zipf_alpha > 0.0) generate_zipf(ff, full_sparse[t], n, s0 + 17 + t, dlrm.embedding_size[t], dlrm.zipf_alpha);
    else ff.check(ff.api->ffh_gen_indices(ff.ctx, full_sparse[t], n, s0 + 17 + t, 0, dlrm.embedding_size[t], ff.stream), "gen_indices");
    // --synthetic-bag-fill F < 1 (with --embedding-padding): a slot keeps its id with probability F, else it becomes the pad id; a stream per table,
    // indexed by the slot's global position, so every rank that holds the table's ids masks them alike
    if (ff.config.embedding_padding && dlrm.synthetic_bag_fill < 1.0)
      ff.check(ff.api->pad->ffh_pad_mask_indices(ff.ctx, full_sparse[t], n, s0 + 0x9AD + 31 * t, 0, (float)dlrm.synthetic_bag_fill, ff.stream), "pad_mask_indices");
  }
  // dense features and labels: this rank's slice [rank*Bl, (rank+1)*Bl) of every batch
  full_dense = (float*)ff.dmalloc((size_t)nb * Bl * dense_dim * sizeof(float));
  full_label = (float*)ff.dmalloc((size_t)nb * Bl * sizeof(float));
  for (int k = 0; k < nb; k++) {
    const int64_t n0 = (int64_t)k * B + (int64_t)ff.rank * Bl;
    ff.check(ff.api->ffh_gen_uniform01(ff.ctx, full_dense + (int64_t)k * Bl * dense_dim, Bl * dense_dim, s0 + 5, n0 * dense_dim, ff.stream), "gen dense");
    ff.check(ff.api->ffh_gen_bernoulli(ff.ctx, full_label + (int64_t)k * Bl, Bl, s0 + 7, n0, ff.stream), "gen label");
  }
  if (ff.config.synthetic_labels == 1) {
    // --synthetic-labels logistic: label ~ Bernoulli(sigmoid(4 * sum_j a_j (x_j - 1/2))) with hidden weights a_j in [-1, 1) fixed by the hash
    // (not by --seed: every seed draws other samples from the SAME model), the coin of sample n the hash stream the Bernoulli labels use.
    // On the host, from the dense features read back: same code for every kernel library.
    const size_t nd = (size_t)nb * Bl * dense_dim, nl = (size_t)nb * Bl;
    std::vector<float> xd(nd), lab(nl), a((size_t)dense_dim);
    for (int j = 0; j < dense_dim; j++) a[j] = ffh_uniform(ffh_hash(0x10615C1CULL, (uint64_t)j), -1.0f, 1.0f);
    ff.check(ff.api->ffh_stream_sync(ff.ctx, ff.stream), "synthetic labels");
    ff.check(ff.api->ffh_memcpy_d2h(ff.ctx, xd.data(), full_dense, nd * sizeof(float), ff.stream), "synthetic labels d2h");
    ff.check(ff.api->ffh_stream_sync(ff.ctx, ff.stream), "synthetic labels");
    for (int k = 0; k < nb; k++)
      for (int64_t i = 0; i < Bl; i++) {
        const size_t r = (size_t)k * Bl + (size_t)i;
        double z = 0.0;
        for (int j = 0; j < dense_dim; j++) z += (double)a[j] * ((double)xd[r * dense_dim + j] - 0.5);
        const double p = 1.0 / (1.0 + std::exp(-4.0 * z));
        const uint64_t n = (uint64_t)k * B + (uint64_t)ff.rank * Bl + (uint64_t)i;
        lab[r] = (double)ffh_u24(ffh_hash(s0 + 7, n)) < p ? 1.0f : 0.0f;
      }
    ff.check(ff.api->ffh_memcpy_h2d(ff.ctx, full_label, lab.data(), nl * sizeof(float), ff.stream), "synthetic labels h2d");
    ff.check(ff.api->ffh_stream_sync(ff.ctx, ff.stream), "synthetic labels");
    if (chatty) printf("[DLRM] synthetic labels: logistic model of the %d dense features\n", dense_dim);
  }
}

// --zipf-alpha A (not in the reference, whose ids are uniform: SURVEY 8d's duplicate-row stress).  Rank k of R is drawn
// with probability ~ (k+1)^-A through the inverse CDF of the continuous power law on [1, R+1); ranks are spread over the
// table by a golden-ratio multiplicative permutation so that hot rows are not neighbours.  Drawn on the host in double precision from
// the counter hash -- the same code feeds the HIP backend and the oracle backend, so both see identical ids.
void DataLoader::generate_zipf(FFModel& ff, int64_t* dst, int64_t n, uint64_t seed, int64_t rows, double alpha) {
  std::vector<int64_t> ids((size_t)n);
  const double a1 = 1.0 - alpha;
  const bool log_law = std::fabs(a1) < 1e-9;                    // alpha == 1: x = (R+1)^u
  const double top = log_law ? std::log((double)rows + 1.0) : std::pow((double)rows + 1.0, a1) - 1.0;
  uint64_t stride = (uint64_t)((double)rows * 0.6180339887498949) + 1;   // golden-ratio step, made coprime with the row count
  auto gcd = [](uint64_t a, uint64_t b) { while (b) { const uint64_t t = a % b; a = b; b = t; } return a; };
  while (gcd(stride, (uint64_t)rows) != 1) stride++;
  const uint64_t shift = ffh_hash(seed, ~0ULL) % (uint64_t)rows;
  for (int64_t i = 0; i < n; i++) {
    const double u = (double)(ffh_hash(seed, (uint64_t)i) >> 11) * (1.0 / 9007199254740992.0);
    const double x = log_law ? std::exp(u * top) : std::pow(1.0 + u * top, 1.0 / a1);
    int64_t k = (int64_t)x - 1;
    if (k < 0) k = 0;
    if (k >= rows) k = rows - 1;
    ids[(size_t)i] = (int64_t)(((uint64_t)k * (stride % (uint64_t)rows) + shift) % (uint64_t)rows);
  }
  ff.check(ff.api->ffh_memcpy_h2d(ff.ctx, dst, ids.data(), (size_t)n * sizeof(int64_t), ff.stream), "zipf ids H2D");
  ff.check(ff.api->ffh_stream_sync(ff.ctx, ff.stream), "zipf ids sync");
}

// The Criteo file of the reference [ref: examples/cpp/DLRM/dlrm.cc:279-326 (shape checks), :421-479 (H5Dread of X_cat as
// LLONG, X_int and y as FLOAT); written by preprocess_hdf.py:14-24]: X_int [N][dense] float (already log(x+1)),
// X_cat [N][sum of the tables' bag sizes] integer, y [N] or [N][1] float.  The whole set becomes device-resident in the same layout the
// synthetic generator produces; the file is read in row chunks so that host memory stays bounded.
void DataLoader::load_hdf5(FFModel& ff, const DLRMConfig& dlrm) {
  const bool chatty = ff.world_size <= 1 || ff.rank == 0;
  if (chatty) printf("[DLRM] Start loading dataset from %s\n", dlrm.dataset_path.c_str());
  Hdf5File file(dlrm.dataset_path);
  auto bad = [&](const char* what) {
    fprintf(stderr, "FATAL: --dataset %s: %s\n", dlrm.dataset_path.c_str(), what);
    abort();
  };
  const Hdf5Dataset xi = file.describe("X_int"), xc = file.describe("X_cat"), yy = file.describe("y");
  const size_t T = batch_sparse_inputs.size();
  if (xi.dims.size() != 2 || xi.type_class != 1) bad("X_int must be a 2-D float dataset");
  if ((int)xi.dims[1] != dense_dim) bad("X_int's second dimension must equal --arch-mlp-bot[0]");                 // [ref: dlrm.cc:292]
  if (xc.dims.size() != 2 || xc.type_class != 0) bad("X_cat must be a 2-D integer dataset");
  if (xc.dims[0] != xi.dims[0] || yy.dims[0] != xi.dims[0]) bad("X_int, X_cat and y must have the same number of samples");
  size_t C = 0;                      // X_cat's columns: table t's ids in [sum of the bag sizes before it, ... + bags[t])
  std::vector<size_t> col0(T);
  int max_bag = 1;
  for (size_t t = 0; t < T; t++) { col0[t] = C; C += (size_t)bags[t]; max_bag = std::max(max_bag, bags[t]); }
  if (xc.dims[1] != C) {             // [ref: dlrm.cc:307]
    char msg[192];
    snprintf(msg, sizeof msg, "X_cat's second dimension must equal the sum of the tables' bag sizes, %zu (it is %llu)", C, (unsigned long long)xc.dims[1]);
    bad(msg);
  }
  if (yy.dims.size() == 2 && yy.dims[1] != 1) bad("y must be [N] or [N][1]");
  const int B = ff.config.batchSize;
  uint64_t n_file = xi.dims[0];
  if (dlrm.data_size > 0 && (uint64_t)dlrm.data_size < n_file) n_file = (uint64_t)dlrm.data_size;   // --data-size caps what is loaded
  if (n_file / B == 0) bad("fewer samples than one batch");
  if (n_file / B * B > 0x7fffffffULL) bad("more than 2^31 samples");
  num_samples = (int)(n_file / B * B);       // the reference iterates num_samples / batchSize whole batches (dlrm.cc:157)
  const int nb = num_samples / B;
  const int64_t Bl = ff.local_batch;
  for (size_t t = 0; t < T; t++)
    if (batch_sparse_inputs[t].impl->ptr) full_sparse[t] = (int64_t*)ff.dmalloc((size_t)num_samples * bags[t] * sizeof(int64_t));
  full_dense = (float*)ff.dmalloc((size_t)nb * Bl * dense_dim * sizeof(float));
  full_label = (float*)ff.dmalloc((size_t)nb * Bl * sizeof(float));

  const int batches_per_chunk = std::max(1, (1 << 18) / B);       // about 256k samples per pass over the file
  std::vector<int64_t> cat((size_t)batches_per_chunk * B * C), col((size_t)batches_per_chunk * B * max_bag);
  std::vector<float> xint((size_t)batches_per_chunk * B * dense_dim), lab((size_t)batches_per_chunk * B);
  for (int k0 = 0; k0 < nb; k0 += batches_per_chunk) {
    const int kb = std::min(batches_per_chunk, nb - k0);
    const uint64_t row0 = (uint64_t)k0 * B, rows = (uint64_t)kb * B;
    file.read_rows_i64("X_cat", row0, rows, cat.data());
    file.read_rows_f32("X_int", row0, rows, xint.data());
    file.read_rows_f32("y", row0, rows, lab.data());
    for (size_t t = 0; t < T; t++) {
      if (!full_sparse[t]) continue;
      const int64_t R = dlrm.embedding_size[t];
      const int bag = bags[t];
      for (uint64_t i = 0; i < rows; i++)
        for (int j = 0; j < bag; j++) {
          const int64_t id = cat[i * C + col0[t] + j];
          // the reference gathers without a bounds check on the GPU and asserts on the CPU path (src/ops/embedding.cc:71-73)
          // ... but for the pad id -1, "no lookup", under --embedding-padding (include/ff_hip_pad.h)
          if ((id < 0 || id >= R) && !(id == FFH_EMB_PAD_ID && ff.config.embedding_padding)) {
            fprintf(stderr, "FATAL: --dataset %s: X_cat[%llu][%zu] = %lld is outside table %zu (%lld rows)%s\n", dlrm.dataset_path.c_str(),
                    (unsigned long long)(row0 + i), col0[t] + j, (long long)id, t, (long long)R,
                    id == FFH_EMB_PAD_ID ? "; if -1 means \"no lookup\" in this file, add --embedding-padding" : "");
            abort();
          }
          col[i * bag + j] = id;
        }
      ff.check(ff.api->ffh_memcpy_h2d(ff.ctx, full_sparse[t] + row0 * bag, col.data(), rows * bag * sizeof(int64_t), ff.stream), "dataset H2D");
      ff.check(ff.api->ffh_stream_sync(ff.ctx, ff.stream), "dataset sync");     // col is reused for the next table
    }
    for (int k = 0; k < kb; k++) {
      const size_t src = (size_t)k * B + (size_t)ff.rank * Bl;                   // this rank's slice of batch k0 + k
      ff.check(ff.api->ffh_memcpy_h2d(ff.ctx, full_dense + (int64_t)(k0 + k) * Bl * dense_dim, xint.data() + src * dense_dim,
                                      (size_t)Bl * dense_dim * sizeof(float), ff.stream), "dataset H2D");
      ff.check(ff.api->ffh_memcpy_h2d(ff.ctx, full_label + (int64_t)(k0 + k) * Bl, lab.data() + src, (size_t)Bl * sizeof(float), ff.stream), "dataset H2D");
    }
    ff.check(ff.api->ffh_stream_sync(ff.ctx, ff.stream), "dataset sync");
  }
  if (chatty) {
    printf("[DLRM] Finish loading dataset from %s\n", dlrm.dataset_path.c_str());
    printf("[DLRM] Loaded %d samples\n", num_samples);
  }
}

DataLoader::~DataLoader() {
  for (int64_t* p : full_sparse) if (p) model->api->ffh_free(model->ctx, p);
  if (full_dense) model->api->ffh_free(model->ctx, full_dense);
  if (full_label) model->api->ffh_free(model->ctx, full_label);
}

// [ref: examples/cpp/DLRM/dlrm.cc:482-585, dlrm.cu:19-122]: device-to-device copies on the compute stream
void DataLoader::next_batch(FFModel& ff) {
  const int B = ff.config.batchSize;
  if (next_index + B > num_train) { next_index = 0; epoch++; }      // (file order: every epoch is the same)
  if (ff.config.data_randomize) gather_batch(ff, next_index / B);
  else load_batch(ff, next_index / B);
  next_index += B;
}

// --data-randomize total (include/ffh_perm.h states the order and the stripe rule): where load_batch copies one block per
// array, the rows of a shuffled batch are scattered -- one gather launch on the compute stream, outside any captured step
void DataLoader::gather_batch(FFModel& ff, int64_t step) {
  const int64_t Bl = ff.local_batch;
  ffh_batch_order order;
  order.seed = ff.config.seed;
  order.epoch = epoch;
  order.step = step;
  order.local_batch = Bl;
  order.n_local = (int64_t)(num_train / ff.config.batchSize) * Bl;
  order.world = std::max(1, ff.world_size);
  order.rank = ff.rank;
  ff.order_input_writes_behind_update();       // as load_batch
  ff.check(ff.api->data->ffh_batch_gather(ff.ctx, segments.data(), (int)segments.size(), &order, ff.stream), "batch gather");
  ff.inputs_dirty = true;
}

void DataLoader::load_batch(FFModel& ff, int k) {
  const int B = ff.config.batchSize;
  const int64_t Bl = ff.local_batch;
  const int64_t first = (int64_t)k * B;          // first sample of batch k
  ff.order_input_writes_behind_update();       // eager steps: the last step's table update may still be reading the ids
  for (size_t t = 0; t < batch_sparse_inputs.size(); t++) {
    if (!full_sparse[t]) continue;
    ff.check(ff.api->ffh_memcpy_d2d(ff.ctx, batch_sparse_inputs[t].impl->ptr, full_sparse[t] + first * bags[t],
                                    (size_t)B * bags[t] * sizeof(int64_t), ff.stream), "load sparse");
  }
  ff.check(ff.api->ffh_memcpy_d2d(ff.ctx, batch_dense_input.impl->ptr, full_dense + (int64_t)k * Bl * dense_dim,
                                  (size_t)Bl * dense_dim * sizeof(float), ff.stream), "load dense");
  ff.check(ff.api->ffh_memcpy_d2d(ff.ctx, batch_label.impl->ptr, full_label + (int64_t)k * Bl, (size_t)Bl * sizeof(float), ff.stream),
           "load label");
  ff.inputs_dirty = true;
}

// =============================================================================================
// --backtrace-on-crash (debugging aid): SIGSEGV / SIGBUS / SIGABRT print the native call stack of the faulting thread before the
// process dies (glibc backtrace_symbols_fd: async-signal-safe enough for a last word; the GPU box has no core dumps to look at)
static void crash_backtrace(int sig) {
  void* frames[64];
  const int n = backtrace(frames, 64);
  const char msg[] = "\n[DLRM] fatal signal, native backtrace:\n";
  if (write(2, msg, sizeof msg - 1) < 0) {}
  backtrace_symbols_fd(frames, n, 2);
  signal(sig, SIG_DFL);
  raise(sig);
}

DLRMApp::DLRMApp(int argc, char** argv, const ffcomm* comm) : ff(nullptr), loader(nullptr), warmed_up(false) {
  for (int i = 1; i < argc; i++)
    if (!strcmp(argv[i], "--backtrace-on-crash")) { signal(SIGSEGV, crash_backtrace); signal(SIGBUS, crash_backtrace); signal(SIGABRT, crash_backtrace); }
  ffconfig.parse_args(argv, argc);
  if (comm) ffconfig.comm = *comm;
  parse_input_args(argv, argc, dlrm);
  const bool chatty = ffconfig.comm.world_size <= 1 || ffconfig.comm.rank == 0;
  if (chatty) {
    printf("[DLRM] batchSize(%d) workersPerNodes(%d) numNodes(%d)\n", ffconfig.batchSize, ffconfig.workersPerNode, ffconfig.numNodes);
    if (dlrm.embedding_bag_sizes.empty()) printf("[DLRM] EmbeddingBagSize(%d)\n", dlrm.embedding_bag_size);
    else {
      std::string list;
      for (size_t i = 0; i < dlrm.embedding_bag_sizes.size(); i++) list += (i ? "-" : "") + std::to_string(dlrm.embedding_bag_sizes[i]);
      printf("[DLRM] EmbeddingBagSizes(%s)\n", list.c_str());
    }
    print_vector("Embedding Vocab Sizes", dlrm.embedding_size);
    print_vector("MLP Top", dlrm.mlp_top);
    print_vector("MLP Bot", dlrm.mlp_bot);
    if (dlrm.arch_interaction_op == "dcn") {      // (flushed: a refusal below aborts, and a pipe would lose what says which model was asked for)
      printf("[DLRM] interaction: dcn layers %d rank %d\n", dlrm.dcn_num_layers, dlrm.dcn_low_rank_dim);
      fflush(stdout);
    }
  }
  if (dlrm.arch_interaction_op == "dcn") {
    if (dlrm.dcn_num_layers < 1) { fprintf(stderr, "FATAL: --dcn-num-layers %d: must be >= 1\n", dlrm.dcn_num_layers); abort(); }
    if (dlrm.dcn_low_rank_dim < 1) { fprintf(stderr, "FATAL: --dcn-low-rank-dim %d: must be >= 1\n", dlrm.dcn_low_rank_dim); abort(); }
    // the cross network keeps the width of its input: the concat of the bottom-MLP output and one vector per table
    const long long D = (long long)dlrm.mlp_bot.back() + (long long)dlrm.embedding_size.size() * dlrm.sparse_feature_size;
    if (dlrm.mlp_top.empty() || dlrm.mlp_top[0] != D) {
      fprintf(stderr, "FATAL: --arch-interaction-op dcn: --arch-mlp-top must start with the interaction's width %lld (bottom-MLP output %d + %zu tables x "
                      "--arch-sparse-feature-size %d), not %d\n", D, dlrm.mlp_bot.back(), dlrm.embedding_size.size(), dlrm.sparse_feature_size,
              dlrm.mlp_top.empty() ? 0 : dlrm.mlp_top[0]);
      abort();
    }
  }
  if (!dlrm.embedding_bag_sizes.empty()) {
    // --embedding-bag-sizes: one entry >= 1 per table, instead of --embedding-bag-size
    if (dlrm.bag_size_given) {
      fprintf(stderr, "FATAL: --embedding-bag-sizes and --embedding-bag-size were both given: give the per-table list or the one size, not both\n");
      abort();
    }
    if (dlrm.embedding_bag_sizes.size() != dlrm.embedding_size.size()) {
      fprintf(stderr, "FATAL: --embedding-bag-sizes has %zu entries for %zu tables (--arch-embedding-size): give one bag size per table, or one for all with "
                      "--embedding-bag-size\n", dlrm.embedding_bag_sizes.size(), dlrm.embedding_size.size());
      abort();
    }
    for (size_t i = 0; i < dlrm.embedding_bag_sizes.size(); i++)
      if (dlrm.embedding_bag_sizes[i] < 1) {
        fprintf(stderr, "FATAL: --embedding-bag-sizes: entry %zu is %d, a bag size must be >= 1 (--embedding-bag-size has the same rule)\n", i, dlrm.embedding_bag_sizes[i]);
        abort();
      }
  }
  if (dlrm.embedding_size.size() > MAX_NUM_EMB) { fprintf(stderr, "FATAL: more than %d tables\n", MAX_NUM_EMB); abort(); }
  ff = new FFModel(ffconfig);

  for (size_t i = 0; i < dlrm.embedding_size.size(); i++) {
    const int dims[] = {ffconfig.batchSize, dlrm.bag_of(i)};
    sparse_inputs.push_back(ff->create_tensor<2>(dims, DT_INT64));
  }
  {
    const int dims[] = {ffconfig.batchSize, dlrm.mlp_bot[0]};
    dense_input = ff->create_tensor<2>(dims, DT_FLOAT);
  }
  // Step 1 create dense_mlp
  Tensor x = create_mlp(ff, dense_input, dlrm.mlp_bot, dlrm.sigmoid_bot);
  std::vector<Tensor> ly;
  for (size_t i = 0; i < dlrm.embedding_size.size(); i++)
    ly.push_back(create_emb(ff, sparse_inputs[i], dlrm.embedding_size[i], dlrm.sparse_feature_size, (int)i, dlrm.mean_pooling ? AGGR_MODE_AVG : AGGR_MODE_SUM));
  Tensor z = interact_features(ff, x, ly, dlrm.arch_interaction_op, dlrm.dcn_num_layers, dlrm.dcn_low_rank_dim);
  create_mlp(ff, z, dlrm.mlp_top, (int)dlrm.mlp_top.size() - 2);
  if (dlrm.loss_threshold > 0.0f && dlrm.loss_threshold < 1.0f) {
    fprintf(stderr, "FATAL: --loss-threshold clamp is not implemented (the reference asserts here, dlrm.cc:125-128)\n");
    abort();
  }
  // Use SGD Optimizer [ref: examples/cpp/DLRM/dlrm.cc:130: SGDOptimizer(&ff, 0.01f), the reference driver's only choice].
  // --optimizer (this build): the other optimizers of the reference's library behind the same driver -- "sgd-momentum" =
  // SGDOptimizer(lr 0.01, momentum 0.9), "adam" = AdamOptimizer with its defaults [ref: include/optimizer.h:40-42,62-85]
  // SGD's rate is --lr (FFConfig::learningRate; its default is the reference driver's 0.01f): the base rate of the schedule
  if (dlrm.optimizer == "sgd") optimizer = new SGDOptimizer(ff, ffconfig.learningRate);
  else if (dlrm.optimizer == "sgd-momentum") optimizer = new SGDOptimizer(ff, ffconfig.learningRate, 0.9f);
  else if (dlrm.optimizer == "adam") optimizer = new AdamOptimizer(ff);
  // "adagrad" (DESIGN section 16): torch.optim.Adagrad's element-wise rule at rate --lr, no weight decay -- the MLPerf DLRM-DCNv2 recipe's
  else if (dlrm.optimizer == "adagrad") optimizer = new AdagradOptimizer(ff, ffconfig.learningRate, 0.0, ffconfig.adagrad_eps, ffconfig.adagrad_initial_accumulator);
  else { fprintf(stderr, "FATAL: --optimizer %s: 'sgd', 'sgd-momentum', 'adam' or 'adagrad'\n", dlrm.optimizer.c_str()); abort(); }
  std::vector<MetricsType> metrics;
  metrics.push_back(METRICS_ACCURACY);
  metrics.push_back(METRICS_MEAN_SQUARED_ERROR);
  const bool bce = ffconfig.driver_loss == LOSS_BINARY_CROSSENTROPY;
  if (bce) metrics.push_back(METRICS_BINARY_CROSSENTROPY);
  if (ffconfig.eval_batches > 0) metrics.push_back(METRICS_AUC);
  if (ffconfig.eval_only && ffconfig.eval_batches <= 0) { fprintf(stderr, "FATAL: --eval-only needs --eval-batches N\n"); abort(); }
  // (synthetic data: its size is known here, so a hold-out that leaves nothing to train on is refused before anything is allocated; a file: by the loader)
  if (ffconfig.eval_batches > 0 && dlrm.dataset_path.empty())
    check_eval_batches(ffconfig.eval_batches, random_num_samples(ffconfig, dlrm, std::max(1, ffconfig.comm.world_size)) / ffconfig.batchSize);
  if (chatty) printf("[DLRM] loss: %s\n", bce ? "bce" : "mse");
  // --data-randomize total reorders what train_steps loads; a run that loads nothing per step has nothing to reorder
  if (ffconfig.data_randomize && dlrm.dataset_path.empty() && ffconfig.synthetic_labels != 1) {
    fprintf(stderr, "FATAL: --data-randomize total: this run never advances its batch (plain synthetic data trains on the warm-up batch again and again); "
                    "give it a data set to walk with --dataset FILE or --synthetic-labels logistic, or use --data-randomize none\n");
    abort();
  }
  if (chatty) {
    if (!ffconfig.data_randomize) printf("[DLRM] data order: none (file order, the same every epoch)\n");
    else printf("[DLRM] data order: total (seed %llu, a new order every epoch%s)\n", (unsigned long long)ffconfig.seed,
                ffconfig.comm.world_size > 1 ? ", per-rank stripes" : "");
  }
  if (dlrm.bag_fill_given && !ffconfig.embedding_padding) {
    fprintf(stderr, "FATAL: --synthetic-bag-fill %g leaves slots of a bag without a lookup, which only --embedding-padding trains on: add --embedding-padding, "
                    "or drop --synthetic-bag-fill\n", dlrm.synthetic_bag_fill);
    abort();
  }
  ff->compile(optimizer, (LossType)ffconfig.driver_loss, metrics);
  if (chatty && ffconfig.embedding_padding) printf("[DLRM] embedding padding: id -1 is no lookup (synthetic fill %g)\n", dlrm.synthetic_bag_fill);
  // --embedding-pooling, only when given: a mean divides by a table's bag size L_t, or under --embedding-padding by the lookups a bag really has
  if (chatty && dlrm.pooling_given)
    printf("[DLRM] embedding pooling: %s\n", !dlrm.mean_pooling ? "sum" : ffconfig.embedding_padding ? "mean (over the lookups that are there)" : "mean (over L_t slots)");
  if (chatty && !dlrm.embedding_bag_sizes.empty()) printf("[DLRM] embedding gather: %s\n", ff->bag_gather_line().c_str());      // a per-table list: how the gather runs
  if (chatty && ff->mixed_bags && ff->fused_embedding_update()) printf("[DLRM] embedding update: %s\n", ff->bag_update_line().c_str());      // ... and, where the sizes differ, the update
  if (const AdagradOptimizer* ag = dynamic_cast<const AdagradOptimizer*>(optimizer)) {
    // what --optimizer adagrad allocated on this rank: S beside every fp32 weight it updates, fp32 beside bf16 tables too (on fp32 tables it doubles their HBM)
    size_t bytes = ag->state_bytes;
    for (const Embedding* e : ff->embeddings)
      if (e->opt_state[0]) bytes += ag->rowwise ? e->weights[0].get_volume() / (size_t)e->out_channels * 4
                                                : e->weights[0].get_volume() * 4 + (e->row_sharded ? (size_t)e->out_channels * 4 : 0);
    if (chatty && ag->rowwise)      // --adagrad-rowwise: one float per table row
      printf("[DLRM] optimizer: adagrad eps=%g A=%g lr=%g, tables: %s, accumulator %zu bytes (%.3f GB) on rank %d\n", ag->epsilon, ag->initial_accumulator, ag->lr,
             ff->embeddings.empty() ? "none" : "fused row-wise", bytes, bytes / 1e9, ff->rank);
    else if (chatty)
      printf("[DLRM] optimizer: adagrad eps=%g A=%g lr=%g, tables: %s, accumulator %zu bytes (%.3f GB) on rank %d\n", ag->epsilon, ag->initial_accumulator, ag->lr,
             ff->embeddings.empty() ? "none" : (ff->fused_embedding_update() ? "fused" : "dense"), bytes, bytes / 1e9, ff->rank);
  }
  // which learning-rate route runs, and why; silent without the flags
  if (chatty && (ffconfig.lr_warmup_steps || ffconfig.lr_num_decay_steps || ffconfig.lr_decay_start_step || ffconfig.device_lr || ffconfig.host_lr_schedule))
    printf("[DLRM] lr schedule: %s\n", ff->lr_schedule_line().c_str());
  if (chatty && ff->q8_on() && !ff->embeddings.empty()) printf("[DLRM] eval tables: %s\n", ff->q8_line().c_str());      // what --eval-embedding-dtype int8 allocated on this rank
  if (chatty && ffconfig.embedding_dtype == DT_BF16) {
    // what --embedding-dtype bf16 did: data-parallel (replicated) tables live in the dense slab and stay fp32
    size_t bytes = 0;
    int n16 = 0;
    std::string fp32_tables;
    for (const Embedding* e : ff->embeddings) {
      if (e->weights[0].impl && e->weights[0].impl->ptr) bytes += e->weights[0].impl->bytes;
      if (e->bf16_weights()) n16++;
      else fp32_tables += std::string(fp32_tables.empty() ? "" : ",") + e->name;
    }
    printf("[DLRM] embedding tables: bf16 (%s rounding) %d of %zu, %.3f GB on rank %d; fp32 (data-parallel): %s\n",
           ffconfig.embedding_rounding == FFH_BF16_ROUND_NEAREST ? "nearest" : "stochastic", n16, ff->embeddings.size(), bytes / 1e9,
           ff->rank, fp32_tables.empty() ? "none" : fp32_tables.c_str());
  }
  loader = new DataLoader(*ff, dlrm, sparse_inputs, dense_input, ff->label_tensor);
  ff->init_layers();
  // checkpoint / resume; silent without the flags
  if (ffconfig.checkpoint_every_epochs > 0 && ffconfig.save_checkpoint_dir.empty()) {
    fprintf(stderr, "FATAL: --checkpoint-every-epochs %d: needs --save-checkpoint DIR to say where\n", ffconfig.checkpoint_every_epochs);
    abort();
  }
  if (!ffconfig.load_checkpoint_dir.empty()) {
    const FFModel::CheckpointInfo info = ff->load_checkpoint(ffconfig.load_checkpoint_dir);
    start_epoch = (int)info.epochs_done;
    if (chatty)
      printf("[DLRM] checkpoint: loaded %s (epoch %lld, step %lld, digest 0x%016llx)\n", ffconfig.load_checkpoint_dir.c_str(), (long long)info.epochs_done,
             (long long)info.steps, (unsigned long long)info.digest);
  } else if (chatty && !ffconfig.save_checkpoint_dir.empty()) {
    printf("[DLRM] checkpoint: none\n");
  }
  if (chatty) fflush(stdout);
}

double DLRMApp::save_checkpoint(int epochs_done) {
  ff->sync();
  const double t0 = now_us();
  ff->save_checkpoint(ffconfig.save_checkpoint_dir, epochs_done);
  if (ffconfig.comm.world_size > 1 && ffconfig.comm.barrier) ffconfig.comm.barrier(ffconfig.comm.user);      // a checkpoint is complete once every rank's file is
  return 1e-6 * (now_us() - t0);
}

DLRMApp::~DLRMApp() {
  if (ff) ff->sync();
  delete loader;
  delete ff;
  delete optimizer;
}

void DLRMApp::warmup() {
  // [ref: examples/cpp/DLRM/dlrm.cc:139-149]; --data-randomize total: batch 0 of epoch 0's order
  loader->reset(0);
  ff->reset_metrics();
  loader->next_batch(*ff);
  ff->forward();
  ff->zero_gradients();
  ff->backward();
  ff->update();
  ff->sync();
  warmed_up = true;
}

double DLRMApp::evaluate(int epoch, EvalMetrics* out) {
  ff->sync();
  const double t0 = now_us();
  const int B = ffconfig.batchSize, first = loader->num_train / B, nb = loader->num_samples / B;
  ff->reset_eval_metrics();
  for (int k = first; k < nb; k++) {
    loader->load_batch(*ff, k);
    ff->eval_batch();
  }
  EvalMetrics m = ff->get_eval_metrics();
  loader->load_batch(*ff, 0);            // what the warm-up left in the inputs: a synthetic run trains on it without reloading
  ff->sync();
  const double secs = 1e-6 * (now_us() - t0);
  if (ff->rank == 0)
    printf("EVAL epoch %d: samples %llu logloss %.4f accuracy %.4f auc %.4f time %.4fs\n", epoch, (unsigned long long)m.samples, m.logloss(), m.accuracy(),
           m.auc, secs);
  if (out) *out = m;
  return secs;
}

void DLRMApp::train_steps(int n, bool trace) {
  for (int it = 0; it < n; it++) {
    // random input: the batch loaded in the warm-up is reused; a dataset advances every iteration, outside the trace
    // [ref: examples/cpp/DLRM/dlrm.cc:167-175]
    if (!dlrm.dataset_path.empty() || ffconfig.synthetic_labels == 1) loader->next_batch(*ff);      // (learnable synthetic labels: iterated like a data set)
    if (trace) ff->begin_trace(111 /*trace_id*/);
    ff->forward();
    ff->zero_gradients();
    ff->backward();
    ff->update();
    if (trace) ff->end_trace(111 /*trace_id*/);
  }
}

double DLRMApp::run_epochs() {
  const bool resumed = !ffconfig.load_checkpoint_dir.empty();
  // (--eval-only: no training step at all.  --load-checkpoint: the warm-up step is part of what the checkpoint holds; the inputs get the batch
  //  the warm-up would have left in them, which a plain synthetic run trains on without ever loading another)
  if (resumed && !warmed_up) { loader->reset(0); loader->load_batch(*ff, 0); warmed_up = true; }
  if (!warmed_up && !ffconfig.eval_only) warmup();
  if (ff->config.trace_mode < 0) ff->config.trace_mode = 0;     // the driver's loop: a step is replayed only where the replay is not slower (FFConfig::trace_mode)
  const bool chatty = ff->rank == 0;
  ff->sync();   // issue_execution_fence + timing measurement
  if (ffconfig.comm.world_size > 1 && ffconfig.comm.barrier) ffconfig.comm.barrier(ffconfig.comm.user);
  if (chatty) {
    printf("[DLRM] Warmup finished...Start timer...\n");
    printf("[DLRM] Num. epochs = %d\n", ffconfig.epochs);
    printf("[DLRM] Num. iterations/epoch = %d\n", loader->num_train / ffconfig.batchSize);
    printf("parameters.size() = %lu\n", ff->parameters.size());
  }
  double eval_secs = 0.0;                // evaluation is outside the timed region: its wall time is taken out again below
  const double ts_start = now_us();
  double save_secs = 0.0;                // ... and so is saving a checkpoint
  int epochs_run = 0;
  if (ffconfig.eval_only) eval_secs += evaluate(start_epoch);      // (a loaded model: under the epoch number its last evaluation had)
  for (int epoch = start_epoch; epoch < ffconfig.epochs && !ffconfig.eval_only; epoch++) {
    loader->reset(epoch);
    ff->reset_metrics();
    const int iterations = loader->num_train / ffconfig.batchSize;
    train_steps(iterations, epoch > 0 /* the reference traces from the second epoch on */);
    if (ffconfig.eval_batches > 0) eval_secs += evaluate(epoch + 1);
    epochs_run++;
    // epoch boundaries only: the data cursor is 0 and the next epoch's order follows from (--seed, epoch) alone
    const bool last = epoch + 1 == ffconfig.epochs;
    if (!ffconfig.save_checkpoint_dir.empty() && (last || (ffconfig.checkpoint_every_epochs > 0 && (epoch + 1) % ffconfig.checkpoint_every_epochs == 0)))
      save_secs += save_checkpoint(epoch + 1);
  }
  // (nothing left to train -- a checkpoint that had already completed --epochs -- or --eval-only: the state is saved as it is)
  if (!ffconfig.save_checkpoint_dir.empty() && epochs_run == 0) save_secs += save_checkpoint(start_epoch);
  ff->sync();
  if (ffconfig.comm.world_size > 1 && ffconfig.comm.barrier) ffconfig.comm.barrier(ffconfig.comm.user);
  const double ts_end = now_us();
  const double run_time = 1e-6 * (ts_end - ts_start) - eval_secs - save_secs;
  if (chatty && !ffconfig.eval_only) {      // (--eval-only trained nothing: no training metrics, no throughput)
    PerfMetrics pm = ff->get_perf_metrics();
    pm.print(ff->metrics_flags);
    // [ref: examples/cpp/DLRM/dlrm.cc:193-194] -- the reference's line as it is; a kernel library other than the product's own
    // (--backend / FFH_BACKEND_LIB: the CPU oracle in tests, an A/B build) is named on it, so a number can never be mistaken
    printf("ELAPSED TIME = %.4fs, THROUGHPUT = %.2f samples/s", run_time, loader->num_train * (double)(resumed ? epochs_run : ffconfig.epochs) / run_time);
    if (ffconfig.eval_batches > 0) printf("  [wall time minus %.4fs of evaluation]", eval_secs);
    if (!ffconfig.save_checkpoint_dir.empty()) printf("  [wall time minus %.4fs of checkpoint saving]", save_secs);
    if (resumed) printf("  [resumed: epochs %d to %d]", start_epoch, start_epoch + epochs_run);
    if (ff->api->overridden) printf("  [kernel library: %s, %s]", ff->api->ffh_backend_name(), ff->api->path.c_str());
    printf("\n");
  }
  return run_time;
}

int dlrm_main(int argc, char** argv, const ffcomm* comm) {
  DLRMApp app(argc, argv, comm);
  app.run_epochs();
  return 0;
}
