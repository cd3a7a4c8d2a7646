// checkpoint.cc -- FFModel::save_checkpoint / load_checkpoint / state_digest
// (one of the translation units of the host shim: model_internal.h lists them)
//
// A checkpoint is a directory with one file per rank, rank-R-of-N.ffck:
//   bytes 0..7    magic "FFHCKPT\n"
//   bytes 8..11   format version (little-endian uint32), bytes 12..15 zero
//   bytes 16..23  length of the manifest in bytes (little-endian uint64)
//   bytes 24..    the manifest: text, one "key value..." line each, closed by "end"
//   zero padding to the next multiple of 4096: the first record byte
//   the records, each at the offset (counted from the first record byte, a multiple of 64) its manifest line gives
// A record is the logical rows x cols contents of one piece of state, row-major without pad columns: a file does not depend on the
// leading dimensions the saving model chose.  Every record carries its digest (include/ff_hip_digest.h, seed ffh_digest_record_seed(ordinal)),
// computed on the device from the buffer itself where the kernel library has the extension and on the host from the bytes copied
// otherwise; load_checkpoint() verifies it the same way after the host-to-device copy.  The big tables move through one bounded staging
// buffer; there is never a second full copy on the host or the device.  The file is written under a temporary name and renamed.
#include "model_internal.h"

#include <sys/stat.h>
#include <sys/types.h>
#include <dirent.h>
#include <unistd.h>
#include <cerrno>
#include <sstream>

#include "../../include/ff_hip_digest.h"

namespace {

constexpr char kMagic[8] = {'F', 'F', 'H', 'C', 'K', 'P', 'T', '\n'};
constexpr uint32_t kVersion = 1;
constexpr size_t kStageBytes = (size_t)8 << 20;      // the staging buffer of the copies
constexpr size_t kDataAlign = 4096, kRecordAlign = 64;

struct CkRecord {
  std::string name, type;        // type: f32 | bf16 | u64 | raw
  int64_t rows = 0, cols = 0;
  int elem = 0;                  // bytes per element (raw: 1)
  char* dev = nullptr;           // device record: element (0, 0) ...
  int64_t ld_bytes = 0;          // ... and the bytes between its rows
  std::vector<char> host;        // host record (optimizer scalars): the bytes themselves
  bool on_host = false;
  char* zero_tail = nullptr;     // load: cleared behind the record (the spare zero row of a row shard)
  size_t zero_tail_bytes = 0;
  // from / for the manifest
  uint64_t offset = 0, digest = 0;
  int64_t row_bytes() const { return cols * elem; }
  uint64_t bytes() const { return (uint64_t)rows * (uint64_t)row_bytes(); }
};

const char* optimizer_kind(const FFModel* ff) {
  if (const SGDOptimizer* s = dynamic_cast<const SGDOptimizer*>(ff->optimizer)) return s->momentum > 0.0 ? "sgd-momentum" : "sgd";
  if (dynamic_cast<const AdamOptimizer*>(ff->optimizer)) return "adam";
  if (const AdagradOptimizer* a = dynamic_cast<const AdagradOptimizer*>(ff->optimizer)) return a->rowwise ? "adagrad-rowwise" : "adagrad";
  return "none";
}
// how the tables are updated: what --sparse-embedding-optimizer / --dense-embedding-update select for this optimizer
const char* table_optimizer_kind(const FFModel* ff) {
  if (ff->embeddings.empty()) return "none";
  if (!ff->fused_embedding_update()) return "dense";
  ffh_sparse_opt rule;
  return ff->sparse_rule(rule) ? "sparse" : "fused-sgd";
}
const char* lr_route_name(int r) { return r == FFModel::kLrDevice ? "device" : (r == FFModel::kLrHost ? "host" : "off"); }

std::string placement_of(const FFModel* ff, const Embedding* e) {
  char buf[128];
  if (e->replicated) return "replicated";
  if (e->row_sharded) { snprintf(buf, sizeof buf, "row:%lld:%lld", (long long)e->row_begin, (long long)e->rows_local); return buf; }
  if (e->column_sharded) {
    int col0 = 0;
    for (const FFModel::EmbShard& s : ff->shards) if (s.e == e && s.owner == ff->rank) col0 = s.col0;
    snprintf(buf, sizeof buf, "column:%d:%d", col0, e->local_cols);
    return buf;
  }
  snprintf(buf, sizeof buf, "table-wise:%d", e->owner_rank);
  return buf;
}

CkRecord device_record(const std::string& name, const char* type, int elem, void* dev, int64_t rows, int64_t cols, int64_t ld_elems) {
  CkRecord r;
  r.name = name; r.type = type; r.elem = elem; r.dev = (char*)dev; r.rows = rows; r.cols = cols; r.ld_bytes = ld_elems * elem;
  return r;
}

// Every piece of state a resumed run needs, in one fixed order (DESIGN section 15 gives the reason for each)
std::vector<CkRecord> collect_records(FFModel* ff) {
  std::vector<CkRecord> out;
  SGDOptimizer* sgd = dynamic_cast<SGDOptimizer*>(ff->optimizer);
  AdamOptimizer* adam = dynamic_cast<AdamOptimizer*>(ff->optimizer);
  AdagradOptimizer* adagrad = dynamic_cast<AdagradOptimizer*>(ff->optimizer);
  for (Op* op : ff->layers) {
    for (int i = 0; i < op->numWeights; i++) {
      const Parameter& p = op->weights[i];
      const TensorImpl* im = p.impl;
      if (!im || !im->ptr) continue;                       // a table another rank holds
      const std::string id = std::string(op->name) + "/" + std::to_string(i);
      const bool bf16 = p.data_type == DT_BF16;
      if (!bf16 && p.data_type != DT_FLOAT) die("checkpoint: parameter %s has an element type a checkpoint cannot carry", id.c_str());
      const int64_t rows = im->rows_local, cols = p.adim[0];
      CkRecord w = device_record("param/" + id, bf16 ? "bf16" : "f32", bf16 ? 2 : 4, im->ptr, rows, cols, im->ld);
      const Embedding* e = op->op_type == OP_EMBEDDING ? static_cast<const Embedding*>(op) : nullptr;
      if (e && e->row_sharded) { w.zero_tail = (char*)im->ptr + im->bytes; w.zero_tail_bytes = (size_t)e->out_channels * 4; }
      out.push_back(w);
      // dense optimizer state, laid out like the weight it belongs to (fp32 parameters only: a bf16 table is updated on the fused path)
      if (sgd) {
        auto it = sgd->v_values.find(im->ptr);
        if (it != sgd->v_values.end() && !bf16) out.push_back(device_record("sgd_v/" + id, "f32", 4, it->second, rows, cols, im->ld));
      }
      if (adam && im->grad && !bf16) {
        float *m = nullptr, *v = nullptr;
        if (in_dense_slab(p)) {
          const size_t off = (size_t)((float*)im->ptr - ff->mlp_weights);
          if (adam->mlp_m) { m = adam->mlp_m + off; v = adam->mlp_v + off; }
        } else {
          auto it = adam->mv_values.find(im->ptr);
          if (it != adam->mv_values.end()) { m = it->second.first; v = it->second.second; }
        }
        if (m) {
          out.push_back(device_record("adam_m/" + id, "f32", 4, m, rows, cols, im->ld));
          out.push_back(device_record("adam_v/" + id, "f32", 4, v, rows, cols, im->ld));
        }
      }
      if (adagrad && im->grad && !bf16) {
        float* S = nullptr;
        if (in_dense_slab(p)) {
          if (adagrad->mlp_s) S = adagrad->mlp_s + (size_t)((float*)im->ptr - ff->mlp_weights);
        } else {
          auto it = adagrad->s_values.find(im->ptr);
          if (it != adagrad->s_values.end()) S = it->second;
        }
        if (S) out.push_back(device_record("adagrad_s/" + id, "f32", 4, S, rows, cols, im->ld));
      }
      // per-row state of --sparse-embedding-optimizer (Adagrad without weight decay: of its default table route): fp32 whatever the table's storage, contiguous
      if (e && i == 0)
        for (int k = 0; k < 2; k++)
          if (e->opt_state[k]) {
            const int64_t scols = adagrad && adagrad->rowwise ? 1 : cols;      // (--adagrad-rowwise: one float per row)
            CkRecord s = device_record("sparse_state" + std::to_string(k) + "/" + id, "f32", 4, e->opt_state[k], rows, scols, scols);
            if (e->row_sharded) { s.zero_tail = (char*)e->opt_state[k] + (size_t)rows * cols * 4; s.zero_tail_bytes = (size_t)e->out_channels * 4; }
            out.push_back(s);
          }
    }
  }
  // Adam's running beta products and step size as the doubles they are: re-deriving them by pow() would round differently.  Not on the device
  // learning-rate route: every launch reads the blocks there, the host copies are dead, and how often next() advanced them depends on how
  // many steps were graph replays
  if (adam && ff->lr_route != FFModel::kLrDevice) {
    CkRecord r;
    r.name = "adam_scalars"; r.type = "raw"; r.elem = 1; r.rows = 1; r.cols = 3 * sizeof(double); r.on_host = true;
    const double s[3] = {adam->beta1_t, adam->beta2_t, adam->alpha_t};
    r.host.assign((const char*)s, (const char*)s + sizeof s);
    out.push_back(r);
  }
  if (ff->lr_route == FFModel::kLrDevice) {
    const int64_t n = (int64_t)ff->api->lr->ffh_lr_state_bytes();
    if (n < 2 || (n & 1)) die("checkpoint: ffh_lr_state_bytes() = %lld is not an even size", (long long)n);
    for (int i = 0; i < 2; i++) out.push_back(device_record("lr_block/" + std::to_string(i), "raw", 1, ff->lr_block[i], 1, n, n));
  }
  if (ff->bf16_counter) out.push_back(device_record("bf16_counter", "u64", 8, ff->bf16_counter, 1, 1, 1));
  uint64_t off = 0;
  for (CkRecord& r : out) {
    r.offset = off;
    off += (r.bytes() + kRecordAlign - 1) / kRecordAlign * kRecordAlign;
  }
  return out;
}

// the digest of a device record from the device buffer itself (needs the extension)
uint64_t device_digest(FFModel* ff, const CkRecord& r, uint64_t seed, bool fold) {
  if (!ff->digest_acc) ff->digest_acc = (uint64_t*)ff->dmalloc(sizeof(uint64_t));
  if (!fold) ff->check(ff->api->ffh_zero(ff->ctx, ff->digest_acc, sizeof(uint64_t), ff->stream), "digest accumulator");
  ff->check(ff->api->digest->ffh_state_digest(ff->ctx, r.dev, r.rows, r.row_bytes(), r.ld_bytes, seed, 0, ff->digest_acc, ff->stream), "state_digest");
  if (fold) return 0;
  uint64_t v = 0;
  ff->check(ff->api->ffh_memcpy_d2h(ff->ctx, &v, ff->digest_acc, sizeof v, ff->stream), "digest d2h");
  ff->check(ff->api->ffh_stream_sync(ff->ctx, ff->stream), "digest sync");
  return v;
}

// rows [r0, r0 + n) of a device record <-> the staging buffer (contiguous rows of row_bytes)
void copy_rows(FFModel* ff, const CkRecord& r, int64_t r0, int64_t n, char* stage, bool to_device) {
  const int64_t rb = r.row_bytes();
  auto one = [&](char* dev, char* host, size_t bytes) {
    if (to_device) ff->check(ff->api->ffh_memcpy_h2d(ff->ctx, dev, host, bytes, ff->stream), "checkpoint h2d");
    else ff->check(ff->api->ffh_memcpy_d2h(ff->ctx, host, dev, bytes, ff->stream), "checkpoint d2h");
  };
  if (r.ld_bytes == rb) one(r.dev + r0 * rb, stage, (size_t)(n * rb));
  else for (int64_t k = 0; k < n; k++) one(r.dev + (r0 + k) * r.ld_bytes, stage + k * rb, (size_t)rb);
  ff->check(ff->api->ffh_stream_sync(ff->ctx, ff->stream), "checkpoint copy sync");      // the staging buffer is reused
}

std::string rank_file(const std::string& dir, int rank, int world) {
  return dir + "/rank-" + std::to_string(rank) + "-of-" + std::to_string(world) + ".ffck";
}

struct Manifest {
  int64_t epochs_done = 0, steps = 0, lr_host_steps = 0;
  std::string optimizer, table_optimizer, embedding_dtype, embedding_rounding, lr_route;
  int world_size = 1, rank = 0;
  std::vector<std::pair<std::string, std::string>> tables;      // (operator, placement)
  uint64_t digest = 0;
  // device learning-rate route: the schedule the blocks were initialised with (they carry it; see load_checkpoint)
  double lr_base = 0.0;
  int64_t lr_warmup = 0, lr_decay_start = 0, lr_decay_steps = 0;
};

std::string manifest_text(const Manifest& m, const std::vector<CkRecord>& recs) {
  std::ostringstream o;
  char buf[64];
  o << "ffck " << kVersion << "\n";
  o << "epochs_done " << m.epochs_done << "\nsteps " << m.steps << "\noptimizer " << m.optimizer << "\ntable_optimizer " << m.table_optimizer << "\n";
  o << "embedding_dtype " << m.embedding_dtype << "\nembedding_rounding " << m.embedding_rounding << "\n";
  o << "world_size " << m.world_size << "\nrank " << m.rank << "\nlr_route " << m.lr_route << "\nlr_host_steps " << m.lr_host_steps << "\n";
  if (m.lr_route == "device") {
    char sched[128];
    snprintf(sched, sizeof sched, "%.17g %lld %lld %lld", m.lr_base, (long long)m.lr_warmup, (long long)m.lr_decay_start, (long long)m.lr_decay_steps);
    o << "lr_schedule " << sched << "\n";
  }
  for (const auto& t : m.tables) o << "table " << t.first << " " << t.second << "\n";
  o << "records " << recs.size() << "\n";
  for (size_t k = 0; k < recs.size(); k++) {
    const CkRecord& r = recs[k];
    snprintf(buf, sizeof buf, "0x%016llx", (unsigned long long)r.digest);      // fixed width: the manifest's length does not depend on the digests
    o << "record " << k << " " << r.name << " " << r.type << " " << r.rows << " " << r.cols << " " << r.offset << " " << buf << "\n";
  }
  snprintf(buf, sizeof buf, "0x%016llx", (unsigned long long)m.digest);
  o << "digest " << buf << "\nend\n";
  return o.str();
}

Manifest describe(FFModel* ff, int64_t epochs_done) {
  Manifest m;
  m.epochs_done = epochs_done;
  m.steps = ff->n_update_calls;
  m.lr_host_steps = ff->lr_host_steps;
  m.optimizer = optimizer_kind(ff);
  m.table_optimizer = table_optimizer_kind(ff);
  m.embedding_dtype = ff->config.embedding_dtype == DT_BF16 ? "bf16" : "fp32";
  m.embedding_rounding = ff->config.embedding_rounding == FFH_BF16_ROUND_NEAREST ? "nearest" : "stochastic";
  m.world_size = std::max(1, ff->world_size);
  m.rank = ff->rank;
  m.lr_route = lr_route_name(ff->lr_route);
  m.lr_base = ff->lr_base; m.lr_warmup = ff->config.lr_warmup_steps; m.lr_decay_start = ff->config.lr_decay_start_step;
  m.lr_decay_steps = ff->config.lr_num_decay_steps;
  for (const Embedding* e : ff->embeddings) m.tables.push_back({e->name, placement_of(ff, e)});
  return m;
}

void write_all(FILE* f, const void* p, size_t n, const std::string& path) {
  if (n && fwrite(p, 1, n, f) != n) die("--save-checkpoint: writing %s failed: %s", path.c_str(), strerror(errno));
}

void make_dirs(const std::string& dir) {
  for (size_t k = 1; k <= dir.size(); k++)
    if (k == dir.size() || dir[k] == '/') {
      const std::string part = dir.substr(0, k);
      if (mkdir(part.c_str(), 0777) != 0 && errno != EEXIST) die("--save-checkpoint: cannot create %s: %s", part.c_str(), strerror(errno));
    }
}

}  // namespace

// =============================================================================================
FFModel::CheckpointInfo FFModel::save_checkpoint(const std::string& dir, int64_t epochs_done) {
  if (!compiled) die("save_checkpoint() before compile()");
  if (capturing_trace >= 0) die("save_checkpoint() inside begin_trace / end_trace");
  sync();
  make_dirs(dir);
  std::vector<CkRecord> recs = collect_records(this);
  Manifest m = describe(this, epochs_done);
  const std::string path = rank_file(dir, rank, m.world_size), tmp = path + ".tmp." + std::to_string((long long)getpid());
  const size_t header = 24 + manifest_text(m, recs).size();
  const size_t data_start = (header + kDataAlign - 1) / kDataAlign * kDataAlign;
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f) die("--save-checkpoint: cannot create %s: %s", tmp.c_str(), strerror(errno));
  std::vector<char> stage(kStageBytes);
  const std::vector<char> zeros(kRecordAlign, 0);
  uint64_t written = 0;
  for (size_t k = 0; k < recs.size(); k++) {
    CkRecord& r = recs[k];
    const uint64_t seed = ffh_digest_record_seed(k);
    if (fseeko(f, (off_t)(data_start + r.offset), SEEK_SET) != 0) die("--save-checkpoint: seek in %s failed: %s", tmp.c_str(), strerror(errno));
    if (r.on_host) {
      r.digest = ffh_state_digest_host(r.host.data(), r.rows, r.row_bytes(), r.row_bytes(), seed, 0);
      write_all(f, r.host.data(), r.host.size(), tmp);
    } else {
      const int64_t rb = r.row_bytes(), W = ffh_digest_row_words(rb);
      if ((size_t)rb > stage.size()) stage.resize((size_t)rb);
      const int64_t per = std::max<int64_t>(1, (int64_t)(stage.size() / (size_t)rb));
      uint64_t host_sum = 0;
      for (int64_t r0 = 0; r0 < r.rows; r0 += per) {
        const int64_t n = std::min(per, r.rows - r0);
        copy_rows(this, r, r0, n, stage.data(), false);
        if (!api->digest) host_sum += ffh_state_digest_host(stage.data(), n, rb, rb, seed, (uint64_t)r0 * (uint64_t)W);
        write_all(f, stage.data(), (size_t)(n * rb), tmp);
      }
      r.digest = api->digest ? device_digest(this, r, seed, false) : host_sum;
    }
    written += r.bytes();
    m.digest += r.digest;
  }
  // the header last, over the hole left for it: its length does not depend on the digests
  const std::string text = manifest_text(m, recs);
  if (24 + text.size() != header) die("checkpoint: the manifest changed its length");
  if (fseeko(f, 0, SEEK_SET) != 0) die("--save-checkpoint: seek in %s failed: %s", tmp.c_str(), strerror(errno));
  unsigned char head[24];
  memcpy(head, kMagic, 8);
  const uint32_t ver[2] = {kVersion, 0};
  memcpy(head + 8, ver, 8);
  const uint64_t len = text.size();
  memcpy(head + 16, &len, 8);
  write_all(f, head, sizeof head, tmp);
  write_all(f, text.data(), text.size(), tmp);
  // a file whose last record is empty or short of its alignment still has its full length
  uint64_t end = data_start;
  if (!recs.empty()) end = data_start + recs.back().offset + recs.back().bytes();
  if (fseeko(f, 0, SEEK_END) != 0 || (uint64_t)ftello(f) < end) {
    if (fseeko(f, (off_t)end - 1, SEEK_SET) != 0) die("--save-checkpoint: seek in %s failed: %s", tmp.c_str(), strerror(errno));
    write_all(f, zeros.data(), 1, tmp);
  }
  if (fflush(f) != 0 || fsync(fileno(f)) != 0 || fclose(f) != 0) die("--save-checkpoint: writing %s failed: %s", tmp.c_str(), strerror(errno));
  if (rename(tmp.c_str(), path.c_str()) != 0) die("--save-checkpoint: cannot rename %s to %s: %s", tmp.c_str(), path.c_str(), strerror(errno));
  CheckpointInfo info;
  info.epochs_done = epochs_done; info.steps = m.steps; info.digest = m.digest; info.bytes = (size_t)(end);
  (void)written;
  return info;
}

// =============================================================================================
namespace {

struct FileRecord { std::string name, type; int64_t rows = 0, cols = 0; uint64_t offset = 0, digest = 0; };

[[noreturn]] void refuse(const std::string& path, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "FATAL: --load-checkpoint %s: ", path.c_str());
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
  abort();
}

// the world size of the files in `dir` (0: none found)
int saved_world_size(const std::string& dir) {
  int found = 0;
  if (DIR* d = opendir(dir.c_str())) {
    while (const dirent* e = readdir(d)) {
      int r = 0, n = 0;
      char tail[8] = {0};
      if (sscanf(e->d_name, "rank-%d-of-%d.ffc%1s", &r, &n, tail) == 3 && !strcmp(tail, "k") && n > found) found = n;
    }
    closedir(d);
  }
  return found;
}

}  // namespace

FFModel::CheckpointInfo FFModel::load_checkpoint(const std::string& dir) {
  if (!compiled) die("load_checkpoint() before compile()");
  if (capturing_trace >= 0) die("load_checkpoint() inside begin_trace / end_trace");
  sync();
  const int world = std::max(1, world_size);
  const std::string path = rank_file(dir, rank, world);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) {
    const int saved = saved_world_size(dir);
    if (saved && saved != world)
      refuse(dir, "it was saved by %d rank%s and this run has %d; a checkpoint loads into the world size that saved it: launch %d rank%s", saved,
             saved == 1 ? "" : "s", world, saved, saved == 1 ? "" : "s");
    refuse(dir, "cannot open %s: %s (a checkpoint is the directory --save-checkpoint DIR wrote)", path.c_str(), strerror(errno));
  }
  struct stat st;
  if (fstat(fileno(f), &st) != 0) refuse(dir, "cannot stat %s: %s", path.c_str(), strerror(errno));
  const uint64_t file_size = (uint64_t)st.st_size;
  unsigned char head[24];
  if (fread(head, 1, sizeof head, f) != sizeof head) refuse(dir, "%s is truncated (shorter than its header); save it again", path.c_str());
  if (memcmp(head, kMagic, 8) != 0) refuse(dir, "%s is not a checkpoint file (wrong magic)", path.c_str());
  uint32_t version;
  uint64_t len;
  memcpy(&version, head + 8, 4);
  memcpy(&len, head + 16, 8);
  if (version != kVersion) refuse(dir, "%s has format version %u, this build reads version %u", path.c_str(), version, kVersion);
  if (24 + len > file_size) refuse(dir, "%s is truncated (its manifest is cut short); save it again", path.c_str());
  std::string text((size_t)len, '\0');
  if (fread(&text[0], 1, (size_t)len, f) != (size_t)len) refuse(dir, "%s is truncated (its manifest is cut short); save it again", path.c_str());
  const uint64_t data_start = (24 + len + kDataAlign - 1) / kDataAlign * kDataAlign;

  Manifest m;
  std::vector<FileRecord> frecs;
  bool ended = false, has_lr_schedule = false;
  {
    std::istringstream in(text);
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ls(line);
      std::string key;
      ls >> key;
      if (key == "ffck") continue;
      else if (key == "epochs_done") ls >> m.epochs_done;
      else if (key == "steps") ls >> m.steps;
      else if (key == "optimizer") ls >> m.optimizer;
      else if (key == "table_optimizer") ls >> m.table_optimizer;
      else if (key == "embedding_dtype") ls >> m.embedding_dtype;
      else if (key == "embedding_rounding") ls >> m.embedding_rounding;
      else if (key == "world_size") ls >> m.world_size;
      else if (key == "rank") ls >> m.rank;
      else if (key == "lr_route") ls >> m.lr_route;
      else if (key == "lr_host_steps") ls >> m.lr_host_steps;
      else if (key == "lr_schedule") {
        std::string base;
        ls >> base >> m.lr_warmup >> m.lr_decay_start >> m.lr_decay_steps;
        if (ls.fail()) refuse(dir, "%s has a malformed manifest line: %s", path.c_str(), line.c_str());
        m.lr_base = strtod(base.c_str(), nullptr);
        has_lr_schedule = true;
      }
      else if (key == "table") { std::string a, b; ls >> a >> b; m.tables.push_back({a, b}); }
      else if (key == "records") continue;
      else if (key == "record") {
        FileRecord r;
        size_t ordinal;
        std::string dg;
        ls >> ordinal >> r.name >> r.type >> r.rows >> r.cols >> r.offset >> dg;
        if (ls.fail() || ordinal != frecs.size()) refuse(dir, "%s has a malformed manifest line: %s", path.c_str(), line.c_str());
        r.digest = strtoull(dg.c_str(), nullptr, 16);
        frecs.push_back(r);
      } else if (key == "digest") { std::string dg; ls >> dg; m.digest = strtoull(dg.c_str(), nullptr, 16); }
      else if (key == "end") { ended = true; break; }
      else refuse(dir, "%s has an unknown manifest line: %s", path.c_str(), line.c_str());
    }
  }
  if (!ended) refuse(dir, "%s is truncated (its manifest has no end line); save it again", path.c_str());

  // ---- the run: what a checkpoint cannot be converted between ----
  const Manifest mine = describe(this, 0);
  if (m.world_size != mine.world_size || m.rank != mine.rank)
    refuse(dir, "%s was saved by rank %d of %d, this is rank %d of %d; a checkpoint loads into the world size that saved it: launch %d rank%s", path.c_str(),
           m.rank, m.world_size, mine.rank, mine.world_size, m.world_size, m.world_size == 1 ? "" : "s");
  if ((m.optimizer == "adagrad-rowwise" && mine.optimizer == "adagrad") || (m.optimizer == "adagrad" && mine.optimizer == "adagrad-rowwise"))
    refuse(dir, "it was saved %s --adagrad-rowwise, this run is %s it; an element-wise accumulator and a row-wise one do not convert: %s --adagrad-rowwise",
           m.optimizer == "adagrad" ? "without" : "with", m.optimizer == "adagrad" ? "with" : "without", m.optimizer == "adagrad" ? "drop" : "add");
  if (m.optimizer != mine.optimizer)
    refuse(dir, "it was saved with --optimizer %s, this run has --optimizer %s; the optimizer state does not convert: use --optimizer %s", m.optimizer.c_str(),
           mine.optimizer.c_str(), m.optimizer.c_str());
  if (m.table_optimizer != mine.table_optimizer)
    refuse(dir, "its tables were updated by the %s table optimizer, this run's by the %s one; %s --sparse-embedding-optimizer (and give --dense-embedding-update "
           "as the saving run did)", m.table_optimizer.c_str(), mine.table_optimizer.c_str(), m.table_optimizer == "sparse" ? "add" : "drop");
  if (m.embedding_dtype != mine.embedding_dtype)
    refuse(dir, "it holds %s tables, this run has --embedding-dtype %s; tables are not converted on load: use --embedding-dtype %s", m.embedding_dtype.c_str(),
           mine.embedding_dtype.c_str(), m.embedding_dtype.c_str());
  if ((m.lr_route == "device") != (mine.lr_route == "device"))
    refuse(dir, "it was saved on the %s learning-rate route, this run is on the %s route; %s", m.lr_route.c_str(), mine.lr_route.c_str(),
           m.lr_route == "device" ? "give the flags that put the rate in device memory (--device-lr, or the same --lr-num-* schedule without --host-lr-schedule)"
                                  : "drop --device-lr, or add --host-lr-schedule to a scheduled run");
  // the device route's blocks come back as the bytes they were and carry the schedule they were initialised with: the kernels would follow the
  // file's schedule whatever the command line says, so the two must be the same one
  if (mine.lr_route == "device") {
    if (!has_lr_schedule) refuse(dir, "%s is on the device learning-rate route and has no lr_schedule line: it is damaged; save it again", path.c_str());
    if (memcmp(&m.lr_base, &mine.lr_base, sizeof(double)) != 0 || m.lr_warmup != mine.lr_warmup || m.lr_decay_start != mine.lr_decay_start ||
        m.lr_decay_steps != mine.lr_decay_steps)
      refuse(dir, "it was saved under the schedule --lr %.17g --lr-num-warmup-steps %lld --lr-decay-start-step %lld --lr-num-decay-steps %lld and this "
             "run gives %.17g / %lld / %lld / %lld; on the device learning-rate route the blocks carry the schedule they were saved under: give the same "
             "--lr / --lr-num-warmup-steps / --lr-decay-start-step / --lr-num-decay-steps (or --host-lr-schedule in both runs to change it on resume)",
             m.lr_base, (long long)m.lr_warmup, (long long)m.lr_decay_start, (long long)m.lr_decay_steps, mine.lr_base, (long long)mine.lr_warmup,
             (long long)mine.lr_decay_start, (long long)mine.lr_decay_steps);
  }
  if (m.tables.size() == mine.tables.size())
    for (size_t t = 0; t < m.tables.size(); t++)
      if (m.tables[t].first == mine.tables[t].first && m.tables[t].second != mine.tables[t].second)
        refuse(dir, "table %s was placed %s when it was saved and is placed %s now; a checkpoint loads into the placement that saved it: give the same "
               "--row-shard-rows / --column-shard-rows / --replicate-embedding-rows / strategy file", m.tables[t].first.c_str(), m.tables[t].second.c_str(),
               mine.tables[t].second.c_str());

  // ---- the records: the file's and the model's must be the same set, of the same shapes ----
  std::vector<CkRecord> recs = collect_records(this);
  const char* shape_flags = "the model flags must be those of the saving run (--arch-mlp-bot, --arch-mlp-top, --arch-embedding-size, --arch-sparse-feature-size, "
                            "--arch-interaction-op, --dcn-*)";
  std::map<std::string, size_t> in_file;
  for (size_t k = 0; k < frecs.size(); k++) in_file[frecs[k].name] = k;
  std::vector<size_t> source(recs.size());
  std::set<std::string> wanted;
  for (size_t k = 0; k < recs.size(); k++) {
    const CkRecord& r = recs[k];
    wanted.insert(r.name);
    auto it = in_file.find(r.name);
    if (it == in_file.end()) refuse(dir, "the model has %s (%s [%lld][%lld]) and %s has no such record; %s", r.name.c_str(), r.type.c_str(), (long long)r.rows,
                                    (long long)r.cols, path.c_str(), shape_flags);
    const FileRecord& fr = frecs[it->second];
    if (fr.type != r.type) refuse(dir, "record %s holds %s elements, the model's are %s; %s", r.name.c_str(), fr.type.c_str(), r.type.c_str(), shape_flags);
    if (fr.rows != r.rows || fr.cols != r.cols)
      refuse(dir, "record %s is [%lld][%lld], the model's is [%lld][%lld]; %s", r.name.c_str(), (long long)fr.rows, (long long)fr.cols, (long long)r.rows,
             (long long)r.cols, shape_flags);
    if (data_start + fr.offset + r.bytes() > file_size)
      refuse(dir, "%s is truncated (record %s ends at byte %llu, the file has %llu); save it again", path.c_str(), r.name.c_str(),
             (unsigned long long)(data_start + fr.offset + r.bytes()), (unsigned long long)file_size);
    source[k] = it->second;
  }
  for (const FileRecord& fr : frecs)
    if (!wanted.count(fr.name)) refuse(dir, "%s has record %s ([%lld][%lld]) and the model has no such state; %s", path.c_str(), fr.name.c_str(), (long long)fr.rows,
                                       (long long)fr.cols, shape_flags);

  // ---- the copies, each verified against its digest ----
  std::vector<char> stage(kStageBytes);
  uint64_t fold = 0;
  for (size_t k = 0; k < recs.size(); k++) {
    CkRecord& r = recs[k];
    const FileRecord& fr = frecs[source[k]];
    const uint64_t seed = ffh_digest_record_seed(source[k]);
    if (fseeko(f, (off_t)(data_start + fr.offset), SEEK_SET) != 0) refuse(dir, "seek in %s failed: %s", path.c_str(), strerror(errno));
    const int64_t rb = r.row_bytes(), W = ffh_digest_row_words(rb);
    uint64_t got = 0;
    if (r.on_host) {
      if (fread(r.host.data(), 1, r.host.size(), f) != r.host.size()) refuse(dir, "%s is truncated inside record %s; save it again", path.c_str(), r.name.c_str());
      got = ffh_state_digest_host(r.host.data(), r.rows, rb, rb, seed, 0);
    } else {
      if ((size_t)rb > stage.size()) stage.resize((size_t)rb);
      const int64_t per = std::max<int64_t>(1, (int64_t)(stage.size() / (size_t)rb));
      for (int64_t r0 = 0; r0 < r.rows; r0 += per) {
        const int64_t n = std::min(per, r.rows - r0);
        if (fread(stage.data(), 1, (size_t)(n * rb), f) != (size_t)(n * rb))
          refuse(dir, "%s is truncated inside record %s; save it again", path.c_str(), r.name.c_str());
        if (!api->digest) got += ffh_state_digest_host(stage.data(), n, rb, rb, seed, (uint64_t)r0 * (uint64_t)W);
        copy_rows(this, r, r0, n, stage.data(), true);
      }
      if (r.zero_tail) check(api->ffh_zero(ctx, r.zero_tail, r.zero_tail_bytes, stream), "checkpoint: spare zero row");
      if (api->digest) got = device_digest(this, r, seed, false);      // of what the device now holds
    }
    if (got != fr.digest)
      refuse(dir, "record %s does not match its digest after the copy (file 0x%016llx, loaded 0x%016llx): %s is damaged; save it again", r.name.c_str(),
             (unsigned long long)fr.digest, (unsigned long long)got, path.c_str());
    fold += got;
    if (!r.on_host && r.name.compare(0, 6, "param/") == 0) note_weight_write(r.dev);
  }
  fclose(f);
  if (fold != m.digest) refuse(dir, "the records' digests do not add up to the manifest's (0x%016llx against 0x%016llx): %s is damaged; save it again",
                               (unsigned long long)fold, (unsigned long long)m.digest, path.c_str());

  // ---- host state ----
  for (const CkRecord& r : recs)
    if (r.name == "adam_scalars") {
      AdamOptimizer* adam = dynamic_cast<AdamOptimizer*>(optimizer);
      double s[3];
      memcpy(s, r.host.data(), sizeof s);
      adam->beta1_t = s[0]; adam->beta2_t = s[1]; adam->alpha_t = s[2];
    }
  n_update_calls = m.steps;
  if (lr_route == kLrHost) { lr_host_steps = m.lr_route == "host" ? m.lr_host_steps : m.steps; lr_host_set(lr_host_steps); }
  if (lr_route == kLrDevice) {
    // the blocks came back as the bytes they were, schedule included: the resuming command line must describe the same schedule
    ffh_lr_values v;
    check(api->lr->ffh_lr_state_read(ctx, lr_block[0], &v, stream), "lr_state_read");
    const float want = (float)ffh_lr_schedule_value(v.k, lr_base, config.lr_warmup_steps, config.lr_decay_start_step, config.lr_num_decay_steps);
    if (memcmp(&want, &v.lr, sizeof want) != 0)
      refuse(dir, "its learning-rate block stands at step %lld with rate %.9g, and this command line's schedule gives %.9g there; on the device route the block "
             "carries the schedule it was saved under: give the same --lr / --lr-num-warmup-steps / --lr-decay-start-step / --lr-num-decay-steps", (long long)v.k,
             (double)v.lr, (double)want);
  }
  sync();
  CheckpointInfo info;
  info.epochs_done = m.epochs_done; info.steps = m.steps; info.digest = m.digest; info.bytes = (size_t)file_size;
  return info;
}

// =============================================================================================
// The fold of every record's digest: what a checkpoint of this state would carry on its "digest" line.  On the device where the kernel
// library has the extension (one accumulator word, one launch per record, nothing copied out but that word), on the host otherwise.
uint64_t FFModel::state_digest() {
  if (!compiled) die("state_digest() before compile()");
  sync();
  std::vector<CkRecord> recs = collect_records(this);
  uint64_t fold = 0;
  std::vector<char> stage;
  bool any_device = false;
  if (api->digest) {
    if (!digest_acc) digest_acc = (uint64_t*)dmalloc(sizeof(uint64_t));
    check(api->ffh_zero(ctx, digest_acc, sizeof(uint64_t), stream), "digest accumulator");
  }
  for (size_t k = 0; k < recs.size(); k++) {
    const CkRecord& r = recs[k];
    const uint64_t seed = ffh_digest_record_seed(k);
    const int64_t rb = r.row_bytes(), W = ffh_digest_row_words(rb);
    if (r.on_host) { fold += ffh_state_digest_host(r.host.data(), r.rows, rb, rb, seed, 0); continue; }
    if (api->digest) { device_digest(this, r, seed, true); any_device = true; continue; }
    if (stage.empty()) stage.resize(kStageBytes);
    if ((size_t)rb > stage.size()) stage.resize((size_t)rb);
    const int64_t per = std::max<int64_t>(1, (int64_t)(stage.size() / (size_t)rb));
    for (int64_t r0 = 0; r0 < r.rows; r0 += per) {
      const int64_t n = std::min(per, r.rows - r0);
      copy_rows(this, r, r0, n, stage.data(), false);
      fold += ffh_state_digest_host(stage.data(), n, rb, rb, seed, (uint64_t)r0 * (uint64_t)W);
    }
  }
  if (any_device) {
    uint64_t v = 0;
    check(api->ffh_memcpy_d2h(ctx, &v, digest_acc, sizeof v, stream), "digest d2h");
    check(api->ffh_stream_sync(ctx, stream), "digest sync");
    fold += v;
  }
  return fold;
}
