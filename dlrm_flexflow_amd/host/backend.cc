#include "backend.h"

#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

// FFH_BACKEND_LIB points the driver at another library exporting include/ff_hip.h (the CPU oracle in tests, an A/B build).  It is
// the one environment variable this layer reads, so it is never silent: load_kernel_api() says on stderr which library an
// override selected, and the driver names the kernel library on its THROUGHPUT line whenever it is not the product's own
// (KernelApi::overridden).
static bool g_env_override = false;
std::string default_backend_path() {
  if (const char* e = getenv("FFH_BACKEND_LIB")) { g_env_override = true; return std::string(e); }
  Dl_info info;
  std::string dir = ".";
  if (dladdr((void*)&default_backend_path, &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    size_t k = p.rfind('/');
    if (k != std::string::npos) dir = p.substr(0, k);
  }
  return dir + "/../csrc/libffhip.so";
}

const KernelApi* load_kernel_api(const std::string& path_in) {
  static std::map<std::string, KernelApi*>& cache = *new std::map<std::string, KernelApi*>();   // one table per library for the life of the process
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  const std::string path = path_in.empty() ? default_backend_path() : path_in;
  auto it = cache.find(path);
  if (it != cache.end()) return it->second;
  void* h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
  if (!h) {
    fprintf(stderr, "FATAL: cannot load kernel library %s: %s\n"
                    "       build it with: python -c 'import __graft_entry__ as g; g.build()'\n", path.c_str(), dlerror());
    abort();
  }
  KernelApi* api = new KernelApi();
  api->handle = h;
  api->path = path;
  api->overridden = !path_in.empty() || g_env_override;
#define FFH_LOAD(name)                                                        \
  api->name = reinterpret_cast<decltype(api->name)>(dlsym(h, #name));         \
  if (!api->name) {                                                           \
    fprintf(stderr, "FATAL: %s does not export %s\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
  FFH_API_LIST(FFH_LOAD)
#undef FFH_LOAD
  if (api->ffh_abi_version() != FFH_ABI_VERSION) {
    fprintf(stderr, "FATAL: %s has ABI version %d, expected %d\n", path.c_str(), api->ffh_abi_version(), FFH_ABI_VERSION);
    abort();
  }
  // the bf16-table extension: absent is fine (the library loads as before), present means complete and of this version
  if (dlsym(h, "ffh_bf16_abi_version")) {
    KernelApiBf16* b = new KernelApiBf16();
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name) {                                                             \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_bf16.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_BF16_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_bf16_abi_version() != FFH_BF16_ABI_VERSION) {
      fprintf(stderr, "FATAL: %s has bf16 ABI version %d, expected %d\n", path.c_str(), b->ffh_bf16_abi_version(), FFH_BF16_ABI_VERSION);
      abort();
    }
    api->bf16 = b;
  }
  // the CTR extension (include/ff_hip_ctr.h): the same rule
  if (dlsym(h, "ffh_ctr_abi_version")) {
    KernelApiCtr* b = new KernelApiCtr();
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name) {                                                             \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_ctr.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_CTR_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_ctr_abi_version() != FFH_CTR_ABI_VERSION) {
      fprintf(stderr, "FATAL: %s has CTR ABI version %d, expected %d\n", path.c_str(), b->ffh_ctr_abi_version(), FFH_CTR_ABI_VERSION);
      abort();
    }
    api->ctr = b;
  }
  // the learning-rate extension (include/ff_hip_lr.h): the same rule
  if (dlsym(h, "ffh_lr_abi_version")) {
    KernelApiLr* b = new KernelApiLr();
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name) {                                                             \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_lr.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_LR_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_lr_abi_version() != FFH_LR_ABI_VERSION) {
      fprintf(stderr, "FATAL: %s has learning-rate ABI version %d, expected %d\n", path.c_str(), b->ffh_lr_abi_version(), FFH_LR_ABI_VERSION);
      abort();
    }
    api->lr = b;
  }
  // the data extension (include/ff_hip_data.h): the same rule
  if (dlsym(h, "ffh_data_abi_version")) {
    KernelApiData* b = new KernelApiData();
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name) {                                                             \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_data.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_DATA_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_data_abi_version() != FFH_DATA_ABI_VERSION) {
      fprintf(stderr, "FATAL: %s has data ABI version %d, expected %d\n", path.c_str(), b->ffh_data_abi_version(), FFH_DATA_ABI_VERSION);
      abort();
    }
    api->data = b;
  }
  // the cross extension (include/ff_hip_cross.h): the same rule
  if (dlsym(h, "ffh_cross_abi_version")) {
    KernelApiCross* b = new KernelApiCross();
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name) {                                                             \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_cross.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_CROSS_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_cross_abi_version() != FFH_CROSS_ABI_VERSION) {
      fprintf(stderr, "FATAL: %s has cross ABI version %d, expected %d\n", path.c_str(), b->ffh_cross_abi_version(), FFH_CROSS_ABI_VERSION);
      abort();
    }
    api->cross = b;
  }
  // the digest extension (include/ff_hip_digest.h): the same rule
  if (dlsym(h, "ffh_digest_abi_version")) {
    KernelApiDigest* b = new KernelApiDigest();
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name) {                                                             \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_digest.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_DIGEST_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_digest_abi_version() != FFH_DIGEST_ABI_VERSION) {
      fprintf(stderr, "FATAL: %s has digest ABI version %d, expected %d\n", path.c_str(), b->ffh_digest_abi_version(), FFH_DIGEST_ABI_VERSION);
      abort();
    }
    api->digest = b;
  }
  // the Adagrad extension (include/ff_hip_adagrad.h): the same rule
  if (dlsym(h, "ffh_adagrad_abi_version")) {
    KernelApiAdagrad* b = new KernelApiAdagrad();
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name) {                                                             \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_adagrad.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_ADAGRAD_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_adagrad_abi_version() != FFH_ADAGRAD_ABI_VERSION) {
      fprintf(stderr, "FATAL: %s has Adagrad ABI version %d, expected %d\n", path.c_str(), b->ffh_adagrad_abi_version(), FFH_ADAGRAD_ABI_VERSION);
      abort();
    }
    api->adagrad = b;
  }
  // the row-wise Adagrad extension (include/ff_hip_rowwise.h): the same rule
  if (dlsym(h, "ffh_rowwise_abi_version")) {
    KernelApiRowwise* b = new KernelApiRowwise();
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name) {                                                             \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_rowwise.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_ROWWISE_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_rowwise_abi_version() != FFH_ROWWISE_ABI_VERSION) {
      fprintf(stderr, "FATAL: %s has row-wise Adagrad ABI version %d, expected %d\n", path.c_str(), b->ffh_rowwise_abi_version(), FFH_ROWWISE_ABI_VERSION);
      abort();
    }
    api->rowwise = b;
  }
  // the fold extension (include/ff_hip_fold.h): the same rule
  // ... except that a library of ABI 2 is taken as it is: the entries ABI 3 added (the data-gradient half) stay null and that half of the route is off
  if (dlsym(h, "ffh_fold_abi_version")) {
    KernelApiFold* b = new KernelApiFold();
    const int fold_abi = reinterpret_cast<int (*)(void)>(dlsym(h, "ffh_fold_abi_version"))();
    auto abi3_entry = [](const char* n) { return !strncmp(n, "ffh_fold_linear_bwd_dx", 22) || !strncmp(n, "ffh_fold_table_update", 21); };
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name && !(fold_abi == 2 && abi3_entry(#name))) {                    \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_fold.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_FOLD_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_fold_abi_version() != FFH_FOLD_ABI_VERSION && fold_abi != 2) {
      fprintf(stderr, "FATAL: %s has fold ABI version %d, expected %d\n", path.c_str(), b->ffh_fold_abi_version(), FFH_FOLD_ABI_VERSION);
      abort();
    }
    api->fold = b;
  }
  // the bags extension (include/ff_hip_bags.h): the same rule
  if (dlsym(h, "ffh_bags_abi_version")) {
    KernelApiBags* b = new KernelApiBags();
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name) {                                                             \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_bags.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_BAGS_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_bags_abi_version() != FFH_BAGS_ABI_VERSION) {
      fprintf(stderr, "FATAL: %s has bags ABI version %d, expected %d\n", path.c_str(), b->ffh_bags_abi_version(), FFH_BAGS_ABI_VERSION);
      abort();
    }
    api->bags = b;
  }
  // the bags-update extension (include/ff_hip_bags_update.h): the same rule
  if (dlsym(h, "ffh_bags_update_abi_version")) {
    KernelApiBagsUpdate* b = new KernelApiBagsUpdate();
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name) {                                                             \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_bags_update.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_BAGS_UPDATE_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_bags_update_abi_version() != FFH_BAGS_UPDATE_ABI_VERSION) {
      fprintf(stderr, "FATAL: %s has bags-update ABI version %d, expected %d\n", path.c_str(), b->ffh_bags_update_abi_version(), FFH_BAGS_UPDATE_ABI_VERSION);
      abort();
    }
    api->bags_update = b;
  }
  // the bags-sort extension (include/ff_hip_bags_sort.h): the same rule
  if (dlsym(h, "ffh_bags_sort_abi_version")) {
    KernelApiBagsSort* b = new KernelApiBagsSort();
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name) {                                                             \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_bags_sort.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_BAGS_SORT_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_bags_sort_abi_version() != FFH_BAGS_SORT_ABI_VERSION) {
      fprintf(stderr, "FATAL: %s has bags-sort ABI version %d, expected %d\n", path.c_str(), b->ffh_bags_sort_abi_version(), FFH_BAGS_SORT_ABI_VERSION);
      abort();
    }
    api->bags_sort = b;
  }
  // the pad extension (include/ff_hip_pad.h): the same rule
  if (dlsym(h, "ffh_pad_abi_version")) {
    KernelApiPad* b = new KernelApiPad();
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name) {                                                             \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_pad.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_PAD_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_pad_abi_version() != FFH_PAD_ABI_VERSION) {
      fprintf(stderr, "FATAL: %s has pad ABI version %d, expected %d\n", path.c_str(), b->ffh_pad_abi_version(), FFH_PAD_ABI_VERSION);
      abort();
    }
    api->pad = b;
  }
  // the pad-mean extension (include/ff_hip_pad_mean.h): the same rule
  if (dlsym(h, "ffh_pad_mean_abi_version")) {
    KernelApiPadMean* b = new KernelApiPadMean();
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name) {                                                             \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_pad_mean.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_PAD_MEAN_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_pad_mean_abi_version() != FFH_PAD_MEAN_ABI_VERSION) {
      fprintf(stderr, "FATAL: %s has pad-mean ABI version %d, expected %d\n", path.c_str(), b->ffh_pad_mean_abi_version(), FFH_PAD_MEAN_ABI_VERSION);
      abort();
    }
    api->pad_mean = b;
  }
  // the q8 extension (include/ff_hip_q8.h): the same rule
  if (dlsym(h, "ffh_q8_abi_version")) {
    KernelApiQ8* b = new KernelApiQ8();
#define FFH_LOAD(name)                                                        \
  b->name = reinterpret_cast<decltype(b->name)>(dlsym(h, #name));             \
  if (!b->name) {                                                             \
    fprintf(stderr, "FATAL: %s exports part of include/ff_hip_q8.h: %s is missing\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
    FFH_Q8_API_LIST(FFH_LOAD)
#undef FFH_LOAD
    if (b->ffh_q8_abi_version() != FFH_Q8_ABI_VERSION) {
      fprintf(stderr, "FATAL: %s has q8 ABI version %d, expected %d\n", path.c_str(), b->ffh_q8_abi_version(), FFH_Q8_ABI_VERSION);
      abort();
    }
    api->q8 = b;
  }
  if (path_in.empty() && g_env_override)
    fprintf(stderr, "[DLRM] FFH_BACKEND_LIB: kernel library %s (%s)\n", path.c_str(), api->ffh_backend_name());
  cache[path] = api;
  return api;
}
