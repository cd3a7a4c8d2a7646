// backend.h -- dlopen loader for a library exporting the kernel C-ABI (include/ff_hip.h).
// The product default is libffhip.so (hand-written gfx950 HIP); loading fails loudly if it is
// missing or incomplete -- there is no CPU fallback in this layer.
#pragma once
#include <string>
#include "../../include/ff_hip.h"
#include "../../include/ff_hip_bf16.h"
#include "../../include/ff_hip_ctr.h"
#include "../../include/ff_hip_lr.h"
#include "../../include/ff_hip_data.h"
#include "../../include/ff_hip_cross.h"
#include "../../include/ff_hip_digest.h"
#include "../../include/ff_hip_adagrad.h"
#include "../../include/ff_hip_rowwise.h"
#include "../../include/ff_hip_fold.h"
#include "../../include/ff_hip_bags.h"
#include "../../include/ff_hip_bags_update.h"
#include "../../include/ff_hip_bags_sort.h"
#include "../../include/ff_hip_pad.h"
#include "../../include/ff_hip_pad_mean.h"
#include "../../include/ff_hip_q8.h"

// The optional bf16-table extension (include/ff_hip_bf16.h): all of its list or none of it.
struct KernelApiBf16 {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_BF16_API_LIST(FFH_DECL)
#undef FFH_DECL
};

// The optional CTR extension (include/ff_hip_ctr.h: binary cross-entropy, evaluation histograms): all of its list or none of it.
struct KernelApiCtr {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_CTR_API_LIST(FFH_DECL)
#undef FFH_DECL
};

// The optional learning-rate extension (include/ff_hip_lr.h: the state block in device memory and the optimizer entries that read it).
struct KernelApiLr {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_LR_API_LIST(FFH_DECL)
#undef FFH_DECL
};

// The optional data extension (include/ff_hip_data.h: one shuffled training batch gathered in one launch).
struct KernelApiData {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_DATA_API_LIST(FFH_DECL)
#undef FFH_DECL
};

// The optional cross extension (include/ff_hip_cross.h: the elementwise combine of a DCNv2 low-rank cross layer and its backward).
struct KernelApiCross {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_CROSS_API_LIST(FFH_DECL)
#undef FFH_DECL
};

// The optional digest extension (include/ff_hip_digest.h: a 64-bit digest of a strided device buffer).
struct KernelApiDigest {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_DIGEST_API_LIST(FFH_DECL)
#undef FFH_DECL
};

// The optional Adagrad extension (include/ff_hip_adagrad.h: the dense launch; the library then also takes FFH_SPARSE_OPT_ADAGRAD in the table update).
struct KernelApiAdagrad {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_ADAGRAD_API_LIST(FFH_DECL)
#undef FFH_DECL
};

// The optional row-wise Adagrad extension (include/ff_hip_rowwise.h: the library takes FFH_SPARSE_OPT_ROWWISE_ADAGRAD in the table update).
struct KernelApiRowwise {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_ROWWISE_API_LIST(FFH_DECL)
#undef FFH_DECL
};

// The optional fold extension (include/ff_hip_fold.h: small embedding tables folded out of the first top layer's forward GEMM).
struct KernelApiFold {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_FOLD_API_LIST(FFH_DECL)
#undef FFH_DECL
};

// The optional bags extension (include/ff_hip_bags.h: the embedding gather with a bag size per table, one launch).
struct KernelApiBags {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_BAGS_API_LIST(FFH_DECL)
#undef FFH_DECL
};

// The optional bags-update extension (include/ff_hip_bags_update.h: the fused table update with a bag size per table, one call).
struct KernelApiBagsUpdate {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_BAGS_UPDATE_API_LIST(FFH_DECL)
#undef FFH_DECL
};

// The optional bags-sort extension (include/ff_hip_bags_sort.h: the ragged update's sort call and apply call).
struct KernelApiBagsSort {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_BAGS_SORT_API_LIST(FFH_DECL)
#undef FFH_DECL
};

// The optional pad extension (include/ff_hip_pad.h: variable-length bags, the id -1 being "no lookup").
struct KernelApiPad {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_PAD_API_LIST(FFH_DECL)
#undef FFH_DECL
};

// The optional pad-mean extension (include/ff_hip_pad_mean.h: the pad entries' mean forms, the divisor being a bag's count of real lookups).
struct KernelApiPadMean {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_PAD_MEAN_API_LIST(FFH_DECL)
#undef FFH_DECL
};

// The optional q8 extension (include/ff_hip_q8.h: tables as 8-bit rows for held-out evaluation, their quantizer and gathers).
struct KernelApiQ8 {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_Q8_API_LIST(FFH_DECL)
#undef FFH_DECL
};

struct KernelApi {
#define FFH_DECL(name) decltype(&::name) name;
  FFH_API_LIST(FFH_DECL)
#undef FFH_DECL
  const KernelApiBf16* bf16 = nullptr;   // null: the library does not export the extension (e.g. the CPU oracle)
  const KernelApiCtr* ctr = nullptr;     // likewise for include/ff_hip_ctr.h
  const KernelApiLr* lr = nullptr;       // likewise for include/ff_hip_lr.h
  const KernelApiData* data = nullptr;   // likewise for include/ff_hip_data.h
  const KernelApiCross* cross = nullptr; // likewise for include/ff_hip_cross.h
  const KernelApiDigest* digest = nullptr;   // likewise for include/ff_hip_digest.h (absent: the host layer computes the same digest from the bytes it copies)
  const KernelApiAdagrad* adagrad = nullptr; // likewise for include/ff_hip_adagrad.h
  const KernelApiRowwise* rowwise = nullptr; // likewise for include/ff_hip_rowwise.h
  const KernelApiFold* fold = nullptr;       // likewise for include/ff_hip_fold.h (absent: no table is folded, the step is the one of before)
  const KernelApiBags* bags = nullptr;       // likewise for include/ff_hip_bags.h (absent: a model of mixed bag sizes gathers once per bag size)
  const KernelApiBagsUpdate* bags_update = nullptr;   // likewise for include/ff_hip_bags_update.h (absent: a model of mixed bag sizes updates once per bag size)
  const KernelApiBagsSort* bags_sort = nullptr;       // likewise for include/ff_hip_bags_sort.h (absent: a model of mixed bag sizes sorts in front of its apply)
  const KernelApiPad* pad = nullptr;                  // likewise for include/ff_hip_pad.h (absent: compile() refuses --embedding-padding)
  const KernelApiPadMean* pad_mean = nullptr;         // likewise for include/ff_hip_pad_mean.h (absent: compile() refuses AGGR_MODE_AVG on a padded table)
  const KernelApiQ8* q8 = nullptr;                    // likewise for include/ff_hip_q8.h (absent: compile() refuses --eval-embedding-dtype int8)
  void* handle;
  std::string path;
  bool overridden = false;      // chosen by --backend or $FFH_BACKEND_LIB rather than the product default: the driver says so on its THROUGHPUT line
};

// Loads `path` (or, when empty, $FFH_BACKEND_LIB, else csrc/libffhip.so next to this library).
// Aborts with a message naming the missing file/symbol.
const KernelApi* load_kernel_api(const std::string& path);
std::string default_backend_path();
