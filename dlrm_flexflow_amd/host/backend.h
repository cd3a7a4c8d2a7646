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

// The optional extensions of the kernel C-ABI, one line each, in the order load_kernel_api() loads them:
//   X(KernelApi field, struct, the header's list, version symbol, the header's version, label of the version message, header under include/
//     [, an older ABI version that is still accepted, {prefixes of the entries a library of that version may lack: they stay null}])
// The rule is the same for all of them (load_extension in backend.cc): absent is fine and leaves the field null; present means all of the
// list and this version.  The structs, the fields of KernelApi and the loads all come from this list: a new extension is one line here.
#define FFH_EXTENSIONS(X)                                                                                                                        \
  /* bf16 tables (absent, as on the CPU oracle: fp32 tables only) */                                                                             \
  X(bf16, KernelApiBf16, FFH_BF16_API_LIST, ffh_bf16_abi_version, FFH_BF16_ABI_VERSION, "bf16", "ff_hip_bf16.h")                                 \
  /* binary cross-entropy, evaluation histograms */                                                                                              \
  X(ctr, KernelApiCtr, FFH_CTR_API_LIST, ffh_ctr_abi_version, FFH_CTR_ABI_VERSION, "CTR", "ff_hip_ctr.h")                                        \
  /* the learning-rate state block in device memory and the optimizer entries that read it */                                                    \
  X(lr, KernelApiLr, FFH_LR_API_LIST, ffh_lr_abi_version, FFH_LR_ABI_VERSION, "learning-rate", "ff_hip_lr.h")                                    \
  /* one shuffled training batch gathered in one launch */                                                                                       \
  X(data, KernelApiData, FFH_DATA_API_LIST, ffh_data_abi_version, FFH_DATA_ABI_VERSION, "data", "ff_hip_data.h")                                 \
  /* the elementwise combine of a DCNv2 low-rank cross layer and its backward */                                                                 \
  X(cross, KernelApiCross, FFH_CROSS_API_LIST, ffh_cross_abi_version, FFH_CROSS_ABI_VERSION, "cross", "ff_hip_cross.h")                          \
  /* a 64-bit digest of a strided device buffer (absent: the host layer computes the same digest from the bytes it copies) */                    \
  X(digest, KernelApiDigest, FFH_DIGEST_API_LIST, ffh_digest_abi_version, FFH_DIGEST_ABI_VERSION, "digest", "ff_hip_digest.h")                   \
  /* the dense Adagrad launch; the library then also takes FFH_SPARSE_OPT_ADAGRAD in the table update */                                         \
  X(adagrad, KernelApiAdagrad, FFH_ADAGRAD_API_LIST, ffh_adagrad_abi_version, FFH_ADAGRAD_ABI_VERSION, "Adagrad", "ff_hip_adagrad.h")            \
  /* the library takes FFH_SPARSE_OPT_ROWWISE_ADAGRAD in the table update */                                                                     \
  X(rowwise, KernelApiRowwise, FFH_ROWWISE_API_LIST, ffh_rowwise_abi_version, FFH_ROWWISE_ABI_VERSION, "row-wise Adagrad", "ff_hip_rowwise.h")   \
  /* small embedding tables folded out of the first top layer's GEMMs (absent: no table is folded, the step is the one of before).  A library   \
     of ABI 2 is taken as it is: the entries ABI 3 added (the data-gradient half) stay null and that half of the route is off */                 \
  X(fold, KernelApiFold, FFH_FOLD_API_LIST, ffh_fold_abi_version, FFH_FOLD_ABI_VERSION, "fold", "ff_hip_fold.h", 2, {"ffh_fold_linear_bwd_dx", "ffh_fold_table_update"}) \
  /* the embedding gather with a bag size per table, one launch (absent: a model of mixed bag sizes gathers once per bag size) */                \
  X(bags, KernelApiBags, FFH_BAGS_API_LIST, ffh_bags_abi_version, FFH_BAGS_ABI_VERSION, "bags", "ff_hip_bags.h")                                 \
  /* the fused table update with a bag size per table, one call (absent: a model of mixed bag sizes updates once per bag size) */                \
  X(bags_update, KernelApiBagsUpdate, FFH_BAGS_UPDATE_API_LIST, ffh_bags_update_abi_version, FFH_BAGS_UPDATE_ABI_VERSION, "bags-update", "ff_hip_bags_update.h") \
  /* the ragged update's sort call and apply call (absent: a model of mixed bag sizes sorts in front of its apply) */                            \
  X(bags_sort, KernelApiBagsSort, FFH_BAGS_SORT_API_LIST, ffh_bags_sort_abi_version, FFH_BAGS_SORT_ABI_VERSION, "bags-sort", "ff_hip_bags_sort.h")  \
  /* variable-length bags, the id -1 being "no lookup" (absent: compile() refuses --embedding-padding) */                                        \
  X(pad, KernelApiPad, FFH_PAD_API_LIST, ffh_pad_abi_version, FFH_PAD_ABI_VERSION, "pad", "ff_hip_pad.h")                                        \
  /* the pad entries' mean forms, the divisor being a bag's count of real lookups (absent: compile() refuses AGGR_MODE_AVG on a padded table) */ \
  X(pad_mean, KernelApiPadMean, FFH_PAD_MEAN_API_LIST, ffh_pad_mean_abi_version, FFH_PAD_MEAN_ABI_VERSION, "pad-mean", "ff_hip_pad_mean.h")      \
  /* tables as 8-bit rows for held-out evaluation, their quantizer and gathers (absent: compile() refuses --eval-embedding-dtype int8) */        \
  X(q8, KernelApiQ8, FFH_Q8_API_LIST, ffh_q8_abi_version, FFH_Q8_ABI_VERSION, "q8", "ff_hip_q8.h")

#define FFH_DECL(name) decltype(&::name) name;

// struct KernelApi<X>: one typed function pointer per entry of the extension's list
#define FFH_DECL_STRUCT(field, Struct, LIST, ...) struct Struct { LIST(FFH_DECL) };
FFH_EXTENSIONS(FFH_DECL_STRUCT)
#undef FFH_DECL_STRUCT

struct KernelApi {
  FFH_API_LIST(FFH_DECL)
  // const KernelApi<X>* <field> = nullptr; null: the library does not export the extension (e.g. the CPU oracle)
#define FFH_DECL_FIELD(field, Struct, ...) const Struct* field = nullptr;
  FFH_EXTENSIONS(FFH_DECL_FIELD)
#undef FFH_DECL_FIELD
  void* handle;
  std::string path;
  bool overridden = false;      // chosen by --backend or $FFH_BACKEND_LIB rather than the product default: the driver says so on its THROUGHPUT line
};
#undef FFH_DECL

// Loads `path` (or, when empty, $FFH_BACKEND_LIB, else csrc/libffhip.so next to this library).
// Aborts with a message naming the missing file/symbol.
const KernelApi* load_kernel_api(const std::string& path);
std::string default_backend_path();
