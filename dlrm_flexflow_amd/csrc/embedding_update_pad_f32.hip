// embedding_update_pad_f32.hip -- the pad forms (include/ff_hip_pad.h) of the ragged table update's apply kernels on fp32 weight rows
// (emb_bags_update.h, PAD = true), pass 0 of the ragged sort in its pad form (it reads no weights: one copy, here) and the launchers
// embedding.hip reaches them through
#include "emb_bags_update.h"

namespace ffh_emb {

bool emb_pad_update_launch_f32(const BagsUpdateLaunch& u) { return emb_bags_update_launch<float, true>(u, std::make_integer_sequence<int, kUpdateEntries>()); }

namespace {
template <int E> void pad_sort_first_pass(const BagsSortArgs& a, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL((bags_radix_hist_kernel<true, E, true>), grid, dim3(kSortThreads), 0, stream, a);
  hipLaunchKernelGGL((bags_radix_scatter_kernel<true, E, true>), grid, dim3(kSortThreads), 0, stream, a);
}
}  // namespace

bool emb_pad_sort_first_pass(const BagsSortArgs& a, int E, dim3 grid, hipStream_t stream) {
  switch (E) {
    case 1: pad_sort_first_pass<1>(a, grid, stream); return true;
    case 2: pad_sort_first_pass<2>(a, grid, stream); return true;
    case 4: pad_sort_first_pass<4>(a, grid, stream); return true;
    case 8: pad_sort_first_pass<8>(a, grid, stream); return true;
  }
  return false;
}

}  // namespace ffh_emb
