// embedding_update_bags_f32.hip -- the ragged table update's apply kernels on fp32 weight rows (emb_bags_update.h), the ragged sort's kernels (they
// read no weights: one copy, here) and the launchers embedding.hip reaches them through
#include "emb_bags_update.h"

namespace ffh_emb {

bool emb_bags_update_launch_f32(const BagsUpdateLaunch& u) { return emb_bags_update_launch<float, false>(u, std::make_integer_sequence<int, kUpdateEntries>()); }

namespace {
template <bool FIRST, int E> void bags_sort_pass(const BagsSortArgs& a, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL((bags_radix_hist_kernel<FIRST, E>), grid, dim3(kSortThreads), 0, stream, a);
  hipLaunchKernelGGL((bags_radix_scatter_kernel<FIRST, E>), grid, dim3(kSortThreads), 0, stream, a);
}
}  // namespace

bool emb_bags_sort_pass(const BagsSortArgs& a, bool first, int E, dim3 grid, hipStream_t stream) {
  switch (E) {
    case 1: first ? bags_sort_pass<true, 1>(a, grid, stream) : bags_sort_pass<false, 1>(a, grid, stream); return true;
    case 2: first ? bags_sort_pass<true, 2>(a, grid, stream) : bags_sort_pass<false, 2>(a, grid, stream); return true;
    case 4: first ? bags_sort_pass<true, 4>(a, grid, stream) : bags_sort_pass<false, 4>(a, grid, stream); return true;
    case 8: first ? bags_sort_pass<true, 8>(a, grid, stream) : bags_sort_pass<false, 8>(a, grid, stream); return true;
  }
  return false;
}

}  // namespace ffh_emb
