// embedding_pad.hip -- include/ff_hip_pad.h: variable-length embedding bags, "no lookup" being the id FFH_EMB_PAD_ID.
// What is here: the extension's version and ffh_pad_mask_indices, the generator of synthetic pads.
// What is where: the pad gather is the PAD form of emb_fwd_bags_kernel (embedding_fwd.hip); the pad update is emb_bwd_bags with `pad` set
// (embedding.hip) on the PAD forms of the ragged kernels (emb_bags_update.h; embedding_update_pad_f32.hip / _bf16.hip).
#include "ffh_common.h"
#include "../../include/ff_hip_pad.h"
#include "../../include/ffh_rng.h"

namespace {

// idx[i] stays where element first + i of stream `seed` falls below `fill`; one 8-byte load and at most one 8-byte store per lane, lanes
// contiguous, grid-stride like the other generators (runtime.hip)
__global__ __launch_bounds__(256) void pad_mask_kernel(int64_t* __restrict__ idx, int64_t n, uint64_t seed, int64_t first, float fill) {
  ffh_kernel_prio();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    if (!(ffh_u24(ffh_hash(seed, (uint64_t)(first + i))) < fill)) idx[i] = FFH_EMB_PAD_ID;
}

}  // namespace

extern "C" {

int ffh_pad_abi_version(void) { return FFH_PAD_ABI_VERSION; }

int ffh_pad_mask_indices(ffh_ctx* c, int64_t* idx, int64_t count, uint64_t seed, int64_t first, float fill, ffh_stream s) {
  FFH_REQUIRE(c, count >= 0 && first >= 0 && (idx || count == 0) && fill == fill, "pad_mask_indices: bad args");
  if (count == 0 || fill >= 1.0f) return FFH_OK;      // (u24 < 1 always: nothing to mask)
  hipLaunchKernelGGL(pad_mask_kernel, dim3(ffh_grid(count, 256)), dim3(256), 0, as_stream(s), idx, count, seed, first, fill);
  FFH_LAUNCH_CHECK(c, "pad_mask_indices");
  return FFH_OK;
}

}  // extern "C"
