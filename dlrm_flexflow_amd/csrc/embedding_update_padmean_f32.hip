// embedding_update_padmean_f32.hip -- the mean forms (include/ff_hip_pad_mean.h) of the ragged table update's apply kernels on fp32 weight rows
// (emb_bags_update.h, PAD = MEAN = true), the kernel that counts every bag's real lookups for them (it reads no weights: one copy, here) and the
// launchers embedding.hip reaches them through
#include "emb_bags_update.h"

namespace ffh_emb {

bool emb_padmean_update_launch_f32(const BagsUpdateLaunch& u) { return emb_bags_update_launch<float, true, true>(u, std::make_integer_sequence<int, kUpdateEntries>()); }

namespace {

// cnt[t][b] = ids >= 0 in bag b of table t.  A FLAT grid without a cap and without a grid-stride loop, like the ragged sort's map: table t owns
// count_wgs(batch, L_t) consecutive workgroups, each a whole number of consecutive bags (count_bags_per_wg: at most kCountSlots id slots, or one
// bag that is longer), so no bag is shared between workgroups and every count is written exactly once.  The threads walk the workgroup's id
// slots contiguously (one 8-byte load per lane) and count into LDS; a 16-bit count holds every bag size (<= 65535).
__global__ __launch_bounds__(kCountThreads) void bags_count_kernel(const BagsCountArgs a) {
  ffh_kernel_prio();
  __shared__ uint32_t s_cnt[kCountSlots];
  int t = 0;
  int64_t local = blockIdx.x;
  for (; t < a.nt; t++) {      // workgroup -> (table, first bag): block-uniform
    const int64_t w = count_wgs(a.batch, a.L[t]);
    if (local < w) break;
    local -= w;
  }
  if (t >= a.nt) return;
  const int L = a.L[t];
  const int bpw = count_bags_per_wg(L);
  const int64_t b0 = local * bpw;
  const int nb = (int)(a.batch - b0 < bpw ? a.batch - b0 : bpw);      // >= 1: local < count_wgs
  for (int i = threadIdx.x; i < nb; i += kCountThreads) s_cnt[i] = 0u;
  __syncthreads();
  const int64_t* __restrict__ ids = a.idx[t] + b0 * L;
  const int n = nb * L;                                               // <= kCountSlots, or one bag's <= 65535
  if (L == 1) {
    for (int i = threadIdx.x; i < n; i += kCountThreads) s_cnt[i] = ids[i] >= 0 ? 1u : 0u;
  } else {
    for (int i = threadIdx.x; i < n; i += kCountThreads)
      if (ids[i] >= 0) atomicAdd(&s_cnt[i / L], 1u);
  }
  __syncthreads();
  uint16_t* out = a.cnt + (int64_t)t * a.batch + b0;
  for (int i = threadIdx.x; i < nb; i += kCountThreads) out[i] = (uint16_t)s_cnt[i];
}

}  // namespace

void emb_padmean_count(const BagsCountArgs& a, hipStream_t stream) {
  int64_t total = 0;
  for (int t = 0; t < a.nt; t++) total += count_wgs(a.batch, a.L[t]);      // <= sum batch * L_t / 512 + nt: far below the grid limit
  hipLaunchKernelGGL(bags_count_kernel, dim3((unsigned)total), dim3(kCountThreads), 0, stream, a);
}

}  // namespace ffh_emb
