// ctr.hip -- binary cross-entropy on a probability and the evaluation metrics (AUC histograms) of include/ff_hip_ctr.h for gfx950.
// The one-launch form of the loss step (ffh_linear_bwd_bce) is a loss kind of the skinny backward in linear.hip.
#include "ffh_common.h"
#include "../../include/ff_hip_ctr.h"

namespace {

// the contract's per-element loss (include/ff_hip_ctr.h): -( y max(log p, -100) + (1 - y) max(log(1 - p), -100) )
__device__ __forceinline__ float bce_element(float p, float y) {
  const float lp = fmaxf(logf(p), -100.0f), lq = fmaxf(logf(1.0f - p), -100.0f);
  return -(y * lp + (1.0f - y) * lq);
}

// metrics_kernel (elementwise.hip) with the BCE loss step: the same reductions, one atomic per counter per workgroup
__global__ __launch_bounds__(256) void bce_metrics_kernel(const float* __restrict__ prob, const float* __restrict__ labels,
                                                          ffh_perf_metrics* __restrict__ perf, float* __restrict__ bce_sum, int64_t ns, int nc,
                                                          int flags, float* __restrict__ lg, float scale) {
  ffh_kernel_prio();
  __shared__ float s_f[4][4];
  __shared__ int   s_i[2][4];
  float mse_s = 0.f, rmse_s = 0.f, mae_s = 0.f, bce_s = 0.f;
  int all = 0, correct = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < ns; b += stride) {
    all += 1;
    float bce = 0.f;
    for (int i = 0; i < nc; i++) {
      const float p = prob[b * nc + i], y = labels[b * nc + i];
      lg[b * nc + i] = __fmul_rn(__fsub_rn(p, y), scale);            // dz = (p - y) * scale: two roundings, no fma
      if (flags & FFH_METRIC_BCE) bce += bce_element(p, y);
    }
    bce_s += bce;
    if (flags & 1) {     // the accuracy rule of ffh_metrics_update
      if (nc == 1) { all += 1; correct += 1; }
      else {
        float max_val = 0.0f; int my = -1, tr = -1;
        for (int i = 0; i < nc; i++) {
          const float lv = prob[b * nc + i];
          if (my == -1 || lv > max_val) { max_val = lv; my = i; }
          if (labels[b * nc + i] > 0.9f) tr = i;
        }
        if (tr == my) correct += 1;
      }
    }
    if (flags & (2 | 4 | 8)) {
      float mse = 0.f, mae = 0.f;
      for (int i = 0; i < nc; i++) {
        const float diff = prob[b * nc + i] - labels[b * nc + i];
        mse = __fmaf_rn(diff, diff, mse);
        mae += fabsf(diff);
      }
      mse_s += mse; rmse_s += sqrtf(mse); mae_s += mae;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mse_s += __shfl_down(mse_s, o); rmse_s += __shfl_down(rmse_s, o); mae_s += __shfl_down(mae_s, o); bce_s += __shfl_down(bce_s, o);
    all += __shfl_down(all, o); correct += __shfl_down(correct, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_f[0][wave] = mse_s; s_f[1][wave] = rmse_s; s_f[2][wave] = mae_s; s_f[3][wave] = bce_s; s_i[0][wave] = all; s_i[1][wave] = correct; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int al = s_i[0][0] + s_i[0][1] + s_i[0][2] + s_i[0][3];
    const int co = s_i[1][0] + s_i[1][1] + s_i[1][2] + s_i[1][3];
    if (al) atomicAdd(&perf->train_all, al);
    if (co) atomicAdd(&perf->train_correct, co);
    if (flags & 2) atomicAdd(&perf->mse_loss, (s_f[0][0] + s_f[0][1]) + (s_f[0][2] + s_f[0][3]));
    if (flags & 4) atomicAdd(&perf->rmse_loss, (s_f[1][0] + s_f[1][1]) + (s_f[1][2] + s_f[1][3]));
    if (flags & 8) atomicAdd(&perf->mae_loss, (s_f[2][0] + s_f[2][1]) + (s_f[2][2] + s_f[2][3]));
    if (flags & FFH_METRIC_BCE) atomicAdd(bce_sum, (s_f[3][0] + s_f[3][1]) + (s_f[3][2] + s_f[3][3]));
  }
}

// Evaluation metrics of a batch.  The two histograms hold 2 x FFH_AUC_BINS 64-bit counters (1 MB): no workgroup can keep a private copy in
// LDS, so every sample is one 64-bit integer atomic on its global bin (they resolve in L2; a batch is at most a few times 10^4 samples).
// The scalar counts are reduced in registers / LDS first: one integer atomic per count per workgroup.
__global__ __launch_bounds__(256) void ctr_eval_kernel(const float* __restrict__ prob, const float* __restrict__ labels,
                                                       ffh_ctr_eval* __restrict__ ev, int64_t ns) {
  ffh_kernel_prio();
  typedef unsigned long long u64;
  __shared__ int   s_i[4][4];
  __shared__ float s_f[4];
  int n = 0, pos = 0, correct = 0, nans = 0;
  float ll = 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < ns; b += stride) {
    const float p = prob[b], y = labels[b];
    if (p != p) { nans += 1; continue; }
    const bool is_pos = y >= 0.5f;
    n += 1;
    pos += is_pos ? 1 : 0;
    correct += ((p >= 0.5f) == is_pos) ? 1 : 0;
    ll += bce_element(p, y);
    const float t = p * (float)FFH_AUC_BINS;                         // exact: FFH_AUC_BINS is a power of two
    const int bin = !(t > 0.0f) ? 0 : (t >= (float)FFH_AUC_BINS ? FFH_AUC_BINS - 1 : (int)t);
    atomicAdd(reinterpret_cast<u64*>(is_pos ? ev->hist_pos : ev->hist_neg) + bin, (u64)1);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_down(n, o); pos += __shfl_down(pos, o); correct += __shfl_down(correct, o); nans += __shfl_down(nans, o);
    ll += __shfl_down(ll, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_i[0][wave] = n; s_i[1][wave] = pos; s_i[2][wave] = correct; s_i[3][wave] = nans; s_f[wave] = ll; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tn = s_i[0][0] + s_i[0][1] + s_i[0][2] + s_i[0][3], tp = s_i[1][0] + s_i[1][1] + s_i[1][2] + s_i[1][3];
    const int tc = s_i[2][0] + s_i[2][1] + s_i[2][2] + s_i[2][3], tx = s_i[3][0] + s_i[3][1] + s_i[3][2] + s_i[3][3];
    if (tn) atomicAdd(reinterpret_cast<u64*>(&ev->samples), (u64)tn);
    if (tp) atomicAdd(reinterpret_cast<u64*>(&ev->positives), (u64)tp);
    if (tc) atomicAdd(reinterpret_cast<u64*>(&ev->correct), (u64)tc);
    if (tx) atomicAdd(reinterpret_cast<u64*>(&ev->nan_predictions), (u64)tx);
    if (tn) atomicAdd(&ev->logloss_sum, (s_f[0] + s_f[1]) + (s_f[2] + s_f[3]));
  }
}

}  // namespace

extern "C" {

int ffh_ctr_abi_version(void) { return FFH_CTR_ABI_VERSION; }

int ffh_bce_bwd_metrics(ffh_ctx* c, float* lg, const float* prob, const float* label, ffh_perf_metrics* perf, float* bce_sum,
                        int64_t ns, int nc, float scale, int flags, ffh_stream s) {
  FFH_REQUIRE(c, ns >= 0 && nc > 0 && perf && ((lg && prob && label) || ns == 0), "bce_bwd_metrics: bad args");
  FFH_REQUIRE(c, bce_sum || !(flags & FFH_METRIC_BCE), "bce_bwd_metrics: FFH_METRIC_BCE needs bce_sum");
  if (ns == 0) return FFH_OK;
  hipLaunchKernelGGL(bce_metrics_kernel, dim3(ffh_grid(ns, 256, 256)), dim3(256), 0, as_stream(s), prob, label, perf, bce_sum, ns, nc, flags, lg, scale);
  FFH_LAUNCH_CHECK(c, "bce_metrics_kernel");
  return FFH_OK;
}

int ffh_ctr_eval_update(ffh_ctx* c, const float* prob, const float* label, ffh_ctr_eval* ev, int64_t ns, ffh_stream s) {
  FFH_REQUIRE(c, ns >= 0 && ev && ((prob && label) || ns == 0), "ctr_eval_update: bad args");
  if (ns == 0) return FFH_OK;
  hipLaunchKernelGGL(ctr_eval_kernel, dim3(ffh_grid(ns, 256, 256)), dim3(256), 0, as_stream(s), prob, label, ev, ns);
  FFH_LAUNCH_CHECK(c, "ctr_eval_kernel");
  return FFH_OK;
}

}  // extern "C"
