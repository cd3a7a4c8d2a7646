// lr_schedule.hip -- the state block of include/ff_hip_lr.h: init, the one-lane advance, read-back
#include "ffh_common.h"
#include "lr_state.h"

#include <math.h>

// The values of step k from the schedule and the running products of t = k + 1.  Host (init) and device (advance) run this one body.
// b1t / b2t arrive through ffh_lr_opaque: the compiler cannot see them as the product b * bt it has just formed, so 1 - b2t stays a
// subtraction of the ROUNDED product (hipcc contracts a*b+c by default; AdamOptimizer::next rounds the product when it stores it).
FFH_LR_INLINE void lr_state_fill(ffh_lr_state* s, int64_t k, double b1t, double b2t) {
  const ffh_lr_schedule& c = s->sched;
  const double rate = ffh_lr_schedule_value(k, c.base, c.warmup_steps, c.decay_start, c.decay_steps);
  b1t = ffh_lr_opaque(b1t);
  b2t = ffh_lr_opaque(b2t);
  const double num = rate * sqrt(1.0 - b2t);          // alpha * sqrt(1 - beta2_t) / (1 - beta1_t), left to right as the host spells it
  const double alpha_t = num / (1.0 - b1t);
  s->k = k;
  s->lr = (float)rate;
  s->alpha_t = (float)alpha_t;
  s->b1t = b1t;
  s->b2t = b2t;
}

__global__ void lr_state_advance_kernel(ffh_lr_state* s) {
  const double b1t = s->b1t * s->sched.beta1;
  const double b2t = s->b2t * s->sched.beta2;
  lr_state_fill(s, s->k + 1, b1t, b2t);
}

extern "C" {

int ffh_lr_abi_version(void) { return FFH_LR_ABI_VERSION; }
size_t ffh_lr_state_bytes(void) { return sizeof(ffh_lr_state); }

int ffh_lr_state_init(ffh_ctx* c, ffh_lr_state* block, const ffh_lr_schedule* sched, int64_t first_step, ffh_stream s) {
  FFH_REQUIRE(c, block && sched, "lr_state_init: null block or schedule");
  FFH_REQUIRE(c, first_step >= 0 && sched->warmup_steps >= 0 && sched->decay_start >= 0 && sched->decay_steps >= 0, "lr_state_init: negative step count");
  FFH_REQUIRE(c, sched->decay_steps == 0 || sched->decay_start >= sched->warmup_steps, "lr_state_init: the decay starts inside the warm-up");
  ffh_lr_state h;
  memset(&h, 0, sizeof h);
  h.sched = *sched;
  double b1t = 1.0, b2t = 1.0;
  for (int64_t i = 0; i <= first_step; i++) { b1t = ffh_lr_opaque(b1t * sched->beta1); b2t = ffh_lr_opaque(b2t * sched->beta2); }
  lr_state_fill(&h, first_step, b1t, b2t);
  FFH_HIP_TRY(c, hipMemcpyAsync(block, &h, sizeof h, hipMemcpyHostToDevice, as_stream(s)));
  FFH_HIP_TRY(c, hipStreamSynchronize(as_stream(s)));      // `h` is on this frame
  return FFH_OK;
}

int ffh_lr_state_advance(ffh_ctx* c, ffh_lr_state* block, ffh_stream s) {
  FFH_REQUIRE(c, block != nullptr, "lr_state_advance: null block");
  hipLaunchKernelGGL(lr_state_advance_kernel, dim3(1), dim3(1), 0, as_stream(s), block);
  FFH_LAUNCH_CHECK(c, "lr_state_advance");
  return FFH_OK;
}

int ffh_lr_state_read(ffh_ctx* c, const ffh_lr_state* block, ffh_lr_values* out, ffh_stream s) {
  FFH_REQUIRE(c, block && out, "lr_state_read: null block or destination");
  ffh_lr_state h;
  FFH_HIP_TRY(c, hipMemcpyAsync(&h, block, sizeof h, hipMemcpyDeviceToHost, as_stream(s)));
  FFH_HIP_TRY(c, hipStreamSynchronize(as_stream(s)));
  out->k = h.k; out->lr = h.lr; out->alpha_t = h.alpha_t; out->beta1_t = h.b1t; out->beta2_t = h.b2t;
  return FFH_OK;
}

}  // extern "C"
