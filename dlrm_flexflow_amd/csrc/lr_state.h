// lr_state.h -- the layout of ffh_lr_state (include/ff_hip_lr.h), shared by the translation units whose kernels read it
#pragma once
#include "../../include/ff_hip_lr.h"

// One block per reader stream.  `lr` and `alpha_t` are what the optimizer kernels load (one wave-uniform 4-byte read); the rest is
// what lr_state_advance_kernel needs to compute the next step's values.
struct ffh_lr_state {
  int64_t k;                 // zero-based index of the step the values below belong to
  float   lr;                // (float)ffh_lr_schedule_value(k, ...)
  float   alpha_t;           // Adam's step size of step k (t = k + 1)
  double  b1t, b2t;          // beta1^(k+1), beta2^(k+1): running products
  ffh_lr_schedule sched;
};
static inline const float* ffh_lr_rate_ptr(const ffh_lr_state* b, bool adam) { return adam ? &b->alpha_t : &b->lr; }
