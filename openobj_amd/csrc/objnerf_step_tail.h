// The arithmetic that the tail of a training step must do bit-identically on every path, defined once: the AdamW
// element update and its per-group preamble (adamw_kernel / adamw_dyn_kernel, finalize_kernel, reduce_parts_kernel,
// featg_finish_adamw_kernel) and the status bits of a loss term (loss_total_kernel, finalize_kernel,
// reduce_parts_kernel, finalize256_kernel, reduce_loss_kernel).  Device functions only.
#pragma once
#include <hip/hip_runtime.h>

// The iteration's early-return flags (render_rays.py:89-94) from the objects' mask counts [K][2]: flag j is set when
// some object has no ray in mask j
__device__ __forceinline__ void early_flags_of_counts(const int* counts, const int K, int& e0, int& e1) {
  e0 = 0; e1 = 0;
  for (int kk = 0; kk < K; ++kk) { e0 |= counts[2 * kk] == 0; e1 |= counts[2 * kk + 1] == 0; }
}

// Optimiser group of arena entry i: 0 = trunk + density head + B, 1 = colour branch [lo1, lo2), 2 = feature branch
// [lo2, hi2)
__device__ __forceinline__ int adamw_group_of(const long i, const long lo1, const long lo2, const long hi2) {
  return (i >= lo1 && i < lo2) ? 1 : ((i >= lo2 && i < hi2) ? 2 : 0);
}

// Group g of a step, from the two early-return flags: when the label-1 masks trigger the early return (f0) the colour
// and feature branches get .grad = None and torch.optim.AdamW skips them entirely (no decay, no moment update, and their
// step count does not advance); with both flags set nothing has a gradient.  Step counters: two banks of three; a call
// READS bank `bank` and ONE block of it (publish) WRITES the advanced counters to the other one -- no second launch,
// and no block can see a counter of its own call already advanced.  The bias corrections are formed in double.
__device__ __forceinline__ void adamw_group_begin(const int g, const bool f0, const bool f1, int* steps, const int bank,
                                                  const double lr, const double b1, const double b2, const bool publish,
                                                  int& active, float& step_size, float& bc2_sqrt) {
  const bool act = g == 0 ? !(f0 && f1) : !f0;
  active = act;
  const int old = steps[3 * bank + g];
  const double st = (double)(old + 1);
  step_size = (float)(lr / (1.0 - pow(b1, st)));
  bc2_sqrt = (float)sqrt(1.0 - pow(b2, st));
  if (publish) steps[3 * (1 - bank) + g] = old + (act ? 1 : 0);
}

// The update's fp32 coefficients from the optimiser's double hyper-parameters
__device__ __forceinline__ void adamw_coeffs(const double lr, const double b1, const double b2, const double wd,
                                             float& decay, float& w1, float& beta2, float& w2) {
  decay = (float)(1.0 - lr * wd); w1 = (float)(1.0 - b1); w2 = (float)(1.0 - b2); beta2 = (float)b2;
}

// torch.optim.AdamW (single-tensor formulation) on element idx with gradient g
__device__ __forceinline__ void adamw_update(float* params, float* m, float* v, const long idx, const float g,
                                             const float decay, const float w1, const float beta2, const float w2,
                                             const float step_size, const float bc2_sqrt, const float eps) {
  float p = params[idx] * decay;
  const float mo = m[idx];
  const float mn = mo + w1 * (g - mo);
  const float vn = v[idx] * beta2 + (w2 * g) * g;
  const float denom = sqrtf(vn) / bc2_sqrt + eps;
  p = p + (-step_size) * (mn / denom);
  params[idx] = p;
  m[idx] = mn;
  v[idx] = vn;
}

// Status bits of one loss term.  Bit 0: above 1e5 (render_rays.py:109-111).  Bit 1: NaN / Inf -- reported, NOT fatal
// (the reference's comparison is false for NaN and it carries on with NaN parameters).
// Only for units built WITHOUT -fno-honor-nans (the Makefile's SCHED32 / SCHED16V2 / SCHED16V2F): there the compiler
// folds the NaN test away, so objnerf_train32.hip and the two bf16v2 units must not call this.
__device__ __forceinline__ int loss_status_bits(const float v) {
  return (v > 100000.f ? 1 : 0) | (!(fabsf(v) <= 3.0e38f) ? 2 : 0);
}
