// The per-ray loss that every step kernel must evaluate bit-identically, defined once: the label masks, the depth
// weighting, the residuals, the gradient seeds, the loss terms, the backward of the compositing per sample and the
// hoisted feature cosine.  Callers: train_fused32_kernel (objnerf_train32.hip), train_fused_bf16_kernel
// (objnerf_train_bf16.hip), the bf16v2 kernels (objnerf_bf16v2_body.h), kernel A of the hidden-256 step in both forms
// (objnerf_train256.hip, objnerf_train256r_body.h), train_small_kernel (objnerf_small_body.h) and loss_kernel
// (objnerf_misc.hip).  Device functions only: scalars in, a small struct of floats out; no memory access, no cross-lane
// operation, no barrier.  Resid and Seeds are passed BY VALUE: by reference the same code changed the instruction order of
// the hidden-256 kernels (profiles/ray_loss_refactor.txt).  How a kernel obtains D, O, C, V (scans, seg_sum, wave_sum64),
// under which condition it accumulates a term and where it stores a result stay with the kernel.  Every expression keeps
// one association: with -ffp-contract=off that is what makes the paths agree to the bit.
#pragma once
#include <hip/hip_runtime.h>

namespace rayloss {

__device__ __forceinline__ float sgn(const float x) { return x > 0.f ? 1.0f : (x < 0.f ? -1.0f : 0.0f); }

// The normaliser of a masked mean (render_rays.py:103) from an object's mask count.  An early-return flag
// (render_rays.py:89-94) zeroes the terms and gradients of its mask: `flag ? 0.0f : mean_norm(n)`.  That conditional stays
// in the callers -- inside a function the compiler lays its branch out the other way round in every kernel's prologue.
__device__ __forceinline__ float mean_norm(const float n) { return 1.0f / (n + 1e-10f); }

// The depth term's weighting by the ray's depth variance (render_rays.py:96-100)
__device__ __forceinline__ float depth_weight(const float V) { return 1.0f / (sqrtf(V) + 1e-4f); }

// One ray's masks, depth weighting and residuals (loss.py:27-79) from its composited depth D, opacity O, colour C and
// depth variance V (loss.py:31-35).  label: 0 = another object, 1 = this object, 2 = unknown
struct Resid { float m1, m2, info, rd, r0, r1, r2, ro; };
__device__ __forceinline__ Resid residuals(const float D, const float O, const float C0, const float C1, const float C2,
                                           const float V, const float gt_depth, const float gt_r, const float gt_g,
                                           const float gt_b, const int label) {
  Resid r;
  r.m1 = (label == 1) ? 1.0f : 0.0f;                   // mask_sem & mask_obj
  r.m2 = (label != 2) ? 1.0f : 0.0f;                   // mask_sem
  const float tgt = (label != 0) ? 1.0f : 0.0f;        // mask_obj.float()
  r.info = depth_weight(V);
  r.rd = D - gt_depth; r.r0 = C0 - gt_r; r.r1 = C1 - gt_g; r.r2 = C2 - gt_b; r.ro = O - tgt;
  return r;
}

// d total / d (D, C, O) of the ray: the L1 terms' signs, scaled and normalised
struct Seeds { float gD, gC0, gC1, gC2, gO; };
__device__ __forceinline__ Seeds seeds(const Resid r, const float color_scaling, const float opacity_scaling,
                                       const float inv1, const float inv2) {
  Seeds g;
  g.gD = r.m1 * sgn(r.rd) * r.info * inv1;
  g.gC0 = color_scaling * r.m1 * sgn(r.r0) * inv1;
  g.gC1 = color_scaling * r.m1 * sgn(r.r1) * inv1;
  g.gC2 = color_scaling * r.m1 * sgn(r.r2) * inv1;
  g.gO = opacity_scaling * r.m2 * sgn(r.ro) * inv2;
  return g;
}

// One ray's contribution to the depth, colour and opacity terms.  Separate functions: a kernel calls them inside its own
// condition (one lane per ray), so nothing is computed for the lanes that drop them.
__device__ __forceinline__ float term_depth(const Resid r, const float inv1) { return r.m1 * fabsf(r.rd) * r.info * inv1; }
__device__ __forceinline__ float term_colour(const Resid r, const float inv1) {
  return r.m1 * (fabsf(r.r0) + fabsf(r.r1) + fabsf(r.r2)) * inv1;
}
__device__ __forceinline__ float term_opacity(const Resid r, const float inv2) { return r.m2 * fabsf(r.ro) * inv2; }

// d total / d weight of a sample at depth z with colour c (without the feature term's part)
__device__ __forceinline__ float sample_dw(const Seeds g, const float z, const float c0, const float c1, const float c2) {
  return g.gD * z + g.gO + g.gC0 * c0 + g.gC1 * c1 + g.gC2 * c2;
}

// Backward of w_i = occ_i T_i, T_i = prod_{j<i} fr_j (render_rays.py:38-43): suffix = sum_{j>i} dw_j w_j
__device__ __forceinline__ float d_occ(const float dw, const float T, const float suffix, const float fr) {
  return dw * T - suffix / fr;
}

// Through the sigmoid of the occupancy: d / d alpha.  The fused kernels differentiate by the RAW network output and
// multiply by the 10 of model.py:88 themselves.
__device__ __forceinline__ float d_alpha(const float docc, const float occ) { return docc * occ * (1.0f - occ); }

// d / d raw colour (pre-sigmoid) of a sample with weight w and colour c
__device__ __forceinline__ float d_raw_colour(const float gC, const float w, const float c) { return gC * w * c * (1.0f - c); }

// ---- feature-distillation term (loss.py:82-99) with the linear head hoisted past the compositing:
// F = W_of fh + b_of O,  fh = sum_s w_s hf_s.  cos(F, g) only needs
//   F.g = fh.u + O beta,   |F|^2 = fh^T G fh + 2 O wb.fh + O^2 bb     (u, beta, |g|, G, wb, bb precomputed)
// Two forms of its reciprocals, which do not agree to the bit: exact division and square root (the fp32 and the layer-wise
// paths, and the pass loop of the first-generation bf16 kernel) and the 1-ulp hardware v_rcp_f32 / v_sqrt_f32 (its one
// caller: train_fused_bf16v2f_kernel).  Returns cos(F, g) of the ray and the two coefficients of its gradient, d total / d F = ar g / |g| + cr F.
enum class Rcp { exact, hardware };
struct FeatCos { float cosv, ar, cr; };
template <Rcp FORM>
__device__ __forceinline__ FeatCos feat_cos(const float fu, const float fGf, const float fwb, const float O,
                                            const float beta, const float ngv, const float bb, const float m1,
                                            const float feat_scaling, const float inv1) {
  const float dotFg = fu + O * beta;
  const float nF2 = fmaxf(fGf + 2.0f * O * fwb + O * O * bb, 0.0f);
  FeatCos f;
  if constexpr (FORM == Rcp::exact) {
    const float nF = fmaxf(sqrtf(nF2), 1e-8f), ngc = fmaxf(ngv, 1e-8f);
    f.cosv = dotFg / (nF * ngc);
    const float gam = -feat_scaling * m1 * inv1;       // d total / d cos
    f.ar = gam / (nF * ngc);
    f.cr = -gam * f.cosv / (nF * nF);
  } else {
    const float nF = fmaxf(__builtin_amdgcn_sqrtf(nF2), 1e-8f), ngc = fmaxf(ngv, 1e-8f);
    const float rnn = __builtin_amdgcn_rcpf(nF * ngc);
    f.cosv = dotFg * rnn;
    const float gam = -feat_scaling * m1 * inv1;       // d total / d cos
    f.ar = gam * rnn;
    f.cr = -gam * f.cosv * __builtin_amdgcn_rcpf(nF * nF);
  }
  return f;
}

// One ray's contribution to the feature term (called by the one lane that accumulates it)
__device__ __forceinline__ float term_feature(const float cosv, const float m1, const float inv1) {
  return m1 * (1.0f - cosv) * inv1;
}

// d total / d opacity, the feature term's part
__device__ __forceinline__ float gof(const float ar, const float cr, const float beta, const float fwb, const float O,
                                     const float bb) {
  return ar * beta + cr * (fwb + O * bb);
}

// d total / d fh, entry h: u = W_of^T g / |g|, Gfh = (G fh)[h], wb = (W_of^T b_of)[h]
__device__ __forceinline__ float gfh(const float ar, const float cr, const float u, const float Gfh, const float O,
                                     const float wb) {
  return ar * u + cr * (Gfh + O * wb);
}

}  // namespace rayloss
