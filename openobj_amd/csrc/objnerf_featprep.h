// The feature head's small preparation passes as device functions: featg_wb_kernel, featg_rowstats_kernel
// (objnerf_generic.hip) and the extra workgroups of gemm_group_kernel (objnerf_gemm.hip) run the same code.  The library
// is built without relocatable device code, so both units see the definitions.
#pragma once
#include "objnerf_device.h"

namespace objgen {

// Optional extra workgroups of a grouped launch (blockIdx.z >= zbeg[count], x = y = 0): the feature branch's small
// preparation passes of the one-launch background iteration -- wb = W_of^T b_of, bb; beta = b_of . g, |g| per ray; a copy of
// [W_of | b_of] for the head's finish -- ride on the launch of its two preparation GEMMs (round 6: three launches fewer).
struct FeatPrepTask {
  int blocks = 0;                         // 0: no task
  const float* params; long ps; int off_w, off_b, C, Hh, R, rin_ld, K;
  const float* gt_feat; float* rayin; float* gram; long gstride; float* snap;
  int nb_wb, nb_rs, nb_snap;              // workgroups per object of the three passes
};
// beta = b_of . g, |g| of ray r of object k (gt_feat [K][R][C]) into the last two columns of its rayin record  (u =
// W_of^T g is a GEMM): the 16 lanes of a DPP row share the ray
__device__ __forceinline__ void featg_ray_stats(const float* B, const int C, const int R, const float* gt_feat,
                                                float* rayin, const int rin_ld, const int k, const long r, const int l16) {
  float bs = 0.f, gs = 0.f;
  if (r < R) {
    const float* gp = gt_feat + ((long)k * R + r) * C;
    for (int cc = l16; cc < C; cc += 16) {
      const float gv = gp[cc];
      bs = fmaf(B[cc], gv, bs);
      gs = fmaf(gv, gv, gs);
    }
  }
  bs = dpp_rowsum16(bs);
  gs = dpp_rowsum16(gs);
  if (r < R && l16 == 0) {
    float* o = rayin + ((long)k * R + r) * rin_ld;
    o[rin_ld - 2] = bs;
    o[rin_ld - 1] = sqrtf(gs);
  }
}
// Entry h of [wb | bb], wb = W_of^T b_of (h < Hh), bb = b_of . b_of (h == Hh): one wave per entry
__device__ __forceinline__ float featg_wb_entry(const float* W, const float* B, const int C, const int Hh, const int h,
                                                const int lane) {
  float acc = 0.f;
  for (int cc = lane; cc < C; cc += 64) acc = fmaf(h < Hh ? W[(long)cc * Hh + h] : B[cc], B[cc], acc);
  return wave_sum64(acc);
}
// FeatPrepTask (512 threads per workgroup): featg_wb_kernel's, featg_rowstats_kernel's work and the [W_of | b_of] copy.
// b = (object, pass-local index)
__device__ void feat_prep_task(const FeatPrepTask& t, int b) {
  const int per = t.nb_wb + t.nb_rs + t.nb_snap;
  const int k = b / per;
  b -= k * per;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* W = t.params + (long)k * t.ps + t.off_w;
  const float* B = t.params + (long)k * t.ps + t.off_b;
  if (b < t.nb_wb) {                                       // wb[h] = W_of[:, h] . b_of (h < Hh), bb = b_of . b_of: a wave per entry
    const int h = 8 * b + wv;
    if (h <= t.Hh) {
      const float acc = featg_wb_entry(W, B, t.C, t.Hh, h, lane);
      if (lane == 0) t.gram[(long)k * t.gstride + (long)t.Hh * t.Hh + h] = acc;
    }
    return;
  }
  b -= t.nb_wb;
  if (b < t.nb_rs) {                                       // beta, |g| of 32 rays: 16 lanes per ray
    const int l16 = tid & 15;
    const long r = (long)b * 32 + (tid >> 4);
    featg_ray_stats(B, t.C, t.R, t.gt_feat, t.rayin, t.rin_ld, k, r, l16);
    return;
  }
  b -= t.nb_rs;
  if (t.snap) {                                            // [W_of (C x Hh) | b_of (C)] as they are BEFORE the step
    float* o = t.snap + (long)k * ((long)t.C * (t.Hh + 1));
    const long tot = (long)t.C * (t.Hh + 1);
    for (long i = (long)b * 2048 + tid; i < tot && i < (long)(b + 1) * 2048; i += 512)
      o[i] = i < (long)t.C * t.Hh ? W[i] : B[i - (long)t.C * t.Hh];
  }
}

}  // namespace objgen
