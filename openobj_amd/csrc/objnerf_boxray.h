// One camera ray against one oriented box: the arithmetic of Trainer.sample_points_bbox (trainer.py:136-167) on
// origin_dirs_W (utils.py:324-336) and ray_box_intersection (utils.py:293-322), written once.  objnerf_box_rays
// (objnerf_misc.hip, one box, every pixel) and objnerf_view_rays_count / _emit (objnerf_mapview.hip, every box of a map
// view) both call it: the units are built with -ffp-contract=off, so the same source gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

struct BoxRay {
  float dw[3];          // the direction in the world frame (un-normalised, as dirs_C is)
  float near_, far_;    // max(near, 0) and far + 0.2 (trainer.py:166-167)
  bool hit;             // utils.py:317
};

// T_WC, T_OC: row-major, rows 0..2 read (4 floats a row); half: the box's extent / 2
__device__ __forceinline__ BoxRay box_ray(const float* __restrict__ T_WC, const float* __restrict__ T_OC,
                                          const float* __restrict__ half, const float d0, const float d1, const float d2) {
  BoxRay b;
  float nr = -INFINITY, fr = INFINITY;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    // utils.py:324-336: R @ d, products accumulated left to right
    b.dw[r] = (T_WC[r * 4] * d0 + T_WC[r * 4 + 1] * d1) + T_WC[r * 4 + 2] * d2;
    const float dr = (T_OC[r * 4] * d0 + T_OC[r * 4 + 1] * d1) + T_OC[r * 4 + 2] * d2;
    const float o = T_OC[r * 4 + 3];
    const float ta = (-half[r] - o) / dr, tb = (half[r] - o) / dr;       // utils.py:311-312
    nr = fmaxf(nr, fminf(ta, tb));
    fr = fminf(fr, fmaxf(ta, tb));
  }
  b.hit = (nr <= fr) && (fr > 0.f);                                       // :317
  b.near_ = fmaxf(nr, 0.f);                                               // trainer.py:166
  b.far_ = fr + 0.2f;                                                     // :167
  return b;
}
