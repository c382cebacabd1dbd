// The per-group body of the fp32 novel-view renderer: 16 rays (lane c <-> ray, lane group g <-> the feature rows
// 4 g + r of the register-resident MFMA chain, objnerf_mlp32.h) stepped through the n_bins - 1 mid-points of their
// stratified bins -- draw, mid-point, embedding, network, compositing, stores (vmap.py:644-676, trainer.py:171-176,
// render_rays.py:6-63).  Written once: objnerf_render_fwd (objnerf_render.hip, one object a launch) and
// objnerf_render_fwd_segmented (objnerf_mapview.hip, every hidden-32 object of a map view in one launch) call it, so a
// ray gets the same instructions -- and, with -ffp-contract=off, the same bits -- from either.
#pragma once
#include "objnerf_mlp32.h"
#include "objnerf_philox.h"

namespace obj32n {

// the rays of ONE object and where their results go; ray r of [0, n) is the Philox counter and the row of u
struct RenderDev {
  long n; int n_bins, G;
  const float* params; const float* scale; const float* origin; const float* dirs_W; const float* near_; const float* far_;
  const float* u; uint64_t seed; uint32_t draw;
  float* depth; float* opacity; float* rgb; float* hfeat; float* z_out;
  Layout L;
};

// group grp (rays 16 grp .. 16 grp + 15) of a; sv / wf: the staged weight image of a's object (stage_weights32)
template <bool FEAT>
__device__ __forceinline__ void render_group(const RenderDev& a, const float* sv, const float* wf, const float scale,
                                             const float ox, const float oy, const float oz, const int S,
                                             const uint32_t st, const int c, const int g, const long grp) {
  asm volatile("" ::: "memory");   // keep the LDS weight reads inside the caller's loop (no LICM into registers)
  const long ray = grp * 16 + c;
  const bool valid = ray < a.n;
  const long r = valid ? ray : a.n - 1;
  const float lo = a.near_[r], hi = a.far_[r];
  const float dx = a.dirs_W[r * 3], dy = a.dirs_W[r * 3 + 1], dz = a.dirs_W[r * 3 + 2];
  const float* ur = a.u ? a.u + r * a.n_bins : nullptr;
  float ublk[4] = {0.f, 0.f, 0.f, 0.f};
  auto draw_u = [&](const int s) {                          // the draw of bin s (injected, or Philox block s >> 2)
    if (ur) return ur[s];
    if ((s & 3) == 0 || s == 0) objrng::uniform4(a.seed, st, (uint32_t)(r >> 32), (uint32_t)r, (uint32_t)(s >> 2), ublk);
    return ublk[s & 3];
  };
  float z0 = strat(lo, hi, 0, a.n_bins, draw_u(0));
  float T = 1.0f;                                           // transmittance in front of the current sample
  float aD = 0.f, aO = 0.f, aC = 0.f;
  T32 aF = zero32();
  for (int s = 0; s < S; ++s) {
    const float z1 = strat(lo, hi, s + 1, a.n_bins, draw_u(s + 1));
    const float z = 0.5f * (z1 + z0);                       // trainer.py:175
    z0 = z1;
    if (a.z_out && valid && g == 0) a.z_out[r * S + s] = z;
    Pe32 pe;
    pe32_project(sv, g, ox + dx * z, oy + dy * z, oz + dz * z, scale, pe);     // trainer.py:176, embedding.py:47-48
    Emb32 e;
    embed32(e, pe, g);
    Acts act;
    float alpha10, col;
    mlp32_forward_all<FEAT>(wf, sv, g, e, act, alpha10, col);
    const float occ = sigmoid_acc(alpha10);                 // render_rays.py:6-14
    const float wgt = occ * T;                              // render_rays.py:32-54
    T *= (1.0f - occ) + 1e-10f;
    aD = fmaf(wgt, z, aD);                                  // render_rays.py:56-63
    aO += wgt;
    aC = fmaf(wgt, col, aC);
    if (FEAT) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) aF.t[tt][rr] = fmaf(wgt, act.hf.t[tt][rr], aF.t[tt][rr]);
    }
  }
  if (valid) {
    if (g == 0) { a.depth[ray] = aD; a.opacity[ray] = aO; }
    else a.rgb[ray * 3 + g - 1] = aC;
    if (FEAT) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
        *reinterpret_cast<float4*>(a.hfeat + ray * H + 16 * tt + 4 * g) =
            make_float4(aF.t[tt][0], aF.t[tt][1], aF.t[tt][2], aF.t[tt][3]);
    }
  }
}

}  // namespace obj32n
