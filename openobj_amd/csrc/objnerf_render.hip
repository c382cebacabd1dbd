// objnerf_render_fwd: novel-view rendering of ONE object inside its box in ONE launch (row f-1 of SURVEY.md 8;
// reference sceneObject.render_2D_syn vmap.py:604-685 on Trainer.sample_points_bbox trainer.py:130-198, the stacked
// modules embedding.py:46-55 + model.py:61-103 and render_rays.py:6-63).
//
// The reference (and rounds 1-3 here) materialise the sample points, then alpha / colour / the 512-d feature of every
// sample, then composite.  Per ray of 149 samples that is 21 KB of per-sample tensors written and read back.  Here a
// lane owns a RAY: a wave steps through the 149 mid-points of 16 rays at once (lane c <-> ray, lane group g <-> the
// feature rows 4 g + r of the register-resident MFMA chain, objnerf_mlp32.h), so the transmittance is a running product
// in a register -- no scan, no shuffle -- and depth / opacity / colour / the 32-wide feature hidden accumulate per lane.
// Nothing per sample ever leaves the registers; a ray costs 20 B of input and 16 + 128 B of output.  The 512-d head is
// applied afterwards to the composited hidden of the rays that pass the masks (exact: the head is linear).
#include "objnerf_render_body.h"
#include "../../include/objnerf_hip.h"

namespace {
using namespace obj32n;

template <bool FEAT>
__global__ __launch_bounds__(256) void render_fwd_kernel(const RenderDev a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  stage_weights32(lds, a.params, a.L, FEAT, tid, 256);
  const float* sv = lds + sv_base(FEAT);
  const float* wf = (const float*)__builtin_assume_aligned(lds + 4 * g * WROW + out_pos(c), 8);
  const float scale = a.scale[0];
  const float ox = a.origin[0], oy = a.origin[1], oz = a.origin[2];
  const int S = a.n_bins - 1;
  const long ngroups = (a.n + 15) / 16;                      // 16 rays per wave step
  const uint32_t st = objrng::S_BOX_U | (a.draw << 3);
  for (long grp = (long)blockIdx.x * 4 + w; grp < ngroups; grp += (long)a.G * 4)
    render_group<FEAT>(a, sv, wf, scale, ox, oy, oz, S, st, c, g, grp);      // objnerf_render_body.h
}

}  // namespace

// objnerf_render_bf16.hip
int objnerf_render_fwd_bf16(const objnerf_net* net, int64_t n, int32_t n_bins, const float* params, const float* scale,
                            const float* origin, const float* dirs_W, const float* near, const float* far, const float* u,
                            uint64_t seed, uint32_t draw, float* out_depth, float* out_opacity, float* out_rgb,
                            float* out_hfeat, float* out_z, void* stream);

extern "C" int objnerf_render_fwd(const objnerf_net* net, int64_t n, int32_t n_bins, const float* params, const float* scale,
                                  const float* origin, const float* dirs_W, const float* near, const float* far,
                                  const float* u, uint64_t seed, uint32_t draw, float* out_depth, float* out_opacity,
                                  float* out_rgb, float* out_hfeat, float* out_z, int32_t mode, void* stream) {
  (void)hipGetLastError();
  if (!net || n <= 0 || n_bins < 2 || !params || !scale || !origin || !dirs_W || !near || !far || !out_depth ||
      !out_opacity || !out_rgb)
    return OBJNERF_EINVAL;
  if (net->hidden != 32 || net->n_freqs != 6) return OBJNERF_ENOTSUP;      // (wider networks: the layer-wise chain)
  if (mode & ~OBJNERF_TRAIN_BF16) return OBJNERF_ENOTSUP;
  if (mode & OBJNERF_TRAIN_BF16)
    return objnerf_render_fwd_bf16(net, n, n_bins, params, scale, origin, dirs_W, near, far, u, seed, draw, out_depth,
                                   out_opacity, out_rgb, out_hfeat, out_z, stream);
  RenderDev d;
  d.n = n; d.n_bins = n_bins;
  d.params = params; d.scale = scale; d.origin = origin; d.dirs_W = dirs_W; d.near_ = near; d.far_ = far;
  d.u = u; d.seed = seed; d.draw = draw;
  d.depth = out_depth; d.opacity = out_opacity; d.rgb = out_rgb; d.hfeat = out_hfeat; d.z_out = out_z;
  d.L = make_layout(net->feat_dim);
  const int cu = objnerf_num_cu();
  const long ngroups = (n + 15) / 16;
  const bool feat = out_hfeat != nullptr;
  const size_t lds_bytes = (size_t)img_floats(feat) * 4;
  long G = 2L * cu;                                           // two workgroups of 4 waves per CU: 2 waves per SIMD
  if (G * 4 > ngroups) G = (ngroups + 3) / 4;
  d.G = (int)G;
  objnerf_once_per_device([] {
    (void)hipFuncSetAttribute((const void*)render_fwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, img_floats(true) * 4);
    (void)hipFuncSetAttribute((const void*)render_fwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, img_floats(false) * 4);
  });
  if (feat) hipLaunchKernelGGL(render_fwd_kernel<true>, dim3((unsigned)G), dim3(256), lds_bytes, (hipStream_t)stream, d);
  else hipLaunchKernelGGL(render_fwd_kernel<false>, dim3((unsigned)G), dim3(256), lds_bytes, (hipStream_t)stream, d);
  return hipGetLastError() == hipSuccess ? OBJNERF_OK : OBJNERF_ELAUNCH;
}
