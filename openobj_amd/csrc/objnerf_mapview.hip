// A novel view of the WHOLE map in one launch chain (gfx950): the loop of train.py:550-612 (`cfg.if_render`) -- one
// sceneObject.render_2D_syn per object (vmap.py:604-685), each with its own box test over every pixel, its own launch and
// a z-buffer merge of four [W, H] images on the host (train.py:581-598) -- as three stages:
//
// 1. objnerf_view_rays_count / _emit: the candidate rays of ALL objects.  Pixel p = w * H + h of the transposed [W, H]
//    image is tested against box k with box_ray (objnerf_boxray.h, the function objnerf_box_rays runs); the hits of an
//    object become one segment of a CSR over the objects in the caller's (dict) order, ascending in p inside a segment
//    (count / scan / emit of objnerf_wg.h: prefixes run in thread order, no atomics), which is the order of the
//    nonzero() in render_2D_syn.  An object with at most one hit gets an EMPTY segment (trainer.py:164-165 of the
//    reference drops it): view_drop_kernel zeroes its counts before the scan.
// 2. objnerf_render_fwd_segmented: render_group (objnerf_render_body.h, the body objnerf_render_fwd runs) over the
//    segments of every hidden-32 object in ONE launch.  The work list is tiles (arena row, first 16-ray group, groups);
//    groups count from the segment's start, so ray r = entry - seg_lo is lane r & 15 of group r >> 4, the row of the
//    injected u and the Philox counter exactly as in the one-object kernel.  Workgroups are persistent: each takes a
//    contiguous share of the tile list and restages the LDS weight image only where the share crosses into another
//    row.  THE RESTAGE HAZARD: the four waves of a workgroup run their groups independently, so when the row changes
//    some waves may still be reading the old image out of LDS -- a workgroup barrier BEFORE stage_weights32 overwrites
//    it -- and no wave may start a group before every thread's part of the new image is written -- a barrier AFTER.
//    Both barriers sit under `row != staged`, which is uniform over the workgroup: every thread walks the same tiles
//    and reads the same row from the same address.  The per-wave group loop holds no barrier.
// 3. objnerf_view_merge: the reference's merge is a sequential fold in dict order in which a background object paints
//    colour and id but never depth.  Its closed form (render_view.merge_closed_form restates it in numpy):
//      an entry is OFFERED iff !((depth < near) | (depth > far) | (opacity < 0.9)) and depth < 100 (false for a NaN);
//      W(p) = the offered foreground entry of smallest depth, ties to the earliest object; depth(p) = depth_W or 100;
//      the painter of p = the LAST offered background entry after W's object with depth_b < depth_W (without W: the
//      last with depth_b < 100), otherwise W.
//    (a) merge_fg_kernel: atomicMin on best_fg [p] of  bits(depth + 0.0f) << 32 | entry  (depths are >= 0, so their
//        bits are monotone; + 0.0f folds -0; the CSR is in dict order, so the smaller entry is the earlier object);
//    (b) merge_bg_kernel: reads best_fg [p], applies the rule, atomicMax of entry + 1 on best_bg [p] (32 bits);
//    (c) merge_out_kernel: per pixel rgb u8 (float * 255, truncated: vmap.py:352 here), maskid, depth, winner.
//    Integer minima and maxima only: the result does not depend on the order the atomics arrive in.
#include "objnerf_render_body.h"
#include "objnerf_boxray.h"
#include "objnerf_wg.h"

namespace {
using namespace obj32n;

constexpr int MV_WG = 256;            // pixels / entries per workgroup of the count, emit and merge kernels
constexpr int MV_SCAN_WG = 1024;
constexpr int MV_BOX = 16;            // floats per box record: T_OC rows 0..2 [3][4] | extent / 2 [3] | unused
constexpr unsigned long long MV_NO_FG = ((unsigned long long)0x42C80000u << 32) | 0xFFFFFFFFull;   // bits(100.0f), no entry

bool mv_sizes_ok(const int64_t P, const int32_t K) { return P > 0 && P <= 0x7fffffff && K > 0 && K <= 65535; }
int64_t mv_blocks(const int64_t n) { return cdiv(n, MV_WG); }
int mv_num_cu() {
  int dev = 0, cu = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev);
  return cu > 0 ? cu : 256;
}

// -------------------------------------------------------------------------------------------------- 1. candidate rays
__device__ __forceinline__ BoxRay view_ray(const float* __restrict__ T_WC, const float* __restrict__ boxes, const int k,
                                           const float* __restrict__ dirs_C, const int64_t p) {
  const float* rec = boxes + (int64_t)k * MV_BOX;
  return box_ray(T_WC, rec, rec + 12, dirs_C[3 * p], dirs_C[3 * p + 1], dirs_C[3 * p + 2]);
}

// grid (nb, K): cnt [k][b] = the hits of object k among the pixels of block b
__global__ void __launch_bounds__(MV_WG) view_count_kernel(const int64_t P, const float* __restrict__ T_WC,
                                                           const float* __restrict__ boxes,
                                                           const float* __restrict__ dirs_C, int64_t* __restrict__ cnt) {
  const int k = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * MV_WG + threadIdx.x;
  const bool hit = p < P && view_ray(T_WC, boxes, k, dirs_C, p).hit;
  __shared__ int wcnt[MV_WG / 64];
  int total;
  wg_exclusive_flag<MV_WG>(hit, wcnt, total);
  if (threadIdx.x == 0) cnt[(int64_t)k * gridDim.x + blockIdx.x] = total;
}
// grid K: an object with at most one hit keeps none (n_rays <= 1, trainer.py:164-165 of the reference)
__global__ void __launch_bounds__(MV_WG) view_drop_kernel(const int64_t nb, int64_t* __restrict__ cnt) {
  int64_t* row = cnt + (int64_t)blockIdx.x * nb;
  int v = 0;                                              // (a block counts at most MV_WG, all of them at most P < 2^31)
  for (int64_t b = threadIdx.x; b < nb; b += MV_WG) v += (int)row[b];
  __shared__ int wsum[MV_WG / 64];
  const int total = wg_sum<MV_WG>(v, wsum);
  if (total > 1) return;                                  // (uniform over the workgroup)
  for (int64_t b = threadIdx.x; b < nb; b += MV_WG) row[b] = 0;
}
// the scanned counts (cnt [K * nb] exclusive, cnt [K * nb] = M) -> seg_off [K + 1]
__global__ void view_seg_off_kernel(const int K, const int64_t nb, const int64_t* __restrict__ cnt,
                                    int64_t* __restrict__ seg_off) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k <= K) seg_off[k] = cnt[(int64_t)k * nb];
}
__global__ void __launch_bounds__(MV_WG) view_emit_kernel(const int64_t P, const float* __restrict__ T_WC,
                                                          const float* __restrict__ boxes,
                                                          const float* __restrict__ dirs_C,
                                                          const int64_t* __restrict__ cnt, const int64_t M,
                                                          int32_t* __restrict__ pix, float* __restrict__ dirs_W,
                                                          float* __restrict__ near_o, float* __restrict__ far_o) {
  const int k = blockIdx.y;
  const int64_t nb = gridDim.x;
  const int64_t p = (int64_t)blockIdx.x * MV_WG + threadIdx.x;
  BoxRay b;
  b.hit = false;
  if (p < P) b = view_ray(T_WC, boxes, k, dirs_C, p);
  __shared__ int wcnt[MV_WG / 64];
  int total;
  const int64_t pos = cnt[(int64_t)k * nb + blockIdx.x] + wg_exclusive_flag<MV_WG>(b.hit, wcnt, total);
  // the end of THIS object's segment: a dropped object (all counts zeroed) owns no slot, its hits go nowhere
  const int64_t end = cnt[((int64_t)k + 1) * nb];
  if (b.hit && pos >= 0 && pos < end && pos < M) {
    pix[pos] = (int32_t)p;
    dirs_W[3 * pos] = b.dw[0]; dirs_W[3 * pos + 1] = b.dw[1]; dirs_W[3 * pos + 2] = b.dw[2];
    near_o[pos] = b.near_;
    far_o[pos] = b.far_;
  }
}

// ---------------------------------------------------------------------------------------------- 2. segmented render
struct SegRenderDev {
  int n_rows, n_bins; long n_tiles, M, u_rows;
  const float* params; long p_stride; const float* scale; const float* origin;
  const int64_t* rows;        // [n_rows][4]: seg_lo, seg_hi (entries of the CSR), u_lo (first row of u; < 0: seeded), draw
  const int32_t* tiles;       // [n_tiles][3]: arena row, first 16-ray group of the segment, groups
  const float* dirs_W; const float* near_; const float* far_; const float* u; uint64_t seed;
  float* depth; float* opacity; float* rgb;
  Layout L;
};

__global__ __launch_bounds__(256) void render_seg_kernel(const SegRenderDev a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const long t0 = a.n_tiles * (long)blockIdx.x / (long)gridDim.x, t1 = a.n_tiles * ((long)blockIdx.x + 1) / (long)gridDim.x;
  const float* sv = lds + sv_base(false);
  const float* wf = (const float*)__builtin_assume_aligned(lds + 4 * g * WROW + out_pos(c), 8);
  const float ox = a.origin[0], oy = a.origin[1], oz = a.origin[2];
  const int S = a.n_bins - 1;
  RenderDev d;
  d.n = 0; d.n_bins = a.n_bins; d.G = 0;
  d.params = nullptr; d.scale = nullptr; d.origin = a.origin;
  d.dirs_W = nullptr; d.near_ = nullptr; d.far_ = nullptr; d.u = nullptr; d.seed = a.seed; d.draw = 0;
  d.depth = nullptr; d.opacity = nullptr; d.rgb = nullptr; d.hfeat = nullptr; d.z_out = nullptr;
  d.L = a.L;
  int staged = -1;
  float scale = 1.0f;
  uint32_t st = 0;
  for (long t = t0; t < t1; ++t) {
    // every thread reads the same three words: row, first and ng are uniform over the workgroup
    const int row = __builtin_amdgcn_readfirstlane(a.tiles[3 * t]);
    const int first = __builtin_amdgcn_readfirstlane(a.tiles[3 * t + 1]);
    const int ng = __builtin_amdgcn_readfirstlane(a.tiles[3 * t + 2]);
    if (row < 0 || row >= a.n_rows || first < 0) continue;
    if (row != staged) {
      __syncthreads();        // every wave is done reading the image of the row before (banner: the restage hazard)
      stage_weights32(lds, a.params + (long)row * a.p_stride, a.L, false, tid, 256);
      __syncthreads();        // the new image is complete before any wave's next group reads it
      const int64_t* rr = a.rows + 4 * (long)row;
      long s0 = rr[0], s1 = rr[1];
      const long ulo = rr[2];
      s0 = s0 < 0 ? 0 : (s0 > a.M ? a.M : s0);              // a segment never leaves the CSR
      s1 = s1 < s0 ? s0 : (s1 > a.M ? a.M : s1);
      const bool inj = a.u != nullptr && ulo >= 0;
      if (inj && ulo + (s1 - s0) > a.u_rows) s1 = s0;        // nor its draws the rows of u: such a row renders nothing
      d.n = s1 - s0;
      d.dirs_W = a.dirs_W + 3 * s0; d.near_ = a.near_ + s0; d.far_ = a.far_ + s0;
      d.u = inj ? a.u + ulo * a.n_bins : nullptr;
      d.draw = (uint32_t)rr[3];
      d.depth = a.depth + s0; d.opacity = a.opacity + s0; d.rgb = a.rgb + 3 * s0;
      scale = a.scale[row];
      st = objrng::S_BOX_U | (d.draw << 3);
      staged = row;
    }
    if (d.n <= 0) continue;
    for (int gi = w; gi < ng; gi += 4)                       // a wave's groups; no barrier in here
      if (((long)first + gi) * 16 < d.n) render_group<false>(d, sv, wf, scale, ox, oy, oz, S, st, c, g, (long)first + gi);
  }
}

// ------------------------------------------------------------------------------------------------------- 3. merge
__device__ __forceinline__ int mv_seg_of(const int K, const int64_t* __restrict__ seg_off, const int64_t e) {
  int lo = 0, hi = K;                                       // the k with seg_off[k] <= e < seg_off[k + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_off[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}
// vmap.py:350 here (the masks of vmap.py:665,672) and the 100 the depth image starts from (train.py:566)
__device__ __forceinline__ bool mv_offered(const float d, const float op, const float nr, const float fr) {
  return !((d < nr) | (d > fr) | (op < 0.9f)) && d < 100.0f;
}

struct MergeDev {
  int64_t P, M; int K;
  const int64_t* seg_off; const int32_t* pix;
  const float* depth; const float* opacity; const float* rgb; const float* near_; const float* far_;
  const int32_t* info;        // [K][2]: background, the id written into maskid
  unsigned long long* best_fg; unsigned int* best_bg;
  uint8_t* out_rgb; int32_t* out_maskid; float* out_depth; int32_t* out_winner;
};

__global__ void __launch_bounds__(MV_WG) merge_init_kernel(const int64_t P, unsigned long long* __restrict__ best_fg,
                                                           unsigned int* __restrict__ best_bg) {
  const int64_t p = (int64_t)blockIdx.x * MV_WG + threadIdx.x;
  if (p < P) { best_fg[p] = MV_NO_FG; best_bg[p] = 0u; }
}
template <bool BG>
__global__ void __launch_bounds__(MV_WG) merge_entry_kernel(const MergeDev a) {
  const int64_t e = (int64_t)blockIdx.x * MV_WG + threadIdx.x;
  if (e >= a.M) return;
  const int k = mv_seg_of(a.K, a.seg_off, e);
  if ((a.info[2 * k] != 0) != BG) return;
  const int64_t p = a.pix[e];
  if (p < 0 || p >= a.P) return;
  const float d = a.depth[e];
  if (!mv_offered(d, a.opacity[e], a.near_[e], a.far_[e])) return;
  const unsigned int bits = __float_as_uint(d + 0.0f);
  if (!BG) {
    atomicMin(a.best_fg + p, ((unsigned long long)bits << 32) | (unsigned long long)(unsigned int)e);
  } else {
    // best_fg is final: launch (a) is complete before this one starts on the stream
    const unsigned long long key = a.best_fg[p];
    const unsigned int ew = (unsigned int)key;
    const float dw = __uint_as_float((unsigned int)(key >> 32));
    const bool after = ew == 0xFFFFFFFFu || (unsigned int)e > ew;        // b's object comes after W's in dict order
    if (after && (d + 0.0f) < dw) atomicMax(a.best_bg + p, (unsigned int)e + 1u);
  }
}
__global__ void __launch_bounds__(MV_WG) merge_out_kernel(const MergeDev a) {
  const int64_t p = (int64_t)blockIdx.x * MV_WG + threadIdx.x;
  if (p >= a.P) return;
  const unsigned long long key = a.best_fg[p];
  const unsigned int ew = (unsigned int)key, eb = a.best_bg[p];
  const int64_t e = eb != 0u ? (int64_t)eb - 1 : (ew != 0xFFFFFFFFu ? (int64_t)ew : -1);
  a.out_depth[p] = __uint_as_float((unsigned int)(key >> 32));
  a.out_winner[p] = (int32_t)e;
  const bool painted = e >= 0 && e < a.M;
  a.out_maskid[p] = painted ? a.info[2 * mv_seg_of(a.K, a.seg_off, e) + 1] : 0;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    a.out_rgb[3 * p + j] = painted ? (uint8_t)(int)(a.rgb[3 * e + j] * 255.0f) : (uint8_t)0;      // truncation
}

}  // namespace

extern "C" {

size_t objnerf_view_rays_workspace_bytes(int64_t P, int32_t K) {
  if (!mv_sizes_ok(P, K)) return 0;
  return align256(((size_t)K * (size_t)mv_blocks(P) + 1) * sizeof(int64_t));
}

int objnerf_view_rays_count(int64_t P, int32_t K, const float* T_WC, const float* boxes, const float* dirs_C, void* ws,
                            size_t ws_bytes, int64_t* seg_off, void* stream) {
  (void)hipGetLastError();
  if (!mv_sizes_ok(P, K) || !T_WC || !boxes || !dirs_C || !ws || !seg_off) return OBJNERF_EINVAL;
  if (ws_bytes < objnerf_view_rays_workspace_bytes(P, K)) return OBJNERF_EINVAL;
  const int64_t nb = mv_blocks(P);
  int64_t* cnt = (int64_t*)ws;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(view_count_kernel, dim3((unsigned)nb, (unsigned)K), dim3(MV_WG), 0, st, P, T_WC, boxes, dirs_C, cnt);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(view_drop_kernel, dim3((unsigned)K), dim3(MV_WG), 0, st, nb, cnt);
  CHECK_LAUNCH();
  hipLaunchKernelGGL((wg_scan_kernel<MV_SCAN_WG, 1, int64_t>), dim3(1), dim3(MV_SCAN_WG), 0, st, cnt, (int64_t)K * nb,
                     cnt + (int64_t)K * nb);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(view_seg_off_kernel, dim3((unsigned)cdiv(K + 1, 256)), dim3(256), 0, st, (int)K, nb,
                     (const int64_t*)cnt, seg_off);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_view_rays_emit(int64_t P, int32_t K, const float* T_WC, const float* boxes, const float* dirs_C, const void* ws,
                           size_t ws_bytes, int64_t M, int32_t* pix, float* dirs_W, float* near, float* far, void* stream) {
  (void)hipGetLastError();
  if (!mv_sizes_ok(P, K) || !T_WC || !boxes || !dirs_C || !ws || M < 0 || M >= (1LL << 32)) return OBJNERF_EINVAL;
  if (ws_bytes < objnerf_view_rays_workspace_bytes(P, K)) return OBJNERF_EINVAL;
  if (M == 0) return OBJNERF_OK;
  if (!pix || !dirs_W || !near || !far) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(view_emit_kernel, dim3((unsigned)mv_blocks(P), (unsigned)K), dim3(MV_WG), 0, (hipStream_t)stream, P,
                     T_WC, boxes, dirs_C, (const int64_t*)ws, M, pix, dirs_W, near, far);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_render_fwd_segmented(const objnerf_net* net, int32_t n_rows, int64_t n_tiles, int32_t n_bins, int64_t M,
                                 const float* params, int64_t p_stride, const float* scale, const float* origin,
                                 const int64_t* rows, const int32_t* tiles, const float* dirs_W, const float* near,
                                 const float* far, const float* u, int64_t u_rows, uint64_t seed, float* out_depth,
                                 float* out_opacity, float* out_rgb, int32_t workgroups, void* stream) {
  (void)hipGetLastError();
  if (!net || n_rows <= 0 || n_tiles < 0 || n_bins < 2 || M < 0 || M >= (1LL << 32) || p_stride <= 0 || workgroups < 0 ||
      u_rows < 0)
    return OBJNERF_EINVAL;
  if (net->hidden != 32 || net->n_freqs != 6) return OBJNERF_ENOTSUP;      // (wider networks: the layer-wise chain)
  if (n_tiles == 0 || M == 0) return OBJNERF_OK;
  if (!params || !scale || !origin || !rows || !tiles || !dirs_W || !near || !far || !out_depth || !out_opacity || !out_rgb)
    return OBJNERF_EINVAL;
  SegRenderDev d;
  d.n_rows = n_rows; d.n_bins = n_bins; d.n_tiles = (long)n_tiles; d.M = (long)M; d.u_rows = u ? (long)u_rows : 0;
  d.params = params; d.p_stride = (long)p_stride; d.scale = scale; d.origin = origin; d.rows = rows; d.tiles = tiles;
  d.dirs_W = dirs_W; d.near_ = near; d.far_ = far; d.u = u; d.seed = seed;
  d.depth = out_depth; d.opacity = out_opacity; d.rgb = out_rgb;
  d.L = make_layout(net->feat_dim);
  // two workgroups of 4 waves per CU (the image is 60 KB), never more than there are tiles
  int64_t G = workgroups > 0 ? (int64_t)workgroups : 2 * (int64_t)mv_num_cu();
  if (G > n_tiles) G = n_tiles;
  hipLaunchKernelGGL(render_seg_kernel, dim3((unsigned)G), dim3(256), (size_t)img_floats(false) * 4, (hipStream_t)stream, d);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_view_merge(int64_t P, int32_t K, int64_t M, const int64_t* seg_off, const int32_t* pix, const float* depth,
                       const float* opacity, const float* rgb, const float* near, const float* far, const int32_t* info,
                       int32_t any_background, uint64_t* best_fg, uint32_t* best_bg, uint8_t* out_rgb, int32_t* out_maskid,
                       float* out_depth, int32_t* out_winner, void* stream) {
  (void)hipGetLastError();
  if (!mv_sizes_ok(P, K) || M < 0 || M >= (1LL << 32) || !seg_off || !info || !best_fg || !best_bg || !out_rgb ||
      !out_maskid || !out_depth || !out_winner)
    return OBJNERF_EINVAL;
  if (M > 0 && (!pix || !depth || !opacity || !rgb || !near || !far)) return OBJNERF_EINVAL;
  MergeDev a;
  a.P = P; a.M = M; a.K = K; a.seg_off = seg_off; a.pix = pix; a.depth = depth; a.opacity = opacity; a.rgb = rgb;
  a.near_ = near; a.far_ = far; a.info = info; a.best_fg = (unsigned long long*)best_fg; a.best_bg = best_bg;
  a.out_rgb = out_rgb; a.out_maskid = out_maskid; a.out_depth = out_depth; a.out_winner = out_winner;
  hipStream_t st = (hipStream_t)stream;
  const dim3 wg(MV_WG), gp((unsigned)mv_blocks(P)), ge((unsigned)mv_blocks(M > 0 ? M : 1));
  hipLaunchKernelGGL(merge_init_kernel, gp, wg, 0, st, P, a.best_fg, a.best_bg);
  CHECK_LAUNCH();
  if (M > 0) {
    hipLaunchKernelGGL((merge_entry_kernel<false>), ge, wg, 0, st, a);
    CHECK_LAUNCH();
    if (any_background) {
      hipLaunchKernelGGL((merge_entry_kernel<true>), ge, wg, 0, st, a);
      CHECK_LAUNCH();
    }
  }
  hipLaunchKernelGGL(merge_out_kernel, gp, wg, 0, st, a);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

}  // extern "C"
