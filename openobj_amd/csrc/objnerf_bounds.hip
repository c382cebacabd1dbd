// Object bounds from keyframes: sceneObject.get_bound (vmap.py:287-384), which the reference runs on the CPU through
// open3d (back-projection + voxel_down_sample) and trimesh (oriented_bounds), one object at a time.
//
// (a) Voxel centroids of K objects' keyframe point clouds, read straight from the device keyframe stores:
//   voxel_scan_kernel      one workgroup per (object, keyframe, tile of 256 columns x 32 rows): a lane per column
//                          reads its 32 depths and state bytes, keeps pixels with state == 1 and depth > 0 (NaN fails
//                          that test, as open3d's), writes the count of every (row, column chunk) segment and the
//                          tile's min / max of the back-projected points (min / max are order-free: exact);
//   voxel_finish_kernel    one workgroup per object: min / max over its tiles, exclusive offsets of the segments in
//                          the reference's point order (keyframe, row i, column j), the object's point count;
//   voxel_emit_kernel      recomputes each point (same code, same rounding) and writes it with its voxel key at
//                          base + segment offset + prefix in the row: the compacted cloud is in the reference's order;
//   (host: torch.sort(keys, stable=True) -- equal keys keep that order)
//   voxel_heads_kernel / wg_scan_kernel (objnerf_wg.h) / voxel_centroid_kernel
//                          voxel heads of the sorted keys, their offsets, and for every head the in-order double sum
//                          of its points / count -- open3d's AddPoint / GetAveragePoint.
// (b) Oriented-box search over K objects' hull candidates (normal n, edge e) in one launch:
//   obb_search_kernel      hull vertices in LDS (tiled past OBB_TILE); per candidate u = e projected onto the plane
//                          normal to n, normalised, v = n x u; volume = product of the vertices' extents on (u, v, n)
//                          (area of the (u, v) rectangle for a coplanar set); a deterministic (volume, index) minimum
//                          per workgroup;
//   obb_pick_kernel        one thread per object: the minimum over its workgroups, then that box's axes, extents and
//                          centre.
// No float atomics anywhere: every output is a fixed function of the inputs, byte-identical from call to call.
// The per-point arithmetic is fp64 without contraction (the Makefile builds with -ffp-contract=off): voxel membership
// is then exactly that of a numpy restatement of the same formulas.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "objnerf_wg.h"

namespace {

constexpr int VX_WG = 256;            // lanes = columns of a tile
constexpr int VX_BY = 32;             // rows of a tile
constexpr int VX_SCAN_WG = 1024;
constexpr int VX_HEAD_WG = 256;
constexpr int VX_HEAD_PER = 4;        // sorted keys per thread of the head kernels
constexpr int VX_HEAD_BLOCK = VX_HEAD_WG * VX_HEAD_PER;
constexpr int OBB_WG = 256;
constexpr int OBB_TILE = 2048;        // hull vertices per LDS tile (48 KiB: 3 workgroups per CU)
constexpr int KEY_SHIFT = 42;         // sort key = (object in chunk) << 42 | linear voxel index

struct VxLayout {
  long nxc, nyb, ntiles, rows;        // column chunks, row bands, tiles per keyframe, segments per object
  size_t counts, offsets, minmax, total;
};

inline VxLayout vx_layout(int K, int F, int W, int H) {
  VxLayout L;
  L.nxc = (W + VX_WG - 1) / VX_WG;
  L.nyb = (H + VX_BY - 1) / VX_BY;
  L.ntiles = L.nxc * L.nyb;
  L.rows = (long)F * H * L.nxc;
  size_t o = 0;
  L.counts = o;  o += align256(sizeof(int32_t) * (size_t)K * L.rows);
  L.offsets = o; o += align256(sizeof(int64_t) * (size_t)K * L.rows);
  L.minmax = o;  o += align256(sizeof(double) * 6 * (size_t)K * F * L.ntiles);
  L.total = o;
  return L;
}

// pixel (row i, column j) of keyframe slot kf with depth z > 0 -> world point: open3d's
// CreatePointCloudFromFloatDepthImage: x = (j - cx) z / fx, y = (i - cy) z / fy, p = camera_pose (x, y, z, 1);
// every product and sum rounded on its own (no FMA), evaluated left to right
__device__ __forceinline__ void backproject(const double* __restrict__ P, const objnerf_voxel_args& a, const int i,
                                            const int j, const float zf, double p[3]) {
  const double z = (double)zf;
  const double x = __ddiv_rn(__dmul_rn(__dsub_rn((double)j, a.cx), z), a.fx);
  const double y = __ddiv_rn(__dmul_rn(__dsub_rn((double)i, a.cy), z), a.fy);
#pragma unroll
  for (int r = 0; r < 3; ++r)
    p[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(P[4 * r], x), __dmul_rn(P[4 * r + 1], y)), __dmul_rn(P[4 * r + 2], z)),
                     P[4 * r + 3]);
}

// the lane's column of a tile: depths and "this object" flags of rows y0 .. y0 + VX_BY - 1 (false past H)
__device__ __forceinline__ void load_column(const objnerf_kf_store& s, const long kf, const int x, const int y0,
                                            const int W, const int H, float d[VX_BY], bool m[VX_BY]) {
  const long pix = (kf * W + x) * (long)H + y0;          // store layout [F][W][H] (the image transposed)
  const float* dp = s.depth + pix;
  const uint8_t* sp = s.rgbs + pix * 4;
  if (y0 + VX_BY <= H && (H & 3) == 0) {                  // 16-byte aligned: 8 + 8 vector loads per lane
#pragma unroll
    for (int q = 0; q < VX_BY / 4; ++q) {
      const float4 dv = *(const float4*)(dp + 4 * q);
      const uint4 sv = *(const uint4*)(sp + 16 * q);
      d[4 * q] = dv.x; d[4 * q + 1] = dv.y; d[4 * q + 2] = dv.z; d[4 * q + 3] = dv.w;
      m[4 * q] = (sv.x >> 24) == 1u; m[4 * q + 1] = (sv.y >> 24) == 1u;
      m[4 * q + 2] = (sv.z >> 24) == 1u; m[4 * q + 3] = (sv.w >> 24) == 1u;
    }
  } else {
#pragma unroll
    for (int r = 0; r < VX_BY; ++r) {
      const bool in = y0 + r < H;
      d[r] = in ? dp[r] : 0.f;
      m[r] = in && sp[4 * r + 3] == 1;
    }
  }
}

// The same column of a cropped store (ABI 13): slot kf holds the pixels of its rect {x0, y0, cw, ch} only, pixel (x, y) at
// element (x - x0) * ch + (y - y0); every other pixel of the image reads as "not this object" without touching memory.
// The element index is also held below the slot's capacity, so that a rect the caller corrupted cannot leave the arena.
__device__ __forceinline__ void load_column(const objnerf_kf_crops& s, const long kf, const int x, const int y0,
                                            const int W, const int H, float d[VX_BY], bool m[VX_BY]) {
  const int4 rc = *(const int4*)(s.rect + kf * 4);
  const uint8_t* sp = s.base + kf * s.cap * 8;
  const float* dp = (const float*)(sp + s.cap * 4);
  const int cx = x - rc.x;
  const bool colin = cx >= 0 && cx < rc.z;
#pragma unroll
  for (int r = 0; r < VX_BY; ++r) {
    const int cy = y0 + r - rc.y;
    const long e = (long)cx * rc.w + cy;
    const bool in = colin && y0 + r < H && cy >= 0 && cy < rc.w && e < s.cap;
    d[r] = in ? dp[e] : 0.f;
    m[r] = in && sp[4 * e + 3] == 1;
  }
}

// the tile's rectangle of columns x .. x + VX_WG - 1, rows y0 .. y0 + VX_BY - 1 holds no pixel of slot kf's crop
__device__ __forceinline__ bool tile_outside(const objnerf_kf_crops& s, const long kf, const int x_lo, const int y0) {
  const int4 rc = *(const int4*)(s.rect + kf * 4);
  return x_lo >= rc.x + rc.z || x_lo + VX_WG <= rc.x || y0 >= rc.y + rc.w || y0 + VX_BY <= rc.y;
}

// CROP: the objects' stores are a.crops (objnerf_kf_crops), else a.table (objnerf_kf_store)
template <bool CROP> struct VxStore;
template <> struct VxStore<false> {
  typedef objnerf_kf_store type;
  static __device__ __forceinline__ type of(const objnerf_voxel_args& a, const int k) { return a.table[k]; }
};
template <> struct VxStore<true> {
  typedef objnerf_kf_crops type;
  static __device__ __forceinline__ type of(const objnerf_voxel_args& a, const int k) { return a.crops[k]; }
};

template <bool CROP>
__global__ void __launch_bounds__(VX_WG) voxel_scan_kernel(const objnerf_voxel_args a, char* __restrict__ ws,
                                                           const VxLayout L) {
  const int k = blockIdx.z, kf = blockIdx.y;
  if (kf >= a.n_keyframes[k]) return;                     // only the live slots are read
  const int tile = blockIdx.x, xc = tile % L.nxc, yb = tile / L.nxc;
  const int x = xc * VX_WG + threadIdx.x, y0 = yb * VX_BY;
  const typename VxStore<CROP>::type s = VxStore<CROP>::of(a, k);
  if constexpr (CROP) {
    if (tile_outside(s, kf, xc * VX_WG, y0)) {            // nothing of the crop here: no points, and nothing is loaded
      int32_t* counts = (int32_t*)(ws + L.counts) + (long)k * L.rows;
      if (threadIdx.x < VX_BY && y0 + threadIdx.x < a.H) counts[((long)kf * a.H + y0 + threadIdx.x) * L.nxc + xc] = 0;
      if (threadIdx.x < 6)
        ((double*)(ws + L.minmax))[(((long)k * a.F + kf) * L.ntiles + tile) * 6 + threadIdx.x] =
            threadIdx.x < 3 ? INFINITY : -INFINITY;
      return;
    }
  }
  const double* P = a.camera_pose + ((long)k * a.F + kf) * 16;
  float d[VX_BY];
  bool m[VX_BY];
  const bool col = x < a.W;
  if (col) load_column(s, kf, x, y0, a.W, a.H, d, m);
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  __shared__ int wcnt[VX_WG / 64][VX_BY];
  __shared__ double red[VX_WG / 64][6];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < VX_BY; ++r) {
    const bool ok = col && m[r] && d[r] > 0.f;
    const unsigned long long b = __ballot(ok);
    if (lane == 0) wcnt[wv][r] = __popcll(b);
    if (ok) {
      double p[3];
      backproject(P, a, y0 + r, x, d[r], p);
#pragma unroll
      for (int c = 0; c < 3; ++c) { mn[c] = fmin(mn[c], p[c]); mx[c] = fmax(mx[c], p[c]); }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    for (int o = 32; o > 0; o >>= 1) {
      mn[c] = fmin(mn[c], __shfl_xor(mn[c], o));
      mx[c] = fmax(mx[c], __shfl_xor(mx[c], o));
    }
  if (lane == 0)
    for (int c = 0; c < 3; ++c) { red[wv][c] = mn[c]; red[wv][3 + c] = mx[c]; }
  __syncthreads();
  int32_t* counts = (int32_t*)(ws + L.counts) + (long)k * L.rows;
  if (threadIdx.x < VX_BY && y0 + threadIdx.x < a.H) {
    int c = 0;
    for (int w = 0; w < VX_WG / 64; ++w) c += wcnt[w][threadIdx.x];
    counts[((long)kf * a.H + y0 + threadIdx.x) * L.nxc + xc] = c;
  }
  if (threadIdx.x < 6) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < VX_WG / 64; ++w) v = threadIdx.x < 3 ? fmin(v, red[w][threadIdx.x]) : fmax(v, red[w][threadIdx.x]);
    double* mm = (double*)(ws + L.minmax) + (((long)k * a.F + kf) * L.ntiles + tile) * 6;
    mm[threadIdx.x] = v;
  }
}

// one workgroup per object: exclusive offsets of its segments (keyframe, row, column chunk) and min / max over tiles
__global__ void __launch_bounds__(VX_SCAN_WG) voxel_finish_kernel(const objnerf_voxel_args a, char* __restrict__ ws,
                                                                  const VxLayout L, int64_t* __restrict__ out_total,
                                                                  double* __restrict__ out_minmax) {
  const int k = blockIdx.x;
  const int nk = a.n_keyframes[k];
  const long n = (long)nk * a.H * L.nxc;                  // the live slots' segments: a prefix of the object's array
  const int32_t* counts = (const int32_t*)(ws + L.counts) + (long)k * L.rows;
  int64_t* offs = (int64_t*)(ws + L.offsets) + (long)k * L.rows;
  int64_t total[1];
  wg_scan_exclusive<VX_SCAN_WG, 1>(counts, offs, n, total);
  if (threadIdx.x == 0) out_total[k] = total[0];
  if (threadIdx.x < 6) {
    const double* mm = (const double*)(ws + L.minmax) + (long)k * a.F * L.ntiles * 6;
    const bool is_min = threadIdx.x < 3;
    double v = is_min ? INFINITY : -INFINITY;
    for (long t = 0; t < (long)nk * L.ntiles; ++t)
      v = is_min ? fmin(v, mm[t * 6 + threadIdx.x]) : fmax(v, mm[t * 6 + threadIdx.x]);
    out_minmax[k * 6 + threadIdx.x] = v;
  }
}

template <bool CROP>
__global__ void __launch_bounds__(VX_WG) voxel_emit_kernel(const objnerf_voxel_args a, const char* __restrict__ ws,
                                                           const VxLayout L, const int k0, const int64_t* __restrict__ base,
                                                           const double* __restrict__ vmin,
                                                           const int64_t* __restrict__ dims, const int64_t n_points,
                                                           double* __restrict__ out_pts, int64_t* __restrict__ out_keys) {
  const int kl = blockIdx.z, k = k0 + kl, kf = blockIdx.y;
  if (kf >= a.n_keyframes[k]) return;
  const int tile = blockIdx.x, xc = tile % L.nxc, yb = tile / L.nxc;
  const int x = xc * VX_WG + threadIdx.x, y0 = yb * VX_BY;
  const int32_t* counts = (const int32_t*)(ws + L.counts) + (long)k * L.rows;
  const int64_t* offs = (const int64_t*)(ws + L.offsets) + (long)k * L.rows;
  const int r_t = threadIdx.x;
  const bool any = r_t < VX_BY && y0 + r_t < a.H && counts[((long)kf * a.H + y0 + r_t) * L.nxc + xc] != 0;
  if (!__syncthreads_or(any)) return;                    // most tiles of a small object hold none of its pixels
  const typename VxStore<CROP>::type s = VxStore<CROP>::of(a, k);
  const double* P = a.camera_pose + ((long)k * a.F + kf) * 16;
  float d[VX_BY];
  bool m[VX_BY];
  const bool col = x < a.W;
  if (col) load_column(s, kf, x, y0, a.W, a.H, d, m);
  const double v = a.voxel;
  const double lo[3] = {vmin[3 * k], vmin[3 * k + 1], vmin[3 * k + 2]};
  const int64_t nx = dims[2 * k], ny = dims[2 * k + 1];
  __shared__ int wcnt[VX_WG / 64][VX_BY];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long bal[VX_BY];
#pragma unroll
  for (int r = 0; r < VX_BY; ++r) {
    bal[r] = __ballot(col && m[r] && d[r] > 0.f);
    if (lane == 0) wcnt[wv][r] = __popcll(bal[r]);
  }
  __syncthreads();                                       // (32 rows through one barrier: wg_exclusive_flag's two halves)
#pragma unroll
  for (int r = 0; r < VX_BY; ++r) {
    if (!((bal[r] >> lane) & 1ull)) continue;
    int pre = wave_rank(bal[r]);
    for (int w = 0; w < wv; ++w) pre += wcnt[w][r];
    const int64_t pos = base[k] + offs[((long)kf * a.H + y0 + r) * L.nxc + xc] + pre;
    if (pos < 0 || pos >= n_points) continue;             // (cannot happen with the scan's counts; never write past)
    double p[3];
    backproject(P, a, y0 + r, x, d[r], p);
    int64_t ix[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) ix[c] = (int64_t)floor(__ddiv_rn(__dsub_rn(p[c], lo[c]), v));
    out_pts[3 * pos] = p[0]; out_pts[3 * pos + 1] = p[1]; out_pts[3 * pos + 2] = p[2];
    out_keys[pos] = ((int64_t)kl << KEY_SHIFT) | (ix[0] + nx * (ix[1] + ny * ix[2]));
  }
}

__device__ __forceinline__ bool is_head(const int64_t* __restrict__ keys, const int64_t i) {
  return i == 0 || keys[i] != keys[i - 1];
}

__global__ void __launch_bounds__(VX_HEAD_WG) voxel_heads_kernel(const int64_t n, const int64_t* __restrict__ keys,
                                                                 int64_t* __restrict__ blk) {
  const int64_t i0 = (int64_t)blockIdx.x * VX_HEAD_BLOCK + threadIdx.x * VX_HEAD_PER;
  int c = 0;
  for (int q = 0; q < VX_HEAD_PER; ++q)
    if (i0 + q < n) c += is_head(keys, i0 + q);
  __shared__ int wsum[VX_HEAD_WG / 64];
  const int t = wg_sum<VX_HEAD_WG>(c, wsum);
  if (threadIdx.x == 0) blk[blockIdx.x] = t;
}

__global__ void __launch_bounds__(VX_HEAD_WG) voxel_centroid_kernel(
    const int64_t n, const int64_t* __restrict__ keys, const int64_t* __restrict__ perm, const double* __restrict__ pts,
    const int64_t* __restrict__ blk, const int64_t max_voxels, double* __restrict__ out_cen,
    int64_t* __restrict__ out_keys, int64_t* __restrict__ out_first) {
  const int64_t i0 = (int64_t)blockIdx.x * VX_HEAD_BLOCK + threadIdx.x * VX_HEAD_PER;
  bool h[VX_HEAD_PER];
  int c = 0;
  for (int q = 0; q < VX_HEAD_PER; ++q) {
    h[q] = i0 + q < n && is_head(keys, i0 + q);
    c += h[q];
  }
  __shared__ int wsum[VX_HEAD_WG / 64];
  int total;
  int64_t j = blk[blockIdx.x] + wg_exclusive<VX_HEAD_WG>(c, wsum, total);
  for (int q = 0; q < VX_HEAD_PER; ++q) {
    if (!h[q]) continue;
    const int64_t i = i0 + q, key = keys[i];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int64_t e = i;
    for (; e < n && keys[e] == key; ++e) {                // in the points' order: the reference's AddPoint sequence
      const int64_t p = perm[e];
      s0 = __dadd_rn(s0, pts[3 * p]); s1 = __dadd_rn(s1, pts[3 * p + 1]); s2 = __dadd_rn(s2, pts[3 * p + 2]);
    }
    const double cnt = (double)(e - i);
    if (j < max_voxels) {
      out_cen[3 * j] = __ddiv_rn(s0, cnt); out_cen[3 * j + 1] = __ddiv_rn(s1, cnt); out_cen[3 * j + 2] = __ddiv_rn(s2, cnt);
      out_keys[j] = key & ((1ll << KEY_SHIFT) - 1);
      if (i == 0 || (keys[i - 1] >> KEY_SHIFT) != (key >> KEY_SHIFT)) out_first[key >> KEY_SHIFT] = j;
    }
    ++j;
  }
}

// ---------------------------------------------------------------------------------------------- oriented-box search
struct ObbAxes { double u[3], v[3], n[3]; bool ok; };

__device__ __forceinline__ double dot3(const double* a, const double* b) {
  return __dadd_rn(__dadd_rn(__dmul_rn(a[0], b[0]), __dmul_rn(a[1], b[1])), __dmul_rn(a[2], b[2]));
}

// candidate c of object k: n = normals[cand[c].x], e = verts[edge].b - verts[edge].a;  u = normalise(e - (e.n) n)
__device__ __forceinline__ ObbAxes obb_axes(const objnerf_obb_args& a, const int64_t c, const int64_t v0) {
  ObbAxes r;
  const int32_t ni = a.cand[2 * c], ei = a.cand[2 * c + 1];
  const int32_t ia = a.edges[2 * ei], ib = a.edges[2 * ei + 1];
  double n[3], e[3];
  for (int q = 0; q < 3; ++q) {
    n[q] = a.normals[3 * (int64_t)ni + q];
    e[q] = __dsub_rn(a.verts[3 * (v0 + ib) + q], a.verts[3 * (v0 + ia) + q]);
  }
  const double en = dot3(e, n);
  double u[3];
  for (int q = 0; q < 3; ++q) u[q] = __dsub_rn(e[q], __dmul_rn(en, n[q]));
  const double len = sqrt(dot3(u, u)), elen = sqrt(dot3(e, e));
  r.ok = len > 1e-12 * elen && len > 0.0;
  const double inv = r.ok ? 1.0 / len : 0.0;
  for (int q = 0; q < 3; ++q) { r.u[q] = u[q] * inv; r.n[q] = n[q]; }
  r.v[0] = __dsub_rn(__dmul_rn(n[1], r.u[2]), __dmul_rn(n[2], r.u[1]));
  r.v[1] = __dsub_rn(__dmul_rn(n[2], r.u[0]), __dmul_rn(n[0], r.u[2]));
  r.v[2] = __dsub_rn(__dmul_rn(n[0], r.u[1]), __dmul_rn(n[1], r.u[0]));
  return r;
}

__device__ __forceinline__ bool better(const double va, const int64_t ia, const double vb, const int64_t ib) {
  return va < vb || (va == vb && ia < ib);
}

__global__ void __launch_bounds__(OBB_WG) obb_search_kernel(const objnerf_obb_args a, double* __restrict__ part_vol,
                                                            int64_t* __restrict__ part_idx) {
  const int k = blockIdx.y;
  const int64_t v0 = a.vert_off[k], nv = a.vert_off[k + 1] - v0;
  const int64_t c0 = a.cand_off[k], nc = a.cand_off[k + 1] - c0;
  __shared__ double sv[OBB_TILE * 3];
  const bool single = nv <= OBB_TILE;
  if (single) {
    for (int64_t t = threadIdx.x; t < 3 * nv; t += OBB_WG) sv[t] = a.verts[3 * v0 + t];
    __syncthreads();
  }
  double best = INFINITY;
  int64_t best_i = INT64_MAX;
  for (int64_t b = (int64_t)blockIdx.x * OBB_WG; b < nc; b += (int64_t)gridDim.x * OBB_WG) {   // uniform loop
    const int64_t c = b + threadIdx.x;
    ObbAxes ax;
    ax.ok = false;
    if (c < nc) ax = obb_axes(a, c0 + c, v0);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t t0 = 0; t0 < nv; t0 += OBB_TILE) {
      const int64_t tn = nv - t0 < OBB_TILE ? nv - t0 : OBB_TILE;
      if (!single) {
        __syncthreads();
        for (int64_t t = threadIdx.x; t < 3 * tn; t += OBB_WG) sv[t] = a.verts[3 * (v0 + t0) + t];
        __syncthreads();
      }
      if (ax.ok)
        for (int64_t t = 0; t < tn; ++t) {
          const double* p = sv + 3 * t;
          const double pu = dot3(p, ax.u), pv = dot3(p, ax.v), pn = dot3(p, ax.n);
          lo[0] = fmin(lo[0], pu); hi[0] = fmax(hi[0], pu);
          lo[1] = fmin(lo[1], pv); hi[1] = fmax(hi[1], pv);
          lo[2] = fmin(lo[2], pn); hi[2] = fmax(hi[2], pn);
        }
    }
    if (ax.ok) {
      const double area = __dmul_rn(__dsub_rn(hi[0], lo[0]), __dsub_rn(hi[1], lo[1]));
      const double vol = a.mode[k] == 1 ? area : __dmul_rn(area, __dsub_rn(hi[2], lo[2]));
      if (better(vol, c, best, best_i)) { best = vol; best_i = c; }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(best, o);
    const int64_t oi = __shfl_xor(best_i, o);
    if (better(ov, oi, best, best_i)) { best = ov; best_i = oi; }
  }
  __shared__ double rv[OBB_WG / 64];
  __shared__ int64_t ri[OBB_WG / 64];
  if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = best; ri[threadIdx.x >> 6] = best_i; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < OBB_WG / 64; ++w)
      if (better(rv[w], ri[w], best, best_i)) { best = rv[w]; best_i = ri[w]; }
    part_vol[(int64_t)k * gridDim.x + blockIdx.x] = best;
    part_idx[(int64_t)k * gridDim.x + blockIdx.x] = best_i;
  }
}

// out[k][16] = R row-major (columns u, v, n), extents (u, v, n), centre, criterion; criterion = +inf: no candidate
__global__ void obb_pick_kernel(const objnerf_obb_args a, const int n_split, const double* __restrict__ part_vol,
                                const int64_t* __restrict__ part_idx, double* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.K) return;
  double best = INFINITY;
  int64_t bi = INT64_MAX;
  for (int s = 0; s < n_split; ++s)
    if (better(part_vol[(int64_t)k * n_split + s], part_idx[(int64_t)k * n_split + s], best, bi)) {
      best = part_vol[(int64_t)k * n_split + s]; bi = part_idx[(int64_t)k * n_split + s];
    }
  double* o = out + 16 * (int64_t)k;
  for (int q = 0; q < 16; ++q) o[q] = 0.0;
  o[15] = best;
  if (bi == INT64_MAX) { o[15] = INFINITY; return; }
  const int64_t v0 = a.vert_off[k], nv = a.vert_off[k + 1] - v0;
  const ObbAxes ax = obb_axes(a, a.cand_off[k] + bi, v0);
  const double* axes[3] = {ax.u, ax.v, ax.n};
  for (int q = 0; q < 3; ++q) {
    double lo = INFINITY, hi = -INFINITY;
    for (int64_t t = 0; t < nv; ++t) {
      const double pq = dot3(a.verts + 3 * (v0 + t), axes[q]);
      lo = fmin(lo, pq); hi = fmax(hi, pq);
    }
    const double mid = 0.5 * (lo + hi);
    for (int r = 0; r < 3; ++r) {
      o[3 * r + q] = axes[q][r];
      o[12 + r] += axes[q][r] * mid;
    }
    o[9 + q] = hi - lo;
  }
}

}  // namespace

extern "C" {

size_t objnerf_voxel_workspace_bytes(int32_t K, int32_t F, int32_t W, int32_t H) {
  if (K <= 0 || F <= 0 || W <= 0 || H <= 0) return 0;
  return vx_layout(K, F, W, H).total;
}

int objnerf_voxel_scan(const objnerf_voxel_args* a, void* ws, size_t ws_bytes, int64_t* out_total, double* out_minmax,
                       void* stream) {
  if (!a || !ws || !out_total || !out_minmax || (!a->table && !a->crops) || !a->n_keyframes || !a->camera_pose)
    return OBJNERF_EINVAL;
  if (a->K <= 0 || a->K > 65535 || a->F <= 0 || a->F > 65535 || a->W <= 0 || a->H <= 0 || !(a->voxel > 0.0))
    return OBJNERF_EINVAL;
  const VxLayout L = vx_layout(a->K, a->F, a->W, a->H);
  if (ws_bytes < L.total) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(a->crops ? voxel_scan_kernel<true> : voxel_scan_kernel<false>,
                     dim3((unsigned)L.ntiles, (unsigned)a->F, (unsigned)a->K), dim3(VX_WG), 0, (hipStream_t)stream, *a,
                     (char*)ws, L);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(voxel_finish_kernel, dim3((unsigned)a->K), dim3(VX_SCAN_WG), 0, (hipStream_t)stream, *a, (char*)ws,
                     L, out_total, out_minmax);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_voxel_emit(const objnerf_voxel_args* a, const void* ws, size_t ws_bytes, int32_t k0, int32_t k1,
                       const int64_t* base, const double* vmin, const int64_t* dims, int64_t n_points, double* out_pts,
                       int64_t* out_keys, void* stream) {
  if (!a || !ws || !base || !vmin || !dims || (!a->table && !a->crops) || !a->n_keyframes || !a->camera_pose)
    return OBJNERF_EINVAL;
  if (k0 < 0 || k1 > a->K || k1 <= k0 || k1 - k0 >= (1 << (63 - KEY_SHIFT)) || a->F > 65535 || a->W <= 0 || a->H <= 0)
    return OBJNERF_EINVAL;
  const VxLayout L = vx_layout(a->K, a->F, a->W, a->H);
  if (ws_bytes < L.total) return OBJNERF_EINVAL;
  if (n_points <= 0) return OBJNERF_OK;
  if (!out_pts || !out_keys) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(a->crops ? voxel_emit_kernel<true> : voxel_emit_kernel<false>,
                     dim3((unsigned)L.ntiles, (unsigned)a->F, (unsigned)(k1 - k0)), dim3(VX_WG), 0, (hipStream_t)stream, *a,
                     (const char*)ws, L, k0, base, vmin, dims, n_points, out_pts, out_keys);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

size_t objnerf_voxel_heads_workspace_bytes(int64_t n) {
  if (n <= 0) return 0;
  return sizeof(int64_t) * (size_t)((n + VX_HEAD_BLOCK - 1) / VX_HEAD_BLOCK + 1);
}

int objnerf_voxel_heads(int64_t n, const int64_t* sorted_keys, int64_t* ws, void* stream) {
  if (n <= 0 || !sorted_keys || !ws) return OBJNERF_EINVAL;
  const int64_t nb = (n + VX_HEAD_BLOCK - 1) / VX_HEAD_BLOCK;
  if (nb > 0x7fffffff) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(voxel_heads_kernel, dim3((unsigned)nb), dim3(VX_HEAD_WG), 0, (hipStream_t)stream, n, sorted_keys, ws);
  CHECK_LAUNCH();
  // blk[0 .. nb) -> exclusive offsets, blk[nb] = the number of heads
  hipLaunchKernelGGL((wg_scan_kernel<VX_SCAN_WG, 1, int64_t>), dim3(1), dim3(VX_SCAN_WG), 0, (hipStream_t)stream, ws, nb,
                     ws + nb);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_voxel_centroids(int64_t n, const int64_t* sorted_keys, const int64_t* perm, const double* pts,
                            const int64_t* ws, int64_t max_voxels, double* out_centroids, int64_t* out_keys,
                            int64_t* out_first, void* stream) {
  if (n <= 0 || !sorted_keys || !perm || !pts || !ws || !out_centroids || !out_keys || !out_first || max_voxels <= 0)
    return OBJNERF_EINVAL;
  const int64_t nb = (n + VX_HEAD_BLOCK - 1) / VX_HEAD_BLOCK;
  if (nb > 0x7fffffff) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(voxel_centroid_kernel, dim3((unsigned)nb), dim3(VX_HEAD_WG), 0, (hipStream_t)stream, n, sorted_keys,
                     perm, pts, ws, max_voxels, out_centroids, out_keys, out_first);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_obb_search(const objnerf_obb_args* a, int32_t n_split, double* ws, double* out, void* stream) {
  if (!a || !ws || !out || a->K <= 0 || a->K > 65535 || n_split <= 0 || n_split > 65535 || !a->verts || !a->vert_off ||
      !a->normals || !a->edges || !a->cand || !a->cand_off || !a->mode)
    return OBJNERF_EINVAL;
  double* part_vol = ws;
  int64_t* part_idx = (int64_t*)(ws + (size_t)a->K * n_split);
  hipLaunchKernelGGL(obb_search_kernel, dim3((unsigned)n_split, (unsigned)a->K), dim3(OBB_WG), 0, (hipStream_t)stream, *a,
                     part_vol, part_idx);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(obb_pick_kernel, dim3((unsigned)((a->K + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *a, n_split,
                     part_vol, part_idx, out);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

}  // extern "C"
