// Cross-frame mask association (the reference's maskclustering/mask_graph.py), the data-parallel parts it runs on the
// CPU through open3d and on the GPU through whole-matrix torch expressions:
//
// (a) Cell keys of point sets on a grid (cell_min_kernel, cell_keys_kernel): per segment the minimum corner (order-free:
//     exact), then per point key = ix << 42 | iy << 21 | iz with i = floor((p - (min - shift)) / cell).  The host sorts the keys
//     per segment (torch.sort(stable=True), twice: by key, then by segment) and hands back keys and permutation.
// (b) Segmented DBSCAN (objnerf_dbscan) over those sorted keys; a thread per sorted position, so neighbouring lanes
//     search the same cells.  Two points within eps lie in cells at most one apart per axis (the cell side is a hair
//     above eps, see the header), so the 27 cells around a point are 9 runs of the sorted keys (iz - 1 .. iz + 1 are
//     adjacent keys): 9 binary searches per point, never all pairs.
//       dbscan_core_kernel     core = at least min_points points with d^2 <= eps^2 (itself included), early exit;
//       dbscan_union_kernel    union-find over the core points: every link points from the larger root to the smaller
//                              (atomicCAS on a root, atomicMin for path halving), so whatever the order of the links
//                              the final root of a component is its smallest index;
//       dbscan_flatten_kernel / wg_scan_kernel (objnerf_wg.h) / dbscan_rank_kernel
//                              roots, and the rank of every root among the roots (count, scan, emit): cluster ids
//                              ascend with the smallest core index of the cluster;
//       dbscan_label_kernel    a core point takes its cluster, a border point the lowest cluster among its core
//                              neighbours (= the smallest root), a point without core neighbour -1.
//     These are the labels of a sequential DBSCAN that scans the points in index order (scikit-learn's).
// (c) objnerf_cloud_overlap: count[a][b] = points of cloud a with some point of cloud b at distance < thr (strict), the
//     same 9-run lookup in cloud b's sorted keys on one grid common to all clouds; integer atomic adds (order-free).
// (e) objnerf_mask_points / objnerf_mask_hist / objnerf_point_bounds: project_mask_pc's back-projection of a frame's
//     mask pixels (fp32 camera point, fp64 world point), the 3 x 32 colour histogram per mask, and exact boxes.
// (f) objnerf_mask_affinity: W = w_geo geo + w_cap cap + w_clip clip + w_color color + w_geo2d geo2d in one pass: a wave
//     per 16 x 16 tile, the three cosine Grams on v_mfma_f32_16x16x4_f32 straight from global rows, the box terms per
//     element; then the edges W >= 1 (i < j) by count per row, scan and ordered emit (objnerf_mask_edges).
// (d) objnerf_mask_ray_boxes: compute_2d_iou_matrix's ray / box pass: a thread per mask box, the frame's every-10th-pixel
//     rays staged in LDS 256 at a time, the slab test in fp64 with IEEE semantics followed literally.
// No float atomics; fp64 arithmetic without contraction (-ffp-contract=off); two calls write the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "objnerf_wg.h"
#include "objnerf_cells.h"

namespace {

constexpr int MG_WG = 256;
constexpr int MG_SCAN_WG = 1024;
constexpr int RAY_STEP = 10;          // get_rays: torch.arange(0, w, 10)

struct DbLayout { size_t parent, root, rank, core, blk, total; int64_t nb; };

inline DbLayout db_layout(int64_t n) {
  DbLayout L;
  L.nb = (n + MG_WG - 1) / MG_WG;
  size_t o = 0;
  L.parent = o; o += align256(sizeof(int32_t) * (size_t)n);
  L.root = o;   o += align256(sizeof(int32_t) * (size_t)n);
  L.rank = o;   o += align256(sizeof(int32_t) * (size_t)n);
  L.core = o;   o += align256((size_t)n);
  L.blk = o;    o += align256(sizeof(int32_t) * (size_t)(L.nb + 1));
  L.total = o;
  return L;
}

// f(q, d2) for every point q of the sorted rows [lo, hi) in the 27 cells around `key`; f returns true to stop
template <class Fn>
__device__ __forceinline__ void for_near(const int64_t n, const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                         const double* __restrict__ pts, const int64_t lo, const int64_t hi,
                                         const int64_t key, const double p[3], Fn&& f) {
  const int64_t cx = (key >> (2 * CELL_BITS)) & CELL_MAX, cy = (key >> CELL_BITS) & CELL_MAX, cz = key & CELL_MAX;
  const int64_t z0 = cz > 0 ? cz - 1 : 0, z1 = cz < CELL_MAX ? cz + 1 : CELL_MAX;
  for (int dx = -1; dx <= 1; ++dx) {
    const int64_t x = cx + dx;
    if (x < 0 || x > CELL_MAX) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const int64_t y = cy + dy;
      if (y < 0 || y > CELL_MAX) continue;
      const int64_t k1 = cell_key(x, y, z1);
      for (int64_t e = lower_bound(keys, lo, hi, cell_key(x, y, z0)); e < hi && keys[e] <= k1; ++e) {
        const int64_t q = perm[e];
        if ((uint64_t)q >= (uint64_t)n) continue;          // (a permutation has no such entry; never read past)
        if (f(q, dist2(pts + 3 * q, p))) return;
      }
    }
  }
}

// one workgroup per segment: the minimum corner of its points (+inf for an empty segment)
__global__ void __launch_bounds__(MG_WG) cell_min_kernel(const int64_t n, const double* __restrict__ pts,
                                                         const int64_t* __restrict__ off, double* __restrict__ out_min) {
  const int s = blockIdx.x;
  int64_t lo = off[s], hi = off[s + 1];
  lo = lo < 0 ? 0 : lo; hi = hi > n ? n : hi;
  double mn[3] = {INFINITY, INFINITY, INFINITY};
  for (int64_t i = lo + threadIdx.x; i < hi; i += MG_WG)
    for (int c = 0; c < 3; ++c) mn[c] = fmin(mn[c], pts[3 * i + c]);
  __shared__ double red[MG_WG / 64][3];
  for (int c = 0; c < 3; ++c)
    for (int o = 32; o > 0; o >>= 1) mn[c] = fmin(mn[c], __shfl_xor(mn[c], o));
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < 3; ++c) red[threadIdx.x >> 6][c] = mn[c];
  __syncthreads();
  if (threadIdx.x < 3) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < MG_WG / 64; ++w) v = fmin(v, red[w][threadIdx.x]);
    out_min[3 * s + threadIdx.x] = v;
  }
}

__global__ void __launch_bounds__(MG_WG) cell_keys_kernel(const int64_t n, const int S, const double* __restrict__ pts,
                                                          const int64_t* __restrict__ off, const double* __restrict__ mins,
                                                          const double cell, const double shift,
                                                          int64_t* __restrict__ out_keys,
                                                          int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * MG_WG + threadIdx.x;
  if (i >= n) return;
  const int s = seg_of(off, S, i);
  int64_t ix[3];
  bool bad = false;
  for (int c = 0; c < 3; ++c) {
    const double v = floor(__ddiv_rn(__dsub_rn(pts[3 * i + c], __dsub_rn(mins[3 * s + c], shift)), cell));
    const bool ok = v >= 0.0 && v <= (double)CELL_MAX;      // false for a NaN or infinite coordinate too
    ix[c] = ok ? (int64_t)v : 0;
    bad |= !ok;
  }
  out_keys[i] = cell_key(ix[0], ix[1], ix[2]);
  if (bad) atomicOr(status, 1);
}

struct DbArgs {
  int64_t n; int S;
  const double* pts; const int64_t* off; const int64_t* keys; const int64_t* perm; const int32_t* min_points;
  double eps2;
  int32_t* parent; int32_t* root; int32_t* rank; uint8_t* core; int32_t* blk; int32_t* labels;
};

__device__ __forceinline__ void seg_range(const DbArgs& a, const int s, int64_t& lo, int64_t& hi) {
  lo = a.off[s]; hi = a.off[s + 1];
  lo = lo < 0 ? 0 : lo; hi = hi > a.n ? a.n : hi;
}

__global__ void __launch_bounds__(MG_WG) dbscan_core_kernel(const DbArgs a) {
  const int64_t t = (int64_t)blockIdx.x * MG_WG + threadIdx.x;
  if (t >= a.n) return;
  const int64_t i = a.perm[t];
  if ((uint64_t)i >= (uint64_t)a.n) return;
  const int s = seg_of(a.off, a.S, t);
  const int mp = a.min_points[s];
  a.parent[i] = (int32_t)i;
  if (mp <= 0) { a.core[i] = 0; return; }
  int64_t lo, hi;
  seg_range(a, s, lo, hi);
  const double p[3] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
  int cnt = 0;
  for_near(a.n, a.keys, a.perm, a.pts, lo, hi, a.keys[t], p, [&](const int64_t, const double d2) {
    cnt += d2 <= a.eps2;
    return cnt >= mp;
  });
  a.core[i] = cnt >= mp;
}

__device__ __forceinline__ int32_t load_parent(int32_t* parent, const int32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x; halves the path on the way (atomicMin: a parent only ever moves to a smaller member of its own set)
__device__ __forceinline__ int32_t find_root(int32_t* parent, int32_t x) {
  int32_t p = load_parent(parent, x);
  while (p != x) {
    const int32_t g = load_parent(parent, p);
    if (g != p) atomicMin(parent + x, g);
    x = p; p = g;
  }
  return x;
}

__device__ __forceinline__ void unite(int32_t* parent, int32_t a, int32_t b) {
  while (true) {
    a = find_root(parent, a); b = find_root(parent, b);
    if (a == b) return;
    if (a < b) { const int32_t t = a; a = b; b = t; }
    const int32_t old = atomicCAS(parent + a, a, b);       // link the larger root under the smaller
    if (old == a) return;
    a = old;                                               // a was linked meanwhile: go on from its new parent
  }
}

__global__ void __launch_bounds__(MG_WG) dbscan_union_kernel(const DbArgs a) {
  const int64_t t = (int64_t)blockIdx.x * MG_WG + threadIdx.x;
  if (t >= a.n) return;
  const int64_t i = a.perm[t];
  if ((uint64_t)i >= (uint64_t)a.n || !a.core[i]) return;
  const int s = seg_of(a.off, a.S, t);
  int64_t lo, hi;
  seg_range(a, s, lo, hi);
  const double p[3] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
  for_near(a.n, a.keys, a.perm, a.pts, lo, hi, a.keys[t], p, [&](const int64_t q, const double d2) {
    if (q < i && d2 <= a.eps2 && a.core[q]) unite(a.parent, (int32_t)i, (int32_t)q);
    return false;
  });
}

// root[i] = the root of core point i (-1: not core), blk[b] = roots in block b
__global__ void __launch_bounds__(MG_WG) dbscan_flatten_kernel(const DbArgs a) {
  const int64_t i = (int64_t)blockIdx.x * MG_WG + threadIdx.x;
  bool is_root = false;
  if (i < a.n) {
    const int32_t r = a.core[i] ? find_root(a.parent, (int32_t)i) : -1;
    a.root[i] = r;
    is_root = r == (int32_t)i;
  }
  __shared__ int wcnt[MG_WG / 64];
  int c;
  wg_exclusive_flag<MG_WG>(is_root, wcnt, c);
  if (threadIdx.x == 0) a.blk[blockIdx.x] = c;
}

// rank[i] = roots among the points before i
__global__ void __launch_bounds__(MG_WG) dbscan_rank_kernel(const DbArgs a) {
  const int64_t i = (int64_t)blockIdx.x * MG_WG + threadIdx.x;
  const bool is_root = i < a.n && a.root[i] == (int32_t)i;
  __shared__ int wcnt[MG_WG / 64];
  int total;
  const int pre = wg_exclusive_flag<MG_WG>(is_root, wcnt, total);
  if (i < a.n) a.rank[i] = a.blk[blockIdx.x] + pre;
}

__global__ void __launch_bounds__(MG_WG) dbscan_label_kernel(const DbArgs a) {
  const int64_t t = (int64_t)blockIdx.x * MG_WG + threadIdx.x;
  if (t >= a.n) return;
  const int64_t i = a.perm[t];
  if ((uint64_t)i >= (uint64_t)a.n) return;
  const int s = seg_of(a.off, a.S, t);
  if (a.min_points[s] <= 0) return;                        // a segment switched off: its labels stay as they are
  int64_t lo, hi;
  seg_range(a, s, lo, hi);
  int32_t r = a.root[i];
  if (r < 0) {
    const double p[3] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
    int32_t best = INT32_MAX;
    for_near(a.n, a.keys, a.perm, a.pts, lo, hi, a.keys[t], p, [&](const int64_t q, const double d2) {
      const int32_t rq = a.root[q];
      if (rq >= 0 && d2 <= a.eps2 && rq < best) best = rq;
      return false;
    });
    r = best == INT32_MAX ? -1 : best;
  }
  a.labels[i] = r < 0 ? -1 : a.rank[r] - a.rank[lo];       // the segment's first row has no root before it in the segment
}

__global__ void __launch_bounds__(MG_WG) overlap_kernel(const int64_t n, const int C, const double* __restrict__ pts,
                                                        const int64_t* __restrict__ off, const int64_t* __restrict__ keys,
                                                        const int64_t* __restrict__ perm, const double thr2,
                                                        unsigned long long* __restrict__ count) {
  const int64_t t = (int64_t)blockIdx.x * MG_WG + threadIdx.x;
  const int b = blockIdx.y;
  if (t >= n) return;
  const int64_t i = perm[t];
  if ((uint64_t)i >= (uint64_t)n) return;
  const int a = seg_of(off, C, t);
  int64_t lo = off[b], hi = off[b + 1];
  lo = lo < 0 ? 0 : lo; hi = hi > n ? n : hi;
  const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
  bool found = false;
  for_near(n, keys, perm, pts, lo, hi, keys[t], p, [&](const int64_t, const double d2) {
    found = d2 < thr2;
    return found;
  });
  if (found) atomicAdd(count + (int64_t)a * C + b, 1ull);
}

// a thread per mask box; the frame's rays pass through LDS 256 at a time
__global__ void __launch_bounds__(MG_WG) boxes2d_kernel(const objnerf_ray_boxes_args a) {
  const int f = blockIdx.y;
  const int m = blockIdx.x * MG_WG + threadIdx.x;
  const bool valid = m < a.N;
  const int rw = a.W / RAY_STEP, rh = a.H / RAY_STEP, R = rw * rh;
  const double* T = a.twc + (int64_t)f * 16;
  const uint16_t* depth = a.depth + (int64_t)f * a.W * a.H;
  const float fx = (float)a.fx, fy = (float)a.fy, cx = (float)a.cx, cy = (float)a.cy;
  double lo[3], hi[3];                                     // bounds_min - origin, bounds_max - origin
  for (int c = 0; c < 3; ++c) {
    const double o = T[4 * c + 3];
    lo[c] = valid ? __dsub_rn(a.boxes[6 * (int64_t)m + c], o) : 0.0;
    hi[c] = valid ? __dsub_rn(a.boxes[6 * (int64_t)m + 3 + c], o) : 0.0;
  }
  __shared__ double sd[MG_WG][3];
  int rmin = INT32_MAX, cmin = INT32_MAX, rmax = -1, cmax = -1;
  for (int r0 = 0; r0 < R; r0 += MG_WG) {
    __syncthreads();
    const int r = r0 + threadIdx.x;
    if (r < R) {
      const int iy = (r / rw) * RAY_STEP, ix = (r % rw) * RAY_STEP;
      // get_rays: ((ix - cx) / fx, (iy - cy) / fy, 1) in fp32, then x depth / 1000.0 in fp64
      const double z = __ddiv_rn((double)depth[(int64_t)iy * a.W + ix], 1000.0);
      const double d[3] = {__dmul_rn((double)__fdiv_rn(__fsub_rn((float)ix, cx), fx), z),
                           __dmul_rn((double)__fdiv_rn(__fsub_rn((float)iy, cy), fy), z), z};
      for (int c = 0; c < 3; ++c)
        sd[threadIdx.x][c] = __dadd_rn(__dadd_rn(__dmul_rn(d[0], T[4 * c]), __dmul_rn(d[1], T[4 * c + 1])),
                                       __dmul_rn(d[2], T[4 * c + 2]));
    }
    __syncthreads();
    if (!valid) continue;
    const int nq = R - r0 < MG_WG ? R - r0 : MG_WG;
    for (int q = 0; q < nq; ++q) {
      double near = -INFINITY, far = INFINITY;
      bool nan = false;
      for (int c = 0; c < 3; ++c) {
        const double tmin = __ddiv_rn(lo[c], sd[q][c]), tmax = __ddiv_rn(hi[c], sd[q][c]);
        nan |= tmin != tmin || tmax != tmax;               // torch.min / max / amax / amin carry a NaN to the end
        const double t1 = tmin < tmax ? tmin : tmax, t2 = tmin < tmax ? tmax : tmin;
        near = t1 > near ? t1 : near;
        far = t2 < far ? t2 : far;
      }
      if (!nan && near <= far && far > 0.0) {
        const int row = (r0 + q) / rw, col = (r0 + q) % rw;
        rmin = row < rmin ? row : rmin; rmax = row > rmax ? row : rmax;
        cmin = col < cmin ? col : cmin; cmax = col > cmax ? col : cmax;
      }
    }
  }
  if (!valid) return;
  int32_t* o = a.out + ((int64_t)f * a.N + m) * 4;
  const bool any = rmax >= 0;
  o[0] = any ? rmin : 0; o[1] = any ? cmin : 0; o[2] = any ? rmax + 1 : 0; o[3] = any ? cmax + 1 : 0;
}


// ------------------------------------------------------------------------------------------- mask clouds of a frame
// one workgroup per segment: the minimum and maximum corner of its points (+inf / -inf for an empty segment)
__global__ void __launch_bounds__(MG_WG) point_bounds_kernel(const int64_t n, const double* __restrict__ pts,
                                                             const int64_t* __restrict__ off, double* __restrict__ out) {
  const int s = blockIdx.x;
  int64_t lo = off[s], hi = off[s + 1];
  lo = lo < 0 ? 0 : lo; hi = hi > n ? n : hi;
  double v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = lo + threadIdx.x; i < hi; i += MG_WG)
    for (int c = 0; c < 3; ++c) { v[c] = fmin(v[c], pts[3 * i + c]); v[3 + c] = fmax(v[3 + c], pts[3 * i + c]); }
  __shared__ double red[MG_WG / 64][6];
  for (int c = 0; c < 6; ++c)
    for (int o = 32; o > 0; o >>= 1) {
      const double t = __shfl_xor(v[c], o);
      v[c] = c < 3 ? fmin(v[c], t) : fmax(v[c], t);
    }
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < 6; ++c) red[threadIdx.x >> 6][c] = v[c];
  __syncthreads();
  if (threadIdx.x < 6) {
    double r = red[0][threadIdx.x];
    for (int w = 1; w < MG_WG / 64; ++w) r = threadIdx.x < 3 ? fmin(r, red[w][threadIdx.x]) : fmax(r, red[w][threadIdx.x]);
    out[6 * s + threadIdx.x] = r;
  }
}

// pixel index -> world point: (u - cx) * d / fx, (v - cy) * d / fy, d in fp32, left to right (project_mask_pc's torch
// expressions), then pose * (x, y, z, 1) in fp64 (open3d's transform), every product and sum rounded on its own
__global__ void __launch_bounds__(MG_WG) mask_points_kernel(const objnerf_mask_points_args a) {
  const int64_t i = (int64_t)blockIdx.x * MG_WG + threadIdx.x;
  if (i >= a.n) return;
  const int32_t p = a.pix[i];
  double* o = a.out + 3 * i;
  if (p < 0 || p >= a.W * a.H) { o[0] = o[1] = o[2] = NAN; return; }     // (not a pixel of the image: never read past)
  const int u = p % a.W, v = p / a.W;
  const float d = a.depth[p];
  const float xf = __fdiv_rn(__fmul_rn(__fsub_rn((float)u, (float)a.cx), d), (float)a.fx);
  const float yf = __fdiv_rn(__fmul_rn(__fsub_rn((float)v, (float)a.cy), d), (float)a.fy);
  const double x = (double)xf, y = (double)yf, z = (double)d;
  const double* P = a.pose;
  for (int r = 0; r < 3; ++r)
    o[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(P[4 * r], x), __dmul_rn(P[4 * r + 1], y)), __dmul_rn(P[4 * r + 2], z)),
                     P[4 * r + 3]);
}

// one workgroup per mask: 3 x 32 bins of width 8 over its pixels, integer counts in LDS (integer adds: order-free)
__global__ void __launch_bounds__(MG_WG) mask_hist_kernel(const int64_t n, const int32_t* __restrict__ pix,
                                                          const int64_t* __restrict__ off, const uint8_t* __restrict__ img,
                                                          const int32_t n_px, float* __restrict__ out) {
  const int m = blockIdx.x;
  int64_t lo = off[m], hi = off[m + 1];
  lo = lo < 0 ? 0 : lo; hi = hi > n ? n : hi;
  __shared__ unsigned int h[96];
  if (threadIdx.x < 96) h[threadIdx.x] = 0u;
  __syncthreads();
  for (int64_t i = lo + threadIdx.x; i < hi; i += MG_WG) {
    const int32_t p = pix[i];
    if (p < 0 || p >= n_px) continue;
    for (int c = 0; c < 3; ++c) atomicAdd(&h[32 * c + (img[3 * (int64_t)p + c] >> 3)], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 96) out[96 * (int64_t)m + threadIdx.x] = (float)h[threadIdx.x];
}

// --------------------------------------------------------------------------------------------------------- affinity
constexpr int AF_T = 32;              // a workgroup's block of W: 2 x 2 tiles of 16 x 16, one per wave

// a wave per row: |x| = fp32(sqrt(fp64 sum of squares)), the lanes' partial sums combined in a fixed order
__global__ void __launch_bounds__(MG_WG) row_norm_kernel(const int N, const int D, const float* __restrict__ x,
                                                         float* __restrict__ out) {
  const int row = blockIdx.x * (MG_WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  double s = 0.0;
  for (int k = lane; k < D; k += 64) {
    const double v = (double)x[(int64_t)row * D + k];
    s = __dadd_rn(s, __dmul_rn(v, v));
  }
  for (int o = 32; o > 0; o >>= 1) s = __dadd_rn(s, __shfl_xor(s, o));
  if (lane == 0) out[row] = (float)sqrt(s);
}

// acc[e] = x[i0 + 4 g + e] . x[j0 + q] (g = lane >> 4, q = lane & 15) on v_mfma_f32_16x16x4_f32: k-step t of chunk c
// takes column 16 c + 4 g + t from lane group g, for both operands; pre: each element divided by its row's norm first
__device__ __forceinline__ floatx4 gram_tile(const float* __restrict__ x, const int D, const int N, const int i0,
                                             const int j0, const float* __restrict__ norm, const bool pre) {
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int ia = i0 + r, jb = j0 + r;
  const bool va = ia < N, vb = jb < N, vec = (D & 3) == 0;
  const float* pa = x + (int64_t)(va ? ia : 0) * D;
  const float* pb = x + (int64_t)(vb ? jb : 0) * D;
  const float na = pre && va ? norm[ia] : 1.f, nb = pre && vb ? norm[jb] : 1.f;
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < (D + 15) / 16; ++c) {                // (a wave-uniform trip count; lane groups past D hold zeros)
    const int k0 = 16 * c + 4 * g;
    float4 fa = vec ? load_row4<true>(pa, k0, D, va) : load_row4<false>(pa, k0, D, va);
    float4 fb = vec ? load_row4<true>(pb, k0, D, vb) : load_row4<false>(pb, k0, D, vb);
    if (pre) {
      fa.x = fa.x / na; fa.y = fa.y / na; fa.z = fa.z / na; fa.w = fa.w / na;
      fb.x = fb.x / nb; fb.y = fb.y / nb; fb.z = fb.z / nb; fb.w = fb.w / nb;
      if (k0 >= D) { fa.x = 0.f; fb.x = 0.f; }              // 0 / 0 of the padding is no part of the row
      if (k0 + 1 >= D) { fa.y = 0.f; fb.y = 0.f; }
      if (k0 + 2 >= D) { fa.z = 0.f; fb.z = 0.f; }
      if (k0 + 3 >= D) { fa.w = 0.f; fb.w = 0.f; }
      if (!va) fa = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!vb) fb = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.x, fb.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.y, fb.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.z, fb.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.w, fb.w, acc, 0, 0, 0);
  }
  return acc;
}

// compute_3d_iou_matrix: intersection volume / the smaller volume, NaN -> 0
__device__ __forceinline__ double geo_term(const double* __restrict__ a, const double* __restrict__ b) {
  const double va = __dmul_rn(__dmul_rn(__dsub_rn(a[3], a[0]), __dsub_rn(a[4], a[1])), __dsub_rn(a[5], a[2]));
  const double vb = __dmul_rn(__dmul_rn(__dsub_rn(b[3], b[0]), __dsub_rn(b[4], b[1])), __dsub_rn(b[5], b[2]));
  double inter = 1.0;
  for (int c = 0; c < 3; ++c) {
    const double d = __dsub_rn(fmin(a[3 + c], b[3 + c]), fmax(a[c], b[c]));
    inter = c == 0 ? (d > 0.0 ? d : 0.0) : __dmul_rn(inter, d > 0.0 ? d : 0.0);
  }
  const double r = __ddiv_rn(inter, va < vb ? va : vb);
  return r != r ? 0.0 : r;
}

// compute_iou_2d on two int32 boxes: integer areas, a true division in fp32, NaN -> 0
__device__ __forceinline__ float iou2d(const int4 a, const int4 b) {
  const int aa = (a.z - a.x) * (a.w - a.y), ab = (b.z - b.x) * (b.w - b.y);
  const int dx = min(a.z, b.z) - max(a.x, b.x), dy = min(a.w, b.w) - max(a.y, b.y);
  const int inter = (dx > 0 ? dx : 0) * (dy > 0 ? dy : 0);
  const float r = __fdiv_rn((float)inter, (float)(aa + ab - inter));
  return r != r ? 0.f : r;
}

__global__ void __launch_bounds__(MG_WG) affinity_kernel(const objnerf_affinity_args a, const float* __restrict__ norms) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, q = lane & 15;
  const int N = a.N;
  const int i0 = blockIdx.y * AF_T + 16 * (wv >> 1), j0 = blockIdx.x * AF_T + 16 * (wv & 1);
  if (i0 >= N || j0 >= N) return;                           // (wave-uniform)
  const float* ncap = norms, *nclip = norms + N, *ncol = norms + 2 * (int64_t)N;
  const floatx4 cap = gram_tile(a.cap, a.d_cap, N, i0, j0, nullptr, false);
  const floatx4 clip = gram_tile(a.clip, a.d_clip, N, i0, j0, nullptr, false);
  const floatx4 col = gram_tile(a.color, 96, N, i0, j0, ncol, true);
  const int j = j0 + q;
  if (j >= N) return;
  const float wcap = (float)a.w_cap, wclip = (float)a.w_clip, wcol = (float)a.w_color, w2d = (float)a.w_geo2d;
  const int64_t NN = (int64_t)N * N;
  for (int e = 0; e < 4; ++e) {
    const int i = i0 + 4 * g + e;
    if (i >= N) continue;
    // adjacent_matrix_feat: mm(x, x^T) / (|x_i| |x_j|) in fp32; no epsilon: a zero row gives NaN
    const float tcap = __fdiv_rn(cap[e], __fmul_rn(ncap[i], ncap[j]));
    const float tclip = __fdiv_rn(clip[e], __fmul_rn(nclip[i], nclip[j]));
    const float tcol = col[e];
    const double tgeo = geo_term(a.boxes + 6 * (int64_t)i, a.boxes + 6 * (int64_t)j);
    float m = 0.f;
    if (a.w_geo2d != 0.0 && a.boxes2d)
      for (int f = 0; f < a.F; ++f) {                       // the reference's running mean, in frame order
        const int4* b = (const int4*)a.boxes2d + (int64_t)f * N;
        m = __fdiv_rn(__fadd_rn(__fmul_rn(m, (float)f), iou2d(b[i], b[j])), (float)(f + 1));
      }
    // MaskGraph.__init__: fp64 geo x weight + the fp32 matrices x their weights (fp32 products), summed in fp64
    double w = __dmul_rn(tgeo, a.w_geo);
    w = __dadd_rn(w, (double)__fmul_rn(tcap, wcap));
    w = __dadd_rn(w, (double)__fmul_rn(tclip, wclip));
    w = __dadd_rn(w, (double)__fmul_rn(tcol, wcol));
    if (a.w_geo2d != 0.0) w = __dadd_rn(w, (double)__fmul_rn(m, w2d));
    const int64_t at = (int64_t)i * N + j;
    a.W[at] = (float)w;
    if (a.terms) {
      a.terms[at] = (float)tgeo; a.terms[NN + at] = tcap; a.terms[2 * NN + at] = tclip; a.terms[3 * NN + at] = tcol;
      a.terms[4 * NN + at] = m;
    }
  }
}

// one workgroup per row: the edges (i, j > i) with W >= 1
__global__ void __launch_bounds__(MG_WG) edge_count_kernel(const int N, const float* __restrict__ W,
                                                           int64_t* __restrict__ row_off) {
  const int i = blockIdx.x;
  int c = 0;
  for (int j = i + 1 + threadIdx.x; j < N; j += MG_WG) c += W[(int64_t)i * N + j] >= 1.0f;
  __shared__ int wsum[MG_WG / 64];
  const int t = wg_sum<MG_WG>(c, wsum);
  if (threadIdx.x == 0) row_off[i] = t;
}

// one workgroup per row: its edges in column order at row_off[i] ..
__global__ void __launch_bounds__(MG_WG) edge_emit_kernel(const int N, const float* __restrict__ W,
                                                          const int64_t* __restrict__ row_off, const int64_t max_edges,
                                                          int32_t* __restrict__ out_ij, float* __restrict__ out_w) {
  const int i = blockIdx.x;
  __shared__ int wcnt[MG_WG / 64];
  int64_t base = row_off[i];
  for (int j0 = i + 1; j0 < N; j0 += MG_WG) {
    const int j = j0 + threadIdx.x;
    const float w = j < N ? W[(int64_t)i * N + j] : 0.f;
    const bool e = j < N && w >= 1.0f;
    __syncthreads();                                       // (the tile before has read wcnt)
    int tot;
    const int64_t pos = base + wg_exclusive_flag<MG_WG>(e, wcnt, tot);
    if (e && pos >= 0 && pos < max_edges) { out_ij[2 * pos] = i; out_ij[2 * pos + 1] = j; out_w[pos] = w; }
    base += tot;
  }
}

}  // namespace

extern "C" {

int objnerf_cell_keys(int64_t n, int32_t S, const double* pts, const int64_t* seg_off, double cell, double shift,
                      double* out_min, int64_t* out_keys, int32_t* status, void* stream) {
  if (n < 0 || n > 0x7fffffff || S <= 0 || S > 0x7fffffff || !seg_off || !out_min || !status || !(cell > 0.0) || !(shift >= 0.0))
    return OBJNERF_EINVAL;
  if (n > 0 && (!pts || !out_keys)) return OBJNERF_EINVAL;
  if (hipMemsetAsync(status, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return OBJNERF_ELAUNCH;
  hipLaunchKernelGGL(cell_min_kernel, dim3((unsigned)S), dim3(MG_WG), 0, (hipStream_t)stream, n, pts, seg_off, out_min);
  CHECK_LAUNCH();
  if (n == 0) return OBJNERF_OK;
  hipLaunchKernelGGL(cell_keys_kernel, dim3((unsigned)((n + MG_WG - 1) / MG_WG)), dim3(MG_WG), 0, (hipStream_t)stream, n,
                     S, pts, seg_off, out_min, cell, shift, out_keys, status);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

size_t objnerf_dbscan_workspace_bytes(int64_t n) {
  if (n <= 0 || n > 0x7fffffff) return 0;
  return db_layout(n).total;
}

int objnerf_dbscan(int64_t n, int32_t S, const double* pts, const int64_t* seg_off, const int64_t* sorted_keys,
                   const int64_t* perm, const int32_t* min_points, double eps, void* ws, size_t ws_bytes, int32_t* labels,
                   void* stream) {
  if (n < 0 || n > 0x7fffffff || S <= 0 || !seg_off || !min_points || !(eps > 0.0)) return OBJNERF_EINVAL;
  if (n == 0) return OBJNERF_OK;
  if (!pts || !sorted_keys || !perm || !ws || !labels) return OBJNERF_EINVAL;
  const DbLayout L = db_layout(n);
  if (ws_bytes < L.total) return OBJNERF_EINVAL;
  char* w = (char*)ws;
  DbArgs a;
  a.n = n; a.S = S; a.pts = pts; a.off = seg_off; a.keys = sorted_keys; a.perm = perm; a.min_points = min_points;
  a.eps2 = eps * eps;
  a.parent = (int32_t*)(w + L.parent); a.root = (int32_t*)(w + L.root); a.rank = (int32_t*)(w + L.rank);
  a.core = (uint8_t*)(w + L.core); a.blk = (int32_t*)(w + L.blk); a.labels = labels;
  const dim3 grid((unsigned)L.nb), wg(MG_WG);
  hipStream_t st = (hipStream_t)stream;
  // (a point the permutation misses would leave its flag unwritten: clear them first)
  if (hipMemsetAsync(a.core, 0, (size_t)n, st) != hipSuccess) return OBJNERF_ELAUNCH;
  hipLaunchKernelGGL(dbscan_core_kernel, grid, wg, 0, st, a);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(dbscan_union_kernel, grid, wg, 0, st, a);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(dbscan_flatten_kernel, grid, wg, 0, st, a);
  CHECK_LAUNCH();
  // blk[0 .. nb) -> exclusive offsets, blk[nb] = the number of roots
  hipLaunchKernelGGL((wg_scan_kernel<MG_SCAN_WG, 1, int32_t>), dim3(1), dim3(MG_SCAN_WG), 0, st, a.blk, L.nb, a.blk + L.nb);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(dbscan_rank_kernel, grid, wg, 0, st, a);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(dbscan_label_kernel, grid, wg, 0, st, a);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_cloud_overlap(int64_t n, int32_t C, const double* pts, const int64_t* cloud_off, const int64_t* sorted_keys,
                          const int64_t* perm, double dis_thre, int64_t* out_count, void* stream) {
  if (n < 0 || n > 0x7fffffff || C <= 0 || C > 65535 || !cloud_off || !out_count || !(dis_thre > 0.0)) return OBJNERF_EINVAL;
  if (hipMemsetAsync(out_count, 0, sizeof(int64_t) * (size_t)C * C, (hipStream_t)stream) != hipSuccess)
    return OBJNERF_ELAUNCH;
  if (n == 0) return OBJNERF_OK;
  if (!pts || !sorted_keys || !perm) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(overlap_kernel, dim3((unsigned)((n + MG_WG - 1) / MG_WG), (unsigned)C), dim3(MG_WG), 0,
                     (hipStream_t)stream, n, C, pts, cloud_off, sorted_keys, perm, dis_thre * dis_thre,
                     (unsigned long long*)out_count);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_mask_ray_boxes(const objnerf_ray_boxes_args* a, void* stream) {
  if (!a || a->F <= 0 || a->F > 65535 || a->N <= 0 || a->W <= 0 || a->H <= 0 || !a->depth || !a->twc || !a->boxes || !a->out)
    return OBJNERF_EINVAL;
  if (a->W % RAY_STEP || a->H % RAY_STEP) return OBJNERF_EINVAL;         // the reference's hit.view(...) fails on these
  hipLaunchKernelGGL(boxes2d_kernel, dim3((unsigned)((a->N + MG_WG - 1) / MG_WG), (unsigned)a->F), dim3(MG_WG), 0,
                     (hipStream_t)stream, *a);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}


int objnerf_point_bounds(int64_t n, int32_t S, const double* pts, const int64_t* seg_off, double* out, void* stream) {
  if (n < 0 || S <= 0 || !seg_off || !out || (n > 0 && !pts)) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(point_bounds_kernel, dim3((unsigned)S), dim3(MG_WG), 0, (hipStream_t)stream, n, pts, seg_off, out);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_mask_points(const objnerf_mask_points_args* a, void* stream) {
  if (!a || a->n < 0 || a->W <= 0 || a->H <= 0 || (int64_t)a->W * a->H > 0x7fffffff || !a->depth || !a->pose)
    return OBJNERF_EINVAL;
  if (a->n == 0) return OBJNERF_OK;
  if (!a->pix || !a->out) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(mask_points_kernel, dim3((unsigned)((a->n + MG_WG - 1) / MG_WG)), dim3(MG_WG), 0, (hipStream_t)stream,
                     *a);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_mask_hist(int64_t n, int32_t M, const int32_t* pix, const int64_t* mask_off, const uint8_t* img, int32_t W,
                      int32_t H, float* out, void* stream) {
  if (n < 0 || M <= 0 || W <= 0 || H <= 0 || (int64_t)W * H > 0x7fffffff || !mask_off || !img || !out || (n > 0 && !pix))
    return OBJNERF_EINVAL;
  hipLaunchKernelGGL(mask_hist_kernel, dim3((unsigned)M), dim3(MG_WG), 0, (hipStream_t)stream, n, pix, mask_off, img,
                     W * H, out);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

size_t objnerf_affinity_workspace_bytes(int32_t N) {
  if (N <= 0) return 0;
  return align256(sizeof(float) * 3 * (size_t)N);
}

int objnerf_mask_affinity(const objnerf_affinity_args* a, void* ws, size_t ws_bytes, int64_t* row_off, void* stream) {
  if (!a || !ws || !row_off || a->N <= 0 || a->N > 65535 * AF_T || a->d_cap <= 0 || a->d_cap > 1024 || a->d_clip <= 0 ||
      a->d_clip > 1024 || !a->boxes || !a->cap || !a->clip || !a->color || !a->W)
    return OBJNERF_EINVAL;
  if (a->w_geo2d != 0.0 && (!a->boxes2d || a->F <= 0)) return OBJNERF_EINVAL;
  if (ws_bytes < objnerf_affinity_workspace_bytes(a->N)) return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  float* norms = (float*)ws;
  const dim3 ng((unsigned)((a->N + MG_WG / 64 - 1) / (MG_WG / 64)));
  hipLaunchKernelGGL(row_norm_kernel, ng, dim3(MG_WG), 0, st, a->N, a->d_cap, a->cap, norms);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(row_norm_kernel, ng, dim3(MG_WG), 0, st, a->N, a->d_clip, a->clip, norms + a->N);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(row_norm_kernel, ng, dim3(MG_WG), 0, st, a->N, 96, a->color, norms + 2 * (size_t)a->N);
  CHECK_LAUNCH();
  const unsigned nb = (unsigned)((a->N + AF_T - 1) / AF_T);
  hipLaunchKernelGGL(affinity_kernel, dim3(nb, nb), dim3(MG_WG), 0, st, *a, (const float*)norms);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(edge_count_kernel, dim3((unsigned)a->N), dim3(MG_WG), 0, st, a->N, (const float*)a->W, row_off);
  CHECK_LAUNCH();
  // row_off[0 .. N) -> exclusive offsets, row_off[N] = the number of edges
  hipLaunchKernelGGL((wg_scan_kernel<MG_SCAN_WG, 1, int64_t>), dim3(1), dim3(MG_SCAN_WG), 0, st, row_off, (int64_t)a->N,
                     row_off + a->N);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_mask_edges(int32_t N, const float* W, const int64_t* row_off, int64_t max_edges, int32_t* out_ij, float* out_w,
                       void* stream) {
  if (N <= 0 || !W || !row_off || max_edges < 0) return OBJNERF_EINVAL;
  if (max_edges == 0) return OBJNERF_OK;
  if (!out_ij || !out_w) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(edge_emit_kernel, dim3((unsigned)N), dim3(MG_WG), 0, (hipStream_t)stream, N, W, row_off, max_edges,
                     out_ij, out_w);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

}  // extern "C"
