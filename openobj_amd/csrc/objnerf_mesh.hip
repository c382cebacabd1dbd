// Marching cubes on a dense fp32 volume [d][d][d] (last axis fastest): the iso-surface extraction behind
// Trainer.meshing / vis.marching_cubes (trainer.py:46-103, vis.py:6-22), which the reference runs through
// skimage.measure.marching_cubes(vol, level, gradient_direction='ascent') on the CPU.
//
// Count, scan, emit -- four short launches, no inter-workgroup protocol, no float atomics:
//   mc_count_kernel   one thread per lattice point p (the last axis on the lanes): the 3-bit mask of the +axis edges
//                     p owns that cross the level, and the triangle count of the cell whose lowest corner is p; each
//                     256-thread workgroup writes its two totals (int64 [nb][2]);
//   wg_scan_kernel    (objnerf_wg.h) one workgroup turns those totals into exclusive offsets and writes V, F;
//   mc_verts_kernel   recomputes the mask, the intra-workgroup prefix (wave ballots + 4 LDS slots), writes the
//                     vertices and normals and stores (local vertex base << 3 | mask) per point (uint16 [d^3]);
//   mc_faces_kernel   recomputes the case and the prefix of the triangle counts; a triangle's vertex on cell edge e
//                     is owned by corner o = cell + offset(MC_EDGE_C0[e]) along MC_EDGE_AXIS[e]:
//                     id = offset[block(o)].V + base(o) + popcount(mask(o) & lower axes).
// Order: vertices by (owning lattice point, axis), faces by (cell, table order): a deterministic function of the
// volume, byte-identical from call to call.  Corner classification: above <=> value > level (a value equal to the
// level counts as below, as in skimage), so a tie never opens the surface.  Vertex on edge (p, p + e_a):
// p + t e_a, t = (level - v(p)) / (v(p + e_a) - v(p)).  Normal: -((1 - t) g(p) + t g(p + e_a)), normalised, g = central
// differences (one-sided at the border): skimage's normals point down the gradient whatever gradient_direction says.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "objnerf_wg.h"

namespace mc_host {
#define OBJNERF_MC_QUAL static const
#include "objnerf_mc_tables.h"
#undef OBJNERF_MC_QUAL
}  // namespace mc_host

namespace mc_dev {
#define OBJNERF_MC_QUAL static __constant__ const
#include "objnerf_mc_tables.h"
#undef OBJNERF_MC_QUAL
}  // namespace mc_dev

namespace {

constexpr int MC_WG = 256;                 // points (and cells) per workgroup: 4 waves
constexpr int MC_SCAN_WG = 1024;

inline long mc_blocks(long n) { return (n + MC_WG - 1) / MC_WG; }

// corner c's linear offset from the cell's lowest point: (c & 1) d^2 + ((c >> 1) & 1) d + ((c >> 2) & 1)
__device__ __forceinline__ long corner_off(const int c, const long d) {
  return (long)(c & 1) * d * d + (long)((c >> 1) & 1) * d + (long)((c >> 2) & 1);
}

__device__ __forceinline__ long axis_stride(const int a, const long d) { return a == 0 ? d * d : (a == 1 ? d : 1); }

// 3-bit crossing mask of the +axis edges point (i, j, k) owns
__device__ __forceinline__ int point_mask(const float* __restrict__ vol, const long p, const int i, const int j,
                                          const int k, const int d, const float level) {
  const bool a0 = vol[p] > level;
  int m = 0;
  if (i + 1 < d && ((vol[p + (long)d * d] > level) != a0)) m |= 1;
  if (j + 1 < d && ((vol[p + d] > level) != a0)) m |= 2;
  if (k + 1 < d && ((vol[p + 1] > level) != a0)) m |= 4;
  return m;
}

// the case of the cell whose lowest corner is (i, j, k), -1 without such a cell
__device__ __forceinline__ int cell_case(const float* __restrict__ vol, const long p, const int i, const int j,
                                         const int k, const int d, const float level) {
  if (i + 1 >= d || j + 1 >= d || k + 1 >= d) return -1;
  int c = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) c |= (vol[p + corner_off(q, d)] > level) << q;
  return c;
}

// exclusive prefix over the workgroup of a value of at most 3 bits, and the workgroup total: a ballot per bit into
// objnerf_wg.h's halves, one barrier.  (wg_exclusive's integer form, a wave scan, measured 7 - 8 % slower on each of
// the three kernels below: profiles/wg_prims_refactor.txt.)
__device__ __forceinline__ int wg_prefix3(const int v, int* wsum, int& total) {
  int pre = 0, tot = 0;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const unsigned long long bal = __ballot((v >> b) & 1);
    pre += wave_rank(bal) << b;
    tot += __popcll(bal) << b;
  }
  return wg_fold<MC_WG>((threadIdx.x & 63) == 0, tot, wsum, total) + pre;
}

__device__ __forceinline__ void point_coords(const long p, const int d, int& i, int& j, int& k) {
  k = (int)(p % d);
  const long r = p / d;
  j = (int)(r % d);
  i = (int)(r / d);
}

__global__ void __launch_bounds__(MC_WG) mc_count_kernel(const float* __restrict__ vol, int d, float level, long n,
                                                         long long* __restrict__ blk) {
  __shared__ int wsum_v[MC_WG / 64], wsum_f[MC_WG / 64];
  const long p = (long)blockIdx.x * MC_WG + threadIdx.x;
  int nv = 0, nt = 0;
  if (p < n) {
    int i, j, k;
    point_coords(p, d, i, j, k);
    nv = __popc(point_mask(vol, p, i, j, k, d, level));
    const int c = cell_case(vol, p, i, j, k, d, level);
    nt = c < 0 ? 0 : mc_dev::MC_NTRI[c];
  }
  int tv, tf;
  wg_prefix3(nv, wsum_v, tv);
  wg_prefix3(nt, wsum_f, tf);
  if (threadIdx.x == 0) {
    blk[2 * blockIdx.x] = tv;
    blk[2 * blockIdx.x + 1] = tf;
  }
}

__device__ __forceinline__ float grad_axis(const float* __restrict__ vol, const long q, const int c, const int d,
                                           const long s) {
  if (c == 0) return vol[q + s] - vol[q];
  if (c == d - 1) return vol[q] - vol[q - s];
  return (vol[q + s] - vol[q - s]) * 0.5f;
}

__global__ void __launch_bounds__(MC_WG) mc_verts_kernel(const float* __restrict__ vol, int d, float level, long n,
                                                         const long long* __restrict__ blk,
                                                         uint16_t* __restrict__ pt, long long max_v,
                                                         float* __restrict__ verts, float* __restrict__ normals) {
  __shared__ int wsum[MC_WG / 64];
  const long p = (long)blockIdx.x * MC_WG + threadIdx.x;
  int i = 0, j = 0, k = 0, m = 0;
  if (p < n) {
    point_coords(p, d, i, j, k);
    m = point_mask(vol, p, i, j, k, d, level);
  }
  int total;                                  // (unused here)
  const int local = wg_prefix3(__popc(m), wsum, total);
  if (p >= n) return;
  pt[p] = (uint16_t)((local << 3) | m);
  if (!m) return;
  long long vid = blk[2 * blockIdx.x] + local;
  const int ci[3] = {i, j, k};
  const float v0 = vol[p];
  float g0[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) g0[b] = grad_axis(vol, p, ci[b], d, axis_stride(b, d));
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!((m >> a) & 1)) continue;
    if (vid >= max_v) return;
    const long s = axis_stride(a, d);
    const long q = p + s;
    const float v1 = vol[q];
    const float t = (level - v0) / (v1 - v0);
    float x[3] = {(float)i, (float)j, (float)k};
    x[a] += t;
    int cq[3] = {i, j, k};
    cq[a] += 1;
    float nr[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const float g1 = grad_axis(vol, q, cq[b], d, axis_stride(b, d));
      nr[b] = -((1.0f - t) * g0[b] + t * g1);
    }
    const float len = sqrtf(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2]);
    const float inv = len > 0.f ? 1.0f / len : 0.f;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      verts[3 * vid + b] = x[b];
      normals[3 * vid + b] = nr[b] * inv;
    }
    ++vid;
  }
}

__global__ void __launch_bounds__(MC_WG) mc_faces_kernel(const float* __restrict__ vol, int d, float level, long n,
                                                         const long long* __restrict__ blk,
                                                         const uint16_t* __restrict__ pt, int descent,
                                                         long long max_f, int32_t* __restrict__ faces) {
  __shared__ int wsum[MC_WG / 64];
  const long p = (long)blockIdx.x * MC_WG + threadIdx.x;
  int c = -1;
  if (p < n) {
    int i, j, k;
    point_coords(p, d, i, j, k);
    c = cell_case(vol, p, i, j, k, d, level);
  }
  const int nt = c < 0 ? 0 : mc_dev::MC_NTRI[c];
  int total;
  const int local = wg_prefix3(nt, wsum, total);
  if (!nt) return;
  long long fid = blk[2 * blockIdx.x + 1] + local;
  for (int t = 0; t < nt; ++t, ++fid) {
    if (fid >= max_f) return;
    int32_t id[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int e = mc_dev::MC_TRI[c][3 * t + r];
      const int a = mc_dev::MC_EDGE_AXIS[e];
      const long o = p + corner_off(mc_dev::MC_EDGE_C0[e], d);
      const int w = pt[o];
      id[r] = (int32_t)(blk[2 * (o / MC_WG)] + (w >> 3) + __popc(w & 7 & ((1 << a) - 1)));
    }
    faces[3 * fid + 0] = descent ? id[2] : id[0];
    faces[3 * fid + 1] = id[1];
    faces[3 * fid + 2] = descent ? id[0] : id[2];
  }
}

bool mc_dim_ok(int32_t dim) { return dim >= 2 && dim <= 1024; }

}  // namespace

extern "C" {

size_t objnerf_mc_workspace_bytes(int32_t dim) {
  if (!mc_dim_ok(dim)) return 0;
  const long n = (long)dim * dim * dim;
  return align256((size_t)mc_blocks(n) * 2 * sizeof(long long)) + align256((size_t)n * sizeof(uint16_t));
}

int objnerf_mc_count(int32_t dim, float level, const float* vol, void* ws, size_t ws_bytes, int64_t* out_counts,
                     void* stream) {
  (void)hipGetLastError();
  if (!mc_dim_ok(dim) || !vol || !ws || !out_counts || ws_bytes < objnerf_mc_workspace_bytes(dim)) return OBJNERF_EINVAL;
  const long n = (long)dim * dim * dim, nb = mc_blocks(n);
  long long* blk = (long long*)ws;
  hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)nb), dim3(MC_WG), 0, (hipStream_t)stream, vol, dim, level, n, blk);
  CHECK_LAUNCH();
  // one workgroup over nb / 4096 tiles (16 at 256^3, 1024 at 1024^3): the first thing to make multi-workgroup if
  // larger grids matter
  hipLaunchKernelGGL((wg_scan_kernel<MC_SCAN_WG, 2, long long>), dim3(1), dim3(MC_SCAN_WG), 0, (hipStream_t)stream, blk,
                     (int64_t)nb, (long long*)out_counts);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_mc_emit(int32_t dim, float level, int32_t flags, const float* vol, void* ws, size_t ws_bytes,
                    int64_t max_verts, int64_t max_faces, float* out_verts, float* out_normals, int32_t* out_faces,
                    void* stream) {
  (void)hipGetLastError();
  if (!mc_dim_ok(dim) || !vol || !ws || ws_bytes < objnerf_mc_workspace_bytes(dim) || max_verts < 0 || max_faces < 0 ||
      (max_verts > 0 && (!out_verts || !out_normals)) || (max_faces > 0 && !out_faces) || (flags & ~1))
    return OBJNERF_EINVAL;
  const long n = (long)dim * dim * dim, nb = mc_blocks(n);
  const long long* blk = (const long long*)ws;
  uint16_t* pt = (uint16_t*)((char*)ws + align256((size_t)nb * 2 * sizeof(long long)));
  hipLaunchKernelGGL(mc_verts_kernel, dim3((unsigned)nb), dim3(MC_WG), 0, (hipStream_t)stream, vol, dim, level, n, blk, pt,
                     (long long)max_verts, out_verts, out_normals);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(mc_faces_kernel, dim3((unsigned)nb), dim3(MC_WG), 0, (hipStream_t)stream, vol, dim, level, n, blk,
                     (const uint16_t*)pt, flags & OBJNERF_MC_DESCENT, (long long)max_faces, out_faces);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_mc_tables(uint8_t* edge_c0, uint8_t* edge_axis, uint8_t* ntri, uint8_t* tri) {
  if (edge_c0) for (int e = 0; e < 12; ++e) edge_c0[e] = mc_host::MC_EDGE_C0[e];
  if (edge_axis) for (int e = 0; e < 12; ++e) edge_axis[e] = mc_host::MC_EDGE_AXIS[e];
  if (ntri) for (int c = 0; c < 256; ++c) ntri[c] = mc_host::MC_NTRI[c];
  if (tri)
    for (int c = 0; c < 256; ++c)
      for (int s = 0; s < 3 * OBJNERF_MC_MAX_TRIS; ++s) tri[c * 3 * OBJNERF_MC_MAX_TRIS + s] = mc_host::MC_TRI[c][s];
  return OBJNERF_MC_MAX_TRIS;
}

}  // extern "C"
