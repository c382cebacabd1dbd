// Geometry evaluation of a finished map (openobj_amd/map_eval.py; vMAP's accuracy / completion / completion ratio between
// points sampled on two sets of meshes -- the reference has no counterpart):
//
// (a) objnerf_mesh_sample: area-weighted points on S meshes at once.  Everything whose order could matter is an integer:
//       ms_area_kernel    per face 0.5 |(B - A) x (C - A)| in fp64 (a face with a vertex outside [0, V) or a non-finite
//                         area counts as area 0 and sets a status bit);
//       ms_amax_kernel    the exact maximum per segment (a maximum is order-free);
//       ms_weight_kernel  q = (uint64) floor(area / amax * 2^32), in place of the area;
//       ms_scan_kernel    one workgroup per segment: the exclusive integer prefix of q (objnerf_wg.h), W = its total;
//       ms_draw_kernel    sample i of segment s: the Philox block of (s, i, 0) on stream S_MESH, t = mulhi64(x << 32 | y, W),
//                         the face with prefix[k] <= t < prefix[k + 1] by binary search (a face with q = 0 is never it),
//                         then p = (1 - s) A + (s (1 - u2)) B + (s u2) C with s = sqrt(u1), u1 = u01(z), u2 = u01(w).
//     A draw is a function of (seed, s, i): no dependence on N or on the launch geometry.
// (b) objnerf_nearest: for every query of segment s the nearest reference point of segment s, exactly, for any cell side.
//       nn_extent_kernel  the largest cell index per axis and segment, from the sorted keys (integer maxima);
//       nn_ring_kernel    a thread per query.  c0 = the query's cell, clamped into the segment's grid [0, ext].  Ring r =
//                         the cells at Chebyshev distance r from c0; a column (x, y) of the ring is one run of the sorted
//                         keys (its rim) or two single cells (top and bottom).  After ring r every reference point not yet
//                         seen lies r + 1 cells or more from c0 on some axis, so more than r cell away on that axis, up to
//                         the rounding of the cell-index division (at most 2^-31 cells for either point): the search
//                         stops when the best d^2 < (r cell)^2 (1 - 2^-20), STRICTLY (a tie farther out may carry a
//                         smaller row), or when the rings have covered the grid.  A query still open after ring
//                         `max_rings` is marked, and counted per workgroup (count / scan / emit, objnerf_wg.h);
//       nn_emit_kernel    the open queries, in query order;
//       nn_brute_kernel   a workgroup per open query over all reference rows of its segment: per thread ascending rows
//                         (strict <: the smallest row of a tie), then a reduction of (d2, row), by d2, then by row.
//     Both tiers compute dist2 of objnerf_cells.h: (dx dx + dy dy) + dz dz, every operation rounded on its own.
// (c) objnerf_seg_stats: per segment counts, sum, sum of squares, maximum and counts below thresholds, one workgroup per
//     segment: thread-strided partial sums, then a fixed tree.
// No float atomics, no allocation, no synchronisation; fp64 without contraction; two calls write the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "objnerf_wg.h"
#include "objnerf_cells.h"
#include "objnerf_philox.h"

namespace {

constexpr int ME_WG = 256;
constexpr int ME_SCAN_WG = 1024;
constexpr int NN_RINGS = 2;           // the last ring of tier 1 (profiles/mapeval_bench.txt)
constexpr int NN_RINGS_MAX = 64;
constexpr int NN_BRUTE_GRID = 4096;
constexpr int64_t NN_OPEN = -2;       // out_idx of a query tier 1 left open
constexpr double NN_SLACK = 1.0 - 1.0 / 1048576.0;        // 1 - 2^-20, as ops._CELL_SLACK

enum : int32_t { MS_BAD_INDEX = 1, MS_BAD_AREA = 2, MS_NO_AREA = 4 };
enum : int32_t { NN_BAD_QUERY = 1 };

__device__ __forceinline__ void seg_clamp(const int64_t* __restrict__ off, const int s, const int64_t n, int64_t& lo,
                                          int64_t& hi) {
  lo = off[s]; hi = off[s + 1];
  lo = lo < 0 ? 0 : lo; hi = hi > n ? n : hi;
}

// ------------------------------------------------------------------------------------------------------ mesh sampling
struct MsLayout { size_t q, amax, wtot, total; };

inline MsLayout ms_layout(int64_t F, int32_t S) {
  MsLayout L;
  size_t o = 0;
  L.q = o;    o += align256(sizeof(int64_t) * (size_t)F);       // the area (fp64), then q, then its prefix: one slot a face
  L.amax = o; o += align256(sizeof(double) * (size_t)S);
  L.wtot = o; o += align256(sizeof(int64_t) * (size_t)S);
  L.total = o;
  return L;
}

__global__ void __launch_bounds__(ME_WG) ms_area_kernel(const int64_t V, const int64_t F, const double* __restrict__ verts,
                                                        const int32_t* __restrict__ faces, double* __restrict__ area,
                                                        int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * ME_WG + threadIdx.x;
  if (f >= F) return;
  const int64_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) {
    area[f] = 0.0;
    atomicOr(status, MS_BAD_INDEX);
    return;
  }
  const double* A = verts + 3 * ia, *B = verts + 3 * ib, *Cc = verts + 3 * ic;
  const double e1[3] = {__dsub_rn(B[0], A[0]), __dsub_rn(B[1], A[1]), __dsub_rn(B[2], A[2])};
  const double e2[3] = {__dsub_rn(Cc[0], A[0]), __dsub_rn(Cc[1], A[1]), __dsub_rn(Cc[2], A[2])};
  const double cx = __dsub_rn(__dmul_rn(e1[1], e2[2]), __dmul_rn(e1[2], e2[1]));
  const double cy = __dsub_rn(__dmul_rn(e1[2], e2[0]), __dmul_rn(e1[0], e2[2]));
  const double cz = __dsub_rn(__dmul_rn(e1[0], e2[1]), __dmul_rn(e1[1], e2[0]));
  const double a = __dmul_rn(0.5, __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(cx, cx), __dmul_rn(cy, cy)), __dmul_rn(cz, cz))));
  const bool ok = a - a == 0.0;                             // false for a NaN or an infinity
  area[f] = ok ? a : 0.0;
  if (!ok) atomicOr(status, MS_BAD_AREA);
}

// one workgroup per segment
__global__ void __launch_bounds__(ME_WG) ms_amax_kernel(const int64_t F, const double* __restrict__ area,
                                                        const int64_t* __restrict__ face_off, double* __restrict__ amax) {
  const int s = blockIdx.x;
  int64_t lo, hi;
  seg_clamp(face_off, s, F, lo, hi);
  double m = 0.0;
  for (int64_t f = lo + threadIdx.x; f < hi; f += ME_WG) m = fmax(m, area[f]);
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  __shared__ double red[ME_WG / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < ME_WG / 64; ++w) m = fmax(m, red[w]);
    amax[s] = m;
  }
}

__global__ void __launch_bounds__(ME_WG) ms_weight_kernel(const int64_t F, const int S, int64_t* __restrict__ q,
                                                          const int64_t* __restrict__ face_off,
                                                          const double* __restrict__ amax) {
  const int64_t f = (int64_t)blockIdx.x * ME_WG + threadIdx.x;
  if (f >= F) return;
  const double a = __longlong_as_double(q[f]);
  const double m = amax[seg_of(face_off, S, f)];
  // area / amax is in [0, 1]; times 2^32 is exact
  q[f] = m > 0.0 ? (int64_t)(uint64_t)floor(__dmul_rn(__ddiv_rn(a, m), 4294967296.0)) : 0;
}

// one workgroup per segment: q -> its exclusive prefix in place, W[s] = the total
__global__ void __launch_bounds__(ME_SCAN_WG) ms_scan_kernel(const int64_t F, int64_t* __restrict__ q,
                                                             const int64_t* __restrict__ face_off,
                                                             int64_t* __restrict__ wtot) {
  const int s = blockIdx.x;
  int64_t lo, hi;
  seg_clamp(face_off, s, F, lo, hi);
  int64_t t[1];
  wg_scan_exclusive<ME_SCAN_WG, 1>(q + lo, q + lo, hi > lo ? hi - lo : 0, t);
  if (threadIdx.x == 0) wtot[s] = t[0];
}

struct MsDraw {
  int64_t F, N; int S;
  const double* verts; const int32_t* faces; const int64_t* face_off; const int64_t* samp_off;
  const int64_t* prefix; const int64_t* wtot;
  uint64_t seed;
  double* out_pts; int32_t* out_tri; int32_t* status;
};

__global__ void __launch_bounds__(ME_WG) ms_draw_kernel(const MsDraw a) {
  const int64_t j = (int64_t)blockIdx.x * ME_WG + threadIdx.x;
  if (j >= a.N) return;
  const int s = seg_of(a.samp_off, a.S, j);
  const int64_t i = j - a.samp_off[s];
  const uint64_t W = (uint64_t)a.wtot[s];
  int64_t lo, hi;
  seg_clamp(a.face_off, s, a.F, lo, hi);
  double* o = a.out_pts + 3 * j;
  if (W == 0 || hi <= lo) {
    o[0] = o[1] = o[2] = NAN;
    a.out_tri[j] = -1;
    atomicOr(a.status, MS_NO_AREA);
    return;
  }
  const objrng::U4 r = objrng::philox4x32_10(objrng::U4{(uint32_t)s, (uint32_t)i, 0u, objrng::S_MESH}, (uint32_t)a.seed,
                                             (uint32_t)(a.seed >> 32));
  const uint64_t t = __umul64hi(((uint64_t)r.x << 32) | r.y, W);
  // the last k with prefix[k] <= t: t < W, so q[k] > 0
  int64_t l = lo, h = hi;
  while (h - l > 1) {
    const int64_t m = (l + h) >> 1;
    if ((uint64_t)a.prefix[m] <= t) l = m; else h = m;
  }
  const int32_t* fc = a.faces + 3 * l;                      // q > 0: ms_area_kernel found its three rows inside [0, V)
  const double* A = a.verts + 3 * (int64_t)fc[0], *B = a.verts + 3 * (int64_t)fc[1], *Cc = a.verts + 3 * (int64_t)fc[2];
  const double u1 = (double)objrng::u01(r.z), u2 = (double)objrng::u01(r.w);
  const double sq = __dsqrt_rn(u1);
  const double wa = __dsub_rn(1.0, sq), wb = __dmul_rn(sq, __dsub_rn(1.0, u2)), wc = __dmul_rn(sq, u2);
  for (int c = 0; c < 3; ++c)
    o[c] = __dadd_rn(__dadd_rn(__dmul_rn(wa, A[c]), __dmul_rn(wb, B[c])), __dmul_rn(wc, Cc[c]));
  a.out_tri[j] = (int32_t)l;
}

// ------------------------------------------------------------------------------------------------------ nearest point
struct NnLayout { size_t ext, blk, list, total; int64_t nb; };

inline NnLayout nn_layout(int64_t nq, int32_t S) {
  NnLayout L;
  L.nb = cdiv(nq, ME_WG);
  size_t o = 0;
  L.ext = o;  o += align256(sizeof(int32_t) * 3 * (size_t)S);
  L.blk = o;  o += align256(sizeof(int32_t) * (size_t)(L.nb + 1));
  L.list = o; o += align256(sizeof(int32_t) * (size_t)nq);
  L.total = o;
  return L;
}

struct NnArgs {
  int64_t nr, nq; int S; int rings;
  const double* ref; const int64_t* r_off; const int64_t* keys; const int64_t* perm; const double* mins;
  double cell;
  const double* qry; const int64_t* q_off;
  int32_t* ext; int32_t* blk; int32_t* list;
  double* out_d2; int64_t* out_idx; int32_t* status;
};

// one workgroup per segment: the largest cell index on every axis
__global__ void __launch_bounds__(ME_WG) nn_extent_kernel(const NnArgs a) {
  const int s = blockIdx.x;
  int64_t lo, hi;
  seg_clamp(a.r_off, s, a.nr, lo, hi);
  int m[3] = {0, 0, 0};
  for (int64_t e = lo + threadIdx.x; e < hi; e += ME_WG) {
    const int64_t k = a.keys[e];
    m[0] = max(m[0], (int)((k >> (2 * CELL_BITS)) & CELL_MAX));
    m[1] = max(m[1], (int)((k >> CELL_BITS) & CELL_MAX));
    m[2] = max(m[2], (int)(k & CELL_MAX));
  }
  __shared__ int red[ME_WG / 64][3];
  for (int c = 0; c < 3; ++c)
    for (int o = 32; o > 0; o >>= 1) m[c] = max(m[c], __shfl_xor(m[c], o));
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < 3; ++c) red[threadIdx.x >> 6][c] = m[c];
  __syncthreads();
  if (threadIdx.x < 3) {
    int v = red[0][threadIdx.x];
    for (int w = 1; w < ME_WG / 64; ++w) v = max(v, red[w][threadIdx.x]);
    a.ext[3 * s + threadIdx.x] = v;
  }
}

struct Best { double d2; int64_t row; };

__device__ __forceinline__ void take(Best& b, const double d2, const int64_t row) {
  if (d2 < b.d2 || (d2 == b.d2 && row < b.row)) { b.d2 = d2; b.row = row; }
}

// the reference points of the cells (x, y, za .. zb): one run of the segment's sorted keys
__device__ __forceinline__ void scan_run(const NnArgs& a, const int64_t lo, const int64_t hi, const int64_t x, const int64_t y,
                                         const int64_t za, const int64_t zb, const double q[3], Best& b) {
  const int64_t k1 = cell_key(x, y, zb);
  for (int64_t e = lower_bound(a.keys, lo, hi, cell_key(x, y, za)); e < hi && a.keys[e] <= k1; ++e) {
    const int64_t row = a.perm[e];
    if ((uint64_t)row >= (uint64_t)a.nr) continue;          // (a permutation has no such entry; never read past)
    take(b, dist2(a.ref + 3 * row, q), row);
  }
}

__global__ void __launch_bounds__(ME_WG) nn_ring_kernel(const NnArgs a) {
  const int64_t i = (int64_t)blockIdx.x * ME_WG + threadIdx.x;
  bool open = false;
  if (i < a.nq) {
    const int s = seg_of(a.q_off, a.S, i);
    int64_t lo, hi;
    seg_clamp(a.r_off, s, a.nr, lo, hi);
    const double q[3] = {a.qry[3 * i], a.qry[3 * i + 1], a.qry[3 * i + 2]};
    Best b = {INFINITY, -1};
    if (!(q[0] - q[0] == 0.0 && q[1] - q[1] == 0.0 && q[2] - q[2] == 0.0)) {
      atomicOr(a.status, NN_BAD_QUERY);
    } else if (hi > lo) {
      b.row = INT64_MAX;
      int64_t c0[3], ext[3], rmax = 0;
      for (int c = 0; c < 3; ++c) {
        // the query's signed cell index, clamped into the grid (a query outside only gains distance by it)
        const double v = floor(__ddiv_rn(__dsub_rn(q[c], a.mins[3 * s + c]), a.cell));
        ext[c] = a.ext[3 * s + c];
        c0[c] = !(v > 0.0) ? 0 : v >= (double)ext[c] ? ext[c] : (int64_t)v;
        rmax = max(rmax, max(c0[c], ext[c] - c0[c]));
      }
      open = true;
      for (int64_t r = 0; r <= a.rings; ++r) {
        const int64_t x0 = max(c0[0] - r, (int64_t)0), x1 = min(c0[0] + r, ext[0]);
        const int64_t y0 = max(c0[1] - r, (int64_t)0), y1 = min(c0[1] + r, ext[1]);
        const int64_t zl = c0[2] - r, zh = c0[2] + r;
        for (int64_t x = x0; x <= x1; ++x)
          for (int64_t y = y0; y <= y1; ++y) {
            const bool rim = x - c0[0] == r || c0[0] - x == r || y - c0[1] == r || c0[1] - y == r;
            if (rim) {
              scan_run(a, lo, hi, x, y, max(zl, (int64_t)0), min(zh, ext[2]), q, b);
            } else {
              if (zl >= 0) scan_run(a, lo, hi, x, y, zl, zl, q, b);
              if (zh <= ext[2]) scan_run(a, lo, hi, x, y, zh, zh, q, b);
            }
          }
        const double rc = __dmul_rn((double)r, a.cell);
        if (r >= rmax || b.d2 < __dmul_rn(__dmul_rn(rc, rc), NN_SLACK)) { open = false; break; }
      }
      if (b.row == INT64_MAX) b.row = -1;
    }
    a.out_d2[i] = b.d2;
    a.out_idx[i] = open ? NN_OPEN : b.row;
  }
  __shared__ int wcnt[ME_WG / 64];
  int c;
  wg_exclusive_flag<ME_WG>(open, wcnt, c);
  if (threadIdx.x == 0) a.blk[blockIdx.x] = c;
}

__global__ void __launch_bounds__(ME_WG) nn_emit_kernel(const NnArgs a) {
  const int64_t i = (int64_t)blockIdx.x * ME_WG + threadIdx.x;
  const bool open = i < a.nq && a.out_idx[i] == NN_OPEN;
  __shared__ int wcnt[ME_WG / 64];
  int total;
  const int64_t pos = (int64_t)a.blk[blockIdx.x] + wg_exclusive_flag<ME_WG>(open, wcnt, total);
  if (open && pos >= 0 && pos < a.nq) a.list[pos] = (int32_t)i;
}

__global__ void __launch_bounds__(ME_WG) nn_brute_kernel(const NnArgs a, const int64_t nb) {
  __shared__ double rd[ME_WG / 64];
  __shared__ int64_t rr[ME_WG / 64];
  int64_t n_open = a.blk[nb];
  n_open = n_open > a.nq ? a.nq : n_open;
  for (int64_t o = blockIdx.x; o < n_open; o += gridDim.x) {
    const int64_t i = a.list[o];
    if ((uint64_t)i >= (uint64_t)a.nq) continue;            // (workgroup-uniform)
    const int s = seg_of(a.q_off, a.S, i);
    int64_t lo, hi;
    seg_clamp(a.r_off, s, a.nr, lo, hi);
    const double q[3] = {a.qry[3 * i], a.qry[3 * i + 1], a.qry[3 * i + 2]};
    Best b = {INFINITY, INT64_MAX};
    for (int64_t e = lo + threadIdx.x; e < hi; e += ME_WG) take(b, dist2(a.ref + 3 * e, q), e);
    for (int w = 32; w > 0; w >>= 1) {
      const double od = __shfl_xor(b.d2, w);
      const int64_t orow = __shfl_xor((long long)b.row, w);
      take(b, od, orow);
    }
    __syncthreads();                                        // (the query before has read rd / rr)
    if ((threadIdx.x & 63) == 0) { rd[threadIdx.x >> 6] = b.d2; rr[threadIdx.x >> 6] = b.row; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < ME_WG / 64; ++w) take(b, rd[w], rr[w]);
      a.out_d2[i] = b.d2;
      a.out_idx[i] = b.row == INT64_MAX ? -1 : b.row;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- stats
constexpr int ST_MAX_T = 4;
struct StArgs { int64_t n; int T; double thr[ST_MAX_T]; const double* d; const int64_t* off; double* out; };

__global__ void __launch_bounds__(ME_WG) seg_stats_kernel(const StArgs a) {
  const int s = blockIdx.x;
  int64_t lo, hi;
  seg_clamp(a.off, s, a.n, lo, hi);
  // 0 finite, 1 non-finite, 2 sum, 3 sum of squares, 4 max, 5.. counts below the thresholds (counts are exact in fp64)
  double v[5 + ST_MAX_T] = {0.0, 0.0, 0.0, 0.0, -INFINITY, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = lo + threadIdx.x; i < hi; i += ME_WG) {
    const double d = a.d[i];
    if (!(d - d == 0.0)) { v[1] += 1.0; continue; }
    v[0] += 1.0;
    v[2] = __dadd_rn(v[2], d);
    v[3] = __dadd_rn(v[3], __dmul_rn(d, d));
    v[4] = fmax(v[4], d);
    for (int t = 0; t < ST_MAX_T; ++t) v[5 + t] += t < a.T && d < a.thr[t] ? 1.0 : 0.0;
  }
  __shared__ double red[5 + ST_MAX_T][ME_WG];
  for (int c = 0; c < 5 + ST_MAX_T; ++c) red[c][threadIdx.x] = v[c];
  __syncthreads();
  for (int w = ME_WG / 2; w > 0; w >>= 1) {                 // a fixed tree: thread t takes t + w
    if ((int)threadIdx.x < w)
      for (int c = 0; c < 5 + ST_MAX_T; ++c) {
        const double x = red[c][threadIdx.x], y = red[c][threadIdx.x + w];
        red[c][threadIdx.x] = c == 4 ? fmax(x, y) : __dadd_rn(x, y);
      }
    __syncthreads();
  }
  if ((int)threadIdx.x < 5 + a.T) a.out[(int64_t)s * (5 + a.T) + threadIdx.x] = red[threadIdx.x][0];
}

}  // namespace

extern "C" {

size_t objnerf_mesh_sample_workspace_bytes(int64_t F, int32_t S) {
  if (F < 0 || F > 0x7fffffff || S <= 0) return 0;
  return ms_layout(F > 0 ? F : 1, S).total;
}

int objnerf_mesh_sample(int64_t V, int64_t F, int32_t S, int64_t N, const double* verts, const int32_t* faces,
                        const int64_t* face_off, const int64_t* samp_off, uint64_t seed, void* ws, size_t ws_bytes,
                        double* out_pts, int32_t* out_tri, int32_t* status, void* stream) {
  if (V < 0 || V > 0x7fffffff || F < 0 || F > 0x7fffffff || S <= 0 || S > 0x7fffffff || N < 0 || N > 0x7fffffff ||
      !face_off || !samp_off || !status)
    return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return OBJNERF_ELAUNCH;
  if (N == 0) return OBJNERF_OK;
  if (!out_pts || !out_tri) return OBJNERF_EINVAL;
  if (F > 0 && (!verts || !faces)) return OBJNERF_EINVAL;
  const MsLayout L = ms_layout(F > 0 ? F : 1, S);          // (no face anywhere: every sample reports MS_NO_AREA)
  if (!ws || ws_bytes < L.total) return OBJNERF_EINVAL;
  MsDraw a;
  a.F = F; a.N = N; a.S = S; a.verts = verts; a.faces = faces; a.face_off = face_off; a.samp_off = samp_off; a.seed = seed;
  a.out_pts = out_pts; a.out_tri = out_tri; a.status = status;
  char* w = (char*)ws;
  int64_t* q = (int64_t*)(w + L.q);
  double* amax = (double*)(w + L.amax);
  int64_t* wtot = (int64_t*)(w + L.wtot);
  a.prefix = q; a.wtot = wtot;
  if (F > 0) {
    const dim3 fgrid((unsigned)cdiv(F, ME_WG));
    hipLaunchKernelGGL(ms_area_kernel, fgrid, dim3(ME_WG), 0, st, V, F, verts, faces, (double*)q, status);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(ms_amax_kernel, dim3((unsigned)S), dim3(ME_WG), 0, st, F, (const double*)q, face_off, amax);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(ms_weight_kernel, fgrid, dim3(ME_WG), 0, st, F, S, q, face_off, (const double*)amax);
    CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(ms_scan_kernel, dim3((unsigned)S), dim3(ME_SCAN_WG), 0, st, F, q, face_off, wtot);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(ms_draw_kernel, dim3((unsigned)cdiv(N, ME_WG)), dim3(ME_WG), 0, st, a);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

size_t objnerf_nearest_workspace_bytes(int64_t nq, int32_t S) {
  if (nq <= 0 || nq > 0x7fffffff || S <= 0) return 0;
  return nn_layout(nq, S).total;
}

int objnerf_nearest(int64_t nr, int64_t nq, int32_t S, const double* ref, const int64_t* r_off, const int64_t* sorted_keys,
                    const int64_t* perm, const double* mins, double cell, const double* qry, const int64_t* q_off,
                    int32_t max_rings, void* ws, size_t ws_bytes, double* out_d2, int64_t* out_idx, int32_t* status,
                    void* stream) {
  if (nr < 0 || nr > 0x7fffffff || nq < 0 || nq > 0x7fffffff || S <= 0 || S > 0x7fffffff || !r_off || !q_off || !mins ||
      !status || !(cell > 0.0) || max_rings > NN_RINGS_MAX)
    return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return OBJNERF_ELAUNCH;
  if (nq == 0) return OBJNERF_OK;
  if (!qry || !out_d2 || !out_idx || !ws) return OBJNERF_EINVAL;
  if (nr > 0 && (!ref || !sorted_keys || !perm)) return OBJNERF_EINVAL;
  const NnLayout L = nn_layout(nq, S);
  if (ws_bytes < L.total) return OBJNERF_EINVAL;
  char* w = (char*)ws;
  NnArgs a;
  a.nr = nr; a.nq = nq; a.S = S; a.rings = max_rings > 0 ? max_rings : NN_RINGS;
  a.ref = ref; a.r_off = r_off; a.keys = sorted_keys; a.perm = perm; a.mins = mins; a.cell = cell; a.qry = qry; a.q_off = q_off;
  a.ext = (int32_t*)(w + L.ext); a.blk = (int32_t*)(w + L.blk); a.list = (int32_t*)(w + L.list);
  a.out_d2 = out_d2; a.out_idx = out_idx; a.status = status;
  const dim3 grid((unsigned)L.nb), wg(ME_WG);
  hipLaunchKernelGGL(nn_extent_kernel, dim3((unsigned)S), wg, 0, st, a);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(nn_ring_kernel, grid, wg, 0, st, a);
  CHECK_LAUNCH();
  // blk[0 .. nb) -> exclusive offsets, blk[nb] = the number of open queries
  hipLaunchKernelGGL((wg_scan_kernel<ME_SCAN_WG, 1, int32_t>), dim3(1), dim3(ME_SCAN_WG), 0, st, a.blk, L.nb, a.blk + L.nb);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(nn_emit_kernel, grid, wg, 0, st, a);
  CHECK_LAUNCH();
  const int64_t bg = nq < NN_BRUTE_GRID ? nq : NN_BRUTE_GRID;
  hipLaunchKernelGGL(nn_brute_kernel, dim3((unsigned)bg), wg, 0, st, a, L.nb);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_seg_stats(int64_t n, int32_t S, const double* d, const int64_t* off, int32_t T, const double* thresholds,
                      double* out, void* stream) {
  if (n < 0 || S <= 0 || S > 0x7fffffff || !off || !out || T < 0 || T > ST_MAX_T || (T > 0 && !thresholds) || (n > 0 && !d))
    return OBJNERF_EINVAL;
  StArgs a;
  a.n = n; a.T = T; a.d = d; a.off = off; a.out = out;
  for (int t = 0; t < ST_MAX_T; ++t) a.thr[t] = t < T ? thresholds[t] : 0.0;
  hipLaunchKernelGGL(seg_stats_kernel, dim3((unsigned)S), dim3(ME_WG), 0, (hipStream_t)stream, a);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

}  // extern "C"
