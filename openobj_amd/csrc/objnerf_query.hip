// Open-vocabulary queries over the exported map: the numerical core of visualization/vis_interaction.py, which the
// reference runs per object through torch / sklearn / matplotlib on the host.
//
//   project_kernel        out [V][Q] = f . W + b for every row of every segment (f / max(|f|, 1e-8) against
//                         W[:, q] / max(|W[:, q]|, 1e-8) with OBJNERF_PROJ_COSINE: F.cosine_similarity, :372, :388),
//                         W [D][Q] (Q <= 16) in LDS as the B operand of v_mfma_f32_16x16x4_f32, a 16-row block of f
//                         as the A operand (k-step j of chunk c takes column 16 c + 4 g + j from lane group g: each lane
//                         streams float4s of its row); per-workgroup min / max of every column of its segment;
//   project_minmax_kernel the segment's min / max over its workgroups (min / max are order-free: exact).
//   moments_mean_kernel / moments_mean_finish_kernel
//                         fp64 column sums of contiguous row chunks, combined chunk by chunk in fp64 -> the mean;
//   moments_scatter_kernel
//                         one 64 x 64 tile (ti <= tj) of sum (f - m)(f - m)^T per workgroup: 32 rows at a time are
//                         centred (fp32 mean) into LDS, 4 waves x (2 x 2) v_mfma_f32_16x16x4_f32 blocks accumulate in
//                         fp32 and fold into fp64 registers every 128 rows; the tile and its mirror are written;
//   moments_scatter_sum_kernel
//                         the row-split partial tiles (small S only) summed in split order in fp64;
//   color_kernel          per-vertex colours from a per-segment mode: RGB x factor (:299-301, :347-349), a constant
//                         (:337-345), matplotlib's "rainbow" of a normalised column (:329-332, :389-392), or the PCA
//                         colouring (:211-214) with sklearn 1.3.2's u-based sign rule taken from the column min / max.
// No float atomics anywhere: every output is a fixed function of the inputs, byte-identical from call to call.
// Built with -ffp-contract=off and without fast-math: the colour arithmetic is that of the numpy / torch statement.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include "objnerf_wg.h"

namespace {

constexpr int PJ_WG = 256;                      // 4 waves
constexpr int PJ_RB = 4;                        // 16-row blocks per wave and pass
constexpr int PJ_ROWS = (PJ_WG / 64) * PJ_RB * 16;   // rows per workgroup pass
constexpr int PJ_TARGET = 8192;                 // workgroups aimed at over all segments
constexpr int MM_WG = 256;
constexpr int MM_TARGET = 2048;
constexpr int SC_T = 64;                        // scatter tile edge
constexpr int SC_K = 32;                        // rows staged per LDS pass
constexpr int SC_PAD = 80;                      // LDS row pitch (floats): rows 0 / 1 of a k-step on disjoint banks
constexpr int SC_FOLD = 4;                      // LDS passes between fp64 folds (128 rows)
constexpr int SC_TARGET = 1024;
constexpr int SC_MAX_SPLIT = 16;
constexpr int CL_WG = 256;

inline int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// workgroups per segment: enough in total to fill the GPU, never more passes than rows
inline int pj_split(int S, int64_t V) {
  return (int)clamp64(std::min<int64_t>(cdiv(PJ_TARGET, S), cdiv(V, (int64_t)S * PJ_ROWS)), 1, 65535);
}
inline int mm_split(int S, int D) { return (int)clamp64(cdiv(MM_TARGET, (int64_t)S * cdiv(D, MM_WG)), 1, 256); }
inline int sc_pairs(int D) { const int T = (int)cdiv(D, SC_T); return T * (T + 1) / 2; }
inline int sc_split(int S, int D) { return (int)clamp64(cdiv(SC_TARGET, (int64_t)S * sc_pairs(D)), 1, SC_MAX_SPLIT); }

// segment bounds clamped to [0, V]: a bad offset never reads or writes past the arrays
__device__ __forceinline__ int64_t seg_at(const int64_t* off, int s, int64_t V) {
  const int64_t v = off[s];
  return v < 0 ? 0 : (v > V ? V : v);
}

// ------------------------------------------------------------------------------------------------ projection
// NCH: 16-column chunks the LDS copy of W holds (D <= 16 NCH)
template <int NCH, bool VEC>
__global__ void __launch_bounds__(PJ_WG) project_kernel(const objnerf_project_args a, float* __restrict__ part) {
  const int s = blockIdx.y;
  const int D = a.D, Q = a.Q, nch = (D + 15) / 16;
  const bool per = (a.flags & OBJNERF_PROJ_PER_SEGMENT) != 0;
  const float* __restrict__ W = a.W + (per ? (int64_t)s * D * Q : 0);
  const float* __restrict__ B = a.bias ? a.bias + (per ? (int64_t)s * Q : 0) : nullptr;
  __shared__ float4 sw[NCH * 64];                         // [chunk][g][q]: W[16 c + 4 g + j][q] in element j
  __shared__ float red[PJ_WG];
  __shared__ float snorm[16];
  __shared__ float smm[PJ_WG / 64][16][2];
  for (int t = threadIdx.x; t < nch * 64; t += PJ_WG) {
    const int c = t >> 6, g = (t >> 4) & 3, q = t & 15;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 16 * c + 4 * g + j;
      v[j] = (k < D && q < Q) ? W[(int64_t)k * Q + q] : 0.f;
    }
    sw[t] = make_float4(v[0], v[1], v[2], v[3]);
  }
  __syncthreads();
  const bool cosine = (a.flags & OBJNERF_PROJ_COSINE) != 0;
  if (cosine) {                                           // W[:, q] / max(|W[:, q]|, 1e-8), fixed summation order
    const int q = threadIdx.x & 15, p = threadIdx.x >> 4;
    float acc = 0.f;
    for (int c = p; c < nch; c += 16)
      for (int g = 0; g < 4; ++g) {
        const float4 w = sw[c * 64 + g * 16 + q];
        acc = fmaf(w.x, w.x, acc); acc = fmaf(w.y, w.y, acc); acc = fmaf(w.z, w.z, acc); acc = fmaf(w.w, w.w, acc);
      }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < 16) {
      float n2 = 0.f;
      for (int pp = 0; pp < 16; ++pp) n2 += red[pp * 16 + threadIdx.x];
      snorm[threadIdx.x] = fmaxf(sqrtf(n2), 1e-8f);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nch * 64; t += PJ_WG) {
      const float n = snorm[t & 15];
      float4 w = sw[t];
      w.x = w.x / n; w.y = w.y / n; w.z = w.z / n; w.w = w.w / n;
      sw[t] = w;
    }
    __syncthreads();
  }
  const int64_t r0 = seg_at(a.seg_off, s, a.V), r1 = seg_at(a.seg_off, s + 1, a.V);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4, q = lane & 15;
  const float bq = (B && q < Q) ? B[q] : 0.f;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t base = r0 + (int64_t)blockIdx.x * PJ_ROWS; base < r1; base += (int64_t)gridDim.x * PJ_ROWS) {
    const int64_t wb = base + (int64_t)wv * PJ_RB * 16;
    floatx4 acc[PJ_RB];
    float ss[PJ_RB];
    const float* rp[PJ_RB];
    bool rv[PJ_RB];
#pragma unroll
    for (int b = 0; b < PJ_RB; ++b) {
      const int64_t row = wb + 16 * b + r;
      rv[b] = row < r1;
      rp[b] = a.feat + (rv[b] ? row : r0) * a.row_stride;
      acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};
      ss[b] = 0.f;
    }
    for (int c = 0; c < nch; ++c) {
      const float4 w = sw[c * 64 + g * 16 + q];
      const int k0 = 16 * c + 4 * g;
      float4 f[PJ_RB];
#pragma unroll
      for (int b = 0; b < PJ_RB; ++b) f[b] = load_row4<VEC>(rp[b], k0, D, rv[b]);
#pragma unroll
      for (int b = 0; b < PJ_RB; ++b) {
        if (cosine) {
          ss[b] = fmaf(f[b].x, f[b].x, ss[b]); ss[b] = fmaf(f[b].y, f[b].y, ss[b]);
          ss[b] = fmaf(f[b].z, f[b].z, ss[b]); ss[b] = fmaf(f[b].w, f[b].w, ss[b]);
        }
        acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[b].x, w.x, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[b].y, w.y, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[b].z, w.z, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[b].w, w.w, acc[b], 0, 0, 0);
      }
    }
#pragma unroll
    for (int b = 0; b < PJ_RB; ++b) {
      if (cosine) {                                       // lanes r, r + 16, r + 32, r + 48 hold row r's parts
        ss[b] += __shfl_xor(ss[b], 16);
        ss[b] += __shfl_xor(ss[b], 32);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {                       // C/D: column q = lane & 15, row 4 g + e
        const int rr = 4 * g + e;
        float v = acc[b][e];
        if (cosine) v = v / fmaxf(sqrtf(__shfl(ss[b], rr)), 1e-8f);
        v = v + bq;
        const int64_t row = wb + 16 * b + rr;
        if (row < r1 && q < Q) {
          a.out[row * Q + q] = v;
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
        }
      }
    }
  }
  mn = fminf(mn, __shfl_xor(mn, 16)); mn = fminf(mn, __shfl_xor(mn, 32));
  mx = fmaxf(mx, __shfl_xor(mx, 16)); mx = fmaxf(mx, __shfl_xor(mx, 32));
  if (lane < 16) { smm[wv][lane][0] = mn; smm[wv][lane][1] = mx; }
  __syncthreads();
  if (threadIdx.x < (unsigned)Q) {
    float lo = smm[0][threadIdx.x][0], hi = smm[0][threadIdx.x][1];
    for (int w = 1; w < PJ_WG / 64; ++w) { lo = fminf(lo, smm[w][threadIdx.x][0]); hi = fmaxf(hi, smm[w][threadIdx.x][1]); }
    float* p = part + (((int64_t)s * gridDim.x + blockIdx.x) * Q + threadIdx.x) * 2;
    p[0] = lo;
    p[1] = hi;
  }
}

__global__ void project_minmax_kernel(const int S, const int Q, const int G, const float* __restrict__ part,
                                      float* __restrict__ minmax) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)S * Q) return;
  const int64_t s = i / Q, q = i % Q;
  float lo = INFINITY, hi = -INFINITY;
  for (int g = 0; g < G; ++g) {
    const float* p = part + ((s * G + g) * Q + q) * 2;
    lo = fminf(lo, p[0]);
    hi = fmaxf(hi, p[1]);
  }
  minmax[2 * i] = lo;
  minmax[2 * i + 1] = hi;
}

// ------------------------------------------------------------------------------------------------ moments
__global__ void __launch_bounds__(MM_WG) moments_mean_kernel(const objnerf_moments_args a, double* __restrict__ part) {
  const int d = blockIdx.x * MM_WG + threadIdx.x, s = blockIdx.y, G = gridDim.z, gz = blockIdx.z;
  const int64_t r0 = seg_at(a.seg_off, s, a.V), r1 = seg_at(a.seg_off, s + 1, a.V);
  const int64_t n = r1 > r0 ? r1 - r0 : 0, chunk = (n + G - 1) / G;
  const int64_t lo = r0 + gz * chunk, hi = r1 < lo + chunk ? r1 : lo + chunk;
  if (d >= a.D) return;
  double s0 = 0.0, s1 = 0.0;                              // two chains (even / odd rows), joined once
  int64_t i = lo;
  for (; i + 1 < hi; i += 2) {
    s0 += (double)a.feat[i * a.row_stride + d];
    s1 += (double)a.feat[(i + 1) * a.row_stride + d];
  }
  if (i < hi) s0 += (double)a.feat[i * a.row_stride + d];
  part[((int64_t)s * G + gz) * a.D + d] = s0 + s1;
}

__global__ void moments_mean_finish_kernel(const objnerf_moments_args a, const int G, const double* __restrict__ part) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)a.S * a.D) return;
  const int64_t s = i / a.D, d = i % a.D;
  const int64_t n = seg_at(a.seg_off, (int)s + 1, a.V) - seg_at(a.seg_off, (int)s, a.V);
  double t = 0.0;
  for (int g = 0; g < G; ++g) t += part[(s * G + g) * a.D + d];
  a.mean[i] = n > 0 ? t / (double)n : 0.0;
}

// dst [G][S][D][D] (the row splits' partial sums in the workspace) or, G = 1, the output [S][D][D]
template <bool VEC>
__global__ void __launch_bounds__(256) moments_scatter_kernel(const objnerf_moments_args a, double* __restrict__ dst) {
  const int s = blockIdx.y, G = gridDim.z, gz = blockIdx.z;
  const int D = a.D;
  int ti = 0, tj = 0;
  {
    const int T = (D + SC_T - 1) / SC_T;
    int p = blockIdx.x;
    while (p >= T - ti) { p -= T - ti; ++ti; }
    tj = ti + p;
  }
  const bool diag = ti == tj;
  const int64_t r0 = seg_at(a.seg_off, s, a.V), r1 = seg_at(a.seg_off, s + 1, a.V);
  const int64_t n = r1 > r0 ? r1 - r0 : 0, chunk = (n + G - 1) / G;
  const int64_t lo = r0 + gz * chunk, hi = r1 < lo + chunk ? r1 : lo + chunk;
  __shared__ float sa[SC_K][SC_PAD];
  __shared__ float sb[SC_K][SC_PAD];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wi = wv & 1, wj = wv >> 1;
  const int cc = 4 * (t & 15), rr = t >> 4;               // loader: 4 columns, rows rr and rr + 16
  const int ca = ti * SC_T + cc, cb = tj * SC_T + cc;
  float ma[4], mb[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ma[e] = ca + e < D ? (float)a.mean[(int64_t)s * D + ca + e] : 0.f;
    mb[e] = cb + e < D ? (float)a.mean[(int64_t)s * D + cb + e] : 0.f;
  }
  floatx4 acc[2][2];
  double acc64[2][2][4];
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      acc[bi][bj] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) acc64[bi][bj][e] = 0.0;
    }
  int stage = 0;
  for (int64_t kb = lo; kb < hi; kb += SC_K) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t row = kb + rr + 16 * h;
      const bool ok = row < hi;
      const float* p = a.feat + (ok ? row : r0) * a.row_stride;
      const float4 fa = load_row4<VEC>(p, ca, D, ok);       // zero past D and past the chunk: adds nothing
      float* da = sa[rr + 16 * h] + cc;
      da[0] = ok && ca < D ? fa.x - ma[0] : 0.f;
      da[1] = ok && ca + 1 < D ? fa.y - ma[1] : 0.f;
      da[2] = ok && ca + 2 < D ? fa.z - ma[2] : 0.f;
      da[3] = ok && ca + 3 < D ? fa.w - ma[3] : 0.f;
      if (!diag) {
        const float4 fb = load_row4<VEC>(p, cb, D, ok);
        float* db = sb[rr + 16 * h] + cc;
        db[0] = ok && cb < D ? fb.x - mb[0] : 0.f;
        db[1] = ok && cb + 1 < D ? fb.y - mb[1] : 0.f;
        db[2] = ok && cb + 2 < D ? fb.z - mb[2] : 0.f;
        db[3] = ok && cb + 3 < D ? fb.w - mb[3] : 0.f;
      }
    }
    __syncthreads();
    const float(*Bt)[SC_PAD] = diag ? sa : sb;
#pragma unroll
    for (int ks = 0; ks < SC_K / 4; ++ks) {               // A[i][k] = y[k][i], B[k][j] = y[k][j]: k = the row
      const int k = 4 * ks + (lane >> 4);
      const float a0 = sa[k][32 * wi + (lane & 15)], a1 = sa[k][32 * wi + 16 + (lane & 15)];
      const float b0 = Bt[k][32 * wj + (lane & 15)], b1 = Bt[k][32 * wj + 16 + (lane & 15)];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
    if (++stage == SC_FOLD) {
      stage = 0;
#pragma unroll
      for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc64[bi][bj][e] += (double)acc[bi][bj][e];
          acc[bi][bj] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
    }
  }
  double* o = dst + ((int64_t)gz * gridDim.y + s) * D * D;   // split gz's slice (gz = 0: the output itself)
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double v = acc64[bi][bj][e] + (double)acc[bi][bj][e];
        const int i = ti * SC_T + 32 * wi + 16 * bi + 4 * (lane >> 4) + e;   // C/D: row 4 (lane >> 4) + e
        const int j = tj * SC_T + 32 * wj + 16 * bj + (lane & 15);           //      column lane & 15
        if (i < D && j < D) {
          o[(int64_t)i * D + j] = v;
          if (!diag) o[(int64_t)j * D + i] = v;
        }
      }
}

__global__ void moments_scatter_sum_kernel(const int64_t n, const int G, const double* __restrict__ ws,
                                           double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double t = ws[i];
  for (int g = 1; g < G; ++g) t += ws[(int64_t)g * n + i];
  out[i] = t;
}

// ------------------------------------------------------------------------------------------------ colours
// matplotlib's "rainbow" (_cm.py: red |2x - 0.5|, green sin(pi x), blue cos(pi x / 2)) at numpy.linspace(0, 1, 256)
// (i * (1 / 255), the last point exactly 1), clipped to [0, 1], in fp64, rounded to fp32
__host__ __device__ inline void rainbow_entry(const int i, float rgb[3]) {
  const double x = i == 255 ? 1.0 : (double)i * (1.0 / 255.0);
  const double r = fabs(2.0 * x - 0.5), g = sin(x * M_PI), b = cos(x * M_PI / 2.0);
  rgb[0] = (float)fmin(fmax(r, 0.0), 1.0);
  rgb[1] = (float)fmin(fmax(g, 0.0), 1.0);
  rgb[2] = (float)fmin(fmax(b, 0.0), 1.0);
}

// Colormap.__call__ for a float32 x: x * 256, 256 -> 255; x < 0 -> entry 0 (under), x * 256 >= 256 -> 255 (over),
// NaN -> the bad colour (0, 0, 0); else entry trunc(x * 256)
__device__ __forceinline__ int rainbow_index(const float x) {
  if (isnan(x)) return -1;
  float xs = x * 256.f;
  if (xs == 256.f) xs = 255.f;
  if (xs < 0.f) return 0;
  if (xs >= 256.f) return 255;
  return (int)xs;
}

__device__ __forceinline__ float norm01(const float v, const float lo, const float hi) {
  return __fdiv_rn(__fsub_rn(v, lo), __fsub_rn(hi, lo));   // (s - min) / (max - min), each step rounded, as torch
}

__global__ void __launch_bounds__(CL_WG) color_kernel(const objnerf_color_args a) {
  const int s = blockIdx.y;
  const int mode = a.mode[s];
  __shared__ float lut[256][3];
  if (mode == OBJNERF_COLOR_RAINBOW) {                    // uniform per workgroup
    rainbow_entry(threadIdx.x, lut[threadIdx.x]);
    __syncthreads();
  }
  const int64_t r0 = seg_at(a.seg_off, s, a.V), r1 = seg_at(a.seg_off, s + 1, a.V);
  const int Q = a.Q;
  float c0 = 0.f, c1 = 0.f, c2 = 0.f, lo = 0.f, hi = 0.f, sg[3] = {1.f, 1.f, 1.f};
  int col = 0;
  double fac = 0.0;
  if (mode == OBJNERF_COLOR_CONSTANT) {
    c0 = a.constant[3 * s]; c1 = a.constant[3 * s + 1]; c2 = a.constant[3 * s + 2];
  } else if (mode == OBJNERF_COLOR_RGB) {
    fac = a.factor[s];
  } else if (mode == OBJNERF_COLOR_RAINBOW) {
    col = a.column[s];
    lo = a.minmax[((int64_t)s * Q + col) * 2];
    hi = a.minmax[((int64_t)s * Q + col) * 2 + 1];
  } else if (mode == OBJNERF_COLOR_PCA) {                  // u-based sign: each column's largest |score| positive
    lo = INFINITY; hi = -INFINITY;
    for (int c = 0; c < 3; ++c) {
      const float cl = a.minmax[((int64_t)s * Q + c) * 2], ch = a.minmax[((int64_t)s * Q + c) * 2 + 1];
      sg[c] = -cl > ch ? -1.f : 1.f;
      lo = fminf(lo, sg[c] > 0.f ? cl : -ch);
      hi = fmaxf(hi, sg[c] > 0.f ? ch : -cl);
    }
  }
  for (int64_t row = r0 + (int64_t)blockIdx.x * CL_WG + threadIdx.x; row < r1; row += (int64_t)gridDim.x * CL_WG) {
    float o[3];
    if (mode == OBJNERF_COLOR_RGB) {
      const uint8_t* p = a.rgb + row * a.rgb_stride;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = (float)__dmul_rn(__ddiv_rn((double)p[c], 255.0), fac);
    } else if (mode == OBJNERF_COLOR_RAINBOW) {
      const int i = rainbow_index(norm01(a.proj[row * Q + col], lo, hi));
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = i < 0 ? 0.f : lut[i][c];
    } else if (mode == OBJNERF_COLOR_PCA) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float x = norm01(sg[c] * a.proj[row * Q + c], lo, hi);
        o[c] = x > 0.f ? (x < 1.f ? x : 1.f) : 0.f;       // clip(0, 1); NaN (a constant segment) -> 0
      }
    } else {
      o[0] = c0; o[1] = c1; o[2] = c2;
    }
    a.out[3 * row] = o[0];
    a.out[3 * row + 1] = o[1];
    a.out[3 * row + 2] = o[2];
  }
}

template <int NCH>
int launch_project(const objnerf_project_args* a, const dim3 grid, float* part, hipStream_t st) {
  const bool vec = a->D % 4 == 0 && a->row_stride % 4 == 0 && ((uintptr_t)a->feat & 15) == 0;
  if (vec)
    hipLaunchKernelGGL((project_kernel<NCH, true>), grid, dim3(PJ_WG), 0, st, *a, part);
  else
    hipLaunchKernelGGL((project_kernel<NCH, false>), grid, dim3(PJ_WG), 0, st, *a, part);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

}  // namespace

extern "C" {

size_t objnerf_project_workspace_bytes(int32_t S, int32_t Q, int64_t V) {
  if (S <= 0 || S > 65535 || Q <= 0 || Q > 16 || V < 0) return 0;
  return align256(sizeof(float) * 2 * (size_t)S * Q * pj_split(S, V));
}

int objnerf_project(const objnerf_project_args* a, void* ws, size_t ws_bytes, void* stream) {
  if (!a || !ws || !a->seg_off || !a->W || !a->out || !a->minmax) return OBJNERF_EINVAL;
  if (a->S <= 0 || a->S > 65535 || a->D < 1 || a->D > 1024 || a->Q < 1 || a->Q > 16 || a->V < 0 ||
      a->row_stride < a->D || (a->flags & ~(OBJNERF_PROJ_COSINE | OBJNERF_PROJ_PER_SEGMENT)))
    return OBJNERF_EINVAL;
  if (a->V > 0 && !a->feat) return OBJNERF_EINVAL;
  if (ws_bytes < objnerf_project_workspace_bytes(a->S, a->Q, a->V)) return OBJNERF_EINVAL;
  const int G = pj_split(a->S, a->V);
  const dim3 grid((unsigned)G, (unsigned)a->S);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  const int rc = a->D <= 128 ? launch_project<8>(a, grid, part, st)
               : a->D <= 512 ? launch_project<32>(a, grid, part, st) : launch_project<64>(a, grid, part, st);
  if (rc != OBJNERF_OK) return rc;
  const int64_t n = (int64_t)a->S * a->Q;
  hipLaunchKernelGGL(project_minmax_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, a->S, a->Q, G, part,
                     a->minmax);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

size_t objnerf_moments_workspace_bytes(int32_t S, int32_t D) {
  if (S <= 0 || S > 65535 || D < 1 || D > 1024) return 0;
  const int Gs = sc_split(S, D);
  return align256(sizeof(double) * (size_t)S * mm_split(S, D) * D) +
         (Gs > 1 ? align256(sizeof(double) * (size_t)Gs * S * D * D) : 0);
}

int objnerf_moments(const objnerf_moments_args* a, void* ws, size_t ws_bytes, void* stream) {
  if (!a || !ws || !a->seg_off || !a->mean || !a->scatter) return OBJNERF_EINVAL;
  if (a->S <= 0 || a->S > 65535 || a->D < 1 || a->D > 1024 || a->V < 0 || a->row_stride < a->D) return OBJNERF_EINVAL;
  if (a->V > 0 && !a->feat) return OBJNERF_EINVAL;
  if (ws_bytes < objnerf_moments_workspace_bytes(a->S, a->D)) return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int Gm = mm_split(a->S, a->D), Gs = sc_split(a->S, a->D);
  double* mpart = (double*)ws;
  double* spart = (double*)((char*)ws + align256(sizeof(double) * (size_t)a->S * Gm * a->D));
  hipLaunchKernelGGL(moments_mean_kernel, dim3((unsigned)cdiv(a->D, MM_WG), (unsigned)a->S, (unsigned)Gm), dim3(MM_WG),
                     0, st, *a, mpart);
  CHECK_LAUNCH();
  const int64_t nm = (int64_t)a->S * a->D;
  hipLaunchKernelGGL(moments_mean_finish_kernel, dim3((unsigned)cdiv(nm, 256)), dim3(256), 0, st, *a, Gm, mpart);
  CHECK_LAUNCH();
  const dim3 grid((unsigned)sc_pairs(a->D), (unsigned)a->S, (unsigned)Gs);
  double* dst = Gs > 1 ? spart : a->scatter;
  const bool vec = a->D % 4 == 0 && a->row_stride % 4 == 0 && ((uintptr_t)a->feat & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(moments_scatter_kernel<true>, grid, dim3(256), 0, st, *a, dst);
  else
    hipLaunchKernelGGL(moments_scatter_kernel<false>, grid, dim3(256), 0, st, *a, dst);
  CHECK_LAUNCH();
  if (Gs > 1) {
    const int64_t n = (int64_t)a->S * a->D * a->D;
    hipLaunchKernelGGL(moments_scatter_sum_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, n, Gs, spart,
                       a->scatter);
    CHECK_LAUNCH();
  }
  return OBJNERF_OK;
}

int objnerf_vertex_colors(const objnerf_color_args* a, void* stream) {
  if (!a || !a->seg_off || !a->mode || !a->out || a->S <= 0 || a->S > 65535 || a->V < 0 || a->Q < 0 || a->Q > 16)
    return OBJNERF_EINVAL;
  if (a->V == 0) return OBJNERF_OK;
  const int G = (int)clamp64(std::min<int64_t>(cdiv(4096, a->S), cdiv(a->V, (int64_t)a->S * CL_WG)), 1, 65535);
  hipLaunchKernelGGL(color_kernel, dim3((unsigned)G, (unsigned)a->S), dim3(CL_WG), 0, (hipStream_t)stream, *a);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_rainbow_lut(float* out) {
  if (!out) return OBJNERF_EINVAL;
  for (int i = 0; i < 256; ++i) rainbow_entry(i, out + 3 * i);
  return 256;
}

}  // extern "C"
