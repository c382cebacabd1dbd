// Field gradients of the finished map (gfx950): d alpha / d p for every (point, object) candidate pair, the object whose
// surface is nearest to a point, and the normal equations of a rigid alignment of a cloud to the map.
// The reference has no counterpart: it never differentiates a network in position.
//
//   mp_grad_kernel        over the candidate pairs of the hidden-32 objects (seg_walk, objnerf_segments.h), without the
//       feature layer in the image.  Per tile the density trunk runs
//       forward (mlp32_forward_density), the four ReLU masks are kept as 32 bits per lane, and the chain runs backwards
//       through the transposed operand reads (mma_t32 / mma_t16): seed 10 w_alpha masked by h4 > 0, mid2^T, cat^T (d h2
//       and the cat layer's d x1), mid1^T, in^T (added to d x1); pe32_x1_tile_fb leaves the projection gradient d p_j in
//       the lane that owns direction j; d t = sum_j d p_j B_j plus the three direct x / scale entries, the four lane
//       groups of a sample summed in one fixed order (xgroup_sum), divided by the scale.  Octaves 4 and 5 feed colour
//       only.  288 MFMAs a tile (144 forward, 144 backward) against 184 of mp_eval_kernel without the feature layer.
//       A sample is one column of every MFMA B operand: its arithmetic does not depend on its tile, its place in the
//       tile or the segment length.
//   embed_bwd_pts_kernel  d pts of UniDirsEmbed.forward (embedding.py:46-55) from d emb: all six octaves and the three
//       linear entries, one thread per point, no atomics.
//   select_kernel         d = alpha / max(|grad|, g_min) per pair, one 64-bit atomicMin per pair into best [N]:
//       bits 62..31 = the bits of |d| (order-preserving for a non-negative float), bits 30..0 = the pair.  A minimum does
//       not depend on arrival order and no two pairs share a key.
//   resolve_kernel        best [N] -> object, d, alpha, grad of the selected pair.
//   transform_kernel      q = float32(T p) with T in fp64: the cloud in the map's frame under the current pose.
//   accumulate_kernel / reduce_kernel   J = [(q - pivot) x n, n], n = grad / max(|grad|, g_min), in fp64: the 21 upper
//       entries of J J^T, the 6 of J d, sum d^2 and the inlier count.  A workgroup owns 1024 consecutive points whatever
//       the device; its partial sums go to the caller's workspace and one workgroup adds them in an order fixed by N.
#include "objnerf_segments.h"

using namespace obj32;

namespace {

constexpr int MA_SUMS = 29;           // 21 + 6 + 1 + 1
constexpr int MA_WG = 256;
constexpr int MA_PER = 4;             // points per thread of accumulate_kernel

struct MaGrad : SegWalkArgs {
  float* pair_alpha; float* pair_grad;
};
// the ReLU branch bits of one layer: bit 4 tt + r of the byte <-> feature 16 tt + 4 g + r
__device__ __forceinline__ unsigned relu_bits(const T32& h) {
  unsigned b = 0;
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int r = 0; r < 4; ++r) b |= (h.t[tt][r] > 0.0f ? 1u : 0u) << (4 * tt + r);
  return b;
}
__device__ __forceinline__ T32 mask_bits(const T32& d, const unsigned bits) {
  T32 o;
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int r = 0; r < 4; ++r) o.t[tt][r] = ((bits >> (4 * tt + r)) & 1u) ? d.t[tt][r] : 0.0f;
  return o;
}

__global__ __launch_bounds__(256) void mp_grad_kernel(const MaGrad a) {
  using namespace obj32n;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const float* sv = lds + sv_base(false);
  const float* wf = (const float*)__builtin_assume_aligned(lds + 4 * g * WROW + out_pos(c), 8);
  const float* wt0 = (const float*)__builtin_assume_aligned(lds + c * WROW + 8 * g + 4 * (g & 1), 16);
  const float* wt1 = (const float*)__builtin_assume_aligned(lds + c * WROW + 8 * g + 4 * (1 - (g & 1)), 16);
  seg_walk<false>(a, lds, [&](const int64_t m, const bool valid, const int64_t n, const float scale, const float oc, int) {
    const float* p = a.pts + n * 3;
    Pe32 pe;
    pe32_project(sv, g, p[0] - oc, p[1] - oc, p[2] - oc, scale, pe);
    unsigned bits;
    float alpha;
    {
      Emb32 e;
      embed32_x1(e, pe, g);
      Acts act;
      alpha = mlp32_forward_density(wf, sv, g, e, act);        // group 0: 10 * raw alpha
      bits = relu_bits(act.h1) | (relu_bits(act.h2) << 8) | (relu_bits(act.h3) << 16) | (relu_bits(act.h4) << 24);
    }
    // d alpha / d h4 = 10 w_alpha (model.py:88), then the trunk backwards
    T32 d_h4;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        d_h4.t[tt][r] = ((bits >> (24 + 4 * tt + r)) & 1u) ? sv[SV_WA + 16 * tt + 4 * g + r] * 10.0f : 0.0f;
    T32 d_h3 = zero32();
    mma_t32(d_h3, wt0, wt1, R_M2, d_h4);
    d_h3 = mask_bits(d_h3, bits >> 16);
    T32 d_h2 = zero32();
    mma_t32(d_h2, wt0, wt1, R_CAT, d_h3);
    d_h2 = mask_bits(d_h2, bits >> 8);
    T32 d_h1 = zero32();
    mma_t32(d_h1, wt0, wt1, R_M1, d_h2);
    d_h1 = mask_bits(d_h1, bits);
    // d x1 tile = cat^T d_h3 + in^T d_h1; a tile is one direction slot with its octaves 0..3
    float dps[6];
    float dlin = 0.0f;               // group g = 1..3: the gradient of the direct entry (x / scale)[g - 1]
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      dps[i] = 0.0f;
      f32x4 d_x = zero4();
      mma_t16(d_x, wt0, wt1, R_CAT + 32 + 16 * i, d_h3);
      mma_t16(d_x, wt0, wt1, R_IN + 16 * i, d_h1);
      (void)pe32_x1_tile_fb(pe, i, g, d_x, dps[i]);
      if (i == 5) dlin = (g == 0) ? 0.0f : d_x[0];
    }
    // d t = sum_j d p_j B_j (embedding.py:48) over this lane's directions j = 4 i + g, plus the direct entry
    const float* bl = sv + SV_PEB + 3 * g;
    float gt[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      float v = 0.0f;
#pragma unroll
      for (int i = 0; i < 6; ++i) v = fmaf(dps[i], bl[12 * i + x], v);
      v += (g == x + 1) ? dlin : 0.0f;
      gt[x] = xgroup_sum(v);         // (g0 + g1) + (g2 + g3) on every lane
    }
    if (valid) {
      if (g == 0) a.pair_alpha[m] = alpha;
      else a.pair_grad[m * 3 + g - 1] = ((g == 1) ? gt[0] : ((g == 2) ? gt[1] : gt[2])) / scale;      // embedding.py:47
    }
  });
}

// ------------------------------------------------------------------------------------------- embedding, d / d pts
// grid (blocks, K): d_pts [k][n][x] = (d_emb [x] + sum_j B [j][x] sum_f d_emb [3 + 21 f + j] cos(arg) pi 2^f) / scale
__global__ void __launch_bounds__(256) embed_bwd_pts_kernel(const int64_t N, const float* __restrict__ params, const long p_stride,
                                                            const int off_B, const float* __restrict__ scale,
                                                            const float* __restrict__ pts, const float* __restrict__ d_emb,
                                                            float* __restrict__ d_pts) {
  __shared__ float Bs[OBJ_NDIR * 3];
  const long z = blockIdx.y;
  if (threadIdx.x < OBJ_NDIR * 3) Bs[threadIdx.x] = params[z * p_stride + off_B + threadIdx.x];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float sc = scale[z];
  const float* p = pts + (z * N + i) * 3;
  const float* de = d_emb + (z * N + i) * OBJ_EMB;
  const float t0 = p[0] / sc, t1 = p[1] / sc, t2 = p[2] / sc;
  float g0 = de[0], g1 = de[1], g2 = de[2];
  for (int j = 0; j < OBJ_NDIR; ++j) {
    const float b0 = Bs[3 * j], b1 = Bs[3 * j + 1], b2 = Bs[3 * j + 2];
    const float pj = fmaf(t2, b2, fmaf(t1, b1, t0 * b0));
    float dp = 0.f;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
      const float sf = (float)(1 << f);
      float sn, cv;
      sincos_acc((pj * sf) * OBJ_PI_F, sn, cv);
      dp += de[3 + f * OBJ_NDIR + j] * ((cv * OBJ_PI_F) * sf);
    }
    g0 = fmaf(dp, b0, g0);
    g1 = fmaf(dp, b1, g1);
    g2 = fmaf(dp, b2, g2);
  }
  float* o = d_pts + (z * N + i) * 3;
  o[0] = g0 / sc; o[1] = g1 / sc; o[2] = g2 / sc;
}

// --------------------------------------------------------------------------------------------------------- select
__global__ void __launch_bounds__(256) select_kernel(const int64_t M, const int64_t N, const int32_t* __restrict__ pair_pt,
                                                     const float* __restrict__ pair_alpha, const float* __restrict__ pair_grad,
                                                     const float g_min, unsigned long long* __restrict__ best) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int64_t n = pair_pt[m];
  if (n < 0 || n >= N) return;
  const float gx = pair_grad[3 * m], gy = pair_grad[3 * m + 1], gz = pair_grad[3 * m + 2];
  const float gn = sqrtf((gx * gx + gy * gy) + gz * gz);
  const float d = fabsf(pair_alpha[m] / fmaxf(gn, g_min));
  atomicMin(best + n, ((unsigned long long)__float_as_uint(d) << 31) | (unsigned long long)m);
}
__global__ void __launch_bounds__(256) select_resolve_kernel(const int64_t N, const int K, const int64_t M,
                                                             const unsigned long long* __restrict__ best,
                                                             const int64_t* __restrict__ seg_off,
                                                             const float* __restrict__ pair_alpha,
                                                             const float* __restrict__ pair_grad, const float g_min,
                                                             int32_t* __restrict__ out_obj, int32_t* __restrict__ out_pair,
                                                             float* __restrict__ out_d, float* __restrict__ out_alpha,
                                                             float* __restrict__ out_grad) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const unsigned long long key = best[n];
  const int64_t m = (int64_t)(key & SEG_PAIR_LOW);
  const bool has = (key >> 63) == 0ull && m < M;        // the caller's fill (all ones) has bit 63 set
  float al = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, d = INFINITY;
  if (has) {
    al = pair_alpha[m];
    gx = pair_grad[3 * m]; gy = pair_grad[3 * m + 1]; gz = pair_grad[3 * m + 2];
    const float gn = sqrtf((gx * gx + gy * gy) + gz * gz);
    d = al / fmaxf(gn, g_min);
  }
  out_obj[n] = has ? seg_of(seg_off, K, m) : -1;
  if (out_pair) out_pair[n] = has ? (int32_t)m : -1;
  out_d[n] = d;
  out_alpha[n] = al;
  out_grad[3 * n] = gx; out_grad[3 * n + 1] = gy; out_grad[3 * n + 2] = gz;
}

// q = float32(R p + t), every operation in fp64 and rounded on its own, in one fixed order
struct Rigid {
  double m[12];                       // rows of [R | t]
};
__global__ void __launch_bounds__(256) transform_kernel(const int64_t N, const float* __restrict__ pts, const Rigid T,
                                                        float* __restrict__ out) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const double x = pts[3 * n], y = pts[3 * n + 1], z = pts[3 * n + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r) out[3 * n + r] = (float)(((T.m[4 * r] * x + T.m[4 * r + 1] * y) + T.m[4 * r + 2] * z) + T.m[4 * r + 3]);
}

// ----------------------------------------------------------------------------------------------------- accumulate
struct Piv {
  double c[3];
};
__device__ __forceinline__ double wave_sum_f64(double v) {   // the same sum on every lane: a + b is commutative
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}
// the workgroup's MA_SUMS totals from every thread's: lanes of a wave by a butterfly, then waves 0..3 in order
__device__ __forceinline__ void wg_sums_store(const double (&s)[MA_SUMS], double (*red)[MA_SUMS], double* __restrict__ dst) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < MA_SUMS; ++e) {
    const double v = wave_sum_f64(s[e]);
    if (lane == 0) red[wv][e] = v;
  }
  __syncthreads();
  if (threadIdx.x < MA_SUMS) dst[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}
// workgroup b owns points [b * 1024, (b + 1) * 1024); thread t the points b * 1024 + t + 256 u, u = 0..3, in that order
__global__ void __launch_bounds__(MA_WG) accumulate_kernel(const int64_t N, const float* __restrict__ pts,
                                                           const int32_t* __restrict__ obj, const float* __restrict__ alpha,
                                                           const float* __restrict__ grad, const Piv piv, const double tau,
                                                           const double g_min, double* __restrict__ part) {
  __shared__ double red[MA_WG / 64][MA_SUMS];
  double s[MA_SUMS];
#pragma unroll
  for (int e = 0; e < MA_SUMS; ++e) s[e] = 0.0;
#pragma unroll 1
  for (int u = 0; u < MA_PER; ++u) {
    const int64_t n = ((int64_t)blockIdx.x * MA_PER + u) * MA_WG + threadIdx.x;
    if (n >= N || obj[n] < 0) continue;
    const double gx = grad[3 * n], gy = grad[3 * n + 1], gz = grad[3 * n + 2];
    const double gn = sqrt((gx * gx + gy * gy) + gz * gz);
    const double den = gn > g_min ? gn : g_min;
    const double d = (double)alpha[n] / den;
    if (!(fabs(d) <= tau)) continue;
    const double nx = gx / den, ny = gy / den, nz = gz / den;
    const double rx = (double)pts[3 * n] - piv.c[0], ry = (double)pts[3 * n + 1] - piv.c[1], rz = (double)pts[3 * n + 2] - piv.c[2];
    const double J[6] = {ry * nz - rz * ny, rz * nx - rx * nz, rx * ny - ry * nx, nx, ny, nz};
    int e = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) { s[e] += J[i] * J[j]; ++e; }
#pragma unroll
    for (int i = 0; i < 6; ++i) s[21 + i] += J[i] * d;
    s[27] += d * d;
    s[28] += 1.0;
  }
  wg_sums_store(s, red, part + (int64_t)blockIdx.x * MA_SUMS);
}
// one workgroup: thread t adds the partials t, t + 256, ... in that order, then the same tree
__global__ void __launch_bounds__(MA_WG) accumulate_reduce_kernel(const int64_t nb, const double* __restrict__ part,
                                                                  double* __restrict__ out) {
  __shared__ double red[MA_WG / 64][MA_SUMS];
  double s[MA_SUMS];
#pragma unroll
  for (int e = 0; e < MA_SUMS; ++e) s[e] = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += MA_WG) {
#pragma unroll
    for (int e = 0; e < MA_SUMS; ++e) s[e] += part[b * MA_SUMS + e];
  }
  wg_sums_store(s, red, out);
}

int64_t ma_blocks(const int64_t N) { return cdiv(N, (int64_t)MA_WG * MA_PER); }

}  // namespace

extern "C" {

int objnerf_mappoints_grad(const objnerf_net* net, int32_t K, int64_t N, int64_t M, const float* params, int64_t p_stride,
                           const float* scale, const float* pts, const float* boxes, const int32_t* info,
                           const int64_t* seg_off, const int32_t* pair_pt, float* pair_alpha, float* pair_grad,
                           void* stream) {
  (void)hipGetLastError();
  MaGrad d;
  const int rc = seg_walk_args(d, net, K, N, M, params, p_stride, scale, pts, boxes, info, seg_off, pair_pt);
  if (rc != OBJNERF_OK || M == 0) return rc;
  if (!pair_alpha || !pair_grad) return OBJNERF_EINVAL;
  d.pair_alpha = pair_alpha; d.pair_grad = pair_grad;
  const size_t lds_bytes = (size_t)obj32n::img_floats(false) * 4;      // 60 KB: two workgroups a compute unit
  hipLaunchKernelGGL(mp_grad_kernel, seg_walk_grid(M, K), dim3(256), lds_bytes, (hipStream_t)stream, d);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_embed_bwd_pts(const objnerf_net* net, int32_t K, int64_t N, const float* params, int64_t p_stride,
                          const float* scale, const float* pts, const float* d_emb, float* d_pts, void* stream) {
  (void)hipGetLastError();
  if (!net || !params || !scale || !pts || !d_emb || !d_pts || K <= 0 || K > 65535 || N <= 0 || N > 0x7fffffff)
    return OBJNERF_EINVAL;
  if (net->n_freqs != 6) return OBJNERF_ENOTSUP;
  int64_t offs[OBJNERF_N_TENSORS + 1];
  if (objnerf_param_layout(net, offs) < 0) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(embed_bwd_pts_kernel, dim3((unsigned)cdiv(N, 256), (unsigned)K), dim3(256), 0, (hipStream_t)stream, N,
                     params, (long)p_stride, (int)offs[OBJNERF_T_PE_B], scale, pts, d_emb, d_pts);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_mapalign_select(int64_t N, int64_t M, const int32_t* pair_pt, const float* pair_alpha, const float* pair_grad,
                            float g_min, uint64_t* best, void* stream) {
  (void)hipGetLastError();
  if (N <= 0 || N > 0x7fffffff || M < 0 || M > 0x7fffffffLL || !best || !(g_min > 0.0f)) return OBJNERF_EINVAL;
  if (M == 0) return OBJNERF_OK;
  if (!pair_pt || !pair_alpha || !pair_grad) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(select_kernel, dim3((unsigned)cdiv(M, 256)), dim3(256), 0, (hipStream_t)stream, M, N, pair_pt, pair_alpha,
                     pair_grad, g_min, (unsigned long long*)best);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_mapalign_resolve(int64_t N, int32_t K, int64_t M, const uint64_t* best, const int64_t* seg_off,
                             const float* pair_alpha, const float* pair_grad, float g_min, int32_t* out_obj,
                             int32_t* out_pair, float* out_d, float* out_alpha, float* out_grad, void* stream) {
  (void)hipGetLastError();
  if (!seg_sizes_ok(N, K) || M < 0 || M > 0x7fffffffLL || !best || !seg_off || !out_obj || !out_d || !out_alpha || !out_grad ||
      !(g_min > 0.0f))
    return OBJNERF_EINVAL;
  if (M > 0 && (!pair_alpha || !pair_grad)) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(select_resolve_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, N, (int)K, M,
                     (const unsigned long long*)best, seg_off, pair_alpha, pair_grad, g_min, out_obj, out_pair, out_d,
                     out_alpha, out_grad);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_mapalign_transform(int64_t N, const float* pts, const double* t_rows, float* out, void* stream) {
  (void)hipGetLastError();
  if (N <= 0 || N > 0x7fffffff || !pts || !t_rows || !out) return OBJNERF_EINVAL;
  Rigid T;
  for (int i = 0; i < 12; ++i) T.m[i] = t_rows[i];
  hipLaunchKernelGGL(transform_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, N, pts, T, out);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

size_t objnerf_mapalign_workspace_bytes(int64_t N) {
  if (N <= 0 || N > 0x7fffffff) return 0;
  return align256((size_t)ma_blocks(N) * MA_SUMS * sizeof(double));
}

int objnerf_mapalign_accumulate(int64_t N, const float* pts, const int32_t* obj, const float* alpha, const float* grad,
                                const double* pivot, double tau, double g_min, void* ws, size_t ws_bytes, double* out,
                                void* stream) {
  (void)hipGetLastError();
  if (N <= 0 || N > 0x7fffffff || !pts || !obj || !alpha || !grad || !pivot || !ws || !out || !(g_min > 0.0) || !(tau >= 0.0))
    return OBJNERF_EINVAL;
  if (ws_bytes < objnerf_mapalign_workspace_bytes(N)) return OBJNERF_EINVAL;
  Piv pv;
  pv.c[0] = pivot[0]; pv.c[1] = pivot[1]; pv.c[2] = pivot[2];
  const int64_t nb = ma_blocks(N);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)nb), dim3(MA_WG), 0, st, N, pts, obj, alpha, grad, pv, tau, g_min,
                     (double*)ws);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(accumulate_reduce_kernel, dim3(1), dim3(MA_WG), 0, st, nb, (const double*)ws, out);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

}  // extern "C"
