// Labelling arbitrary 3-D points against the whole map (gfx950): which object does each point belong to, and what are its
// colour and part feature?  The 3-D counterpart of the z-buffer merge of train.py:550-612, over Trainer.eval_points
// (trainer.py:105-128) restricted to each object's fitted box (the "bbox" of obj_<id>.pth, vmap.py:556-576).
//
//   objnerf_mappoints_count / _emit   the candidate CSR of objnerf_segments.h under the test InBox: point n is a candidate
//       of object k iff |R_k^T (p_n - c_k)| <= extent_k / 2, component-wise, fp32.  pair_pt [M] is object-major and
//       ascending in the point index inside an object.
//   mp_eval_kernel      the ragged fused evaluation of the hidden-32 objects (seg_walk, objnerf_segments.h): a lane
//       gathers its point through pair_pt and runs the chain of objnerf_mlp32.h.
//   gather_kernel / merge_kernel   around objnerf_eval_points_ws for a wider network (the hidden-128 background): its
//       segment of pair_pt is contiguous, so it is gathered, evaluated rectangularly and merged with the same keys.
//   resolve_kernel      best [N] -> obj, alpha, the winning pair, the winner's colour.
//   win_count_kernel / wg_scan_kernel / win_emit_kernel / head_kernel   the 512-d feature of the winners only.
//
// THE WINNER IS A MAXIMUM.  Every candidate pair m of point n offers one 64-bit key to atomicMax(best[n]):
//   bit 63        the object is a foreground object and alpha > 0 (an occupied foreground candidate hides the background
//                 whatever the background's alpha is: train.py:593-594);
//   bits 62..31   alpha's bits made order-preserving (negative: all bits flipped, else the sign bit set);
//   bits 30..0    0x7FFFFFFF - m: among equal alphas the lowest pair wins, and pairs are object-major, so that is the
//                 object that comes first in the caller's list.
// The maximum of a set does not depend on the order its elements arrive in and no two pairs share a key, so best [N] --
// and everything derived from it -- is the same bits on every run, whatever the order of the atomics.  Key 0 is never
// offered (m <= 2^31 - 2 leaves the low field >= 1): a point that keeps 0 has no candidate.
//
// The arithmetic on a pair does not depend on where the pair sits: a sample is one column of the MFMA B operand and
// every column goes through the same instructions (as in eval_kernel), the head sums h in one fixed order per row.
#include "objnerf_segments.h"

using namespace obj32;

namespace {

// box record: c [3] | R [3][3] row-major | extent / 2 [3] | obj_center
struct Box {
  float c[3], R[9], h[3];
};
// (the whole record at once, through a restrict pointer: the test's scalar loads then come in two rounds, not three)
__device__ __forceinline__ Box load_box(const float* __restrict__ boxes, const int k) {
  Box b;
  const float* p = boxes + (int64_t)k * SEG_BOX_FLOATS;
#pragma unroll
  for (int i = 0; i < 3; ++i) b.c[i] = p[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) b.R[i] = p[3 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) b.h[i] = p[12 + i];
  return b;
}
struct InBox {
  const float* pts; const float* boxes; int32_t* pair_pt;
  struct Payload {};
  // |R^T (p - c)| <= extent / 2 in every component
  __device__ __forceinline__ bool hit(const int k, const int64_t n, Payload&) const {
    const Box b = load_box(boxes, k);
    const float dx = pts[3 * n] - b.c[0], dy = pts[3 * n + 1] - b.c[1], dz = pts[3 * n + 2] - b.c[2];
    bool in = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float l = fmaf(dz, b.R[6 + j], fmaf(dy, b.R[3 + j], dx * b.R[j]));
      in = in && fabsf(l) <= b.h[j];
    }
    return in;
  }
  __device__ __forceinline__ void store(const int64_t pos, const int64_t n, const Payload&) const { pair_pt[pos] = (int32_t)n; }
};

// ------------------------------------------------------------------------------------------------------------ keys
__device__ __forceinline__ unsigned long long make_key(const float alpha, const bool fg, const int64_t m) {
  const unsigned u = __float_as_uint(alpha);
  const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  const unsigned long long top = (fg && alpha > 0.0f) ? 1ull : 0ull;
  return (top << 63) | ((unsigned long long)ord << 31) | (SEG_PAIR_LOW - (unsigned long long)m);
}
__device__ __forceinline__ float key_alpha(const unsigned long long key) {
  const unsigned ord = (unsigned)(key >> 31);
  return __uint_as_float((ord & 0x80000000u) ? (ord & 0x7FFFFFFFu) : ~ord);
}
__device__ __forceinline__ int64_t key_pair(const unsigned long long key) { return (int64_t)(SEG_PAIR_LOW - (key & SEG_PAIR_LOW)); }
// the pair that labels its point, or -1: the maximum, when it is occupied
__device__ __forceinline__ int64_t key_winner(const unsigned long long key) {
  return (key != 0ull && key_alpha(key) > 0.0f) ? key_pair(key) : -1;
}

// ------------------------------------------------------------------------------------------- the ragged evaluation
struct MpEval : SegWalkArgs {          // info's flag: the object is a background
  float* pair_alpha; float* pair_color; float* pair_hfeat;
  unsigned long long* best;
};
template <bool FEAT>
__global__ __launch_bounds__(256) void mp_eval_kernel(const MpEval a) {
  using namespace obj32n;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const float* sv = lds + sv_base(FEAT);
  const float* wf = (const float*)__builtin_assume_aligned(lds + 4 * g * WROW + out_pos(c), 8);
  seg_walk<FEAT>(a, lds, [&](const int64_t m, const bool valid, const int64_t n, const float scale, const float oc, const int bg) {
    const float* p = a.pts + n * 3;
    Pe32 pe;
    pe32_project(sv, g, p[0] - oc, p[1] - oc, p[2] - oc, scale, pe);
    Emb32 e;
    embed32(e, pe, g);
    Acts act;
    const float hout = mlp32_forward<FEAT>(wf, sv, g, e, act);    // group 0: 10 * raw alpha, groups 1..3: colour g - 1
    if (valid) {
      if (g == 0) {
        a.pair_alpha[m] = hout;
        atomicMax(a.best + n, make_key(hout, bg == 0, m));
      } else if (a.pair_color) {
        a.pair_color[m * 3 + g - 1] = hout;
      }
      if (FEAT) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          float4 v = make_float4(act.hf.t[tt][0], act.hf.t[tt][1], act.hf.t[tt][2], act.hf.t[tt][3]);
          *reinterpret_cast<float4*>(a.pair_hfeat + m * H + 16 * tt + 4 * g) = v;
        }
      }
    }
  });
}

// ------------------------------------------------------------------------------------- a wide object's segment
__global__ void __launch_bounds__(256) gather_kernel(const int64_t n, const int32_t* __restrict__ pair_pt,
                                                     const float* __restrict__ pts, const float oc, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* p = pts + (int64_t)pair_pt[i] * 3;
  out[3 * i] = p[0] - oc; out[3 * i + 1] = p[1] - oc; out[3 * i + 2] = p[2] - oc;
}
__global__ void __launch_bounds__(256) merge_kernel(const int64_t n, const int64_t pair0, const int32_t* __restrict__ pair_pt,
                                                    const float* __restrict__ alpha, const int fg,
                                                    unsigned long long* __restrict__ best) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  atomicMax(best + pair_pt[pair0 + i], make_key(alpha[pair0 + i], fg != 0, pair0 + i));
}

// ---------------------------------------------------------------------------------------------------------- resolve
__global__ void __launch_bounds__(256) resolve_kernel(const int64_t N, const int K, const unsigned long long* __restrict__ best,
                                                      const int64_t* __restrict__ seg_off, const float* __restrict__ pair_color,
                                                      int32_t* __restrict__ out_obj, float* __restrict__ out_alpha,
                                                      int32_t* __restrict__ out_pair, float* __restrict__ out_color) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const unsigned long long key = best[n];
  const int64_t m = key_winner(key);
  out_alpha[n] = key != 0ull ? key_alpha(key) : -INFINITY;
  out_obj[n] = m >= 0 ? seg_of(seg_off, K, m) : -1;
  if (out_pair) out_pair[n] = (int32_t)m;
  if (out_color) {
#pragma unroll
    for (int j = 0; j < 3; ++j) out_color[3 * n + j] = m >= 0 ? pair_color[3 * m + j] : 0.0f;
  }
}

// ------------------------------------------------------------------------------------- the feature of the winners
__device__ __forceinline__ bool pair_wins(const int64_t m, const int64_t M, const int32_t* __restrict__ pair_pt,
                                          const unsigned long long* __restrict__ best) {
  return m < M && key_winner(best[pair_pt[m]]) == m;
}
__global__ void __launch_bounds__(SEG_WG) win_count_kernel(const int64_t M, const int32_t* __restrict__ pair_pt,
                                                          const unsigned long long* __restrict__ best,
                                                          int64_t* __restrict__ cnt) {
  const bool win = pair_wins((int64_t)blockIdx.x * SEG_WG + threadIdx.x, M, pair_pt, best);
  __shared__ int wcnt[SEG_WG / 64];
  int total;
  wg_exclusive_flag<SEG_WG>(win, wcnt, total);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}
// win [3][max_win]: the winning pairs in pair order (object-major), their points, their objects
__global__ void __launch_bounds__(SEG_WG) win_emit_kernel(const int64_t M, const int K, const int32_t* __restrict__ pair_pt,
                                                         const unsigned long long* __restrict__ best,
                                                         const int64_t* __restrict__ seg_off, const int64_t* __restrict__ cnt,
                                                         const int64_t max_win, int32_t* __restrict__ win) {
  const int64_t m = (int64_t)blockIdx.x * SEG_WG + threadIdx.x;
  const bool wins = pair_wins(m, M, pair_pt, best);
  __shared__ int wcnt[SEG_WG / 64];
  int total;
  const int64_t pos = cnt[blockIdx.x] + wg_exclusive_flag<SEG_WG>(wins, wcnt, total);
  if (wins && pos >= 0 && pos < max_win) {
    win[pos] = (int32_t)m;
    win[max_win + pos] = pair_pt[m];
    win[2 * max_win + pos] = seg_of(seg_off, K, m);
  }
}

// out_feat [point] = of_w . hfeat [winning pair] + of_b (model.py:101; the head is linear), LDS-staged VALU.
// A workgroup takes a contiguous share of the 32-winner tiles.  Per tile, 32 threads fetch their winner's pair, point and
// object (win_emit_kernel left them side by side: one round of loads); the tile is cut into runs of one object (mostly
// one).  A thread owns NC output columns of a block of 256 NC columns (hidden 32: NC = 2, the whole 512-wide row in one pass; 64 / 128: NC = 1) and keeps their weight
// rows, NC x H floats, in registers for as long as the object stays the same; the winners' hidden rows are read from LDS
// as broadcasts.  The column block is the OUTER loop over the whole share, so a wide object's weights are fetched once
// per workgroup and pass, not once per tile.  The sum over h runs h = 0 .. H - 1 in one fma chain per (winner, column),
// whatever the tile.  A row of out_feat leaves as 1 KB wave stores.  Other widths (multiples of 32) take the same route in
// 32-input chunks without the register cache.  One launch per width present (the caller names them): a launch walks
// every tile and serves the runs of its width, so each instantiation keeps only its own weights in registers.
constexpr int HD_TW = 32;             // winners per tile
constexpr int HD_HMAX = 128;          // the widest hidden row the register cache holds
struct HeadTile {
  int64_t pair[HD_TW], pt[HD_TW];
  int k[HD_TW];
};
struct HeadCache {
  int k, cb;
};
template <int HW>
__device__ __forceinline__ void head_run(const objnerf_mappoints_head_obj& hd, const int k, const int cb, const int C,
                                         const HeadTile& tl, const int r0, const int nr, float (*xs)[HD_HMAX],
                                         float (&w)[HW == 32 ? 64 : HW], HeadCache& have, float* __restrict__ out_feat) {
  constexpr int NC = HW == 32 ? 2 : 1;
  const int tid = threadIdx.x;
  __syncthreads();                                      // the run before has read xs
  for (int e = tid; e < nr * HW; e += 256) {
    const int r = e / HW, h = e % HW;
    xs[r][h] = hd.hfeat[(tl.pair[r0 + r] - hd.row0) * HW + h];
  }
  int c[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) c[j] = cb + 256 * j + tid;
  if (have.k != k || have.cb != cb) {
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int h = 0; h < HW; h += 4) {
        const float4 v = *reinterpret_cast<const float4*>(hd.of_w + (int64_t)(c[j] < C ? c[j] : C - 1) * HW + h);   // (a column past C is never stored)
        w[j * HW + h] = v.x; w[j * HW + h + 1] = v.y; w[j * HW + h + 2] = v.z; w[j * HW + h + 3] = v.w;
      }
    have.k = k; have.cb = cb;
  }
  float bias[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) bias[j] = c[j] < C ? hd.of_b[c[j]] : 0.f;
  __syncthreads();
#pragma unroll 1
  for (int r = 0; r < nr; ++r) {
    float acc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = bias[j];
#pragma unroll
    for (int h = 0; h < HW; h += 4) {
      const float4 x = *reinterpret_cast<const float4*>(&xs[r][h]);
#pragma unroll
      for (int j = 0; j < NC; ++j)
        acc[j] = fmaf(w[j * HW + h + 3], x.w, fmaf(w[j * HW + h + 2], x.z, fmaf(w[j * HW + h + 1], x.y, fmaf(w[j * HW + h], x.x, acc[j]))));
      if ((h & 15) == 12) __builtin_amdgcn_sched_barrier(0);      // at most four rows of x in flight: the registers hold w
    }
    float* o = out_feat + tl.pt[r0 + r] * C;
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (c[j] < C) o[c[j]] = acc[j];
  }
}
// any multiple of 32: the same sums, the weights read again for every run
__device__ __forceinline__ void head_run_any(const objnerf_mappoints_head_obj& hd, const int cb, const int C, const HeadTile& tl,
                                             const int r0, const int nr, float (*xs)[HD_HMAX], float* __restrict__ out_feat) {
  const int tid = threadIdx.x, c = cb + tid;
  float acc[HD_TW];
  const float b = c < C ? hd.of_b[c] : 0.f;
#pragma unroll
  for (int r = 0; r < HD_TW; ++r) acc[r] = b;
  for (int h0 = 0; h0 < hd.H; h0 += 32) {
    __syncthreads();
    for (int e = tid; e < nr * 32; e += 256) xs[e >> 5][e & 31] = hd.hfeat[(tl.pair[r0 + (e >> 5)] - hd.row0) * hd.H + h0 + (e & 31)];
    float wv[32];
#pragma unroll
    for (int h = 0; h < 32; ++h) wv[h] = c < C ? hd.of_w[(int64_t)c * hd.H + h0 + h] : 0.f;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < HD_TW; ++r)
      if (r < nr) {
#pragma unroll
        for (int h = 0; h < 32; ++h) acc[r] = fmaf(wv[h], xs[r][h], acc[r]);
      }
  }
#pragma unroll
  for (int r = 0; r < HD_TW; ++r)
    if (r < nr && c < C) out_feat[tl.pt[r0 + r] * C + c] = acc[r];
}
template <int HW>            // the objects of hidden width HW (32 / 64 / 128: register cache); 0: every other width
__global__ void __launch_bounds__(256, HW == 128 ? 1 : 2) head_kernel(const int K, const int C, const int64_t* __restrict__ n_win,
                                                   const int32_t* __restrict__ win, const int64_t max_win,
                                                   const objnerf_mappoints_head_obj* __restrict__ heads, float* __restrict__ out_feat) {
  __shared__ __attribute__((aligned(16))) float xs[HD_TW][HD_HMAX];
  __shared__ HeadTile tl;
  const int tid = threadIdx.x;
  const int64_t W = *n_win;
  const int64_t T = (W + HD_TW - 1) / HD_TW;
  const int64_t t0 = T * (int64_t)blockIdx.x / (int64_t)gridDim.x, t1 = T * ((int64_t)blockIdx.x + 1) / (int64_t)gridDim.x;
  float w[HW ? (HW == 32 ? 64 : HW) : 1];
  HeadCache have = {-1, -1};
  for (int pass = 0; pass * 256 * (HW == 32 ? 2 : 1) < C; ++pass) {      // column blocks of 256 NC columns, outermost
    for (int64_t t = t0; t < t1; ++t) {
      const int64_t wbeg = t * HD_TW;
      const int nw = (int)(wbeg + HD_TW < W ? HD_TW : W - wbeg);
      __syncthreads();                                  // the tile before is done with tl
      if (tid < nw) {
        tl.pair[tid] = win[wbeg + tid];
        tl.pt[tid] = win[max_win + wbeg + tid];
        tl.k[tid] = win[2 * max_win + wbeg + tid];
      }
      __syncthreads();
      int r0 = 0;
      while (r0 < nw) {                                 // the runs of one object inside the tile (uniform)
        const int k = tl.k[r0];
        int r1 = r0 + 1;
        while (r1 < nw && tl.k[r1] == k) ++r1;
        const objnerf_mappoints_head_obj hd = heads[k];
        const int cb = pass * 256 * (HW == 32 ? 2 : 1);
        if (cb < C) {
          if constexpr (HW == 0) {
            if (hd.H != 32 && hd.H != 64 && hd.H != 128) head_run_any(hd, cb, C, tl, r0, r1 - r0, xs, out_feat);
          } else {
            if (hd.H == HW) head_run<HW>(hd, k, cb, C, tl, r0, r1 - r0, xs, w, have, out_feat);
          }
        }
        r0 = r1;
      }
    }
  }
}


}  // namespace

extern "C" {

size_t objnerf_mappoints_workspace_bytes(int64_t N, int32_t K) { return seg_csr_workspace_bytes(N, K); }

int objnerf_mappoints_count(int64_t N, int32_t K, const float* pts, const float* boxes, void* ws, size_t ws_bytes,
                            int64_t* seg_off, void* stream) {
  (void)hipGetLastError();
  if (!seg_sizes_ok(N, K) || !pts || !boxes || !ws || !seg_off) return OBJNERF_EINVAL;
  if (ws_bytes < seg_csr_workspace_bytes(N, K)) return OBJNERF_EINVAL;
  return seg_csr_count(N, K, InBox{pts, boxes, nullptr}, 1, ws, seg_off, (hipStream_t)stream);
}

int objnerf_mappoints_emit(int64_t N, int32_t K, const float* pts, const float* boxes, const void* ws, size_t ws_bytes,
                           int64_t M, int32_t* pair_pt, void* stream) {
  (void)hipGetLastError();
  if (!seg_sizes_ok(N, K) || !pts || !boxes || !ws || M < 0 || M > 0x7fffffffLL) return OBJNERF_EINVAL;
  if (ws_bytes < seg_csr_workspace_bytes(N, K)) return OBJNERF_EINVAL;
  if (M == 0) return OBJNERF_OK;
  if (!pair_pt) return OBJNERF_EINVAL;
  return seg_csr_emit(N, K, InBox{pts, boxes, pair_pt}, ws, M, (hipStream_t)stream);
}

int objnerf_mappoints_eval(const objnerf_net* net, int32_t K, int64_t N, int64_t M, const float* params, int64_t p_stride,
                           const float* scale, const float* pts, const float* boxes, const int32_t* info,
                           const int64_t* seg_off, const int32_t* pair_pt, float* pair_alpha, float* pair_color,
                           float* pair_hfeat, uint64_t* best, void* stream) {
  (void)hipGetLastError();
  if (!best) return OBJNERF_EINVAL;
  MpEval d;
  const int rc = seg_walk_args(d, net, K, N, M, params, p_stride, scale, pts, boxes, info, seg_off, pair_pt);
  if (rc != OBJNERF_OK || M == 0) return rc;
  if (!pair_alpha) return OBJNERF_EINVAL;
  d.pair_alpha = pair_alpha; d.pair_color = pair_color; d.pair_hfeat = pair_hfeat;
  d.best = (unsigned long long*)best;
  const bool feat = pair_hfeat != nullptr;
  const size_t lds_bytes = (size_t)obj32n::img_floats(feat) * 4;
  objnerf_once_per_device([] {                          // the image with the feature layer exceeds the 64 KB default
    (void)hipFuncSetAttribute((const void*)mp_eval_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              obj32n::img_floats(true) * 4);
  });
  const dim3 grid = seg_walk_grid(M, K), blk(256);
  if (feat) hipLaunchKernelGGL((mp_eval_kernel<true>), grid, blk, lds_bytes, (hipStream_t)stream, d);
  else hipLaunchKernelGGL((mp_eval_kernel<false>), grid, blk, lds_bytes, (hipStream_t)stream, d);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_mappoints_gather(int64_t n, const int32_t* pair_pt, const float* pts, float obj_center, float* out, void* stream) {
  (void)hipGetLastError();
  if (n < 0 || n > 0x7fffffff) return OBJNERF_EINVAL;
  if (n == 0) return OBJNERF_OK;
  if (!pair_pt || !pts || !out) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, n, pair_pt, pts,
                     obj_center, out);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_mappoints_merge(int64_t n, int64_t pair0, const int32_t* pair_pt, const float* pair_alpha, int32_t background,
                            uint64_t* best, void* stream) {
  (void)hipGetLastError();
  if (n < 0 || pair0 < 0 || pair0 + n > 0x7fffffffLL) return OBJNERF_EINVAL;
  if (n == 0) return OBJNERF_OK;
  if (!pair_pt || !pair_alpha || !best) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, n, pair0, pair_pt,
                     pair_alpha, background ? 0 : 1, (unsigned long long*)best);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_mappoints_resolve(int64_t N, int32_t K, int64_t M, const uint64_t* best, const int64_t* seg_off,
                              const float* pair_color, int32_t* out_obj, float* out_alpha, int32_t* out_pair,
                              float* out_color, void* stream) {
  (void)hipGetLastError();
  if (!seg_sizes_ok(N, K) || M < 0 || M > 0x7fffffffLL || !best || !seg_off || !out_obj || !out_alpha) return OBJNERF_EINVAL;
  // (without a pair nothing can win: every colour is 0 and pair_color, an empty buffer, is never read)
  if (out_color && !pair_color && M > 0) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, N, (int)K,
                     (const unsigned long long*)best, seg_off, pair_color, out_obj, out_alpha, out_pair, out_color);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

size_t objnerf_mappoints_head_workspace_bytes(int64_t M) {
  if (M <= 0 || M > 0x7fffffffLL) return 0;
  return align256(((size_t)seg_blocks(M) + 1) * sizeof(int64_t));
}

int objnerf_mappoints_head(int32_t K, int32_t C, int64_t N, int64_t M, const uint64_t* best, const int64_t* seg_off,
                           const int32_t* pair_pt, const objnerf_mappoints_head_obj* heads, int32_t widths, void* ws,
                           size_t ws_bytes, int32_t* win_pair, float* out_feat, void* stream) {
  (void)hipGetLastError();
  if (!seg_sizes_ok(N, K) || C <= 0 || M < 0 || M > 0x7fffffffLL || !best || !seg_off || !heads) return OBJNERF_EINVAL;
  if (M == 0) return OBJNERF_OK;
  if (!pair_pt || !ws || !win_pair || !out_feat || ws_bytes < objnerf_mappoints_head_workspace_bytes(M)) return OBJNERF_EINVAL;
  const int64_t nb = seg_blocks(M);
  int64_t* cnt = (int64_t*)ws;
  hipStream_t st = (hipStream_t)stream;
  const unsigned long long* b = (const unsigned long long*)best;
  hipLaunchKernelGGL(win_count_kernel, dim3((unsigned)nb), dim3(SEG_WG), 0, st, M, pair_pt, b, cnt);
  CHECK_LAUNCH();
  hipLaunchKernelGGL((wg_scan_kernel<SEG_SCAN_WG, 1, int64_t>), dim3(1), dim3(SEG_SCAN_WG), 0, st, cnt, nb, cnt + nb);
  CHECK_LAUNCH();
  const int64_t max_win = N < M ? N : M;                // a point has one winner at the most: win_pair holds 3 x min(N, M)
  hipLaunchKernelGGL(win_emit_kernel, dim3((unsigned)nb), dim3(SEG_WG), 0, st, M, (int)K, pair_pt, b, seg_off, cnt, max_win,
                     win_pair);
  CHECK_LAUNCH();
  int64_t G = 8 * (int64_t)objnerf_num_cu();
  const int64_t t_max = cdiv(max_win, HD_TW);
  if (G > t_max) G = t_max;
  const int64_t* n_win = cnt + nb;
#define MP_HEAD_LAUNCH(HW)                                                                                              \
  do {                                                                                                                  \
    hipLaunchKernelGGL((head_kernel<HW>), dim3((unsigned)G), dim3(256), 0, st, (int)K, (int)C, n_win, win_pair, max_win, \
                       heads, out_feat);                                                                                 \
    CHECK_LAUNCH();                                                                                                     \
  } while (0)
  if (widths & OBJNERF_MAPPOINTS_W32) MP_HEAD_LAUNCH(32);
  if (widths & OBJNERF_MAPPOINTS_W64) MP_HEAD_LAUNCH(64);
  if (widths & OBJNERF_MAPPOINTS_W128) MP_HEAD_LAUNCH(128);
  if (widths & OBJNERF_MAPPOINTS_WOTHER) MP_HEAD_LAUNCH(0);
#undef MP_HEAD_LAUNCH
  return OBJNERF_OK;
}

}  // extern "C"
