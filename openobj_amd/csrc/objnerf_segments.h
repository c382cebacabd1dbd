// The segment CSR, written once: seg_off [K + 1] over K segments, entries segment-major and ascending inside a segment.
// For the map units the segments are the K objects of a map: objnerf_mappoints.hip
// (candidate points), objnerf_mapview.hip (candidate rays) and objnerf_mapalign.hip (field gradients over the candidate
// points).  objnerf_maskprep.hip uses the candidate CSR alone, with the frames of a batch as segments:
// the roots of the connected components in raster order.
//
//   seg_of                     the object of an entry.
//   seg_csr_count / _emit      THE CANDIDATE CSR: count / scan / emit over the primitives of objnerf_wg.h, templated on a
//       test object passed by value.  The test carries its pointers and exposes
//         bool hit(k, i, Payload&)         is item i a candidate of object k?  (may leave what it computed in the payload)
//         void store(pos, i, Payload)      entry pos of the CSR is item i
//       Grid (blocks of SEG_WG items, K); cnt [k][b] = the hits of object k in block b, scanned in place by one workgroup,
//       so the CSR is OBJECT-MAJOR; inside a block wg_exclusive_flag runs the prefix in thread order, so an object's
//       entries ASCEND in the item index; NO ATOMICS: the same inputs give the same lists.  min_keep: an object with
//       fewer hits keeps none (its counts are zeroed before the scan).  Emit bounds an entry by the end of its own
//       object's segment, so the hits of such an object go nowhere; without a drop the bound never bites.
//   seg_walk                   THE RAGGED WALK of the hidden-32 objects' segments by persistent workgroups: a flat list of
//       (object, 64-entry tile) cut into one contiguous share per workgroup; the LDS weight image is restaged
//       (stage_weights32) only where a share crosses into another object.
#pragma once
#include "objnerf_mlp32.h"
#include "objnerf_wg.h"

namespace {

// the segment of entry i: the largest s with off[s] <= i (off[0] = 0 <= i < off[S]; empty segments are stepped over)
__device__ __forceinline__ int seg_of(const int64_t* __restrict__ off, const int S, const int64_t i) {
  int lo = 0, hi = S;
  while (hi - lo > 1) {
    const int m = (lo + hi) >> 1;
    if (off[m] <= i) lo = m; else hi = m;
  }
  return lo;
}

constexpr int SEG_BOX_FLOATS = 16;    // floats per box record of an object; the units lay out [0, 15) as their test needs
constexpr unsigned long long SEG_PAIR_LOW = 0x7FFFFFFFull;      // the 31-bit pair field of the 64-bit keys
// items (points, pixels) in 31 bits; the objects are the y dimension of a grid
inline bool seg_sizes_ok(const int64_t n, const int32_t K) { return n > 0 && n <= 0x7fffffff && K > 0 && K <= 65535; }
// slot 15 of a point box (map_points.box_record): the obj_center its network subtracts from a point
__device__ __forceinline__ float box_obj_center(const float* __restrict__ boxes, const int k) {
  return boxes[(int64_t)k * SEG_BOX_FLOATS + 15];
}

// ---------------------------------------------------------------------------------------------- the candidate CSR
constexpr int SEG_WG = 256;           // items per workgroup of the count and emit kernels
constexpr int SEG_SCAN_WG = 1024;

template <class Test>
__global__ void __launch_bounds__(SEG_WG) seg_count_kernel(const int64_t n, const Test test, int64_t* __restrict__ cnt) {
  const int k = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * SEG_WG + threadIdx.x;
  typename Test::Payload pl;
  const bool hit = i < n && test.hit(k, i, pl);
  __shared__ int wcnt[SEG_WG / 64];
  int total;
  wg_exclusive_flag<SEG_WG>(hit, wcnt, total);
  if (threadIdx.x == 0) cnt[(int64_t)k * gridDim.x + blockIdx.x] = total;
}
// grid K: an object with fewer than min_keep hits keeps none.  (This and seg_off_kernel are templates so that only a unit
// that builds a CSR carries them.)
template <int WG>
__global__ void __launch_bounds__(WG) seg_drop_kernel(const int64_t nb, const int min_keep, int64_t* __restrict__ cnt) {
  int64_t* row = cnt + (int64_t)blockIdx.x * nb;
  int v = 0;                                              // (a block counts at most WG, all of them at most n < 2^31)
  for (int64_t b = threadIdx.x; b < nb; b += WG) v += (int)row[b];
  __shared__ int wsum[WG / 64];
  const int total = wg_sum<WG>(v, wsum);
  if (total >= min_keep) return;                          // (uniform over the workgroup)
  for (int64_t b = threadIdx.x; b < nb; b += WG) row[b] = 0;
}
// the scanned counts (cnt [K * nb] exclusive, cnt [K * nb] = M) -> seg_off [K + 1]
template <class T>
__global__ void seg_off_kernel(const int K, const int64_t nb, const T* __restrict__ cnt, T* __restrict__ seg_off) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k <= K) seg_off[k] = cnt[(int64_t)k * nb];
}
template <class Test>
__global__ void __launch_bounds__(SEG_WG) seg_emit_kernel(const int64_t n, const Test test, const int64_t* __restrict__ cnt,
                                                          const int64_t M) {
  const int64_t k = blockIdx.y, nb = gridDim.x;           // (64 bits from the start: the row address stays scalar)
  const int64_t i = (int64_t)blockIdx.x * SEG_WG + threadIdx.x;
  typename Test::Payload pl;
  const bool hit = i < n && test.hit((int)k, i, pl);
  __shared__ int wcnt[SEG_WG / 64];
  int total;
  // both offsets are read here, after the test and ahead of the barrier, in uniform control flow: scalar loads
  const int64_t* row = cnt + k * nb;
  const int64_t end = row[nb];                            // the end of THIS object's segment (banner)
  const int64_t pos = row[blockIdx.x] + wg_exclusive_flag<SEG_WG>(hit, wcnt, total);
  if (hit && pos >= 0 && pos < end && pos < M) test.store(pos, i, pl);
}

inline int64_t seg_blocks(const int64_t n) { return cdiv(n, SEG_WG); }
// 0: n or K out of range
inline size_t seg_csr_workspace_bytes(const int64_t n, const int32_t K) {
  if (!seg_sizes_ok(n, K)) return 0;
  return align256(((size_t)K * (size_t)seg_blocks(n) + 1) * sizeof(int64_t));
}
// ws: seg_csr_workspace_bytes(n, K), kept by the caller until seg_csr_emit has run on the same n, K and test inputs
template <class Test>
int seg_csr_count(const int64_t n, const int32_t K, const Test& test, const int min_keep, void* ws, int64_t* seg_off,
                  hipStream_t st) {
  const int64_t nb = seg_blocks(n);
  int64_t* cnt = (int64_t*)ws;
  hipLaunchKernelGGL(seg_count_kernel<Test>, dim3((unsigned)nb, (unsigned)K), dim3(SEG_WG), 0, st, n, test, cnt);
  CHECK_LAUNCH();
  if (min_keep > 1) {
    hipLaunchKernelGGL(seg_drop_kernel<SEG_WG>, dim3((unsigned)K), dim3(SEG_WG), 0, st, nb, min_keep, cnt);
    CHECK_LAUNCH();
  }
  hipLaunchKernelGGL((wg_scan_kernel<SEG_SCAN_WG, 1, int64_t>), dim3(1), dim3(SEG_SCAN_WG), 0, st, cnt, (int64_t)K * nb,
                     cnt + (int64_t)K * nb);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(seg_off_kernel<int64_t>, dim3((unsigned)cdiv(K + 1, 256)), dim3(256), 0, st, (int)K, nb, (const int64_t*)cnt,
                     seg_off);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}
template <class Test>
int seg_csr_emit(const int64_t n, const int32_t K, const Test& test, const void* ws, const int64_t M, hipStream_t st) {
  hipLaunchKernelGGL(seg_emit_kernel<Test>, dim3((unsigned)seg_blocks(n), (unsigned)K), dim3(SEG_WG), 0, st, n, test,
                     (const int64_t*)ws, M);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

// ------------------------------------------------------------------------------------------------ the ragged walk
struct SegWalkArgs {
  int K;
  const float* params; long p_stride; const float* scale;         // the arena of the hidden-32 objects
  const float* pts; const float* boxes;
  const int32_t* info;                // [K][2]: arena row (-1: not a hidden-32 object, no tile), a flag for the caller
  const int64_t* seg_off; const int32_t* pair_pt;
  obj32::Layout L;
};
__device__ __forceinline__ long seg_tiles(const SegWalkArgs& a, const int k) {
  return a.info[2 * k] >= 0 ? (long)((a.seg_off[k + 1] - a.seg_off[k] + 63) >> 6) : 0L;
}
// Workgroups of 4 independent waves, 16 entries per wave per tile (eval_kernel's form, objnerf_train.hip).  Per tile and
// lane: body(m, valid, n, scale, oc, flag) -- entry m of the CSR, whether it lies inside the object's segment (the last
// tile of a segment is padded with the segment's first entry), its item n = pair_pt[m], the object's scale, obj_center
// and info flag.
// THE RESTAGE HAZARD: the waves run their tiles independently, so where the object changes some may still be reading
// the old image out of LDS: a workgroup barrier BEFORE stage_weights32 overwrites it; stage_weights32 itself ends in
// the barrier that completes the new image.  `staged != k` is uniform over the workgroup (every thread walks the same
// tiles), and body holds no barrier.
template <bool FEAT, class Body>
__device__ __forceinline__ void seg_walk(const SegWalkArgs& a, float* lds, Body&& body) {
  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), c = tid & 15;
  long T = 0;
  for (int k = 0; k < a.K; ++k) T += seg_tiles(a, k);
  const long t0 = T * (long)blockIdx.x / (long)gridDim.x, t1 = T * ((long)blockIdx.x + 1) / (long)gridDim.x;
  int k = 0;
  long kt0 = 0, kt1 = seg_tiles(a, 0);                  // object k owns tiles [kt0, kt1)
  int staged = -1, flag = 0;
  float scale = 1.0f, oc = 0.0f;
  int64_t s0 = 0, s1 = 0;
  for (long t = t0; t < t1; ++t) {
    while (t >= kt1) { ++k; kt0 = kt1; kt1 += seg_tiles(a, k); }      // k < K: t < T
    if (staged != k) {
      __syncthreads();                                  // every wave is done with the image of the object before
      const int row = a.info[2 * k];
      obj32n::stage_weights32(lds, a.params + (long)row * a.p_stride, a.L, FEAT, tid, 256);
      scale = a.scale[row];
      oc = box_obj_center(a.boxes, k);
      flag = a.info[2 * k + 1];
      s0 = a.seg_off[k]; s1 = a.seg_off[k + 1];
      staged = k;
    }
    asm volatile("" ::: "memory");   // keep the LDS weight reads inside the loop (no LICM into registers)
    const int64_t m = s0 + (t - kt0) * 64 + 16 * w + c;
    const bool valid = m < s1;
    body(m, valid, (int64_t)a.pair_pt[valid ? m : s0], scale, oc, flag);
  }
}

// the checks the walks share and their arguments; OBJNERF_OK with M == 0: nothing to launch
inline int seg_walk_args(SegWalkArgs& d, const objnerf_net* net, const int32_t K, const int64_t N, const int64_t M,
                         const float* params, const int64_t p_stride, const float* scale, const float* pts,
                         const float* boxes, const int32_t* info, const int64_t* seg_off, const int32_t* pair_pt) {
  if (!net || !seg_sizes_ok(N, K) || M < 0 || M > (int64_t)SEG_PAIR_LOW || !params || !scale || !pts || !boxes || !info ||
      !seg_off)
    return OBJNERF_EINVAL;
  if (net->hidden != 32 || net->n_freqs != 6) return OBJNERF_ENOTSUP;
  if (M > 0 && !pair_pt) return OBJNERF_EINVAL;
  d.K = K; d.params = params; d.p_stride = (long)p_stride; d.scale = scale; d.pts = pts; d.boxes = boxes; d.info = info;
  d.seg_off = seg_off; d.pair_pt = pair_pt;
  d.L = obj32::make_layout(net->feat_dim);
  return OBJNERF_OK;
}
// two workgroups a compute unit (the image is 60 / 73 KB), never more than the tiles there can be
inline dim3 seg_walk_grid(const int64_t M, const int32_t K) {
  const int64_t G = 2 * (int64_t)objnerf_num_cu(), t_max = M / 64 + K;
  return dim3((unsigned)(G > t_max ? t_max : G));
}

}  // namespace
