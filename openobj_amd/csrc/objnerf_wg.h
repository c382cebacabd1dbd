// Workgroup scan / compaction primitives and the host helpers of the map-side units (mesh, bounds, query, mask graph,
// part maps): count / scan / emit is written here once.  Every value is an integer, so any summation order gives the
// same bits; prefixes run in thread order (thread t's items come before thread t + 1's), which is what keeps the
// emitted vertices, points, labels and edges in the order the callers document.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/objnerf_hip.h"

// ------------------------------------------------------------------------------------------------------------- host
#define CHECK_LAUNCH() do { if (hipGetLastError() != hipSuccess) return OBJNERF_ELAUNCH; } while (0)

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// --------------------------------------------------------------------------- over the threads of one workgroup of WG
// WG is a multiple of 64; `lds` holds WG / 64 ints and is free again after the caller's next barrier.  Every thread
// of the workgroup makes the call (there is a barrier inside).

// the per-wave halves: set bits of a ballot below this lane; inclusive prefix of v over the lanes of the wave
__device__ __forceinline__ int wave_rank(const unsigned long long ballot) {
  return __popcll(ballot & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// (a 32- or 64-bit integer through the 32-bit DPP / readlane paths)
template <int CTRL, class T>
__device__ __forceinline__ T dpp_or_zero(const T v) {       // v of the lane CTRL selects in this row of 16, 0 without one
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "32- or 64-bit integers");
  if constexpr (sizeof(T) == 4) {
    return (T)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
  } else {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned long long)v, CTRL, 0xF, 0xF, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)((unsigned long long)v >> 32), CTRL, 0xF, 0xF, false);
    return (T)(((unsigned long long)hi << 32) | lo);
  }
}

template <class T>
__device__ __forceinline__ T lane_get(const T v, const int l) {
  if constexpr (sizeof(T) == 4) {
    return (T)__builtin_amdgcn_readlane((int)v, l);
  } else {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned long long)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)((unsigned long long)v >> 32), l);
    return (T)(((unsigned long long)hi << 32) | lo);
  }
}

// row_shr:1 / 2 / 4 / 8 inside each row of 16 lanes on the VALU, the rows linked by three v_readlane broadcasts (the
// form of objnerf_device.h's SegRows::scan_add): no LDS permutes.  With __shfl_up (six ds_bpermute a 32-bit word) the
// one-workgroup scan below was LDS-bound and slower than the serial scan it replaced (profiles/wg_prims_refactor.txt).
template <class T>
__device__ __forceinline__ T wave_inclusive(T v) {
  v += dpp_or_zero<0x111>(v);
  v += dpp_or_zero<0x112>(v);
  v += dpp_or_zero<0x114>(v);
  v += dpp_or_zero<0x118>(v);
  const int row = (threadIdx.x & 63) >> 4;
  const T t0 = lane_get(v, 15), t1 = lane_get(v, 31), t2 = lane_get(v, 47);
  return v + (row > 0 ? t0 : (T)0) + (row > 1 ? t1 : (T)0) + (row > 2 ? t2 : (T)0);
}

// the per-wave totals (handed in by one lane per wave) -> the sum over the waves before this one, and over all
template <int WG>
__device__ __forceinline__ int wg_fold(const bool writer, const int wave_total, int* lds, int& total) {
  const int wave = threadIdx.x >> 6;
  if (writer) lds[wave] = wave_total;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < WG / 64; ++w) {
    before += w < wave ? lds[w] : 0;
    total += lds[w];
  }
  return before;
}

// exclusive prefix of v in thread order, and the workgroup's total
template <int WG>
__device__ __forceinline__ int wg_exclusive(const int v, int* lds, int& total) {
  const int inc = wave_inclusive(v);
  return wg_fold<WG>((threadIdx.x & 63) == 63, inc, lds, total) + inc - v;
}

// the same for one flag per thread: a ballot and a population count (a name of its own: an int that holds a flag
// must not pick the scan by accident)
template <int WG>
__device__ __forceinline__ int wg_exclusive_flag(const bool flag, int* lds, int& total) {
  const unsigned long long bal = __ballot(flag);
  return wg_fold<WG>((threadIdx.x & 63) == 0, __popcll(bal), lds, total) + wave_rank(bal);
}

// the workgroup's sum of v, in every thread
template <int WG>
__device__ __forceinline__ int wg_sum(int v, int* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  int total;
  wg_fold<WG>((threadIdx.x & 63) == 0, v, lds, total);
  return total;
}

// ------------------------------------------------------------------------------------------------------ union-find
// L[a] <= a always, and only ever decreases: every loop below ends, and a stale read is still an ancestor.
__device__ __forceinline__ int uf_find(const volatile int* L, int a) {
  int p;
  while ((p = L[a]) != a) a = p;
  return a;
}
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
  for (;;) {
    a = uf_find(L, a);
    b = uf_find(L, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[b], a);           // b was a root: hang it under a, unless somebody got there first
    if (old == b) return;
    b = old;
  }
}

// ------------------------------------------------------------------- over an array in global memory, by one workgroup
// out[i][c] = in[0][c] + .. + in[i - 1][c] for i < n, total[c] = the sum of all n (in every thread), over NCH
// interleaved channels.  Tiles of WG x WG_SCAN_ITEMS elements; a wave owns 64 x WG_SCAN_ITEMS neighbours and takes
// them 64 at a time (coalesced): a wave scan of each step on top of the wave's running sum, then the waves' totals
// through LDS and the carry in a register; two barriers a tile.  out may alias in when In == Out: an element is read
// and written by the same thread, read first.
constexpr int WG_SCAN_ITEMS = 4;

template <int WG, int NCH, class In, class Out>
__device__ __forceinline__ void wg_scan_exclusive(const In* in, Out* out, const int64_t n, Out total[NCH]) {
  __shared__ Out wtot[NCH][WG / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < NCH; ++c) total[c] = 0;
  for (int64_t c0 = 0; c0 < n; c0 += WG * WG_SCAN_ITEMS) {
    const int64_t i0 = c0 + (int64_t)wave * (64 * WG_SCAN_ITEMS) + lane;
    Out v[WG_SCAN_ITEMS][NCH], inc[WG_SCAN_ITEMS][NCH], run[NCH];
#pragma unroll
    for (int k = 0; k < WG_SCAN_ITEMS; ++k)
#pragma unroll
      for (int c = 0; c < NCH; ++c) v[k][c] = i0 + 64 * k < n ? (Out)in[(i0 + 64 * k) * NCH + c] : (Out)0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      run[c] = 0;
#pragma unroll
      for (int k = 0; k < WG_SCAN_ITEMS; ++k) {
        inc[k][c] = run[c] + wave_inclusive(v[k][c]);
        run[c] = lane_get(inc[k][c], 63);
      }
      if (lane == 0) wtot[c][wave] = run[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      Out before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < WG / 64; ++w) {
        before += w < wave ? wtot[c][w] : (Out)0;
        all += wtot[c][w];
      }
#pragma unroll
      for (int k = 0; k < WG_SCAN_ITEMS; ++k)
        if (i0 + 64 * k < n) out[(i0 + 64 * k) * NCH + c] = total[c] + before + inc[k][c] - v[k][c];
      total[c] += all;
    }
    __syncthreads();                                       // wtot is free for the next tile
  }
}

// v [n][NCH] -> its exclusive prefix in place, the totals at total[0 .. NCH); launched with one workgroup
template <int WG, int NCH, class T>
static __global__ void __launch_bounds__(WG) wg_scan_kernel(T* v, const int64_t n, T* total) {
  T t[NCH];
  wg_scan_exclusive<WG, NCH>(v, v, n, t);
  if (threadIdx.x == 0)
    for (int c = 0; c < NCH; ++c) total[c] = t[c];
}

// ------------------------------------------------------------------------------------------------------------- rows
typedef float floatx4 __attribute__((ext_vector_type(4)));

// elements k0 .. k0 + 3 of a row of D floats; zero past D, and the whole of it unless ok (p is not read then).
// VEC: D % 4 == 0 and the row is 16-byte aligned, so the float4 is whole and inside the row.
template <bool VEC>
__device__ __forceinline__ float4 load_row4(const float* __restrict__ p, const int k0, const int D, const bool ok) {
  float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!ok || k0 >= D) return f;
  if (VEC) return *(const float4*)(p + k0);
  f.x = p[k0];
  if (k0 + 1 < D) f.y = p[k0 + 1];
  if (k0 + 2 < D) f.z = p[k0 + 2];
  if (k0 + 3 < D) f.w = p[k0 + 3];
  return f;
}
