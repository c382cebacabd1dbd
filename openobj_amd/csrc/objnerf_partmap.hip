// Part-level feature maps in their compact form (the reference's partlevel/sam_clip_dir.py:113-133): a frame with M
// masks holds at most M + 1 distinct feature vectors, so the map is an index image plus a table of rows.
//
// (a) objnerf_part_index: the mask loop of :118-125 without the features.  The reference assigns mask after mask, so a
//     pixel keeps the LAST mask that covers it: a thread per pixel scans the masks from the last to the first and stops
//     at the first set byte (lanes of a wave read neighbouring bytes of one mask: coalesced), -1 where none is set.
// (b) objnerf_part_dense: out[p][:] = table[index[p]][:], the reference's dense [H'][W'][C] image from the compact form:
//     a wave per pixel, 16 bytes per lane when the rows allow it (the sampler's row copy, objnerf_misc.hip).
// Both clamp what they read into the table; plain stores, no atomics; two calls write the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "objnerf_wg.h"

namespace {

#define CLEAR_STALE() (void)hipGetLastError()

constexpr int PM_WG = 256;

__global__ __launch_bounds__(PM_WG) void part_index_kernel(const int M, const long n_px, const uint8_t* __restrict__ masks,
                                                           int32_t* __restrict__ out) {
  const long p = (long)blockIdx.x * PM_WG + threadIdx.x;
  if (p >= n_px) return;
  int found = -1;
  for (int m = M - 1; m >= 0; --m) {
    if (masks[(long)m * n_px + p]) { found = m; break; }
  }
  out[p] = found;
}

__global__ __launch_bounds__(PM_WG) void part_dense_kernel(const long n_px, const int C, const int rows,
                                                           const int32_t* __restrict__ index,
                                                           const float* __restrict__ table, float* __restrict__ out,
                                                           const int vec) {
  const int lane = threadIdx.x & 63;
  const long p = (long)blockIdx.x * (PM_WG / 64) + (threadIdx.x >> 6);           // a wave per pixel
  if (p >= n_px) return;
  const int r = min(max(index[p], 0), rows - 1);
  const float* src = table + (long)r * C;
  float* dst = out + p * C;
  if (vec) {
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    for (int c = lane; c < C / 4; c += 64) ((f32x4v*)dst)[c] = ((const f32x4v*)src)[c];
  } else {
    for (int c = lane; c < C; c += 64) dst[c] = src[c];
  }
}

}  // namespace

extern "C" {

int objnerf_part_index(int32_t M, int32_t Hp, int32_t Wp, const uint8_t* masks, int32_t* out, void* stream) {
  CLEAR_STALE();
  if (M < 0 || Hp <= 0 || Wp <= 0 || !out || (M > 0 && !masks)) return OBJNERF_EINVAL;
  const long n_px = (long)Hp * Wp;
  if ((n_px + PM_WG - 1) / PM_WG > 0x7fffffffl) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(part_index_kernel, dim3((unsigned)((n_px + PM_WG - 1) / PM_WG)), dim3(PM_WG), 0, (hipStream_t)stream,
                     M, n_px, masks, out);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_part_dense(int64_t n_px, int32_t C, int32_t rows, const int32_t* index, const float* table, float* out,
                       void* stream) {
  CLEAR_STALE();
  if (n_px <= 0 || C <= 0 || rows <= 0 || !index || !table || !out) return OBJNERF_EINVAL;
  const long blocks = (n_px + PM_WG / 64 - 1) / (PM_WG / 64);
  if (blocks > 0x7fffffffl) return OBJNERF_EINVAL;
  const int vec = (C & 3) == 0 && (((size_t)table | (size_t)out) & 15) == 0;
  hipLaunchKernelGGL(part_dense_kernel, dim3((unsigned)blocks), dim3(PM_WG), 0, (hipStream_t)stream, (long)n_px, C, rows,
                     index, table, out, vec);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

}  // extern "C"
