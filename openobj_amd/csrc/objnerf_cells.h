// Grid cells over fp64 point sets, shared by the units that search sorted cell keys (objnerf_maskgraph.hip: fixed-radius
// questions; objnerf_mapeval.hip: exact nearest points).  A key is ix << 42 | iy << 21 | iz with 21 bits an axis, written
// by objnerf_cell_keys; sorted per segment, the cells (x, y, z0 .. z1) of one column are one run of adjacent keys.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "objnerf_segments.h"       // seg_of: the segment of a row

namespace {

constexpr int CELL_BITS = 21;
constexpr int64_t CELL_MAX = (1ll << CELL_BITS) - 1;

__device__ __forceinline__ int64_t cell_key(const int64_t x, const int64_t y, const int64_t z) {
  return (x << (2 * CELL_BITS)) | (y << CELL_BITS) | z;
}

__device__ __forceinline__ int64_t lower_bound(const int64_t* __restrict__ keys, int64_t lo, int64_t hi, const int64_t k) {
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (keys[m] < k) lo = m + 1; else hi = m;
  }
  return lo;
}

__device__ __forceinline__ double dist2(const double* __restrict__ q, const double p[3]) {
  const double dx = __dsub_rn(q[0], p[0]), dy = __dsub_rn(q[1], p[1]), dz = __dsub_rn(q[2], p[2]);
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

}  // namespace
