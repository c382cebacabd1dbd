// Part regions: the connected surface patches of a part query on the map's meshes, with pose.
//
// (a) objnerf_regions_label   vertex v of object s is SELECTED iff sims[v][q] >= thr[s] (one fp32 compare; a NaN on either
//     side selects nothing).  Two selected vertices are connected iff some face names both.  Union-find whose parent is
//     always a smaller index (uf_find / uf_union of objnerf_wg.h) over the packed vertex ids, one thread per face (which
//     then points its vertices at the root it finds, to keep the chains short), then a flatten: the root of a region is its smallest packed vertex index, whatever order the unions ran in.
// (b) the roots compacted per object in ascending vertex order (seg_csr_count / _emit of objnerf_segments.h with the
//     objects as segments: no atomic decides an order) -> reg_off [S + 1], label [V] = the row of the vertex's region.
// (c) objnerf_regions_table   one int64 table [R][32], filled by integer atomics only: any schedule gives the same bytes.
//     A vertex launch (count, box, peak), face pass A (faces, area, first moments, normal), a launch over the rows (the
//     centroid relative to the object's anchor, fp64), face pass B (second moments about that centroid, and the first
//     moments that are left about it: the centroid's own rounding, which the host adds back).
// Every fp64 operation of the face passes is rounded on its own (_rn intrinsics; the unit is built with
// -ffp-contract=off as well); the sequence stands in include/objnerf_hip.h.
// THE WAVE FOLD: marching cubes emits faces in cell order, so neighbouring lanes mostly share a row.  A segmented scan
// over lane order folds every run of equal rows; the last lane of a run issues its atomics.  64 lanes of one row cost 8
// atomics instead of 512; 64 lanes of 64 rows cost what they would have cost without the fold, plus the scan.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "objnerf_segments.h"

namespace {

#define CLEAR_STALE() (void)hipGetLastError()

constexpr int RG_WG = 256;
constexpr int RG_ROW = OBJNERF_REGION_ROW;
// columns of a row
constexpr int RG_ROOT = 0, RG_OBJ = 1, RG_NV = 2, RG_NF = 3, RG_AREA = 4, RG_M1 = 5, RG_NRM = 8, RG_MIN = 11, RG_MAX = 14,
              RG_PEAK = 17, RG_CEN = 18, RG_M2 = 21, RG_RES = 27;
constexpr int RG_BAD_ID = 1, RG_CROSS = 2, RG_NONFINITE = 4;
constexpr double RG_SCALE = 17592186044416.0;               // 2^44
constexpr double RG_LIMIT = 4611686018427387904.0;          // 2^62: a scaled value at or past it counts as non-finite

struct RegArgs {
  int64_t V, F; int S, Q, q;
  const int64_t* vert_off; const int64_t* face_off;
  const double* verts; const int32_t* faces; const float* sims; const float* thr;
  int32_t* root; int32_t* label; int64_t R; int64_t* table; int32_t* status;
};

// order-preserving key of an fp32: a < b as floats <=> key(a) < key(b) as unsigned (-0 below +0)
__device__ __forceinline__ uint32_t f32_key(const float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The three packed vertex ids of face f and its object.  false: the face joins nothing and contributes nothing (an id
// outside [0, V): bit 0; an id outside the face's own object: bit 1).  Nothing is read through a rejected id.
__device__ __forceinline__ bool face_ids(const RegArgs& a, const int64_t f, int& ia, int& ib, int& ic, int& s) {
  ia = a.faces[3 * f]; ib = a.faces[3 * f + 1]; ic = a.faces[3 * f + 2];
  s = seg_of(a.face_off, a.S, f);
  if (ia < 0 || ia >= a.V || ib < 0 || ib >= a.V || ic < 0 || ic >= a.V) {
    atomicOr(a.status, RG_BAD_ID);
    return false;
  }
  const int64_t v0 = a.vert_off[s], v1 = a.vert_off[s + 1];
  if (ia < v0 || ia >= v1 || ib < v0 || ib >= v1 || ic < v0 || ic >= v1) {
    atomicOr(a.status, RG_CROSS);
    return false;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------------- labelling
__global__ __launch_bounds__(RG_WG) void rg_select_kernel(const RegArgs a) {
  const int64_t v = (int64_t)blockIdx.x * RG_WG + threadIdx.x;
  if (v >= a.V) return;
  const int s = seg_of(a.vert_off, a.S, v);
  a.root[v] = a.sims[v * a.Q + a.q] >= a.thr[s] ? (int32_t)v : -1;
}

// one thread per face; uf_union's loops end because a parent is always a smaller index and only ever decreases
__global__ __launch_bounds__(RG_WG) void rg_union_kernel(const RegArgs a) {
  const int64_t f = (int64_t)blockIdx.x * RG_WG + threadIdx.x;
  if (f >= a.F) return;
  int ia, ib, ic, s;
  if (!face_ids(a, f, ia, ib, ic, s)) return;
  const bool sa = a.root[ia] >= 0, sb = a.root[ib] >= 0, sc = a.root[ic] >= 0;   // (selected: never changes sign)
  if (sa && sb) uf_union(a.root, ia, ib);
  if (sb && sc) uf_union(a.root, ib, ic);
  if (sa && sc && !sb) uf_union(a.root, ia, ic);
  // Shorten the chains that later finds walk: an entry may take any of its ancestors (it stays <= its index, only ever
  // decreases, and still leads to the root), so the invariants of uf_find / uf_union hold.
  if (sa) atomicMin(&a.root[ia], uf_find(a.root, ia));
  if (sb) atomicMin(&a.root[ib], uf_find(a.root, ib));
  if (sc) atomicMin(&a.root[ic], uf_find(a.root, ic));
}

__global__ __launch_bounds__(RG_WG) void rg_flatten_kernel(const int64_t V, int32_t* root) {
  const int64_t v = (int64_t)blockIdx.x * RG_WG + threadIdx.x;
  if (v >= V) return;
  if (root[v] >= 0) root[v] = uf_find(root, (int)v);
}

// the roots of object k in ascending vertex order; item i is the object's i-th vertex
struct RegionRootTest {
  typedef int64_t Payload;
  const int64_t* vert_off; const int32_t* root; int32_t* label; int64_t V;
  __device__ bool hit(const int k, const int64_t i, int64_t& v) const {
    v = vert_off[k] + i;
    return v >= 0 && v < V && v < vert_off[k + 1] && root[v] == (int32_t)v;
  }
  __device__ void store(const int64_t pos, const int64_t, const int64_t v) const { label[v] = (int32_t)pos; }
};

// every other vertex takes its root's row (the emit wrote the roots' entries, this writes only the others')
__global__ __launch_bounds__(RG_WG) void rg_spread_kernel(const int64_t V, const int32_t* __restrict__ root, int32_t* label) {
  const int64_t v = (int64_t)blockIdx.x * RG_WG + threadIdx.x;
  if (v >= V) return;
  const int r = root[v];
  if (r == (int32_t)v) return;
  label[v] = r >= 0 && r < V ? label[r] : -1;
}

// ------------------------------------------------------------------------------------------------------ the wave fold
// Runs of equal row over lane order: `start` is the first lane of this lane's run, the LAST lane of a run is its leader.
struct WaveRuns {
  int lane, start; bool leader;
  __device__ __forceinline__ explicit WaveRuns(const int64_t row) {
    lane = threadIdx.x & 63;
    const int64_t prev = __shfl_up((long long)row, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != row);
    start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
    leader = lane == 63 || ((heads >> (lane + 1)) & 1ull);
  }
  // the inclusive segmented scan: in the leader, op over the whole run (64-bit values travel as two 32-bit halves)
  template <class T, class Op>
  __device__ __forceinline__ T fold(T v, const Op op) const {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const T u = __shfl_up(v, d);
      if (lane - d >= start) v = op(v, u);
    }
    return v;
  }
};
struct OpAdd { __device__ __forceinline__ long long operator()(const long long x, const long long y) const { return x + y; } };
struct OpMin {
  __device__ __forceinline__ unsigned long long operator()(const unsigned long long x, const unsigned long long y) const {
    return x < y ? x : y;
  }
};
struct OpMax {
  __device__ __forceinline__ unsigned long long operator()(const unsigned long long x, const unsigned long long y) const {
    return x > y ? x : y;
  }
};

__device__ __forceinline__ void row_add(int64_t* row, const int col, const long long v) {
  if (v != 0) atomicAdd((unsigned long long*)&row[col], (unsigned long long)v);
}

// x * 2^44 rounded to the nearest integer (ties to even); a NaN, an infinity or a value at or past 2^62 counts as 0
__device__ __forceinline__ long long q44(const double x, bool& bad) {
  const double y = __dmul_rn(x, RG_SCALE);
  if (!(fabs(y) < RG_LIMIT)) { bad = true; return 0; }
  return llrint(y);
}

// ---------------------------------------------------------------------------------------------------------- the table
__global__ __launch_bounds__(RG_WG) void rg_rows_init_kernel(const int64_t R, int64_t* __restrict__ table) {
  const int64_t i = (int64_t)blockIdx.x * RG_WG + threadIdx.x;
  if (i >= R * RG_ROW) return;
  const int c = (int)(i % RG_ROW);
  table[i] = c >= RG_MIN && c < RG_MIN + 3 ? 0xFFFFFFFFll : 0;
}

// one thread per vertex: the count, the box of the coordinates rounded to fp32, the peak; the root writes root and object
__global__ __launch_bounds__(RG_WG) void rg_vertex_kernel(const RegArgs a) {
  const int64_t v = (int64_t)blockIdx.x * RG_WG + threadIdx.x;
  int64_t row = -1;
  unsigned long long key[3] = {0, 0, 0}, peak = 0;
  if (v < a.V) {
    const int r = a.label[v];
    if (r >= 0 && r < a.R) {
      row = r;
      for (int c = 0; c < 3; ++c) key[c] = f32_key((float)a.verts[3 * v + c]);
      peak = ((unsigned long long)f32_key(a.sims[v * a.Q + a.q]) << 32) | (unsigned long long)(~(uint32_t)v);
      if (a.root[v] == (int32_t)v) {
        a.table[row * RG_ROW + RG_ROOT] = v;
        a.table[row * RG_ROW + RG_OBJ] = seg_of(a.vert_off, a.S, v);
      }
    }
  }
  if (__ballot(row >= 0) == 0ull) return;                   // (uniform over the wave)
  const WaveRuns runs(row);
  const long long cnt = runs.fold((long long)(row >= 0), OpAdd());
  unsigned long long lo[3], hi[3];
  for (int c = 0; c < 3; ++c) {
    lo[c] = runs.fold(key[c], OpMin());
    hi[c] = runs.fold(key[c], OpMax());
  }
  peak = runs.fold(peak, OpMax());
  if (!runs.leader || row < 0) return;
  int64_t* t = a.table + row * RG_ROW;
  row_add(t, RG_NV, cnt);
  for (int c = 0; c < 3; ++c) {
    atomicMin((unsigned long long*)&t[RG_MIN + c], lo[c]);
    atomicMax((unsigned long long*)&t[RG_MAX + c], hi[c]);
  }
  atomicMax((unsigned long long*)&t[RG_PEAK], peak);
}

// the centroid of every region relative to its object's anchor: m1 / area in fp64, 0 for a region without area
__global__ __launch_bounds__(RG_WG) void rg_centroid_kernel(const int64_t R, int64_t* __restrict__ table) {
  const int64_t r = (int64_t)blockIdx.x * RG_WG + threadIdx.x;
  if (r >= R) return;
  int64_t* t = table + r * RG_ROW;
  const double area = (double)t[RG_AREA];
  for (int c = 0; c < 3; ++c) t[RG_CEN + c] = __double_as_longlong(area > 0.0 ? __ddiv_rn((double)t[RG_M1 + c], area) : 0.0);
}

// One thread per face.  PASS 0: face count, area, first moments, normal (8 values); PASS 1: the six second moments about
// the centroid and the three residual first moments (9 values).  A face contributes iff all three of its vertices are selected: they are then in one region.
template <int PASS>
__global__ __launch_bounds__(RG_WG) void rg_face_kernel(const RegArgs a) {
  constexpr int NV = PASS == 0 ? 8 : 9;
  const int64_t f = (int64_t)blockIdx.x * RG_WG + threadIdx.x;
  int64_t row = -1;
  long long val[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) val[i] = 0;
  int ia, ib, ic, s;
  if (f < a.F && face_ids(a, f, ia, ib, ic, s)) {
    const int ra = a.label[ia], rb = a.label[ib], rc = a.label[ic];
    if (ra >= 0 && rb >= 0 && rc >= 0 && ra < a.R) {
      row = ra;
      const double* an = a.verts + 3 * a.vert_off[s];
      const double* A = a.verts + 3 * (int64_t)ia, *B = a.verts + 3 * (int64_t)ib, *Cc = a.verts + 3 * (int64_t)ic;
      double dA[3], dB[3], dC[3], u[3], w[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        dA[c] = __dsub_rn(A[c], an[c]); dB[c] = __dsub_rn(B[c], an[c]); dC[c] = __dsub_rn(Cc[c], an[c]);
        u[c] = __dsub_rn(dB[c], dA[c]); w[c] = __dsub_rn(dC[c], dA[c]);
      }
      const double cr[3] = {__dsub_rn(__dmul_rn(u[1], w[2]), __dmul_rn(u[2], w[1])),
                            __dsub_rn(__dmul_rn(u[2], w[0]), __dmul_rn(u[0], w[2])),
                            __dsub_rn(__dmul_rn(u[0], w[1]), __dmul_rn(u[1], w[0]))};
      const double area = __dmul_rn(0.5, __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(cr[0], cr[0]), __dmul_rn(cr[1], cr[1])),
                                                              __dmul_rn(cr[2], cr[2]))));
      bool bad = false;
      if (PASS == 0) {
        val[0] = 1;
        val[1] = q44(area, bad);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double sc = __dadd_rn(__dadd_rn(dA[c], dB[c]), dC[c]);
          val[2 + c] = q44(__ddiv_rn(__dmul_rn(area, sc), 3.0), bad);
          val[5 + c] = q44(__dmul_rn(0.5, cr[c]), bad);
        }
      } else {
        const int64_t* t = a.table + row * RG_ROW;
        double e[3][3], tt[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double cen = __longlong_as_double(t[RG_CEN + c]);
          e[0][c] = __dsub_rn(dA[c], cen); e[1][c] = __dsub_rn(dB[c], cen); e[2][c] = __dsub_rn(dC[c], cen);
          tt[c] = __dadd_rn(__dadd_rn(e[0][c], e[1][c]), e[2][c]);
        }
        int n = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
          for (int k = j; k < 3; ++k) {
            const double m = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(e[0][j], e[0][k]), __dmul_rn(e[1][j], e[1][k])),
                                                 __dmul_rn(e[2][j], e[2][k])), __dmul_rn(tt[j], tt[k]));
            val[n++] = q44(__ddiv_rn(__dmul_rn(area, m), 12.0), bad);
          }
#pragma unroll
        for (int c = 0; c < 3; ++c) val[6 + c] = q44(__ddiv_rn(__dmul_rn(area, tt[c]), 3.0), bad);
      }
      if (bad) atomicOr(a.status, RG_NONFINITE);
    }
  }
  if (__ballot(row >= 0) == 0ull) return;                   // (uniform over the wave)
  const WaveRuns runs(row);
#pragma unroll
  for (int i = 0; i < NV; ++i) val[i] = runs.fold(val[i], OpAdd());
  if (!runs.leader || row < 0) return;
  int64_t* t = a.table + row * RG_ROW;
  if (PASS == 0) {
    row_add(t, RG_NF, val[0]);
    row_add(t, RG_AREA, val[1]);
#pragma unroll
    for (int c = 0; c < 3; ++c) { row_add(t, RG_M1 + c, val[2 + c]); row_add(t, RG_NRM + c, val[5 + c]); }
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) row_add(t, i < 6 ? RG_M2 + i : RG_RES + i - 6, val[i]);
  }
}

inline bool rg_sizes_ok(const int64_t V, const int64_t F, const int32_t S) {
  return V >= 1 && V <= 0x7fffffff && F >= 0 && F <= 0x7fffffff && S >= 1 && S <= 65535;
}

}  // namespace

extern "C" {

size_t objnerf_regions_workspace_bytes(int64_t V, int64_t F, int32_t S) {
  if (!rg_sizes_ok(V, F, S)) return 0;
  return seg_csr_workspace_bytes(V, S);
}

int objnerf_regions_label(int64_t V, int64_t F, int32_t S, int64_t vmax, int32_t Q, int32_t q, const int64_t* vert_off,
                          const int64_t* face_off, const int32_t* faces, const float* sims, const float* thr, void* ws,
                          size_t ws_bytes, int32_t* root, int32_t* label, int64_t* reg_off, int32_t* status, void* stream) {
  CLEAR_STALE();
  if (!rg_sizes_ok(V, F, S) || vmax < 1 || vmax > V || Q < 1 || Q > 16 || q < 0 || q >= Q) return OBJNERF_EINVAL;
  if (!vert_off || !face_off || (F > 0 && !faces) || !sims || !thr || !ws || !root || !label || !reg_off || !status)
    return OBJNERF_EINVAL;
  if (ws_bytes < objnerf_regions_workspace_bytes(V, F, S)) return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  RegArgs a{V, F, S, Q, q, vert_off, face_off, nullptr, faces, sims, thr, root, label, 0, nullptr, status};
  const dim3 gv((unsigned)cdiv(V, RG_WG)), gf((unsigned)cdiv(F, RG_WG));
  hipLaunchKernelGGL(rg_select_kernel, gv, dim3(RG_WG), 0, st, a);
  CHECK_LAUNCH();
  if (F > 0) {
    hipLaunchKernelGGL(rg_union_kernel, gf, dim3(RG_WG), 0, st, a);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(rg_flatten_kernel, gv, dim3(RG_WG), 0, st, V, root);
    CHECK_LAUNCH();
  }
  const RegionRootTest test{vert_off, root, label, V};
  int rc = seg_csr_count(vmax, S, test, 1, ws, reg_off, st);
  if (rc != OBJNERF_OK) return rc;
  rc = seg_csr_emit(vmax, S, test, ws, V, st);
  if (rc != OBJNERF_OK) return rc;
  hipLaunchKernelGGL(rg_spread_kernel, gv, dim3(RG_WG), 0, st, V, (const int32_t*)root, label);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_regions_table(int64_t V, int64_t F, int32_t S, int32_t Q, int32_t q, const int64_t* vert_off,
                          const int64_t* face_off, const double* verts, const int32_t* faces, const float* sims,
                          const int32_t* root, const int32_t* label, int64_t R, int64_t* table, int32_t* status,
                          void* stream) {
  CLEAR_STALE();
  if (!rg_sizes_ok(V, F, S) || Q < 1 || Q > 16 || q < 0 || q >= Q || R < 0 || R > V) return OBJNERF_EINVAL;
  if (!vert_off || !face_off || !verts || (F > 0 && !faces) || !sims || !root || !label || (R > 0 && !table) || !status)
    return OBJNERF_EINVAL;
  if (R == 0) return OBJNERF_OK;
  hipStream_t st = (hipStream_t)stream;
  RegArgs a{V, F, S, Q, q, vert_off, face_off, verts, faces, sims, nullptr, (int32_t*)root, (int32_t*)label, R, table, status};
  const dim3 gv((unsigned)cdiv(V, RG_WG)), gf((unsigned)cdiv(F, RG_WG)), gr((unsigned)cdiv(R, RG_WG));
  hipLaunchKernelGGL(rg_rows_init_kernel, dim3((unsigned)cdiv(R * RG_ROW, RG_WG)), dim3(RG_WG), 0, st, R, table);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(rg_vertex_kernel, gv, dim3(RG_WG), 0, st, a);
  CHECK_LAUNCH();
  if (F > 0) {
    hipLaunchKernelGGL(rg_face_kernel<0>, gf, dim3(RG_WG), 0, st, a);
    CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(rg_centroid_kernel, gr, dim3(RG_WG), 0, st, R, table);
  CHECK_LAUNCH();
  if (F > 0) {
    hipLaunchKernelGGL(rg_face_kernel<1>, gf, dim3(RG_WG), 0, st, a);
    CHECK_LAUNCH();
  }
  return OBJNERF_OK;
}

}  // extern "C"
