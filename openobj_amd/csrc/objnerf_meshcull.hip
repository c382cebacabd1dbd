// Culling meshes to what the frames of a sequence observed (openobj_amd/map_cull.py; the step vMAP's, iMAP's and
// NICE-SLAM's evaluations run before accuracy / completion -- the reference has no counterpart):
//
// (a) objnerf_vertex_views: views[v] += the number of the batch's frames that see vertex v.  A thread owns a vertex and
//     walks the frames; per (vertex p, frame f), in fp64, every operation rounded once and in this order:
//       xc = ((M[0] px + M[1] py) + M[2] pz) + M[3]    (yc: M[4..7], zc: M[8..11]; M = T_CW[f], 3 x 4 row-major)
//       front  = zc > z_min
//       u = (fx xc) / zc + cx,  v = (fy yc) / zc + cy;  iu = floor(u + 0.5),  iv = floor(v + 0.5)
//       inside = front and margin <= iu <= W - 1 - margin and margin <= iv <= H - 1 - margin     (compared as doubles)
//       seen   = inside and d > 0 and zc <= d + eps,  d = (double) depth[f][iu][iv]               (depth is [W][H])
//     A NaN or an infinity makes a comparison false, so nothing is converted to an integer or read before `inside`
//     holds.  The frame index is workgroup-uniform: the twelve pose doubles come through scalar loads.  The count lives
//     in a register and is added to views[v] once by the owning thread: no atomics; a sequence streamed through in any
//     batches gives the same integers.
// (b) objnerf_mesh_cull_count / _emit: the faces a vertex mask keeps and exactly the vertices those faces use, both in
//     their original order (count / scan / emit of objnerf_wg.h):
//       mcl_face_kernel   per face: kept under the rule (ALL / ANY corner kept; a corner outside [0, V) drops the face,
//                         sets the status word and is never dereferenced) -> plain byte stores of 1 into the zeroed
//                         used[] (racing writers store the same value) and the workgroup's number of kept faces;
//       mcl_vert_kernel   the workgroup's number of used vertices;
//       wg_scan_kernel    over each array of totals;
//       mcl_vert_emit / mcl_face_emit   new_of_old, old_of_new, then the kept faces re-indexed and their old rows.
//     Integers only, no atomics (the status word is a plain store of its one bit); two calls write the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "objnerf_wg.h"

namespace {

constexpr int CULL_WG = 256;
constexpr int VV_GRID_CAP = 4096;         // workgroups of objnerf_vertex_views; the vertices beyond are grid-strided

enum : int32_t { CULL_BAD_INDEX = 1 };

// ------------------------------------------------------------------------------------------------------ vertex views
struct VvArgs {
  int64_t V; int32_t B, W, H;
  double fx, fy, cx, cy, z_min, eps;
  double u_lo, u_hi, v_lo, v_hi;            // margin, W - 1 - margin, margin, H - 1 - margin
};

__device__ __forceinline__ double row_dot(const double* __restrict__ m, const double px, const double py, const double pz) {
  return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[0], px), __dmul_rn(m[1], py)), __dmul_rn(m[2], pz)), m[3]);
}

__global__ void __launch_bounds__(CULL_WG) vertex_views_kernel(const VvArgs a, const double* __restrict__ verts,
                                                               const double* __restrict__ t_cw,
                                                               const float* __restrict__ depth,
                                                               int32_t* __restrict__ views) {
  const int64_t frame_px = (int64_t)a.W * a.H;
  for (int64_t v = (int64_t)blockIdx.x * CULL_WG + threadIdx.x; v < a.V; v += (int64_t)gridDim.x * CULL_WG) {
    const double px = verts[3 * v], py = verts[3 * v + 1], pz = verts[3 * v + 2];
    int c = 0;
    for (int f = 0; f < a.B; ++f) {
      const double* __restrict__ m = t_cw + 12 * (int64_t)f;            // uniform over the workgroup
      const double zc = row_dot(m + 8, px, py, pz);
      if (!(zc > a.z_min)) continue;
      const double xc = row_dot(m, px, py, pz), yc = row_dot(m + 4, px, py, pz);
      const double iu = floor(__dadd_rn(__dadd_rn(__ddiv_rn(__dmul_rn(a.fx, xc), zc), a.cx), 0.5));
      const double iv = floor(__dadd_rn(__dadd_rn(__ddiv_rn(__dmul_rn(a.fy, yc), zc), a.cy), 0.5));
      if (!(iu >= a.u_lo && iu <= a.u_hi && iv >= a.v_lo && iv <= a.v_hi)) continue;   // false for a NaN
      // 0 <= iu <= W - 1 and 0 <= iv <= H - 1 hold here (u_lo, v_lo >= 0): the conversions are exact and in range
      const double d = (double)depth[(int64_t)f * frame_px + (int64_t)iu * a.H + (int64_t)iv];
      c += (d > 0.0 && zc <= __dadd_rn(d, a.eps)) ? 1 : 0;
    }
    views[v] += c;
  }
}

// -------------------------------------------------------------------------------------------------------- compaction
struct CullLayout { size_t used, vblk, fblk, total; int64_t nbv, nbf; };

inline CullLayout cull_layout(int64_t V, int64_t F) {
  CullLayout L;
  L.nbv = cdiv(V, CULL_WG);
  L.nbf = cdiv(F, CULL_WG);
  size_t o = 0;
  L.used = o; o += align256((size_t)(V > 0 ? V : 1));
  L.vblk = o; o += align256(sizeof(int32_t) * (size_t)(L.nbv + 1));
  L.fblk = o; o += align256(sizeof(int32_t) * (size_t)(L.nbf + 1));
  L.total = o;
  return L;
}

// whether face f stays; its corners in ia, ib, ic when it does (all three inside [0, V) then)
__device__ __forceinline__ bool face_kept(const int64_t V, const int32_t rule, const uint8_t* __restrict__ keep_v,
                                          const int32_t* __restrict__ faces, const int64_t f, int64_t& ia, int64_t& ib,
                                          int64_t& ic, bool& bad) {
  ia = faces[3 * f]; ib = faces[3 * f + 1]; ic = faces[3 * f + 2];
  bad = ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V;
  if (bad) return false;
  const bool ka = keep_v[ia] != 0, kb = keep_v[ib] != 0, kc = keep_v[ic] != 0;
  return rule == OBJNERF_CULL_ANY ? (ka || kb || kc) : (ka && kb && kc);
}

__global__ void __launch_bounds__(CULL_WG) mcl_face_kernel(const int64_t V, const int64_t F, const int32_t rule,
                                                           const uint8_t* __restrict__ keep_v,
                                                           const int32_t* __restrict__ faces, uint8_t* __restrict__ used,
                                                           int32_t* __restrict__ fblk, int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * CULL_WG + threadIdx.x;
  bool keep = false;
  if (f < F) {
    int64_t ia, ib, ic;
    bool bad;
    keep = face_kept(V, rule, keep_v, faces, f, ia, ib, ic, bad);
    if (bad) *status = CULL_BAD_INDEX;                      // (every writer stores this value)
    if (keep) { used[ia] = 1; used[ib] = 1; used[ic] = 1; }
  }
  __shared__ int wcnt[CULL_WG / 64];
  int total;
  wg_exclusive_flag<CULL_WG>(keep, wcnt, total);
  if (threadIdx.x == 0) fblk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(CULL_WG) mcl_vert_kernel(const int64_t V, const uint8_t* __restrict__ used,
                                                           int32_t* __restrict__ vblk) {
  const int64_t v = (int64_t)blockIdx.x * CULL_WG + threadIdx.x;
  __shared__ int wcnt[CULL_WG / 64];
  int total;
  wg_exclusive_flag<CULL_WG>(v < V && used[v] != 0, wcnt, total);
  if (threadIdx.x == 0) vblk[blockIdx.x] = total;
}

__global__ void mcl_totals_kernel(const int32_t* __restrict__ vtot, const int32_t* __restrict__ ftot,
                                  int64_t* __restrict__ counts) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { counts[0] = vtot ? *vtot : 0; counts[1] = ftot ? *ftot : 0; }
}

__global__ void __launch_bounds__(CULL_WG) mcl_vert_emit_kernel(const int64_t V, const int64_t Vn,
                                                                const uint8_t* __restrict__ used,
                                                                const int32_t* __restrict__ vblk,
                                                                int32_t* __restrict__ new_of_old,
                                                                int32_t* __restrict__ old_of_new) {
  const int64_t v = (int64_t)blockIdx.x * CULL_WG + threadIdx.x;
  const bool flag = v < V && used[v] != 0;
  __shared__ int wcnt[CULL_WG / 64];
  int total;
  const int64_t pos = (int64_t)vblk[blockIdx.x] + wg_exclusive_flag<CULL_WG>(flag, wcnt, total);
  const bool ok = flag && pos >= 0 && pos < Vn;
  if (v < V) new_of_old[v] = ok ? (int32_t)pos : -1;
  if (ok) old_of_new[pos] = (int32_t)v;
}

__global__ void __launch_bounds__(CULL_WG) mcl_face_emit_kernel(const int64_t V, const int64_t F, const int64_t Fn,
                                                                const int32_t rule, const uint8_t* __restrict__ keep_v,
                                                                const int32_t* __restrict__ faces,
                                                                const int32_t* __restrict__ fblk,
                                                                const int32_t* __restrict__ new_of_old,
                                                                int32_t* __restrict__ faces_out,
                                                                int32_t* __restrict__ face_old) {
  const int64_t f = (int64_t)blockIdx.x * CULL_WG + threadIdx.x;
  bool keep = false, bad;
  int64_t ia = 0, ib = 0, ic = 0;
  if (f < F) keep = face_kept(V, rule, keep_v, faces, f, ia, ib, ic, bad);
  __shared__ int wcnt[CULL_WG / 64];
  int total;
  const int64_t pos = (int64_t)fblk[blockIdx.x] + wg_exclusive_flag<CULL_WG>(keep, wcnt, total);
  if (keep && pos >= 0 && pos < Fn) {
    faces_out[3 * pos] = new_of_old[ia];
    faces_out[3 * pos + 1] = new_of_old[ib];
    faces_out[3 * pos + 2] = new_of_old[ic];
    face_old[pos] = (int32_t)f;
  }
}

inline bool cull_sizes_ok(int64_t V, int64_t F, int32_t rule) {
  return V >= 0 && V <= 0x7fffffff && F >= 0 && F <= 0x7fffffff && (rule == OBJNERF_CULL_ALL || rule == OBJNERF_CULL_ANY);
}

}  // namespace

extern "C" {

int objnerf_vertex_views(int64_t V, int32_t B, int32_t W, int32_t H, const double* verts, const double* t_cw,
                         const float* depth, double fx, double fy, double cx, double cy, double z_min, double eps,
                         int32_t margin, int32_t* views, void* stream) {
  if (V < 0 || V > 0x7fffffff || B < 0 || W <= 0 || H <= 0 || margin < 0) return OBJNERF_EINVAL;
  if (V == 0 || B == 0) return OBJNERF_OK;
  if (!verts || !t_cw || !depth || !views) return OBJNERF_EINVAL;
  VvArgs a;
  a.V = V; a.B = B; a.W = W; a.H = H;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.z_min = z_min; a.eps = eps;
  a.u_lo = (double)margin; a.u_hi = (double)((int64_t)W - 1 - margin);
  a.v_lo = (double)margin; a.v_hi = (double)((int64_t)H - 1 - margin);
  const int64_t nb = cdiv(V, CULL_WG);
  hipLaunchKernelGGL(vertex_views_kernel, dim3((unsigned)(nb < VV_GRID_CAP ? nb : VV_GRID_CAP)), dim3(CULL_WG), 0,
                     (hipStream_t)stream, a, verts, t_cw, depth, views);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

size_t objnerf_mesh_cull_workspace_bytes(int64_t V, int64_t F) {
  if (V < 0 || V > 0x7fffffff || F < 0 || F > 0x7fffffff) return 0;
  return cull_layout(V, F).total;
}

int objnerf_mesh_cull_count(int64_t V, int64_t F, int32_t rule, const uint8_t* keep_v, const int32_t* faces, void* ws,
                            size_t ws_bytes, int64_t* counts, int32_t* status, void* stream) {
  if (!cull_sizes_ok(V, F, rule) || !ws || !counts || !status || (V > 0 && !keep_v) || (F > 0 && !faces))
    return OBJNERF_EINVAL;
  const CullLayout L = cull_layout(V, F);
  if (ws_bytes < L.total) return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  uint8_t* used = (uint8_t*)(w + L.used);
  int32_t* vblk = (int32_t*)(w + L.vblk), *fblk = (int32_t*)(w + L.fblk);
  if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return OBJNERF_ELAUNCH;
  if (hipMemsetAsync(used, 0, (size_t)(V > 0 ? V : 1), st) != hipSuccess) return OBJNERF_ELAUNCH;
  const dim3 wg(CULL_WG);
  if (F > 0) {
    hipLaunchKernelGGL(mcl_face_kernel, dim3((unsigned)L.nbf), wg, 0, st, V, F, rule, keep_v, faces, used, fblk, status);
    CHECK_LAUNCH();
  }
  if (V > 0) {
    hipLaunchKernelGGL(mcl_vert_kernel, dim3((unsigned)L.nbv), wg, 0, st, V, (const uint8_t*)used, vblk);
    CHECK_LAUNCH();
  }
  // vblk[0 .. nbv) and fblk[0 .. nbf) -> exclusive offsets, the totals behind them (0 entries: the total alone)
  hipLaunchKernelGGL((wg_scan_kernel<CULL_WG, 1, int32_t>), dim3(1), wg, 0, st, vblk, L.nbv, vblk + L.nbv);
  CHECK_LAUNCH();
  hipLaunchKernelGGL((wg_scan_kernel<CULL_WG, 1, int32_t>), dim3(1), wg, 0, st, fblk, L.nbf, fblk + L.nbf);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(mcl_totals_kernel, dim3(1), dim3(64), 0, st, (const int32_t*)(vblk + L.nbv),
                     (const int32_t*)(fblk + L.nbf), counts);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_mesh_cull_emit(int64_t V, int64_t F, int32_t rule, const uint8_t* keep_v, const int32_t* faces, const void* ws,
                           size_t ws_bytes, int64_t Vn, int64_t Fn, int32_t* new_of_old, int32_t* old_of_new,
                           int32_t* faces_out, int32_t* face_old, void* stream) {
  if (!cull_sizes_ok(V, F, rule) || !ws || Vn < 0 || Vn > V || Fn < 0 || Fn > F || (V > 0 && (!keep_v || !new_of_old)) ||
      (F > 0 && !faces) || (Vn > 0 && !old_of_new) || (Fn > 0 && (!faces_out || !face_old)))
    return OBJNERF_EINVAL;
  const CullLayout L = cull_layout(V, F);
  if (ws_bytes < L.total) return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const char* w = (const char*)ws;
  const dim3 wg(CULL_WG);
  if (V > 0) {
    hipLaunchKernelGGL(mcl_vert_emit_kernel, dim3((unsigned)L.nbv), wg, 0, st, V, Vn, (const uint8_t*)(w + L.used),
                       (const int32_t*)(w + L.vblk), new_of_old, old_of_new);
    CHECK_LAUNCH();
  }
  if (F > 0 && Fn > 0) {
    hipLaunchKernelGGL(mcl_face_emit_kernel, dim3((unsigned)L.nbf), wg, 0, st, V, F, Fn, rule, keep_v, faces,
                       (const int32_t*)(w + L.fblk), (const int32_t*)new_of_old, faces_out, face_old);
    CHECK_LAUNCH();
  }
  return OBJNERF_OK;
}

}  // extern "C"
