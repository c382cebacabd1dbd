// A rasteriser for the exported map's meshes: headless views of what MapQuery colours.
//
// The result is defined by integers (the rules stand in include/objnerf_hip.h): a vertex becomes a fixed-point screen
// position (1/256 pixel) and one fp64 inverse depth; a face covers the pixels whose three int64 edge functions are
// >= 0; per covered pixel ONE fp64 sequence gives the depth, rounded to fp32; the visibility buffer holds the minimum
// of (depth bits << 32 | face) per pixel under a 64-bit atomicMin.  The minimum does not depend on the order in which
// the faces arrive, so any schedule writes the same bytes.
//
//   (a) rs_vertex_kernel   one thread per vertex -> a 16-byte record {X, Y, iz}; a dropped vertex has X = INT_MIN and
//       Y = the reason (1: in front of z_near or NaN, 2: outside the coordinate bound).
//   (b) rs_face_kernel     one thread per face: the setup, the box clipped to the screen, the early rejection of a box
//       without a sample point (the common case on marching-cubes meshes), the small faces rasterised in the thread;
//       a larger face is appended to a list (one atomic per wave: the order of the list decides nothing).  The eight
//       counters of `stats` are summed per wave first.
//   (c) rs_large_kernel    a fixed grid of waves walks the list (its length is read on the device); a wave covers the
//       box of a face in 8 x 8 tiles.
//   (d) rs_resolve_kernel  one thread per pixel: the object by a search of face_off, the three edge functions again,
//       the images; counts with one atomic per run of equal objects in a wave.
// Only integer atomics; no workgroup waits on another.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "objnerf_segments.h"

namespace {

#define CLEAR_STALE() (void)hipGetLastError()

constexpr int RS_WG = 256;
constexpr int RS_SMALL_DEFAULT = 4;                 // a box of at most 4 x 4 pixels is rasterised by the face's thread
constexpr int RS_LARGE_WGS = 1024;                  // the large pass: at most this many workgroups of four waves
constexpr double RS_BOUND = 33554432.0;             // 2^25 (1/256 pixel): every edge function stays below 2^53
constexpr int RS_DROP_NEAR = 1, RS_DROP_BOUND = 2;
constexpr int RS_BAD_ID = 1;
// the counters of stats
constexpr int ST_SMALL = 0, ST_LARGE = 1, ST_NOSAMPLE = 2, ST_NEAR = 3, ST_BOUND = 4, ST_DEGEN = 5, ST_BADID = 6, ST_HIDDEN = 7;
constexpr unsigned long long RS_EMPTY = ~0ull;

struct RsVertex { int32_t X, Y; double iz; };       // 16 bytes

struct RsWs { RsVertex* rec; int32_t* list; unsigned int* n_large; };

inline size_t rs_align(const size_t n) { return (n + 255) / 256 * 256; }
inline size_t rs_rec_bytes(const int64_t V) { return rs_align(sizeof(RsVertex) * (size_t)(V > 0 ? V : 1)); }
inline size_t rs_list_bytes(const int64_t F) { return rs_align(sizeof(int32_t) * (size_t)(F > 0 ? F : 1)); }
inline RsWs rs_carve(void* ws, const int64_t V, const int64_t F) {
  char* p = (char*)ws;
  RsWs w;
  w.rec = (RsVertex*)p; p += rs_rec_bytes(V);
  w.list = (int32_t*)p; p += rs_list_bytes(F);
  w.n_large = (unsigned int*)p;
  return w;
}

struct RsArgs {
  int64_t V, F; int S, W, H;
  const double* verts; const int32_t* faces; const int64_t* face_off; const uint8_t* hide; const double* t_cw;
  double fx, fy, cx, cy, z_near; int small;
  RsWs ws; unsigned long long* key; int64_t* stats; int32_t* status;
};

// ---------------------------------------------------------------------------------------------------- the vertex pass
__global__ __launch_bounds__(RS_WG) void rs_vertex_kernel(const RsArgs a) {
  const int64_t v = (int64_t)blockIdx.x * RS_WG + threadIdx.x;
  if (v >= a.V) return;
  const double px = a.verts[3 * v], py = a.verts[3 * v + 1], pz = a.verts[3 * v + 2];
  const double* M = a.t_cw;
  const double xc = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M[0], px), __dmul_rn(M[1], py)), __dmul_rn(M[2], pz)), M[3]);
  const double yc = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M[4], px), __dmul_rn(M[5], py)), __dmul_rn(M[6], pz)), M[7]);
  const double zc = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M[8], px), __dmul_rn(M[9], py)), __dmul_rn(M[10], pz)), M[11]);
  const double u = __dadd_rn(__ddiv_rn(__dmul_rn(a.fx, xc), zc), a.cx);
  const double w = __dadd_rn(__ddiv_rn(__dmul_rn(a.fy, yc), zc), a.cy);
  const double X = floor(__dadd_rn(__dmul_rn(u, 256.0), 0.5));
  const double Y = floor(__dadd_rn(__dmul_rn(w, 256.0), 0.5));
  RsVertex r;
  if (!(zc >= a.z_near)) {                                  // (a NaN lands here)
    r.X = INT_MIN; r.Y = RS_DROP_NEAR; r.iz = 0.0;
  } else if (!(fabs(X) <= RS_BOUND && fabs(Y) <= RS_BOUND)) {
    r.X = INT_MIN; r.Y = RS_DROP_BOUND; r.iz = 0.0;
  } else {
    r.X = (int32_t)X; r.Y = (int32_t)Y; r.iz = __ddiv_rn(1.0, zc);
  }
  a.ws.rec[v] = r;
}

// ----------------------------------------------------------------------------------------------------- the face setup
struct RsFace {
  long long x0, y0, x1, y1, x2, y2;                          // corners 1 and 2 swapped where A < 0
  double iz0, iz1, iz2, Ad;
  int i0, i1, j0, j1;                                        // the box clipped to the screen (empty: i0 > i1 or j0 > j1)
  bool swapped;
};

__device__ __forceinline__ long long rs_edge(const long long ax, const long long ay, const long long bx, const long long by,
                                             const long long px, const long long py) {
  return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}
__device__ __forceinline__ long long rs_min3(const long long a, const long long b, const long long c) {
  return a < b ? (a < c ? a : c) : (b < c ? b : c);
}
__device__ __forceinline__ long long rs_max3(const long long a, const long long b, const long long c) {
  return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

// Why a face is not drawn, or -1 with `t` filled.  ia, ib, ic: ids already known to lie in [0, V).
__device__ __forceinline__ int rs_setup(const RsVertex* __restrict__ rec, const int ia, const int ib, const int ic, const int W,
                                        const int H, RsFace& t) {
  const RsVertex r0 = rec[ia], r1 = rec[ib], r2 = rec[ic];
  const bool d0 = r0.X == INT_MIN, d1 = r1.X == INT_MIN, d2 = r2.X == INT_MIN;
  if (d0 || d1 || d2) {
    const bool near = (d0 && r0.Y == RS_DROP_NEAR) || (d1 && r1.Y == RS_DROP_NEAR) || (d2 && r2.Y == RS_DROP_NEAR);
    return near ? ST_NEAR : ST_BOUND;
  }
  t.x0 = r0.X; t.y0 = r0.Y; t.x1 = r1.X; t.y1 = r1.Y; t.x2 = r2.X; t.y2 = r2.Y;
  t.iz0 = r0.iz; t.iz1 = r1.iz; t.iz2 = r2.iz;
  long long A = (t.x1 - t.x0) * (t.y2 - t.y0) - (t.y1 - t.y0) * (t.x2 - t.x0);
  if (A == 0) return ST_DEGEN;
  t.swapped = A < 0;
  if (t.swapped) {
    long long s = t.x1; t.x1 = t.x2; t.x2 = s;
    s = t.y1; t.y1 = t.y2; t.y2 = s;
    const double z = t.iz1; t.iz1 = t.iz2; t.iz2 = z;
    A = -A;
  }
  t.Ad = (double)A;
  // pixel i is a sample of the box iff xmin <= 256 i <= xmax  (>> 8 of a negative value rounds down)
  const long long xa = rs_min3(t.x0, t.x1, t.x2), xb = rs_max3(t.x0, t.x1, t.x2);
  const long long ya = rs_min3(t.y0, t.y1, t.y2), yb = rs_max3(t.y0, t.y1, t.y2);
  const long long i0 = (xa + 255) >> 8, i1 = xb >> 8, j0 = (ya + 255) >> 8, j1 = yb >> 8;
  t.i0 = (int)(i0 < 0 ? 0 : i0); t.i1 = (int)(i1 > W - 1 ? W - 1 : i1);
  t.j0 = (int)(j0 < 0 ? 0 : j0); t.j1 = (int)(j1 > H - 1 ? H - 1 : j1);
  return -1;
}

// the three edge functions of pixel (i, j); covered iff all are >= 0
__device__ __forceinline__ bool rs_cover(const RsFace& t, const int i, const int j, long long& w0, long long& w1, long long& w2) {
  const long long px = 256ll * i, py = 256ll * j;
  w0 = rs_edge(t.x1, t.y1, t.x2, t.y2, px, py);
  w1 = rs_edge(t.x2, t.y2, t.x0, t.y0, px, py);
  w2 = rs_edge(t.x0, t.y0, t.x1, t.y1, px, py);
  return (w0 | w1 | w2) >= 0;
}

// q = ((w0 iz0) + (w1 iz1)) + (w2 iz2), the products left in t0..t2
__device__ __forceinline__ double rs_q(const RsFace& t, const long long w0, const long long w1, const long long w2, double& t0,
                                       double& t1, double& t2) {
  t0 = __dmul_rn((double)w0, t.iz0); t1 = __dmul_rn((double)w1, t.iz1); t2 = __dmul_rn((double)w2, t.iz2);
  return __dadd_rn(__dadd_rn(t0, t1), t2);
}

__device__ __forceinline__ void rs_paint(const RsFace& t, const int i, const int j, const int H, const uint32_t f,
                                         unsigned long long* __restrict__ key) {
  long long w0, w1, w2;
  if (!rs_cover(t, i, j, w0, w1, w2)) return;
  double t0, t1, t2;
  const double q = rs_q(t, w0, w1, w2, t0, t1, t2);
  const float d = (float)__ddiv_rn(t.Ad, q);
  const unsigned long long k = ((unsigned long long)__float_as_uint(d) << 32) | f;
  unsigned long long* slot = key + ((int64_t)i * H + j);
  // (the read only spares atomics: a slot only ever decreases, so a stale value is larger and the atomic still decides)
  if (k < __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMin(slot, k);
}

// ------------------------------------------------------------------------------------------------------ the face pass
__global__ __launch_bounds__(RS_WG) void rs_face_kernel(const RsArgs a) {
  const int64_t f = (int64_t)blockIdx.x * RS_WG + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int cat = -1;                                             // the counter this face adds to; -1: no face
  bool large = false;
  if (f < a.F) {
    const int ia = a.faces[3 * f], ib = a.faces[3 * f + 1], ic = a.faces[3 * f + 2];
    if (ia < 0 || ia >= a.V || ib < 0 || ib >= a.V || ic < 0 || ic >= a.V) {
      atomicOr(a.status, RS_BAD_ID);
      cat = ST_BADID;
    } else if (a.hide[seg_of(a.face_off, a.S, f)]) {
      cat = ST_HIDDEN;
    } else {
      RsFace t;
      cat = rs_setup(a.ws.rec, ia, ib, ic, a.W, a.H, t);
      if (cat < 0) {
        if (t.i0 > t.i1 || t.j0 > t.j1) {
          cat = ST_NOSAMPLE;
        } else if (t.i1 - t.i0 < a.small && t.j1 - t.j0 < a.small) {
          cat = ST_SMALL;
          for (int i = t.i0; i <= t.i1; ++i)
            for (int j = t.j0; j <= t.j1; ++j) rs_paint(t, i, j, a.H, (uint32_t)f, a.key);
        } else {
          cat = ST_LARGE;
          large = true;
        }
      }
    }
  }
  // every lane of the wave arrives here
  const unsigned long long m = __ballot(large);
  if (m != 0ull) {
    const int leader = __ffsll((long long)m) - 1;
    unsigned int base = 0;
    if (lane == leader) base = atomicAdd(a.ws.n_large, (unsigned int)__popcll(m));
    base = __shfl(base, leader);
    if (large) {
      const unsigned int pos = base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
      if (pos < (unsigned long long)a.F) a.ws.list[pos] = (int32_t)f;
    }
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const unsigned long long b = __ballot(cat == c);
    if (lane == 0 && b != 0ull) atomicAdd((unsigned long long*)&a.stats[c], (unsigned long long)__popcll(b));
  }
}

// ------------------------------------------------------------------------------------------------- the large-face pass
__global__ __launch_bounds__(RS_WG) void rs_large_kernel(const RsArgs a) {
  const int lane = threadIdx.x & 63;
  const unsigned int n_raw = *a.ws.n_large;
  const unsigned int n = n_raw < (unsigned long long)a.F ? n_raw : (unsigned int)a.F;
  const unsigned int waves = gridDim.x * (RS_WG / 64);
  for (unsigned int e = blockIdx.x * (RS_WG / 64) + (threadIdx.x >> 6); e < n; e += waves) {
    const int64_t f = a.ws.list[e];
    if (f < 0 || f >= a.F) continue;                        // (uniform over the wave)
    const int ia = a.faces[3 * f], ib = a.faces[3 * f + 1], ic = a.faces[3 * f + 2];
    if (ia < 0 || ia >= a.V || ib < 0 || ib >= a.V || ic < 0 || ic >= a.V) continue;
    RsFace t;
    if (rs_setup(a.ws.rec, ia, ib, ic, a.W, a.H, t) >= 0) continue;
    const int di = lane >> 3, dj = lane & 7;
    for (int ti = t.i0; ti <= t.i1; ti += 8)
      for (int tj = t.j0; tj <= t.j1; tj += 8) {
        const int i = ti + di, j = tj + dj;
        if (i <= t.i1 && j <= t.j1) rs_paint(t, i, j, a.H, (uint32_t)f, a.key);
      }
  }
}

// ---------------------------------------------------------------------------------------------------- the resolve pass
struct RsResolve {
  int64_t V, F; int S, W, H;
  const double* verts; const int32_t* faces; const int64_t* face_off; const int32_t* ids; const float* colors;
  const RsVertex* rec; const unsigned long long* key;
  double cam[3], ambient; int shade; uint8_t bg[3];
  uint8_t* rgb; int32_t* maskid; float* depth; int32_t* winner; int32_t* face; int32_t* vertex; int64_t* counts;
};

__device__ __forceinline__ uint8_t rs_quant(const double c) {
  const double x = c >= 0.0 ? (c <= 1.0 ? c : 1.0) : 0.0;    // (a NaN counts as 0)
  return (uint8_t)floor(__dadd_rn(__dmul_rn(x, 255.0), 0.5));
}

// ambient + (1 - ambient) |n . d| / (|n| |d|) of the face (ia, ib, ic) in its own corner order; 1 where |n| |d| is not > 0
__device__ __forceinline__ double rs_shade(const RsResolve& a, const int ia, const int ib, const int ic) {
  const double* A = a.verts + 3 * (int64_t)ia, *B = a.verts + 3 * (int64_t)ib, *Cc = a.verts + 3 * (int64_t)ic;
  double e1[3], e2[3], d[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    e1[c] = __dsub_rn(B[c], A[c]); e2[c] = __dsub_rn(Cc[c], A[c]);
    d[c] = __dsub_rn(__ddiv_rn(__dadd_rn(__dadd_rn(A[c], B[c]), Cc[c]), 3.0), a.cam[c]);
  }
  const double n[3] = {__dsub_rn(__dmul_rn(e1[1], e2[2]), __dmul_rn(e1[2], e2[1])),
                       __dsub_rn(__dmul_rn(e1[2], e2[0]), __dmul_rn(e1[0], e2[2])),
                       __dsub_rn(__dmul_rn(e1[0], e2[1]), __dmul_rn(e1[1], e2[0]))};
  const double dot = __dadd_rn(__dadd_rn(__dmul_rn(n[0], d[0]), __dmul_rn(n[1], d[1])), __dmul_rn(n[2], d[2]));
  const double nn = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(n[0], n[0]), __dmul_rn(n[1], n[1])), __dmul_rn(n[2], n[2])));
  const double dd = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(d[0], d[0]), __dmul_rn(d[1], d[1])), __dmul_rn(d[2], d[2])));
  const double den = __dmul_rn(nn, dd);
  if (!(den > 0.0)) return 1.0;
  return __dadd_rn(a.ambient, __dmul_rn(__dsub_rn(1.0, a.ambient), __ddiv_rn(fabs(dot), den)));
}

__global__ __launch_bounds__(RS_WG) void rs_resolve_kernel(const RsResolve a) {
  const int64_t P = (int64_t)a.W * a.H;
  const int64_t p = (int64_t)blockIdx.x * RS_WG + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int s = -1;
  if (p < P) {
    int32_t o_face = -1, o_vertex = -1, o_mask = 0;
    float o_depth = 100.0f;
    uint8_t o_rgb[3] = {a.bg[0], a.bg[1], a.bg[2]};
    const unsigned long long k = a.key[p];
    const int64_t f = (int64_t)(k & 0xFFFFFFFFull);
    if (k != RS_EMPTY && f < a.F) {
      const int ia = a.faces[3 * f], ib = a.faces[3 * f + 1], ic = a.faces[3 * f + 2];
      RsFace t;
      if (ia >= 0 && ia < a.V && ib >= 0 && ib < a.V && ic >= 0 && ic < a.V && rs_setup(a.rec, ia, ib, ic, a.W, a.H, t) < 0) {
        s = seg_of(a.face_off, a.S, f);
        const int i = (int)(p / a.H), j = (int)(p % a.H);
        long long w0, w1, w2;
        rs_cover(t, i, j, w0, w1, w2);
        double t0, t1, t2;
        const double q = rs_q(t, w0, w1, w2, t0, t1, t2);
        const int c1 = t.swapped ? ic : ib, c2 = t.swapped ? ib : ic;     // the corners in the swapped order
        o_face = (int32_t)f;
        o_mask = a.ids[s];
        o_depth = __uint_as_float((uint32_t)(k >> 32));
        o_vertex = ia;
        double best = t0;
        if (t1 > best) { best = t1; o_vertex = c1; }
        if (t2 > best) { best = t2; o_vertex = c2; }
        const double b0 = __ddiv_rn(t0, q), b1 = __ddiv_rn(t1, q), b2 = __ddiv_rn(t2, q);
        const double sh = a.shade ? rs_shade(a, ia, ib, ic) : 1.0;
        const float* k0 = a.colors + 3 * (int64_t)ia, *k1 = a.colors + 3 * (int64_t)c1, *k2 = a.colors + 3 * (int64_t)c2;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double col = __dadd_rn(__dadd_rn(__dmul_rn(b0, (double)k0[c]), __dmul_rn(b1, (double)k1[c])),
                                       __dmul_rn(b2, (double)k2[c]));
          o_rgb[c] = rs_quant(a.shade ? __dmul_rn(col, sh) : col);
        }
      }
    }
    a.rgb[3 * p] = o_rgb[0]; a.rgb[3 * p + 1] = o_rgb[1]; a.rgb[3 * p + 2] = o_rgb[2];
    a.maskid[p] = o_mask; a.depth[p] = o_depth; a.winner[p] = s; a.face[p] = o_face; a.vertex[p] = o_vertex;
  }
  // counts: one atomic per run of equal objects over lane order (every lane of the wave arrives here)
  const int prev = __shfl_up(s, 1);
  const unsigned long long heads = __ballot(lane == 0 || prev != s);
  if (s >= 0 && ((heads >> lane) & 1ull)) {
    const unsigned long long later = lane == 63 ? 0ull : (heads >> (lane + 1));
    const int len = later ? __ffsll((long long)later) : 64 - lane;
    atomicAdd((unsigned long long*)&a.counts[s], (unsigned long long)len);
  }
}

inline bool rs_sizes_ok(const int64_t V, const int64_t F, const int32_t S, const int32_t W, const int32_t H) {
  return V >= 0 && V <= 0x7fffffff && F >= 0 && F <= 0x7fffffff && S >= 0 && S <= 65535 && W >= 1 && W <= 65536 && H >= 1 &&
         H <= 65536 && (int64_t)W * H <= 0x7fffffff && (F == 0 || (S >= 1 && V >= 1));
}

}  // namespace

extern "C" {

size_t objnerf_raster_workspace_bytes(int64_t V, int64_t F) {
  if (V < 0 || V > 0x7fffffff || F < 0 || F > 0x7fffffff) return 0;
  return rs_rec_bytes(V) + rs_list_bytes(F) + 256;
}

int objnerf_raster_visibility(int64_t V, int64_t F, int32_t S, int32_t W, int32_t H, const double* verts,
                              const int32_t* faces, const int64_t* face_off, const uint8_t* hide, const double* t_cw,
                              double fx, double fy, double cx, double cy, double z_near, int32_t small_box,
                              int32_t passes, void* ws, size_t ws_bytes, uint64_t* key, int64_t* stats, int32_t* status, void* stream) {
  CLEAR_STALE();
  if (!rs_sizes_ok(V, F, S, W, H) || !(z_near > 0.0) || passes < 0 || passes > 7) return OBJNERF_EINVAL;
  if (passes == 0) passes = 7;
  if ((V > 0 && !verts) || (F > 0 && (!faces || !face_off || !hide)) || !t_cw || !ws || !key || !stats || !status)
    return OBJNERF_EINVAL;
  if (ws_bytes < objnerf_raster_workspace_bytes(V, F)) return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  RsArgs a{V, F, S, W, H, verts, faces, face_off, hide, t_cw, fx, fy, cx, cy, z_near,
           small_box < 0 ? RS_SMALL_DEFAULT : small_box, rs_carve(ws, V, F), (unsigned long long*)key, stats, status};
  if (passes & 2) {
    if (hipMemsetAsync(key, 0xFF, sizeof(uint64_t) * (size_t)W * H, st) != hipSuccess) return OBJNERF_ELAUNCH;
    if (hipMemsetAsync(stats, 0, 8 * sizeof(int64_t), st) != hipSuccess) return OBJNERF_ELAUNCH;
    if (hipMemsetAsync(a.ws.n_large, 0, sizeof(unsigned int), st) != hipSuccess) return OBJNERF_ELAUNCH;
  }
  if (V > 0 && (passes & 1)) {
    hipLaunchKernelGGL(rs_vertex_kernel, dim3((unsigned)cdiv(V, RS_WG)), dim3(RS_WG), 0, st, a);
    CHECK_LAUNCH();
  }
  if (F > 0 && (passes & 2)) {
    hipLaunchKernelGGL(rs_face_kernel, dim3((unsigned)cdiv(F, RS_WG)), dim3(RS_WG), 0, st, a);
    CHECK_LAUNCH();
  }
  if (F > 0 && (passes & 4)) {
    const int64_t wgs = cdiv(F, RS_WG / 64);
    hipLaunchKernelGGL(rs_large_kernel, dim3((unsigned)(wgs < RS_LARGE_WGS ? wgs : RS_LARGE_WGS)), dim3(RS_WG), 0, st, a);
    CHECK_LAUNCH();
  }
  return OBJNERF_OK;
}

int objnerf_raster_resolve(int64_t V, int64_t F, int32_t S, int32_t W, int32_t H, const double* verts,
                           const int32_t* faces, const int64_t* face_off, const int32_t* ids, const float* colors,
                           const void* ws, size_t ws_bytes, const uint64_t* key, double cam_x, double cam_y, double cam_z,
                           double ambient, int32_t shading, int32_t background, uint8_t* rgb, int32_t* maskid, float* depth,
                           int32_t* winner, int32_t* face, int32_t* vertex, int64_t* counts, void* stream) {
  CLEAR_STALE();
  if (!rs_sizes_ok(V, F, S, W, H) || shading < 0 || shading > 1 || !(ambient >= 0.0 && ambient <= 1.0)) return OBJNERF_EINVAL;
  if ((V > 0 && (!verts || !colors)) || (F > 0 && (!faces || !face_off || !ids)) || !ws || !key || !rgb || !maskid || !depth ||
      !winner || !face || !vertex || (S > 0 && !counts))
    return OBJNERF_EINVAL;
  if (ws_bytes < objnerf_raster_workspace_bytes(V, F)) return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  RsResolve a{V, F, S, W, H, verts, faces, face_off, ids, colors, rs_carve((void*)ws, V, F).rec,
              (const unsigned long long*)key, {cam_x, cam_y, cam_z}, ambient, shading,
              {(uint8_t)((background >> 16) & 255), (uint8_t)((background >> 8) & 255), (uint8_t)(background & 255)},
              rgb, maskid, depth, winner, face, vertex, counts};
  if (S > 0 && hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)S, st) != hipSuccess) return OBJNERF_ELAUNCH;
  hipLaunchKernelGGL(rs_resolve_kernel, dim3((unsigned)cdiv((int64_t)W * H, RS_WG)), dim3(RS_WG), 0, st, a);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

}  // extern "C"
