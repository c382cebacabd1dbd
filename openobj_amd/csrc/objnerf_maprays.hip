// Ray casting over the exported map's meshes: first hit and line of sight.
//
// The result is defined WITHOUT the hierarchy (the rules stand in include/objnerf_hip.h): a face is hit iff its own padded
// fp64 box passes one slab sequence, one Moeller-Trumbore sequence accepts, and t lies in the window and not before the
// box's entry; a ray's result is the minimum of (bits((float) t) << 32 | face) over the hit faces.  Every operation rounds
// once in fp64 (the unit is compiled with -ffp-contract=off).  The hierarchy only skips nodes that provably hold no
// smaller key: a node's box contains its faces' boxes, so under the SAME slab sequence its entry is <= and its exit is >=
// theirs by the monotonicity of IEEE rounding alone.
//
//   (a) ry_code_kernel     one thread per face: validity, the padded fp64 box, the 63-bit Morton code of its centre inside
//       the scene box; an invalid face gets the largest code, so it sorts last.  (The caller sorts the codes, stably.)
//   (b) ry_leaf_kernel     one thread per leaf of `leaf` consecutive sorted faces: the slot records {face or -1, object}
//       and the leaf's box, fp64 union rounded OUTWARD to fp32.
//   (c) ry_level_kernel    one launch per level of the implicit complete tree in heap order (children 2n, 2n + 1), bottom
//       up: the union of the children and the axis on which their centres differ most.  No atomics, no workgroup waits
//       for another, every node is written: the node array has the same bytes in every run.
//   (d) ry_cast_kernel     one thread per ray.  <ANY, NEAR>: any-hit stops at the first hit; NEAR visits the nearer child
//       first (by the sign of d on the node's axis) with a 64-bit trail of pending siblings held in registers, otherwise
//       the children are visited in fixed order with the stackless successor (n + 1) >> ctz(n + 1).  No stack, no scratch.
//   (e) ry_resolve_kernel  one thread per ray: the winning face again, exactly.
// Only integer atomics (status bits, five counters a wave).
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "objnerf_segments.h"

namespace {

#define CLEAR_STALE() (void)hipGetLastError()

constexpr int RY_WG = 256;
constexpr int RY_LEAF_DEFAULT = 4;
constexpr int RY_BAD_ID = 1, RY_BAD_RAY = 2;
constexpr int RY_RAYS = 0, RY_HITS = 1, RY_BADRAYS = 2, RY_VISITS = 3, RY_TESTS = 4, RY_NSTATS = 5;
constexpr unsigned long long RY_EMPTY = ~0ull;
constexpr int RY_MODE_ANY = 1, RY_MODE_FIXED = 2;

struct RyNode { float lo[3], hi[3]; int32_t axis, zero; };   // 32 bytes; axis: bits 0-1 the split axis, bit 2: the second
                                                             // child lies on the lower side of it
struct RySlot { int32_t face, obj; };                        // face -1: never hit (a bad id or a corner that is not finite)
struct D3 { double x, y, z; };

inline int64_t ry_leaves(const int64_t F, const int leaf) { const int64_t n = cdiv(F, leaf); return n > 0 ? n : 1; }
inline int64_t ry_pow2(const int64_t n) { int64_t p = 1; while (p < n) p <<= 1; return p; }
inline size_t ry_node_bytes(const int64_t P) { return align256(sizeof(RyNode) * 2 * (size_t)P); }
inline size_t ry_slot_bytes(const int64_t F) { return align256(sizeof(RySlot) * (size_t)(F > 0 ? F : 1)); }
inline bool ry_sizes_ok(const int64_t V, const int64_t F, const int32_t S, const int32_t leaf) {
  return V >= 0 && V <= 0x7fffffff && F >= 0 && F <= 0x7fffffff && S >= 0 && S <= 65535 && leaf >= 1 &&
         (F == 0 || (S >= 1 && V >= 1));
}

// ------------------------------------------------------------------------------------------------------ device helpers
__device__ __forceinline__ bool ry_finite(const double x) { return fabs(x) <= DBL_MAX; }        // (a NaN: false)
__device__ __forceinline__ bool ry_finite3(const D3 p) { return ry_finite(p.x) && ry_finite(p.y) && ry_finite(p.z); }
__device__ __forceinline__ D3 ry_load3(const double* __restrict__ p, const int64_t i) { return D3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ double ry_min3(const double a, const double b, const double c) { return fmin(fmin(a, b), c); }
__device__ __forceinline__ double ry_max3(const double a, const double b, const double c) { return fmax(fmax(a, b), c); }

// the largest float <= x / the smallest float >= x; never a subnormal, so that no flush mode can move it inward
__device__ __forceinline__ float ry_down(const double x) {
  float f = (float)x;
  if ((double)f > x) {
    const uint32_t b = __float_as_uint(f);
    f = __uint_as_float(f > 0.0f ? b - 1u : b + 1u);
  }
  if (fabsf(f) < FLT_MIN) f = x < 0.0 ? -FLT_MIN : 0.0f;
  return f;
}
__device__ __forceinline__ float ry_up(const double x) { return -ry_down(-x); }

struct RyRay {
  D3 o, d, inv;
  bool px, py, pz;                                           // the parallel axes: inv is not finite
  double t0, t1;
};

// the slab test of the header, one axis
__device__ __forceinline__ void ry_axis(const bool par, const double o, const double inv, const double lo, const double hi,
                                        double& tn, double& tf, bool& ok) {
  if (par) {
    ok = ok && lo <= o && o <= hi;
  } else {
    const double a = __dmul_rn(__dsub_rn(lo, o), inv), b = __dmul_rn(__dsub_rn(hi, o), inv);
    tn = fmax(tn, fmin(a, b));
    tf = fmin(tf, fmax(a, b));
  }
}
__device__ __forceinline__ bool ry_slab(const RyRay& r, const D3 lo, const D3 hi, double& tn) {
  double tf = INFINITY;
  bool ok = true;
  tn = -INFINITY;
  ry_axis(r.px, r.o.x, r.inv.x, lo.x, hi.x, tn, tf, ok);
  ry_axis(r.py, r.o.y, r.inv.y, lo.y, hi.y, tn, tf, ok);
  ry_axis(r.pz, r.o.z, r.inv.z, lo.z, hi.z, tn, tf, ok);
  return ok && tn <= tf && tf >= r.t0 && tn <= r.t1;
}

__device__ __forceinline__ D3 ry_sub(const D3 a, const D3 b) { return D3{__dsub_rn(a.x, b.x), __dsub_rn(a.y, b.y), __dsub_rn(a.z, b.z)}; }
__device__ __forceinline__ D3 ry_cross(const D3 a, const D3 b) {
  return D3{__dsub_rn(__dmul_rn(a.y, b.z), __dmul_rn(a.z, b.y)), __dsub_rn(__dmul_rn(a.z, b.x), __dmul_rn(a.x, b.z)),
            __dsub_rn(__dmul_rn(a.x, b.y), __dmul_rn(a.y, b.x))};
}
__device__ __forceinline__ double ry_dot(const D3 a, const D3 b) {
  return __dadd_rn(__dadd_rn(__dmul_rn(a.x, b.x), __dmul_rn(a.y, b.y)), __dmul_rn(a.z, b.z));
}

// the Moeller-Trumbore sequence of the header: accepted?  det, U, Vv, T come back with det > 0 (neg: they were negated)
__device__ __forceinline__ bool ry_triangle(const D3 o, const D3 d, const D3 p0, const D3 e1, const D3 e2, double& det, double& U,
                                            double& Vv, double& T, bool& neg) {
  const D3 pv = ry_cross(d, e2);
  det = ry_dot(e1, pv);
  if (!(det != 0.0) || det != det) return false;
  const D3 tv = ry_sub(o, p0);
  const D3 qv = ry_cross(tv, e1);
  U = ry_dot(tv, pv); Vv = ry_dot(d, qv); T = ry_dot(e2, qv);
  neg = det < 0.0;
  if (neg) { det = -det; U = -U; Vv = -Vv; T = -T; }
  return U >= 0.0 && Vv >= 0.0 && __dadd_rn(U, Vv) <= det;
}

__device__ __forceinline__ bool ry_ids_ok(const int ia, const int ib, const int ic, const int64_t V) {
  return ia >= 0 && ia < V && ib >= 0 && ib < V && ic >= 0 && ic < V;
}

// ---------------------------------------------------------------------------------------------------------- the build
struct RyBuild {
  int64_t V, F, P; int S, leaf;
  const double* verts; const int32_t* faces; const int64_t* face_off;
  double pad; D3 blo, bhi;
  int64_t* codes; const int64_t* order; RyNode* nodes; RySlot* slots; int32_t* status;
};

// valid: the ids lie in [0, V) (else status bit 0) and the corners are finite; then [lo, hi] is the padded box
__device__ __forceinline__ bool ry_face_box(const RyBuild& a, const int64_t f, D3& lo, D3& hi) {
  const int ia = a.faces[3 * f], ib = a.faces[3 * f + 1], ic = a.faces[3 * f + 2];
  if (!ry_ids_ok(ia, ib, ic, a.V)) { atomicOr(a.status, RY_BAD_ID); return false; }
  const D3 p0 = ry_load3(a.verts, ia), p1 = ry_load3(a.verts, ib), p2 = ry_load3(a.verts, ic);
  if (!(ry_finite3(p0) && ry_finite3(p1) && ry_finite3(p2))) return false;
  lo = D3{__dsub_rn(ry_min3(p0.x, p1.x, p2.x), a.pad), __dsub_rn(ry_min3(p0.y, p1.y, p2.y), a.pad), __dsub_rn(ry_min3(p0.z, p1.z, p2.z), a.pad)};
  hi = D3{__dadd_rn(ry_max3(p0.x, p1.x, p2.x), a.pad), __dadd_rn(ry_max3(p0.y, p1.y, p2.y), a.pad), __dadd_rn(ry_max3(p0.z, p1.z, p2.z), a.pad)};
  return true;
}

// 21 bits of the centre's position inside the scene box (a NaN, a flat box: 0)
__device__ __forceinline__ unsigned long long ry_cell(const double lo, const double hi, const double blo, const double bhi) {
  const double c = __dmul_rn(__dadd_rn(lo, hi), 0.5);
  const double q = __dmul_rn(__ddiv_rn(__dsub_rn(c, blo), __dsub_rn(bhi, blo)), 2097152.0);
  return q >= 0.0 ? (q < 2097151.0 ? (unsigned long long)q : 2097151ull) : 0ull;
}
__device__ __forceinline__ unsigned long long ry_spread(unsigned long long x) {        // bit i -> bit 3 i
  x &= 0x1FFFFFull;
  x = (x | (x << 32)) & 0x1F00000000FFFFull;
  x = (x | (x << 16)) & 0x1F0000FF0000FFull;
  x = (x | (x << 8)) & 0x100F00F00F00F00Full;
  x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
  x = (x | (x << 2)) & 0x1249249249249249ull;
  return x;
}

__global__ __launch_bounds__(RY_WG) void ry_code_kernel(const RyBuild a) {
  const int64_t f = (int64_t)blockIdx.x * RY_WG + threadIdx.x;
  if (f >= a.F) return;
  D3 lo, hi;
  long long code = LLONG_MAX;
  if (ry_face_box(a, f, lo, hi))
    code = (long long)((ry_spread(ry_cell(lo.x, hi.x, a.blo.x, a.bhi.x)) << 2) | (ry_spread(ry_cell(lo.y, hi.y, a.blo.y, a.bhi.y)) << 1) |
                       ry_spread(ry_cell(lo.z, hi.z, a.blo.z, a.bhi.z)));
  a.codes[f] = code;
}

__device__ __forceinline__ RyNode ry_empty_node() {
  RyNode n;
  n.lo[0] = n.lo[1] = n.lo[2] = INFINITY; n.hi[0] = n.hi[1] = n.hi[2] = -INFINITY; n.axis = 0; n.zero = 0;
  return n;
}

__global__ __launch_bounds__(RY_WG) void ry_leaf_kernel(const RyBuild a) {
  const int64_t i = (int64_t)blockIdx.x * RY_WG + threadIdx.x;
  if (i >= a.P) return;
  if (i == 0) a.nodes[0] = ry_empty_node();                  // (never visited; written so that every byte is defined)
  D3 lo{INFINITY, INFINITY, INFINITY}, hi{-INFINITY, -INFINITY, -INFINITY};
  bool any = false;
  const int64_t s0 = i * a.leaf, s1 = s0 + a.leaf < a.F ? s0 + a.leaf : a.F;
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t f = a.order[s];
    RySlot slot{-1, 0};
    if (f >= 0 && f < a.F) {
      slot.obj = seg_of(a.face_off, a.S, f);
      D3 l, h;
      if (ry_face_box(a, f, l, h)) {
        slot.face = (int32_t)f;
        any = true;
        lo = D3{fmin(lo.x, l.x), fmin(lo.y, l.y), fmin(lo.z, l.z)};
        hi = D3{fmax(hi.x, h.x), fmax(hi.y, h.y), fmax(hi.z, h.z)};
      }
    }
    a.slots[s] = slot;
  }
  RyNode n = ry_empty_node();
  if (any) {
    n.lo[0] = ry_down(lo.x); n.lo[1] = ry_down(lo.y); n.lo[2] = ry_down(lo.z);
    n.hi[0] = ry_up(hi.x); n.hi[1] = ry_up(hi.y); n.hi[2] = ry_up(hi.z);
  }
  a.nodes[a.P + i] = n;
}

// nodes [first, first + count): the union of the two children (an empty child, +inf .. -inf, adds nothing)
__global__ __launch_bounds__(RY_WG) void ry_level_kernel(RyNode* __restrict__ nodes, const int64_t first, const int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * RY_WG + threadIdx.x;
  if (i >= count) return;
  const int64_t n = first + i;
  const RyNode l = nodes[2 * n], r = nodes[2 * n + 1];
  RyNode o;
  o.zero = 0;
  float best = -1.0f;
  int axis = 0;
  const bool both = !(l.lo[0] > l.hi[0]) && !(r.lo[0] > r.hi[0]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o.lo[k] = fminf(l.lo[k], r.lo[k]);
    o.hi[k] = fmaxf(l.hi[k], r.hi[k]);
    const float c = __fsub_rn(__fadd_rn(r.lo[k], r.hi[k]), __fadd_rn(l.lo[k], l.hi[k]));
    if (both && fabsf(c) > best) { best = fabsf(c); axis = k | (c < 0.0f ? 4 : 0); }
  }
  o.axis = axis;
  nodes[n] = o;
}

// ----------------------------------------------------------------------------------------------------------- the cast
struct RyCast {
  int64_t V, F, P, N; int S, leaf;
  const double* verts; const int32_t* faces; const uint8_t* hide; const RyNode* nodes; const RySlot* slots;
  double pad; const double* o; const double* d; double t_min, t_max; const double* t_min_ray; const double* t_max_ray;
  unsigned long long* key; uint8_t* hit; int64_t* stats; int32_t* status;
};

// the faces of one leaf against the ray; true once a hit is found in any-hit mode
template <bool ANY>
__device__ __forceinline__ bool ry_leaf(const RyCast& a, const RyRay& r, const int64_t leaf_id, unsigned long long& key, float& dbest,
                                        unsigned int& tests) {
  const int64_t s0 = leaf_id * a.leaf, s1 = s0 + a.leaf < a.F ? s0 + a.leaf : a.F;
  for (int64_t s = s0; s < s1; ++s) {
    const RySlot slot = a.slots[s];
    const int64_t f = slot.face;
    if (f < 0 || f >= a.F || slot.obj < 0 || slot.obj >= a.S) continue;
    if (a.hide[slot.obj]) continue;
    const int ia = a.faces[3 * f], ib = a.faces[3 * f + 1], ic = a.faces[3 * f + 2];
    if (!ry_ids_ok(ia, ib, ic, a.V)) continue;
    ++tests;
    const D3 p0 = ry_load3(a.verts, ia), p1 = ry_load3(a.verts, ib), p2 = ry_load3(a.verts, ic);
    const D3 lo{__dsub_rn(ry_min3(p0.x, p1.x, p2.x), a.pad), __dsub_rn(ry_min3(p0.y, p1.y, p2.y), a.pad), __dsub_rn(ry_min3(p0.z, p1.z, p2.z), a.pad)};
    const D3 hi{__dadd_rn(ry_max3(p0.x, p1.x, p2.x), a.pad), __dadd_rn(ry_max3(p0.y, p1.y, p2.y), a.pad), __dadd_rn(ry_max3(p0.z, p1.z, p2.z), a.pad)};
    double tnf;
    if (!ry_slab(r, lo, hi, tnf)) continue;                                             // gate (b)
    double det, U, Vv, T;
    bool neg;
    if (!ry_triangle(r.o, r.d, p0, ry_sub(p1, p0), ry_sub(p2, p0), det, U, Vv, T, neg)) continue;    // (c)
    const double t = __dadd_rn(__ddiv_rn(T, det), 0.0);
    if (!(r.t0 <= t && t <= r.t1 && tnf <= t)) continue;                                // gate (d)
    const float tf = (float)t;
    const unsigned long long k = ((unsigned long long)__float_as_uint(tf) << 32) | (unsigned long long)f;
    if (k < key) { key = k; dbest = tf; }
    if (ANY) return true;
  }
  return false;
}

template <bool ANY, bool NEAR>
__global__ __launch_bounds__(RY_WG) void ry_cast_kernel(const RyCast a) {
  const int64_t i = (int64_t)blockIdx.x * RY_WG + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = i < a.N;
  bool bad = false;
  unsigned long long key = RY_EMPTY;
  unsigned int visits = 0, tests = 0;
  if (live) {
    RyRay r;
    r.o = ry_load3(a.o, i); r.d = ry_load3(a.d, i);
    r.t0 = a.t_min_ray ? a.t_min_ray[i] : a.t_min;
    r.t1 = a.t_max_ray ? a.t_max_ray[i] : a.t_max;
    bad = !(ry_finite3(r.o) && ry_finite3(r.d)) || (r.d.x == 0.0 && r.d.y == 0.0 && r.d.z == 0.0);
    if (!bad) {
      r.inv = D3{__ddiv_rn(1.0, r.d.x), __ddiv_rn(1.0, r.d.y), __ddiv_rn(1.0, r.d.z)};
      r.px = !ry_finite(r.inv.x); r.py = !ry_finite(r.inv.y); r.pz = !ry_finite(r.inv.z);
      const unsigned int back = (r.d.x < 0.0 ? 1u : 0u) | (r.d.y < 0.0 ? 2u : 0u) | (r.d.z < 0.0 ? 4u : 0u);
      float dbest = INFINITY;
      unsigned long long n = 1, trail = 0;                   // trail (NEAR): bit 0 set = the sibling of n is still to visit
      const unsigned long long P = (unsigned long long)a.P;
      for (;;) {
        const float4 q0 = *(const float4*)&a.nodes[n], q1 = *((const float4*)&a.nodes[n] + 1);
        ++visits;
        bool down = false;
        if (!(q0.x > q0.w)) {                             // (an empty node: lo = +inf > hi = -inf)
          double tn;
          if (ry_slab(r, D3{(double)q0.x, (double)q0.y, (double)q0.z}, D3{(double)q0.w, (double)q1.x, (double)q1.y}, tn) &&
              !((float)tn > dbest)) {
            if (n >= P) {
              if (ry_leaf<ANY>(a, r, (int64_t)(n - P), key, dbest, tests)) break;
            } else {
              down = true;
            }
          }
        }
        if (NEAR) {
          if (down) {
            const unsigned int ax = (unsigned int)__float_as_int(q1.z);
            const unsigned int far_first = ((back >> (ax & 3u)) ^ (ax >> 2)) & 1u;
            n = 2 * n + far_first;
            trail = (trail << 1) | 1ull;
            continue;
          }
          while (!(trail & 1ull) && n != 1) { trail >>= 1; n >>= 1; }
          if (n == 1) break;
          n ^= 1ull; trail ^= 1ull;
        } else {
          if (down) { n = 2 * n; continue; }
          n = (n + 1) >> __builtin_ctzll(n + 1);             // the next node in fixed order; back at the root: done
          if (n == 1) break;
        }
      }
    }
    if (ANY) a.hit[i] = key != RY_EMPTY ? 1 : 0; else a.key[i] = key;
  }
  // every lane of the wave arrives here: one ballot and one add per counter and wave
  const unsigned long long m_live = __ballot(live), m_hit = __ballot(live && key != RY_EMPTY), m_bad = __ballot(bad);
  const unsigned long long v = wave_inclusive<unsigned long long>((unsigned long long)visits);
  const unsigned long long t = wave_inclusive<unsigned long long>((unsigned long long)tests);
  if (m_bad != 0ull && lane == 0) atomicOr(a.status, RY_BAD_RAY);
  if (lane == 63 && m_live != 0ull) {
    atomicAdd((unsigned long long*)&a.stats[RY_RAYS], (unsigned long long)__popcll(m_live));
    if (m_hit) atomicAdd((unsigned long long*)&a.stats[RY_HITS], (unsigned long long)__popcll(m_hit));
    if (m_bad) atomicAdd((unsigned long long*)&a.stats[RY_BADRAYS], (unsigned long long)__popcll(m_bad));
    if (v) atomicAdd((unsigned long long*)&a.stats[RY_VISITS], v);
    if (t) atomicAdd((unsigned long long*)&a.stats[RY_TESTS], t);
  }
}

// -------------------------------------------------------------------------------------------------------- the resolve
struct RyResolve {
  int64_t V, F, N; int S;
  const double* verts; const int32_t* faces; const int64_t* face_off; const int32_t* ids; const double* o; const double* d;
  const unsigned long long* key;
  uint8_t* hit; float* t; int32_t* face; int32_t* winner; int32_t* maskid; int32_t* vertex; double* bary; double* point; double* normal;
};

__global__ __launch_bounds__(RY_WG) void ry_resolve_kernel(const RyResolve a) {
  const int64_t i = (int64_t)blockIdx.x * RY_WG + threadIdx.x;
  if (i >= a.N) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  uint8_t o_hit = 0;
  float o_t = INFINITY;
  int32_t o_face = -1, o_winner = -1, o_mask = 0, o_vertex = -1;
  double o_b[2] = {nan, nan}, o_p[3] = {nan, nan, nan}, o_n[3] = {nan, nan, nan};
  const unsigned long long k = a.key[i];
  const int64_t f = (int64_t)(k & 0xFFFFFFFFull);
  if (k != RY_EMPTY && f < a.F) {
    const int ia = a.faces[3 * f], ib = a.faces[3 * f + 1], ic = a.faces[3 * f + 2];
    if (ry_ids_ok(ia, ib, ic, a.V)) {
      const D3 o = ry_load3(a.o, i), d = ry_load3(a.d, i);
      const D3 p0 = ry_load3(a.verts, ia), p1 = ry_load3(a.verts, ib), p2 = ry_load3(a.verts, ic);
      const D3 e1 = ry_sub(p1, p0), e2 = ry_sub(p2, p0);
      double det, U, Vv, T;
      bool neg = false;
      ry_triangle(o, d, p0, e1, e2, det, U, Vv, T, neg);
      const double t = __dadd_rn(__ddiv_rn(T, det), 0.0);
      const double u = __ddiv_rn(U, det), v = __ddiv_rn(Vv, det);
      const double w = __dsub_rn(__dsub_rn(1.0, u), v);
      const D3 nn = ry_cross(e1, e2);
      o_hit = 1;
      o_t = __uint_as_float((uint32_t)(k >> 32));
      o_face = (int32_t)f;
      o_winner = seg_of(a.face_off, a.S, f);
      o_mask = a.ids[o_winner];
      o_vertex = ia;
      double best = w;
      if (u > best) { best = u; o_vertex = ib; }
      if (v > best) { best = v; o_vertex = ic; }
      o_b[0] = u; o_b[1] = v;
      o_p[0] = __dadd_rn(o.x, __dmul_rn(t, d.x)); o_p[1] = __dadd_rn(o.y, __dmul_rn(t, d.y)); o_p[2] = __dadd_rn(o.z, __dmul_rn(t, d.z));
      o_n[0] = neg ? -nn.x : nn.x; o_n[1] = neg ? -nn.y : nn.y; o_n[2] = neg ? -nn.z : nn.z;
    }
  }
  a.hit[i] = o_hit; a.t[i] = o_t; a.face[i] = o_face; a.winner[i] = o_winner; a.maskid[i] = o_mask; a.vertex[i] = o_vertex;
  a.bary[2 * i] = o_b[0]; a.bary[2 * i + 1] = o_b[1];
#pragma unroll
  for (int c = 0; c < 3; ++c) { a.point[3 * i + c] = o_p[c]; a.normal[3 * i + c] = o_n[c]; }
}

}  // namespace

extern "C" {

size_t objnerf_rays_workspace_bytes(int64_t F, int32_t leaf) {
  if (leaf < 0) leaf = RY_LEAF_DEFAULT;
  if (F < 0 || F > 0x7fffffff || leaf < 1) return 0;
  return ry_node_bytes(ry_pow2(ry_leaves(F, leaf))) + ry_slot_bytes(F);
}

int objnerf_rays_build(int32_t stage, int64_t V, int64_t F, int32_t S, int32_t leaf, const double* verts, const int32_t* faces,
                       const int64_t* face_off, double pad, double lo_x, double lo_y, double lo_z, double hi_x, double hi_y,
                       double hi_z, int64_t* codes, const int64_t* order, void* ws, size_t ws_bytes, int32_t* status,
                       void* stream) {
  CLEAR_STALE();
  if (leaf < 0) leaf = RY_LEAF_DEFAULT;
  if (!ry_sizes_ok(V, F, S, leaf) || !(pad >= 0.0) || (stage != 1 && stage != 2)) return OBJNERF_EINVAL;
  if ((V > 0 && !verts) || (F > 0 && (!faces || !face_off)) || !status) return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  RyBuild a{V, F, ry_pow2(ry_leaves(F, leaf)), S, leaf, verts, faces, face_off, pad, {lo_x, lo_y, lo_z}, {hi_x, hi_y, hi_z},
            codes, order, nullptr, nullptr, status};
  if (stage == 1) {
    if (F > 0 && !codes) return OBJNERF_EINVAL;
    if (F > 0) {
      hipLaunchKernelGGL(ry_code_kernel, dim3((unsigned)cdiv(F, RY_WG)), dim3(RY_WG), 0, st, a);
      CHECK_LAUNCH();
    }
    return OBJNERF_OK;
  }
  if ((F > 0 && !order) || !ws || ws_bytes < objnerf_rays_workspace_bytes(F, leaf)) return OBJNERF_EINVAL;
  a.nodes = (RyNode*)ws;
  a.slots = (RySlot*)((char*)ws + ry_node_bytes(a.P));
  hipLaunchKernelGGL(ry_leaf_kernel, dim3((unsigned)cdiv(a.P, RY_WG)), dim3(RY_WG), 0, st, a);
  CHECK_LAUNCH();
  for (int64_t first = a.P >> 1; first >= 1; first >>= 1) {
    hipLaunchKernelGGL(ry_level_kernel, dim3((unsigned)cdiv(first, RY_WG)), dim3(RY_WG), 0, st, a.nodes, first, first);
    CHECK_LAUNCH();
  }
  return OBJNERF_OK;
}

int objnerf_rays_cast(int32_t mode, int64_t V, int64_t F, int32_t S, int32_t leaf, int64_t N, const double* verts,
                      const int32_t* faces, const uint8_t* hide, const void* ws, size_t ws_bytes, double pad, const double* o,
                      const double* d, double t_min, double t_max, const double* t_min_ray, const double* t_max_ray,
                      uint64_t* key, uint8_t* hit, int64_t* stats, int32_t* status, void* stream) {
  CLEAR_STALE();
  if (leaf < 0) leaf = RY_LEAF_DEFAULT;
  if (!ry_sizes_ok(V, F, S, leaf) || N < 0 || N > 0x7fffffff || !(pad >= 0.0) || mode < 0 || mode > 3 || !(t_min >= 0.0) ||
      t_max != t_max)
    return OBJNERF_EINVAL;
  const bool any = (mode & RY_MODE_ANY) != 0, fixed = (mode & RY_MODE_FIXED) != 0;
  if ((V > 0 && !verts) || (F > 0 && (!faces || !hide)) || !ws || !stats || !status || (N > 0 && (!o || !d || (any ? !hit : !key))))
    return OBJNERF_EINVAL;
  if (ws_bytes < objnerf_rays_workspace_bytes(F, leaf)) return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(stats, 0, RY_NSTATS * sizeof(int64_t), st) != hipSuccess) return OBJNERF_ELAUNCH;
  if (N == 0) return OBJNERF_OK;
  const int64_t P = ry_pow2(ry_leaves(F, leaf));
  RyCast a{V, F, P, N, S, leaf, verts, faces, hide, (const RyNode*)ws, (const RySlot*)((const char*)ws + ry_node_bytes(P)), pad, o, d,
           t_min, t_max, t_min_ray, t_max_ray, (unsigned long long*)key, hit, stats, status};
  const dim3 grid((unsigned)cdiv(N, RY_WG)), wg(RY_WG);
  if (any && fixed) hipLaunchKernelGGL((ry_cast_kernel<true, false>), grid, wg, 0, st, a);
  else if (any) hipLaunchKernelGGL((ry_cast_kernel<true, true>), grid, wg, 0, st, a);
  else if (fixed) hipLaunchKernelGGL((ry_cast_kernel<false, false>), grid, wg, 0, st, a);
  else hipLaunchKernelGGL((ry_cast_kernel<false, true>), grid, wg, 0, st, a);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_rays_resolve(int64_t V, int64_t F, int32_t S, int64_t N, const double* verts, const int32_t* faces,
                         const int64_t* face_off, const int32_t* ids, const double* o, const double* d, const uint64_t* key,
                         uint8_t* hit, float* t, int32_t* face, int32_t* winner, int32_t* maskid, int32_t* vertex, double* bary,
                         double* point, double* normal, void* stream) {
  CLEAR_STALE();
  if (!ry_sizes_ok(V, F, S, 1) || N < 0 || N > 0x7fffffff) return OBJNERF_EINVAL;
  if ((V > 0 && !verts) || (F > 0 && (!faces || !face_off || !ids))) return OBJNERF_EINVAL;
  if (N == 0) return OBJNERF_OK;
  if (!o || !d || !key || !hit || !t || !face || !winner || !maskid || !vertex || !bary || !point || !normal) return OBJNERF_EINVAL;
  RyResolve a{V, F, N, S, verts, faces, face_off, ids, o, d, (const unsigned long long*)key, hit, t, face, winner, maskid, vertex,
              bary, point, normal};
  hipLaunchKernelGGL(ry_resolve_kernel, dim3((unsigned)cdiv(N, RY_WG)), dim3(RY_WG), 0, (hipStream_t)stream, a);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

}  // extern "C"
