// A navigation volume of the map (gfx950): an axis-aligned voxel grid labelled through MapPoints, and three integer passes
// over it -- the exact Euclidean distance to the nearest occupied voxel, the shortest 26-connected path cost from a start
// voxel, the closest reachable voxel to every object -- plus the walk back along a path (openobj_amd/map_volume.py,
// DESIGN.md 4.29).  idx = (z * ny + y) * nx + x; label >= 0 is OCCUPIED.
//
//   mv_centres_kernel   the fp32 centres of a slab of z-planes, origin + (float(i) + 0.5f) * voxel: one multiply, one add
//                       (the unit is built with contraction off), so numpy fp32 gives the same bits.
//   mv_project_kernel   one axis collapsed: the label of the first occupied voxel of every column.
//   mv_edt_x_kernel / mv_edt_axis_kernel   the distance transform, one pass per axis.  A voxel carries ONE 64-bit key,
//                       dist2 << 32 | site (site = the linear index of an occupied voxel), absent = INT32_MAX << 32 | ~0.
//                       A pass takes, per output, the minimum over the line of key + (d * d << 32): the lexicographic
//                       minimum of (partial dist2, site).  Brute force over the line, the sources staged through LDS in
//                       chunks of 64; a chunk without a site is skipped.  Lines along y and z are taken 32 x-columns at a
//                       time, so every global access runs along x.
//   mv_reach_kernel     one relaxation round of the path cost: an ACTIVE 8 x 8 x 8 tile loads itself and its halo into LDS,
//                       relaxes there until nothing changes, writes what dropped with atomicMin and flags the tiles whose
//                       halo it changed for the next round.  No workgroup waits for another.
//   mv_goals_kernel     one 64-bit atomicMin of dist2 << 32 | idx per (wave, object) into a K-row table.
//   mv_paths_kernel     one wave per goal walks back to the start; the 26 lanes test the 26 neighbours, the first wins.
//
// Every value is an integer and every reduction is a minimum over keys that no two candidates share, so the volumes are the
// same bytes whatever the schedule.
#include "objnerf_wg.h"

namespace {

typedef unsigned long long u64;
constexpr u64 MV_ABSENT = ((u64)0x7FFFFFFFu << 32) | 0xFFFFFFFFu;
constexpr uint32_t MV_INF = 0xFFFFFFFFu;
constexpr int MV_MAX_AXIS = 1024;

inline bool mv_dims_ok(const int32_t nx, const int32_t ny, const int32_t nz) {
  return nx >= 1 && ny >= 1 && nz >= 1 && nx <= MV_MAX_AXIS && ny <= MV_MAX_AXIS && nz <= MV_MAX_AXIS &&
         (int64_t)nx * ny * nz <= 0x7fffffffLL;
}

// ---------------------------------------------------------------------------------------------------------- centres
__global__ void __launch_bounds__(256) mv_centres_kernel(const int nx, const int ny, const int z0, const int64_t n,
                                                         const float ox, const float oy, const float oz, const float voxel,
                                                         float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % nx);
  const int64_t r = i / nx;
  const int y = (int)(r % ny), z = z0 + (int)(r / ny);
  out[3 * i] = ox + ((float)x + 0.5f) * voxel;
  out[3 * i + 1] = oy + ((float)y + 0.5f) * voxel;
  out[3 * i + 2] = oz + ((float)z + 0.5f) * voxel;
}

// ---------------------------------------------------------------------------------------------------------- project
// out [n_out]: the output voxel o sits at base(o) in the input; its column runs nA voxels of stride sA from there
__global__ void __launch_bounds__(256) mv_project_kernel(const int nx, const int ny, const int nz, const int axis,
                                                         const int32_t* __restrict__ label, int32_t* __restrict__ out) {
  const int ox = axis == 0 ? 1 : nx, oy = axis == 1 ? 1 : ny, oz = axis == 2 ? 1 : nz;
  const int64_t n = (int64_t)ox * oy * oz, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % ox), y = (int)((i / ox) % oy), z = (int)(i / ((int64_t)ox * oy));
  const int64_t base = ((int64_t)z * ny + y) * nx + x;
  const int nA = axis == 0 ? nx : axis == 1 ? ny : nz;
  const int64_t sA = axis == 0 ? 1 : axis == 1 ? nx : (int64_t)nx * ny;
  int32_t l = -1;
  for (int a = 0; a < nA && l < 0; ++a) l = label[base + a * sA];
  out[i] = l < 0 ? -1 : l;
}

// -------------------------------------------------------------------------------------------- the distance transform
__device__ __forceinline__ u64 mv_offer(const u64 best, const u64 k, const int d) {
  const u64 cand = k == MV_ABSENT ? MV_ABSENT : k + ((u64)(uint32_t)(d * d) << 32);
  return cand < best ? cand : best;
}

// along x, from the labels: a wave owns one line and 64 outputs of it; its sources go through the wave's own LDS row
__global__ void __launch_bounds__(256) mv_edt_x_kernel(const int nx, const int64_t nlines, const int segs,
                                                       const int32_t* __restrict__ label, int32_t* __restrict__ d_out,
                                                       int32_t* __restrict__ s_out) {
  __shared__ u64 src[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = (int)(blockIdx.x % segs);
  const int64_t line = (int64_t)(blockIdx.x / segs) * 4 + wave;
  const bool lvalid = line < nlines;
  const int x = seg * 64 + lane;
  u64 best = MV_ABSENT;
  for (int c0 = 0; c0 < nx; c0 += 64) {
    __syncthreads();
    const int sx = c0 + lane;
    u64 k = MV_ABSENT;
    if (lvalid && sx < nx) {
      const int64_t idx = line * nx + sx;
      if (label[idx] >= 0) k = (u64)(uint32_t)idx;
    }
    src[wave][lane] = k;
    __syncthreads();
    if (__ballot(k != MV_ABSENT) == 0ull) continue;         // (the row is this wave's own: the decision is per wave)
    const int m = nx - c0 < 64 ? nx - c0 : 64;
    for (int j = 0; j < m; ++j) best = mv_offer(best, src[wave][j], x - (c0 + j));
  }
  if (lvalid && x < nx) {
    d_out[line * nx + x] = (int32_t)(best >> 32);
    s_out[line * nx + x] = (int32_t)(uint32_t)best;
  }
}

// along y or z, from the keys of the pass before: a workgroup owns 32 x-columns and 32 outputs along the axis (thread
// (tx, ty) the outputs a0 + ty + 8 i), and reads the whole line of its columns in chunks of 64
constexpr int MV_EX = 32, MV_EA = 32, MV_CH = 64;
__global__ void __launch_bounds__(256) mv_edt_axis_kernel(const int nx, const int nA, const int64_t sA, const int nB,
                                                          const int64_t sB, const int nxt, const int nat,
                                                          const int32_t* __restrict__ d_in, const int32_t* __restrict__ s_in,
                                                          int32_t* __restrict__ d_out, int32_t* __restrict__ s_out) {
  __shared__ u64 src[MV_CH][MV_EX];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int xt = (int)(blockIdx.x % nxt);
  const int64_t r = blockIdx.x / nxt;
  const int at = (int)(r % nat), b = (int)(r / nat);
  const int x = xt * MV_EX + tx, a0 = at * MV_EA;
  const int64_t base = (int64_t)b * sB + x;
  u64 best[4] = {MV_ABSENT, MV_ABSENT, MV_ABSENT, MV_ABSENT};
  for (int c0 = 0; c0 < nA; c0 += MV_CH) {
    __syncthreads();
    int any = 0;
    for (int rr = ty; rr < MV_CH; rr += 8) {
      const int sa = c0 + rr;
      u64 k = MV_ABSENT;
      if (x < nx && sa < nA) {
        const int64_t idx = base + (int64_t)sa * sA;
        const int32_t s = s_in[idx];
        if (s >= 0) k = ((u64)(uint32_t)d_in[idx] << 32) | (uint32_t)s;
      }
      src[rr][tx] = k;
      any |= k != MV_ABSENT;
    }
    if (!__syncthreads_or(any)) continue;                   // (the same answer in every thread)
    const int m = nA - c0 < MV_CH ? nA - c0 : MV_CH;
    for (int j = 0; j < m; ++j) {
      const u64 k = src[j][tx];
#pragma unroll
      for (int i = 0; i < 4; ++i) best[i] = mv_offer(best[i], k, a0 + ty + 8 * i - (c0 + j));
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int a = a0 + ty + 8 * i;
    if (x < nx && a < nA) {
      d_out[base + (int64_t)a * sA] = (int32_t)(best[i] >> 32);
      s_out[base + (int64_t)a * sA] = (int32_t)(uint32_t)best[i];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ reach
constexpr int MV_RT = 8, MV_RH = MV_RT + 2, MV_RCELLS = MV_RH * MV_RH * MV_RH, MV_RWG = MV_RT * MV_RT * MV_RT;
// a cost chain inside a tile visits each of its voxels once at the most: after MV_RWG sweeps nothing can change
constexpr int MV_RSWEEPS = MV_RWG + 1;

__device__ __forceinline__ bool mv_traversable(const int32_t* __restrict__ label, const int32_t* __restrict__ dist2,
                                               const int32_t r2, const int64_t idx) {
  return label[idx] < 0 && dist2[idx] >= r2;
}

__global__ void __launch_bounds__(MV_RWG) mv_reach_kernel(const int nx, const int ny, const int nz, const int ntx,
                                                          const int nty, const int ntz, const int32_t* __restrict__ label,
                                                          const int32_t* __restrict__ dist2, const int32_t r2,
                                                          uint32_t* cost, int32_t* act_in, int32_t* act_out, int32_t* changed) {
  __shared__ uint32_t c[MV_RCELLS];
  __shared__ int s_act;
  const int t = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_act = act_in[t];
  __syncthreads();
  if (!s_act) return;                                       // (the same word in every thread: read once, through LDS)
  if (tid == 0) act_in[t] = 0;                              // this buffer is the next round's output: left clean
  const int tcx = t % ntx, tcy = (t / ntx) % nty, tcz = t / (ntx * nty);
  const int x0 = tcx * MV_RT, y0 = tcy * MV_RT, z0 = tcz * MV_RT;
  for (int i = tid; i < MV_RCELLS; i += MV_RWG) {
    const int gx = x0 + i % MV_RH - 1, gy = y0 + (i / MV_RH) % MV_RH - 1, gz = z0 + i / (MV_RH * MV_RH) - 1;
    uint32_t v = MV_INF;
    if (gx >= 0 && gy >= 0 && gz >= 0 && gx < nx && gy < ny && gz < nz) {
      const int64_t idx = ((int64_t)gz * ny + gy) * nx + gx;
      if (mv_traversable(label, dist2, r2, idx)) v = cost[idx];
    }
    c[i] = v;                                               // an obstacle or a voxel outside the grid offers nothing
  }
  __syncthreads();
  const int lx = tid & 7, ly = (tid >> 3) & 7, lz = tid >> 6;
  const int li = ((lz + 1) * MV_RH + ly + 1) * MV_RH + lx + 1;
  const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
  const bool inside = gx < nx && gy < ny && gz < nz;
  const int64_t idx = ((int64_t)gz * ny + gy) * nx + gx;
  const bool trav = inside && mv_traversable(label, dist2, r2, idx);
  uint32_t mine = c[li];
  const uint32_t first = mine;
  bool stable = false;
  for (int sweep = 0; sweep < MV_RSWEEPS; ++sweep) {
    uint32_t best = mine;
    if (trav) {
#pragma unroll
      for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            if (dx == 0 && dy == 0 && dz == 0) continue;
            const uint32_t v = c[li + (dz * MV_RH + dy) * MV_RH + dx];
            const uint32_t w = 2u + (dx != 0) + (dy != 0) + (dz != 0);
            // (the host admits only grids whose largest possible cost stays below MV_INF - 5)
            if (v != MV_INF && v + w < best) best = v + w;
          }
    }
    const int dropped = best < mine;
    __syncthreads();                                        // every read of this sweep before any write
    if (dropped) { mine = best; c[li] = best; }
    if (!__syncthreads_or(dropped)) { stable = true; break; }
  }
  if (!stable && tid == 0) { act_out[t] = 1; *changed = 1; }     // unreachable by the bound above; never a wrong volume
  if (mine < first) {
    atomicMin(cost + idx, mine);
    *changed = 1;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int ox = lx + dx < 0 ? -1 : lx + dx >= MV_RT ? 1 : 0, oy = ly + dy < 0 ? -1 : ly + dy >= MV_RT ? 1 : 0,
                    oz = lz + dz < 0 ? -1 : lz + dz >= MV_RT ? 1 : 0;
          if (ox == 0 && oy == 0 && oz == 0) continue;
          const int ux = tcx + ox, uy = tcy + oy, uz = tcz + oz;
          if (ux >= 0 && uy >= 0 && uz >= 0 && ux < ntx && uy < nty && uz < ntz) act_out[(uz * nty + uy) * ntx + ux] = 1;
        }
  }
}

// ------------------------------------------------------------------------------------------------------------ goals
__global__ void __launch_bounds__(256) mv_goals_kernel(const int64_t n, const int K, const int32_t* __restrict__ label,
                                                       const int32_t* __restrict__ dist2, const int32_t* __restrict__ site,
                                                       const uint32_t* __restrict__ cost, const int32_t r2,
                                                       u64* __restrict__ table) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int k = -1;
  u64 key = ~0ull;
  if (u < n && label[u] < 0 && dist2[u] >= r2 && cost[u] != MV_INF && site[u] >= 0) {
    k = label[site[u]];
    key = ((u64)(uint32_t)dist2[u] << 32) | (uint32_t)u;
  }
  bool pending = k >= 0 && k < K;
  // the lanes of a wave that share an object hand in one minimum: every turn retires its leader, 64 turns at the most
  for (int turn = 0; turn < 64; ++turn) {
    const u64 bal = __ballot(pending);
    if (bal == 0ull) break;
    const int leader = __ffsll((long long)bal) - 1;
    const int kk = __shfl(k, leader);
    const bool mine = pending && k == kk;
    u64 v = mine ? key : ~0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const u64 w = __shfl_xor(v, o);
      v = w < v ? w : v;
    }
    if (lane == leader) atomicMin(table + kk, v);
    pending = pending && !mine;
  }
}

// ------------------------------------------------------------------------------------------------------------ paths
// neighbour n = 0 .. 25: the offsets (dz, dy, dx) in {-1, 0, 1}^3 in lexicographic order, dz slowest, without the centre
__global__ void __launch_bounds__(64) mv_paths_kernel(const int nx, const int ny, const int nz,
                                                      const int32_t* __restrict__ label, const int32_t* __restrict__ dist2,
                                                      const int32_t r2, const uint32_t* __restrict__ cost,
                                                      const int32_t* __restrict__ goals, const int32_t cap,
                                                      int32_t* __restrict__ out, int32_t* __restrict__ len) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const int64_t nvox = (int64_t)nx * ny * nz;
  int32_t u = goals[g];
  int64_t n = 0;
  if (u >= 0 && u < nvox && cost[u] != MV_INF && mv_traversable(label, dist2, r2, u)) {
    uint32_t cu = cost[u];
    const uint32_t max_steps = cu / 3u + 1u;
    if (lane == 0 && n < cap) out[(int64_t)g * cap + n] = u;
    n = 1;
    for (uint32_t step = 0; step < max_steps && cu != 0u; ++step) {
      bool ok = false;
      int32_t v = -1;
      uint32_t cv = MV_INF;
      if (lane < 26) {
        const int o = lane < 13 ? lane : lane + 1;
        const int dx = o % 3 - 1, dy = (o / 3) % 3 - 1, dz = o / 9 - 1;
        const int x = u % nx + dx, y = (u / nx) % ny + dy, z = u / (nx * ny) + dz;
        if (x >= 0 && y >= 0 && z >= 0 && x < nx && y < ny && z < nz) {
          v = (int32_t)(((int64_t)z * ny + y) * nx + x);
          cv = cost[v];
          const uint32_t w = 2u + (dx != 0) + (dy != 0) + (dz != 0);
          ok = cv != MV_INF && mv_traversable(label, dist2, r2, v) && cv + w == cu;
        }
      }
      const u64 bal = __ballot(ok);
      if (bal == 0ull) break;                               // not a volume reach() wrote: the walk ends where it stands
      const int first = __ffsll((long long)bal) - 1;
      u = __shfl(v, first);
      cu = __shfl(cv, first);
      if (lane == 0 && n < cap) out[(int64_t)g * cap + n] = u;
      ++n;
    }
  }
  if (lane == 0) len[g] = (int32_t)(n <= cap ? n : -n);
}

}  // namespace

// ====================================================================================================== entry points
extern "C" {

int objnerf_volume_centres(int32_t nx, int32_t ny, int32_t nz, int32_t z0, int32_t nzs, const float* origin, float voxel,
                           float* out, void* stream) {
  (void)hipGetLastError();
  if (!mv_dims_ok(nx, ny, nz) || z0 < 0 || nzs < 0 || z0 + (int64_t)nzs > nz || !origin || !(voxel > 0.0f)) return OBJNERF_EINVAL;
  if (nzs == 0) return OBJNERF_OK;
  if (!out) return OBJNERF_EINVAL;
  const int64_t n = (int64_t)nx * ny * nzs;
  hipLaunchKernelGGL(mv_centres_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (int)nx, (int)ny,
                     (int)z0, n, origin[0], origin[1], origin[2], voxel, out);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_volume_project(int32_t nx, int32_t ny, int32_t nz, int32_t axis, const int32_t* label, int32_t* out,
                           void* stream) {
  (void)hipGetLastError();
  if (!mv_dims_ok(nx, ny, nz) || axis < 0 || axis > 2 || !label || !out) return OBJNERF_EINVAL;
  const int64_t n = (int64_t)nx * ny * nz / (axis == 0 ? nx : axis == 1 ? ny : nz);
  hipLaunchKernelGGL(mv_project_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (int)nx, (int)ny,
                     (int)nz, (int)axis, label, out);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_volume_clearance(int32_t nx, int32_t ny, int32_t nz, const int32_t* label, int32_t* dist2, int32_t* site,
                             int32_t* tmp_dist2, int32_t* tmp_site, void* stream) {
  (void)hipGetLastError();
  if (!mv_dims_ok(nx, ny, nz) || !label || !dist2 || !site || !tmp_dist2 || !tmp_site) return OBJNERF_EINVAL;
  if (dist2 == tmp_dist2 || site == tmp_site) return OBJNERF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nlines = (int64_t)ny * nz;
  const int segs = (int)cdiv(nx, 64);
  // x: label -> (dist2, site); y: -> tmp; z: -> (dist2, site)
  hipLaunchKernelGGL(mv_edt_x_kernel, dim3((unsigned)(segs * cdiv(nlines, 4))), dim3(256), 0, s, (int)nx, nlines, segs,
                     label, dist2, site);
  CHECK_LAUNCH();
  const int nxt = (int)cdiv(nx, MV_EX);
  const int64_t plane = (int64_t)nx * ny;
  int nat = (int)cdiv(ny, MV_EA);
  hipLaunchKernelGGL(mv_edt_axis_kernel, dim3((unsigned)((int64_t)nxt * nat * nz)), dim3(256), 0, s, (int)nx, (int)ny,
                     (int64_t)nx, (int)nz, plane, nxt, nat, (const int32_t*)dist2, (const int32_t*)site, tmp_dist2, tmp_site);
  CHECK_LAUNCH();
  nat = (int)cdiv(nz, MV_EA);
  hipLaunchKernelGGL(mv_edt_axis_kernel, dim3((unsigned)((int64_t)nxt * nat * ny)), dim3(256), 0, s, (int)nx, (int)nz, plane,
                     (int)ny, (int64_t)nx, nxt, nat, (const int32_t*)tmp_dist2, (const int32_t*)tmp_site, dist2, site);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int64_t objnerf_volume_reach_tiles(int32_t nx, int32_t ny, int32_t nz) {
  if (!mv_dims_ok(nx, ny, nz)) return 0;
  return cdiv(nx, MV_RT) * cdiv(ny, MV_RT) * cdiv(nz, MV_RT);
}

int objnerf_volume_reach_rounds(int32_t nx, int32_t ny, int32_t nz, const int32_t* label, const int32_t* dist2, int32_t r2,
                                uint32_t* cost, int32_t* active, int32_t round0, int32_t n_rounds, int32_t* changed,
                                void* stream) {
  (void)hipGetLastError();
  if (!mv_dims_ok(nx, ny, nz) || r2 < 0 || round0 < 0 || n_rounds < 0 || !label || !dist2 || !cost || !active || !changed)
    return OBJNERF_EINVAL;
  const int ntx = (int)cdiv(nx, MV_RT), nty = (int)cdiv(ny, MV_RT), ntz = (int)cdiv(nz, MV_RT);
  const int64_t nt = (int64_t)ntx * nty * ntz;
  for (int r = 0; r < n_rounds; ++r) {
    const int in = (round0 + r) & 1;
    hipLaunchKernelGGL(mv_reach_kernel, dim3((unsigned)nt), dim3(MV_RWG), 0, (hipStream_t)stream, (int)nx, (int)ny, (int)nz,
                       ntx, nty, ntz, label, dist2, r2, cost, active + in * nt, active + (in ^ 1) * nt, changed + r);
    CHECK_LAUNCH();
  }
  return OBJNERF_OK;
}

int objnerf_volume_goals(int32_t nx, int32_t ny, int32_t nz, int32_t K, const int32_t* label, const int32_t* dist2,
                         const int32_t* site, const uint32_t* cost, int32_t r2, uint64_t* table, void* stream) {
  (void)hipGetLastError();
  if (!mv_dims_ok(nx, ny, nz) || K < 1 || r2 < 0 || !label || !dist2 || !site || !cost || !table) return OBJNERF_EINVAL;
  const int64_t n = (int64_t)nx * ny * nz;
  hipLaunchKernelGGL(mv_goals_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, n, (int)K, label,
                     dist2, site, cost, r2, (u64*)table);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_volume_paths(int32_t nx, int32_t ny, int32_t nz, const int32_t* label, const int32_t* dist2, int32_t r2,
                         const uint32_t* cost, int32_t G, const int32_t* goals, int32_t cap, int32_t* out, int32_t* len,
                         void* stream) {
  (void)hipGetLastError();
  if (!mv_dims_ok(nx, ny, nz) || r2 < 0 || G < 0 || cap < 0 || !label || !dist2 || !cost) return OBJNERF_EINVAL;
  if (G == 0) return OBJNERF_OK;
  if (!goals || !len || (cap > 0 && !out)) return OBJNERF_EINVAL;
  hipLaunchKernelGGL(mv_paths_kernel, dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream, (int)nx, (int)ny, (int)nz, label,
                     dist2, r2, cost, goals, cap, out, len);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

}  // extern "C"
