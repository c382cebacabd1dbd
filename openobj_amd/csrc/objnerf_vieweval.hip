// Scoring a rendered map view against a frame of the sequence (gfx950): objnerf_view_compare, one launch per frame
// (openobj_amd/map_view_eval.py).  Photometric error, exact-integer SSIM, depth error and the 2-D
// instance confusion of the mask-id image in one pass over the images MapView.render leaves on the device.  The
// definition -- the tap table, the integer moments and the fixed fp64 sequence -- stands with the declaration in
// include/objnerf_hip.h; this banner is about the shape of the kernel.
//
// Tiles.  A workgroup of 256 threads takes VE_T x VE_T = 32 x 32 pixels (4 per thread; lanes run along h, the
// contiguous axis of a [W][H] image) and walks the tile list with a stride of the grid, so any grid covers the image.
// The two colour images are staged ONCE per tile with the 5-pixel halo of the 11 x 11 window: 42 rows (w) of 42 x 3
// interleaved bytes, pitch 128.  SSIM is separable: per channel, pass 1 runs the 11 taps along h for the 42 halo rows
// (five sums per point: x, y, x^2, y^2, xy; <= 65536 * 65025 < 2^32, so uint32) into `mid` [5][42][32]; pass 2 runs them
// along w in uint64 (< 2^48).  In pass 1 consecutive lanes read bytes 3 apart (at most two lanes per bank dword, which
// broadcast or sit in different banks) and write consecutive dwords; in pass 2 they read consecutive dwords of one mid
// row: both passes are free of bank conflicts beyond that.  The channel loop keeps `mid` at 26 KB instead of 79 KB.
//
// Tables (Guideline 12).  Every pixel adds to row r of acc and to one cell of conf.  A frame in which every pixel has
// one id would put all 816 000 pixels of a native frame onto nine addresses, so contributions are reduced three times
// before they reach global memory:
//   1. in the wave: the lanes are grouped by their key (acc row, conf column); per distinct key the counts are
//      ballots + popcounts, the sums a butterfly of __shfl_xor, and ONE lane adds the group's nine values;
//   2. in the workgroup: that lane adds into an LDS-private copy of the tables (acc int64 [G + 1][9], conf uint32
//      [G][G + 1]: a workgroup's share of a cell is far below 2^32) -- LDS atomics, <= 4 waves on an address;
//   3. per workgroup, after its last tile: one 64-bit global atomic per non-zero cell.
// A single-id frame then costs about ten global atomics per workgroup.  The LDS copy holds G <= VE_ROWS = 64 rows
// (4.7 KB + 16.6 KB; with the staging 59 KB, two workgroups per compute unit).  Above that the lane of step 1 adds to
// global memory directly (view_compare_kernel<false>): wave-aggregated global atomics, one per wave, key and column.
// Every accumulated value is an integer, so both paths, every grid and every arrival order give the same tables.
#include "objnerf_device.h"
#include "objnerf_wg.h"

namespace {

constexpr int VE_T = OBJNERF_VIEW_EVAL_TILE;
constexpr int VE_R = 5;                               // the window's radius
constexpr int VE_HALO = VE_T + 2 * VE_R;              // 42
constexpr int VE_ROWB = VE_HALO * 3;                  // 126 bytes of a staged row
constexpr int VE_PITCH = 128;
constexpr int VE_WG = 256;
constexpr int VE_PPT = VE_T * VE_T / VE_WG;           // pixels per thread
constexpr int VE_ROWS = OBJNERF_VIEW_EVAL_LDS_ROWS;
constexpr int VE_COLS = 9;
static_assert(VE_T == 32 && VE_PPT * VE_WG == VE_T * VE_T, "the pixel <-> thread map below assumes a 32 x 32 tile");

constexpr double VE_C1 = 6.5025, VE_C2 = 58.5225;    // (0.01 * 255)^2, (0.03 * 255)^2

struct ViewCmp {
  int W, H, n_lut, G, tiles_h, n_tiles;
  const uint8_t *rgb_r, *rgb_g, *painted;
  const float *depth_r, *depth_g;
  const int32_t *id_r, *id_g, *lut;
  long long* acc;
  long long* conf;
  float* ssim_map;
};

__device__ __forceinline__ unsigned tap(const int k) {
  constexpr unsigned t[11] = {67, 498, 2359, 7167, 13960, 17434, 13960, 7167, 2359, 498, 67};
  return t[k];
}

__device__ __forceinline__ int row_of(const int id, const int32_t* __restrict__ lut, const int n_lut, const int G) {
  if (id < 0 || id >= n_lut) return G;
  const int r = lut[id];
  return (r >= 0 && r < G) ? r : G;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ void add_cell(long long* cell, const long long v) {
  if (v != 0) atomicAdd((unsigned long long*)cell, (unsigned long long)v);
}

// one channel's s from the five integer moments: the fp64 sequence of the header, one rounding per operation
__device__ __forceinline__ double ssim_term(const unsigned long long Mx, const unsigned long long My, const unsigned long long Mxx,
                                            const unsigned long long Myy, const unsigned long long Mxy) {
  constexpr double S = 1.0 / 4294967296.0;
  const double mx = (double)Mx * S, my = (double)My * S, exx = (double)Mxx * S, eyy = (double)Myy * S, exy = (double)Mxy * S;
  const double mxmx = mx * mx, mymy = my * my, mxmy = mx * my;
  const double vx = exx - mxmx, vy = eyy - mymy, cv = exy - mxmy;
  const double a1 = 2.0 * mxmy + VE_C1, a2 = 2.0 * cv + VE_C2;
  const double b1 = (mxmx + mymy) + VE_C1, b2 = (vx + vy) + VE_C2;
  return (a1 * a2) / (b1 * b2);
}

template <bool LDS_TABLES>
__global__ void __launch_bounds__(VE_WG) view_compare_kernel(const ViewCmp a) {
  __shared__ uint8_t xs[VE_HALO * VE_PITCH], ys[VE_HALO * VE_PITCH];
  __shared__ unsigned mid[5][VE_HALO][VE_T];
  __shared__ long long acc_l[LDS_TABLES ? (VE_ROWS + 1) * VE_COLS : 1];
  __shared__ unsigned conf_l[LDS_TABLES ? VE_ROWS * (VE_ROWS + 1) : 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int W = a.W, H = a.H, G = a.G;
  const int n_acc = (G + 1) * VE_COLS, n_conf = a.conf ? G * (G + 1) : 0;
  if (LDS_TABLES) {
    for (int i = tid; i < n_acc; i += VE_WG) acc_l[i] = 0;
    for (int i = tid; i < n_conf; i += VE_WG) conf_l[i] = 0;
  }
  long long* const acc_dst = LDS_TABLES ? acc_l : a.acc;
  // (the first barrier of the tile loop orders the zeroing before any add)
  for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const int w0 = (tile / a.tiles_h) * VE_T, h0 = (tile % a.tiles_h) * VE_T;
    // ---- stage both colour images with the halo; outside the image: zeros, which no interior pixel's window reads
    for (int i = tid; i < VE_HALO * VE_ROWB; i += VE_WG) {
      const int r = i / VE_ROWB, b = i - r * VE_ROWB;
      const int w = w0 - VE_R + r, h = h0 - VE_R + b / 3;
      uint8_t x = 0, y = 0;
      if (w >= 0 && w < W && h >= 0 && h < H) {
        const int64_t g = ((int64_t)w * H + h) * 3 + b % 3;
        x = a.rgb_r[g];
        y = a.rgb_g[g];
      }
      xs[r * VE_PITCH + b] = x;
      ys[r * VE_PITCH + b] = y;
    }
    __syncthreads();
    // a tile holds an interior pixel iff its ranges meet [5, W - 5) x [5, H - 5): uniform over the workgroup
    const bool any_interior = w0 + VE_T > VE_R && w0 < W - VE_R && h0 + VE_T > VE_R && h0 < H - VE_R;
    double sv[VE_PPT];
    bool interior[VE_PPT];
#pragma unroll
    for (int j = 0; j < VE_PPT; ++j) {
      const int i = j * VE_WG + tid, w = w0 + (i >> 5), h = h0 + (i & 31);
      interior[j] = w >= VE_R && w < W - VE_R && h >= VE_R && h < H - VE_R;
      sv[j] = 0.0;
    }
    if (any_interior) {
      for (int ch = 0; ch < 3; ++ch) {
        for (int i = tid; i < VE_HALO * VE_T; i += VE_WG) {                // pass 1: along h
          const int r = i >> 5, c = i & 31;
          const uint8_t* px = xs + r * VE_PITCH + c * 3 + ch;
          const uint8_t* py = ys + r * VE_PITCH + c * 3 + ch;
          unsigned sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
          for (int k = 0; k < 11; ++k) {
            const unsigned x = px[3 * k], y = py[3 * k], t = tap(k);
            sx += t * x; sy += t * y; sxx += t * (x * x); syy += t * (y * y); sxy += t * (x * y);
          }
          mid[0][r][c] = sx; mid[1][r][c] = sy; mid[2][r][c] = sxx; mid[3][r][c] = syy; mid[4][r][c] = sxy;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < VE_PPT; ++j) {                                  // pass 2: along w
          if (!interior[j]) continue;
          const int i = j * VE_WG + tid, wl = i >> 5, hl = i & 31;
          unsigned long long M[5] = {0, 0, 0, 0, 0};
#pragma unroll
          for (int k = 0; k < 11; ++k) {
            const unsigned long long t = tap(k);
#pragma unroll
            for (int m = 0; m < 5; ++m) M[m] += t * (unsigned long long)mid[m][wl + k][hl];
          }
          const double s = ssim_term(M[0], M[1], M[2], M[3], M[4]);
          sv[j] = ch == 0 ? s : sv[j] + s;                                  // (s_R + s_G) + s_B
        }
        __syncthreads();                                                    // mid is free for the next channel
      }
    }
    // ---- per pixel: the nine columns, the confusion cell, the map; reduced in the wave per key
#pragma unroll
    for (int j = 0; j < VE_PPT; ++j) {
      const int i = j * VE_WG + tid, wl = i >> 5, hl = i & 31, w = w0 + wl, h = h0 + hl;
      const bool valid = w < W && h < H;
      int key = -1, rg = G, rp = G;
      unsigned se = 0;
      bool pt = false, f4 = false, f5 = false;
      long long dq = 0, q = 0;
      if (valid) {
        const int64_t p = (int64_t)w * H + h;
        const uint8_t* cx = xs + (wl + VE_R) * VE_PITCH + (hl + VE_R) * 3;
        const uint8_t* cy = ys + (wl + VE_R) * VE_PITCH + (hl + VE_R) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int d = (int)cx[c] - (int)cy[c];
          se += (unsigned)(d * d);
        }
        pt = a.painted ? a.painted[p] != 0 : true;
        const float dg = a.depth_g[p], dr = a.depth_r[p];
        f4 = dg > 0.0f;
        f5 = f4 && dr < 100.0f;
        if (f5) dq = (long long)floor((double)fminf(fabsf(dr - dg), 4194304.0f) * 1048576.0);
        rg = row_of(a.id_g[p], a.lut, a.n_lut, G);
        if (a.conf && rg < G) rp = row_of(a.id_r[p], a.lut, a.n_lut, G);
        key = rg * (G + 1) + (a.conf && rg < G ? rp : 0);
        float out = __builtin_nanf("");
        if (interior[j]) {
          const double value = sv[j] / 3.0;
          q = (long long)floor(value * 4294967296.0);
          out = (float)value;
        }
        if (a.ssim_map) a.ssim_map[p] = out;
      }
      unsigned long long todo = __ballot(valid);
      while (todo) {                                                        // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, leader);
        const bool mine = key == k;
        const unsigned long long m = __ballot(mine);
        const long long n0 = __popcll(m), n1 = __popcll(__ballot(mine && pt)), n4 = __popcll(__ballot(mine && f4)),
                        n5 = __popcll(__ballot(mine && f5)), n7 = __popcll(__ballot(mine && interior[j]));
        const unsigned s2 = wave_sum(mine ? se : 0u), s3 = wave_sum(mine && pt ? se : 0u);
        const long long s6 = wave_sum(mine ? dq : 0ll), s8 = wave_sum(mine ? q : 0ll);
        if (lane == leader) {
          long long* row = acc_dst + (int64_t)rg * VE_COLS;
          add_cell(row + 0, n0); add_cell(row + 1, n1); add_cell(row + 2, (long long)s2); add_cell(row + 3, (long long)s3);
          add_cell(row + 4, n4); add_cell(row + 5, n5); add_cell(row + 6, s6); add_cell(row + 7, n7); add_cell(row + 8, s8);
          if (a.conf && rg < G) {
            if (LDS_TABLES) atomicAdd(conf_l + rg * (G + 1) + rp, (unsigned)n0);
            else add_cell(a.conf + (int64_t)rg * (G + 1) + rp, n0);
          }
        }
        todo &= ~m;
      }
    }
    __syncthreads();                                                        // xs / ys are free for the next tile
  }
  if (LDS_TABLES) {
    __syncthreads();
    for (int i = tid; i < n_acc; i += VE_WG) add_cell(a.acc + i, acc_l[i]);
    for (int i = tid; i < n_conf; i += VE_WG) add_cell(a.conf + i, (long long)conf_l[i]);
  }
}

}  // namespace

extern "C" {

int objnerf_view_compare(int32_t W, int32_t H, const uint8_t* rgb_r, const float* depth_r, const int32_t* id_r,
                         const uint8_t* painted, const uint8_t* rgb_g, const float* depth_g, const int32_t* id_g,
                         const int32_t* lut, int32_t n_lut, int32_t G, int64_t* acc, int64_t* conf, float* ssim_map,
                         int32_t workgroups, void* stream) {
  (void)hipGetLastError();
  if (W < 1 || H < 1 || (int64_t)W * H > 0x7fffffff || G < 1 || G > OBJNERF_VIEW_EVAL_MAX_ROWS || n_lut < 0 || workgroups < 0)
    return OBJNERF_EINVAL;
  if (!rgb_r || !depth_r || !id_r || !rgb_g || !depth_g || !id_g || !acc || (n_lut > 0 && !lut)) return OBJNERF_EINVAL;
  ViewCmp a;
  a.W = W; a.H = H; a.n_lut = n_lut; a.G = G;
  a.tiles_h = (int)cdiv(H, VE_T);
  a.n_tiles = (int)(cdiv(W, VE_T) * a.tiles_h);
  a.rgb_r = rgb_r; a.rgb_g = rgb_g; a.painted = painted; a.depth_r = depth_r; a.depth_g = depth_g;
  a.id_r = id_r; a.id_g = id_g; a.lut = lut;
  a.acc = (long long*)acc; a.conf = (long long*)conf; a.ssim_map = ssim_map;
  // two workgroups fit a compute unit (LDS); four per unit in the queue keep the tail short
  int64_t grid = workgroups > 0 ? (int64_t)workgroups : 4 * (int64_t)objnerf_num_cu();
  if (grid > a.n_tiles) grid = a.n_tiles;
  hipStream_t st = (hipStream_t)stream;
  if (G <= VE_ROWS) hipLaunchKernelGGL(view_compare_kernel<true>, dim3((unsigned)grid), dim3(VE_WG), 0, st, a);
  else hipLaunchKernelGGL(view_compare_kernel<false>, dim3((unsigned)grid), dim3(VE_WG), 0, st, a);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

}  // extern "C"
