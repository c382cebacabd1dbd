// The mask front end: the image work of the reference's maskclustering/mask_gen.py between its models.
//
// (a) objnerf_cc_label     the 8-connected components of EVERY mask of F id images in one pass (split_mask's
//     cv2.connectedComponentsWithStats per mask, :168).  Union-find whose parent is always a smaller index: a tile of
//     32 x 32 pixels in LDS, then the pixels on the tile borders in global memory, then a flatten.  The root of a set is
//     its smallest index = the component's first pixel in raster order, whatever order the unions ran in.
// (b) objnerf_cc_table     the roots compacted in raster order into a per-frame CSR (seg_csr_count / _emit of
//     objnerf_segments.h: no atomics decide the order), then area and box of every component with integer atomics.
// (c) objnerf_cc_boundary, objnerf_cc_gaps   the boundary pixels of the selected components as a CSR, and the exact minimum
//     squared distance of pairs of them by LDS-tiled brute force (closest_distance, :139-160, without its sampling).
// (d) objnerf_cc_relabel   component -> final id, the new id image, area and box of every final id.
// (e) objnerf_clip_crops   PIL's two-pass integer bicubic resample + CLIP's normalisation of the padded crops (:495-516).
// Everything is integer up to the last two fp32 operations of (e), which are rounded one by one (-ffp-contract=off):
// two calls write the same bytes.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "objnerf_segments.h"

namespace {

#define CLEAR_STALE() (void)hipGetLastError()

constexpr int CC_T = 32;                   // tile side: 1024 pixels, four per thread
constexpr int CC_WG = 256;
constexpr int CC_ROW = 8;                  // ints per row of the component and final-id tables
constexpr int CC_RUN = 8;                  // consecutive pixels of a row per thread of the statistics kernels
constexpr int CC_MAX_SIDE = 32767;
constexpr int CC_FINAL_IDS = 256;

// (uf_find / uf_union, the union-find whose parent is always a smaller index: objnerf_wg.h)
// grid (tiles in x, tiles in y, F)
__global__ __launch_bounds__(CC_WG) void cc_local_kernel(const int H, const int W, const int32_t* __restrict__ ids,
                                                         int32_t* __restrict__ label) {
  __shared__ int sid[CC_T * CC_T];
  __shared__ int L[CC_T * CC_T];
  const int x0 = blockIdx.x * CC_T, y0 = blockIdx.y * CC_T;
  const int64_t base = (int64_t)blockIdx.z * H * W;
  for (int i = threadIdx.x; i < CC_T * CC_T; i += CC_WG) {
    const int x = x0 + (i & (CC_T - 1)), y = y0 + i / CC_T;
    sid[i] = x < W && y < H ? ids[base + (int64_t)y * W + x] : 0;
    L[i] = i;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CC_T * CC_T; i += CC_WG) {
    const int c = sid[i], lx = i & (CC_T - 1), ly = i / CC_T;
    if (c == 0) continue;
    if (lx > 0 && sid[i - 1] == c) uf_union(L, i, i - 1);
    if (ly > 0) {
      if (sid[i - CC_T] == c) uf_union(L, i, i - CC_T);
      if (lx > 0 && sid[i - CC_T - 1] == c) uf_union(L, i, i - CC_T - 1);
      if (lx < CC_T - 1 && sid[i - CC_T + 1] == c) uf_union(L, i, i - CC_T + 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CC_T * CC_T; i += CC_WG) {
    const int x = x0 + (i & (CC_T - 1)), y = y0 + i / CC_T;
    if (x >= W || y >= H) continue;
    int out = -1;
    if (sid[i] != 0) {
      const int r = uf_find(L, i);                 // local raster order = global raster order inside a tile
      out = (y0 + r / CC_T) * W + x0 + (r & (CC_T - 1));
    }
    label[base + (int64_t)y * W + x] = out;
  }
}

// a thread per pixel; the pixels of a tile's first row, first and last column join their neighbours in other tiles
__global__ __launch_bounds__(CC_WG) void cc_border_kernel(const int H, const int W, const int32_t* __restrict__ ids,
                                                          int32_t* label) {
  const int64_t n = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * CC_WG + threadIdx.x;
  if (p >= n) return;
  const int x = (int)(p % W), y = (int)(p / W), lx = x & (CC_T - 1), ly = y & (CC_T - 1);
  if (lx != 0 && ly != 0 && lx != CC_T - 1) return;
  const int32_t* id = ids + (int64_t)blockIdx.y * n;
  int* L = label + (int64_t)blockIdx.y * n;
  const int c = id[p];
  if (c == 0) return;
  if (lx == 0 && x > 0 && id[p - 1] == c) uf_union(L, (int)p, (int)p - 1);
  if (y > 0) {
    if (ly == 0 && id[p - W] == c) uf_union(L, (int)p, (int)p - W);
    if ((lx == 0 || ly == 0) && x > 0 && id[p - W - 1] == c) uf_union(L, (int)p, (int)p - W - 1);
    if ((lx == CC_T - 1 || ly == 0) && x + 1 < W && id[p - W + 1] == c) uf_union(L, (int)p, (int)p - W + 1);
  }
}

__global__ __launch_bounds__(CC_WG) void cc_flatten_kernel(const int64_t n, int32_t* label) {
  const int64_t p = (int64_t)blockIdx.x * CC_WG + threadIdx.x;
  if (p >= n) return;
  int* L = label + (int64_t)blockIdx.y * n;
  if (L[p] >= 0) L[p] = uf_find(L, (int)p);
}

// ------------------------------------------------------------------------------------------------- the component table
// the roots of frame k, in raster order (seg_csr_count / _emit); a row starts with an empty box
struct RootTest {
  typedef int Payload;
  const int32_t* label; const int32_t* ids; int64_t n; int32_t* table; int32_t* slot;
  __device__ bool hit(const int k, const int64_t i, int& frame) const {
    frame = k;
    return label[(int64_t)k * n + i] == (int32_t)i;
  }
  __device__ void store(const int64_t pos, const int64_t i, const int frame) const {
    int32_t* row = table + pos * CC_ROW;
    row[0] = (int32_t)i; row[1] = ids[(int64_t)frame * n + i]; row[2] = 0;
    row[3] = INT_MAX; row[4] = INT_MAX; row[5] = 0; row[6] = 0; row[7] = frame;
    slot[(int64_t)frame * n + i] = (int32_t)pos;
  }
};

// Area and box of the rows a Key maps the pixels to (-1: none).  A thread walks CC_RUN neighbours of one image row and
// issues its atomics once per run of equal rows, not once per pixel.  Integer atomics: any order gives the same table.
template <class Key>
__global__ __launch_bounds__(CC_WG) void cc_stats_kernel(const int H, const int W, const Key key, const int64_t rows,
                                                         int32_t* __restrict__ table) {
  const int chunks = (W + CC_RUN - 1) / CC_RUN;
  const int64_t t = (int64_t)blockIdx.x * CC_WG + threadIdx.x;
  if (t >= (int64_t)H * chunks) return;
  const int y = (int)(t / chunks), xa = (int)(t % chunks) * CC_RUN, xb = min(xa + CC_RUN, W);
  const int f = blockIdx.y;
  int64_t cur = -1;
  int cnt = 0, xmin = 0;
  for (int x = xa; x <= xb; ++x) {
    const int64_t r = x < xb ? key(f, y, x) : -2;                       // (x == xb: flush the last run)
    if (r == cur) { ++cnt; continue; }
    if (cur >= 0 && cur < rows) {
      int32_t* row = table + cur * CC_ROW;
      atomicAdd(&row[2], cnt);
      atomicMin(&row[3], xmin); atomicMin(&row[4], y);
      atomicMax(&row[5], x); atomicMax(&row[6], y + 1);                 // (x: one past the run's last column)
    }
    cur = r; cnt = 1; xmin = x;
  }
}

struct ComponentKey {
  const int32_t* label; const int32_t* slot; int64_t n; int W;
  __device__ int64_t operator()(const int f, const int y, const int x) const {
    const int r = label[(int64_t)f * n + (int64_t)y * W + x];
    return r < 0 || r >= n ? -1 : (int64_t)slot[(int64_t)f * n + r];
  }
};
// the final id of a pixel, written to the new id image on the way; row f * 256 + id of the final table
struct FinalKey {
  ComponentKey comp; const int32_t* final_id; int64_t rows; int32_t* out_ids;
  __device__ int64_t operator()(const int f, const int y, const int x) const {
    const int64_t pos = comp(f, y, x);
    int id = pos >= 0 && pos < rows ? final_id[pos] : 0;
    if (id < 0 || id >= CC_FINAL_IDS) id = 0;
    out_ids[(int64_t)f * comp.n + (int64_t)y * comp.W + x] = id;
    return id ? (int64_t)f * CC_FINAL_IDS + id : -1;
  }
};

__global__ void cc_final_init_kernel(const int64_t rows, int32_t* __restrict__ table) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  int32_t* row = table + r * CC_ROW;
  row[0] = -1; row[1] = (int32_t)(r % CC_FINAL_IDS); row[2] = 0;
  row[3] = INT_MAX; row[4] = INT_MAX; row[5] = 0; row[6] = 0; row[7] = (int32_t)(r / CC_FINAL_IDS);
}

// ------------------------------------------------------------------------------------------- boundary lists and gaps
// the list of pixel p (-1: not a boundary pixel of a selected component): a 4-neighbour outside the component
__device__ __forceinline__ int boundary_list(const int H, const int W, const int32_t* __restrict__ L,
                                             const int32_t* __restrict__ slot, const int32_t* __restrict__ sel,
                                             const int64_t rows, const int S, const int64_t p) {
  const int64_t n = (int64_t)H * W;
  const int r = L[p];
  if (r < 0 || r >= n) return -1;
  const int pos = slot[r];
  if (pos < 0 || pos >= rows) return -1;
  const int s = sel[pos];
  if (s < 0 || s >= S) return -1;
  const int x = (int)(p % W), y = (int)(p / W);
  const bool edge = x == 0 || y == 0 || x == W - 1 || y == H - 1 || L[p - 1] != r || L[p + 1] != r || L[p - W] != r ||
                    L[p + W] != r;
  return edge ? s : -1;
}
template <bool EMIT>
__global__ __launch_bounds__(CC_WG) void cc_boundary_kernel(const int H, const int W, const int32_t* __restrict__ label,
                                                            const int32_t* __restrict__ slot,
                                                            const int32_t* __restrict__ sel, const int64_t rows,
                                                            const int S, int32_t* __restrict__ boff,
                                                            int32_t* __restrict__ cursor, uint32_t* __restrict__ bpix,
                                                            const int64_t bcap) {
  const int64_t n = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * CC_WG + threadIdx.x;
  if (p >= n) return;
  const int s = boundary_list(H, W, label + (int64_t)blockIdx.y * n, slot + (int64_t)blockIdx.y * n, sel, rows, S, p);
  if (s < 0) return;
  if (!EMIT) {
    atomicAdd(&boff[s], 1);                        // (the counts; scanned in place afterwards)
  } else {
    const int64_t q = (int64_t)boff[s] + atomicAdd(&cursor[s], 1);
    if (q >= 0 && q < boff[s + 1] && q < bcap) bpix[q] = ((uint32_t)(p / W) << 16) | (uint32_t)(p % W);
  }
}

__global__ void cc_fill_kernel(const int n, const int32_t v, int32_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = v;
}

constexpr int GAP_WG = 256;
constexpr int GAP_SPLIT = 8;       // workgroups that share the first list of a pair
// grid (P, GAP_SPLIT): a thread holds one pixel of the first list, the second list passes through LDS 256 at a time
__global__ __launch_bounds__(GAP_WG) void cc_gaps_kernel(const int32_t* __restrict__ pairs, const int S,
                                                         const int32_t* __restrict__ boff,
                                                         const uint32_t* __restrict__ bpix, const int64_t bcap,
                                                         int32_t* __restrict__ d2) {
  __shared__ uint32_t sb[GAP_WG];
  __shared__ int wmin[GAP_WG / 64];
  const int a = pairs[2 * blockIdx.x], b = pairs[2 * blockIdx.x + 1];
  if (a < 0 || a >= S || b < 0 || b >= S) return;                       // (uniform over the workgroup, like all below)
  const int64_t a0 = min((int64_t)boff[a], bcap), a1 = min((int64_t)boff[a + 1], bcap);
  const int64_t b0 = min((int64_t)boff[b], bcap), b1 = min((int64_t)boff[b + 1], bcap);
  int best = INT_MAX;
  for (int64_t ca = a0 + (int64_t)blockIdx.y * GAP_WG; ca < a1; ca += (int64_t)gridDim.y * GAP_WG) {
    const bool valid = ca + threadIdx.x < a1;
    const uint32_t pa = valid ? bpix[ca + threadIdx.x] : 0u;
    const int ax = (int)(pa & 0xffffu), ay = (int)(pa >> 16);
    int mine = INT_MAX;
    for (int64_t cb = b0; cb < b1; cb += GAP_WG) {
      __syncthreads();                                                  // the tile before is read
      if (cb + threadIdx.x < b1) sb[threadIdx.x] = bpix[cb + threadIdx.x];
      __syncthreads();
      const int m = (int)min((int64_t)GAP_WG, b1 - cb);
      for (int j = 0; j < m; ++j) {
        const int dx = ax - (int)(sb[j] & 0xffffu), dy = ay - (int)(sb[j] >> 16);
        mine = min(mine, dx * dx + dy * dy);
      }
    }
    if (valid) best = min(best, mine);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < GAP_WG / 64; ++w) best = min(best, wmin[w]);
    if (best != INT_MAX) atomicMin(&d2[blockIdx.x], best);
  }
}

// ------------------------------------------------------------------------------------------------------ CLIP crops
constexpr int CLIP_S = OBJNERF_CLIP_SIDE;
constexpr int PIL_BITS = 22;                       // PRECISION_BITS of PIL's 8-bit resample: 32 - 8 - 2

__device__ __forceinline__ int clampi(const int v, const int lo, const int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ uint8_t clip8(const int v) { return (uint8_t)clampi(v >> PIL_BITS, 0, 255); }

// grid (blocks over tmp_rows * 224, n): the horizontal pass, or the copy that stands for it, into tmp
__global__ __launch_bounds__(CC_WG) void clip_rows_kernel(const int H, const int W, const uint8_t* __restrict__ image,
                                                          const int32_t* __restrict__ desc, const int kh,
                                                          const int32_t* __restrict__ hb, const int32_t* __restrict__ hk,
                                                          const int tmp_rows, uint8_t* __restrict__ tmp) {
  const int j = blockIdx.y;
  const int32_t* d = desc + j * 8;
  const int t = blockIdx.x * CC_WG + threadIdx.x;
  const int r = t / CLIP_S, ox = t % CLIP_S;
  if (r >= min(d[5], tmp_rows)) return;
  const int sy = clampi(d[1] + d[4] + r, 0, H - 1);
  const uint8_t* src = image + (int64_t)sy * W * 3;
  uint8_t* dst = tmp + (((int64_t)j * tmp_rows + r) * CLIP_S + ox) * 3;
  if (d[6] >= 0) {
    const int sx = clampi(d[0] + d[6] + ox, 0, W - 1);
    dst[0] = src[sx * 3]; dst[1] = src[sx * 3 + 1]; dst[2] = src[sx * 3 + 2];
    return;
  }
  const int32_t* bnd = hb + ((int64_t)j * CLIP_S + ox) * 2;
  const int32_t* k = hk + ((int64_t)j * CLIP_S + ox) * kh;
  const int cnt = clampi(bnd[1], 0, kh);
  int s0 = 1 << (PIL_BITS - 1), s1 = s0, s2 = s0;
  for (int i = 0; i < cnt; ++i) {
    const int sx = clampi(d[0] + bnd[0] + i, 0, W - 1), c = k[i];
    s0 += src[sx * 3] * c; s1 += src[sx * 3 + 1] * c; s2 += src[sx * 3 + 2] * c;
  }
  dst[0] = clip8(s0); dst[1] = clip8(s1); dst[2] = clip8(s2);
}

// grid (blocks over 224 * 224, n): the vertical pass over tmp, then ToTensor and Normalize
__global__ __launch_bounds__(CC_WG) void clip_cols_kernel(const int32_t* __restrict__ desc, const int kv,
                                                          const int32_t* __restrict__ vb, const int32_t* __restrict__ vk,
                                                          const int tmp_rows, const uint8_t* __restrict__ tmp,
                                                          float* __restrict__ out) {
  const int j = blockIdx.y;
  const int32_t* d = desc + j * 8;
  const int t = blockIdx.x * CC_WG + threadIdx.x;
  if (t >= CLIP_S * CLIP_S) return;
  const int oy = t / CLIP_S, ox = t % CLIP_S;
  const int last = max(min(d[5], tmp_rows), 1) - 1;
  const uint8_t* col = tmp + ((int64_t)j * tmp_rows * CLIP_S + ox) * 3;
  int v0, v1, v2;
  if (d[7] >= 0) {
    const uint8_t* px = col + (int64_t)clampi(d[7] + oy - d[4], 0, last) * CLIP_S * 3;
    v0 = px[0]; v1 = px[1]; v2 = px[2];
  } else {
    const int32_t* bnd = vb + ((int64_t)j * CLIP_S + oy) * 2;
    const int32_t* k = vk + ((int64_t)j * CLIP_S + oy) * kv;
    const int cnt = clampi(bnd[1], 0, kv);
    int s0 = 1 << (PIL_BITS - 1), s1 = s0, s2 = s0;
    for (int i = 0; i < cnt; ++i) {
      const uint8_t* px = col + (int64_t)clampi(bnd[0] - d[4] + i, 0, last) * CLIP_S * 3;
      const int c = k[i];
      s0 += px[0] * c; s1 += px[1] * c; s2 += px[2] * c;
    }
    v0 = clip8(s0); v1 = clip8(s1); v2 = clip8(s2);
  }
  // torchvision's ToTensor (a true division by 255) and Normalize with CLIP's constants, each operation rounded to fp32
  float* o = out + (int64_t)j * 3 * CLIP_S * CLIP_S + t;
  o[0] = ((float)v0 / 255.0f - 0.48145466f) / 0.26862954f;
  o[CLIP_S * CLIP_S] = ((float)v1 / 255.0f - 0.4578275f) / 0.26130258f;
  o[2 * CLIP_S * CLIP_S] = ((float)v2 / 255.0f - 0.40821073f) / 0.27577711f;
}

inline bool cc_sizes_ok(const int32_t F, const int32_t H, const int32_t W) {
  return F >= 1 && F <= 65535 && H >= 1 && H <= CC_MAX_SIDE && W >= 1 && W <= CC_MAX_SIDE;
}

}  // namespace

extern "C" {

int objnerf_cc_label(int32_t F, int32_t H, int32_t W, const int32_t* ids, int32_t* label, void* stream) {
  CLEAR_STALE();
  if (!cc_sizes_ok(F, H, W) || !ids || !label) return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)H * W;
  const dim3 px((unsigned)cdiv(n, CC_WG), (unsigned)F);
  hipLaunchKernelGGL(cc_local_kernel, dim3((unsigned)cdiv(W, CC_T), (unsigned)cdiv(H, CC_T), (unsigned)F), dim3(CC_WG), 0, st,
                     H, W, ids, label);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_border_kernel, px, dim3(CC_WG), 0, st, H, W, ids, label);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_flatten_kernel, px, dim3(CC_WG), 0, st, n, label);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

size_t objnerf_cc_table_workspace_bytes(int32_t F, int32_t H, int32_t W) {
  if (!cc_sizes_ok(F, H, W)) return 0;
  return seg_csr_workspace_bytes((int64_t)H * W, F);
}

int objnerf_cc_table(int32_t F, int32_t H, int32_t W, const int32_t* ids, const int32_t* label, void* ws, size_t ws_bytes,
                     int64_t cap, int64_t* comp_off, int32_t* table, int32_t* slot, void* stream) {
  CLEAR_STALE();
  if (!cc_sizes_ok(F, H, W) || !ids || !label || !ws || cap < 1 || cap > 0x7fffffff || !comp_off || !table || !slot)
    return OBJNERF_EINVAL;
  if (ws_bytes < objnerf_cc_table_workspace_bytes(F, H, W)) return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)H * W;
  if (hipMemsetAsync(slot, 0xff, (size_t)F * n * sizeof(int32_t), st) != hipSuccess) return OBJNERF_ELAUNCH;
  const RootTest test{label, ids, n, table, slot};
  int rc = seg_csr_count(n, F, test, 1, ws, comp_off, st);
  if (rc != OBJNERF_OK) return rc;
  rc = seg_csr_emit(n, F, test, ws, cap, st);
  if (rc != OBJNERF_OK) return rc;
  const ComponentKey key{label, slot, n, W};
  hipLaunchKernelGGL(cc_stats_kernel<ComponentKey>, dim3((unsigned)cdiv((int64_t)H * cdiv(W, CC_RUN), CC_WG), (unsigned)F),
                     dim3(CC_WG), 0, st, H, W, key, cap, table);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_cc_boundary(int32_t F, int32_t H, int32_t W, const int32_t* label, const int32_t* slot, const int32_t* sel,
                        int64_t rows, int32_t S, int32_t* boff, int32_t* cursor, uint32_t* bpix, int64_t bcap,
                        void* stream) {
  CLEAR_STALE();
  if (!cc_sizes_ok(F, H, W) || !label || !slot || !sel || rows < 1 || S < 1 || !boff || !cursor || !bpix || bcap < 1 ||
      bcap > 0x7fffffff)
    return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)H * W;
  const dim3 px((unsigned)cdiv(n, CC_WG), (unsigned)F);
  if (hipMemsetAsync(boff, 0, ((size_t)S + 1) * sizeof(int32_t), st) != hipSuccess) return OBJNERF_ELAUNCH;
  if (hipMemsetAsync(cursor, 0, (size_t)S * sizeof(int32_t), st) != hipSuccess) return OBJNERF_ELAUNCH;
  hipLaunchKernelGGL(cc_boundary_kernel<false>, px, dim3(CC_WG), 0, st, H, W, label, slot, sel, rows, S, boff, cursor, bpix,
                     bcap);
  CHECK_LAUNCH();
  hipLaunchKernelGGL((wg_scan_kernel<SEG_SCAN_WG, 1, int32_t>), dim3(1), dim3(SEG_SCAN_WG), 0, st, boff, (int64_t)S, boff + S);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_boundary_kernel<true>, px, dim3(CC_WG), 0, st, H, W, label, slot, sel, rows, S, boff, cursor, bpix,
                     bcap);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_cc_gaps(int32_t P, const int32_t* pairs, int32_t S, const int32_t* boff, const uint32_t* bpix, int64_t bcap,
                    int32_t* d2, void* stream) {
  CLEAR_STALE();
  if (P < 1 || !pairs || S < 1 || !boff || !bpix || bcap < 1 || !d2) return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_fill_kernel, dim3((unsigned)cdiv(P, 256)), dim3(256), 0, st, P, INT_MAX, d2);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_gaps_kernel, dim3((unsigned)P, GAP_SPLIT), dim3(GAP_WG), 0, st, pairs, S, boff, bpix, bcap, d2);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_cc_relabel(int32_t F, int32_t H, int32_t W, const int32_t* label, const int32_t* slot, const int32_t* final_id,
                       int64_t rows, int32_t* out_ids, int32_t* stats, void* stream) {
  CLEAR_STALE();
  if (!cc_sizes_ok(F, H, W) || !label || !slot || !final_id || rows < 1 || !out_ids || !stats) return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)H * W, frows = (int64_t)F * CC_FINAL_IDS;
  hipLaunchKernelGGL(cc_final_init_kernel, dim3((unsigned)cdiv(frows, 256)), dim3(256), 0, st, frows, stats);
  CHECK_LAUNCH();
  const FinalKey key{ComponentKey{label, slot, n, W}, final_id, rows, out_ids};
  hipLaunchKernelGGL(cc_stats_kernel<FinalKey>, dim3((unsigned)cdiv((int64_t)H * cdiv(W, CC_RUN), CC_WG), (unsigned)F),
                     dim3(CC_WG), 0, st, H, W, key, frows, stats);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_clip_crops(int32_t n, int32_t H, int32_t W, const uint8_t* image, const int32_t* desc, int32_t kh,
                       const int32_t* hb, const int32_t* hk, int32_t kv, const int32_t* vb, const int32_t* vk,
                       int32_t tmp_rows, uint8_t* tmp, float* out, void* stream) {
  CLEAR_STALE();
  if (n < 1 || n > 65535 || H < 1 || W < 1 || (int64_t)H * W > 0x7fffffff / 3 || !image || !desc || kh < 1 || kv < 1 || !hb ||
      !hk || !vb || !vk || tmp_rows < 1 || tmp_rows > 0x7fffffff / CLIP_S - 1 || !tmp || !out)
    return OBJNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(clip_rows_kernel, dim3((unsigned)cdiv((int64_t)tmp_rows * CLIP_S, CC_WG), (unsigned)n), dim3(CC_WG), 0, st,
                     H, W, image, desc, kh, hb, hk, tmp_rows, tmp);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(clip_cols_kernel, dim3((unsigned)cdiv(CLIP_S * CLIP_S, CC_WG), (unsigned)n), dim3(CC_WG), 0, st, desc, kv,
                     vb, vk, tmp_rows, tmp, out);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

}  // extern "C"
