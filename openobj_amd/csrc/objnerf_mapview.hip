// A novel view of the WHOLE map in one launch chain (gfx950): the loop of train.py:550-612 (`cfg.if_render`) -- one
// sceneObject.render_2D_syn per object (vmap.py:604-685), each with its own box test over every pixel, its own launch and
// a z-buffer merge of four [W, H] images on the host (train.py:581-598) -- as three stages:
//
// 1. objnerf_view_rays_count / _emit: the candidate rays of ALL objects.  Pixel p = w * H + h of the transposed [W, H]
//    image is tested against box k with box_ray (objnerf_boxray.h, the function objnerf_box_rays runs); the hits of an
//    object become one segment of the candidate CSR of objnerf_segments.h over the objects in the caller's (dict)
//    order, ascending in p inside a segment, which is the order of the nonzero() in render_2D_syn.  An object with at
//    most one hit gets an EMPTY segment (n_rays <= 1, trainer.py:164-165 of the reference drops it): min_keep = 2.
// 2. objnerf_render_fwd_segmented: render_group (objnerf_render_body.h, the body objnerf_render_fwd runs) over the
//    segments of every hidden-32 object in ONE launch.  The work list is tiles (arena row, first 16-ray group, groups);
//    groups count from the segment's start, so ray r = entry - seg_lo is lane r & 15 of group r >> 4, the row of the
//    injected u and the Philox counter exactly as in the one-object kernel.  Workgroups are persistent: each takes a
//    contiguous share of the tile list and restages the LDS weight image only where the share crosses into another
//    row.  THE RESTAGE HAZARD: the four waves of a workgroup run their groups independently, so when the row changes
//    some waves may still be reading the old image out of LDS -- a workgroup barrier BEFORE stage_weights32 overwrites
//    it -- and no wave may start a group before every thread's part of the new image is written -- a barrier AFTER.
//    Both barriers sit under `row != staged`, which is uniform over the workgroup: every thread walks the same tiles
//    and reads the same row from the same address.  The per-wave group loop holds no barrier.
// 3. objnerf_view_merge: the reference's merge is a sequential fold in dict order in which a background object paints
//    colour and id but never depth.  Its closed form (render_view.merge_closed_form restates it in numpy):
//      an entry is OFFERED iff !((depth < near) | (depth > far) | (opacity < 0.9)) and depth < 100 (false for a NaN);
//      W(p) = the offered foreground entry of smallest depth, ties to the earliest object; depth(p) = depth_W or 100;
//      the painter of p = the LAST offered background entry after W's object with depth_b < depth_W (without W: the
//      last with depth_b < 100), otherwise W.
//    (a) merge_fg_kernel: atomicMin on best_fg [p] of  bits(depth + 0.0f) << 32 | entry  (depths are >= 0, so their
//        bits are monotone; + 0.0f folds -0; the CSR is in dict order, so the smaller entry is the earlier object);
//    (b) merge_bg_kernel: reads best_fg [p], applies the rule, atomicMax of entry + 1 on best_bg [p] (32 bits);
//    (c) merge_out_kernel: per pixel rgb u8 (float * 255, truncated: vmap.py:352 here), maskid, depth, winner.
//    Integer minima and maxima only: the result does not depend on the order the atomics arrive in.
// 4. objnerf_view_query: the 512-d part feature of the painted pixels from the feature hidden that
//    objnerf_render_fwd_segmented_feat composites in stage 2 -- cosines against query vectors, the label image and rows
//    for a pixel list, for the winners of stage 3 only; its banner stands ahead of its kernels below.
#include "objnerf_render_body.h"
#include "objnerf_boxray.h"
#include "objnerf_segments.h"

namespace {
using namespace obj32n;

constexpr int MV_WG = 256;            // pixels / entries per workgroup of the merge kernels
constexpr unsigned long long MV_NO_FG = ((unsigned long long)0x42C80000u << 32) | 0xFFFFFFFFull;   // bits(100.0f), no entry

int64_t mv_blocks(const int64_t n) { return cdiv(n, MV_WG); }

// -------------------------------------------------------------------------------------------------- 1. candidate rays
// box record: T_OC rows 0..2 [3][4] | extent / 2 [3] | unused
struct ViewRay {
  const float* T_WC; const float* boxes; const float* dirs_C;
  int32_t* pix; float* dirs_W; float* near_o; float* far_o;
  typedef BoxRay Payload;
  __device__ __forceinline__ bool hit(const int k, const int64_t p, BoxRay& b) const {
    const float* rec = boxes + (int64_t)k * SEG_BOX_FLOATS;
    b = box_ray(T_WC, rec, rec + 12, dirs_C[3 * p], dirs_C[3 * p + 1], dirs_C[3 * p + 2]);
    return b.hit;
  }
  __device__ __forceinline__ void store(const int64_t pos, const int64_t p, const BoxRay& b) const {
    pix[pos] = (int32_t)p;
    dirs_W[3 * pos] = b.dw[0]; dirs_W[3 * pos + 1] = b.dw[1]; dirs_W[3 * pos + 2] = b.dw[2];
    near_o[pos] = b.near_;
    far_o[pos] = b.far_;
  }
};

// ---------------------------------------------------------------------------------------------- 2. segmented render
struct SegRenderDev {
  int n_rows, n_bins; long n_tiles, M, u_rows;
  const float* params; long p_stride; const float* scale; const float* origin;
  const int64_t* rows;        // [n_rows][4]: seg_lo, seg_hi (entries of the CSR), u_lo (first row of u; < 0: seeded), draw
  const int32_t* tiles;       // [n_tiles][3]: arena row, first 16-ray group of the segment, groups
  const float* dirs_W; const float* near_; const float* far_; const float* u; uint64_t seed;
  float* depth; float* opacity; float* rgb;
  Layout L;
  float* hfeat;               // [M][32], CSR-aligned: the composited feature hidden (FEAT only)
};

// FEAT: the weight image carries the feature layer too (ROWS_FEAT rows, 73 KB: the launch opts in to that much dynamic
// LDS) and render_group<true> stores the composited 32-wide feature hidden of a ray to hfeat + 32 * entry
template <bool FEAT>
__global__ __launch_bounds__(256) void render_seg_kernel(const SegRenderDev a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const long t0 = a.n_tiles * (long)blockIdx.x / (long)gridDim.x, t1 = a.n_tiles * ((long)blockIdx.x + 1) / (long)gridDim.x;
  const float* sv = lds + sv_base(FEAT);
  const float* wf = (const float*)__builtin_assume_aligned(lds + 4 * g * WROW + out_pos(c), 8);
  const float ox = a.origin[0], oy = a.origin[1], oz = a.origin[2];
  const int S = a.n_bins - 1;
  RenderDev d;
  d.n = 0; d.n_bins = a.n_bins; d.G = 0;
  d.params = nullptr; d.scale = nullptr; d.origin = a.origin;
  d.dirs_W = nullptr; d.near_ = nullptr; d.far_ = nullptr; d.u = nullptr; d.seed = a.seed; d.draw = 0;
  d.depth = nullptr; d.opacity = nullptr; d.rgb = nullptr; d.hfeat = nullptr; d.z_out = nullptr;
  d.L = a.L;
  int staged = -1;
  float scale = 1.0f;
  uint32_t st = 0;
  for (long t = t0; t < t1; ++t) {
    // every thread reads the same three words: row, first and ng are uniform over the workgroup
    const int row = __builtin_amdgcn_readfirstlane(a.tiles[3 * t]);
    const int first = __builtin_amdgcn_readfirstlane(a.tiles[3 * t + 1]);
    const int ng = __builtin_amdgcn_readfirstlane(a.tiles[3 * t + 2]);
    if (row < 0 || row >= a.n_rows || first < 0) continue;
    if (row != staged) {
      __syncthreads();        // every wave is done reading the image of the row before (banner: the restage hazard)
      stage_weights32(lds, a.params + (long)row * a.p_stride, a.L, FEAT, tid, 256);
      __syncthreads();        // the new image is complete before any wave's next group reads it
      const int64_t* rr = a.rows + 4 * (long)row;
      long s0 = rr[0], s1 = rr[1];
      const long ulo = rr[2];
      s0 = s0 < 0 ? 0 : (s0 > a.M ? a.M : s0);              // a segment never leaves the CSR
      s1 = s1 < s0 ? s0 : (s1 > a.M ? a.M : s1);
      const bool inj = a.u != nullptr && ulo >= 0;
      if (inj && ulo + (s1 - s0) > a.u_rows) s1 = s0;        // nor its draws the rows of u: such a row renders nothing
      d.n = s1 - s0;
      d.dirs_W = a.dirs_W + 3 * s0; d.near_ = a.near_ + s0; d.far_ = a.far_ + s0;
      d.u = inj ? a.u + ulo * a.n_bins : nullptr;
      d.draw = (uint32_t)rr[3];
      d.depth = a.depth + s0; d.opacity = a.opacity + s0; d.rgb = a.rgb + 3 * s0;
      if (FEAT) d.hfeat = a.hfeat + 32 * s0;
      scale = a.scale[row];
      st = objrng::S_BOX_U | (d.draw << 3);
      staged = row;
    }
    if (d.n <= 0) continue;
    for (int gi = w; gi < ng; gi += 4)                       // a wave's groups; no barrier in here
      if (((long)first + gi) * 16 < d.n) render_group<FEAT>(d, sv, wf, scale, ox, oy, oz, S, st, c, g, (long)first + gi);
  }
}

// ------------------------------------------------------------------------------------------------------- 3. merge
// vmap.py:350 here (the masks of vmap.py:665,672) and the 100 the depth image starts from (train.py:566)
__device__ __forceinline__ bool mv_offered(const float d, const float op, const float nr, const float fr) {
  return !((d < nr) | (d > fr) | (op < 0.9f)) && d < 100.0f;
}

struct MergeDev {
  int64_t P, M; int K;
  const int64_t* seg_off; const int32_t* pix;
  const float* depth; const float* opacity; const float* rgb; const float* near_; const float* far_;
  const int32_t* info;        // [K][2]: background, the id written into maskid
  unsigned long long* best_fg; unsigned int* best_bg;
  uint8_t* out_rgb; int32_t* out_maskid; float* out_depth; int32_t* out_winner;
};

__global__ void __launch_bounds__(MV_WG) merge_init_kernel(const int64_t P, unsigned long long* __restrict__ best_fg,
                                                           unsigned int* __restrict__ best_bg) {
  const int64_t p = (int64_t)blockIdx.x * MV_WG + threadIdx.x;
  if (p < P) { best_fg[p] = MV_NO_FG; best_bg[p] = 0u; }
}
template <bool BG>
__global__ void __launch_bounds__(MV_WG) merge_entry_kernel(const MergeDev a) {
  const int64_t e = (int64_t)blockIdx.x * MV_WG + threadIdx.x;
  if (e >= a.M) return;
  const int k = seg_of(a.seg_off, a.K, e);
  if ((a.info[2 * k] != 0) != BG) return;
  const int64_t p = a.pix[e];
  if (p < 0 || p >= a.P) return;
  const float d = a.depth[e];
  if (!mv_offered(d, a.opacity[e], a.near_[e], a.far_[e])) return;
  const unsigned int bits = __float_as_uint(d + 0.0f);
  if (!BG) {
    atomicMin(a.best_fg + p, ((unsigned long long)bits << 32) | (unsigned long long)(unsigned int)e);
  } else {
    // best_fg is final: launch (a) is complete before this one starts on the stream
    const unsigned long long key = a.best_fg[p];
    const unsigned int ew = (unsigned int)key;
    const float dw = __uint_as_float((unsigned int)(key >> 32));
    const bool after = ew == 0xFFFFFFFFu || (unsigned int)e > ew;        // b's object comes after W's in dict order
    if (after && (d + 0.0f) < dw) atomicMax(a.best_bg + p, (unsigned int)e + 1u);
  }
}
__global__ void __launch_bounds__(MV_WG) merge_out_kernel(const MergeDev a) {
  const int64_t p = (int64_t)blockIdx.x * MV_WG + threadIdx.x;
  if (p >= a.P) return;
  const unsigned long long key = a.best_fg[p];
  const unsigned int ew = (unsigned int)key, eb = a.best_bg[p];
  const int64_t e = eb != 0u ? (int64_t)eb - 1 : (ew != 0xFFFFFFFFu ? (int64_t)ew : -1);
  a.out_depth[p] = __uint_as_float((unsigned int)(key >> 32));
  a.out_winner[p] = (int32_t)e;
  const bool painted = e >= 0 && e < a.M;
  a.out_maskid[p] = painted ? a.info[2 * seg_of(a.seg_off, a.K, e) + 1] : 0;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    a.out_rgb[3 * p + j] = painted ? (uint8_t)(int)(a.rgb[3 * e + j] * 255.0f) : (uint8_t)0;      // truncation
}

// ------------------------------------------------------------------------------------ 4. part features and queries
// The 512-d part feature of a pixel is  F = of_w . h + of_b * opacity  of the entry that PAINTED it (vmap.py:678: the head
// is linear, so it is applied after compositing and after the merge), h the composited feature hidden of stage 2.
// Only the winners are evaluated, and F never reaches memory unless a pixel list asks for rows of it.
//
// An item is an entry of the CSR (query pass) or a row of the pixel list (feature pass); a wave takes 16 items at a time
// (lane c <-> item, lane group g <-> rows 4 g + r, as in objnerf_mlp32.h) from a contiguous share of all items.  An item is
// LIVE iff the entry is the winner of its pixel and its object's head serves it (vq_server); a 16-item chunk without a
// live lane costs one ballot.  The live lanes of a chunk are served object by object (in the CSR a chunk straddles an
// object boundary at most K - 1 times per view; a pixel list is in any order).
//
// Per object and 16 channels:  F^T block [16 channels][16 items] = of_w block [16][H] . h^T [H][16]  on
// v_mfma_f32_16x16x4_f32 with k-step (T, r) <-> hidden feature 16 T + 4 g + r: the A operand is of_w [16 cb + c][that
// feature] (one 128-bit load per T and lane, 16 rows of of_w back to back: whole cache lines), the B operand h of item c
// (held in registers for all C / 16 blocks).  The accumulator of that product has channel 16 cb + 4 g + r of item c in
// register r -- the B operand layout of a k-step of the SECOND product  dot [16 queries][16 items] += queries [q][those
// 16 channels] . F^T block, whose A operand is queries [q = c][16 cb + 4 g + r] out of LDS (padded to 16 queries with
// zero rows, row pitch C + 4 floats).  The squares of the block go into a per-lane partial of |F|^2, summed over the lane
// groups at the end.  No LDS round trip between the products.  The order of every sum is fixed by this sequence and an
// item's column of an MFMA depends on no other column: the outputs do not depend on the grid or on which items share a
// chunk.
//
// The heads are NOT staged in LDS: the hidden-128 background's is 256 KB (it does not fit), a hidden-32 object's 64 KB
// (one workgroup per CU), and every chunk reads all of it exactly once -- as A operands it streams through L2 instead,
// so there is no restage and no barrier in the item loop.
constexpr int VQ_QPAD = 4;            // floats of padding per query row in LDS

struct ViewQueryDev {
  int64_t P, M, n_items; int K, C, Q;
  const int64_t* seg_off; const int32_t* pix; const float* opacity; const int32_t* winner;
  const objnerf_view_head_obj* heads; const float* queries; const int32_t* feat_pix;
  float* out_sim; int32_t* out_label; float* out_best; float* out_feat;
};

__device__ __forceinline__ bool vq_width_built(const int H) { return H == 32 || H == 64 || H == 128; }
// the object of entry e if its head serves e, else -1
__device__ __forceinline__ int vq_server(const ViewQueryDev& a, const int64_t e) {
  const int k = seg_of(a.seg_off, a.K, e);
  const objnerf_view_head_obj& h = a.heads[k];
  const int64_t rel = e - h.row0;
  return (h.of_w && h.of_b && h.hfeat && vq_width_built(h.H) && rel >= 0 && rel < h.n_rows) ? k : -1;
}
// the entry that painted pixel p, or -1 (winner holds the low 32 bits of an entry, all ones = none; M < 2^32)
__device__ __forceinline__ int64_t vq_entry_of_pixel(const ViewQueryDev& a, const int64_t p) {
  if (p < 0 || p >= a.P) return -1;
  const int64_t w = (int64_t)(uint32_t)a.winner[p];
  return (w < a.M && (int64_t)a.pix[w] == p) ? w : -1;
}
// np.argmax's order: a NaN is above every number
__device__ __forceinline__ bool vq_above(const float x, const float y) { return x > y || (x != x && y == y); }

// the lanes `mine` of one chunk, all of object hd: e their entries, dst the pixel (query pass) or the row (LIST)
template <int HW, bool LIST>
__device__ __forceinline__ void vq_body(const ViewQueryDev& a, const float* qs, const objnerf_view_head_obj& hd,
                                        const bool mine, const int64_t e, const int64_t dst, const int c, const int g) {
  f32x4 hb[HW / 16];
#pragma unroll
  for (int T = 0; T < HW / 16; ++T) hb[T] = zero4();
  float op = 0.0f;
  if (mine) {
    const float* hr = hd.hfeat + (e - hd.row0) * HW + 4 * g;
#pragma unroll
    for (int T = 0; T < HW / 16; ++T) hb[T] = *reinterpret_cast<const f32x4*>(hr + 16 * T);
    op = a.opacity[e];
  }
  const float* wa = hd.of_w + (int64_t)c * HW + 4 * g;
  const float* qa = qs + c * (a.C + VQ_QPAD) + 4 * g;
  f32x4 dot = zero4();
  float n2 = 0.0f;
  for (int cb = 0; cb < a.C / 16; ++cb) {
    const float* wr = wa + (int64_t)cb * 16 * HW;
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(hd.of_b + 16 * cb + 4 * g);
    f32x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = b4[r] * op;
#pragma unroll
    for (int T = 0; T < HW / 16; ++T) {
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(wr + 16 * T);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc = OBJ_MFMA(w4[r], hb[T][r], acc);
    }
    if (LIST) {
      if (mine) *reinterpret_cast<f32x4*>(a.out_feat + dst * a.C + 16 * cb + 4 * g) = acc;
    } else {
      const f32x4 q4 = *reinterpret_cast<const f32x4*>(qa + 16 * cb);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        n2 = fmaf(acc[r], acc[r], n2);
        dot = OBJ_MFMA(q4[r], acc[r], dot);
      }
    }
  }
  if (LIST) return;
  const float den = fmaxf(sqrtf(xgroup_sum(n2)), 1e-8f);         // objnerf_project's cosine convention
  float bv = 0.0f;
  int bq = 1 << 20;                                             // (no query yet)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = 4 * g + r;
    const float s = dot[r] / den;
    if (q < a.Q) {
      if (mine && a.out_sim) a.out_sim[(int64_t)q * a.P + dst] = s;
      if (bq == (1 << 20) || vq_above(s, bv)) { bv = s; bq = q; }            // (q ascends: equal values keep the first)
    }
  }
  // the first arg-max over the four lane groups of the item: the larger value, equal values to the smaller q
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oq = __shfl_xor(bq, off, 64);
    const bool take = oq < (1 << 20) && (bq == (1 << 20) || vq_above(ov, bv) || (!vq_above(bv, ov) && oq < bq));
    bv = take ? ov : bv;
    bq = take ? oq : bq;
  }
  if (mine && g == 0) {
    if (a.out_label) a.out_label[dst] = bq;
    if (a.out_best) a.out_best[dst] = bv;
  }
}

template <bool LIST>
__global__ __launch_bounds__(256) void view_query_kernel(const ViewQueryDev a) {
  extern __shared__ __attribute__((aligned(16))) float qs[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  if (!LIST) {
    const int pitch = a.C + VQ_QPAD;
    for (int i = tid; i < 16 * pitch; i += 256) {
      const int q = i / pitch, ch = i - q * pitch;
      qs[i] = (q < a.Q && ch < a.C) ? a.queries[(int64_t)q * a.C + ch] : 0.0f;
    }
    __syncthreads();                                             // the only barrier: the item loop holds none
  }
  const long nch = (long)((a.n_items + 15) / 16), nw = (long)gridDim.x * 4, wv = (long)blockIdx.x * 4 + w;
  const long ch1 = nch * (wv + 1) / nw;
  for (long ch = nch * wv / nw; ch < ch1; ++ch) {
    const int64_t item = (int64_t)ch * 16 + c;
    int64_t e = -1, dst = item;
    int k = -1;
    if (item < a.n_items) {
      if (LIST) {
        e = vq_entry_of_pixel(a, (int64_t)a.feat_pix[item]);
      } else {
        const int64_t p = a.pix[item];
        if (p >= 0 && p < a.P && (uint32_t)a.winner[p] == (uint32_t)item) { e = item; dst = p; }
      }
      if (e >= 0) k = vq_server(a, e);
    }
    unsigned long long todo = __ballot(k >= 0);
    while (todo) {                                               // (uniform over the wave)
      const int kk = __builtin_amdgcn_readlane(k, __ffsll(todo) - 1);
      const objnerf_view_head_obj hd = a.heads[kk];
      const bool mine = k == kk;
      const int Hk = __builtin_amdgcn_readfirstlane(hd.H);
      if (Hk == 32) vq_body<32, LIST>(a, qs, hd, mine, e, dst, c, g);
      else if (Hk == 64) vq_body<64, LIST>(a, qs, hd, mine, e, dst, c, g);
      else vq_body<128, LIST>(a, qs, hd, mine, e, dst, c, g);   // (vq_server admits no other width)
      todo &= ~__ballot(mine);
    }
    if (LIST && item < a.n_items && k < 0) {                     // a row without a served painter: zeros
      float* row = a.out_feat + item * a.C + 4 * g;
      for (int cb = 0; cb < a.C / 16; ++cb) *reinterpret_cast<f32x4*>(row + 16 * cb) = zero4();
    }
  }
}
// one thread per pixel: exactly the pixels no live entry writes
__global__ void __launch_bounds__(MV_WG) view_query_fill_kernel(const ViewQueryDev a) {
  const int64_t p = (int64_t)blockIdx.x * MV_WG + threadIdx.x;
  if (p >= a.P) return;
  const int64_t e = vq_entry_of_pixel(a, p);
  if (e >= 0 && vq_server(a, e) >= 0) return;
  const float nan = __uint_as_float(0x7FC00000u);
  if (a.out_sim)
    for (int q = 0; q < a.Q; ++q) a.out_sim[(int64_t)q * a.P + p] = nan;
  if (a.out_label) a.out_label[p] = -1;
  if (a.out_best) a.out_best[p] = nan;
}

}  // namespace

extern "C" {

size_t objnerf_view_rays_workspace_bytes(int64_t P, int32_t K) { return seg_csr_workspace_bytes(P, K); }

int objnerf_view_rays_count(int64_t P, int32_t K, const float* T_WC, const float* boxes, const float* dirs_C, void* ws,
                            size_t ws_bytes, int64_t* seg_off, void* stream) {
  (void)hipGetLastError();
  if (!seg_sizes_ok(P, K) || !T_WC || !boxes || !dirs_C || !ws || !seg_off) return OBJNERF_EINVAL;
  if (ws_bytes < seg_csr_workspace_bytes(P, K)) return OBJNERF_EINVAL;
  return seg_csr_count(P, K, ViewRay{T_WC, boxes, dirs_C, nullptr, nullptr, nullptr, nullptr}, 2, ws, seg_off,
                       (hipStream_t)stream);
}

int objnerf_view_rays_emit(int64_t P, int32_t K, const float* T_WC, const float* boxes, const float* dirs_C, const void* ws,
                           size_t ws_bytes, int64_t M, int32_t* pix, float* dirs_W, float* near, float* far, void* stream) {
  (void)hipGetLastError();
  if (!seg_sizes_ok(P, K) || !T_WC || !boxes || !dirs_C || !ws || M < 0 || M >= (1LL << 32)) return OBJNERF_EINVAL;
  if (ws_bytes < seg_csr_workspace_bytes(P, K)) return OBJNERF_EINVAL;
  if (M == 0) return OBJNERF_OK;
  if (!pix || !dirs_W || !near || !far) return OBJNERF_EINVAL;
  return seg_csr_emit(P, K, ViewRay{T_WC, boxes, dirs_C, pix, dirs_W, near, far}, ws, M, (hipStream_t)stream);
}

// both entries of the segmented renderer: out_hfeat selects the instantiation
static int render_fwd_segmented(const objnerf_net* net, int32_t n_rows, int64_t n_tiles, int32_t n_bins, int64_t M,
                                const float* params, int64_t p_stride, const float* scale, const float* origin,
                                const int64_t* rows, const int32_t* tiles, const float* dirs_W, const float* near,
                                const float* far, const float* u, int64_t u_rows, uint64_t seed, float* out_depth,
                                float* out_opacity, float* out_rgb, float* out_hfeat, int32_t workgroups, void* stream) {
  (void)hipGetLastError();
  if (!net || n_rows <= 0 || n_tiles < 0 || n_bins < 2 || M < 0 || M >= (1LL << 32) || p_stride <= 0 || workgroups < 0 ||
      u_rows < 0)
    return OBJNERF_EINVAL;
  if (net->hidden != 32 || net->n_freqs != 6) return OBJNERF_ENOTSUP;      // (wider networks: the layer-wise chain)
  if (n_tiles == 0 || M == 0) return OBJNERF_OK;
  if (!params || !scale || !origin || !rows || !tiles || !dirs_W || !near || !far || !out_depth || !out_opacity || !out_rgb)
    return OBJNERF_EINVAL;
  SegRenderDev d;
  d.n_rows = n_rows; d.n_bins = n_bins; d.n_tiles = (long)n_tiles; d.M = (long)M; d.u_rows = u ? (long)u_rows : 0;
  d.params = params; d.p_stride = (long)p_stride; d.scale = scale; d.origin = origin; d.rows = rows; d.tiles = tiles;
  d.dirs_W = dirs_W; d.near_ = near; d.far_ = far; d.u = u; d.seed = seed;
  d.depth = out_depth; d.opacity = out_opacity; d.rgb = out_rgb; d.hfeat = out_hfeat;
  d.L = make_layout(net->feat_dim);
  // two workgroups of 4 waves per CU (the image is 60 KB; 73 KB with the feature layer), never more than there are tiles
  int64_t G = workgroups > 0 ? (int64_t)workgroups : 2 * (int64_t)objnerf_num_cu();
  if (G > n_tiles) G = n_tiles;
  if (out_hfeat) {
    // 73 KB of dynamic LDS is above the 64 KB a kernel gets without asking
    objnerf_once_per_device([] {
      (void)hipFuncSetAttribute((const void*)render_seg_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                img_floats(true) * 4);
    });
    hipLaunchKernelGGL(render_seg_kernel<true>, dim3((unsigned)G), dim3(256), (size_t)img_floats(true) * 4,
                       (hipStream_t)stream, d);
  } else {
    hipLaunchKernelGGL(render_seg_kernel<false>, dim3((unsigned)G), dim3(256), (size_t)img_floats(false) * 4,
                       (hipStream_t)stream, d);
  }
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_render_fwd_segmented(const objnerf_net* net, int32_t n_rows, int64_t n_tiles, int32_t n_bins, int64_t M,
                                 const float* params, int64_t p_stride, const float* scale, const float* origin,
                                 const int64_t* rows, const int32_t* tiles, const float* dirs_W, const float* near,
                                 const float* far, const float* u, int64_t u_rows, uint64_t seed, float* out_depth,
                                 float* out_opacity, float* out_rgb, int32_t workgroups, void* stream) {
  return render_fwd_segmented(net, n_rows, n_tiles, n_bins, M, params, p_stride, scale, origin, rows, tiles, dirs_W, near,
                              far, u, u_rows, seed, out_depth, out_opacity, out_rgb, nullptr, workgroups, stream);
}

int objnerf_render_fwd_segmented_feat(const objnerf_net* net, int32_t n_rows, int64_t n_tiles, int32_t n_bins, int64_t M,
                                      const float* params, int64_t p_stride, const float* scale, const float* origin,
                                      const int64_t* rows, const int32_t* tiles, const float* dirs_W, const float* near,
                                      const float* far, const float* u, int64_t u_rows, uint64_t seed, float* out_depth,
                                      float* out_opacity, float* out_rgb, float* out_hfeat, int32_t workgroups,
                                      void* stream) {
  if (!out_hfeat && n_tiles > 0 && M > 0) return OBJNERF_EINVAL;
  return render_fwd_segmented(net, n_rows, n_tiles, n_bins, M, params, p_stride, scale, origin, rows, tiles, dirs_W, near,
                              far, u, u_rows, seed, out_depth, out_opacity, out_rgb, out_hfeat, workgroups, stream);
}

// the workgroups of render_seg_kernel the runtime places on one compute unit (0: the query failed)
int objnerf_render_fwd_segmented_occupancy(int32_t with_hfeat) {
  int n = 0;
  const size_t lds = (size_t)img_floats(with_hfeat != 0) * 4;
  if (with_hfeat)
    (void)hipFuncSetAttribute((const void*)render_seg_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const hipError_t e = with_hfeat
      ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)render_seg_kernel<true>, 256, lds)
      : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)render_seg_kernel<false>, 256, lds);
  (void)hipGetLastError();
  return e == hipSuccess ? n : 0;
}

int objnerf_view_merge(int64_t P, int32_t K, int64_t M, const int64_t* seg_off, const int32_t* pix, const float* depth,
                       const float* opacity, const float* rgb, const float* near, const float* far, const int32_t* info,
                       int32_t any_background, uint64_t* best_fg, uint32_t* best_bg, uint8_t* out_rgb, int32_t* out_maskid,
                       float* out_depth, int32_t* out_winner, void* stream) {
  (void)hipGetLastError();
  if (!seg_sizes_ok(P, K) || M < 0 || M >= (1LL << 32) || !seg_off || !info || !best_fg || !best_bg || !out_rgb ||
      !out_maskid || !out_depth || !out_winner)
    return OBJNERF_EINVAL;
  if (M > 0 && (!pix || !depth || !opacity || !rgb || !near || !far)) return OBJNERF_EINVAL;
  MergeDev a;
  a.P = P; a.M = M; a.K = K; a.seg_off = seg_off; a.pix = pix; a.depth = depth; a.opacity = opacity; a.rgb = rgb;
  a.near_ = near; a.far_ = far; a.info = info; a.best_fg = (unsigned long long*)best_fg; a.best_bg = best_bg;
  a.out_rgb = out_rgb; a.out_maskid = out_maskid; a.out_depth = out_depth; a.out_winner = out_winner;
  hipStream_t st = (hipStream_t)stream;
  const dim3 wg(MV_WG), gp((unsigned)mv_blocks(P)), ge((unsigned)mv_blocks(M > 0 ? M : 1));
  hipLaunchKernelGGL(merge_init_kernel, gp, wg, 0, st, P, a.best_fg, a.best_bg);
  CHECK_LAUNCH();
  if (M > 0) {
    hipLaunchKernelGGL((merge_entry_kernel<false>), ge, wg, 0, st, a);
    CHECK_LAUNCH();
    if (any_background) {
      hipLaunchKernelGGL((merge_entry_kernel<true>), ge, wg, 0, st, a);
      CHECK_LAUNCH();
    }
  }
  hipLaunchKernelGGL(merge_out_kernel, gp, wg, 0, st, a);
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

int objnerf_view_query(int64_t P, int32_t K, int64_t M, int32_t C, int32_t Q, const int64_t* seg_off, const int32_t* pix,
                       const float* opacity, const int32_t* winner, const objnerf_view_head_obj* heads,
                       const objnerf_view_head_obj* heads_host, const float* queries, float* out_sim, int32_t* out_label,
                       float* out_best, int64_t n_feat, const int32_t* feat_pix, float* out_feat, int32_t workgroups,
                       void* stream) {
  (void)hipGetLastError();
  if (Q < 1 || Q > 16 || M < 0 || M >= (1LL << 32) || !seg_sizes_ok(P, K) || C <= 0 || n_feat < 0 || workgroups < 0)
    return OBJNERF_EINVAL;
  if (!seg_off || !winner || !heads || !heads_host || (M > 0 && (!pix || !opacity))) return OBJNERF_EINVAL;
  const bool ask = out_sim || out_label || out_best;
  if ((ask && !queries) || (n_feat > 0 && (!feat_pix || !out_feat))) return OBJNERF_EINVAL;
  auto misaligned = [](const void* p) { return ((uintptr_t)p & 15) != 0; };        // (128-bit loads; NULL passes)
  bool built = C % 16 == 0 && (size_t)16 * (size_t)(C + VQ_QPAD) * 4 <= 64 * 1024;
  for (int k = 0; k < K; ++k) {
    const objnerf_view_head_obj& h = heads_host[k];
    if (h.H <= 0 || h.H % 32 != 0 || h.n_rows < 0 || misaligned(h.of_w) || misaligned(h.of_b) || misaligned(h.hfeat))
      return OBJNERF_EINVAL;
    if (h.H != 32 && h.H != 64 && h.H != 128) built = false;
  }
  if (!built) return OBJNERF_ENOTSUP;
  ViewQueryDev a;
  a.P = P; a.M = M; a.K = K; a.C = C; a.Q = Q; a.seg_off = seg_off; a.pix = pix; a.opacity = opacity; a.winner = winner;
  a.heads = heads; a.queries = queries; a.feat_pix = feat_pix;
  a.out_sim = out_sim; a.out_label = out_label; a.out_best = out_best; a.out_feat = out_feat;
  hipStream_t st = (hipStream_t)stream;
  // four workgroups of 4 waves per CU (33 KB of LDS each at C = 512), never more waves than 16-item chunks
  auto grid = [&](const int64_t items) {
    int64_t G = workgroups > 0 ? (int64_t)workgroups : 4 * (int64_t)objnerf_num_cu();
    const int64_t need = cdiv(cdiv(items, 16), 4);
    return dim3((unsigned)(G > need ? need : G));
  };
  if (ask) {
    a.n_items = M;
    hipLaunchKernelGGL(view_query_fill_kernel, dim3((unsigned)mv_blocks(P)), dim3(MV_WG), 0, st, a);
    CHECK_LAUNCH();
    if (M > 0) {
      hipLaunchKernelGGL(view_query_kernel<false>, grid(M), dim3(256), (size_t)16 * (size_t)(C + VQ_QPAD) * 4, st, a);
      CHECK_LAUNCH();
    }
  }
  if (n_feat > 0) {
    a.n_items = n_feat;
    hipLaunchKernelGGL(view_query_kernel<true>, grid(n_feat), dim3(256), 0, st, a);
    CHECK_LAUNCH();
  }
  return OBJNERF_OK;
}

}  // extern "C"
