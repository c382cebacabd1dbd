// The compact exported map: a vertex's unit part feature f^ = (W h + b) / max(|W h + b|, 1e-8) is
// linear in the row  r = [h s, s],  s = 1 / max(|W h + b|, 1e-8):  f^ = A r  with  A = [W | b]  ([C][H + 1]).
//
//   part_kernel<HW, false>   objnerf_part_rows: rows [V][H + 1] from the feature hidden [V][H] and one object's head;
//   part_kernel<HW, true>    objnerf_part_expand: out [n][C] = A r of chosen rows (an index outside [0, V): zeros).
//
// Both are the first product of objnerf_view_query (objnerf_mapview.hip, section 4): a wave takes 16 items at a time
// (lane c <-> item, lane group g <-> rows 4 g + e of an accumulator); per 16 channels
//   F^T block [16 channels][16 items] = A block [16][H] . h^T [H][16]   on v_mfma_f32_16x16x4_f32,
// k-step (T, e) <-> hidden feature 16 T + 4 g + e: the A operand is the head's row 16 cb + c at that feature (one 128-bit
// load per T and lane where the head's rows are 16-byte aligned, as of_w's are), the B operand h of item c, held in
// registers for all C / 16 blocks.  The accumulator starts at b (times s for the expansion) and ends with channel
// 16 cb + 4 g + e of item c in element e.  For the rows its squares go into a per-lane partial of |f|^2, summed over
// the four lane groups at the end; the 512-d vector never reaches memory.  A wave keeps NB chunks of 16 items in
// registers per pass over the head (NB x H <= 256 floats a lane), so the head streams through L2 once per 16 NB items.
// Every output location has one writer and the order of every sum is fixed by this sequence: an item's results depend
// on nothing but its own inputs, two calls write the same bytes.  No atomics, no LDS, no barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include "objnerf_wg.h"

namespace {

constexpr int PR_WG = 256;                      // 4 waves
constexpr int PR_MAX_WG = 4096;

struct PartDev {
  int64_t V, n;                                 // rows of src; items (part_rows: n = V)
  int C;
  const float* src; int64_t src_stride;         // hfeat [V][H] (part_rows) or rows [V][H + 1] (part_expand)
  const float* w; int64_t w_pitch;              // head row c: w + c * w_pitch, H floats
  const float* bias; int64_t bias_stride;       // head bias of channel c: bias[c * bias_stride]
  const int64_t* index;                         // part_expand: item -> row, or NULL (item i is row i)
  float* out; int64_t out_stride;
  int vec_src, vec_w, vec_out;                  // 128-bit accesses are whole and aligned
};

template <int HW> struct PartNb { static constexpr int v = HW <= 64 ? 4 : (HW <= 128 ? 2 : 1); };

__device__ __forceinline__ floatx4 pr_ld4(const float* __restrict__ p, const bool vec) {
  if (vec) return *reinterpret_cast<const floatx4*>(p);
  return floatx4{p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ void pr_st4(float* __restrict__ p, const floatx4 v, const bool vec) {
  if (vec) { *reinterpret_cast<floatx4*>(p) = v; return; }
  p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
}

template <int HW, bool EXPAND>
__global__ void __launch_bounds__(PR_WG) part_kernel(const PartDev a) {
  constexpr int NB = PartNb<HW>::v, NT = HW / 16;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int64_t ngroups = (a.n + 16 * NB - 1) / (16 * NB);
  for (int64_t grp = (int64_t)blockIdx.x * (PR_WG / 64) + wv; grp < ngroups; grp += (int64_t)gridDim.x * (PR_WG / 64)) {
    floatx4 hb[NB][NT];
    float op[NB], n2[NB];
    int64_t item[NB], row[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      item[b] = (grp * NB + b) * 16 + c;
      row[b] = -1;
      if (item[b] < a.n) {
        const int64_t idx = (EXPAND && a.index) ? a.index[item[b]] : item[b];
        if (idx >= 0 && idx < a.V) row[b] = idx;
      }
      op[b] = EXPAND ? 0.f : 1.f;
      n2[b] = 0.f;
#pragma unroll
      for (int T = 0; T < NT; ++T) hb[b][T] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (row[b] >= 0) {
        const float* p = a.src + row[b] * a.src_stride;
#pragma unroll
        for (int T = 0; T < NT; ++T) hb[b][T] = pr_ld4(p + 16 * T + 4 * g, a.vec_src != 0);
        if (EXPAND) op[b] = p[HW];
      }
    }
    for (int cb = 0; cb < a.C / 16; ++cb) {
      const float* wr = a.w + (int64_t)(16 * cb + c) * a.w_pitch + 4 * g;
      floatx4 w4[NT];
#pragma unroll
      for (int T = 0; T < NT; ++T) w4[T] = pr_ld4(wr + 16 * T, a.vec_w != 0);
      float bb[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) bb[e] = a.bias[(int64_t)(16 * cb + 4 * g + e) * a.bias_stride];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        floatx4 acc;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = EXPAND ? bb[e] * op[b] : bb[e];
#pragma unroll
        for (int T = 0; T < NT; ++T)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[T][e], hb[b][T][e], acc, 0, 0, 0);
        if (EXPAND) {
          if (item[b] < a.n)
            pr_st4(a.out + item[b] * a.out_stride + 16 * cb + 4 * g,
                   row[b] >= 0 ? acc : floatx4{0.f, 0.f, 0.f, 0.f}, a.vec_out != 0);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) n2[b] = fmaf(acc[e], acc[e], n2[b]);
        }
      }
    }
    if (EXPAND) continue;
#pragma unroll
    for (int b = 0; b < NB; ++b) {                          // lanes c, c + 16, c + 32, c + 48 hold item c's parts
      float t = n2[b];
      t += __shfl_xor(t, 16);
      t += __shfl_xor(t, 32);
      const float s = 1.0f / fmaxf(sqrtf(t), 1e-8f);
      if (row[b] < 0) continue;
      float* o = a.out + row[b] * a.out_stride;
#pragma unroll
      for (int T = 0; T < NT; ++T) {
        floatx4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = hb[b][T][e] * s;
        pr_st4(o + 16 * T + 4 * g, v, a.vec_out != 0);
      }
      if (g == 0) {
        o[HW] = s;
        for (int64_t k = HW + 1; k < a.out_stride && k < HW + 4; ++k) o[k] = 0.f;   // the alignment padding: defined bytes
      }
    }
  }
}

template <bool EXPAND>
int part_launch(const PartDev& a, const int H, hipStream_t st) {
  const int nb = H <= 64 ? 4 : (H <= 128 ? 2 : 1);      // PartNb<H>::v
  const int64_t ngroups = cdiv(a.n, 16 * nb);
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(ngroups, PR_WG / 64), PR_MAX_WG)));
  switch (H) {
    case 32: hipLaunchKernelGGL((part_kernel<32, EXPAND>), grid, dim3(PR_WG), 0, st, a); break;
    case 64: hipLaunchKernelGGL((part_kernel<64, EXPAND>), grid, dim3(PR_WG), 0, st, a); break;
    case 96: hipLaunchKernelGGL((part_kernel<96, EXPAND>), grid, dim3(PR_WG), 0, st, a); break;
    case 128: hipLaunchKernelGGL((part_kernel<128, EXPAND>), grid, dim3(PR_WG), 0, st, a); break;
    case 160: hipLaunchKernelGGL((part_kernel<160, EXPAND>), grid, dim3(PR_WG), 0, st, a); break;
    case 192: hipLaunchKernelGGL((part_kernel<192, EXPAND>), grid, dim3(PR_WG), 0, st, a); break;
    case 224: hipLaunchKernelGGL((part_kernel<224, EXPAND>), grid, dim3(PR_WG), 0, st, a); break;
    case 256: hipLaunchKernelGGL((part_kernel<256, EXPAND>), grid, dim3(PR_WG), 0, st, a); break;
    default: return OBJNERF_ENOTSUP;
  }
  CHECK_LAUNCH();
  return OBJNERF_OK;
}

inline bool part_widths_built(const int H, const int C) {
  return H >= 32 && H <= 256 && H % 32 == 0 && C >= 16 && C <= 1024 && C % 16 == 0;
}
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int objnerf_part_rows(int64_t V, int32_t H, int32_t C, const float* hfeat, int64_t hfeat_stride, const float* of_w,
                      const float* of_b, float* rows, int64_t row_stride_out, void* stream) {
  if (V < 0 || H < 1 || C < 1) return OBJNERF_EINVAL;
  if (!part_widths_built(H, C)) return OBJNERF_ENOTSUP;
  if (!of_w || !of_b || hfeat_stride < H || row_stride_out < H + 1) return OBJNERF_EINVAL;
  if (V == 0) return OBJNERF_OK;
  if (!hfeat || !rows) return OBJNERF_EINVAL;
  PartDev a{};
  a.V = V; a.n = V; a.C = C;
  a.src = hfeat; a.src_stride = hfeat_stride;
  a.w = of_w; a.w_pitch = H; a.bias = of_b; a.bias_stride = 1;
  a.index = nullptr; a.out = rows; a.out_stride = row_stride_out;
  a.vec_src = al16(hfeat) && hfeat_stride % 4 == 0;
  a.vec_w = al16(of_w);                                   // (H is a multiple of 32: every row starts aligned)
  a.vec_out = al16(rows) && row_stride_out % 4 == 0;
  return part_launch<false>(a, H, (hipStream_t)stream);
}

int objnerf_part_expand(int64_t V, int32_t H, int32_t C, const float* rows, int64_t row_stride, const float* head,
                        int64_t n, const int64_t* index, float* out, void* stream) {
  if (V < 0 || n < 0 || H < 1 || C < 1) return OBJNERF_EINVAL;
  if (!part_widths_built(H, C)) return OBJNERF_ENOTSUP;
  if (!head || row_stride < H + 1) return OBJNERF_EINVAL;
  if (n == 0) return OBJNERF_OK;
  if (!out || (V > 0 && !rows) || (!index && n != V)) return OBJNERF_EINVAL;
  PartDev a{};
  a.V = V; a.n = n; a.C = C;
  a.src = rows; a.src_stride = row_stride;
  a.w = head; a.w_pitch = H + 1; a.bias = head + H; a.bias_stride = H + 1;
  a.index = index; a.out = out; a.out_stride = C;
  a.vec_src = al16(rows) && row_stride % 4 == 0;
  a.vec_w = 0;                                            // rows of [C][H + 1] are not 16-byte aligned
  a.vec_out = al16(out);
  return part_launch<true>(a, H, (hipStream_t)stream);
}

}  // extern "C"
