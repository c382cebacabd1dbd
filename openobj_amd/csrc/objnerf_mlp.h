// Shared by the hidden-32 units (fp32 / bf16 training, evaluation, rendering): the arena layout of one object's
// parameters and the block type of the register-resident MFMA chains.
//
// "D16 layout": a 32(feature) x 16(sample) fp32 block lives in one wave64 as 8 registers per lane:
// lane l = (c = l & 15 sample column, g = l >> 4), T32.t[tt][r] <-> feature 16*tt + 4*g + r.  A layer's
// output block is directly the B operand of the next layer's MFMAs (k-step (tt, r) consumes register
// (tt, r); the A operand supplies the weight column of the same feature), so activations never leave
// registers between layers, and a wave needs only 8 registers per activation -- two waves per SIMD fit.
#pragma once
#include "objnerf_device.h"

namespace obj32 {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int H = 32;
// arena offsets of the 19 tensors of one object (objnerf_param_layout order)
struct Layout {
  int in_w, in_b, m1_w, m1_b, cat_w, cat_b, m2_w, m2_b, a_w, a_b, cl_w, cl_b, oc_w, oc_b, fl_w, fl_b,
      of_w, of_b, pe_b, total;
};
__host__ __device__ inline Layout make_layout(int C) {
  Layout L;
  int o = 0;
  L.in_w = o; o += H * OBJ_E1;
  L.in_b = o; o += H;
  L.m1_w = o; o += H * H;
  L.m1_b = o; o += H;
  L.cat_w = o; o += H * (H + OBJ_E1);
  L.cat_b = o; o += H;
  L.m2_w = o; o += H * H;
  L.m2_b = o; o += H;
  L.a_w = o; o += H;
  L.a_b = o; o += 1;
  L.cl_w = o; o += H * (H + OBJ_E2);
  L.cl_b = o; o += H;
  L.oc_w = o; o += 3 * H;
  L.oc_b = o; o += 3;
  L.fl_w = o; o += H * (H + OBJ_E2);
  L.fl_b = o; o += H;
  L.of_w = o; o += C * H;
  L.of_b = o; o += C;
  L.pe_b = o; o += OBJ_NDIR * 3;
  L.total = o;
  return L;
}

struct T32 {
  f32x4 t[2];
};
__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

__device__ __forceinline__ T32 zero32() { return T32{{zero4(), zero4()}}; }
__device__ __forceinline__ T32 relu32(const T32& a) {
  T32 o;
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int r = 0; r < 4; ++r) o.t[tt][r] = fmaxf(a.t[tt][r], 0.0f);   // (no inline asm: MFMA->VALU hazards are the compiler's)
  return o;
}
__device__ __forceinline__ T32 relu_mask32(const T32& gr, const T32& act) {
  T32 o;
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int r = 0; r < 4; ++r) o.t[tt][r] = act.t[tt][r] > 0.0f ? gr.t[tt][r] : 0.0f;
  return o;
}

// v_mfma_f32_16x16x4_f32: exact fp32; C/D: col = lane & 15, row = 4 * (lane >> 4) + reg
#define OBJ_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// Forward activations of one 16-sample block.
struct Acts {
  T32 h1, h2, h3, h4, hc, hf;
};

__device__ __forceinline__ float xgroup_sum(float v) {   // sum over the 4 lane groups of a sample, on the VALU
  // v_permlane16_swap: odd 16-lane rows of the first operand <-> even rows of the second: with both = v the
  // two results are (r0,r0,r2,r2) and (r1,r1,r3,r3); v_permlane32_swap likewise for the 32-lane halves.
  const unsigned u = __float_as_uint(v);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const float s16 = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const unsigned u2 = __float_as_uint(s16);
  const auto b = __builtin_amdgcn_permlane32_swap(u2, u2, false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

}  // namespace obj32
