// Layer-wise training iteration for ANY hidden width (multiple of 32): the shared background network
// (hidden 128, train.py:447-463) and the hidden-256 stress configuration.  The hidden-32 object networks
// use the fused kernel in objnerf_train32.hip; wider networks do not fit one CU's LDS / registers, so this
// path materialises activations in the caller's workspace and runs the contraction as batched fp32 MFMA
// GEMMs (objnerf_gemm.hip), with the reference's op order:
//   embedding.py:46-55 -> model.py:61-103 -> loss.py:5-103 (objnerf_step_batch_loss) -> reverse.
#include <algorithm>
#include "objnerf_device.h"
#include "../../include/objnerf_hip.h"
#include "objnerf_generic.h"
#include "objnerf_gemm.h"
#include "objnerf_step_tail.h"
#include "objnerf_ray_loss.h"

namespace objgen {

// ------------------------------------------------------------------------------------------------
// Small-batch forward for hidden 128 (the background network at the reference's native batch, 1200 rays x 14
// samples): the layer-by-layer GEMMs above are then a chain of dependent ~15 us launches for ~1 us of MFMA work
// each.  Here ONE launch runs the whole network: a workgroup owns 16 RT samples (RT chosen so that the grid fills
// the chip once), keeps their activations in two LDS buffers and streams each layer's weight matrix from L2 into
// a third.  Every activation is also written to HBM, as the backward pass and the weight-gradient GEMMs read them.
// Same arithmetic as the GEMM path (fp32 MFMA, k ascending); the concatenated layers accumulate their two parts
// in one accumulator.  LDS rows have pitch 132 floats: conflict-free operand reads (bank = 4 m + k).
struct FwdSmall {
  long n; int feat;
  const float* params; long ps;
  const float* emb;                    // [K][n][OBJ_EMB]
  float *h1, *h2, *h3, *h4, *hc, *hf;  // [K][n][128]
  float *alpha, *color;                // [K][n], [K][n][3]
  int o_in_w, o_in_b, o_m1_w, o_m1_b, o_cat_w, o_cat_b, o_m2_w, o_m2_b, o_a_w, o_a_b, o_cl_w, o_cl_b, o_oc_w, o_oc_b,
      o_fl_w, o_fl_b;
};
constexpr int FS_H = 128, FS_P = 132;
template <int RT> constexpr size_t fs_lds_bytes() { return (size_t)(FS_H + 2 * 16 * RT) * FS_P * sizeof(float); }

// BF: OBJNERF_TRAIN_BF16 -- the same kernel with the contraction on v_mfma_f32_16x16x32_bf16: operands stay fp32 in
// LDS, a lane reads its 8 consecutive k of a 32-block (two ds_read_b128) and rounds them to bf16 on the fly; one MFMA
// replaces eight (the fp32 kernel spends ~60 % of its time in the MFMA loop).
__device__ __forceinline__ bf16x8 cvt_bf16x8(const f32x4& lo, const f32x4& hi) {
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) { o[e] = (__bf16)lo[e]; o[4 + e] = (__bf16)hi[e]; }
  return o;
}
template <int RT, bool BF>
__global__ __launch_bounds__(512) void mlp_fwd_small_kernel(const FwdSmall a) {
  constexpr int BM = 16 * RT, H = FS_H, PT = FS_P;
  extern __shared__ __attribute__((aligned(16))) float fs_lds[];
  float* Wb = fs_lds;                   // [128][132] current layer's weights, [out][in]
  float* Xa = Wb + H * PT;              // [BM][132]
  float* Xb = Xa + BM * PT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;     // 8 waves: wave w owns features 16 w .. 16 w + 15
  const int c = lane & 15, gg = lane >> 4;
  const long z = blockIdx.y, n = a.n;
  const long m0 = (long)blockIdx.x * BM;
  const float* P = a.params + z * a.ps;
  const float* emb = a.emb + z * n * OBJ_EMB;
  const int kk = tid & 127, rg = tid >> 7;          // staging: lanes along k (the contiguous source dimension)
  // The workgroup's slice of the embedding (x1 = columns [0, E1), x2 = [E1, E1 + E2)) is fetched ONCE into
  // registers at the start -- its HBM latency hides behind the first weight fetch -- and written to an LDS buffer
  // where a layer needs it (x1 twice): a global load at that point would sit exposed on the critical path.
  constexpr int ER = (BM + 3) / 4;
  float er1[ER], er2[ER];
#pragma unroll
  for (int i = 0; i < ER; ++i) {
    const int m = rg + 4 * i;
    const bool in = m < BM && m0 + m < n;
    er1[i] = (in && kk < OBJ_E1) ? emb[(m0 + m) * OBJ_EMB + kk] : 0.f;
    er2[i] = (in && kk < OBJ_E2) ? emb[(m0 + m) * OBJ_EMB + OBJ_E1 + kk] : 0.f;
  }
  auto put_emb = [&](float* X, const float (&er)[ER], const int KC) {      // zero-padded to a multiple of 16 (32) columns
    const int KC16 = BF ? ((KC + 31) & ~31) : ((KC + 15) & ~15);
    if (kk < KC16) {
#pragma unroll
      for (int i = 0; i < ER; ++i) {
        const int m = rg + 4 * i;
        if (m < BM) X[m * PT + kk] = er[i];
      }
    }
  };
  // The next layer's weights W[out][ld], columns [0, KC), are fetched into registers BEFORE the current layer's MFMA
  // loop and stored to Wb after it: their L2 latency hides behind the matrix work.
  float wr[32];
  auto fetch_w = [&](const float* W, const int ld, const int KC) {
#pragma unroll
    for (int i = 0; i < 32; ++i) wr[i] = kk < KC ? W[(rg + 4 * i) * ld + kk] : 0.f;
  };
  auto put_w = [&]() {
#pragma unroll
    for (int i = 0; i < 32; ++i) Wb[(rg + 4 * i) * PT + kk] = wr[i];
  };
  f32x4 acc[RT];
  auto zero = [&]() {
#pragma unroll
    for (int i = 0; i < RT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  };
  // acc += X[:, :KC] Wb^T for this wave's column tile, all RT row tiles (KC a multiple of 16).  The contraction index
  // is free to permute: MFMA step j of a 16-block takes k = 16 blk + 4 gg + j from lane group gg, so a lane fetches
  // four steps of an operand with ONE ds_read_b128 (conflict-free with the 132-float pitch); the next block's
  // operands are requested before the current block's 4 RT MFMAs are issued.
  auto mma = [&](const float* X, const int KC) {
    if (BF) {          // KC a multiple of 32 (the callers round up; the padding columns hold zeros on both sides)
      const float* bp = Wb + (16 * w + c) * PT + 8 * gg;
      const float* ap = X + c * PT + 8 * gg;
      for (int kb = 0; kb < KC; kb += 32) {
        const bf16x8 b = cvt_bf16x8(*reinterpret_cast<const f32x4*>(bp + kb), *reinterpret_cast<const f32x4*>(bp + kb + 4));
#pragma unroll
        for (int i = 0; i < RT; ++i) {
          const float* r = ap + 16 * i * PT + kb;
          const bf16x8 av = cvt_bf16x8(*reinterpret_cast<const f32x4*>(r), *reinterpret_cast<const f32x4*>(r + 4));
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b, acc[i], 0, 0, 0);
        }
      }
      return;
    }
    const float* bp = Wb + (16 * w + c) * PT + 4 * gg;
    const float* ap = X + c * PT + 4 * gg;
    f32x4 bc = *reinterpret_cast<const f32x4*>(bp), ac[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) ac[i] = *reinterpret_cast<const f32x4*>(ap + 16 * i * PT);
    for (int kb = 0; kb < KC; kb += 16) {
      f32x4 bn = bc, an[RT];
#pragma unroll
      for (int i = 0; i < RT; ++i) an[i] = ac[i];
      if (kb + 16 < KC) {
        bn = *reinterpret_cast<const f32x4*>(bp + kb + 16);
#pragma unroll
        for (int i = 0; i < RT; ++i) an[i] = *reinterpret_cast<const f32x4*>(ap + 16 * i * PT + kb + 16);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < RT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[i][j], bc[j], acc[i], 0, 0, 0);
      bc = bn;
#pragma unroll
      for (int i = 0; i < RT; ++i) ac[i] = an[i];
    }
  };
  // relu(acc + bias) -> LDS buffer (next layer's input) and the HBM activation
  auto store = [&](float* X, float* hbm, const float bv) {
    float* out = hbm + z * n * H;
    const int f = 16 * w + c;
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * i + 4 * gg + r;
        const float v = fmaxf(acc[i][r] + bv, 0.f);
        X[m * PT + f] = v;
        if (m0 + m < n) out[(m0 + m) * H + f] = v;
      }
  };
  constexpr int E1P = BF ? ((OBJ_E1 + 31) & ~31) : ((OBJ_E1 + 15) & ~15), E2P = BF ? ((OBJ_E2 + 31) & ~31) : ((OBJ_E2 + 15) & ~15);
  // biases and head weights of this lane, fetched before anything waits on them
  const int fb = 16 * w + c;
  const float b_in = P[a.o_in_b + fb], b_m1 = P[a.o_m1_b + fb], b_cat = P[a.o_cat_b + fb], b_m2 = P[a.o_m2_b + fb];
  const float b_cl = P[a.o_cl_b + fb], b_fl = a.feat ? P[a.o_fl_b + fb] : 0.f;
  const float wa0 = P[a.o_a_w + lane], wa1 = P[a.o_a_w + lane + 64];
  const float w00 = P[a.o_oc_w + lane], w01 = P[a.o_oc_w + lane + 64];
  const float w10 = P[a.o_oc_w + H + lane], w11 = P[a.o_oc_w + H + lane + 64];
  const float w20 = P[a.o_oc_w + 2 * H + lane], w21 = P[a.o_oc_w + 2 * H + lane + 64];
  const float ba = P[a.o_a_b], bc0 = P[a.o_oc_b], bc1 = P[a.o_oc_b + 1], bc2 = P[a.o_oc_b + 2];
  // ---- h1 = relu(x1 W_in^T + b)                                  (model.py:63-66)
  fetch_w(P + a.o_in_w, OBJ_E1, OBJ_E1);
  put_emb(Xa, er1, OBJ_E1);
  put_w();
  __syncthreads();
  fetch_w(P + a.o_m1_w, H, H);
  zero();
  mma(Xa, E1P);
  __syncthreads();
  store(Xb, a.h1, b_in);
  put_w();
  __syncthreads();
  // ---- h2
  fetch_w(P + a.o_cat_w, H + OBJ_E1, H);
  zero();
  mma(Xb, H);
  __syncthreads();
  store(Xa, a.h2, b_m1);
  put_w();
  put_emb(Xb, er1, OBJ_E1);
  __syncthreads();
  // ---- h3 = relu([h2 | x1] W_cat^T + b)
  fetch_w(P + a.o_cat_w + H, H + OBJ_E1, OBJ_E1);
  zero();
  mma(Xa, H);
  __syncthreads();
  put_w();
  __syncthreads();
  fetch_w(P + a.o_m2_w, H, H);
  mma(Xb, E1P);
  __syncthreads();
  store(Xa, a.h3, b_cat);
  put_w();
  __syncthreads();
  // ---- h4
  fetch_w(P + a.o_cl_w, H + OBJ_E2, H);
  zero();
  mma(Xa, H);
  __syncthreads();
  store(Xb, a.h4, b_m2);
  put_w();
  put_emb(Xa, er2, OBJ_E2);
  __syncthreads();
  // ---- hc = relu([h4 | x2] W_cl^T + b)
  fetch_w(P + a.o_cl_w + H, H + OBJ_E2, OBJ_E2);
  zero();
  mma(Xb, H);
  __syncthreads();
  put_w();
  __syncthreads();
  if (a.feat) fetch_w(P + a.o_fl_w, H + OBJ_E2, H);
  mma(Xa, E2P);
  __syncthreads();
  // hc goes to a THIRD place: Wb is free until the next put_w and Xa (x2) is needed again by the feature layer
  float* Xc = Wb;
  store(Xc, a.hc, b_cl);
  __syncthreads();
  // ---- heads: alpha = 10 (h4 . wa + ba), colour = sigmoid(hc Woc^T + boc)      (model.py:81-96); a wave per row
  {
    for (int m = w; m < BM; m += 8) {
      const float x0 = Xb[m * PT + lane], x1 = Xb[m * PT + lane + 64];
      const float y0 = Xc[m * PT + lane], y1 = Xc[m * PT + lane + 64];
      const float sa = wave_sum64(fmaf(wa1, x1, wa0 * x0));
      const float s0 = wave_sum64(fmaf(w01, y1, w00 * y0));
      const float s1 = wave_sum64(fmaf(w11, y1, w10 * y0));
      const float s2 = wave_sum64(fmaf(w21, y1, w20 * y0));
      if (lane == 0 && m0 + m < n) {
        const long i = z * n + m0 + m;
        a.alpha[i] = (sa + ba) * 10.0f;
        a.color[i * 3] = sigmoid_acc(s0 + bc0);
        a.color[i * 3 + 1] = sigmoid_acc(s1 + bc1);
        a.color[i * 3 + 2] = sigmoid_acc(s2 + bc2);
      }
    }
  }
  if (!a.feat) return;
  // ---- hf = relu([h4 | x2] W_fl^T + b)     (feature layer, same inputs as the colour layer: Xb = h4, Xa = x2)
  __syncthreads();
  put_w();
  __syncthreads();
  fetch_w(P + a.o_fl_w + H, H + OBJ_E2, OBJ_E2);
  zero();
  mma(Xb, H);
  __syncthreads();
  put_w();
  __syncthreads();
  mma(Xa, E2P);
  float* out = a.hf + z * n * H;
  {
    const int f = 16 * w + c;
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * i + 4 * gg + r;
        if (m0 + m < n) out[(m0 + m) * H + f] = fmaxf(acc[i][r] + b_fl, 0.f);
      }
  }
}

// ------------------------------------------------------------------------------------------------
// The matching backward (input-gradient chain) in one launch: d_hc (+ d_hf) -> d_h4 -> d_h3 -> d_h2 -> d_h1 and the
// embedding gradient, every d_h also written to HBM for the weight-gradient GEMMs.  d_in = d_out W is the same MFMA
// loop with the weight rows read as they lie in memory: Wb[k = out][n = in], pitch 130 (bank = 2 k + n).
struct BwdSmall {
  long n; int feat;
  const float* params; long ps;
  const float *h1, *h2, *h3, *h4;      // relu masks
  const float *d_hc, *d_hf;            // [K][n][128] (d_hf: feature layer, or NULL)
  float *d_h4, *d_h3, *d_h2, *d_h1;    // d_h4 arrives holding the alpha head's contribution (heads_bwd_kernel)
  float* d_emb;                        // [K][n][OBJ_EMB]
  int o_in_w, o_m1_w, o_cat_w, o_m2_w, o_cl_w, o_fl_w;
};
constexpr int BS_PW = 130;
template <int RT> constexpr size_t bs_lds_bytes() { return (size_t)(FS_H * BS_PW + 2 * 16 * RT * FS_P) * sizeof(float); }

template <int RT, bool BF>
__global__ __launch_bounds__(512) void mlp_bwd_small_kernel(const BwdSmall a) {
  constexpr int BM = 16 * RT, H = FS_H, PT = FS_P, PW = BS_PW;
  extern __shared__ __attribute__((aligned(16))) float fs_lds[];
  float* Wb = fs_lds;                   // [k = out][n = in], pitch 130
  float* Da = Wb + H * PW;              // [BM][132]
  float* Db = Da + BM * PT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;     // wave w owns input features 16 w .. 16 w + 15
  const int c = lane & 15, gg = lane >> 4;
  const long z = blockIdx.y, n = a.n;
  const long m0 = (long)blockIdx.x * BM;
  const float* P = a.params + z * a.ps;
  const int kk = tid & 127, rg = tid >> 7;
  auto load_d = [&](float* X, const float* src) {     // rows [m0, m0 + BM) of a [n][128] tensor
    const float* sp = src + z * n * H;
#pragma unroll
    for (int i = 0; i < (BM + 3) / 4; ++i) {
      const int m = rg + 4 * i;
      if (m < BM) X[m * PT + kk] = (m0 + m < n) ? sp[(m0 + m) * H + kk] : 0.f;
    }
  };
  // W[out][ld], columns [col0, col0 + NC): row `out` -> Wb[out][0 .. NC) (zero up to 128), fetched ahead into registers
  float wr[32];
  auto fetch_w = [&](const float* W, const int ld, const int NC) {
#pragma unroll
    for (int i = 0; i < 32; ++i) wr[i] = kk < NC ? W[(rg + 4 * i) * ld + kk] : 0.f;
  };
  // bf16 mode: the weight rows go to LDS ROUNDED, [k = out][n = in] with a 288-byte pitch (72 dwords = 8 mod 64: the
  // eight rows a transposing read's half-wave touches sit on disjoint bank octets)
  constexpr int PW16 = 288;
  auto put_w = [&]() {
    if (BF) {
      __bf16* W16 = reinterpret_cast<__bf16*>(Wb);
#pragma unroll
      for (int i = 0; i < 32; ++i) W16[(rg + 4 * i) * (PW16 / 2) + kk] = (__bf16)wr[i];
      return;
    }
#pragma unroll
    for (int i = 0; i < 32; ++i) Wb[(rg + 4 * i) * PW + kk] = wr[i];
  };
  f32x4 acc[RT], accE[RT];
  auto zero = [&](f32x4 (&v)[RT]) {
#pragma unroll
    for (int i = 0; i < RT; ++i) v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  };
  // v += D (all 128 output-feature columns) x Wb -> this wave's 16 input features.  Same k permutation as the
  // forward kernel (step j of a 16-block takes k = 16 blk + 4 gg + j): D rows by ds_read_b128, the four weight rows
  // by ds_read_b32 (bank = 8 gg + 2 j + n: two lanes per bank, the minimum for 64 lanes).
  auto mma = [&](const float* D, f32x4 (&v)[RT]) {
    if (BF) {
      // bf16 MFMA: the lane's 8 k-slots of a 32-block are output features 4 gg .. 4 gg + 3 and 16 + 4 gg .. + 3.  The
      // weight operand -- 8 k of ONE input column -- comes out of the row-major bf16 image by two transposing reads
      // (lane 4 q + p of a 16-lane group supplies row q, 8-byte chunk p); it used to be eight ds_read_b32 of fp32 rows
      // and four conversions per MFMA.
      const char* bp = reinterpret_cast<const char*>(Wb) + (4 * gg + (c >> 2)) * PW16 + 32 * w + 8 * (c & 3);
      const float* ap = D + c * PT + 4 * gg;
#pragma unroll
      for (int kb = 0; kb < H; kb += 32) {
        const uint2 b0 = lds_tr16(bp + kb * PW16), b1 = lds_tr16(bp + (kb + 16) * PW16);
        const bf16x8 b = __builtin_bit_cast(bf16x8, uint4{b0.x, b0.y, b1.x, b1.y});
#pragma unroll
        for (int i = 0; i < RT; ++i) {
          const float* r = ap + 16 * i * PT + kb;
          const bf16x8 av = cvt_bf16x8(*reinterpret_cast<const f32x4*>(r), *reinterpret_cast<const f32x4*>(r + 16));
          v[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b, v[i], 0, 0, 0);
        }
      }
      return;
    }
    const float* bp = Wb + 4 * gg * PW + 16 * w + c;
    const float* ap = D + c * PT + 4 * gg;
    f32x4 bc, ac[RT];
#pragma unroll
    for (int j = 0; j < 4; ++j) bc[j] = bp[j * PW];
#pragma unroll
    for (int i = 0; i < RT; ++i) ac[i] = *reinterpret_cast<const f32x4*>(ap + 16 * i * PT);
    for (int kb = 0; kb < H; kb += 16) {
      f32x4 bn = bc, an[RT];
#pragma unroll
      for (int i = 0; i < RT; ++i) an[i] = ac[i];
      if (kb + 16 < H) {
#pragma unroll
        for (int j = 0; j < 4; ++j) bn[j] = bp[(kb + 16 + j) * PW];
#pragma unroll
        for (int i = 0; i < RT; ++i) an[i] = *reinterpret_cast<const f32x4*>(ap + 16 * i * PT + kb + 16);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < RT; ++i) v[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[i][j], bc[j], v[i], 0, 0, 0);
      bc = bn;
#pragma unroll
      for (int i = 0; i < RT; ++i) ac[i] = an[i];
    }
  };
  // masked d_h: (acc [+ prior]) where act > 0 -> LDS (next layer's operand) and HBM
  float mk[RT][4];
  auto fetch_mask = [&](const float* act) {
    const float* hp = act + z * n * H;
    const int f = 16 * w + c;
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * i + 4 * gg + r;
        mk[i][r] = (m0 + m < n) ? hp[(m0 + m) * H + f] : 0.f;
      }
  };
  float pr[RT][4];                         // d_h4 arrives holding the alpha head's part: fetched with the mask
  auto fetch_prior = [&](const float* src) {
    const float* sp = src + z * n * H;
    const int f = 16 * w + c;
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * i + 4 * gg + r;
        pr[i][r] = (m0 + m < n) ? sp[(m0 + m) * H + f] : 0.f;
      }
  };
  auto store_dh = [&](float* X, float* hbm, const bool add_prior) {
    float* out = hbm + z * n * H;
    const int f = 16 * w + c;
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * i + 4 * gg + r;
        const bool in = m0 + m < n;
        float v = acc[i][r];
        if (add_prior) v += pr[i][r];
        v = mk[i][r] > 0.f ? v : 0.f;
        X[m * PT + f] = v;
        if (in) out[(m0 + m) * H + f] = v;
      }
  };
  auto store_emb = [&](const int col0, const int NC) {     // accE -> d_emb[:, col0 + f], f < NC
    float* out = a.d_emb + z * n * OBJ_EMB;
    const int f = 16 * w + c;
    if (f < NC) {
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = 16 * i + 4 * gg + r;
          if (m0 + m < n) out[(m0 + m) * OBJ_EMB + col0 + f] = accE[i][r];
        }
    }
  };
  const bool e1_wave = 16 * w < OBJ_E1, e2_wave = 16 * w < OBJ_E2;      // waves that own embedding columns
  zero(acc);
  zero(accE);
  if (a.feat) {
    // ---- feature layer: d_h4 += d_hf W_fl[:, :H], d_x2 = d_hf W_fl[:, H:]
    fetch_w(P + a.o_fl_w, H + OBJ_E2, H);
    load_d(Da, a.d_hf);
    put_w();
    __syncthreads();
    fetch_w(P + a.o_fl_w + H, H + OBJ_E2, OBJ_E2);
    mma(Da, acc);
    __syncthreads();
    put_w();
    __syncthreads();
    if (e2_wave) mma(Da, accE);
    __syncthreads();
  }
  // ---- colour layer: d_h4 = relu'(h4) (alpha-head part + [d_hf W_fl1] + d_hc W_cl[:, :H]), d_x2 (+)= d_hc W_cl[:, H:]
  fetch_w(P + a.o_cl_w, H + OBJ_E2, H);
  load_d(Da, a.d_hc);
  put_w();
  __syncthreads();
  fetch_w(P + a.o_cl_w + H, H + OBJ_E2, OBJ_E2);
  fetch_mask(a.h4);
  fetch_prior(a.d_h4);
  mma(Da, acc);
  __syncthreads();
  store_dh(Db, a.d_h4, true);                    // Db = d_h4
  put_w();
  __syncthreads();
  fetch_w(P + a.o_m2_w, H, H);
  if (e2_wave) mma(Da, accE);
  store_emb(OBJ_E1, OBJ_E2);
  __syncthreads();
  // ---- mid2: d_h3 = relu'(h3) (d_h4 W_m2)
  put_w();
  __syncthreads();
  fetch_w(P + a.o_cat_w, H + OBJ_E1, H);
  fetch_mask(a.h3);
  zero(acc);
  mma(Db, acc);
  __syncthreads();
  store_dh(Da, a.d_h3, false);                   // Da = d_h3
  put_w();
  __syncthreads();
  // ---- cat layer: d_h2 = relu'(h2) (d_h3 W_cat[:, :H]), d_x1 = d_h3 W_cat[:, H:]
  fetch_w(P + a.o_cat_w + H, H + OBJ_E1, OBJ_E1);
  fetch_mask(a.h2);
  zero(acc);
  mma(Da, acc);
  __syncthreads();
  store_dh(Db, a.d_h2, false);                   // Db = d_h2
  put_w();
  __syncthreads();
  fetch_w(P + a.o_m1_w, H, H);
  zero(accE);
  if (e1_wave) mma(Da, accE);
  __syncthreads();
  // ---- mid1: d_h1 = relu'(h1) (d_h2 W_m1)
  put_w();
  __syncthreads();
  fetch_w(P + a.o_in_w, OBJ_E1, OBJ_E1);
  fetch_mask(a.h1);
  zero(acc);
  mma(Db, acc);
  __syncthreads();
  store_dh(Da, a.d_h1, false);                   // Da = d_h1
  put_w();
  __syncthreads();
  // ---- in layer: d_x1 += d_h1 W_in
  if (e1_wave) mma(Da, accE);
  store_emb(0, OBJ_E1);
}

template <int RT>
static void launch_small(hipStream_t st, const BwdSmall& f, int K, bool bf) {
  objnerf_once_per_device([] {
    (void)hipFuncSetAttribute((const void*)mlp_bwd_small_kernel<RT, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)bs_lds_bytes<RT>());
    (void)hipFuncSetAttribute((const void*)mlp_bwd_small_kernel<RT, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)bs_lds_bytes<RT>());
  });
  dim3 grid((unsigned)((f.n + 16 * RT - 1) / (16 * RT)), (unsigned)K);
  if (bf) hipLaunchKernelGGL((mlp_bwd_small_kernel<RT, true>), grid, dim3(512), bs_lds_bytes<RT>(), st, f);
  else hipLaunchKernelGGL((mlp_bwd_small_kernel<RT, false>), grid, dim3(512), bs_lds_bytes<RT>(), st, f);
}

template <int RT>
static void launch_small(hipStream_t st, const FwdSmall& f, int K, bool bf) {
  objnerf_once_per_device([] {
    (void)hipFuncSetAttribute((const void*)mlp_fwd_small_kernel<RT, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)fs_lds_bytes<RT>());
    (void)hipFuncSetAttribute((const void*)mlp_fwd_small_kernel<RT, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)fs_lds_bytes<RT>());
  });
  dim3 grid((unsigned)((f.n + 16 * RT - 1) / (16 * RT)), (unsigned)K);
  if (bf) hipLaunchKernelGGL((mlp_fwd_small_kernel<RT, true>), grid, dim3(512), fs_lds_bytes<RT>(), st, f);
  else hipLaunchKernelGGL((mlp_fwd_small_kernel<RT, false>), grid, dim3(512), fs_lds_bytes<RT>(), st, f);
}
// (RT as a run-time value: small_batch_rt)
template <class Args>
static void launch_small_rt(hipStream_t st, const Args& f, int K, bool bf, int rt) {
  switch (rt) {
    case 1: launch_small<1>(st, f, K, bf); break;
    case 2: launch_small<2>(st, f, K, bf); break;
    case 3: launch_small<3>(st, f, K, bf); break;
    case 4: launch_small<4>(st, f, K, bf); break;
    default: launch_small<5>(st, f, K, bf); break;
  }
}

#include "objnerf_small_body.h"

// row tiles per workgroup: the smallest RT for which K * ceil(n / (16 RT)) workgroups fit the chip in one round;
// 0 = not a small batch
static int small_batch_rt(int operands, int H, long n, int K) {
  if (H != FS_H) return 0;
  for (int rt = 1; rt <= 5; ++rt)
    if ((long)K * ((n + 16 * rt - 1) / (16 * rt)) <= 256) return rt;
  // up to four rounds of 80-sample workgroups the one-launch kernels still win (76 800 samples: 1.02 vs 1.07 ms per
  // step, 38 400: 0.53 vs 0.65); beyond that the GEMM path runs near the MFMA peak
  // (fp32 and bf16 modes: the one-launch kernels exist for both; fp16 keeps the GEMM path from two rounds on)
#ifdef OBJ_NO_SMALL_BF16        // diagnostic: the bf16 mode on the GEMM path from two rounds on (tools/bg_ab.py)
  if (operands == 0 && (long)K * ((n + 79) / 80) <= 1024) return 5;
#else
  if (operands != 2 && (long)K * ((n + 79) / 80) <= 1024) return 5;
#endif
  return 0;
}

// Activation loads of the kernels around the GEMMs: act = 0 fp32 storage, 1 bf16, 2 fp16 (the 16-bit modes keep
// h1 .. hc in the operand type at hidden 256: half the traffic of the HBM-bound layer GEMMs).
__device__ __forceinline__ float act_ld(const float* p, long i, int act) {
  if (act == 0) return p[i];
  if (act == 1) return (float)reinterpret_cast<const __bf16*>(p)[i];
  return (float)reinterpret_cast<const _Float16*>(p)[i];
}
__device__ __forceinline__ float4 act_ld4(const float* p, long i, int act) {       // i % 4 == 0
  if (act == 0) return *reinterpret_cast<const float4*>(p + i);
  const uint2 r = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(p) + i);
  if (act == 1)
    return make_float4(__builtin_bit_cast(float, r.x << 16), __builtin_bit_cast(float, r.x & 0xffff0000u),
                       __builtin_bit_cast(float, r.y << 16), __builtin_bit_cast(float, r.y & 0xffff0000u));
  typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
  const h4_t h = __builtin_bit_cast(h4_t, r);
  return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
}

__device__ __forceinline__ void act_st4(float* p, long i, float4 v, int act, float scale) {     // i % 4 == 0
  if (act == 0) { *reinterpret_cast<float4*>(p + i) = v; return; }
  uint2 r;
  if (act == 1) {
    typedef __bf16 b4_t __attribute__((ext_vector_type(4)));
    const b4_t b = {(__bf16)(v.x * scale), (__bf16)(v.y * scale), (__bf16)(v.z * scale), (__bf16)(v.w * scale)};
    r = __builtin_bit_cast(uint2, b);
  } else {
    typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
    const h4_t h = {Op16<_Float16>::cvt(v.x * scale), Op16<_Float16>::cvt(v.y * scale), Op16<_Float16>::cvt(v.z * scale),
                    Op16<_Float16>::cvt(v.w * scale)};
    r = __builtin_bit_cast(uint2, h);
  }
  *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p) + i) = r;
}

// heads forward: alpha = 10 (h4 . wa + ba), color = sigmoid(hc Woc^T + boc)        (model.py:81-96)
// 16 lanes per sample row (float4 each, coalesced), the four dot products meet by DPP row sums.
__global__ __launch_bounds__(256) void heads_fwd_kernel(int Hh, long n, const float* h4, const float* hc,
                                                        const float* params, long p_stride, int off_wa, int off_ba,
                                                        int off_woc, int off_boc, float* alpha, float* color, int act) {
  extern __shared__ float sw[];            // wa | woc[3]  (4 Hh floats)
  const long z = blockIdx.y;
  const float* P = params + z * p_stride;
  for (int i = threadIdx.x; i < Hh; i += 256) sw[i] = P[off_wa + i];
  for (int i = threadIdx.x; i < 3 * Hh; i += 256) sw[Hh + i] = P[off_woc + i];
  __syncthreads();
  const int l16 = threadIdx.x & 15;
  const long i = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  float sa = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
  if (i < n) {
    const long ro = (z * n + i) * Hh;
    for (int h = 4 * l16; h < Hh; h += 64) {
      const float4 av = act_ld4(h4, ro + h, act);
      const float4 cv = act_ld4(hc, ro + h, act);
      const float* w0 = sw + h;
      sa = fmaf(w0[3], av.w, fmaf(w0[2], av.z, fmaf(w0[1], av.y, fmaf(w0[0], av.x, sa))));
      s0 = fmaf(w0[Hh + 3], cv.w, fmaf(w0[Hh + 2], cv.z, fmaf(w0[Hh + 1], cv.y, fmaf(w0[Hh], cv.x, s0))));
      s1 = fmaf(w0[2 * Hh + 3], cv.w, fmaf(w0[2 * Hh + 2], cv.z, fmaf(w0[2 * Hh + 1], cv.y, fmaf(w0[2 * Hh], cv.x, s1))));
      s2 = fmaf(w0[3 * Hh + 3], cv.w, fmaf(w0[3 * Hh + 2], cv.z, fmaf(w0[3 * Hh + 1], cv.y, fmaf(w0[3 * Hh], cv.x, s2))));
    }
  }
  sa = dpp_rowsum16(sa); s0 = dpp_rowsum16(s0); s1 = dpp_rowsum16(s1); s2 = dpp_rowsum16(s2);
  if (i < n && l16 == 0) {
    alpha[z * n + i] = (sa + P[off_ba]) * 10.0f;
    color[(z * n + i) * 3] = sigmoid_acc(s0 + P[off_boc]);
    color[(z * n + i) * 3 + 1] = sigmoid_acc(s1 + P[off_boc + 1]);
    color[(z * n + i) * 3 + 2] = sigmoid_acc(s2 + P[off_boc + 2]);
  }
}

// heads backward: dhead[n][4] = (10 d_alpha, d_color * color (1 - color)); d_hc = relu'(hc) Woc^T d_craw;
// d_h4 = wa * d_araw  (the colour-layer contribution is accumulated by a GEMM afterwards; d_h4 == NULL: that GEMM adds
// this rank-1 term itself -- bias = wa, per-row factor = dhead[:, 0] -- and the 2 x n x H round trip is saved)
__global__ __launch_bounds__(256) void heads_bwd_kernel(int Hh, long n, const float* hc, const float* color,
                                                        const float* d_alpha, const float* d_color, const float* params,
                                                        long p_stride, int off_wa, int off_woc, float* dhead, float* d_hc,
                                                        float* d_h4, int act, float gscale) {
  extern __shared__ float sw[];            // wa | woc[3]
  const long z = blockIdx.y;
  const float* P = params + z * p_stride;
  for (int i = threadIdx.x; i < Hh; i += 256) sw[i] = P[off_wa + i];
  for (int i = threadIdx.x; i < 3 * Hh; i += 256) sw[Hh + i] = P[off_woc + i];
  __syncthreads();
  const int l16 = threadIdx.x & 15;
  const long i = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (i >= n) return;
  const long o = z * n + i;
  const float da = 10.0f * d_alpha[o];
  float dc[3];
  for (int x = 0; x < 3; ++x) {
    const float cv = color[o * 3 + x];
    dc[x] = d_color[o * 3 + x] * cv * (1.0f - cv);
  }
  if (l16 == 0) *reinterpret_cast<float4*>(dhead + o * 4) = make_float4(da, dc[0], dc[1], dc[2]);
  for (int h = 4 * l16; h < Hh; h += 64) {
    const float4 hv = act_ld4(hc, o * Hh + h, act);
    const float* w0 = sw + h;
    float4 v, u;
    v.x = fmaf(w0[3 * Hh], dc[2], fmaf(w0[2 * Hh], dc[1], w0[Hh] * dc[0]));
    v.y = fmaf(w0[3 * Hh + 1], dc[2], fmaf(w0[2 * Hh + 1], dc[1], w0[Hh + 1] * dc[0]));
    v.z = fmaf(w0[3 * Hh + 2], dc[2], fmaf(w0[2 * Hh + 2], dc[1], w0[Hh + 2] * dc[0]));
    v.w = fmaf(w0[3 * Hh + 3], dc[2], fmaf(w0[2 * Hh + 3], dc[1], w0[Hh + 3] * dc[0]));
    v.x = hv.x > 0.f ? v.x : 0.f; v.y = hv.y > 0.f ? v.y : 0.f; v.z = hv.z > 0.f ? v.z : 0.f; v.w = hv.w > 0.f ? v.w : 0.f;
    u.x = w0[0] * da; u.y = w0[1] * da; u.z = w0[2] * da; u.w = w0[3] * da;
    // (act != 0: the gradient buffers are 16-bit too, stored as the next GEMM's operand -- scaled by gscale)
    act_st4(d_hc, o * Hh + h, v, act, gscale);
    if (d_h4) act_st4(d_h4, o * Hh + h, u, act, gscale);
  }
}

// Head weight gradients: d wa[f] = sum_i dhead[i][0] h4[i][f], d Woc[x][f] = sum_i dhead[i][1+x] hc[i][f], biases =
// column sums of dhead.  A 4 x H output: a GEMM tile would be 94 % padding, so this is a plain reduction over the
// samples (reads h4 and hc once, coalesced along f); one atomic per block and entry into the pre-zeroed gradient.
__global__ __launch_bounds__(256) void head_wgrad_kernel(int Hh, long n, const float* dhead, const float* h4, const float* hc,
                                                         float* grads, long p_stride, int off_wa, int off_ba, int off_woc,
                                                         int off_boc, float* partA, float* partW, float* rsA, float* rsW,
                                                         int act) {
  __shared__ float red[4][256];
  const long z = blockIdx.y;
  const int rows = 256 / Hh > 0 ? 256 / Hh : 1;            // sample rows per pass (H <= 256)
  const int f = threadIdx.x % Hh, row = threadIdx.x / Hh;
  const bool live = row < rows;
  const long per = (n + gridDim.x - 1) / gridDim.x;
  const long i0 = (long)blockIdx.x * per, i1 = i0 + per < n ? i0 + per : n;
  float a = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
  if (live)
    for (long i = i0 + row; i < i1; i += rows) {
      const long o = z * n + i;
      const float4 d = *reinterpret_cast<const float4*>(dhead + o * 4);
      const float hv = act_ld(h4, o * Hh + f, act), cv = act_ld(hc, o * Hh + f, act);
      a = fmaf(d.x, hv, a); c0 = fmaf(d.y, cv, c0); c1 = fmaf(d.z, cv, c1); c2 = fmaf(d.w, cv, c2);
    }
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = c0; red[2][threadIdx.x] = c1; red[3][threadIdx.x] = c2;
  __syncthreads();
  float* G = grads + z * p_stride;
  const long zb = z * gridDim.x + blockIdx.x;       // partial slot (reduce_parts_kernel layout: [z][slice][M][N])
  if (row == 0) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < rows; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) s[q] += red[q][r * Hh + f];
    if (partA) {
      partA[zb * Hh + f] = s[0];
#pragma unroll
      for (int x = 0; x < 3; ++x) partW[(zb * 3 + x) * Hh + f] = s[1 + x];
    } else {
      atomicAdd(G + off_wa + f, s[0]);
#pragma unroll
      for (int x = 0; x < 3; ++x) atomicAdd(G + off_woc + x * Hh + f, s[1 + x]);
    }
  }
  // biases: lanes 0..3 of the last wave sum their dhead column over the block's samples
  if (threadIdx.x >= 192) {
    const int lane = threadIdx.x - 192, q = lane & 3;
    float b = 0.f;
    for (long i = i0 + (lane >> 2); i < i1; i += 16) b += dhead[(z * n + i) * 4 + q];
    b += __shfl_xor(b, 4); b += __shfl_xor(b, 8); b += __shfl_xor(b, 16); b += __shfl_xor(b, 32);
    if (lane < 4) {
      if (partA) { if (q == 0) rsA[zb] = b; else rsW[zb * 3 + q - 1] = b; }
      else atomicAdd(G + (q == 0 ? off_ba : off_boc + q - 1), b);
    }
  }
}

__global__ void relu_mask_kernel(long n, float* d, const float* act) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = act[i] > 0.f ? d[i] : 0.f;
}

// PE backward: d B[j][x] = sum_n t[n][x] sum_f d_emb[n][3 + 21 f + j] cos(arg) pi 2^f     (embedding.py:48-52)
// lane = (sample slot 0..2, direction j): 63 lanes per wave, the six d_emb reads of a lane group are contiguous
// over j; three accumulators per thread, LDS reduction per block, one atomic per block and entry.
__global__ __launch_bounds__(256) void pe_bwd_kernel(long n, const float* params, long p_stride, int off_B,
                                                     const float* scale, const float* pts, const float* d_emb,
                                                     float* dB /* [K][63], pre-zeroed */,
                                                     float* part /* NULL or [K][gridDim.x][63] block partials */) {
  __shared__ float red[4][63][3];
  const long z = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = lane % OBJ_NDIR, s3 = lane / OBJ_NDIR;      // lane 63: s3 == 3 -> idle
  const float* B = params + z * p_stride + off_B;
  const float b0 = B[3 * j], b1 = B[3 * j + 1], b2 = B[3 * j + 2];
  const float sc = scale[z];
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  const long stride = (long)gridDim.x * 12;
  for (long i = ((long)blockIdx.x * 4 + wv) * 3 + s3; i < n && s3 < 3; i += stride) {
    const float* p = pts + (z * n + i) * 3;
    const float t0 = p[0] / sc, t1 = p[1] / sc, t2 = p[2] / sc;
    const float* de = d_emb + (z * n + i) * OBJ_EMB + 3 + j;
    const float pj = fmaf(t2, b2, fmaf(t1, b1, t0 * b0));
    float dp = 0.f;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
      const float sf = (float)(1 << f);
      float sv, cv;
      sincos_acc((pj * sf) * OBJ_PI_F, sv, cv);
      dp += de[f * OBJ_NDIR] * ((cv * OBJ_PI_F) * sf);
    }
    a0 = fmaf(dp, t0, a0);
    a1 = fmaf(dp, t1, a1);
    a2 = fmaf(dp, t2, a2);
  }
  if (lane < 63) { red[wv][lane][0] = a0; red[wv][lane][1] = a1; red[wv][lane][2] = a2; }
  __syncthreads();
  if (threadIdx.x < 63) {
    const int jj = threadIdx.x / 3, x = threadIdx.x % 3;
    float v = 0.f;
    for (int ww = 0; ww < 4; ++ww)
      for (int ss = 0; ss < 3; ++ss) v += red[ww][ss * OBJ_NDIR + jj][x];
    if (part) part[(z * gridDim.x + blockIdx.x) * 63 + threadIdx.x] = v;
    else atomicAdd(&dB[z * 63 + threadIdx.x], v);
  }
}

__global__ void copy_cols_kernel(long rows, int cols, const float* src, long lds_, float* dst, long ldd) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows * cols) dst[(i / cols) * ldd + (i % cols)] = src[(i / cols) * lds_ + (i % cols)];
}


// ------------------------------------------------------------------------------------------------
// Feature-distillation branch with the 512-d head hoisted past the compositing, any hidden width Hh
// (the hidden-32 fused kernel has its own copies in objnerf_train.hip).
__global__ __launch_bounds__(256) void featg_rowstats_kernel(const float* params, long p_stride, int off_b, int C, int R,
                                                             int rin_ld, const float* gt_feat, float* rayin) {
  const int k = blockIdx.y;
  const int l16 = threadIdx.x & 15;
  const long r = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  featg_ray_stats(params + (long)k * p_stride + off_b, C, R, gt_feat, rayin, rin_ld, k, r, l16);
}
// [wb | bb] appended to the Gram matrix: gram[k][Hh * Hh + h], [Hh * Hh + Hh]
__global__ __launch_bounds__(64) void featg_wb_kernel(const float* params, long p_stride, int off_w, int off_b, int C,
                                                      int Hh, float* gram, long gstride) {
  const int k = blockIdx.y, h = blockIdx.x;
  const float* W = params + (long)k * p_stride + off_w;
  const float* B = params + (long)k * p_stride + off_b;
  const float acc = featg_wb_entry(W, B, C, Hh, h, threadIdx.x);
  if (threadIdx.x == 0) gram[(long)k * gstride + (long)Hh * Hh + h] = acc;
}
// X1 = [a fh | a O], X2 = [c fh | c O] from rayfeat rows (fh[Hh], O, a, c)
__global__ void featg_scale_kernel(long n, int Hh, const float* rayfeat, float* X1, float* X2) {
  const int XC = Hh + 1;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * XC) return;
  const long r = i / XC;
  const int j = (int)(i - r * XC);
  const float* rf = rayfeat + r * (Hh + 3);
  const float v = rf[j];
  X1[i] = rf[Hh + 1] * v;
  X2[i] = rf[Hh + 2] * v;
}
// Entry (c, hh) of the head's gradient from row c of W_of, b_c = b_of[c], the rays' moments M [XC][XC] and t = T[c][hh]:
// d W_of[c][h] = T[c][h] + sum_j W_of[c][j] M[j][h] + b_of[c] M[Hh][h];  d b_of[c] (hh == Hh) = T[c][Hh] + W_of[c] . M[Hh][:] + b_of[c] M[Hh][Hh]
__device__ __forceinline__ float featg_head_grad(const float* W, const float bc, const float* M, float v, const int hh,
                                                 const int Hh, const int XC) {
  // four partial sums: the loads of four steps are in flight together (Hh is a multiple of 32)
  float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
  if (hh < Hh) {
    for (int j = 0; j < Hh; j += 4) {
      v0 = fmaf(W[j], M[(long)j * XC + hh], v0);
      v1 = fmaf(W[j + 1], M[(long)(j + 1) * XC + hh], v1);
      v2 = fmaf(W[j + 2], M[(long)(j + 2) * XC + hh], v2);
      v3 = fmaf(W[j + 3], M[(long)(j + 3) * XC + hh], v3);
    }
  } else {
    for (int j = 0; j < Hh; j += 4) {
      v0 = fmaf(W[j], M[(long)Hh * XC + j], v0);
      v1 = fmaf(W[j + 1], M[(long)Hh * XC + j + 1], v1);
      v2 = fmaf(W[j + 2], M[(long)Hh * XC + j + 2], v2);
      v3 = fmaf(W[j + 3], M[(long)Hh * XC + j + 3], v3);
    }
  }
  v += (v0 + v1) + (v2 + v3);
  return fmaf(bc, M[(long)Hh * XC + hh], v);
}
// The head's gradient, one thread per entry of [d W_of (C x Hh) | d b_of (C)] in the order (c, hh)
__global__ __launch_bounds__(256) void featg_finish_kernel(const float* params, long p_stride, int off_w, int off_b, int C,
                                                           int Hh, const float* Tm, const float* mom, float* grads) {
  const int XC = Hh + 1;
  const int k = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)C * XC) return;
  const int cc = (int)(i / XC), hh = (int)(i - (long)cc * XC);
  const float* W = params + (long)k * p_stride + off_w + (long)cc * Hh;
  const float bc = params[(long)k * p_stride + off_b + cc];
  const float gr = featg_head_grad(W, bc, mom + (long)k * XC * XC, Tm[(long)k * C * XC + i], hh, Hh, XC);
  grads[(long)k * p_stride + (hh < Hh ? off_w + (long)cc * Hh + hh : off_b + cc)] = gr;
}

// featg_finish_kernel + the head's AdamW in one launch (the one-launch background iteration with an optimiser attached):
// the entry's gradient is formed from the COPY of [W_of | b_of] (FeatPrepTask; a gradient needs a whole row of W_of that
// other threads of this launch are stepping) and stepped at once as the feature group [lo2, hi2) (objnerf_step_tail.h),
// whose counter the reduction launch has already advanced in the other bank.
struct FeatFinishOpt {
  float* params; float* m; float* v; const int* flags; int* steps; int bank;      // (steps: read only)
  double lr, b1, b2, wd; float eps;
};
__global__ __launch_bounds__(256) void featg_finish_adamw_kernel(const float* snap, long p_stride, int off_w, int off_b, int C,
                                                                 int Hh, const float* Tm, const float* mom, float* grads,
                                                                 const FeatFinishOpt o) {
  const int XC = Hh + 1;
  const int k = blockIdx.y;
  __shared__ float s_step, s_bc2;
  __shared__ int s_act;
  if (threadIdx.x == 0)      // (group 2: skipped when no ray has label 1)
    adamw_group_begin(2, o.flags[0] != 0, o.flags[1] != 0, o.steps, o.bank, o.lr, o.b1, o.b2, false, s_act, s_step, s_bc2);
  __syncthreads();
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)C * XC) return;
  const int cc = (int)(i / XC), hh = (int)(i - (long)cc * XC);
  const float* hs = snap + (long)k * ((long)C * XC);
  const float gr = featg_head_grad(hs + (long)cc * Hh, hs[(long)C * Hh + cc], mom + (long)k * XC * XC,
                                   Tm[(long)k * C * XC + i], hh, Hh, XC);
  const long idx = (long)k * p_stride + (hh < Hh ? off_w + (long)cc * Hh + hh : off_b + cc);
  grads[idx] = gr;
  if (s_act) {
    float decay, w1, beta2, w2;
    adamw_coeffs(o.lr, o.b1, o.b2, o.wd, decay, w1, beta2, w2);
    adamw_update(o.params, o.m, o.v, idx, gr, decay, w1, beta2, w2, s_step, s_bc2, o.eps);
  }
}

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }


// workspace carve (floats)
struct WS {
  float *emb, *h1, *h2, *h3, *h4, *hc, *hf, *alpha, *color, *d_alpha, *d_color, *dhead;
  float *d_hf, *rayin, *gram, *rayfeat, *X1, *X2, *Tm, *mom;      // feature branch (hoisted head)
  float *dA, *dB_, *dC, *dD, *dE, *d_emb, *dBpe, *pts;
  float* parts; size_t parts_floats;      // split-K partial slabs of the step's weight-gradient GEMMs (wgrad())
  float* loss_part;                       // [K R][4] block partials of the loss terms
  float* packb;                           // [K][90112] 16-bit: packed B image of the AFULL layer GEMM in flight
  size_t act_floats;                      // room of each of h1 .. hc (floats)
  int* counts;
  size_t bytes;
};

// the 16-bit modes keep h1 .. hc in the operand type when the resident-panel GEMMs serve the shape (hidden 256, >= 4096
// samples per object): those five buffers then take half the room
static bool acts16_shape(int H, long n) { return H == 256 && n >= 4096; }
static WS carve(char* base, int H, int C, long n, long R, int K, bool feat, bool half_acts = false) {
  WS w;
  char* p = base;
  auto take = [&](size_t floats) { float* r = (float*)p; p += al(floats * 4); return r; };
  w.emb = take((size_t)K * n * OBJ_EMB);
  const size_t act = half_acts ? (size_t)K * n * H / 2 : (size_t)K * n * H;
  w.h1 = take(act); w.h2 = take(act); w.h3 = take(act); w.h4 = take(act); w.hc = take(act);
  w.act_floats = act;
  w.hf = feat ? take((size_t)K * n * H) : nullptr;
  w.d_hf = feat ? take((size_t)K * n * H) : nullptr;
  w.rayin = feat ? take((size_t)K * R * (H + 2)) : nullptr;
  w.gram = feat ? take((size_t)K * ((size_t)H * H + H + 1)) : nullptr;
  w.rayfeat = feat ? take((size_t)K * R * (H + 3)) : nullptr;
  w.X1 = feat ? take((size_t)K * R * (H + 1)) : nullptr;
  w.X2 = feat ? take((size_t)K * R * (H + 1)) : nullptr;
  w.Tm = feat ? take((size_t)K * C * (H + 1) + (size_t)K * (H + 1) * (H + 1)) : nullptr;   // Tm | mom, zeroed together
  w.mom = feat ? w.Tm + (size_t)K * C * (H + 1) : nullptr;
  w.alpha = take((size_t)K * n); w.color = take((size_t)K * n * 3);
  w.d_alpha = take((size_t)K * n); w.d_color = take((size_t)K * n * 3);
  w.dhead = take((size_t)K * n * 4);
  w.dA = take(act); w.dB_ = take(act); w.dC = take(act); w.dD = take(act); w.dE = take(act);
  w.d_emb = take((size_t)K * n * OBJ_EMB);
  w.dBpe = take((size_t)K * 64);
  w.pts = take((size_t)K * n * 3);          // sample positions of the origins / directions form of the batch
  {
    // every weight-gradient GEMM of the step with its own slice count (wgrad()): (M, N, samples, has bias)
    const size_t XC = (size_t)H + 1, Hs = (size_t)H;
    size_t tot = 0;
    auto add = [&](int M, int N, long ns, bool bias) {
      tot += (size_t)K * wgrad_slices(K, M, N, ns) * ((size_t)M * N + (bias ? M : 0)) + 128;
    };
    add(H, H, n, true); add(H, OBJ_E2, n, false);          // colour layer
    add(H, H, n, true);                                    // mid2
    add(H, H, n, true); add(H, OBJ_E1, n, false);          // cat layer
    add(H, H, n, true);                                    // mid1
    add(H, OBJ_E1, n, true);                               // in layer
    add(1, H, n, true); add(3, H, n, true);                // heads (H > 256 only)
    if (feat) {
      add(H, H, n, true); add(H, OBJ_E2, n, false);        // feature layer
      add(C, (int)XC, R, false); add((int)XC, (int)XC, R, false);   // 512-d head moments
    }
    // (+ the block partials of the head weight gradients and of d B: at most 2048 + 1024 blocks of 4 H + 4 / 63 floats)
    w.parts_floats = tot + (size_t)(2048 + K) * (4 * Hs + 68) + (size_t)K * 1024 * 64;
    w.parts = take(w.parts_floats);
    w.loss_part = take((size_t)K * R * 4);
    w.packb = H > 128 ? take((size_t)K * 45056) : nullptr;
  }
  w.counts = (int*)take((size_t)2 * K + 2);
  w.bytes = (size_t)(p - base);
  return w;
}

size_t train_workspace_bytes(const objnerf_net* net, int K, int R, int S, int feat, int sixteen) {
  WS w = carve(nullptr, net->hidden, net->feat_dim, (long)R * S, (long)R, K, feat != 0,
               sixteen && acts16_shape(net->hidden, (long)R * S));
  size_t need = w.bytes + 256;
  if (net->hidden == 256 && (S == 32 || S == 64 || S == 128)) {      // the fused hidden-256 path (16-bit modes)
    const size_t n256 = obj256::workspace_bytes(K, R, S, feat, net->feat_dim);
    if (n256 > need) need = n256;
  }
  return need;
}

}  // namespace objgen

// objnerf_context: the helper stream + events of the layer-wise path, owned by the CALLER (objnerf_context_create /
// _destroy are the only entries of the library that create anything).  Without one every launch stays on `stream`.
struct objnerf_context {
  static constexpr int NEV = 16;
  hipStream_t s = nullptr;             // the side stream train_step forks onto
  hipEvent_t ev[NEV];                  // fork events, used round-robin
  hipEvent_t done, done_all;           // joins: the feature preparation, the whole side stream
  bool own = false;                    // false: single-stream stand-in (s = the caller's stream, no events)
};

extern "C" int objnerf_context_create(objnerf_context** out) {
  if (!out) return OBJNERF_EINVAL;
  objnerf_context* c = new objnerf_context();
  bool ok = hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking) == hipSuccess;   // never synchronises with the null stream
  for (int i = 0; i < objnerf_context::NEV; ++i) ok &= hipEventCreateWithFlags(&c->ev[i], hipEventDisableTiming) == hipSuccess;
  ok &= hipEventCreateWithFlags(&c->done, hipEventDisableTiming) == hipSuccess;
  ok &= hipEventCreateWithFlags(&c->done_all, hipEventDisableTiming) == hipSuccess;
  c->own = true;
  if (!ok) { delete c; return OBJNERF_ELAUNCH; }
  *out = c;
  return OBJNERF_OK;
}

extern "C" int objnerf_context_destroy(objnerf_context* c) {
  if (!c) return OBJNERF_OK;
  if (c->own) {
    (void)hipStreamDestroy(c->s);
    for (int i = 0; i < objnerf_context::NEV; ++i) (void)hipEventDestroy(c->ev[i]);
    (void)hipEventDestroy(c->done);
    (void)hipEventDestroy(c->done_all);
  }
  delete c;
  return OBJNERF_OK;
}

namespace objgen {
namespace {
typedef objnerf_context Side;
}  // namespace

// test hook (objnerf_train_args.relu_masks): one thread per (object, sample, byte of 8 features)
__global__ void relu_mask_kernel(long nb, int H, const float* act /* [K n][H] */, uint8_t* masks /* [K n][6][H/8] */,
                                 int layer, int act_mode) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  const int hb = H / 8;
  const long s = i / hb;
  const int b = (int)(i - s * hb);
  unsigned m = 0;
  for (int j = 0; j < 8; ++j) m |= (act_ld(act, s * H + 8 * b + j, act_mode) > 0.0f ? 1u : 0u) << j;
  masks[(s * 6 + layer) * hb + b] = (uint8_t)m;
}

// pts = (origin + dir * z) - centre, two roundings as vmap.py:548-551 (the fused kernels form it in registers; the
// layer-wise path reads the points three times and keeps them in its workspace)
__global__ void form_points_kernel(long total, int S, const float* origins, const float* dirs, const float* z, float centre,
                                   float* pts) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long ray = i / S;
  const float zz = z[i];
#pragma unroll
  for (int x = 0; x < 3; ++x) pts[i * 3 + x] = (origins[ray * 3 + x] + dirs[ray * 3 + x] * zz) - centre;
}

// ------------------------------------------------------------------------------------------------
// The OccupancyMap chain (model.py:61-103), described once:  in -> mid1 -> cat(+x1) -> mid2 -> colour(+x2) -> heads,
// with the feature layer (+x2) beside the colour layer.  train_step, train_step_small, eval_points and mlp_backward
// emit their layer GEMMs through layer_fwd / layer_wgrad / layer_dgrad: a layer's operand strides are written here only.
constexpr int T_TRAINED_END = OBJNERF_T_FL_W;      // off[..]: end of the tensors that always receive a gradient
constexpr int T_FEAT_END = OBJNERF_T_PE_B;         // off[..]: end of the feature branch (feature layer + 512-d head)
enum { L_IN, L_M1, L_CAT, L_M2, L_CL, L_FL };
struct LayerDesc {
  int w, b;            // OBJNERF_T_* of the weight [H][ld] and the bias [H]
  int in_main;         // width of the main input: E1 (the in layer reads x1 = emb[:, 0 : E1) itself) or H
  int in_side;         // width of the side input behind the main one in the weight's rows (0: none) ...
  int side_col;        // ... and its first column of emb (x1: 0, x2: E1)
  int ld() const { return in_main + in_side; }
  bool from_emb() const { return w == OBJNERF_T_IN_W; }
};
static LayerDesc layer_desc(int l, int H) {
  switch (l) {
    case L_IN: return {OBJNERF_T_IN_W, OBJNERF_T_IN_B, OBJ_E1, 0, 0};
    case L_M1: return {OBJNERF_T_M1_W, OBJNERF_T_M1_B, H, 0, 0};
    case L_CAT: return {OBJNERF_T_CAT_W, OBJNERF_T_CAT_B, H, OBJ_E1, 0};
    case L_M2: return {OBJNERF_T_M2_W, OBJNERF_T_M2_B, H, 0, 0};
    case L_CL: return {OBJNERF_T_CL_W, OBJNERF_T_CL_B, H, OBJ_E2, OBJ_E1};
    default: return {OBJNERF_T_FL_W, OBJNERF_T_FL_B, H, OBJ_E2, OBJ_E1};
  }
}
// one call's view of the K stacked networks and its activation / gradient buffers ([K][n][H] each, NULL: not present)
struct NetView {
  const float* P; float* G; long ps; const int64_t* off; int K; long n; int H;
  const float* emb; float* d_emb;                           // [K][n][OBJ_EMB]
  float *h1, *h2, *h3, *h4, *hc, *hf;
  float *d_hc, *d_h4, *d_h3, *d_h2, *d_h1, *d_hf;
  // storage of those buffers: act16 -- h1 .. hc and d_hc .. d_h1 hold the step's 16-bit operand type (the 16-bit modes at
  // hidden 256, train_step_small in bf16 mode); hf16 -- so do hf and d_hf (train_step_small in bf16 mode only).  emb,
  // d_emb, parameters and gradients are always fp32.
  bool act16, hf16;
  float grad_scale;    // d_hc .. d_h1, d_hf are stored multiplied by this power of two (Gemm::a_scale; fp16 mode)
  bool out16(const LayerDesc& L) const { return L.w == OBJNERF_T_FL_W ? hf16 : act16; }      // a layer's out / d_out
};
// the [K][n][ld] operands of a layer: its main input (an activation, or x1 of emb) and its side input (columns of emb)
static Operand main_rows(const NetView& c, const LayerDesc& L, const float* h) {
  return L.from_emb() ? op_rows(c.emb, OBJ_EMB, c.n * OBJ_EMB) : op_rows(h, c.H, c.n * c.H, c.act16);
}
static Operand side_rows(const NetView& c, const LayerDesc& L) { return op_rows(c.emb + L.side_col, OBJ_EMB, c.n * OBJ_EMB); }

// out = relu([in | side] W^T + b).  fuse2: [in | side] as ONE contraction (the resident-panel kernel reads the side
// input as its second A source: no round trip of the partial result)
static void layer_fwd(GemmStep& E, hipStream_t st, const NetView& c, const LayerDesc& L, const float* in, float* out,
                      bool fuse2 = false) {
  const int H = c.H, K = c.K, M = (int)c.n;
  const long ps = c.ps;
  const Operand a = main_rows(c, L, in), s = side_rows(c, L), o = op_rows(out, H, c.n * H, c.out16(L));
  const float *W = c.P + c.off[L.w], *b = c.P + c.off[L.b];
  if (!L.in_side || fuse2) {
    GemmOpts f = {.relu = true, .bias = b, .bsbias = ps};
    if (L.in_side) f.a2 = A2Src{s.p, s.s0, s.bs, L.in_main};
    gemm(E, st, K, M, H, L.ld(), a, op_cols(W, L.ld(), ps), o, f);
  } else {
    gemm(E, st, K, M, H, L.in_main, a, op_cols(W, L.ld(), ps), o);
    gemm(E, st, K, M, H, L.in_side, s, op_cols(W + L.in_main, L.ld(), ps), o,
         {.accumulate = true, .relu = true, .bias = b, .bsbias = ps});
  }
}
// d W = d_out^T [in | side], d b = column sums of d_out (riding on the main part's GEMM: row sums of its operand tile)
static void layer_wgrad(GemmStep& E, hipStream_t st, const WgradHow& how, const NetView& c, const LayerDesc& L,
                        const float* d_out, const float* in) {
  const int H = c.H, K = c.K;
  const long n = c.n, ps = c.ps;
  const Operand a = main_rows(c, L, in), s = side_rows(c, L), dT = op_cols(d_out, H, n * H, c.out16(L));
  float *dW = c.G + c.off[L.w], *db = c.G + c.off[L.b];
  wgrad(E, st, how, K, H, L.in_main, n, dT, a, op_rows(dW, L.ld(), ps), db, c.grad_scale);
  if (L.in_side) wgrad(E, st, how, K, H, L.in_side, n, dT, s, op_rows(dW + L.in_main, L.ld(), ps), nullptr, c.grad_scale);
}
// d_in (+)= (d_out W_main) o [mask > 0] and d_emb[:, side columns] (+)= d_out W_side; the in layer's input IS x1, so its
// main part lands in d_emb.  fold_dhead (colour layer without the feature branch): the alpha head's rank-1 term
// wa x dhead[:, 0] is added in the epilogue (Gemm::biasrow), so d_in is written once instead of written, read and written.
static void layer_dgrad(GemmStep& E, hipStream_t st, const NetView& c, const LayerDesc& L, const float* d_out, float* d_in,
                        const float* mask, bool accumulate, bool side_accumulate = false, const float* fold_dhead = nullptr) {
  const int H = c.H, K = c.K, M = (int)c.n;
  const long n = c.n, nH = n * H, ps = c.ps;
  const float* W = c.P + c.off[L.w];
  const Operand d = op_rows(d_out, H, nH, c.out16(L));
  const Operand out = L.from_emb() ? op_rows(c.d_emb, OBJ_EMB, n * OBJ_EMB) : op_rows(d_in, H, nH, c.act16);
  GemmOpts o = {.accumulate = accumulate, .a_scale = c.grad_scale};
  if (mask) o.mask = op_rows(mask, H, nH, c.act16);
  if (fold_dhead) {                                                             // (the folded form overwrites)
    o.accumulate = false;
    o.bias = c.P + c.off[OBJNERF_T_ALPHA_W]; o.bsbias = ps;
    o.biasrow = fold_dhead; o.bsbr = n * 4; o.sbr = 4;
  }
  gemm(E, st, K, M, L.in_main, H, d, op_rows(W, L.ld(), ps), out, o);
  if (L.in_side)
    gemm(E, st, K, M, L.in_side, H, d, op_rows(W + L.in_main, L.ld(), ps), op_rows(c.d_emb + L.side_col, OBJ_EMB, n * OBJ_EMB),
         {.accumulate = side_accumulate, .a_scale = c.grad_scale});
}
// h1 .. hc, alpha / color and (hf != NULL) the feature layer.  act16: h1 .. hc live in the operand type (train_step)
static void forward_chain(GemmStep& E, hipStream_t st, const NetView& c, float* alpha, float* color, float* hf, int act16) {
  const int H = c.H;
  const bool fuse2 = panel_ok(E, (int)c.n, H, H + OBJ_E1, 1, 1, false, c.K) && H == 256;
  layer_fwd(E, st, c, layer_desc(L_IN, H), nullptr, c.h1);
  layer_fwd(E, st, c, layer_desc(L_M1, H), c.h1, c.h2);
  layer_fwd(E, st, c, layer_desc(L_CAT, H), c.h2, c.h3, fuse2);
  layer_fwd(E, st, c, layer_desc(L_M2, H), c.h3, c.h4);
  layer_fwd(E, st, c, layer_desc(L_CL, H), c.h4, c.hc, fuse2);
  hipLaunchKernelGGL(heads_fwd_kernel, dim3((unsigned)((c.n + 15) / 16), (unsigned)c.K), dim3(256),
                     (size_t)4 * H * sizeof(float), st, H, c.n, c.h4, c.hc, c.P, c.ps, (int)c.off[OBJNERF_T_ALPHA_W],
                     (int)c.off[OBJNERF_T_ALPHA_B], (int)c.off[OBJNERF_T_OC_W], (int)c.off[OBJNERF_T_OC_B], alpha, color, act16);
  if (hf) layer_fwd(E, st, c, layer_desc(L_FL, H), c.h4, hf);
}
// the weight gradients alone (the dgrad chain ran in a kernel of its own): colour, mid2, cat, mid1, in; the feature
// layer first (train_step's small-batch branch) or last (train_step_small) -- GemmGroup slots and slab addresses follow
static void wgrad_chain(GemmStep& E, hipStream_t st, const WgradHow& how, const NetView& c, bool feat, bool feat_first) {
  const int H = c.H;
  if (feat && feat_first) layer_wgrad(E, st, how, c, layer_desc(L_FL, H), c.d_hf, c.h4);
  layer_wgrad(E, st, how, c, layer_desc(L_CL, H), c.d_hc, c.h4);
  layer_wgrad(E, st, how, c, layer_desc(L_M2, H), c.d_h4, c.h3);
  layer_wgrad(E, st, how, c, layer_desc(L_CAT, H), c.d_h3, c.h2);
  layer_wgrad(E, st, how, c, layer_desc(L_M1, H), c.d_h2, c.h1);
  layer_wgrad(E, st, how, c, layer_desc(L_IN, H), c.d_h1, nullptr);
  if (feat && !feat_first) layer_wgrad(E, st, how, c, layer_desc(L_FL, H), c.d_hf, c.h4);
}
// the layer-wise backward from d_hc / d_h4 (heads_bwd_kernel) and d_hf: per layer the weight gradient on `wst` and the
// input gradient on `st`; fork() runs ahead of every layer but the feature layer (whose caller has just forked).
// d_emb needs no zero fill: the first dgrad into each column block overwrites (x2: feature layer if present, else
// colour layer; x1: cat layer), later ones accumulate; columns 0..2 (d t) are never read.
template <class Fork>
static void backward_chain(GemmStep& E, hipStream_t st, hipStream_t wst, const NetView& c, bool feat,
                           const float* fold_dhead, Fork fork) {
  const int H = c.H;
  if (feat) {     // feature layer: grads + contributions to d_h4 / d_x2
    const LayerDesc L = layer_desc(L_FL, H);
    layer_wgrad(E, wst, {}, c, L, c.d_hf, c.h4);
    layer_dgrad(E, st, c, L, c.d_hf, c.d_h4, nullptr, true, false);
  }
  const struct { int l; const float* d_out; float* h; float* d_in; bool acc; } steps[5] = {
      {L_CL, c.d_hc, c.h4, c.d_h4, true},       // colour layer (acc is IGNORED with fold_dhead: that form overwrites d_h4)
      {L_M2, c.d_h4, c.h3, c.d_h3, false},      // mid2:  d_h4 (masked above) -> grads, d_h3
      {L_CAT, c.d_h3, c.h2, c.d_h2, false},     // cat layer
      {L_M1, c.d_h2, c.h1, c.d_h1, false},      // mid1
      {L_IN, c.d_h1, nullptr, nullptr, true}};  // in layer
  for (const auto& s : steps) {
    const LayerDesc L = layer_desc(s.l, H);
    fork();
    layer_wgrad(E, wst, {}, c, L, s.d_out, s.h);
    layer_dgrad(E, st, c, L, s.d_out, s.d_in, s.h, s.acc, s.l == L_CL && feat, s.l == L_CL ? fold_dhead : nullptr);
  }
}
// ordered reductions into the gradient arena: a head's block partials [K][sk][rows][H] + [K][sk][rows], d B's [K][sk][63]
static RedItem head_red_item(const NetView& c, int t_w, int t_b, int rows, const float* part, const float* rs_part, int sk) {
  RedItem r;
  r.part = part; r.rs_part = rs_part; r.C = c.G + c.off[t_w]; r.rowsum = c.G + c.off[t_b];
  r.M = rows; r.N = c.H; r.sk = sk; r.batch = c.K; r.scm = c.H; r.bsc = c.ps; r.bsrs = c.ps;
  return r;
}
// workgroups of pe_bwd_kernel per object: 12 samples per block and pass, at least 4 passes per block
static int pe_bwd_blocks(long n) { return (int)std::min(std::max((n + 47) / 48, 1L), 1024L); }
static RedItem pe_red_item(const NetView& c, const float* part, int sk) {
  RedItem r;
  r.part = part; r.rs_part = nullptr; r.C = c.G + c.off[OBJNERF_T_PE_B]; r.rowsum = nullptr;
  r.M = 1; r.N = 63; r.sk = sk; r.batch = c.K; r.scm = 63; r.bsc = c.ps; r.bsrs = 0;
  return r;
}
// the parameter offsets of the one-launch kernels' argument structs (FwdSmall, BwdSmall, SmallFused)
template <class T> static void set_weight_offsets(T& f, const int64_t* off) {
  f.o_in_w = (int)off[OBJNERF_T_IN_W]; f.o_m1_w = (int)off[OBJNERF_T_M1_W]; f.o_cat_w = (int)off[OBJNERF_T_CAT_W];
  f.o_m2_w = (int)off[OBJNERF_T_M2_W]; f.o_cl_w = (int)off[OBJNERF_T_CL_W]; f.o_fl_w = (int)off[OBJNERF_T_FL_W];
}
template <class T> static void set_forward_offsets(T& f, const int64_t* off) {
  set_weight_offsets(f, off);
  f.o_in_b = (int)off[OBJNERF_T_IN_B]; f.o_m1_b = (int)off[OBJNERF_T_M1_B]; f.o_cat_b = (int)off[OBJNERF_T_CAT_B];
  f.o_m2_b = (int)off[OBJNERF_T_M2_B]; f.o_cl_b = (int)off[OBJNERF_T_CL_B]; f.o_fl_b = (int)off[OBJNERF_T_FL_B];
  f.o_a_w = (int)off[OBJNERF_T_ALPHA_W]; f.o_a_b = (int)off[OBJNERF_T_ALPHA_B];
  f.o_oc_w = (int)off[OBJNERF_T_OC_W]; f.o_oc_b = (int)off[OBJNERF_T_OC_B];
}

// ---- the hoisted 512-d feature head on the caller's GemmStep and stream.  The head is NOT applied per
// sample: per object G = W_of^T W_of (+ wb, bb), per ray u = W_of^T g, beta, |g| ahead of the loss; behind it the head's
// gradient d W_of = gt_feat^T [a fh] + W_of M2 + b_of m1^T, d b_of = gt_feat^T [a O] + W_of m1 + b_of s2 from the moments
// [M2 m1; . s2] = [c fh | c O]^T [fh | O]: two split-K GEMMs over the rays + a small finish
static void feat_gram_gemm(GemmStep& E, hipStream_t st, const FeatHeadArgs& h, float* gram, long gst, GroupLaunch* group = nullptr) {
  const float* W = h.P + h.off_w;
  gemm(E, st, h.K, h.Hh, h.Hh, h.C, op_cols(W, h.Hh, h.ps), op_rows(W, h.Hh, h.ps), op_rows(gram, h.Hh, gst), {.group = group});
}
static void feat_rays_gemm(GemmStep& E, hipStream_t st, const FeatHeadArgs& h, float* rayin, GroupLaunch* group = nullptr) {
  const long R = h.R;
  gemm(E, st, h.K, h.R, h.Hh, h.C, op_rows(h.gt_feat, h.C, R * h.C), op_rows(h.P + h.off_w, h.Hh, h.ps),
       op_rows(rayin, h.Hh + 2, R * (h.Hh + 2)), {.group = group});
}
static void feat_gram_enqueue(GemmStep& E, hipStream_t st, const FeatHeadArgs& h, float* gram, long gst) {
  feat_gram_gemm(E, st, h, gram, gst);
  hipLaunchKernelGGL(featg_wb_kernel, dim3(h.Hh + 1, h.K), dim3(64), 0, st, h.P, h.ps, h.off_w, h.off_b, h.C, h.Hh, gram, gst);
}
static void feat_prep_enqueue(GemmStep& E, hipStream_t st, const FeatHeadArgs& h, const FeatHead& f) {
  feat_gram_enqueue(E, st, h, f.gram, (long)h.Hh * h.Hh + h.Hh + 1);
  feat_rays_gemm(E, st, h, f.rayin);
  hipLaunchKernelGGL(featg_rowstats_kernel, dim3((unsigned)((h.R + 15) / 16), h.K), dim3(256), 0, st, h.P, h.ps, h.off_b, h.C,
                     h.R, h.Hh + 2, h.gt_feat, f.rayin);
}
// T = gt_feat^T [a fh | a O], M = [c fh | c O]^T [fh | O] over the rays (X1 / X2: featg_scale_kernel or the fused kernel);
// targets and moments, not back-propagated gradients: no gradient scale
static void feat_moments_enqueue(GemmStep& E, hipStream_t st, const WgradHow& how, const FeatHeadArgs& h, const FeatHead& f) {
  const int XC = h.Hh + 1;
  const long R = h.R;
  wgrad(E, st, how, h.K, h.C, XC, R, op_cols(h.gt_feat, h.C, R * h.C), op_rows(f.X1, XC, R * XC), op_rows(f.Tm, XC, (long)h.C * XC));
  wgrad(E, st, how, h.K, XC, XC, R, op_cols(f.X2, XC, R * XC), op_rows(f.rayfeat, h.Hh + 3, R * (h.Hh + 3)),
        op_rows(f.mom, XC, (long)XC * XC));
}
// d W_of = T + W_of M + b_of m^T, d b_of likewise
static void feat_finish_enqueue(hipStream_t st, const FeatHeadArgs& h, const FeatHead& f, float* grads) {
  hipLaunchKernelGGL(featg_finish_kernel, dim3((unsigned)(((long)h.C * (h.Hh + 1) + 255) / 256), h.K), dim3(256), 0, st, h.P,
                     h.ps, h.off_w, h.off_b, h.C, h.Hh, f.Tm, f.mom, grads);
}
static FeatHeadArgs feat_head_args(const NetView& c, int R, int C, const float* gt_feat) {
  return {c.K, R, c.H, C, c.P, c.ps, (int)c.off[OBJNERF_T_OF_W], (int)c.off[OBJNERF_T_OF_B], gt_feat};
}
static NetView net_view(const WS& w, const float* P, float* G, long ps, const int64_t* off, int K, long n, int H) {
  NetView c;
  c.P = P; c.G = G; c.ps = ps; c.off = off; c.K = K; c.n = n; c.H = H;
  c.emb = w.emb; c.d_emb = w.d_emb;
  c.h1 = w.h1; c.h2 = w.h2; c.h3 = w.h3; c.h4 = w.h4; c.hc = w.hc; c.hf = w.hf;
  c.d_hc = w.dA; c.d_h4 = w.dB_; c.d_h3 = w.dC; c.d_h2 = w.dD; c.d_h1 = w.dE; c.d_hf = w.d_hf;
  c.act16 = c.hf16 = false; c.grad_scale = 1.0f;      // (fp32 storage; the 16-bit steps say otherwise)
  return c;
}
// the step's constants from its carve
static GemmStep gemm_step(const WS& w, int operands, int K) {
  GemmStep E;
  E.operands = operands;
  E.parts = w.parts; E.parts_cap = w.parts_floats;
  E.packb = w.packb; E.packb_entries = w.packb ? K : 0;
  return E;
}
// test hook (objnerf_train_args.relu_masks): the iteration's ReLU branch bits; act16 / hf16: storage type of h1 .. hc / hf
static void emit_relu_masks(hipStream_t st, const NetView& c, uint8_t* masks, int act16, int hf16) {
  const float* acts[6] = {c.h1, c.h2, c.h3, c.h4, c.hc, c.hf};
  const long nb = (long)c.K * c.n * (c.H / 8);
  for (int l = 0; l < 6; ++l)
    if (acts[l])
      hipLaunchKernelGGL(relu_mask_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, nb, c.H, acts[l], masks, l,
                         l < 5 ? act16 : hf16);
}
static FeatHead feat_head_view(const WS& w) { return {w.gram, w.rayin, w.rayfeat, w.X1, w.X2, w.Tm, w.mom, nullptr, 0}; }

// The one-launch small-batch iteration: train_small_kernel -> the seven weight-gradient GEMMs as ONE grouped launch ->
// ONE reduction launch (weight-gradient slices, head / d B / loss partials, status, optionally AdamW).  Everything on
// the caller's stream: three dependent launches need no helper stream and no events.
static int train_step_small(const objnerf_net* net, const objnerf_train_args* a, hipStream_t st, const WS& w,
                            const int64_t* off, bool bf, int* done) {
  const int H = net->hidden, K = a->K, S = a->S, C = net->feat_dim;
  // every GEMM of this step goes through a grouped launch, which has its own operand type (bf16 mode: the weight
  // gradients' group); whatever a group does not take is an fp32 GEMM
  GemmStep E = gemm_step(w, 0, K);
  const long n = (long)a->R * S, ps = a->p_stride;
  const bool feat = a->gt_feat != nullptr;
  const int rpw = sf_rays_per_wg(S, feat);
  const int nwg = (int)(((long)a->R + rpw - 1) / rpw);
  const float* P = a->params;
  float* G = a->grads;
  NetView c = net_view(w, P, G, ps, off, K, n, H);
  // bf16 mode: train_small_kernel stores h1 .. hc (hf, d_hf) and d_hc .. d_h1 as bf16 (objnerf_small_body.h, `hst`); the
  // grouped launch passes them through unconverted
  c.act16 = bf; c.hf16 = bf && a->gt_feat != nullptr;
  const FeatHeadArgs fh = feat_head_args(c, a->R, C, a->gt_feat); const FeatHead fhb = feat_head_view(w);
  const bool self_counts = (a->mode & OBJNERF_TRAIN_SELF_COUNTS) != 0;
  if (self_counts && K > 1) {        // several objects: the cross-object flags need every object's labels (one small launch)
    const int rc0 = objnerf_label_counts(K, a->R, a->labels, const_cast<int32_t*>(a->counts), const_cast<int32_t*>(a->flags),
                                         (void*)st);
    if (rc0) return rc0;
  }
  const long R = a->R;
  const int XC = H + 1;
  float* head_snap = nullptr;          // [K][C (H + 1)]: [W_of | b_of] before the step (FeatPrepTask), for the fused finish + AdamW
  if (feat) {
    // the 512-d head's preparation does not depend on the forward pass: ahead of the fused launch
    const long gst = (long)H * H + H + 1;
    // Round 6: ONE launch for the four (the two GEMMs as a group, wb / bb, the rays' beta and |g| and -- with an optimiser
    // attached -- the copy of [W_of | b_of] the head's finish reads, as extra workgroups of the same launch: FeatPrepTask)
    head_snap = a->optim ? E.parts_alloc((size_t)K * C * XC) : nullptr;
    GroupLaunch g0;
    feat_gram_gemm(E, st, fh, w.gram, gst, &g0);
    feat_rays_gemm(E, st, fh, w.rayin, &g0);
    if (E.error) return OBJNERF_EINVAL;
    if (g0.g.count == 2) {
      FeatPrepTask& t = g0.g.task;
      t.params = P; t.ps = ps; t.off_w = fh.off_w; t.off_b = fh.off_b; t.C = C; t.Hh = H; t.R = (int)R; t.rin_ld = H + 2;
      t.K = K; t.gt_feat = a->gt_feat; t.rayin = w.rayin; t.gram = w.gram; t.gstride = gst; t.snap = head_snap;
      t.nb_wb = (H + 1 + 7) / 8; t.nb_rs = (int)((R + 31) / 32);
      t.nb_snap = head_snap ? (int)(((long)C * XC + 2047) / 2048) : 0;
      t.blocks = K * (t.nb_wb + t.nb_rs + t.nb_snap);
      group_launch(st, g0);
    } else {      // (cannot happen for these shapes: the group is dropped, all four launches are redone ungrouped)
      head_snap = nullptr;
      feat_prep_enqueue(E, st, fh, fhb);
    }
  }
  SmallFused f;
  f.K = K; f.R = a->R; f.S = S; f.rpw = rpw;
  f.fs = a->feat_scaling;
  f.rayin = w.rayin; f.gram = w.gram; f.hf = w.hf; f.d_hf = w.d_hf; f.rayfeat = w.rayfeat; f.X1 = w.X1; f.X2 = w.X2;
  f.params = P; f.ps = ps; f.scale = a->scale;
  f.pts = a->pts; f.origins = a->origins; f.dirs = a->dirs; f.z = a->z; f.centre = a->obj_center;
  f.gt_depth = a->gt_depth; f.gt_rgb = a->gt_rgb; f.labels = a->labels;
  f.counts = const_cast<int*>(a->counts); f.flags = const_cast<int*>(a->flags); f.self_counts = (self_counts && K == 1) ? 1 : 0;
  f.cs = a->color_scaling; f.os = a->opacity_scaling;
  f.emb = w.emb; f.h1 = w.h1; f.h2 = w.h2; f.h3 = w.h3; f.h4 = w.h4; f.hc = w.hc;
  f.d_hc = c.d_hc; f.d_h4 = c.d_h4; f.d_h3 = c.d_h3; f.d_h2 = c.d_h2; f.d_h1 = c.d_h1;
  // per-workgroup partials live in workspace regions this path does not use otherwise (d_emb: K n 129 floats, dhead:
  // K n 4, loss_part: K R 4): objnerf_train_step's applicability test checked that they fit
  float* hp = w.d_emb;
  f.partA = hp; hp += (size_t)K * nwg * H;
  f.partW = hp; hp += (size_t)K * nwg * 3 * H;
  f.rsA = hp; hp += (size_t)K * nwg;
  f.rsW = hp;
  f.pe_part = w.dhead;
  f.loss_part = w.loss_part;
  set_forward_offsets(f, off);
  f.o_B = (int)off[OBJNERF_T_PE_B];
  if (feat) {
    if (rpw * S <= 64) launch_train_small<4, true>(st, f, nwg, bf);
    else launch_train_small<5, true>(st, f, nwg, bf);
  } else {
    if (rpw * S <= 64) launch_train_small<4, false>(st, f, nwg, bf);
    else launch_train_small<5, false>(st, f, nwg, bf);
  }
  if (hipGetLastError() != hipSuccess) return OBJNERF_ELAUNCH;
  if (a->relu_masks) emit_relu_masks(st, c, a->relu_masks, bf ? 1 : 0, bf ? 1 : 0);
  // ---- the step's reductions, collected: head partials, d B partials, the weight gradients' split-K slices
  RedGroup red;
  red.count = 0;
  const RedItem partials[3] = {head_red_item(c, OBJNERF_T_ALPHA_W, OBJNERF_T_ALPHA_B, 1, f.partA, f.rsA, nwg),
                               head_red_item(c, OBJNERF_T_OC_W, OBJNERF_T_OC_B, 3, f.partW, f.rsW, nwg),
                               pe_red_item(c, f.pe_part, nwg)};
  red_emit(st, &red, partials, 3);
  // Split-K slices of the grouped launch: its seven GEMMs are ONE 128 x 128 tile each, so `slices` is also the number of
  // workgroups per GEMM.  ~2 rounds of the chip (7 x 37 = 259 workgroups at least), at most ~1024 samples per slice
  // beyond that: every slice writes its partial tile to HBM and the reduction reads it back -- 128 slices at the
  // benchmark's 76 800 background samples were 48 MB each way for 0.4 MB of gradient (reduction 131 us).
  int max_slices;
  {
    long want = (n + 1023) / 1024;
    if (want < 36) want = 36;
    // whole rounds of the chip: 7 GEMMs x slices workgroups on num_cu compute units (75 slices = 525 workgroups left a
    // third round for 13 of them: 260 us against 227)
    const int cu = 256, ng = feat ? 9 : 7;
    long rounds = (want * ng + cu / 2) / cu;
    if (rounds < 1) rounds = 1;
    max_slices = (int)(rounds * cu / ng);
  }
  // (need_parts: no zero-filled gradient arena here -- the deterministic slab form or an error)
  GroupLaunch group(bf, max_slices, &red);
  wgrad_chain(E, st, {.group = &group, .need_parts = true}, c, feat, false);      // (the feature layer LAST here: the slots of
                                                                                  // the other seven do not move with it)
  if (E.parts_failed || E.error) return OBJNERF_EINVAL;
  group_launch(st, group);
  if (feat) {
    // the 512-d head's moments over the RAYS (featg_finish_kernel turns them into d W_of, d b_of after the reduction).
    // A grouped launch of their own: inside the other one their 512-row output made it 5x slower (1.82 against 0.35 ms
    // at the benchmark's background batch -- every GEMM of the group is then launched over four row tiles)
    GroupLaunch g2(false, 0, &red);
    feat_moments_enqueue(E, st, {.group = &g2, .need_parts = true}, fh, fhb);
    if (E.parts_failed || E.error) return OBJNERF_EINVAL;
    group_launch(st, g2);                // (launches whatever was collected; GEMMs the group does not take were launched at once)
  }
  red.tail.loss_part = f.loss_part; red.tail.loss_blocks = nwg; red.tail.K = K; red.tail.loss_terms = a->loss_terms;
  red.tail.status = a->status;
  if (a->optim) {
    const objnerf_adamw_args* o = a->optim;
    RedTail& t = red.tail;
    t.params = const_cast<float*>(a->params); t.grads = G; t.m = o->exp_avg; t.v = o->exp_avg_sq; t.flags = a->flags;
    t.steps = o->group_steps; t.bank = o->bank; t.p_stride = ps; t.arena_floats = (long)K * ps;
    t.lo1 = off[OBJNERF_T_CL_W]; t.lo2 = off[OBJNERF_T_FL_W]; t.hi2 = off[OBJNERF_T_PE_B];
    t.lr = (double)o->lr; t.b1 = (double)o->beta1; t.b2 = (double)o->beta2; t.wd = (double)o->weight_decay; t.eps = o->eps;
    if (done) *done |= 2;
  }
  launch_reductions(st, red);
  if (feat && a->optim && head_snap) {
    // the head's gradient AND its AdamW step in one launch, from the copy of [W_of | b_of] (round 6)
    const objnerf_adamw_args* o = a->optim;
    FeatFinishOpt fo;
    fo.params = const_cast<float*>(a->params); fo.m = o->exp_avg; fo.v = o->exp_avg_sq; fo.flags = a->flags;
    fo.steps = o->group_steps; fo.bank = o->bank;
    fo.lr = (double)o->lr; fo.b1 = (double)o->beta1; fo.b2 = (double)o->beta2; fo.wd = (double)o->weight_decay; fo.eps = o->eps;
    hipLaunchKernelGGL(featg_finish_adamw_kernel, dim3((unsigned)(((long)C * XC + 255) / 256), K), dim3(256), 0, st, head_snap, ps,
                       fh.off_w, fh.off_b, C, H, w.Tm, w.mom, G, fo);
  } else if (feat) {
    feat_finish_enqueue(st, fh, fhb, G);
    if (a->optim) {               // the head's own entries [of_w, pe_b): their gradient exists only now
      const objnerf_adamw_args* o = a->optim;
      // (entries [of_w, pe_b) only: "P" = off[PE_B] with [0, of_w) skipped -- B's gradient behind them was stepped
      // by the reduction launch)
      const int rc = objmisc::adamw_flags_range(K, off[OBJNERF_T_PE_B], ps, const_cast<float*>(a->params), G, o->exp_avg,
                                                o->exp_avg_sq, nullptr, a->flags, o->group_steps, o->bank,
                                                off[OBJNERF_T_CL_W], off[OBJNERF_T_FL_W], off[OBJNERF_T_PE_B], 0,
                                                off[OBJNERF_T_OF_W], o->lr, o->beta1, o->beta2, o->eps, o->weight_decay,
                                                (void*)st);
      if (rc) return rc;
    }
  }
  if (hipGetLastError() != hipSuccess) return OBJNERF_ELAUNCH;
  return OBJNERF_OK;
}

int train_step(const objnerf_net* net, const objnerf_train_args* a_in, void* stream, int* done) {
  objnerf_train_args a_local = *a_in;
  const objnerf_train_args* a = &a_local;
  const int operands = (a->mode & OBJNERF_TRAIN_FP16) ? 2 : (a->mode & OBJNERF_TRAIN_BF16) ? 1 : 0;
  const int H = net->hidden, C = net->feat_dim, K = a->K;
  if (H % 32 != 0 || net->n_freqs != 6) return OBJNERF_ENOTSUP;
  const bool feat = a->gt_feat != nullptr;
  const long n = (long)a->R * a->S;
  int64_t off[OBJNERF_N_TENSORS + 1];
  objnerf_param_layout(net, off);
  const long ps = a->p_stride;
  hipStream_t st = (hipStream_t)stream;
  const bool half_acts = (a->mode & (OBJNERF_TRAIN_FP16 | OBJNERF_TRAIN_BF16)) != 0 && acts16_shape(H, n);
  WS w = carve((char*)a->workspace, H, C, n, (long)a->R, K, feat, half_acts);
  if (a->workspace_bytes < w.bytes) return OBJNERF_EINVAL;
  // ---- small batches of the hidden-128 network without the feature loss: ONE forward + loss + backward launch, the
  // grouped weight gradients, one reduction launch (objnerf_small_body.h)
  {
    const int S = a->S;
    const int rpw = S > 0 && S <= 64 ? sf_rays_per_wg(S, feat) : 0;
    const long nwg = rpw ? ((long)a->R + rpw - 1) / rpw : 0;
#ifndef OBJ_NO_SMALL_FUSED
    // (the per-workgroup partials are parked in workspace regions of n = R S rows per object: the d B partials, 63 floats
    // per workgroup, in dhead (4 n floats) and the head partials, 4 H + 4 per workgroup, in d_emb (129 n) -- tiny batches
    // such as R <= 3 with S = 4 do not fit and take the general path)
    if (H == FS_H && S >= 4 && S <= 64 && (long)K * nwg <= 1536 && !half_acts && K <= 65535 &&
        nwg * 63 <= n * 4 && nwg * (4L * H + 4) <= n * 129 &&
        !(a->mode & OBJNERF_TRAIN_LAYERWISE && K > 8) && (!feat || (C % 4 == 0 && a->R >= 1)))
      return train_step_small(net, a, st, w, off, operands == 1, done);
#endif
  }
  GemmStep E = gemm_step(w, operands, K);      // this call's GEMM constants (nothing outlives the call)
  if (a->mode & OBJNERF_TRAIN_SELF_COUNTS) {
    const int rc0 = objnerf_label_counts(K, a->R, a->labels, const_cast<int32_t*>(a->counts), const_cast<int32_t*>(a->flags),
                                         stream);
    if (rc0) return rc0;
  }
  RedGroup step_red;                 // small-batch path: every ordered reduction of the step in ONE launch, after the join
  step_red.count = 0;
  if (!a->pts) {
    const long total = (long)K * n;
    hipLaunchKernelGGL(form_points_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, a->S, a->origins,
                       a->dirs, a->z, a->obj_center, w.pts);
    a_local.pts = w.pts;
  }
  const float* P = a->params;
  float* G = a->grads;
  // 16-bit modes at hidden 256 (configs[4]): h1 .. hc and d_hc .. d_h1 live in the operand type -- written by the forward
  // GEMMs' epilogues, read as panels / masks / weight-gradient operands and by the head kernels (act_ld).  Their buffers
  // keep the fp32 spacing in the workspace.  hf / d_hf stay fp32.
  const int act16 = half_acts ? operands : 0;
  // fp16 operands: every backward GEMM has the back-propagated gradient as its A operand.  Those values are of order
  // (loss scale) / R per ray times a per-sample weight -- mostly below fp16's smallest normal number (6.1e-5) -- so A is
  // scaled by ~8 R (a power of two: exact) before rounding and the product scaled back (Gemm::a_scale).
  const float grad_scale = exp2f(floorf(log2f((float)a->R)) + 3.0f);
  NetView c = net_view(w, P, G, ps, off, K, n, H);
  c.act16 = act16 != 0; c.grad_scale = grad_scale;
  const FeatHeadArgs fh = feat_head_args(c, a->R, C, a->gt_feat); const FeatHead fhb = feat_head_view(w);

  // helper stream: work that only READS what the main chain produced (or, for the feature preparation below, only
  // parameters and inputs) runs beside it; fork = the side stream waits for everything enqueued on `st` so far
  Side single;                                   // no context: one stream, program order replaces every event
  single.s = st;
  Side& sd = a->context ? *(Side*)a->context : single;
  const bool multi = sd.own;
  int fk = 0;
  auto fork = [&]() {
    if (!multi) return;
    (void)hipEventRecord(sd.ev[fk], st);
    (void)hipStreamWaitEvent(sd.s, sd.ev[fk], 0);
    fk = (fk + 1) % Side::NEV;
  };
  hipStream_t ss = sd.s;
  // Weight / bias gradients are accumulated with split-K atomics by GEMMs on the side stream: zero them there, now,
  // off the critical path (feature-branch entries only when they receive a gradient, so "no gradient" stays
  // "untouched").  The previous step's consumer of the gradient arena (AdamW) is ordered before this fork.
  fork();
  for (int k = 0; k < K; ++k) {
    (void)hipMemsetAsync(a->grads + (long)k * ps, 0, (size_t)off[T_TRAINED_END] * 4, ss);
    if (feat)
      (void)hipMemsetAsync(a->grads + (long)k * ps + off[T_TRAINED_END], 0, (size_t)(off[T_FEAT_END] - off[T_TRAINED_END]) * 4, ss);
  }
  if (feat) {
    // None of the head's preparation depends on the forward pass: side stream, joined before the loss.
    feat_prep_enqueue(E, ss, fh, fhb);
    if (multi) (void)hipEventRecord(sd.done, ss);
  }

  // ---- forward
  int rc = objnerf_embed(net, K, n, P, ps, a->scale, a->pts, w.emb, stream);
  if (rc) return rc;
  dim3 eg((unsigned)((n + 15) / 16), (unsigned)K);      // 16 lanes per sample row
  const size_t head_lds = (size_t)4 * H * sizeof(float);
  const int small_rt = small_batch_rt(operands, H, n, K);
  // the small-batch kernels come in fp32 and bf16-MFMA form (fp16 mode: fp32 there); the GEMMs behind them -- the
  // feature head's moments, the grouped weight gradients -- are fp32 whatever the mode (WgradHow::fp32, the group's type)
  const bool small_bf = small_rt && operands == 1;
  if (act16 && !panel_ok(E, (int)n, H, H + OBJ_E1, 1, 1, false, K)) return OBJNERF_EINVAL;      // (cannot happen: same conditions)
  if (small_rt) {
    FwdSmall f;
    f.n = n; f.feat = feat ? 1 : 0; f.params = P; f.ps = ps; f.emb = w.emb;
    f.h1 = w.h1; f.h2 = w.h2; f.h3 = w.h3; f.h4 = w.h4; f.hc = w.hc; f.hf = feat ? w.hf : nullptr;
    f.alpha = w.alpha; f.color = w.color;
    set_forward_offsets(f, off);
    launch_small_rt(st, f, K, small_bf, small_rt);
  } else {
    forward_chain(E, st, c, w.alpha, w.color, w.hf, act16);
  }
  if (a->relu_masks) emit_relu_masks(st, c, a->relu_masks, act16, 0);
  if (feat && multi) (void)hipStreamWaitEvent(st, sd.done, 0);      // the feature preparation (side stream) is needed from here
  // ---- loss + d(alpha, color, clip)      (loss.py:5-103)
  objnerf_loss_args la;
  la.K = K; la.R = a->R; la.S = a->S; la.C = C;
  la.color_scaling = a->color_scaling; la.opacity_scaling = a->opacity_scaling; la.feat_scaling = a->feat_scaling;
  la.reserved = 0;
  la.alpha = w.alpha; la.color = w.color; la.z = a->z; la.gt_depth = a->gt_depth; la.gt_rgb = a->gt_rgb;
  la.labels = a->labels; la.pred_feat = nullptr; la.gt_feat = a->gt_feat; la.flags_in = a->flags;
  la.counts_in = a->counts;
  la.loss_terms = a->loss_terms; la.total = nullptr; la.d_alpha = w.d_alpha; la.d_color = w.d_color;
  la.d_pred_feat = nullptr; la.counts = w.counts; la.status = a->status;
  objmisc::LossHoisted hz;
  hz.Hh = H; hz.hf = w.hf; hz.rayin = w.rayin; hz.gram = w.gram; hz.d_hf = w.d_hf; hz.rayfeat = w.rayfeat;
  rc = objmisc::step_batch_loss_impl(&la, feat ? &hz : nullptr, stream, w.loss_part);
  if (rc) return rc;
  // ---- backward
  // Weight-gradient GEMMs only READ the d-output / activation buffers and write the gradient arena, so they run on a
  // side stream beside the dgrad chain (each of these GEMMs alone leaves most of the chip idle).  Every d_h has its own
  // buffer: nothing a side-stream GEMM reads is overwritten before the join at the end.
  const bool fold_a = !feat && !small_rt;      // (layer_dgrad's fold_dhead form of the colour layer)
  hipLaunchKernelGGL(heads_bwd_kernel, eg, dim3(256), head_lds, st, H, n, w.hc, w.color, w.d_alpha, w.d_color, P, ps,
                     (int)off[OBJNERF_T_ALPHA_W], (int)off[OBJNERF_T_OC_W], w.dhead, c.d_hc, fold_a ? nullptr : c.d_h4, act16,
                     act16 == 2 ? grad_scale : 1.0f);
  // head weight grads: d wa = dhead[:,0]^T h4, d Woc = dhead[:,1:4]^T hc; biases = column sums of dhead
  // (every bias gradient rides on its layer's weight-gradient GEMM: row sums of the d-output operand tile)
  fork();
  if (H > 256) {
    wgrad(E, ss, {}, K, 1, H, n, op_cols(w.dhead, 4, n * 4), op_rows(w.h4, H, n * H, c.act16),
          op_rows(G + off[OBJNERF_T_ALPHA_W], H, ps), G + off[OBJNERF_T_ALPHA_B], grad_scale);
    wgrad(E, ss, {}, K, 3, H, n, op_cols(w.dhead + 1, 4, n * 4), op_rows(w.hc, H, n * H, c.act16),
          op_rows(G + off[OBJNERF_T_OC_W], H, ps), G + off[OBJNERF_T_OC_B], grad_scale);
  } else {
    // 64 samples per block (32 iterations of a 2-row pass at H = 128): the loop is a chain of load latencies, so the
    // reduction wants many short blocks (512 samples per block: 183 us for the background batch; now ~25 us)
    int hb = (int)((n + 63) / 64);
    const int cap = (2048 + K - 1) / K;
    if (hb > cap) hb = cap;
    // block partials + an ordered reduction (reduce_parts_kernel: "GEMMs" of M = 1 / 3 rows with hb slices)
    float* pA = E.parts_alloc((size_t)K * hb * H), *pW = E.parts_alloc((size_t)K * hb * 3 * H);
    float* rA = E.parts_alloc((size_t)K * hb), *rW = E.parts_alloc((size_t)K * hb * 3);
    if (!(pA && pW && rA && rW)) pA = pW = rA = rW = nullptr;        // no scratch: float atomics
    hipLaunchKernelGGL(head_wgrad_kernel, dim3((unsigned)hb, (unsigned)K), dim3(256), 0, ss, H, n, w.dhead, w.h4, w.hc, G, ps,
                       (int)off[OBJNERF_T_ALPHA_W], (int)off[OBJNERF_T_ALPHA_B], (int)off[OBJNERF_T_OC_W],
                       (int)off[OBJNERF_T_OC_B], pA, pW, rA, rW, act16);
    if (pA) {
      const RedItem heads[2] = {head_red_item(c, OBJNERF_T_ALPHA_W, OBJNERF_T_ALPHA_B, 1, pA, rA, hb),
                                head_red_item(c, OBJNERF_T_OC_W, OBJNERF_T_OC_B, 3, pW, rW, hb)};
      red_emit(ss, small_rt ? &step_red : nullptr, heads, 2);
    }
  }
  if (feat) {
    // d_hf (pre-activation gradient of the feature layer) came out of the loss kernel; the 512-d head's gradient from
    // the rays' moments (side stream)
    const int XC = H + 1;
    const long nr = (long)K * a->R;
    fork();
    hipLaunchKernelGGL(featg_scale_kernel, dim3((unsigned)((nr * XC + 255) / 256)), dim3(256), 0, ss, nr, H, w.rayfeat, w.X1,
                       w.X2);
    (void)hipMemsetAsync(w.Tm, 0, ((size_t)K * C * XC + (size_t)K * XC * XC) * 4, ss);
    feat_moments_enqueue(E, ss, {.fp32 = small_rt != 0}, fh, fhb);
    feat_finish_enqueue(ss, fh, fhb, G);
  }
  if (small_rt) {
    // small batch: the whole input-gradient chain in one launch, then the (independent) weight-gradient GEMMs
    // as one grouped launch on the side stream
    BwdSmall b;
    b.n = n; b.feat = feat ? 1 : 0; b.params = P; b.ps = ps;
    b.h1 = w.h1; b.h2 = w.h2; b.h3 = w.h3; b.h4 = w.h4; b.d_hc = c.d_hc; b.d_hf = feat ? w.d_hf : nullptr;
    b.d_h4 = c.d_h4; b.d_h3 = c.d_h3; b.d_h2 = c.d_h2; b.d_h1 = c.d_h1; b.d_emb = w.d_emb;
    set_weight_offsets(b, off);
    launch_small_rt(st, b, K, small_bf, small_rt);
    fork();
    GroupLaunch group(small_bf, 0, &step_red);      // bf16 mode: the weight gradients take bf16 operands like every other
                                                    // GEMM of the mode
    wgrad_chain(E, ss, {.group = &group}, c, feat, true);
    group_launch(ss, group);
  } else {
    backward_chain(E, st, ss, c, feat, fold_a ? w.dhead : nullptr, fork);
  }
  // embedding directions: block partials + ordered reduction straight into the gradient arena (float atomics into dBpe
  // and a copy when the scratch is exhausted)
  const int pg = pe_bwd_blocks(n);
  float* pe_part = E.parts_alloc((size_t)K * pg * 63);
  if (!pe_part) (void)hipMemsetAsync(w.dBpe, 0, (size_t)K * 64 * 4, st);
  hipLaunchKernelGGL(pe_bwd_kernel, dim3(pg, K), dim3(256), 0, st, n, P, ps, (int)off[OBJNERF_T_PE_B], a->scale, a->pts,
                     w.d_emb, w.dBpe, pe_part);
  if (pe_part) {
    const RedItem r = pe_red_item(c, pe_part, pg);
    red_emit(st, small_rt ? &step_red : nullptr, &r, 1);
  } else {
    hipLaunchKernelGGL(copy_cols_kernel, dim3((unsigned)((K * 63 + 255) / 256)), dim3(256), 0, st, (long)K, 63, w.dBpe, 63L,
                       G + off[OBJNERF_T_PE_B], ps);
  }
  if (multi) {   // join: the caller's stream continues after the weight gradients
    (void)hipEventRecord(sd.done_all, ss);
    (void)hipStreamWaitEvent(st, sd.done_all, 0);
  }
  launch_reductions(st, step_red);
  if (hipGetLastError() != hipSuccess) return OBJNERF_ELAUNCH;
  if (E.error) return OBJNERF_EINVAL;
  return OBJNERF_OK;
}

// ------------------------------------------------------------------------------------------------
// Inference (embedding.py:46-55 + model.py:61-103) for any hidden width: the forward half of train_step with
// ping-pong activation buffers.  workspace: emb [K][N][129] | A | B | C  ([K][N][H] each).
size_t eval_workspace_bytes(const objnerf_net* net, int K, long N) {
  return al((size_t)K * N * OBJ_EMB * 4) + 3 * al((size_t)K * N * net->hidden * 4) + 256;
}

int eval_points(const objnerf_net* net, int K, long N, const float* params, long p_stride, const float* scale,
                const float* pts, float* out_alpha, float* out_color, float* out_hfeat, float* out_clip,
                void* workspace, size_t workspace_bytes, void* stream, const float* emb_in) {
  const int H = net->hidden, C = net->feat_dim;
  if (H % 32 != 0 || net->n_freqs != 6) return OBJNERF_ENOTSUP;
  if (!workspace || workspace_bytes < eval_workspace_bytes(net, K, N) - 256) return OBJNERF_EINVAL;
  GemmStep E;                                  // fp32, no scratch
  int64_t off[OBJNERF_N_TENSORS + 1];
  objnerf_param_layout(net, off);
  hipStream_t st = (hipStream_t)stream;
  char* p = (char*)workspace;
  float* emb_ws = (float*)p; p += al((size_t)K * N * OBJ_EMB * 4);
  float* bA = (float*)p;  p += al((size_t)K * N * H * 4);
  float* bB = (float*)p;  p += al((size_t)K * N * H * 4);
  float* bC = (float*)p;
  const float* emb = emb_in;
  if (!emb_in) {
    int rc = objnerf_embed(net, K, N, params, p_stride, scale, pts, emb_ws, stream);
    if (rc) return rc;
    emb = emb_ws;
  }
  NetView c = {};                              // (fp32 storage)
  c.grad_scale = 1.0f;
  c.P = params; c.ps = p_stride; c.off = off; c.K = K; c.n = N; c.H = H; c.emb = emb;
  c.h1 = bA; c.h2 = bB; c.h3 = bA; c.h4 = bB; c.hc = bA;
  float* hf = (out_hfeat || out_clip) ? (out_hfeat ? out_hfeat : bC) : nullptr;
  forward_chain(E, st, c, out_alpha, out_color, hf, 0);
  if (out_clip)
    gemm(E, st, K, N, C, H, op_rows(hf, H, N * H), op_cols(params + off[OBJNERF_T_OF_W], H, p_stride),
         op_rows(out_clip, C, N * C), {.bias = params + off[OBJNERF_T_OF_B], .bsbias = p_stride});
  if (hipGetLastError() != hipSuccess) return OBJNERF_ELAUNCH;
  return OBJNERF_OK;
}

// ------------------------------------------------------------------------------------------------
// Backward of model.py:61-103 alone (objnerf_mlp_backward_ws): what loss.backward() runs through the stacked networks
// when a caller keeps the reference's loop body (train.py:424-436) instead of the fused step.  fp32.  The activations
// are recomputed from `emb` (the forward entry keeps none), then the same dgrad / weight-gradient GEMMs as train_step's
// layer-wise chain; with d_clip the 512-d head is differentiated directly (no hoisting: the loss is the caller's).
size_t mlp_backward_workspace_bytes(const objnerf_net* net, int K, long N, int with_clip) {
  WS w = carve(nullptr, net->hidden, net->feat_dim, N, 1, K, with_clip != 0);
  size_t extra = 0;
  if (with_clip) {
    const size_t M = (size_t)net->feat_dim, Hn = (size_t)net->hidden;
    extra = al(((size_t)K * wgrad_slices(K, (int)M, (int)Hn, N) * (M * Hn + M) + 256) * 4);
  }
  return w.bytes + extra + 256;
}

int mlp_backward(const objnerf_net* net, int K, long N, const float* params, long p_stride, const float* emb,
                 const float* d_alpha, const float* d_color, const float* d_clip, float* grads, float* d_emb,
                 void* workspace, size_t workspace_bytes, void* stream) {
  const int H = net->hidden, C = net->feat_dim;
  if (H % 32 != 0 || net->n_freqs != 6) return OBJNERF_ENOTSUP;
  const bool feat = d_clip != nullptr;
  const long n = N, ps = p_stride, nH = n * H;
  if (!workspace || workspace_bytes + 256 < mlp_backward_workspace_bytes(net, K, N, feat)) return OBJNERF_EINVAL;
  int64_t off[OBJNERF_N_TENSORS + 1];
  objnerf_param_layout(net, off);
  hipStream_t st = (hipStream_t)stream;
  WS w = carve((char*)workspace, H, C, n, 1, K, feat);
  GemmStep E;                         // fp32; no packed-B scratch
  E.parts = w.parts; E.parts_cap = w.parts_floats;
  const float* P = params;
  float* G = grads;
  NetView c = net_view(w, P, G, ps, off, K, n, H);
  c.emb = emb; c.d_emb = d_emb;
  for (int k = 0; k < K; ++k)      // feature-branch entries only when they receive a gradient ("no gradient" = untouched)
    (void)hipMemsetAsync(G + (long)k * ps, 0, (size_t)(feat ? off[T_FEAT_END] : off[T_TRAINED_END]) * 4, st);
  // ---- forward (recompute)
  forward_chain(E, st, c, w.alpha, w.color, w.hf, 0);
  // ---- backward
  hipLaunchKernelGGL(heads_bwd_kernel, dim3((unsigned)((n + 15) / 16), (unsigned)K), dim3(256), (size_t)4 * H * sizeof(float),
                     st, H, n, w.hc, w.color, d_alpha, d_color, P, ps, (int)off[OBJNERF_T_ALPHA_W], (int)off[OBJNERF_T_OC_W],
                     w.dhead, c.d_hc, c.d_h4, 0, 1.0f);
  wgrad(E, st, {}, K, 1, H, n, op_cols(w.dhead, 4, n * 4), op_rows(w.h4, H, nH), op_rows(G + off[OBJNERF_T_ALPHA_W], H, ps),
        G + off[OBJNERF_T_ALPHA_B]);
  wgrad(E, st, {}, K, 3, H, n, op_cols(w.dhead + 1, 4, n * 4), op_rows(w.hc, H, nH), op_rows(G + off[OBJNERF_T_OC_W], H, ps),
        G + off[OBJNERF_T_OC_B]);
  if (feat) {
    // 512-d head: d W_of = d_clip^T hf, d b_of = column sums, d_hf = (d_clip W_of) o [hf > 0]
    GemmStep Eh;                      // (its slabs have a region of their own behind the carve)
    Eh.parts = (float*)((char*)workspace + w.bytes);
    Eh.parts_cap = (size_t)K * wgrad_slices(K, C, H, n) * ((size_t)C * H + C) + 256;
    wgrad(Eh, st, {}, K, C, H, n, op_cols(d_clip, C, n * C), op_rows(w.hf, H, nH), op_rows(G + off[OBJNERF_T_OF_W], H, ps),
          G + off[OBJNERF_T_OF_B]);
    gemm(E, st, K, n, H, C, op_rows(d_clip, C, n * C), op_rows(P + off[OBJNERF_T_OF_W], H, ps), op_rows(w.d_hf, H, nH),
         {.mask = op_rows(w.hf, H, nH)});
  }
  backward_chain(E, st, st, c, feat, nullptr, [] {});
  if (hipGetLastError() != hipSuccess) return OBJNERF_ELAUNCH;
  return OBJNERF_OK;
}

// Backward of embedding.py:46-55 alone (objnerf_embed_bwd): d B [K][21][3] from d_emb [K][N][129]; scratch [K][64] floats
int embed_backward(const objnerf_net* net, int K, long N, const float* params, long p_stride, const float* scale,
                   const float* pts, const float* d_emb, float* d_B, float* scratch, void* stream) {
  if (net->n_freqs != 6) return OBJNERF_ENOTSUP;
  int64_t off[OBJNERF_N_TENSORS + 1];
  objnerf_param_layout(net, off);
  hipStream_t st = (hipStream_t)stream;
  const int pg = pe_bwd_blocks(N);
  (void)hipMemsetAsync(scratch, 0, (size_t)K * 64 * 4, st);
  hipLaunchKernelGGL(pe_bwd_kernel, dim3(pg, K), dim3(256), 0, st, N, params, p_stride, (int)off[OBJNERF_T_PE_B], scale, pts,
                     d_emb, scratch, (float*)nullptr);
  hipLaunchKernelGGL(copy_cols_kernel, dim3((unsigned)((K * 63 + 255) / 256)), dim3(256), 0, st, (long)K, 63, scratch, 63L, d_B,
                     63L);
  if (hipGetLastError() != hipSuccess) return OBJNERF_ELAUNCH;
  return OBJNERF_OK;
}

// ---- the hoisted 512-d feature head around a fused kernel of another width (objnerf_generic.h)
size_t feat_head_workspace_bytes(int K, int R, int Hh, int C) {
  const size_t XC = (size_t)Hh + 1;
  size_t fl = (size_t)K * ((size_t)Hh * Hh + Hh + 1) + (size_t)K * R * (Hh + 2) + (size_t)K * R * (Hh + 3) + 2 * (size_t)K * R * XC +
              (size_t)K * C * XC + (size_t)K * XC * XC;
  const size_t parts = wgrad_parts_floats(K, C, (int)XC, R) + wgrad_parts_floats(K, (int)XC, (int)XC, R) + 256;
  return (fl + parts) * 4 + 10 * 256;
}
FeatHead feat_head_carve(char* base, int K, int R, int Hh, int C) {
  FeatHead f;
  char* p = base;
  auto take = [&](size_t floats) { float* r = (float*)p; p += al(floats * 4); return r; };
  const size_t XC = (size_t)Hh + 1;
  f.gram = take((size_t)K * ((size_t)Hh * Hh + Hh + 1));
  f.rayin = take((size_t)K * R * (Hh + 2));
  f.rayfeat = take((size_t)K * R * (Hh + 3));
  f.X1 = take((size_t)K * R * XC);
  f.X2 = take((size_t)K * R * XC);
  f.Tm = take((size_t)K * C * XC);
  f.mom = take((size_t)K * XC * XC);
  f.parts_floats = wgrad_parts_floats(K, C, (int)XC, R) + wgrad_parts_floats(K, (int)XC, (int)XC, R) + 256;
  f.parts = take(f.parts_floats);
  return f;
}
int feat_head_prep(void* stream, const FeatHeadArgs& h, const FeatHead& f, int operands) {
  GemmStep E;
  E.operands = operands;
  feat_prep_enqueue(E, (hipStream_t)stream, h, f);
  if (E.error) return OBJNERF_EINVAL;
  return hipGetLastError() == hipSuccess ? OBJNERF_OK : OBJNERF_ELAUNCH;
}
int feat_head_grads(void* stream, const FeatHeadArgs& h, const FeatHead& f, float* grads, int operands) {
  GemmStep E;
  E.operands = operands;
  E.parts = f.parts; E.parts_cap = f.parts_floats;
  feat_moments_enqueue(E, (hipStream_t)stream, {.need_parts = true}, h, f);
  if (E.parts_failed || E.error) return OBJNERF_EINVAL;
  feat_finish_enqueue((hipStream_t)stream, h, f, grads);
  return hipGetLastError() == hipSuccess ? OBJNERF_OK : OBJNERF_ELAUNCH;
}

// G = W_of^T W_of, wb = W_of^T b_of, bb = b_of . b_of of K objects: gram[k][Hh * Hh | Hh | 1], batch stride gstride
void feat_gram(void* stream, const FeatHeadArgs& h, float* gram, long gstride) {
  GemmStep E;
  feat_gram_enqueue(E, (hipStream_t)stream, h, gram, gstride);
}
// out[k][m][:] = W_of[k] hfeat[k][m] + b_of[k] * weight[k][m]   (model.py:101 applied after compositing; weight NULL = 1)
void feature_head(void* stream, const FeatHeadArgs& h, long n, const float* hfeat, const float* weight, float* out) {
  GemmStep E;
  gemm(E, (hipStream_t)stream, h.K, (int)n, h.C, h.Hh, op_rows(hfeat, h.Hh, n * h.Hh), op_cols(h.P + h.off_w, h.Hh, h.ps),
       op_rows(out, h.C, n * h.C), {.bias = h.P + h.off_b, .bsbias = h.ps, .biasrow = weight, .bsbr = n});
}
void gemm_f32(void* stream, int batch, int M, int N, int Kd, const Operand& A, const Operand& B, const Operand& C,
              bool accumulate) {
  GemmStep E;
  gemm(E, (hipStream_t)stream, batch, M, N, Kd, A, B, C, {.accumulate = accumulate});
}
size_t wgrad_parts_floats(int batch, int M, int N, long n) {
  return (size_t)batch * wgrad_slices(batch, M, N, n) * M * N + 64;
}
void wgrad_f32(void* stream, int batch, int M, int N, long n, const Operand& A, const Operand& B, const Operand& C,
               float* parts, size_t parts_floats) {
  GemmStep E;
  E.parts = parts; E.parts_cap = parts ? parts_floats : 0;
  wgrad(E, (hipStream_t)stream, {}, batch, M, N, n, A, B, C);
}

}  // namespace objgen
