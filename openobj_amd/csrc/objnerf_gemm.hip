// The GEMM layer of the layer-wise path (objnerf_generic.hip) and of the hoisted feature head: batched fp32 MFMA GEMMs
// (v_mfma_f32_16x16x4_f32, 64 x 64 x 16 tiles), their 16-bit operand variants, the grouped launches, deterministic
// split-K (partial slabs + reduce_parts_kernel), and the host calls that choose and launch them (objnerf_gemm.h).
#include <algorithm>
#include "objnerf_device.h"
#include "objnerf_gemm.h"
#include "objnerf_step_tail.h"

namespace objgen {

#ifndef OBJ_GEMM_BK
#define OBJ_GEMM_BK 16
#endif
constexpr int BK = OBJ_GEMM_BK;
#ifndef OBJ_WGRAD_MINPER
#define OBJ_WGRAD_MINPER 256
#endif

// Workgroup tile (32*TM*2) x (32*TN*2): 4 waves as 2 x 2, each wave TM x TN MFMA tiles of 16 x 16.
// <1,1> = 64 x 64 (small problems), <2,2> = 128 x 128 (the n x H x H layer GEMMs: 2 MFMAs per LDS read).
template <int TM, int TN, int BKT = BK, int WM = 2, int WN = 2>
__device__ __forceinline__ void gemm_tile(const Gemm& g, const int bx, const int by, const int bz) {
  constexpr int BK = BKT;      // k depth of one LDS stage (shadows the default)
  constexpr int BM = 16 * TM * WM, BN = 16 * TN * WN;      // (per wave 16*TM x 16*TN, workgroup WM x WN waves)
  constexpr int NTH = 64 * WM * WN;
  __shared__ float As[BK][BM + 4];
  __shared__ float Bs[BK][BN + 4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane & 15, gg = lane >> 4;
  const int wm = w / WN, wn = w % WN;
  const int m0 = by * BM, n0 = bx * BN;
  const int sk = g.splitk > 1 ? g.splitk : 1;
  const long z = bz / sk;
  const int slice = bz % sk;
  const float* A = g.A + z * g.bsa;
  const float* B = g.B + z * g.bsb;
  float* C = g.C + z * g.bsc;
  const int kper = ((g.Kd + sk - 1) / sk + BK - 1) / BK * BK;
  const int kbeg = slice * kper, kend = min(g.Kd, kbeg + kper);
  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int NA = BM * BK / NTH, NB = BN * BK / NTH;
  float ra[NA], rb[NB];
  // a thread's elements of the two tiles: fixed (row, k-slot) per element, so each keeps a pointer that advances by one
  // k stage per load (the per-element stride products of every stage were ~12 VALU instructions per load -- 40 % on top
  // of the MFMA time of the 8-deep wide kernel, and VALU time adds to fp32 MFMA time here)
  const float* pa[NA]; const float* pb[NB];
  int ka[NA], kb[NB];          // the element's current k; < 0: row out of range
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int e = tid + NTH * i;
    int am, ak;
    if (g.sak == 1) { ak = e % BK; am = e / BK; } else { am = e % BM; ak = e / BM; }
    const int gm = m0 + am;
    pa[i] = A + (long)gm * g.sam + (long)(kbeg + ak) * g.sak;
    ka[i] = gm < g.M ? kbeg + ak : INT_MAX / 2;
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int e = tid + NTH * i;
    int bn, bk;
    if (g.sbk == 1) { bk = e % BK; bn = e / BK; } else { bn = e % BN; bk = e / BN; }
    const int gn = n0 + bn;
    pb[i] = B + (long)(kbeg + bk) * g.sbk + (long)gn * g.sbn;
    kb[i] = gn < g.N ? kbeg + bk : INT_MAX / 2;
  }
  const long stepa = (long)BK * g.sak, stepb = (long)BK * g.sbk;
  auto load_tiles = [&](int) {                 // (stages are requested in order: the argument is implied)
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      ra[i] = ka[i] < kend ? *pa[i] : 0.f;
      pa[i] += stepa; ka[i] += BK;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      rb[i] = kb[i] < kend ? *pb[i] : 0.f;
      pb[i] += stepb; kb[i] += BK;
    }
  };
  auto store_tiles = [&]() {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int e = tid + NTH * i;
      int am, ak;
      if (g.sak == 1) { ak = e % BK; am = e / BK; } else { am = e % BM; ak = e / BM; }
      As[ak][am] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int e = tid + NTH * i;
      int bn, bk;
      if (g.sbk == 1) { bk = e % BK; bn = e / BK; } else { bn = e % BN; bk = e / BN; }
      Bs[bk][bn] = rb[i];
    }
  };
  float rs = 0.f;
  const bool do_rs = g.rowsum != nullptr && bx == 0 && tid < BM;
  if (kbeg < kend) load_tiles(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    store_tiles();
    __syncthreads();
    if (k0 + BK < kend) load_tiles(k0 + BK);       // next tile's global loads fly under the MFMAs
    if (do_rs) {
#pragma unroll
      for (int kk = 0; kk < BK; ++kk) rs += As[kk][tid];
    }
#pragma unroll
    for (int ks = 0; ks < BK / 4; ++ks) {
      float a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = As[4 * ks + gg][16 * TM * wm + 16 * i + c];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = Bs[4 * ks + gg][16 * TN * wn + 16 * j + c];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  if (do_rs && m0 + tid < g.M) {
    if (g.rs_part) g.rs_part[(z * sk + slice) * g.M + m0 + tid] = rs;
    else atomicAdd(g.rowsum + z * g.bsrs + m0 + tid, rs);
  }
  // epilogue: D layout: col n = lane & 15, row m = 4 * (lane >> 4) + r.  Offsets are advanced incrementally (the 64-bit
  // stride products per element were ~15 VALU instructions each, and VALU time adds to fp32 MFMA time on this part).
  const int mb = m0 + 16 * TM * wm + 4 * gg, nb = n0 + 16 * TN * wn + c;
  long ci = (long)mb * g.scm + (long)nb * g.scn;                        // into C (this batch entry)
  long mi = z * g.bsm + (long)mb * g.smm + (long)nb * g.smn;            // into g.mask
  long ri = z * g.bsbr + (long)mb * g.sbr;                              // into g.biasrow
  const long c16m = 16 * g.scm, c16n = 16 * g.scn, m16m = 16 * g.smm, m16n = 16 * g.smn, r16 = 16 * (long)g.sbr;
#pragma unroll
  for (int i = 0; i < TM; ++i, ci += c16m, mi += m16m, ri += r16) {
    long cj = ci, mj = mi;
#pragma unroll
    for (int j = 0; j < TN; ++j, cj += c16n, mj += m16n) {
      const int n = nb + 16 * j;
      const float bn_ = (g.bias && n < g.N && sk <= 1) ? g.bias[z * g.bsbias + n] : 0.f;
      long co = cj, mo = mj, ro = ri;
#pragma unroll
      for (int r = 0; r < 4; ++r, co += g.scm, mo += g.smm, ro += g.sbr) {
        const int m = mb + 16 * i + r;
        if (m < g.M && n < g.N) {
          float v = acc[i][j][r];
          if (sk > 1) {
            if (g.part) g.part[((z * sk + slice) * g.M + m) * g.N + n] = v;
            else atomicAdd(C + co, v);
            continue;
          }
          if (g.accumulate) v += C[co];
          if (g.bias) v += bn_ * (g.biasrow ? g.biasrow[ro] : 1.0f);
          if (g.relu) v = fmaxf(v, 0.f);
          if (g.mask) v = g.mask[mo] > 0.f ? v : 0.f;
          C[co] = v;
        }
      }
    }
  }
}


template <int TM, int TN, int BKT = BK>
__global__ __launch_bounds__(256) void gemm_kernel(const Gemm g) {
  gemm_tile<TM, TN, BKT>(g, blockIdx.x, blockIdx.y, blockIdx.z);
}
// 128 x 128 tile on 8 waves (4 x 2 waves of 32 x 64)
#ifndef OBJ_GEMM_BK_WIDE
#define OBJ_GEMM_BK_WIDE 8      // measured on the hidden-256 layer GEMMs (configs[4] share): 8 -> 422 ms, 16 -> 452, 32 -> 457
#endif
#ifndef OBJ_GEMM_WIDE_TM
#define OBJ_GEMM_WIDE_TM 2      // row tiles per wave of the wide kernel: workgroup tile (64 TM) x 128
#endif
__global__ __launch_bounds__(512, 8) void gemm_kernel8(const Gemm g) {
  gemm_tile<OBJ_GEMM_WIDE_TM, 4, OBJ_GEMM_BK_WIDE, 4, 2>(g, blockIdx.x, blockIdx.y, blockIdx.z);
}

// 8 waves per workgroup on a 128 x 128 output tile (4 x 2 waves of 32 x 64): every operand slice is read once
// (64 x 64 tiles of 4 waves read it once per tile: 0.297 -> 0.287 ms for the background step)
__global__ __launch_bounds__(512) void gemm_group_kernel(const GemmGroup gr) {
  if ((int)blockIdx.z >= gr.zbeg[gr.count]) {            // (extra workgroups: FeatPrepTask)
    if (blockIdx.x == 0 && blockIdx.y == 0) feat_prep_task(gr.task, (int)blockIdx.z - gr.zbeg[gr.count]);
    return;
  }
  int i = 0;
  while (i + 1 < gr.count && (int)blockIdx.z >= gr.zbeg[i + 1]) ++i;
  const Gemm& g = gr.g[i];
  if ((int)blockIdx.x * 128 >= g.N || (int)blockIdx.y * 128 >= g.M) return;
  gemm_tile<2, 4, BK, 4, 2>(g, blockIdx.x, blockIdx.y, blockIdx.z - gr.zbeg[i]);
}

// ------------------------------------------------------------------------------------------------
// bf16-operand variant (OBJNERF_TRAIN_BF16 on the layer-wise path): same interface and epilogue, operands are
// rounded to bf16 when they are staged in LDS ([row][k], k contiguous: one ds_read_b128 per MFMA operand),
// v_mfma_f32_16x16x32_bf16, fp32 accumulation.  64 x 64 (or, for wide layers, 128 x 128) tiles, 32-deep k steps:
// 4 (16) MFMAs per wave and step, so the kernel is bound by the operand traffic, not by the matrix core.
//
// OT = _Float16 is the OBJNERF_TRAIN_FP16 mode (v_mfma_f32_16x16x32_f16): 11 significant bits instead of 8, but a
// narrow exponent -- operands are clamped to +-65504 when rounded, and the backward GEMMs scale their gradient
// operand (Gemm::a_scale).
#ifndef OBJ_G16_BK
#define OBJ_G16_BK 32
#endif
#ifndef OBJ_G16_BK_WIDE
#define OBJ_G16_BK_WIDE 32
#endif
// BKB: k-stage depth (OBJ_G16_BK / OBJ_G16_BK_WIDE).  Measured on MI355X (tools/gemm16_ab.sh): deeper stages LOSE --
// background step in bf16 mode 0.92 ms at 32, 1.19 ms at 64, 2.2 ms at 128; configs[4] share in fp16 2.18 / 2.37 /
// 2.60 s -- the prefetch registers and the larger LDS tiles cost more occupancy than the saved barriers return.  (Again
// with both weight-gradient operands 16-bit pass-through, 8 registers per stage: share per 8 objects 83 ms at 32,
// 104 at 64, 85 at 128.)
// WM x WN waves per workgroup, TM x TN MFMA tiles per wave.  The 128 x 128 tile runs on 8 waves (4 x 2, 32 x 64 per wave:
// 32 accumulator and 16 staging registers): as 4 waves of 64 x 64 it needed 197 registers, ONE wave per SIMD, and ran
// the hidden-256 layer GEMMs at 28 TFLOP/s -- slower than the fp32 kernel.
//
// AKM / BKM: the operand's ROWS (m / n) are the contiguous dimension in memory (weight gradients: A = d_out^T, B =
// activations; input gradients: B = W as stored).  Such a tile is staged K-MAJOR -- four consecutive rows per thread,
// one 8-byte LDS store, coalesced -- and the MFMA operand (8 consecutive k of one row) is gathered by two
// ds_read_b64_tr_b16 (gfx950's transposing LDS read: a 16-lane group reads a 4 k x 16 rows block column-wise;
// tools/ubench_tr.hip checks the lane map).  Before, those tiles went to the [row][k] image as 2-byte stores with a
// 4-way bank conflict and the hidden-256 weight gradients ran at 18 TFLOP/s.
// The read is the compiler's builtin (__builtin_amdgcn_ds_read_tr16_b64_*): it knows the instruction returns through
// LGKM, so it places the s_waitcnt itself and a batch of reads stays in flight together.  (Rounds 2-3 issued it as bare
// inline asm with a hand-written wait tied to the destination registers: correct only as long as the register
// allocator never copied a destination before that wait.)
// (the 8-wave tile is held to 128 registers -- two workgroups per CU: at 130 the fp16 forward variant lost one)
//
// AFULL (layer GEMMs over the sample axis: M = 10^6 rows, contraction <= 256, A rows k-contiguous): the workgroup's A
// panel -- BM rows x the WHOLE contraction -- is fetched with one burst of loads before the k-loop (64 KB in flight
// per workgroup) and stays in LDS.  B -- the layer's weights -- is NOT staged by the workgroup at all: pack_b_kernel
// rounds it ONCE per GEMM into a 16-bit image laid out as MFMA operands ([k / 32][n / 16][lane][8], 128 KB for 256 x
// 256, L2-resident) and every lane fetches its operand with one 16-byte load.  No barrier and no conversion in the
// k-loop.  (The plain kernel re-read and re-rounded the fp32 weights in every workgroup: rocprof counted 36 VALU
// instructions per MFMA on the hidden-256 layer GEMMs, which ran at ~2 TB/s of HBM traffic with the matrix core 90 %
// idle.)  With BN = 256 the panel is read exactly once.  The epilogue's LDS patch aliases the panel.
// (the body takes its block coordinates as arguments: gemm_group16_kernel below runs it for several GEMMs per launch)
template <int TM, int TN, typename OT, int BKB, int WM = 2, int WN = 2, bool AKM = false, bool BKM = false,
          bool AFULL = false, int KMAX = 256>
__device__ __forceinline__ void gemm_bf16_body(const Gemm& g, const int bx, const int by, const int bz) {
  constexpr int BM = 16 * TM * WM, BN = 16 * TN * WN, LDK = BKB + 8, NTH = 64 * WM * WN;
  constexpr int PA = BM + 8, PB = BN + 8;                 // k-major row pitches (elements; 8-byte aligned rows)
  constexpr int LDA = AFULL ? KMAX + 8 : LDK;   // AFULL: panel row pitch (conflict-free b128 reads: 132 / 180 dwords)
  static_assert(!(AFULL && AKM), "the resident panel is row-major");
  typedef typename Op16<OT>::V OV;
  constexpr int EC_ = 16 * TN, EP_ = EC_ + 4;
  constexpr size_t a_bytes = sizeof(OT) * (AFULL ? BM * LDA : (AKM ? BKB * PA : BM * LDK));
  constexpr size_t ep_bytes = sizeof(float) * WM * WN * 16 * EP_;
  __shared__ __attribute__((aligned(16))) char a_raw[AFULL ? (a_bytes > ep_bytes ? a_bytes : ep_bytes) : a_bytes];
  OT* const Asm = reinterpret_cast<OT*>(a_raw);
  __shared__ __attribute__((aligned(16))) OT Bsm[AFULL ? 8 : (BKM ? BKB * PB : BN * LDK)];
  const float a_scale = g.a_scale, inv_scale = 1.0f / g.a_scale;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane & 15, gg = lane >> 4;
  const int wm = w / WN, wn = w % WN;
  const int m0 = by * BM, n0 = bx * BN;
  const int sk = g.splitk > 1 ? g.splitk : 1;
  const long z = bz / sk;
  const int slice = bz % sk;
  const float* A = g.A + z * g.bsa;
  const float* B = g.B + z * g.bsb;
  const int kper = ((g.Kd + sk - 1) / sk + BKB - 1) / BKB * BKB;
  const int kbeg = slice * kper, kend = min(g.Kd, kbeg + kper);
  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int NA = AFULL ? 0 : BM * BKB / NTH, NB = AFULL ? 0 : BN * BKB / NTH;
  float ra[NA ? NA : 1], rb[NB ? NB : 1];
  if constexpr (AFULL) {
    // the panel: columns [0, ka) from A (lanes along k; 16-byte loads when g.vec4: rows 16-byte aligned, ka a multiple
    // of 8), then, for the 352-deep variant, columns [256, 352) from the second source (x1 / x2 inside the 129-float
    // embedding rows: scalars).  Everything else of the panel is zero.
    constexpr int KA = 256;
    const int ka = min(g.k2, g.Kd);                     // columns [0, ka) from A, [ka, Kd) from A2 (then ka == KA)
    if (g.a16) {
      constexpr int N8 = BM * KA / 8 / NTH;
      const OT* A16 = reinterpret_cast<const OT*>(g.A) + z * g.bsa;
      uint4 pv[N8];
#pragma unroll
      for (int i = 0; i < N8; ++i) {
        const int q = tid + NTH * i, am = q / (KA / 8), ak = 8 * (q % (KA / 8));
        const int gm = m0 + am;
        pv[i] = (gm < g.M && ak < ka) ? *reinterpret_cast<const uint4*>(A16 + gm * g.sam + ak) : uint4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int i = 0; i < N8; ++i) {
        const int q = tid + NTH * i, am = q / (KA / 8), ak = 8 * (q % (KA / 8));
        *reinterpret_cast<uint4*>(&Asm[am * LDA + ak]) = pv[i];
      }
    } else if (g.vec4) {
      constexpr int NV = BM * KA / 4 / NTH;
      f32x4 pv[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int q = tid + NTH * i, am = q / (KA / 4), ak = 4 * (q % (KA / 4));
        const int gm = m0 + am;
        pv[i] = (gm < g.M && ak < ka) ? *reinterpret_cast<const f32x4*>(A + gm * g.sam + ak) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int q = tid + NTH * i, am = q / (KA / 4), ak = 4 * (q % (KA / 4));
        typedef OT ot4 __attribute__((ext_vector_type(4)));
        ot4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = Op16<OT>::cvt(a_scale != 1.0f ? pv[i][j] * a_scale : pv[i][j]);
        *reinterpret_cast<ot4*>(&Asm[am * LDA + ak]) = v;
      }
    } else {
      constexpr int NS = BM * KA / NTH / 2;
#pragma unroll
      for (int h = 0; h < 2; ++h) {          // two bursts of scalar loads
        float ps[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          const int e = tid + NTH * (NS * h + i), am = e / KA, ak = e % KA;
          const int gm = m0 + am;
          ps[i] = (gm < g.M && ak < ka) ? A[gm * g.sam + ak] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          const int e = tid + NTH * (NS * h + i), am = e / KA, ak = e % KA;
          Asm[am * LDA + ak] = Op16<OT>::cvt(ps[i] * a_scale);
        }
      }
    }
    if constexpr (KMAX > KA) {
      constexpr int K2 = KMAX - KA, N2 = BM * K2 / NTH;
      static_assert(BM * K2 % NTH == 0, "second-source share");
      const float* A2 = g.A2 + z * g.bsa2;
      float ps[N2];
#pragma unroll
      for (int i = 0; i < N2; ++i) {
        const int e = tid + NTH * i, am = e / K2, ak = KA + e % K2;
        const int gm = m0 + am;
        ps[i] = (gm < g.M && ak >= ka && ak < g.Kd) ? A2[gm * g.sam2 + (ak - ka)] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < N2; ++i) {
        const int e = tid + NTH * i, am = e / K2, ak = KA + e % K2;
        Asm[am * LDA + ak] = Op16<OT>::cvt(ps[i] * a_scale);
      }
    }
  }
  // element e of a thread's share -> (row, k): lanes along the operand's contiguous dimension
  auto load_tiles = [&](int k0) {
    if (AKM && g.a16) {
      // A is a 16-bit gradient array (stored already scaled by a_scale): four consecutive m per lane, one 8-byte load,
      // passed through to the k-major image (host-checked alignment)
      const OT* A16 = reinterpret_cast<const OT*>(g.A) + z * g.bsa;
#pragma unroll
      for (int i = 0; i < NA / 4; ++i) {
        const int q = tid + NTH * i, am = 4 * (q % (BM / 4)), ak = q / (BM / 4);
        const int gm = m0 + am, gk = k0 + ak;
        const uint2 u = (gm < g.M && gk < kend) ? *reinterpret_cast<const uint2*>(A16 + gk * g.sak + gm) : uint2{0u, 0u};
        ra[2 * i] = __builtin_bit_cast(float, u.x); ra[2 * i + 1] = __builtin_bit_cast(float, u.y);
      }
    } else if (AKM && g.vec4) {
      // rows contiguous and 16-byte aligned (weight gradients: A = d_out^T): four consecutive m per lane, one dwordx4
#pragma unroll
      for (int i = 0; i < NA / 4; ++i) {
        const int q = tid + NTH * i, am = 4 * (q % (BM / 4)), ak = q / (BM / 4);
        const int gm = m0 + am, gk = k0 + ak;
        const f32x4 v = (gm < g.M && gk < kend) ? *reinterpret_cast<const f32x4*>(A + gk * g.sak + gm) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) ra[4 * i + j] = v[j];
      }
    } else
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      int am, ak;
      if (AKM) { const int e = tid + NTH * i; am = e % BM; ak = e / BM; }
      else { const int e = tid + NTH * i; ak = e % BKB; am = e / BKB; }
      const int gm = m0 + am, gk = k0 + ak;
      ra[i] = (gm < g.M && gk < kend) ? A[gm * g.sam + gk * g.sak] : 0.f;
    }
    if (BKM && g.b16) {
      // B is a 16-bit activation array (weight gradients in the 16-bit modes): four consecutive n per lane, one 8-byte
      // load, passed through to the k-major image unchanged (host-checked: sbn == 1, sbk and N multiples of 4)
      const OT* B16 = reinterpret_cast<const OT*>(g.B) + z * g.bsb;
#pragma unroll
      for (int i = 0; i < NB / 4; ++i) {
        const int q = tid + NTH * i, bn = 4 * (q % (BN / 4)), bk = q / (BN / 4);
        const int gn = n0 + bn, gk2 = k0 + bk;
        const uint2 u = (gn < g.N && gk2 < kend) ? *reinterpret_cast<const uint2*>(B16 + gk2 * g.sbk + gn) : uint2{0u, 0u};
        rb[2 * i] = __builtin_bit_cast(float, u.x); rb[2 * i + 1] = __builtin_bit_cast(float, u.y);
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      int bn, bk;
      if (BKM) { const int e = tid + NTH * i; bn = e % BN; bk = e / BN; }
      else { const int e = tid + NTH * i; bk = e % BKB; bn = e / BKB; }
      const int gn = n0 + bn, gk2 = k0 + bk;
      rb[i] = (gn < g.N && gk2 < kend) ? B[gk2 * g.sbk + gn * g.sbn] : 0.f;
    }
  };
  auto store_tiles = [&]() {
    if (AFULL) {
    } else if (AKM && g.a16) {
#pragma unroll
      for (int i = 0; i < NA / 4; ++i) {
        const int q = tid + NTH * i;
        *reinterpret_cast<uint2*>(&Asm[(q / (BM / 4)) * PA + 4 * (q % (BM / 4))]) =
            uint2{__builtin_bit_cast(uint32_t, ra[2 * i]), __builtin_bit_cast(uint32_t, ra[2 * i + 1])};
      }
    } else if (AKM && g.vec4) {
#pragma unroll
      for (int i = 0; i < NA / 4; ++i) {
        const int q = tid + NTH * i;
        typedef OT ot4 __attribute__((ext_vector_type(4)));
        ot4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = Op16<OT>::cvt(ra[4 * i + j] * a_scale);
        *reinterpret_cast<ot4*>(&Asm[(q / (BM / 4)) * PA + 4 * (q % (BM / 4))]) = v;
      }
    } else if (AKM) {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int e = tid + NTH * i;
        Asm[(e / BM) * PA + e % BM] = Op16<OT>::cvt(ra[i] * a_scale);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int e = tid + NTH * i;
        Asm[(e / BKB) * LDK + e % BKB] = Op16<OT>::cvt(ra[i] * a_scale);
      }
    }
    if (BKM && g.b16) {
#pragma unroll
      for (int i = 0; i < NB / 4; ++i) {
        const int q = tid + NTH * i;
        *reinterpret_cast<uint2*>(&Bsm[(q / (BN / 4)) * PB + 4 * (q % (BN / 4))]) =
            uint2{__builtin_bit_cast(uint32_t, rb[2 * i]), __builtin_bit_cast(uint32_t, rb[2 * i + 1])};
      }
    } else if (BKM) {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int e = tid + NTH * i;
        Bsm[(e / BN) * PB + e % BN] = Op16<OT>::cvt(rb[i]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int e = tid + NTH * i;
        Bsm[(e / BKB) * LDK + e % BKB] = Op16<OT>::cvt(rb[i]);
      }
    }
  };
  // MFMA operands of the wave's T row tiles (first tile-local row row0), k-slots ks + 8 gg .. + 7
  auto operands_km = [&](auto& out, const OT* img, const int pitch, const int row0, const int ks) {
    constexpr int T = sizeof(out) / sizeof(out[0]);
    uint2 lo[T], hi[T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
      const OT* p = img + (ks + 8 * gg + (c >> 2)) * pitch + row0 + 16 * i + 4 * (c & 3);
      lo[i] = lds_tr16(p);
      hi[i] = lds_tr16(p + 4 * pitch);
    }
#pragma unroll
    for (int i = 0; i < T; ++i) out[i] = __builtin_bit_cast(OV, uint4{lo[i].x, lo[i].y, hi[i].x, hi[i].y});
  };
  auto operands_rm = [&](auto& out, const OT* img, const int pitch, const int row0, const int ks) {
    constexpr int T = sizeof(out) / sizeof(out[0]);
#pragma unroll
    for (int i = 0; i < T; ++i) out[i] = *reinterpret_cast<const OV*>(img + (row0 + 16 * i + c) * pitch + ks + 8 * gg);
  };
  float rs = 0.f;
  const bool do_rs = !AFULL && g.rowsum != nullptr && bx == 0 && tid < BM;
  if constexpr (AFULL) {
    __syncthreads();                     // the panel is complete
    const int nks = (g.Kd + 31) / 32;
    const uint4* bp = reinterpret_cast<const uint4*>(g.Bp) + ((z * (KMAX / 32)) * (BN / 16) + TN * wn) * 64 + lane;
    for (int ks = 0; ks < nks; ++ks) {     // (no operand prefetch: 64 registers -> four workgroups per CU hide the round trip)
      OV bcur[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) bcur[j] = __builtin_bit_cast(OV, bp[(ks * (BN / 16) + j) * 64]);
      OV a[TM];
      operands_rm(a, Asm, LDA, 16 * TM * wm, 32 * ks);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = Op16<OT>::mfma(a[i], bcur[j], acc[i][j]);
    }
    __syncthreads();                     // every wave is done with the panel: the epilogue patch may overwrite it
  }
  if (!AFULL && kbeg < kend) load_tiles(kbeg);
  for (int k0 = kbeg; !AFULL && k0 < kend; k0 += BKB) {
    store_tiles();
    __syncthreads();
    if (k0 + BKB < kend) load_tiles(k0 + BKB);
    if (do_rs) {
#pragma unroll
      for (int kk = 0; kk < BKB; ++kk) rs += (float)(AKM ? Asm[kk * PA + tid] : Asm[tid * LDK + kk]);
    }
#pragma unroll
    for (int ks = 0; ks < BKB; ks += 32) {
      OV a[TM], b[TN];
      if (AKM) operands_km(a, Asm, PA, 16 * TM * wm, ks); else operands_rm(a, Asm, LDA, 16 * TM * wm, ks);
      if (BKM) operands_km(b, Bsm, PB, 16 * TN * wn, ks); else operands_rm(b, Bsm, LDK, 16 * TN * wn, ks);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = Op16<OT>::mfma(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
  if (do_rs && m0 + tid < g.M) {
    if (g.rs_part) g.rs_part[(z * sk + slice) * g.M + m0 + tid] = rs * inv_scale;
    else atomicAdd(g.rowsum + z * g.bsrs + m0 + tid, rs * inv_scale);
  }
  // Epilogue through LDS: the accumulator layout gives a lane ONE column of four rows, i.e. 64-byte runs per output row
  // (and the same for the mask / accumulate reads) -- each wave turns a 16-row strip of its tile around in its own LDS
  // patch so that the lanes run ALONG a row: 256-byte (128-byte for the 64-wide tile) coalesced rows for every global
  // access of the epilogue.
  constexpr int EC = 16 * TN, EP = EC + 4, RPI = 64 / EC;            // strip columns, pitch, rows per pass
  __shared__ float Ep_own[AFULL ? 1 : WM * WN][AFULL ? 1 : 16][AFULL ? 1 : EP];
  float (*const Ep)[16][EP] = AFULL ? reinterpret_cast<float (*)[16][EP]>(a_raw) : reinterpret_cast<float (*)[16][EP]>(Ep_own);
  const int ecol = lane % EC, erow0 = lane / EC;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) Ep[w][4 * gg + r][16 * j + c] = acc[i][j][r] * inv_scale;
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int n = n0 + EC * wn + ecol;
    // (element offsets of the strip's first row, advanced by one row pass each: the per-row 64-bit products of the
    // generic strides were most of this kernel's VALU work -- 15 instructions per MFMA on the hidden-256 layer GEMMs)
    const int mfirst = m0 + 16 * TM * wm + 16 * i + erow0;
    long coff = z * g.bsc + (long)mfirst * g.scm + (long)n * g.scn;             // into g.C (float or 16-bit elements)
    long moff = z * g.bsm + (long)mfirst * g.smm + (long)n * g.smn;             // into g.mask
    long roff = z * g.bsbr + (long)mfirst * g.sbr;                              // into g.biasrow
    const long cstep = (long)RPI * g.scm, mstep = (long)RPI * g.smm, rstep = (long)RPI * g.sbr;
    const float bn_ = (g.bias && n < g.N) ? g.bias[z * g.bsbias + n] : 0.f;
#pragma unroll
    for (int rr = 0; rr < 16; rr += RPI, coff += cstep, moff += mstep, roff += rstep) {
      const int m = mfirst + rr;
      float v = Ep[w][rr + erow0][ecol];
      if (m < g.M && n < g.N) {
        if (sk > 1) {
          if (g.part) g.part[((z * sk + slice) * g.M + m) * g.N + n] = v;
          else atomicAdd(g.C + coff, v);
          continue;
        }
        if (g.accumulate) v += g.c16 ? (float)reinterpret_cast<const OT*>(g.C)[coff] * inv_scale : g.C[coff];
        if (g.bias) v += bn_ * (g.biasrow ? g.biasrow[roff] : 1.0f);
        if (g.relu) v = fmaxf(v, 0.f);
        if (g.mask) {
          const bool on = g.m16 ? (float)reinterpret_cast<const OT*>(g.mask)[moff] > 0.f : g.mask[moff] > 0.f;
          v = on ? v : 0.f;
        }
        // (16-bit outputs are stored as the NEXT GEMM's operand: gradients already scaled by a_scale -- 1 in the forward)
        if (g.c16) reinterpret_cast<OT*>(g.C)[coff] = Op16<OT>::cvt(v * a_scale);
        else g.C[coff] = v;
      }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
  }
}

template <int TM, int TN, typename OT, int BKB, int WM = 2, int WN = 2, bool AKM = false, bool BKM = false,
          bool AFULL = false, int KMAX = 256>
__global__ __launch_bounds__(64 * WM * WN, (WM * WN >= 8) ? ((AFULL && KMAX == 256) ? 8 : 4) : 1) void gemm_bf16_kernel(const Gemm g) {
  // Workgroups are handed to the 8 XCDs round-robin in launch order (x fastest), so the column tiles of one row
  // block -- which read the same A rows -- would land on different L2s.  Re-map: consecutive workgroups OF ONE XCD
  // take the column tiles of one row block (rows beyond the last multiple of 8 row blocks keep the plain order).
  // Split-K weight gradients (few output tiles, hundreds of slices): the tiles of ONE slice read the same operand slabs,
  // so they go to one XCD the same way.
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (gridDim.x > 1 && gridDim.y >= 8) {
    const unsigned gx = gridDim.x, L = blockIdx.x + gx * blockIdx.y, full = (gridDim.y / 8) * 8 * gx;
    if (L < full) {
      const unsigned xcd = L % 8, s = L / 8;
      bx = (int)(s % gx);
      by = (int)((s / gx) * 8 + xcd);
    }
  } else if (gridDim.x * gridDim.y > 1 && gridDim.z >= 8) {
    const unsigned gx = gridDim.x, T = gx * gridDim.y, L = blockIdx.x + gx * blockIdx.y + T * blockIdx.z;
    const unsigned full = (gridDim.z / 8) * 8 * T;
    if (L < full) {
      const unsigned xcd = L % 8, s = L / 8, tile = s % T;
      bx = (int)(tile % gx);
      by = (int)(tile / gx);
      bz = (int)((s / T) * 8 + xcd);
    }
  }
  gemm_bf16_body<TM, TN, OT, BKB, WM, WN, AKM, BKM, AFULL, KMAX>(g, bx, by, bz);
}

// The weight-gradient GEMMs of a small-batch step in bf16 mode, in ONE launch (the fp32 twin: gemm_group_kernel): 128 x 128
// tiles on 8 waves (every operand slice read once), both operands k-major (d_out^T and the activations as they lie in
// memory), split-K partial tiles.
__global__ __launch_bounds__(512) void gemm_group16_kernel(const GemmGroup gr) {
  if ((int)blockIdx.z >= gr.zbeg[gr.count]) return;      // (tasks ride on the fp32 grouped launch only)
  int i = 0;
  while (i + 1 < gr.count && (int)blockIdx.z >= gr.zbeg[i + 1]) ++i;
  const Gemm& g = gr.g[i];
  if ((int)blockIdx.x * 128 >= g.N || (int)blockIdx.y * 128 >= g.M) return;
  gemm_bf16_body<2, 4, __bf16, OBJ_G16_BK_WIDE, 4, 2, true, true>(g, blockIdx.x, blockIdx.y, blockIdx.z - gr.zbeg[i]);
}

// B (generic strides, fp32) -> the AFULL kernel's operand image: thread (ks, jt, lane) writes the 8 values
// B[32 ks + 8 (lane >> 4) + e][16 jt + (lane & 15)], e = 0..7, rounded to OT; zero beyond Kd / N.
template <typename OT, int KS>
__global__ __launch_bounds__(256) void pack_b_kernel(const Gemm g, OT* __restrict__ out) {
  typedef typename Op16<OT>::V OV;
  const int t = blockIdx.x * 256 + threadIdx.x;              // (ks, jt, lane), KS * 16 * 64 per batch entry
  const int lane = t & 63, jt = (t >> 6) & 15, ks = t >> 10;
  const long z = blockIdx.y;
  const float* B = g.B + z * g.bsb;
  const int n = 16 * jt + (lane & 15);
  OV v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = 32 * ks + 8 * (lane >> 4) + e;
    v[e] = Op16<OT>::cvt((k < g.Kd && n < g.N) ? B[k * g.sbk + n * g.sbn] : 0.f);
  }
  reinterpret_cast<OV*>(out)[z * (KS * 1024) + t] = v;
}

// ---- deterministic split-K: partial-tile slabs + an ordered reduction (instead of float atomics)
#ifndef OBJ_WGRAD_TARGET
#define OBJ_WGRAD_TARGET 512         // 64 x 64 output tiles x slices a weight-gradient GEMM should at least have
#endif
#ifndef OBJ_WGRAD_MAXSLICES
#define OBJ_WGRAD_MAXSLICES 128      // (32 was measured: the background step in bf16 mode 0.92 -> 1.4 ms, too few workgroups)
#endif
// split-K slices of a weight-gradient GEMM over n samples: 512 samples per slice; 256 when that would leave most of the
// chip idle (the background network at the reference's native batch of 16 800 samples: step 0.55 -> 0.46 ms)
int wgrad_slices(int batch, int M, int N, long n) {
  const long tiles = (long)batch * ((M + 63) / 64) * ((N + 63) / 64);
  long per = 512;
  while (per > OBJ_WGRAD_MINPER && tiles * ((n + per - 1) / per) < OBJ_WGRAD_TARGET) per >>= 1;
  int sk = (int)((n + per - 1) / per);
  if (sk < 2) sk = 2;
  if (sk > 256) sk = 256;
  if (sk > OBJ_WGRAD_MAXSLICES) sk = OBJ_WGRAD_MAXSLICES;
  return sk;
}
// one thread per output (m, n) of a batch entry (+ one per row sum): adds the sk slices in slice order
__global__ __launch_bounds__(256) void reduce_parts_kernel(const RedGroup gr) {
  // a block = 64 consecutive outputs x 4 waves; wave w adds slices [w sk / 4, (w + 1) sk / 4) of its outputs in order
  // (coalesced: lanes along the outputs; 16 loads in flight), the four quarter sums meet in LDS and are added in wave
  // order -- a fixed association, so the result is bit-reproducible
  __shared__ float quarter[4][64];
  __shared__ float s_step_size[3], s_bc2_sqrt[3];
  __shared__ int s_active[3];
  const RedTail& tl = gr.tail;
  const bool tail_block = (int)blockIdx.x == gr.beg[gr.count];      // (only launched when the tail is set)
  if (tl.params && threadIdx.x < 3) {
    const int g = threadIdx.x;
    adamw_group_begin(g, tl.flags[0] != 0, tl.flags[1] != 0, tl.steps, tl.bank, tl.lr, tl.b1, tl.b2, tail_block,
                      s_active[g], s_step_size[g], s_bc2_sqrt[g]);
  }
  if (tail_block) {
    // the objects' loss terms from the workgroups' partial sums, in workgroup order, and their status bits
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    int bad = 0;
    // a wave per (object, term): lane l adds partials l, l + 64, .. in order, then the lanes meet in a fixed butterfly --
    // one association for every run (bit-reproducible), 64 loads in flight instead of a chain of `loss_blocks` latencies
    // (1200 workgroups at the benchmark shape: 120 us as one thread per term)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int e = wv; e < 4 * tl.K; e += 4) {
      const float* p = tl.loss_part + (long)(e >> 2) * tl.loss_blocks * 4 + (e & 3);
      float v = 0.f;
      for (int b = lane; b < tl.loss_blocks; b += 64) v += p[4 * b];
      for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
      if (lane == 0) {
        tl.loss_terms[e] = v;
        bad |= loss_status_bits(v);
      }
    }
    if (bad) atomicOr(&s_bad, bad);
    __syncthreads();
    if (threadIdx.x == 0 && tl.status) *tl.status = s_bad;
    return;
  }
  int i = 0;
  while (i + 1 < gr.count && (int)blockIdx.x >= gr.beg[i + 1]) ++i;
  const RedItem& r = gr.it[i];
  const long per = (long)r.M * r.N, nrs = r.rs_part ? r.M : 0;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long e = ((long)blockIdx.x - gr.beg[i]) * 64 + lane;
  const bool live = e < (long)r.batch * (per + nrs);
  const long z = live ? e / (per + nrs) : 0, q = live ? e - z * (per + nrs) : 0;
  const bool is_c = q < per;
  const float* p = is_c ? r.part + z * r.sk * per + q : r.rs_part + z * r.sk * r.M + (q - per);
  const long stride = is_c ? per : r.M;
  const int s0 = (int)((long)r.sk * w / 4), s1 = (int)((long)r.sk * (w + 1) / 4);
  float v = 0.f;
  if (live) {
    int s = s0;
    for (; s + 16 <= s1; s += 16) {
      float t[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) t[j] = p[(s + j) * stride];
#pragma unroll
      for (int j = 0; j < 16; ++j) v += t[j];
    }
    for (; s < s1; ++s) v += p[s * stride];
  }
  quarter[w][lane] = v;
  __syncthreads();
  if (w == 0 && live) {
    const float sum = ((quarter[0][lane] + quarter[1][lane]) + quarter[2][lane]) + quarter[3][lane];
    float* dst;
    if (is_c) {
      const long m = q / r.N, n = q - m * r.N;
      dst = r.C + z * r.bsc + m * r.scm + n;
    } else {
      dst = r.rowsum + z * r.bsrs + (q - per);
    }
    *dst = sum;
    const long idx = dst - tl.grads;                         // position in the gradient arena = in params / moments
    if (tl.params && idx >= 0 && idx < tl.arena_floats) {    // (the 512-d head's moment sums go to the workspace)
      const int g = adamw_group_of(idx % tl.p_stride, tl.lo1, tl.lo2, tl.hi2);
      if (s_active[g]) {
        float decay, w1, beta2, w2;
        adamw_coeffs(tl.lr, tl.b1, tl.b2, tl.wd, decay, w1, beta2, w2);
        adamw_update(tl.params, tl.m, tl.v, idx, sum, decay, w1, beta2, w2, s_step_size[g], s_bc2_sqrt[g], tl.eps);
      }
    }
  }
}
static int red_blocks(const RedItem& r) {
  return (int)(((long)r.batch * ((long)r.M * r.N + (r.rs_part ? r.M : 0)) + 63) / 64);
}
static void red_append(RedGroup& rg, const RedItem& r) {
  if (rg.count == 0) rg.beg[0] = 0;
  rg.it[rg.count] = r;
  rg.beg[rg.count + 1] = rg.beg[rg.count] + red_blocks(r);
  ++rg.count;
}
void launch_reductions(hipStream_t st, RedGroup& rg) {
  const int tail = rg.tail.loss_part ? 1 : 0;
  if (rg.count) hipLaunchKernelGGL(reduce_parts_kernel, dim3((unsigned)(rg.beg[rg.count] + tail)), dim3(256), 0, st, rg);
  rg.count = 0;
}
// items collected into the step's reduction launch (collect != NULL), or launched now as a group of their own
void red_emit(hipStream_t st, RedGroup* collect, const RedItem* items, int count) {
  RedGroup own;
  own.count = 0;
  RedGroup& rg = collect ? *collect : own;
  for (int i = 0; i < count; ++i) red_append(rg, items[i]);
  if (!collect) launch_reductions(st, own);
}
bool panel_ok(const GemmStep& E, int M, int N, int Kd, long sak, int splitk, bool rowsum, int nz) {
  return E.operands && sak == 1 && Kd <= 352 && N <= 256 && splitk <= 1 && M >= 4096 && !rowsum && E.packb &&
         nz <= E.packb_entries;
}

void gemm(GemmStep& E, hipStream_t st, int batch, int M, int N, int Kd, const Operand& A, const Operand& B, const Operand& C,
          const GemmOpts& o) {
  const long sam = A.s0, sak = A.s1, bsa = A.bs, sbk = B.s0, sbn = B.s1, bsb = B.bs;
  const int splitk = o.splitk;
  Gemm g;
  g.M = M; g.N = N; g.Kd = Kd;
  g.A = A.p; g.sam = sam; g.sak = sak; g.bsa = bsa;
  g.B = B.p; g.sbk = sbk; g.sbn = sbn; g.bsb = bsb;
  g.C = const_cast<float*>(C.p); g.scm = C.s0; g.scn = C.s1; g.bsc = C.bs;      // (the one written operand)
  g.bias = o.bias; g.bsbias = o.bsbias; g.mask = o.mask.p; g.smm = o.mask.s0; g.smn = o.mask.s1; g.bsm = o.mask.bs;
  g.accumulate = o.accumulate; g.relu = o.relu; g.splitk = splitk;
  g.rowsum = o.rowsum; g.bsrs = o.bsrs;
  g.biasrow = o.biasrow; g.bsbr = o.bsbr; g.sbr = o.sbr;
  g.vec4 = 0; g.Bp = nullptr; g.A2 = nullptr; g.sam2 = g.bsa2 = 0; g.k2 = Kd;
  g.a16 = A.h16; g.b16 = B.h16; g.m16 = o.mask.p && o.mask.h16; g.c16 = C.h16;
  const int operands = (o.fp32 || o.group) ? 0 : E.operands;
  g.a_scale = operands == 2 ? o.a_scale : 1.0f;
  g.part = o.part; g.rs_part = o.rs_part;
  const int nz = batch * (splitk > 1 ? splitk : 1);
  if (o.group && !(M >= 256 && N >= 192) && o.group->g.count < GemmGroup::MAXG) {
    GemmGroup& gr = o.group->g;             // collected; launched by group_launch()
    if (o.group->op16) {
      // gemm_group16_kernel stages both operands k-major: rows contiguous in memory (weight gradients are)
      if (!(sak != 1 && sam == 1 && sbk != 1 && sbn == 1)) { E.error = true; return; }      // (needs k-major operands)
      g.vec4 = (sak % 4 == 0 && bsa % 4 == 0 && M % 4 == 0 && ((uintptr_t)A.p & 15) == 0) ? 1 : 0;
    }
    if (gr.count == 0) gr.zbeg[0] = 0;
    gr.g[gr.count] = g;
    gr.zbeg[gr.count + 1] = gr.zbeg[gr.count] + nz;
    ++gr.count;
    return;
  }
  if (operands) {
    // operands whose rows are the contiguous dimension are staged k-major (exec is full at the transposing reads:
    // out-of-range elements are zero-filled, never masked)
    const bool akm = sak != 1 && sam == 1, bkm = sbk != 1 && sbn == 1;
    // (split-K weight gradients with a narrow output -- the x1 / x2 columns of the concatenated layers, N = 87 / 42 --
    // take the 128-row tile too: the streamed d_out^T operand is then read once instead of once per 64-row tile)
    const bool wide = M >= 256 && (N >= 192 || (akm && splitk > 1 && N >= 40)), f16 = operands == 2;
    const dim3 grid(wide ? (N + 127) / 128 : (N + 63) / 64, wide ? (M + 127) / 128 : (M + 63) / 64, nz);
    // layer GEMMs over the sample axis: resident A panel (64 rows x the whole contraction), 64 x 256 tiles
    if (panel_ok(E, M, N, Kd, sak, splitk, o.rowsum != nullptr, nz) && (wide || Kd >= 128)) {
      const int ka = o.a2.A2 ? o.a2.k2 : Kd;
      g.A2 = o.a2.A2 ? o.a2.A2 : A.p; g.sam2 = o.a2.sam2; g.bsa2 = o.a2.bsa2; g.k2 = ka;
      g.vec4 = (ka % 8 == 0 && sam % 8 == 0 && bsa % 8 == 0 && ((uintptr_t)A.p & 15) == 0) ? 1 : 0;
      if ((g.a16 && !g.vec4) || (g.c16 && g.b16)) { E.error = true; return; }   // (16-bit panel: aligned rows, one 16-bit side)
      g.Bp = E.packb;
      const dim3 pgrid(1, (M + 63) / 64, nz);
#define OBJ_G16_PANEL(OT_, KM_)                                                                                         \
      do {                                                                                                              \
        hipLaunchKernelGGL((pack_b_kernel<OT_, KM_ / 32>), dim3(KM_ / 8, nz), dim3(256), 0, st, g, (OT_*)E.packb);      \
        hipLaunchKernelGGL((gemm_bf16_kernel<2, 4, OT_, 32, 2, 4, false, false, true, KM_>), pgrid, dim3(512), 0, st, g); \
      } while (0)
      if (Kd <= 256) { if (f16) OBJ_G16_PANEL(_Float16, 256); else OBJ_G16_PANEL(__bf16, 256); }
      else { if (f16) OBJ_G16_PANEL(_Float16, 352); else OBJ_G16_PANEL(__bf16, 352); }
#undef OBJ_G16_PANEL
      return;
    }
    g.vec4 = (akm && sak % 4 == 0 && bsa % 4 == 0 && M % 4 == 0 && ((uintptr_t)A.p & 15) == 0) ? 1 : 0;
    if ((g.a16 && !(akm && g.vec4)) || g.c16 || (g.b16 && !(bkm && sbk % 4 == 0 && N % 4 == 0 && bsb % 4 == 0))) {
      E.error = true;                 // (16-bit activations in a GEMM shape that does not take them)
      return;
    }
#define OBJ_G16_LAUNCH(OT_, AK_, BK_)                                                                                   \
    do {                                                                                                                \
      if (wide) hipLaunchKernelGGL((gemm_bf16_kernel<2, 4, OT_, OBJ_G16_BK_WIDE, 4, 2, AK_, BK_>), grid, dim3(512), 0, st, g); \
      else hipLaunchKernelGGL((gemm_bf16_kernel<2, 2, OT_, OBJ_G16_BK, 2, 2, AK_, BK_>), grid, dim3(256), 0, st, g);    \
    } while (0)
#define OBJ_G16_LAUNCH_T(OT_)                                                                                           \
    do {                                                                                                                \
      if (akm && bkm) OBJ_G16_LAUNCH(OT_, true, true);                                                                  \
      else if (bkm) OBJ_G16_LAUNCH(OT_, false, true);                                                                   \
      else if (akm) OBJ_G16_LAUNCH(OT_, true, false);                                                                   \
      else OBJ_G16_LAUNCH(OT_, false, false);                                                                           \
    } while (0)
    if (f16) OBJ_G16_LAUNCH_T(_Float16); else OBJ_G16_LAUNCH_T(__bf16);
#undef OBJ_G16_LAUNCH_T
#undef OBJ_G16_LAUNCH
    return;
  }
  if (M >= 256 && N >= 192) {         // wide layer GEMMs (hidden 256): 128 x 128 tiles on 8 waves (3.5 % faster than the
                                      // same tile on 4 waves with 64 accumulator registers each).  Up to N = 128 the
                                      // 64 x 64 tiles win (measured, hidden 128): 4x the workgroups, 16 instead
                                      // of 64 accumulator registers -> occupancy hides the operand latency
    dim3 grid((N + 127) / 128, (M + 64 * OBJ_GEMM_WIDE_TM - 1) / (64 * OBJ_GEMM_WIDE_TM), nz);
    hipLaunchKernelGGL(gemm_kernel8, grid, dim3(512), 0, st, g);
  } else {
    dim3 grid((N + 63) / 64, (M + 63) / 64, nz);
    // (64-deep k stages for small grids were measured: slower -- the transposed LDS store conflicts dominate)
    hipLaunchKernelGGL((gemm_kernel<2, 2>), grid, dim3(256), 0, st, g);
  }
}

void wgrad(GemmStep& E, hipStream_t st, const WgradHow& how, int batch, int M, int N, long n, const Operand& A,
           const Operand& B, const Operand& C, float* bias_grad, float a_scale) {
  int sk = wgrad_slices(batch, M, N, n);
  if (how.group && how.group->max_slices > 0 && sk > how.group->max_slices) sk = how.group->max_slices;
  GemmOpts o;
  o.splitk = sk; o.rowsum = bias_grad; o.bsrs = C.bs; o.a_scale = a_scale; o.fp32 = how.fp32; o.group = how.group;
  // deterministic form: every slice stores its partial tile; an ordered reduction follows
  float* part = E.parts_alloc((size_t)batch * sk * M * N);
  float* rs_part = (part && bias_grad) ? E.parts_alloc((size_t)batch * sk * M) : nullptr;
  if (part && (!bias_grad || rs_part)) {
    o.part = part; o.rs_part = rs_part;
    gemm(E, st, batch, M, N, (int)n, A, B, C, o);
    RedItem r;
    r.part = part; r.rs_part = rs_part; r.C = const_cast<float*>(C.p); r.rowsum = bias_grad;
    r.M = M; r.N = N; r.sk = sk; r.batch = batch; r.scm = C.s0; r.bsc = C.bs; r.bsrs = C.bs;
    RedGroup* red = how.group ? how.group->red : nullptr;
    red_emit(st, (red && red->count < RedGroup::MAXG) ? red : nullptr, &r, 1);
    return;
  }
  if (how.need_parts) { E.parts_failed = true; return; }
  gemm(E, st, batch, M, N, (int)n, A, B, C, o);      // (no slab: float atomics)
}

void group_launch(hipStream_t st, GroupLaunch& gl) {
  GemmGroup& gr = gl.g;
  if (gr.count == 0) return;
  int mx = 1, my = 1;
  for (int i = 0; i < gr.count; ++i) {
    mx = std::max(mx, (gr.g[i].N + 63) / 64);
    my = std::max(my, (gr.g[i].M + 63) / 64);
  }
  if (gl.op16) hipLaunchKernelGGL(gemm_group16_kernel, dim3((mx + 1) / 2, (my + 1) / 2, gr.zbeg[gr.count]), dim3(512), 0, st, gr);
  else hipLaunchKernelGGL(gemm_group_kernel, dim3((mx + 1) / 2, (my + 1) / 2, gr.zbeg[gr.count] + gr.task.blocks), dim3(512), 0, st, gr);
  gr.count = 0;
  gr.task.blocks = 0;
}

}  // namespace objgen
