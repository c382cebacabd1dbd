// Hidden-32 training step and point evaluation (gfx950): the C entry points, the step's workspace and the kernels
// around the fused training kernel.
//
// Replaces, for cfg.training_strategy == "hip", the reference's per-iteration op sequence
//   vmap(pe_model) -> vmap(fc_model) -> loss.step_batch_loss -> backward          (train.py:424-472).
// objnerf_train_step sends other widths, longer rays and the layer-wise / fp16 modes to objnerf_generic.hip and
// objnerf_train256.hip.  A hidden-32 step with S <= 64 runs
//   * with the feature loss, feat_pre_kernel (or a GEMM + feat_rowstats_kernel): the 512-d head's per-ray inputs;
//   * the fused training kernel: launch_train32 (fp32, objnerf_train32.hip) or launch_train_bf16 (bf16,
//     objnerf_train_bf16.hip / objnerf_bf16v2_body.h), one partial-gradient slab per workgroup;
//   * with the feature loss, feat_post_kernel (or feat_scale_kernel + two split-K GEMMs) and, unless finalize_kernel
//     folds it in, feat_finish_kernel: the 512-d head's gradient;
//   * finalize_kernel: sums the slabs (no atomics on global memory, bit-reproducible run to run), the loss terms and
//     the status word, and steps AdamW when an optimiser is attached.
// eval_kernel is the forward of objnerf_eval_points / objnerf_mlp_forward.
#include <mutex>
#include "objnerf_mlp32.h"
#include "objnerf_train_common.h"
#include "objnerf_generic.h"
#include "objnerf_wg.h"
#include "objnerf_step_tail.h"

using namespace obj32;
using namespace objtrain;

namespace {

struct EvalDev {
  int K, G; long N;
  const float* params; long p_stride; const float* scale; const float* pts; const float* emb;
  float* alpha; float* color; float* hfeat;
  Layout L;
};

// ------------------------------------------------------------------------------------------------
// The step's last launch: grads[k][i] = sum_g slab[k][g][i] for every entry this configuration differentiates,
// loss_terms[k][:] = sum_g loss_part, the status word -- and, with an optimiser attached (objnerf_train_args.optim),
// torch.optim.AdamW on the element just summed (adamw_update; objnerf_step_tail.h).
// No byte mask and no zero fill: [ng_lo, ng_hi) are the entries WITHOUT a gradient (the feature branch when gt_feat is
// NULL: .grad stays None, train.py:435-438), [ext_lo, ext_hi) the entries whose gradient another kernel has already
// written to `grads` (the 512-d head: feat_finish_kernel).  Block (0, 0) also sums the loss terms of ALL objects and
// WRITES the status word (bit 0: a term above 1e5, render_rays.py:109-111; bit 1: a term that is not finite).
// flat_nwg > 0 (objnerf_train_common.h): object k's partial slabs are those of the workgroups whose share touches it,
// slot 0 .. cnt - 1 of its Gs
constexpr int XCOLS = 33;      // [fh (32) | O]: the columns of the 512-d head's per-ray records and moments
struct FinalizeArgs {
  const float* slab; const float* loss_part;
  int K, G; long P, slab_stride, p_stride;
  long ng_lo, ng_hi, ext_lo, ext_hi;
  float* grads; float* loss_terms; int* status;
  int flat_nwg, NT, Gs;
  // AdamW (params == NULL: gradients only)
  float* params; float* m; float* v; const int* flags; int* steps; int bank;
  long lo1, lo2, hi2;
  double lr, b1, b2, wd; float eps;
  const int* counts_in; int* flags_out;      // OBJNERF_TRAIN_SELF_COUNTS: derive the flags from counts [K][2], publish them
  // the 512-d head's gradient, folded in (round 6; feat_finish_kernel's arithmetic, element for element): Tpart
  // [K][Gfin][C][33], Mpart [K][Gfin][33][33] of feat_post_kernel; NULL: the entries [ext_lo, ext_hi) of `grads` were
  // written by an earlier launch.  head_w [K][C 32 + C]: feat_pre_kernel's copy of [W_of | b_of] from BEFORE the step (the
  // head gradient of an entry reads a whole row of W_of and b_of, which other threads of this launch are stepping)
  const float* Tpart; const float* Mpart; const float* head_w; int Gfin, C; long of_w, of_b;
};
// Round 6: FIN_EPT elements per thread (their slab loads are independent: FIN_EPT x G requests in flight instead of a
// chain of G latencies per thread), so an object is ~30 workgroups instead of 120 and the whole grid is resident at once
// -- the double-precision pow() preamble of the optimiser (a few microseconds of one thread, ahead of the block's
// barrier) is paid ONCE, in parallel, instead of once per round of the chip (118 -> 53 us at 50 objects, 79 beside the background chain).
constexpr int FIN_EPT = 4;
__global__ __launch_bounds__(256) void finalize_kernel(const FinalizeArgs a) {
  const int k = blockIdx.y;
  const long i0 = (long)blockIdx.x * (256 * FIN_EPT) + threadIdx.x;
  __shared__ float s_step_size[3], s_bc2_sqrt[3];
  __shared__ int s_active[3];
  __shared__ int s_bad;
  __shared__ float s_M[XCOLS * XCOLS];
  const bool first = blockIdx.x == 0 && blockIdx.y == 0;
  if (a.counts_in && first && threadIdx.x == 64) {     // derived flags: published for the host / later launches
    int e0, e1;
    early_flags_of_counts(a.counts_in, a.K, e0, e1);
    a.flags_out[0] = e0; a.flags_out[1] = e1;
  }
  if (a.params && threadIdx.x < 3) {
    const int g = threadIdx.x;
    int e0, e1;
    if (a.counts_in) early_flags_of_counts(a.counts_in, a.K, e0, e1);
    else { e0 = a.flags[0]; e1 = a.flags[1]; }
    adamw_group_begin(g, e0 != 0, e1 != 0, a.steps, a.bank, a.lr, a.b1, a.b2, first, s_active[g], s_step_size[g],
                      s_bc2_sqrt[g]);
  }
  if (first && threadIdx.x == 0) s_bad = 0;
  // the head's moments (workgroups that hold entries of [ext_lo, ext_hi) only): M = sum of the chunks' partials, in chunk order
  const long blk_lo = (long)blockIdx.x * (256 * FIN_EPT), blk_hi = blk_lo + 256 * FIN_EPT;
  const bool head_blk = a.Tpart && blk_lo < a.ext_hi && blk_hi > a.ext_lo;
  if (head_blk)
    for (int e = threadIdx.x; e < XCOLS * XCOLS; e += 256) {
      float v = 0.f;
      for (int g = 0; g < a.Gfin; ++g) v += a.Mpart[((long)k * a.Gfin + g) * XCOLS * XCOLS + e];
      s_M[e] = v;
    }
  if (a.params || first || head_blk) __syncthreads();
  int G = a.G;
  if (a.flat_nwg) {
    const long T = (long)a.K * a.NT;
    G = flat_wg_of(T, a.flat_nwg, (long)(k + 1) * a.NT - 1) - flat_wg_of(T, a.flat_nwg, (long)k * a.NT) + 1;
  }
  const int stride = a.flat_nwg ? a.Gs : a.G;
  float s[FIN_EPT];
  bool live[FIN_EPT], slabbed[FIN_EPT];
#pragma unroll
  for (int e = 0; e < FIN_EPT; ++e) {
    const long i = i0 + 256 * e;
    live[e] = i < a.P && !(i >= a.ng_lo && i < a.ng_hi);
    slabbed[e] = live[e] && !(i >= a.ext_lo && i < a.ext_hi);
    s[e] = 0.f;
  }
  const float* sl0 = a.slab + (long)k * stride * a.slab_stride + i0;
  for (int g = 0; g < G; ++g) {               // (slab order: one association for every run)
    float t[FIN_EPT];
#pragma unroll
    for (int e = 0; e < FIN_EPT; ++e) t[e] = slabbed[e] ? sl0[(long)g * a.slab_stride + 256 * e] : 0.f;
#pragma unroll
    for (int e = 0; e < FIN_EPT; ++e) s[e] += t[e];
  }
#pragma unroll
  for (int e = 0; e < FIN_EPT; ++e) {
    const long i = i0 + 256 * e;
    if (!live[e]) continue;
    const long idx = (long)k * a.p_stride + i;
    float sv_ = s[e];
    if (!slabbed[e]) {
      if (a.Tpart) {
        // d W_of[c][h] = T[c][h] + sum_j W_of[c][j] M2[j][h] + b_of[c] m1[h];  d b_of[c] = T[c][32] + W_of[c] . m1 + b_of[c] s2
        const bool is_b = i >= a.of_b;
        const int cc = is_b ? (int)(i - a.of_b) : (int)((i - a.of_w) >> 5), hh = is_b ? 32 : (int)((i - a.of_w) & 31);
        const float* hw = a.head_w + (long)k * ((long)a.C * 33);
        const float* W = hw + cc * 32;
        const float bc = hw[a.C * 32 + cc];
        float v = 0.f;
        for (int g = 0; g < a.Gfin; ++g) v += a.Tpart[((long)k * a.Gfin + g) * a.C * XCOLS + cc * XCOLS + hh];
        if (!is_b) {
          for (int j = 0; j < 32; ++j) v = fmaf(W[j], s_M[j * XCOLS + hh], v);
          sv_ = fmaf(bc, s_M[32 * XCOLS + hh], v);
        } else {
          for (int j = 0; j < 32; ++j) v = fmaf(W[j], s_M[32 * XCOLS + j], v);
          sv_ = fmaf(bc, s_M[32 * XCOLS + 32], v);
        }
      } else {
        sv_ = a.grads[idx];
      }
    }
    s[e] = sv_;
  }
#pragma unroll
  for (int e = 0; e < FIN_EPT; ++e) {
    const long i = i0 + 256 * e;
    if (!live[e]) continue;
    const long idx = (long)k * a.p_stride + i;
    const float sv_ = s[e];
    if (slabbed[e] || a.Tpart) a.grads[idx] = sv_;
    if (a.params) {
      const int g = adamw_group_of(i, a.lo1, a.lo2, a.hi2);
      if (s_active[g]) {
        float decay, w1, beta2, w2;
        adamw_coeffs(a.lr, a.b1, a.b2, a.wd, decay, w1, beta2, w2);
        adamw_update(a.params, a.m, a.v, idx, sv_, decay, w1, beta2, w2, s_step_size[g], s_bc2_sqrt[g], a.eps);
      }
    }
  }
  if (first) {
    int bad = 0;
    for (int e = threadIdx.x; e < 4 * a.K; e += blockDim.x) {
      const int kk = e >> 2;
      int Gk = a.G;
      if (a.flat_nwg) {
        const long T = (long)a.K * a.NT;
        Gk = flat_wg_of(T, a.flat_nwg, (long)(kk + 1) * a.NT - 1) - flat_wg_of(T, a.flat_nwg, (long)kk * a.NT) + 1;
      }
      float sl = 0.f;
      for (int g = 0; g < Gk; ++g) sl += a.loss_part[((long)kk * stride + g) * 4 + (e & 3)];
      a.loss_terms[e] = sl;
      bad |= loss_status_bits(sl);
    }
    if (bad) atomicOr(&s_bad, bad);
    __syncthreads();
    if (threadIdx.x == 0) *a.status = s_bad;
  }
}

// ------------------------------------------------------------------------------------------------
// Inference: 4 independent waves per workgroup, 16 points per wave per step (second-generation chain, objnerf_mlp32.h).
template <bool FEAT, bool FROM_EMB>
__global__ __launch_bounds__(256) void eval_kernel(const EvalDev a) {
  using namespace obj32n;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int k = blockIdx.x / a.G, gi = blockIdx.x % a.G;
  stage_weights32(lds, a.params + (long)k * a.p_stride, a.L, FEAT, tid, 256);
  const float* sv = lds + sv_base(FEAT);
  const float* wf = (const float*)__builtin_assume_aligned(lds + 4 * g * WROW + out_pos(c), 8);
  const float scale = FROM_EMB ? 1.0f : a.scale[k];
  const long ntiles = (a.N + 63) / 64;
  for (long tile = gi; tile < ntiles; tile += a.G) {
    asm volatile("" ::: "memory");   // keep the LDS weight reads inside the loop (no LICM into registers)
    const long n = tile * 64 + 16 * w + c;
    const bool valid = n < a.N;
    const long o = (long)k * a.N + (valid ? n : 0);
    Emb32 e;
    if (FROM_EMB) {
      embed32_load(e, a.emb + o * OBJ_EMB, g);
    } else {
      const float* p = a.pts + o * 3;
      Pe32 pe;
      pe32_project(sv, g, p[0], p[1], p[2], scale, pe);
      embed32(e, pe, g);
    }
    Acts act;
    const float hout = mlp32_forward<FEAT>(wf, sv, g, e, act);    // group 0: 10 * raw alpha, groups 1..3: colour g - 1
    if (valid) {
      if (g == 0) a.alpha[o] = hout;
      else a.color[o * 3 + g - 1] = hout;
      if (FEAT) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          float4 v = make_float4(act.hf.t[tt][0], act.hf.t[tt][1], act.hf.t[tt][2], act.hf.t[tt][3]);
          *reinterpret_cast<float4*>(a.hfeat + o * H + 16 * tt + 4 * g) = v;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Feature head hoisting, per-step helper kernels (HBM-bound on gt_feat, read twice per step).
// pre: u[r] = W_of^T g[r] is a batched GEMM (objgen::gemm_f32); this kernel adds beta[r] = b_of . g[r] and |g[r]|:
// one 16-lane group per ray, float4 loads.
__global__ __launch_bounds__(256) void feat_rowstats_kernel(const float* params, long p_stride, int off_b, int C, int R,
                                                            const float* gt_feat, float* rayin) {
  const int k = blockIdx.y;
  const int l16 = threadIdx.x & 15;
  const long r = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const float* B = params + (long)k * p_stride + off_b;
  float bs = 0.f, gs = 0.f;
  if (r < R) {
    const float* gp = gt_feat + ((long)k * R + r) * C;
    for (int cc = 4 * l16; cc < C; cc += 64) {
      const float4 gv = *reinterpret_cast<const float4*>(gp + cc);
      bs = fmaf(B[cc + 3], gv.w, fmaf(B[cc + 2], gv.z, fmaf(B[cc + 1], gv.y, fmaf(B[cc], gv.x, bs))));
      gs = fmaf(gv.w, gv.w, fmaf(gv.z, gv.z, fmaf(gv.y, gv.y, fmaf(gv.x, gv.x, gs))));
    }
  }
  bs = dpp_rowsum16(bs);
  gs = dpp_rowsum16(gs);
  if (r < R && l16 == 0) {
    float* o = rayin + ((long)k * R + r) * RAYIN;
    o[32] = bs;
    o[33] = sqrtf(gs);
  }
}
// The same three quantities in ONE pass over gt_feat (round 3): rayin[r] = [u (32) | beta | |g|] with u = W_of^T g[r],
// beta = b_of . g[r].  A workgroup of 8 waves takes 128 rays; [W_of | b_of] sits in LDS as the B operand of
// v_mfma_f32_16x16x4_f32 (two 16-column tiles of u; beta and |g|^2 on the VALU); a lane streams ITS ray's features as float4 --
// k-step j of block s uses feature 16 s + 4 q + j, a permutation of the contraction both operands share -- and squares
// them on the way for |g|.  gt_feat is read once instead of twice (GEMM + feat_rowstats_kernel: 240 + 101 us at
// K = 50, R = 4096 -> ~100 us).  C <= 512, C % 16 == 0.
constexpr int FEAT_PRE_MAXC = 512;
__global__ __launch_bounds__(512, 4) void feat_pre_kernel(const float* __restrict__ params, long p_stride, int off_w, int off_b,
                                                       int C, int R, const float* __restrict__ gt_feat,
                                                       float* __restrict__ rayin, float* __restrict__ gram,
                                                       float* __restrict__ head_snap, const uint8_t* __restrict__ labels,
                                                       int* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) float fp_lds[];       // W image [C / 16][2][64][4] | b_of [C]
  const int k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = lane & 15, q = lane >> 4;
  const float* W = params + (long)k * p_stride + off_w;
  const float* Bv = params + (long)k * p_stride + off_b;
  const int nblk = C / 16;
  // B image: W_of row-major [c][h] read coalesced, scattered into (block c >> 4, tile h >> 4, lane (h & 15) + 16 ((c >> 2) & 3),
  // element c & 3).  Round 6: beta = b_of . g runs on the VALU beside |g|^2 (4 FMAs per float4 instead of the four MFMAs
  // of a third, 15/16 empty column tile: a third of the kernel's matrix-core time), b_of is a plain vector behind the
  // image, and the 66 KB of LDS let TWO workgroups share a compute unit.
  float* fp_b = fp_lds + nblk * 2 * 64 * 4;
  for (int i = tid; i < C * 32; i += 512) {
    const int c = i >> 5, hc = i & 31;
    fp_lds[(((c >> 4) * 2 + (hc >> 4)) * 64 + (hc & 15) + 16 * ((c >> 2) & 3)) * 4 + (c & 3)] = W[i];
  }
  for (int i = tid; i < C; i += 512) fp_b[i] = Bv[i];
  __syncthreads();
  if (blockIdx.x == 0) {
    // Round 6: the object's first workgroup also forms what used to be two launches ahead of this one (a batched GEMM +
    // featg_wb_kernel) -- G = W_of^T W_of, wb = W_of^T b_of, bb = b_of . b_of for the hoisted head, from
    // the image just staged -- and a copy of [W_of | b_of] as they are BEFORE the step: finalize_kernel forms the head's
    // gradient from it while the optimiser in the same launch is already writing the parameters.
    auto lw = [&](const int c, const int h) {
      return fp_lds[(((c >> 4) * 2 + (h >> 4)) * 64 + (h & 15) + 16 * ((c >> 2) & 3)) * 4 + (c & 3)];
    };
    auto lb = [&](const int c) { return fp_b[c]; };
    if (gram)
      for (int o = tid; o < 32 * 32 + 33; o += 512) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        if (o < 1024) {
          const int h1 = o >> 5, h2 = o & 31;
          for (int c = 0; c < C; c += 4) {
            s0 = fmaf(lw(c, h1), lw(c, h2), s0); s1 = fmaf(lw(c + 1, h1), lw(c + 1, h2), s1);
            s2 = fmaf(lw(c + 2, h1), lw(c + 2, h2), s2); s3 = fmaf(lw(c + 3, h1), lw(c + 3, h2), s3);
          }
        } else if (o < 1056) {
          const int h = o - 1024;
          for (int c = 0; c < C; c += 4) {
            s0 = fmaf(lw(c, h), lb(c), s0); s1 = fmaf(lw(c + 1, h), lb(c + 1), s1);
            s2 = fmaf(lw(c + 2, h), lb(c + 2), s2); s3 = fmaf(lw(c + 3, h), lb(c + 3), s3);
          }
        } else {
          for (int c = 0; c < C; c += 4) {
            s0 = fmaf(lb(c), lb(c), s0); s1 = fmaf(lb(c + 1), lb(c + 1), s1);
            s2 = fmaf(lb(c + 2), lb(c + 2), s2); s3 = fmaf(lb(c + 3), lb(c + 3), s3);
          }
        }
        gram[(long)k * GRAM + o] = (s0 + s1) + (s2 + s3);
      }
    if (head_snap) {
      float* hs = head_snap + (long)k * ((long)C * 33);
      for (int i = tid; i < C * 32; i += 512) hs[i] = W[i];
      for (int i = tid; i < C; i += 512) hs[C * 32 + i] = Bv[i];
    }
    if (counts) {      // OBJNERF_TRAIN_SELF_COUNTS: this object's n(label == 1), n(label != 2) (label_counts_kernel's job: a launch less)
      __shared__ int s_c[16];
      int c1 = 0, c2 = 0;
      for (int r = tid; r < R; r += 512) {
        const int l = labels[(long)k * R + r];
        c1 += (l == 1); c2 += (l != 2);
      }
      for (int d = 32; d >= 1; d >>= 1) { c1 += __shfl_xor(c1, d, 64); c2 += __shfl_xor(c2, d, 64); }
      if (lane == 0) { s_c[2 * w] = c1; s_c[2 * w + 1] = c2; }
      __syncthreads();
      if (tid < 2) {
        int t = 0;
        for (int q_ = 0; q_ < 8; ++q_) t += s_c[2 * q_ + tid];
        counts[2 * k + tid] = t;
      }
    }
  }
  const f32x4* bl = reinterpret_cast<const f32x4*>(fp_lds) + lane;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  constexpr int PF = 8;                                                 // float4 loads in flight per lane: 8 blocks ahead
  for (long t0 = (long)blockIdx.x * 128; t0 < R; t0 += (long)gridDim.x * 128) {
    const long r = t0 + 16 * w + n;                                     // this lane's ray (as A row)
    const bool on = r < R;
    const float* gp = gt_feat + ((long)k * R + (on ? r : 0)) * C + 4 * q;
    f32x4 acc0 = zero, acc1 = zero;
    float gs = 0.f, bs = 0.f;
    f32x4 buf[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) buf[i] = (on && i < nblk) ? *reinterpret_cast<const f32x4*>(gp + 16 * i) : zero;
    for (int s0 = 0; s0 < nblk; s0 += PF) {
#pragma unroll
      for (int i = 0; i < PF; ++i) {
        const int sblk = s0 + i;
        const f32x4 av = buf[i];
        buf[i] = (on && sblk + PF < nblk) ? *reinterpret_cast<const f32x4*>(gp + 16 * (sblk + PF)) : zero;
        if (sblk < nblk) {
          const f32x4 b0 = bl[(sblk * 2 + 0) * 64], b1 = bl[(sblk * 2 + 1) * 64];
          const f32x4 bv = *reinterpret_cast<const f32x4*>(fp_b + 16 * sblk + 4 * q);      // b_of of this lane's four features
          gs = fmaf(av[3], av[3], fmaf(av[2], av[2], fmaf(av[1], av[1], fmaf(av[0], av[0], gs))));
          bs = fmaf(av[3], bv[3], fmaf(av[2], bv[2], fmaf(av[1], bv[1], fmaf(av[0], bv[0], bs))));
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], b0[j], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], b1[j], acc1, 0, 0, 0);
          }
        }
      }
    }
    // |g|^2 and beta: the four lanes (q) of a ray
    gs += __shfl_xor(gs, 16, 64);
    gs += __shfl_xor(gs, 32, 64);
    bs += __shfl_xor(bs, 16, 64);
    bs += __shfl_xor(bs, 32, 64);
    if (on && q == 0) {
      rayin[((long)k * R + r) * RAYIN + 32] = bs;
      rayin[((long)k * R + r) * RAYIN + 33] = sqrtf(gs);
    }
    // D: lane (n, q) register rr = row 4 q + rr (ray), column n
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const long ro = t0 + 16 * w + 4 * q + rr;
      if (ro < R) {
        float* o = rayin + ((long)k * R + ro) * RAYIN;
        o[n] = acc0[rr];
        o[16 + n] = acc1[rr];
      }
    }
  }
}
// post: the fused kernel left (fh[32], O, a, c) per ray.  d W_of = sum_r (a_r g_r + c_r F_r) fh_r^T with
// F_r = W_of fh_r + b_of O_r, so  d W_of = gt_feat^T [a fh] + W_of M2 + b_of m1^T  and
// d b_of = gt_feat^T [a O] + W_of m1 + b_of s2  with the moments  [M2 m1; . s2] = [c fh | c O]^T [fh | O].
// This kernel writes the two row-scaled copies X1 = [a fh | a O], X2 = [c fh | c O]; two GEMMs do the sums.
__global__ void feat_scale_kernel(long n, const float* rayfeat, float* X1, float* X2) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * XCOLS) return;
  const long r = i / XCOLS;
  const int j = (int)(i - r * XCOLS);
  const float* rf = rayfeat + r * RAYFEAT;
  const float v = rf[j];                  // fh[0..31], O
  X1[i] = rf[33] * v;
  X2[i] = rf[34] * v;
}
// post, round 3: the same sums in ONE pass over gt_feat, straight from the fused kernel's per-ray record (fh[32], O, a, c)
// -- no X1 / X2 copies, no split-K GEMM launches, no zero fills.  Workgroup (g, k) takes the g-th chunk of object k's
// rays; wave w owns target-feature block [64 w, 64 w + 64).  v_mfma_f32_16x16x4_f32 with the RAY as contraction index:
// A lane (i, q) streams gt_feat[ray 4 s + q][64 w + 4 i + j] as float4 (element j = the A operand of MFMA j, whose
// output rows are the features 64 w + 4 m + j), B lane (n, q) = a_r [fh | O][16 t + n] for the three column tiles ->
// T = gt_feat^T [a fh | a O].  The moments M = [c fh | c O]^T [fh | O] ride along: the B values of a lane are also its A
// values (same lane index), each wave takes every eighth ray quad, the partial tiles meet in LDS.  Partials
// Tpart [K][G][C][33], Mpart [K][G][33][33] are summed by feat_finish_kernel.  C == 512.
#ifndef FEAT_POST_PF
#define FEAT_POST_PF 4
#endif
#ifndef FEAT_POST_PFF
#define FEAT_POST_PFF 1
#endif
#ifndef FEAT_POST_WPE
#define FEAT_POST_WPE 4          // waves per SIMD the register budget is set for (4 = two 512-thread workgroups per compute unit)
#endif
__global__ __launch_bounds__(512, FEAT_POST_WPE) void feat_post_kernel(int C, int R, const float* __restrict__ gt_feat,
                                                           const float* __restrict__ rayfeat, float* __restrict__ Tpart,
                                                           float* __restrict__ Mpart) {
  // Round 6: the column of O (T[:, 32] = gt_feat^T [a O], M[32][:] = M[:][32] = sum c O fh, M[32][32] = sum c O^2) is
  // formed on the VALU -- it used to be a third 16-column MFMA tile with one live column (4 of 12 MFMAs per ray quad, 5 of the
  // 9 moment MFMAs): a third less matrix-core time, 34 KB of LDS instead of 74 (two workgroups per compute unit).
  __shared__ float s_m[8][4][64][4];                   // per wave: the 2 x 2 fh x fh moment tiles as D fragments
  __shared__ float s_o[8][36];                         // per wave: sum c O fh[0..31], sum c O^2
  const int k = blockIdx.y, g = blockIdx.x, G = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const long r_lo = (long)R * g / G, r_hi = (long)R * (g + 1) / G;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4][2], macc[2][2];
  float t32[4] = {0.f, 0.f, 0.f, 0.f};                 // sum_r a_r O_r g_r[64 w + 4 i + j] over this lane's rays (q)
  float mo0 = 0.f, mo1 = 0.f, moo = 0.f;               // sum c O fh[i], sum c O fh[16 + i], sum c O^2 (this wave's quads)
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = zero;
#pragma unroll
  for (int a_ = 0; a_ < 2; ++a_) macc[a_][0] = macc[a_][1] = zero;
  const float* gbase = gt_feat + (long)k * R * C + 64 * w + 4 * i;
  const float* fbase = rayfeat + (long)k * R * RAYFEAT;
  const long nq = (r_hi - r_lo + 3) / 4;               // ray quads of this chunk
  // in flight per lane: FEAT_POST_PF target-feature float4s (HBM) and FEAT_POST_PFF ray records (L2: the fused kernel has
  // just written them) -- 128 registers per wave at two workgroups per compute unit leave room for ~28 of prefetch
  constexpr int PF = FEAT_POST_PF, PFF = FEAT_POST_PFF;
  static_assert(PF % PFF == 0, "the record ring is indexed statically inside the unrolled loop");
  f32x4 abuf[PF];
  float fb[PFF][5];                                    // fh[i], fh[16 + i], O, a, c of this lane's ray
  auto fetch_g = [&](const long sq, f32x4& av) {
    const long r = r_lo + 4 * sq + q;
    av = (sq < nq && r < r_hi) ? *reinterpret_cast<const f32x4*>(gbase + r * C) : zero;
  };
  auto fetch_f = [&](const long sq, float (&f)[5]) {
    const long r = r_lo + 4 * sq + q;
    if (sq < nq && r < r_hi) {
      const float* rf = fbase + r * RAYFEAT;
      f[0] = rf[i]; f[1] = rf[16 + i]; f[2] = rf[32]; f[3] = rf[33]; f[4] = rf[34];
    } else {
      f[0] = f[1] = f[2] = f[3] = f[4] = 0.f;
    }
  };
#pragma unroll
  for (int p = 0; p < PF; ++p) fetch_g(p, abuf[p]);
#pragma unroll
  for (int p = 0; p < PFF; ++p) fetch_f(p, fb[p]);
  for (long s0 = 0; s0 < nq; s0 += PF) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const long sq = s0 + p;
      const f32x4 av = abuf[p];
      const float f0 = fb[p % PFF][0], f1 = fb[p % PFF][1], fo = fb[p % PFF][2], ar = fb[p % PFF][3], cr = fb[p % PFF][4];
      fetch_g(sq + PF, abuf[p]);
      fetch_f(sq + PFF, fb[p % PFF]);
      if (sq < nq) {
        const float x0 = ar * f0, x1 = ar * f1, xo = ar * fo;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], x0, acc[j][0], 0, 0, 0);
          acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], x1, acc[j][1], 0, 0, 0);
          t32[j] = fmaf(av[j], xo, t32[j]);
        }
        if ((int)(sq & 7) == w) {                      // (wave-uniform) this wave's share of the moments
          const float y0 = cr * f0, y1 = cr * f1, yo = cr * fo;
          macc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(y0, f0, macc[0][0], 0, 0, 0);
          macc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(y0, f1, macc[0][1], 0, 0, 0);
          macc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(y1, f0, macc[1][0], 0, 0, 0);
          macc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(y1, f1, macc[1][1], 0, 0, 0);
          mo0 = fmaf(yo, f0, mo0);
          mo1 = fmaf(yo, f1, mo1);
          moo = fmaf(yo, fo, moo);
        }
      }
    }
  }
  // T partial: D lane (n = i, q) register rr of MFMA j = T[c = 64 w + 4 (4 q + rr) + j][16 t + n]
  float* Tp = Tpart + ((long)k * G + g) * C * XCOLS;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      float* row = Tp + (long)(64 * w + 4 * (4 * q + rr) + j) * XCOLS;
      row[i] = acc[j][0][rr];
      row[16 + i] = acc[j][1][rr];
    }
  // column 32: the four lanes (q) of a feature group meet
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float v = t32[j];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (q == 0) Tp[(long)(64 * w + 4 * i + j) * XCOLS + 32] = v;
  }
  // moments: the O row per wave (lanes q of an entry meet), then the eight waves' partial tiles / rows in LDS
  mo0 += __shfl_xor(mo0, 16, 64); mo0 += __shfl_xor(mo0, 32, 64);
  mo1 += __shfl_xor(mo1, 16, 64); mo1 += __shfl_xor(mo1, 32, 64);
  moo += __shfl_xor(moo, 16, 64); moo += __shfl_xor(moo, 32, 64);
  if (q == 0) { s_o[w][i] = mo0; s_o[w][16 + i] = mo1; if (i == 0) s_o[w][32] = moo; }
#pragma unroll
  for (int a_ = 0; a_ < 2; ++a_)
#pragma unroll
    for (int b_ = 0; b_ < 2; ++b_)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) s_m[w][2 * a_ + b_][lane][rr] = macc[a_][b_][rr];
  __syncthreads();
  float* Mp = Mpart + ((long)k * G + g) * XCOLS * XCOLS;
  for (int e = tid; e < 4 * 64 * 4; e += 512) {
    const int rr = e & 3, ln = (e >> 2) & 63, tile = e >> 8;
    float v = 0.f;
#pragma unroll
    for (int ww = 0; ww < 8; ++ww) v += s_m[ww][tile][ln][rr];
    const int m = 16 * (tile >> 1) + 4 * (ln >> 4) + rr, nn = 16 * (tile & 1) + (ln & 15);
    Mp[m * XCOLS + nn] = v;
  }
  if (tid < 33) {                                      // M is symmetric in its O row / column: sum_r c_r O_r fh_r[h]
    float v = 0.f;
#pragma unroll
    for (int ww = 0; ww < 8; ++ww) v += s_o[ww][tid];
    Mp[32 * XCOLS + tid] = v;
    if (tid < 32) Mp[tid * XCOLS + 32] = v;
  }
}
// d W_of[c][h] = T[c][h] + sum_j W_of[c][j] M2[j][h] + b_of[c] m1[h];  d b_of[c] = T[c][32] + W_of[c] . m1 + b_of[c] s2
__global__ __launch_bounds__(256) void feat_finish_kernel(const float* params, long p_stride, int off_w, int off_b, int C,
                                                          const float* Tm /* [K][G][C][33] */,
                                                          const float* mom /* [K][G][33][33] */, float* grads, int G) {
  __shared__ float M[XCOLS][XCOLS];
  const int k = blockIdx.y;
  for (int i = threadIdx.x; i < XCOLS * XCOLS; i += 256) {
    float v = 0.f;
    for (int g = 0; g < G; ++g) v += mom[((long)k * G + g) * XCOLS * XCOLS + i];
    M[i / XCOLS][i % XCOLS] = v;
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * XCOLS) return;
  const int cc = i / XCOLS, hh = i - cc * XCOLS;
  const float* W = params + (long)k * p_stride + off_w + cc * 32;
  const float bc = params[(long)k * p_stride + off_b + cc];
  float v = 0.f;
  for (int g = 0; g < G; ++g) v += Tm[((long)k * G + g) * C * XCOLS + i];
  if (hh < 32) {
    for (int j = 0; j < 32; ++j) v = fmaf(W[j], M[j][hh], v);              // M2[j][h]  (c fh_j . fh_h)
    grads[(long)k * p_stride + off_w + cc * 32 + hh] = fmaf(bc, M[32][hh], v);   // m1[h] = (c O) . fh_h
  } else {
    for (int j = 0; j < 32; ++j) v = fmaf(W[j], M[32][j], v);
    grads[(long)k * p_stride + off_b + cc] = fmaf(bc, M[32][32], v);      // s2 = (c O) . O
  }
}

int eval_launch(const objnerf_net* net, int32_t K, int64_t N, const float* params, int64_t p_stride,
                const float* scale, const float* pts, const float* emb, float* out_alpha, float* out_color,
                float* out_hfeat, float* out_clip, void* stream) {
  EvalDev d;
  d.K = K; d.N = N; d.params = params; d.p_stride = p_stride; d.scale = scale; d.pts = pts; d.emb = emb;
  d.alpha = out_alpha; d.color = out_color; d.hfeat = out_hfeat;
  d.L = make_layout(net->feat_dim);
  const long ntiles = (N + 63) / 64;
  long G = (2L * objnerf_num_cu()) / K;
  if (G < 1) G = 1;
  if (G > ntiles) G = ntiles;
  d.G = (int)G;
  hipStream_t st = (hipStream_t)stream;
  const bool feat = out_hfeat != nullptr;
  const size_t lds_bytes = (size_t)obj32n::img_floats(feat) * 4;
  // the image with the feature layer exceeds the 64 KB default
  objnerf_once_per_device([] {
    (void)hipFuncSetAttribute((const void*)eval_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              obj32n::img_floats(true) * 4);
    (void)hipFuncSetAttribute((const void*)eval_kernel<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              obj32n::img_floats(true) * 4);
  });
  const dim3 grid(K * d.G), blk(256);
  if (emb) {
    if (feat) hipLaunchKernelGGL((eval_kernel<true, true>), grid, blk, lds_bytes, st, d);
    else hipLaunchKernelGGL((eval_kernel<false, true>), grid, blk, lds_bytes, st, d);
  } else {
    if (feat) hipLaunchKernelGGL((eval_kernel<true, false>), grid, blk, lds_bytes, st, d);
    else hipLaunchKernelGGL((eval_kernel<false, false>), grid, blk, lds_bytes, st, d);
  }
  if (hipGetLastError() != hipSuccess) return OBJNERF_ELAUNCH;
  if (out_clip) return objnerf_feature_head(net, K, N, params, p_stride, out_hfeat, nullptr, out_clip, stream);
  return OBJNERF_OK;
}

}  // namespace

extern "C" {

int objnerf_abi_version(void) { return OBJNERF_ABI_VERSION; }

int64_t objnerf_param_layout(const objnerf_net* net, int64_t offsets[OBJNERF_N_TENSORS + 1]) {
  if (!net || !offsets || net->hidden <= 0 || net->feat_dim <= 0) return OBJNERF_EINVAL;
  const int64_t H_ = net->hidden, C = net->feat_dim;
  const int64_t sizes[OBJNERF_N_TENSORS] = {H_ * OBJ_E1, H_, H_ * H_, H_, H_ * (H_ + OBJ_E1), H_, H_ * H_, H_, H_, 1,
                                            H_ * (H_ + OBJ_E2), H_, 3 * H_, 3, H_ * (H_ + OBJ_E2), H_, C * H_, C,
                                            OBJ_NDIR * 3};
  int64_t o = 0;
  for (int i = 0; i < OBJNERF_N_TENSORS; ++i) { offsets[i] = o; o += sizes[i]; }
  offsets[OBJNERF_N_TENSORS] = o;
  return (o + 63) / 64 * 64;
}

// Workgroups per object.  One workgroup per compute unit at a time (LDS), each sweeps NT / G tiles of its object and
// pays a fixed cost (weight staging, slab write + reduction) of about TILE_EQUIV tiles.  G = #CU / K fills the chip
// in one round when K divides it well (K = 50 -> 5 x 50 = 250 of 256); otherwise (K = 100, 130, 300 ...) more,
// shorter workgroups in several rounds come closer to K * NT / #CU tiles per compute unit.
static int grid_cap(int K) {
  const int g = objnerf_num_cu() / (K > 0 ? K : 1);
  return g > 32 ? g : 32;
}
static int train_grid(int K, int NT) {
  constexpr long TILE_EQUIV = 4;
  const int cu = objnerf_num_cu();
  int gmax = grid_cap(K);
  if (gmax > NT) gmax = NT;
  if (gmax < 1) gmax = 1;
  int best = 1;
  long best_cost = -1;
  for (int G = 1; G <= gmax; ++G) {
    const long rounds = ((long)K * G + cu - 1) / cu;
    const long cost = rounds * ((NT + G - 1) / G + TILE_EQUIV);
    if (best_cost < 0 || cost < best_cost) { best = G; best_cost = cost; }
  }
  return best;
}

// Flat mode of the second-generation fp32 kernel (objnerf_train_common.h): one workgroup per CU, equal shares of the flat
// (object, tile) space.  Taken when its longest workgroup (tiles + a fixed cost per segment) beats the strided grid's and
// an object's partial slabs fit the workspace (grid_cap(K) slots).
// tile_equiv: the fixed cost of a segment (LDS clear, weight staging, slab write + reduction) in tiles: ~4 for the fp32
// kernel (22 us per tile).  The bf16 kernel stays on the strided grid: its segment costs ~10 of its 7-us tiles, and
// wrapping its body in the segment loop alone cost 3.5 % (measured: 2.74 -> 2.83 ms strided, 2.79 flat).
static void choose_flat(TrainDev& d, int K, const long TILE_EQUIV) {
  const int cu = objnerf_num_cu();
  const long T = (long)K * d.NT;
  if (T < cu) return;
  const long share = (T + cu - 1) / cu;
  const long segs = 1 + (share + d.NT - 1) / d.NT;                    // segments a share can be cut into
  const long cost_flat = share + segs * TILE_EQUIV;
  const long rounds = ((long)K * d.G + cu - 1) / cu;
  const long cost_strided = rounds * ((d.NT + d.G - 1) / d.G + TILE_EQUIV);
  const long gs = ((long)d.NT * cu + T - 1) / T + 1;                  // workgroups that can touch one object
  if (cost_flat < cost_strided && gs <= grid_cap(K)) { d.flat_nwg = cu; d.Gs = (int)gs; }
}

// The hidden-32 step's workspace, laid out in one place: objnerf_train_workspace_bytes sizes it (base 0),
// objnerf_train_step hands out its regions.  Every region starts on a 256-byte boundary.
struct Workspace32 {
  float* slab;                  // [K][grid_cap(K)][ps]: the partial-gradient slabs (grid_cap bounds the workgroups per object)
  float* loss_part;             // [K][grid_cap(K)][4]
  // the feature loss only (NULL without it)
  float *rayin, *gram, *rayfeat;
  float *X1, *X2;               // [K][R][XCOLS] each, adjacent: the one-pass route keeps its partials in the room of both
  float *Tm, *mom;              // [K][C][XCOLS] | [K][XCOLS][XCOLS], one region
  float *parts_t, *parts_m;     // objgen::wgrad_f32's split-K partials of Tm and mom
  float* head_snap;             // [K][C][XCOLS]: feat_pre_kernel's copy of [W_of | b_of] for finalize_kernel
  size_t bytes;
};
static Workspace32 workspace32(uintptr_t base, int K, int R, int C, int64_t ps, bool feat) {
  Workspace32 w = {};
  auto take = [&](size_t floats) { float* p = (float*)(base + w.bytes); w.bytes += align256(floats * 4); return p; };
  w.slab = take((size_t)K * grid_cap(K) * ps);
  w.loss_part = take((size_t)K * grid_cap(K) * 4);
  if (feat) {
    w.rayin = take((size_t)K * R * RAYIN);
    w.gram = take((size_t)K * GRAM);
    w.rayfeat = take((size_t)K * R * RAYFEAT);
    w.X1 = take((size_t)K * R * XCOLS);
    w.X2 = take((size_t)K * R * XCOLS);
    w.Tm = take((size_t)K * C * XCOLS + (size_t)K * XCOLS * XCOLS);
    w.mom = w.Tm + (size_t)K * C * XCOLS;
    w.parts_t = take(objgen::wgrad_parts_floats(K, C, XCOLS, R));
    w.parts_m = take(objgen::wgrad_parts_floats(K, XCOLS, XCOLS, R));
    w.head_snap = take((size_t)K * C * XCOLS);
  }
  return w;
}

size_t objnerf_train_workspace_bytes(const objnerf_net* net, int32_t K, int32_t R, int32_t S, int32_t with_feat) {
  if (!net || K <= 0 || R <= 0 || S <= 0) return 0;
  // bit 1 of with_feat (value 2): size for the layer-wise path (OBJNERF_TRAIN_LAYERWISE)
  if (net->hidden != 32 || S > 64 || (with_feat & 2)) return objgen::train_workspace_bytes(net, K, R, S, with_feat & 1, (with_feat & 4) != 0);
  int64_t offs[OBJNERF_N_TENSORS + 1];
  const int64_t ps = objnerf_param_layout(net, offs);
  return workspace32(0, K, R, net->feat_dim, ps, (with_feat & 1) != 0).bytes;
}

int objnerf_train_step(const objnerf_net* net, const objnerf_train_args* a, void* stream) {
  (void)hipGetLastError();   // drop stale non-sticky errors of other HIP users of this thread
  if (!net || !a || !a->params || !a->scale || !a->z || !a->gt_depth || !a->gt_rgb || !a->labels || !a->counts ||
      !a->flags || !a->grads || !a->loss_terms || !a->status || !a->workspace)
    return OBJNERF_EINVAL;
  if (!a->pts && (!a->origins || !a->dirs)) return OBJNERF_EINVAL;
  if (a->K <= 0 || a->R <= 0 || a->S <= 0) return OBJNERF_EINVAL;
  if (net->n_freqs != 6) return OBJNERF_ENOTSUP;
  if ((a->mode & OBJNERF_TRAIN_FP16) && (a->mode & OBJNERF_TRAIN_BF16)) return OBJNERF_EINVAL;
  if (a->optim && (!a->optim->exp_avg || !a->optim->exp_avg_sq || !a->optim->group_steps ||
                   (a->optim->bank != 0 && a->optim->bank != 1)))
    return OBJNERF_EINVAL;
  if (net->hidden != 32 || a->S > 64 || (a->mode & (OBJNERF_TRAIN_LAYERWISE | OBJNERF_TRAIN_FP16))) {
    // wider networks (background: hidden 128) and long rays: layer-wise path, activations in the workspace
    if (a->workspace_bytes < objgen::train_workspace_bytes(net, a->K, a->R, a->S, a->gt_feat != nullptr,
                                                           (a->mode & (OBJNERF_TRAIN_FP16 | OBJNERF_TRAIN_BF16)) != 0))
      return OBJNERF_EINVAL;
    if (a->emb_debug) return OBJNERF_ENOTSUP;
    // (objgen::train_step takes OBJNERF_TRAIN_SELF_COUNTS and the optimiser itself where its one-launch kernels run
    // -- it reports what it has done through `done` -- and leaves them to the launches below otherwise)
    int done = 0;
    int rc;
#ifndef OBJ_NO_TRAIN256
    if (!(a->mode & OBJNERF_TRAIN_LAYERWISE) && obj256::applicable(net, a)) {
      if (a->mode & OBJNERF_TRAIN_SELF_COUNTS) {
        rc = objnerf_label_counts(a->K, a->R, a->labels, const_cast<int32_t*>(a->counts), const_cast<int32_t*>(a->flags), stream);
        if (rc) return rc;
      }
      rc = obj256::train_step(net, a, stream);
    } else
#endif
    rc = objgen::train_step(net, a, stream, &done);
    if (rc) return rc;
    if (a->optim && !(done & 2)) {
      int64_t offs[OBJNERF_N_TENSORS + 1];
      objnerf_param_layout(net, offs);
      const bool feat_ = a->gt_feat != nullptr;
      const objnerf_adamw_args* o = a->optim;
      return objmisc::adamw_flags_range(a->K, offs[OBJNERF_N_TENSORS], a->p_stride, const_cast<float*>(a->params), a->grads,
                                        o->exp_avg, o->exp_avg_sq, nullptr, a->flags, o->group_steps, o->bank,
                                        offs[OBJNERF_T_CL_W], offs[OBJNERF_T_FL_W], offs[OBJNERF_T_PE_B],
                                        feat_ ? offs[OBJNERF_N_TENSORS] : offs[OBJNERF_T_FL_W],
                                        feat_ ? offs[OBJNERF_N_TENSORS] : offs[OBJNERF_T_PE_B], o->lr, o->beta1, o->beta2,
                                        o->eps, o->weight_decay, stream);
    }
    return OBJNERF_OK;
  }
  const bool self_counts = (a->mode & OBJNERF_TRAIN_SELF_COUNTS) != 0;
  const bool feat = a->gt_feat != nullptr;
  // (with the feature loss feat_pre_kernel's first workgroup of every object counts the labels: no launch of its own)
  const bool counts_in_pre = self_counts && feat && net->feat_dim <= FEAT_PRE_MAXC && net->feat_dim % 16 == 0;
  if (self_counts && !counts_in_pre) {
    // per-object counts only (one workgroup per object, no zero fill, no atomics): the fused kernel's workgroups derive
    // the cross-object flags from them and finalize_kernel publishes the pair
    const int rc = objmisc::label_counts_only(a->K, a->R, a->labels, const_cast<int32_t*>(a->counts), stream);
    if (rc) return rc;
  }
  if (feat && (TS / a->S) > 16) return OBJNERF_ENOTSUP;
  const bool bf16 = (a->mode & OBJNERF_TRAIN_BF16) != 0;
  if (bf16 && (a->relu_masks || a->emb_debug)) return OBJNERF_ENOTSUP;
  int64_t offs[OBJNERF_N_TENSORS + 1];
  const int64_t ps = objnerf_param_layout(net, offs);
  if (a->p_stride < offs[OBJNERF_N_TENSORS]) return OBJNERF_EINVAL;
  const int C = net->feat_dim;
  const Workspace32 ws = workspace32((uintptr_t)a->workspace, a->K, a->R, C, ps, feat);
  if (a->workspace_bytes < ws.bytes) return OBJNERF_EINVAL;

  TrainDev d;
  d.K = a->K; d.R = a->R; d.S = a->S;
  d.TR = TS / a->S;
  d.NT = (a->R + d.TR - 1) / d.TR;
  d.G = train_grid(a->K, d.NT);
  d.flat_nwg = 0; d.Gs = 0;
  d.color_scaling = a->color_scaling; d.opacity_scaling = a->opacity_scaling; d.feat_scaling = a->feat_scaling;
  d.obj_center = a->obj_center;
  d.params = a->params; d.p_stride = a->p_stride; d.scale = a->scale;
  d.pts = a->pts; d.origins = a->origins; d.dirs = a->dirs; d.z = a->z;
  d.gt_depth = a->gt_depth; d.gt_rgb = a->gt_rgb; d.labels = a->labels; d.gt_feat = a->gt_feat;
  d.counts = a->counts; d.flags = a->flags; d.derive_flags = self_counts ? 1 : 0;
  d.L = make_layout(net->feat_dim);
  d.slab = ws.slab;
  d.slab_stride = ps;
  d.loss_part = ws.loss_part;
  d.rayin = ws.rayin; d.gram = ws.gram; d.rayfeat = ws.rayfeat;
  d.relu_masks = a->relu_masks;
  d.emb_debug = a->emb_debug;

  hipStream_t st = (hipStream_t)stream;
  // (no byte mask and no zero fills: finalize_kernel takes the ranges without a gradient as arguments -- without
  // gt_feat the whole feature branch has none (train.py:435-438 -> .grad stays None); with it, the 512-d head's
  // gradient is produced by feat_finish_kernel instead of the slabs -- and writes the status word itself)
  const float *fin_T = nullptr, *fin_M = nullptr;
  int fin_G = 0;
  if (feat) {
    const bool pre_one = C <= FEAT_PRE_MAXC && C % 16 == 0;
    if (!pre_one) objgen::feat_gram(stream, {a->K, 0, 32, C, a->params, (long)a->p_stride, d.L.of_w, d.L.of_b, nullptr}, ws.gram, GRAM);
    // u = gt_feat W_of  ([R x C] [C x 32] per object) on the batched MFMA GEMM; beta, |g| beside it
    if (pre_one) {
      // u, beta, |g| in one pass over gt_feat (feat_pre_kernel)
      const size_t pre_lds = ((size_t)(C / 16) * 2 * 64 * 4 + C) * sizeof(float);
      objnerf_once_per_device([] {
        (void)hipFuncSetAttribute((const void*)feat_pre_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(((FEAT_PRE_MAXC / 16) * 2 * 64 * 4 + FEAT_PRE_MAXC) * sizeof(float)));
      });
      int gpo = 2 * objnerf_num_cu() / a->K;              // workgroups per object: one round of the chip at two per compute unit
      if (gpo < 1) gpo = 1;
      if (gpo > (a->R + 127) / 128) gpo = (a->R + 127) / 128;
      hipLaunchKernelGGL(feat_pre_kernel, dim3(gpo, a->K), dim3(512), pre_lds, st, a->params, (long)a->p_stride,
                         d.L.of_w, d.L.of_b, C, a->R, a->gt_feat, ws.rayin, ws.gram, ws.head_snap, a->labels,
                         counts_in_pre ? const_cast<int32_t*>(a->counts) : nullptr);
    } else {
      objgen::gemm_f32(stream, a->K, a->R, 32, C, objgen::op_rows(a->gt_feat, C, (long)a->R * C),
                       objgen::op_rows(a->params + d.L.of_w, 32, (long)a->p_stride),
                       objgen::op_rows(ws.rayin, RAYIN, (long)a->R * RAYIN), false);
      hipLaunchKernelGGL(feat_rowstats_kernel, dim3((a->R + 15) / 16, a->K), dim3(256), 0, st, a->params,
                         (long)a->p_stride, d.L.of_b, C, a->R, a->gt_feat, ws.rayin);
    }
    if (bf16) launch_train_bf16(d, stream, true);
    else { choose_flat(d, a->K, 4); launch_train32(d, stream, true); }
    if (hipGetLastError() != hipSuccess) return OBJNERF_ELAUNCH;
    // 512-d head gradient from the per-ray (fh, O, a, c): two split-K GEMMs over the rays + a small finish
    const long nr = (long)a->K * a->R;
    int gpo = 2 * objnerf_num_cu() / a->K;                // ray chunks per object: one round of the chip at two workgroups per compute unit
    if (gpo < 1) gpo = 1;
    if (gpo > 16) gpo = 16;
    // the partials live in the room of X1 AND X2 (adjacent in the workspace, both unused on this route): 2 K R XCOLS floats.
    // (Round 4 used X1's room only and at most 8 chunks: a rank's share of configs[3] -- 15 objects -- then ran 105
    // workgroups over 126 MB of target features, 1.1 TB/s.)
    const size_t part_room = ((size_t)((char*)ws.X2 - (char*)ws.X1) / 4 + (size_t)a->K * a->R * XCOLS) / (size_t)a->K;
    while (gpo > 1 && (size_t)gpo * ((size_t)C * XCOLS + XCOLS * XCOLS) > part_room) --gpo;
    const bool one_pass = C == 512 && (size_t)gpo * ((size_t)C * XCOLS + XCOLS * XCOLS) <= part_room;
    int Gfin = 1;
    const float *Tsrc = ws.Tm, *Msrc = ws.mom;
    if (one_pass) {
      float* Tpart = ws.X1;
      float* Mpart = ws.X1 + (size_t)a->K * gpo * C * XCOLS;
      hipLaunchKernelGGL(feat_post_kernel, dim3(gpo, a->K), dim3(512), 0, st, C, a->R, a->gt_feat, ws.rayfeat, Tpart, Mpart);
      Gfin = gpo; Tsrc = Tpart; Msrc = Mpart;
    } else {
      hipLaunchKernelGGL(feat_scale_kernel, dim3((unsigned)((nr * XCOLS + 255) / 256)), dim3(256), 0, st, nr, ws.rayfeat, ws.X1, ws.X2);
      (void)hipMemsetAsync(ws.Tm, 0, ((size_t)a->K * C * XCOLS + (size_t)a->K * XCOLS * XCOLS) * 4, st);
      objgen::wgrad_f32(stream, a->K, C, XCOLS, a->R, objgen::op_cols(a->gt_feat, C, (long)a->R * C),
                        objgen::op_rows(ws.X1, XCOLS, (long)a->R * XCOLS), objgen::op_rows(ws.Tm, XCOLS, (long)C * XCOLS),
                        ws.parts_t, objgen::wgrad_parts_floats(a->K, C, XCOLS, a->R));
      objgen::wgrad_f32(stream, a->K, XCOLS, XCOLS, a->R, objgen::op_cols(ws.X2, XCOLS, (long)a->R * XCOLS),
                        objgen::op_rows(ws.rayfeat, RAYFEAT, (long)a->R * RAYFEAT),
                        objgen::op_rows(ws.mom, XCOLS, (long)XCOLS * XCOLS), ws.parts_m,
                        objgen::wgrad_parts_floats(a->K, XCOLS, XCOLS, a->R));
    }
    if (one_pass && pre_one) {      // finalize_kernel forms the head's gradient itself (round 6: one launch fewer)
      fin_T = Tsrc; fin_M = Msrc; fin_G = Gfin;
    } else {
      hipLaunchKernelGGL(feat_finish_kernel, dim3((C * XCOLS + 255) / 256, a->K), dim3(256), 0, st, a->params,
                         (long)a->p_stride, d.L.of_w, d.L.of_b, C, Tsrc, Msrc, a->grads, Gfin);
    }
  } else if (bf16) {
    launch_train_bf16(d, stream, false);
  } else {
    choose_flat(d, a->K, 4);
    launch_train32(d, stream, false);
  }
  if (hipGetLastError() != hipSuccess) return OBJNERF_ELAUNCH;
  const long P = offs[OBJNERF_N_TENSORS];
  dim3 fg((unsigned)((P + 256 * FIN_EPT - 1) / (256 * FIN_EPT)), (unsigned)a->K);
  FinalizeArgs fa;
  fa.slab = d.slab; fa.loss_part = d.loss_part; fa.K = a->K; fa.G = d.G; fa.P = P; fa.slab_stride = (long)ps;
  fa.p_stride = (long)a->p_stride;
  fa.ng_lo = feat ? P : d.L.fl_w; fa.ng_hi = feat ? P : d.L.pe_b;
  fa.ext_lo = feat ? d.L.of_w : P; fa.ext_hi = feat ? d.L.pe_b : P;
  fa.grads = a->grads; fa.loss_terms = a->loss_terms; fa.status = a->status;
  fa.flat_nwg = d.flat_nwg; fa.NT = d.NT; fa.Gs = d.Gs;
  fa.params = nullptr; fa.m = fa.v = nullptr; fa.flags = a->flags; fa.steps = nullptr; fa.bank = 0;
  fa.lo1 = offs[OBJNERF_T_CL_W]; fa.lo2 = offs[OBJNERF_T_FL_W]; fa.hi2 = offs[OBJNERF_T_PE_B];
  fa.lr = fa.b1 = fa.b2 = fa.wd = 0.0; fa.eps = 0.f;
  fa.counts_in = self_counts ? a->counts : nullptr; fa.flags_out = const_cast<int*>(a->flags);
  fa.Tpart = fin_T; fa.Mpart = fin_M; fa.head_w = ws.head_snap; fa.Gfin = fin_G; fa.C = C; fa.of_w = d.L.of_w; fa.of_b = d.L.of_b;
  if (a->optim) {
    const objnerf_adamw_args* o = a->optim;
    fa.params = const_cast<float*>(a->params); fa.m = o->exp_avg; fa.v = o->exp_avg_sq; fa.steps = o->group_steps;
    fa.bank = o->bank; fa.lr = (double)o->lr; fa.b1 = (double)o->beta1; fa.b2 = (double)o->beta2;
    fa.wd = (double)o->weight_decay; fa.eps = o->eps;
  }
  hipLaunchKernelGGL(finalize_kernel, fg, dim3(256), 0, st, fa);
  if (hipGetLastError() != hipSuccess) return OBJNERF_ELAUNCH;
  return OBJNERF_OK;
}

int objnerf_eval_points(const objnerf_net* net, int32_t K, int64_t N, const float* params, int64_t p_stride,
                        const float* scale, const float* pts, float* out_alpha, float* out_color, float* out_hfeat,
                        float* out_clip, void* stream) {
  (void)hipGetLastError();
  if (!net || !params || !scale || !pts || !out_alpha || !out_color || K <= 0 || N <= 0) return OBJNERF_EINVAL;
  if (net->hidden != 32 || net->n_freqs != 6) return OBJNERF_ENOTSUP;
  if (out_clip && !out_hfeat) return OBJNERF_EINVAL;   // the head runs on the H-wide hidden
  return eval_launch(net, K, N, params, p_stride, scale, pts, nullptr, out_alpha, out_color, out_hfeat, out_clip,
                     stream);
}

size_t objnerf_eval_workspace_bytes(const objnerf_net* net, int32_t K, int64_t N) {
  if (!net || K <= 0 || N <= 0 || net->hidden == 32) return 0;
  return objgen::eval_workspace_bytes(net, K, (long)N);
}

int objnerf_eval_points_ws(const objnerf_net* net, int32_t K, int64_t N, const float* params, int64_t p_stride,
                           const float* scale, const float* pts, float* out_alpha, float* out_color, float* out_hfeat,
                           float* out_clip, void* workspace, size_t workspace_bytes, void* stream) {
  (void)hipGetLastError();
  if (!net || !params || !scale || !pts || !out_alpha || !out_color || K <= 0 || N <= 0) return OBJNERF_EINVAL;
  if (net->hidden == 32)
    return objnerf_eval_points(net, K, N, params, p_stride, scale, pts, out_alpha, out_color, out_hfeat, out_clip, stream);
  return objgen::eval_points(net, K, (long)N, params, (long)p_stride, scale, pts, out_alpha, out_color, out_hfeat,
                             out_clip, workspace, workspace_bytes, stream);
}

int objnerf_mlp_forward(const objnerf_net* net, int32_t K, int64_t N, const float* params, int64_t p_stride,
                        const float* emb, float* out_alpha, float* out_color, float* out_hfeat, float* out_clip,
                        void* stream) {
  (void)hipGetLastError();
  if (!net || !params || !emb || !out_alpha || !out_color || K <= 0 || N <= 0) return OBJNERF_EINVAL;
  if (net->hidden != 32 || net->n_freqs != 6) return OBJNERF_ENOTSUP;
  if (out_clip && !out_hfeat) return OBJNERF_EINVAL;
  return eval_launch(net, K, N, params, p_stride, nullptr, nullptr, emb, out_alpha, out_color, out_hfeat, out_clip,
                     stream);
}

int objnerf_mlp_forward_ws(const objnerf_net* net, int32_t K, int64_t N, const float* params, int64_t p_stride,
                           const float* emb, float* out_alpha, float* out_color, float* out_hfeat, float* out_clip,
                           void* workspace, size_t workspace_bytes, void* stream) {
  (void)hipGetLastError();
  if (!net || !params || !emb || !out_alpha || !out_color || K <= 0 || N <= 0) return OBJNERF_EINVAL;
  if (net->hidden == 32)
    return objnerf_mlp_forward(net, K, N, params, p_stride, emb, out_alpha, out_color, out_hfeat, out_clip, stream);
  return objgen::eval_points(net, K, (long)N, params, (long)p_stride, nullptr, nullptr, out_alpha, out_color, out_hfeat,
                             out_clip, workspace, workspace_bytes, stream, emb);
}

size_t objnerf_mlp_backward_workspace_bytes(const objnerf_net* net, int32_t K, int64_t N, int32_t with_clip) {
  if (!net || K <= 0 || N <= 0) return 0;
  return objgen::mlp_backward_workspace_bytes(net, K, (long)N, with_clip);
}

int objnerf_mlp_backward_ws(const objnerf_net* net, int32_t K, int64_t N, const float* params, int64_t p_stride,
                            const float* emb, const float* d_alpha, const float* d_color, const float* d_clip,
                            float* grads, float* d_emb, void* workspace, size_t workspace_bytes, void* stream) {
  (void)hipGetLastError();
  if (!net || !params || !emb || !d_alpha || !d_color || !grads || !d_emb || K <= 0 || N <= 0) return OBJNERF_EINVAL;
  return objgen::mlp_backward(net, K, (long)N, params, (long)p_stride, emb, d_alpha, d_color, d_clip, grads, d_emb, workspace,
                              workspace_bytes, stream);
}

int objnerf_embed_bwd(const objnerf_net* net, int32_t K, int64_t N, const float* params, int64_t p_stride,
                      const float* scale, const float* pts, const float* d_emb, float* d_B, float* scratch, void* stream) {
  (void)hipGetLastError();
  if (!net || !params || !scale || !pts || !d_emb || !d_B || !scratch || K <= 0 || N <= 0) return OBJNERF_EINVAL;
  return objgen::embed_backward(net, K, (long)N, params, (long)p_stride, scale, pts, d_emb, d_B, scratch, stream);
}

}  // extern "C"
