// Internal interface of the layer-wise path's GEMM layer (objnerf_gemm.hip): the kernels' argument structs and the host
// calls that choose and launch them.  A call names its operands (Operand, objnerf_generic.h) and its modifiers
// (GemmOpts / WgradHow); a step holds what does not change between its calls (GemmStep); a grouped launch is an object
// of its own (GroupLaunch).  Nothing here means "the next call".
#pragma once
#include <hip/hip_runtime.h>
#include "objnerf_generic.h"
#include "objnerf_featprep.h"

namespace objgen {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// C[m][n] (+)= sum_k A(m,k) B(k,n), generic strides, batched over blockIdx.z.  Epilogue (in order):
// + bias[n], * scale, relu, mask (C = mask(m,n) > 0 ? C : 0).
struct Gemm {
  int M, N, Kd;
  const float* A; long sam, sak, bsa;
  const float* B; long sbk, sbn, bsb;
  float* C; long scm, scn, bsc;
  const float* bias; long bsbias;
  const float* mask; long smm, smn, bsm;
  int accumulate, relu;
  int splitk;      // > 1: blockIdx.z = batch * splitk + slice; each slice atomically adds its partial into C
  float* rowsum; long bsrs;   // optional: rowsum[m] += sum_k A(m,k)  (bias gradient riding on the weight-gradient GEMM)
  const float* biasrow; long bsbr;   // optional per-row factor of the bias: + bias[n] * biasrow[m sbr]
  int sbr;
  float* part; float* rs_part;   // split-K with these set: slice s of batch z STORES its partial tile at part[((z sk + s) M + m)
                                 // N + n] (row sums: rs_part[(z sk + s) M + m]) and reduce_parts_kernel adds the slices in
                                 // order -- bit-reproducible; NULL: float atomics into C / rowsum
  int vec4;        // A is read with dwordx4 loads: AFULL panel rows / k-major A rows are 16-byte aligned
  const void* Bp;  // AFULL: B packed as 16-bit MFMA operands, [z][k / 32][n / 16][lane][8] (pack_b_kernel)
  int a16, b16, m16, c16;   // 16-bit kernels: A / B / mask / C are arrays of the kernel's operand type (the layer-wise
                            // path keeps h1 .. hc in 16 bit in the 16-bit modes); element strides as for floats
  const float* A2; long sam2, bsa2; int k2;   // AFULL: columns k >= k2 of A come from A2[m sam2 + (k - k2)] (the
                                              // concatenated layers [h | x] as ONE contraction); k2 >= Kd: none
  float a_scale;   // 16-bit operand kernels: A is multiplied by this power of two before it is rounded and the result
                   // divided by it (keeps back-propagated gradients out of fp16's subnormal range); 1 elsewhere
};

// Several independent GEMMs in ONE launch (the weight-gradient GEMMs of a small-batch step: each alone is ~260
// workgroups of latency-bound work): blockIdx.z runs over the concatenated (batch x split-K) slices of all of them.
struct GemmGroup {
  static constexpr int MAXG = 11;
  int count;
  int zbeg[MAXG + 1];
  Gemm g[MAXG];
  FeatPrepTask task;
};

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
template <typename OT> struct Op16;
template <> struct Op16<__bf16> {
  typedef bf16x8 V;
  static __device__ __forceinline__ __bf16 cvt(float x) { return (__bf16)x; }
  static __device__ __forceinline__ f32x4 mfma(V a, V b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Op16<_Float16> {
  typedef f16x8 V;
  static __device__ __forceinline__ _Float16 cvt(float x) { return (_Float16)fminf(fmaxf(x, -65504.0f), 65504.0f); }
  static __device__ __forceinline__ f32x4 mfma(V a, V b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
// gfx950's transposing LDS read (see the k-major staging of gemm_bf16_body, objnerf_gemm.hip)
typedef short s16x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint2 lds_tr16(const void* p) {
  const s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3)))*)(p));
  return __builtin_bit_cast(uint2, v);
}

struct RedItem {
  const float* part; const float* rs_part; float* C; float* rowsum;
  int M, N, sk, batch;
  long scm, bsc, bsrs;
};
// Optional tail of the step's reduction launch (the one-launch small-batch iteration, objnerf_small_body.h): the block
// after the last item's sums the per-workgroup loss terms in workgroup order and WRITES the status word
// (loss_total_kernel's job), and -- with params set -- every thread that has just summed a gradient element applies
// torch.optim.AdamW to it (objnerf_step_tail.h; the flag-dependent skipping and the per-group step counters
// included), so the iteration has no optimiser launch and the gradient is not read back.
struct RedTail {
  const float* loss_part = nullptr; int loss_blocks, K; float* loss_terms; int* status;      // loss_part == NULL: no tail
  float* params = nullptr; const float* grads; float* m; float* v; const int* flags; int* steps; int bank;   // params == NULL: no AdamW
  long p_stride, lo1, lo2, hi2, arena_floats;      // (sums that land outside [grads, grads + arena_floats) are not parameters' gradients)
  double lr, b1, b2, wd; float eps;
};
struct RedGroup {
  static constexpr int MAXG = 16;        // (>= the GEMM group's capacity + head sums + d B: a step's reductions in ONE launch)
  int count;
  int beg[MAXG + 1];      // first block of each item
  RedItem it[MAXG];
  RedTail tail;
};

// ---- what a STEP holds: filled once when the workspace is carved and not written by the step's code afterwards (the
// calls below advance the slab allocator and raise the sticky flags).  One per C-ABI call, on that call's stack.
struct GemmStep {
  int operands = 0;                 // 0: fp32 GEMMs, 1: bf16 operands, 2: fp16 operands
  void* packb = nullptr;            // scratch of the resident-panel GEMMs' packed B images (176 KB per batch entry)
  long packb_entries = 0;
  // bump allocator over the caller's workspace region for the partial slabs of ONE step (the weight-gradient GEMMs of
  // a step run side by side, so each has its own slab); exhausted or absent -> atomics
  float* parts = nullptr;
  size_t parts_cap = 0, parts_off = 0;
  bool error = false;               // a GEMM of the step was handed operands its kernel does not take: the step returns
                                    // OBJNERF_EINVAL (a library call never ends the host process)
  bool parts_failed = false;        // a weight gradient that needs the slab form (WgradHow) did not get its slab
  float* parts_alloc(size_t floats) {
    floats = (floats + 63) / 64 * 64;
    if (!parts || parts_off + floats > parts_cap) return nullptr;
    float* p = parts + parts_off;
    parts_off += floats;
    return p;
  }
};

// ---- a grouped launch: owns its kernel argument, the operand type of its GEMMs, the slice cap of the weight gradients
// added to it and the reduction group their ordered sums are collected into.  gemm() / wgrad() add to it
// (GemmOpts::group, WgradHow::group); group_launch() enqueues what was added and empties it -- nothing else changes.
// The caller launches the collected reductions (launch_reductions).
struct GroupLaunch {
  GemmGroup g;
  const bool op16;                  // bf16 operands, both k-major (gemm_group16_kernel); else fp32 (gemm_group_kernel)
  const int max_slices;             // > 0: a weight gradient added here is cut into at most this many split-K slices
  RedGroup* const red;              // non-null: those weight gradients' reductions are appended here, not launched
  explicit GroupLaunch(bool op16_ = false, int max_slices_ = 0, RedGroup* red_ = nullptr)
      : op16(op16_), max_slices(max_slices_), red(red_) { g.count = 0; }
};
void group_launch(hipStream_t st, GroupLaunch& gl);

// ---- the modifiers of ONE gemm() call
struct A2Src { const float* A2; long sam2, bsa2; int k2; };
struct GemmOpts {
  bool accumulate = false, relu = false;
  const float* bias = nullptr; long bsbias = 0;                    // + bias[n]
  const float* biasrow = nullptr; long bsbr = 0; int sbr = 1;      // ... times biasrow[z bsbr + m sbr]
  Operand mask = {nullptr, 0, 0, 0, false};                        // C = mask(m, n) > 0 ? C : 0
  int splitk = 1;                                                  // with its row sums of A and its partial slabs (Gemm)
  float* rowsum = nullptr; long bsrs = 0;
  float* part = nullptr; float* rs_part = nullptr;
  A2Src a2 = {nullptr, 0, 0, 0};    // second A source (Gemm::A2); taken by the resident-panel kernel only
  float a_scale = 1.0f;             // Gemm::a_scale (fp16 operands: A is a back-propagated gradient)
  bool fp32 = false;                // an fp32 GEMM whatever the step's operand precision
  GroupLaunch* group = nullptr;     // add to this grouped launch; a GEMM it does not take runs at once, as an fp32 GEMM
};
void gemm(GemmStep& E, hipStream_t st, int batch, int M, int N, int Kd, const Operand& A, const Operand& B, const Operand& C,
          const GemmOpts& o = {});
// the layer GEMMs the resident-panel kernel takes (16-bit modes, rows k-contiguous, contraction <= 352, N <= 256)
bool panel_ok(const GemmStep& E, int M, int N, int Kd, long sak, int splitk, bool rowsum, int nz);

// ---- weight gradient: C[M][N] = sum over the n samples (C.s1 == 1); few output tiles, long contraction -> split-K, every
// slice storing its partial tile in a slab of the step and an ordered reduction behind it (bit-reproducible).  Without a
// slab: float atomics into a pre-zeroed C.  bias_grad (optional): [M] column sums of the output-gradient operand A, same pass.
struct WgradHow {
  GroupLaunch* group = nullptr;     // the GEMM joins this grouped launch, its reduction the group's RedGroup
  bool need_parts = false;          // the slab form is required (the gradient arena is not zero-filled): no slab = error
  bool fp32 = false;                // as GemmOpts::fp32
};
int wgrad_slices(int batch, int M, int N, long n);
void wgrad(GemmStep& E, hipStream_t st, const WgradHow& how, int batch, int M, int N, long n, const Operand& A,
           const Operand& B, const Operand& C, float* bias_grad = nullptr, float a_scale = 1.0f);

// ---- ordered reductions (reduce_parts_kernel): items collected into a step's RedGroup (collect != NULL) or launched now
void red_emit(hipStream_t st, RedGroup* collect, const RedItem* items, int count);
void launch_reductions(hipStream_t st, RedGroup& rg);

}  // namespace objgen
