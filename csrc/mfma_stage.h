// Device-side staging shared by the bf16 MFMA kernels: the vector types, the transposed LDS read, the 16-byte
// global->LDS DMA, fragment reads of the two operand images of tile_index.h, the NS-buffer ring loop and the GELU
// epilogue math. One definition of each; the kernels keep only what is specific to them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tile_index.h"

namespace {

typedef __bf16 bf16;
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef __bf16 v4bf __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef short v8s __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) v4s lds_v4s;

// ds_read_b64_tr_b16: a 16-lane group supplies 4 rows x 16 columns, each lane receives one column's 4 row values
__device__ __forceinline__ v4s tr_read(const void* p) { return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)p); }
__device__ __forceinline__ v8bf cat8(v4s a, v4s b) {
  const v8s r = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(v8bf, r);
}

// 16-byte global->LDS DMA (no VGPR round trip). The LDS destination is wave-uniform: lane l lands at dst + 16 l.
// (A macro: behind a function the two-buffer rings of csrc/gemm_tn.hip compile to different code.)
#define glds16(src, dst) \
  __builtin_amdgcn_global_load_lds((const void*)(src), (__attribute__((address_space(3))) void*)(dst), 16, 0, 0)

// fragment of a row-major swizzled image: 8 consecutive k (chunk `chunk`) of image row `row`, one ds_read_b128
__device__ __forceinline__ v8bf row_frag(const unsigned char* img, int row, int chunk) {
  return *(const v8bf*)(img + row * 128 + swz(row, chunk) * 16);
}
// fragment of a token-major rotated image (t, c0, p as for tok_frag_off): 8 consecutive tokens from t of this lane's
// column, as two transposed reads 4 token rows apart at tok_frag_off (the pointers are formed in two steps, as the
// kernels always did: in one step they compile to different code)
template <int CPR>
__device__ __forceinline__ v8bf tok_frag(const unsigned char* img, int t, int c0, int p) {
  const int t2 = t + 4, c = c0 + (p >> 1);
  const unsigned char* p1 = img + tok_slot<CPR>(t, c) * 16 + 8 * (p & 1);
  const unsigned char* p2 = img + tok_slot<CPR>(t2, c) * 16 + 8 * (p & 1);
  return cat8(tr_read(p1), tr_read(p2));
}

// NS-buffer ring, NS - 1 K-tiles in flight: one K-tile's MFMAs are far shorter than a DMA's latency from L2 / MALL, so
// the loads of the next NS - 2 tiles overlap the wait for this one. issue(kt, buf) starts tile kt's DMAs into buffer
// buf, G per thread (the same count in every thread: whole DMA rounds only). A kernel issues tiles 0 .. NS - 2, then
// calls ring_next at the top of each K-tile kt and runs the tile's MFMAs on the buffer it returns. A counted
// `s_waitcnt vmcnt` retires only the oldest tile (vmcnt(0) in the tail, where nothing younger is in flight); the raw
// barrier (no vmcnt(0) drain) then orders it for every wave and frees the buffer read in the previous iteration,
// which the refill takes. (The prologue and the MFMA block stay in the kernels' own loops: wrapped in callables they
// compile to different code.)
template <int NS, int G, typename Issue>
__device__ __forceinline__ int ring_next(int kt, int KT, Issue&& issue) {
  constexpr int WAIT_STEADY = vm_wait((NS - 2) * G);
  if (kt + NS - 2 <= KT - 1)
    __builtin_amdgcn_s_waitcnt(WAIT_STEADY);  // tile kt retired, the NS - 2 after it still in flight
  else
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  if (kt + NS - 1 < KT) issue(kt + NS - 1, (kt + NS - 1) % NS);
  return kt % NS;
}

// The epilogues every NT kernel builds (csrc/gemm8.hip continues from 5). EPI_ADD_R: Y = X W^T + R (R bf16 [M, N],
// passed as `bias`): an input-gradient GEMM with the residual gradient folded in. EPI_GELU_BWD: Y = dZ = (X W^T) o
// GELU'(Z + bias), Z the saved pre-bias product of the FFN-in GEMM, plus per-workgroup column sums of the stored dZ
// (the bias gradient) into part[M / BM][N].
enum Epi { EPI_NONE = 0, EPI_BIAS = 1, EPI_BIAS_GELU = 2, EPI_ADD_R = 3, EPI_GELU_BWD = 4 };

// GELU(erf) with a branch-free erf (Abramowitz & Stegun 7.1.26: |error| <= 1.5e-7, far below the bf16 output's
// 2^-9 relative step): the library erff evaluates piecewise polynomials selected per |x|, which diverge inside a
// wave and made the fused epilogue cost more than the separate bias_gelu pass it replaces.
__device__ __forceinline__ float erf_fast(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(1.f + 0.3275911f * ax);
  const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
  return copysignf(1.f - poly * __expf(-ax * ax), x);
}
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erf_fast(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_grad_f(float x) {
  return 0.5f * (1.f + erf_fast(x * 0.70710678118654752f)) + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}

}  // namespace
