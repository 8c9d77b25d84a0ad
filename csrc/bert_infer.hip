// BERT inference over PACKED variable-length sequences on gfx950 (mifx/models/bert_infer.py): the activations are
// [T, hidden] with T = sum of the sequence lengths, no padding rows. Two kernels; every other op of the forward is
// token-wise and runs the training forward's kernels (csrc/fused_bert.hip at p = 0) on T rows.
//
// attn_fwd_varlen: forward-only self-attention per sequence from a cu_seqlens table; no dropout, no bias, no saved
// statistics: the chunked forward of csrc/attn_chunked.h over its Packed geometry (a workgroup of 8 waves owns 128
// queries of one (sequence, head), that head's K and V rows resident in LDS, keys streamed in chunks of 64 with the
// online softmax), with the ragged edge of a sequence of any length 1 .. 512 as described there. The dynamic LDS is
// sized from the longest sequence of the launch (rounded up to 64), not from 512: a batch of requests of up to 128
// tokens takes 36 KB per workgroup, four workgroups per CU.
// The work list is a block table of (sequence, 128-query block) pairs, one workgroup per entry and head; entries of
// -1 exit at once, so a captured graph launches the grid of its token capacity and the host rewrites the table.
//
// embed_ln_packed: x[t] = LayerNorm(word[ids[t]] + pos[pos_id[t]] + type[tt[t]]) with explicit per-token position
// ids (they restart at 0 in every sequence): one wave per token, fp32 inside, rounded once to bf16 on the way out,
// as the fused add + LayerNorm of the training forward rounds. Tokens with id < 0 (the rows from T up to the token
// capacity) are written as zeros.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_chunked.h"

namespace {

constexpr int varlen_lds(int l64) { return 2 * l64 * LD * 2; }

__global__ __launch_bounds__(NT) void attn_fwd_varlen(const bf16* __restrict__ qkv, const int* __restrict__ cu,
                                                      const int* __restrict__ table, int nseq, int rows, int lmax64,
                                                      float scale, int H, bf16* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) bf16 smem[];
  chunked_fwd<Packed, false>(Packed(cu, table, nseq, rows, lmax64, H, 0), smem, qkv, scale, Drop{}, H, out, nullptr);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ void ld4(const bf16* p, float* o) {
  const v4bf v = *(const v4bf*)p;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (float)v[i];
}

// one wave per token; lane owns chunks of 4 contiguous columns, chunk j of lane l = columns [4 (64 j + l), +4)
// (Hd % 4 == 0, Hd <= 256 NC). An id, position or token type outside its table writes zeros (never an
// out-of-bounds read; the host validates requests before they get here).
template <int NC>
__global__ __launch_bounds__(256) void embed_ln_packed(const int* __restrict__ ids, const int* __restrict__ tts,
                                                       const int* __restrict__ pos_ids, const bf16* __restrict__ word,
                                                       const bf16* __restrict__ pos, const bf16* __restrict__ type,
                                                       const bf16* __restrict__ gamma, const bf16* __restrict__ beta,
                                                       int rows, int Hd, int V, int P, int TV, float eps,
                                                       bf16* __restrict__ x) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= rows) return;
  const int id = ids[t], tt = tts[t], ps = pos_ids[t];
  const bool ok = id >= 0 && id < V && tt >= 0 && tt < TV && ps >= 0 && ps < P;
  float v[NC][4];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int c = 4 * (64 * j + lane);
    v[j][0] = v[j][1] = v[j][2] = v[j][3] = 0.f;
    if (ok && c < Hd) {
      float a[4], b[4], d[4];
      ld4(word + (size_t)id * Hd + c, a);
      ld4(pos + (size_t)ps * Hd + c, b);
      ld4(type + (size_t)tt * Hd + c, d);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[j][e] = a[e] + b[e] + d[e];
        s += v[j][e];
      }
    }
  }
  const float mean = wave_sum(s) / Hd;
  float qq = 0.f;
#pragma unroll
  for (int j = 0; j < NC; ++j)
    if (4 * (64 * j + lane) < Hd)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = v[j][e] - mean;
        qq += d * d;
      }
  const float rstd = rsqrtf(wave_sum(qq) / Hd + eps);
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int c = 4 * (64 * j + lane);
    if (c < Hd) {
      v4f o = kZero4;
      if (ok) {
        float g[4], b[4];
        ld4(gamma + c, g);
        ld4(beta + c, b);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (v[j][e] - mean) * rstd * g[e] + b[e];
      }
      *(v4bf*)(x + (size_t)t * Hd + c) = pack4(o);
    }
  }
}

}  // namespace

extern "C" {

// qkv [rows, 3, H, 64] bf16 (contiguous), cu int32 [nseq + 1] (device): sequence b owns rows cu[b] .. cu[b + 1] - 1,
// 1 <= length <= 512; table int32 [nent, 2] (device): (sequence, 128-query block) per workgroup, -1 entries exit at
// once; out [rows, H, 64] bf16 (rows of no sequence are left untouched). lmax: an upper bound of the longest
// sequence of this launch (the dynamic LDS is sized from it; a longer sequence in the table is skipped).
int mifx_attn_fwd_varlen(const void* qkv, const int* cu, const int* table, int nseq, int nent, int rows, int lmax,
                         int H, float scale, void* out, hipStream_t st) {
  if (nseq <= 0 || nent <= 0 || rows <= 0 || H <= 0 || lmax < 1 || lmax > MAXL) return -1;
  if (((uintptr_t)qkv | (uintptr_t)out) % 16 != 0 || ((uintptr_t)cu | (uintptr_t)table) % 4 != 0) return -1;
  if ((long long)nent * H > 0x7fffffffLL) return -1;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)attn_fwd_varlen, hipFuncAttributeMaxDynamicSharedMemorySize,
                              varlen_lds(MAXL));
    attr = true;
  }
  const int l64 = (lmax + KC - 1) / KC * KC;
  hipLaunchKernelGGL(attn_fwd_varlen, dim3(nent * H), dim3(NT), varlen_lds(l64), st, (const bf16*)qkv, cu, table, nseq,
                     rows, l64, scale, H, (bf16*)out);
  return (int)hipGetLastError();
}

// ids / tts / pos_ids int32 [rows] (device); word [V, Hd], pos [P, Hd], type [TV, Hd], gamma / beta [Hd] bf16;
// x [rows, Hd] bf16, every row written (zeros where ids[t] < 0). Hd % 4 == 0, Hd <= 1024.
int mifx_bert_embed_ln_packed(const int* ids, const int* tts, const int* pos_ids, const void* word, const void* pos,
                              const void* type, const void* gamma, const void* beta, int rows, int Hd, int V, int P,
                              int TV, float eps, void* x, hipStream_t st) {
  if (rows <= 0 || Hd <= 0 || Hd % 4 != 0 || Hd > 1024 || V <= 0 || P <= 0 || TV <= 0) return -1;
  if (((uintptr_t)word | (uintptr_t)pos | (uintptr_t)type | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)x) % 8 != 0)
    return -1;
  const dim3 grid((rows + 3) / 4), block(256);
#define MIFX_EMBED(NC)                                                                                              \
  hipLaunchKernelGGL(embed_ln_packed<NC>, grid, block, 0, st, ids, tts, pos_ids, (const bf16*)word,                 \
                     (const bf16*)pos, (const bf16*)type, (const bf16*)gamma, (const bf16*)beta, rows, Hd, V, P, TV, \
                     eps, (bf16*)x)
  switch ((Hd + 255) / 256) {
    case 1: MIFX_EMBED(1); break;
    case 2: MIFX_EMBED(2); break;
    case 3: MIFX_EMBED(3); break;
    default: MIFX_EMBED(4); break;
  }
#undef MIFX_EMBED
  return (int)hipGetLastError();
}

}  // extern "C"
