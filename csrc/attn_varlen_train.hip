// Self-attention for TRAINING over PACKED variable-length sequences on gfx950 (mifx/ops/attn_varlen.py): forward with
// attention-probability dropout and saved softmax statistics, and the two-kernel backward. The layout is the packed
// inference kernel's (csrc/bert_infer.hip): qkv [rows, 3, H, 64], out / dout [rows, H, 64] with `rows` the token
// capacity of the buffers, a cu_seqlens table (sequence b owns rows cu[b] .. cu[b + 1] - 1, 1 .. 512 of them) and a
// block table of (sequence, 128-row block) pairs, one workgroup per entry and head; entries of -1 exit at once, so
// a captured step launches the grid of its capacity and the host rewrites the tables between replays.
//
// The three kernels are the chunked bodies of csrc/attn_chunked.h over its Packed geometry; the rules of the ragged
// edge, the statistics' layout and the dropout index are given there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_chunked.h"

namespace {

constexpr int kv_lds(int l64) { return 2 * l64 * LD * 2; }
constexpr int dkv_lds(int l64) { return 2 * l64 * LD * 2 + 3 * l64 * 4; }  // + m, log2 l, D of every query row
static_assert(dkv_lds(MAXL) <= 160 * 1024, "Q, dO and the statistics of 512 rows must fit the LDS");

__global__ __launch_bounds__(NT) void attn_fwd_varlen_train(const bf16* __restrict__ qkv, const int* __restrict__ cu,
                                                            const int* __restrict__ table, int nseq, int rows,
                                                            int lmax64, float scale, Drop dp, int H, int h0,
                                                            bf16* __restrict__ out, float* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) bf16 smem[];
  chunked_fwd<Packed, true>(Packed(cu, table, nseq, rows, lmax64, H, h0), smem, qkv, scale, dp, H, out, stats);
}

__global__ __launch_bounds__(NT) void attn_bwd_dq_varlen(const bf16* __restrict__ qkv, const int* __restrict__ cu,
                                                         const int* __restrict__ table, int nseq, int rows, int lmax64,
                                                         const bf16* __restrict__ o, const bf16* __restrict__ dout,
                                                         const float* __restrict__ stats, float scale, Drop dp, int H,
                                                         int h0, bf16* __restrict__ dqkv, float* __restrict__ dsum) {
  extern __shared__ __attribute__((aligned(16))) bf16 smem[];
  chunked_bwd_dq(Packed(cu, table, nseq, rows, lmax64, H, h0), smem, qkv, o, dout, stats, scale, dp, H, dqkv, dsum);
}

__global__ __launch_bounds__(NT) void attn_bwd_dkv_varlen(const bf16* __restrict__ qkv, const int* __restrict__ cu,
                                                          const int* __restrict__ table, int nseq, int rows,
                                                          int lmax64, const bf16* __restrict__ dout,
                                                          const float* __restrict__ stats,
                                                          const float* __restrict__ dsum, float scale, Drop dp, int H,
                                                          int h0, bf16* __restrict__ dqkv) {
  extern __shared__ __attribute__((aligned(16))) bf16 smem[];
  chunked_bwd_dkv(Packed(cu, table, nseq, rows, lmax64, H, h0), smem, qkv, dout, stats, dsum, scale, dp, H, dqkv);
}

bool bad_common(int nseq, int nent, int rows, int lmax, int H, int h0, float p, const int64_t* rng) {
  if (nseq <= 0 || nent <= 0 || rows <= 0 || H <= 0 || h0 < 0 || lmax < 1 || lmax > MAXL) return true;
  if ((long long)nent * H > 0x7fffffffLL) return true;
  return !(p >= 0.f) || p >= 1.f || (p > 0.f && rng == nullptr);
}

}  // namespace

extern "C" {

// qkv [rows, 3, H, 64] bf16 (contiguous), cu int32 [nseq + 1], table int32 [nent, 2] (device), out [rows, H, 64]
// bf16 and stats fp32 [2, H, rows] (rows of no sequence are left untouched). lmax: an upper bound of the longest
// sequence of this launch (the dynamic LDS is sized from it; a longer sequence in the table is skipped). p: attention
// dropout (rng: device int64 [seed, counter]); h0: this rank's first global head (dropout indexing only).
int mifx_attn_fwd_varlen_train(const void* qkv, const int* cu, const int* table, int nseq, int nent, int rows, int lmax,
                               int H, int h0, float scale, float p, const int64_t* rng, int site, void* out,
                               float* stats, hipStream_t st) {
  if (bad_common(nseq, nent, rows, lmax, H, h0, p, rng)) return -1;
  if (((uintptr_t)qkv | (uintptr_t)out) % 16 != 0 || ((uintptr_t)cu | (uintptr_t)table | (uintptr_t)stats) % 4 != 0)
    return -1;
  if (!qkv || !cu || !table || !out || !stats) return -1;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)attn_fwd_varlen_train, hipFuncAttributeMaxDynamicSharedMemorySize,
                              kv_lds(MAXL));
    attr = true;
  }
  const Drop dp{rng, site, drop_threshold(p), 1.f / (1.f - p)};
  const int l64 = (lmax + KC - 1) / KC * KC;
  hipLaunchKernelGGL(attn_fwd_varlen_train, dim3(nent * H), dim3(NT), kv_lds(l64), st, (const bf16*)qkv, cu, table,
                     nseq, rows, l64, scale, dp, H, h0, (bf16*)out, stats);
  return (int)hipGetLastError();
}

// out / dout [rows, H, 64] bf16, stats: the forward's; dqkv [rows, 3, H, 64] bf16 (rows of a listed sequence are
// written, every element once; the others are left as they are: hand it over zeroed); dsum fp32 [H, rows] workspace.
int mifx_attn_bwd_varlen(const void* qkv, const int* cu, const int* table, int nseq, int nent, int rows, int lmax,
                         int H, int h0, float scale, float p, const int64_t* rng, int site, const void* out,
                         const void* dout, const float* stats, void* dqkv, float* dsum, hipStream_t st) {
  if (bad_common(nseq, nent, rows, lmax, H, h0, p, rng)) return -1;
  if (((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)dqkv) % 16 != 0 ||
      ((uintptr_t)cu | (uintptr_t)table | (uintptr_t)stats | (uintptr_t)dsum) % 4 != 0)
    return -1;
  if (!qkv || !cu || !table || !out || !dout || !stats || !dqkv || !dsum) return -1;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)attn_bwd_dq_varlen, hipFuncAttributeMaxDynamicSharedMemorySize,
                              kv_lds(MAXL));
    (void)hipFuncSetAttribute((const void*)attn_bwd_dkv_varlen, hipFuncAttributeMaxDynamicSharedMemorySize,
                              dkv_lds(MAXL));
    attr = true;
  }
  const Drop dp{rng, site, drop_threshold(p), 1.f / (1.f - p)};
  const int l64 = (lmax + KC - 1) / KC * KC;
  hipLaunchKernelGGL(attn_bwd_dq_varlen, dim3(nent * H), dim3(NT), kv_lds(l64), st, (const bf16*)qkv, cu, table, nseq,
                     rows, l64, (const bf16*)out, (const bf16*)dout, stats, scale, dp, H, h0, (bf16*)dqkv, dsum);
  hipLaunchKernelGGL(attn_bwd_dkv_varlen, dim3(nent * H), dim3(NT), dkv_lds(l64), st, (const bf16*)qkv, cu, table,
                     nseq, rows, l64, (const bf16*)dout, (const float*)stats, (const float*)dsum, scale, dp, H, h0,
                     (bf16*)dqkv);
  return (int)hipGetLastError();
}

}  // extern "C"
