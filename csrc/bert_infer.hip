// BERT inference over PACKED variable-length sequences on gfx950 (mifx/models/bert_infer.py): the activations are
// [T, hidden] with T = sum of the sequence lengths, no padding rows. Two kernels; every other op of the forward is
// token-wise and runs the training forward's kernels (csrc/fused_bert.hip at p = 0) on T rows.
//
// attn_fwd_varlen: forward-only self-attention per sequence from a cu_seqlens table; no dropout, no bias, no saved
// statistics. The structure is attn_fwd_long's (csrc/attention.hip): a workgroup of 8 waves owns 128 queries of one
// (sequence, head), that head's K and V rows are resident in LDS, keys stream in chunks of 64 with the online
// softmax, in the transposed orientation (S^T = K Q^T, O^T = V^T P^T chained, V^T by ds_read_tr16_b64). New is the
// ragged edge of a sequence of any length 1 .. 512:
//  * rows at or beyond the sequence's length L are never read from global memory (predicated, not clamped: the row
//    after the last sequence is past the allocation);
//  * the K / V staging rows L .. ceil64(L) - 1 are zero-filled (a garbage V row times P = 0 is NaN if it holds Inf);
//  * keys at or beyond L are masked by select to the running maximum's floor, -3.0e38: exp(floor - m) is exactly 0,
//    so they add nothing to l or O (every chunk holds a live key, L >= 1, so m is finite from the first chunk on);
//  * query rows at or beyond L compute on a zero Q fragment and are not stored; a wave with no live query leaves
//    after the staging barrier;
//  * the dynamic LDS is sized from the longest sequence of the launch (rounded up to 64), not from 512: a batch of
//    requests of up to 128 tokens takes 36 KB per workgroup, four workgroups per CU.
// The work list is a block table of (sequence, 128-query block) pairs, one workgroup per entry and head; entries of
// -1 exit at once, so a captured graph launches the grid of its token capacity and the host rewrites the table.
//
// embed_ln_packed: x[t] = LayerNorm(word[ids[t]] + pos[pos_id[t]] + type[tt[t]]) with explicit per-token position
// ids (they restart at 0 in every sequence): one wave per token, fp32 inside, rounded once to bf16 on the way out,
// as the fused add + LayerNorm of the training forward rounds. Tokens with id < 0 (the rows from T up to the token
// capacity) are written as zeros.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef __bf16 bf16;
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef __bf16 v4bf __attribute__((ext_vector_type(4)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef short v8s __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s lds_v4s;

constexpr int D = 64;      // head dim
constexpr int LD = D + 8;  // LDS row of a [token][d] image (elements): 144 B, as the long training kernels
constexpr int QB = 128, NT = 512, KC = 64, MAXL = 512;
constexpr float kFloor = -3.0e38f;
constexpr v4f kZero4 = {0.f, 0.f, 0.f, 0.f};

constexpr int varlen_lds(int l64) { return 2 * l64 * LD * 2; }

__device__ __forceinline__ v4s tr_read(const bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(p));
}
__device__ __forceinline__ v8bf cat8(v4s a, v4s b) {
  v8s r = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(v8bf, r);
}
__device__ __forceinline__ v8bf ld8(const bf16* p) { return *(const v8bf*)p; }
__device__ __forceinline__ v4f mfma(v8bf a, v8bf b, v4f c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ v8bf pack8(v4f a, v4f b) {
  v8bf o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[i] = (bf16)a[i];
    o[4 + i] = (bf16)b[i];
  }
  return o;
}
__device__ __forceinline__ v4bf pack4(v4f a) {
  v4bf o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (bf16)a[i];
  return o;
}

// rows 0 .. L - 1 of one [T, 3, H, 64]-strided tensor into an LDS [l64][LD] image; rows L .. l64 - 1 zero
__device__ __forceinline__ void stage_rows(bf16* dst, const bf16* src, size_t row_stride, int L, int l64) {
#pragma unroll 4
  for (int c = threadIdx.x; c < l64 * 8; c += NT) {
    const int row = c >> 3, ch = c & 7;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row < L) v = *(const uint4*)(src + (size_t)row * row_stride + ch * 8);
    *(uint4*)(dst + row * LD + ch * 8) = v;
  }
}

// rows: the row count of the qkv / out allocations; lmax64: what the dynamic LDS was sized for. A table entry whose
// sequence does not fit either is skipped (the host validates; this keeps a bad table from reading out of bounds).
__global__ __launch_bounds__(NT) void attn_fwd_varlen(const bf16* __restrict__ qkv, const int* __restrict__ cu,
                                                      const int* __restrict__ table, int nseq, int rows, int lmax64,
                                                      float scale, int H, bf16* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) bf16 smem[];
  const int ent = blockIdx.x / H, hh = blockIdx.x % H;
  const int seq = table[2 * ent], qb = table[2 * ent + 1];
  if (seq < 0 || seq >= nseq || qb < 0) return;  // padding entry (uniform over the workgroup, before any barrier)
  const int row0 = cu[seq], L = cu[seq + 1] - row0;
  const int l64 = (L + KC - 1) / KC * KC;
  if (row0 < 0 || L < 1 || L > MAXL || l64 > lmax64 || row0 + L > rows || qb * QB >= L) return;
  bf16* Ks = smem;
  bf16* Vs = smem + l64 * LD;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, h = lane >> 4, q = r >> 2, p = r & 3;
  const size_t tok = (size_t)3 * H * D;
  const bf16* base = qkv + (size_t)row0 * tok;
  stage_rows(Ks, base + (size_t)(H + hh) * D, tok, L, l64);
  stage_rows(Vs, base + (size_t)(2 * H + hh) * D, tok, L, l64);
  const bool live = qb * QB + 16 * w < L;
  const int qi = qb * QB + 16 * w + r;
  const bool qlive = qi < L;
  v8bf qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const v8s z = {0, 0, 0, 0, 0, 0, 0, 0};
    qf[ks] = __builtin_bit_cast(v8bf, z);
    if (qlive) qf[ks] = ld8(base + (size_t)qi * tok + (size_t)hh * D + 32 * ks + 8 * h);
  }
  __syncthreads();
  if (!live) return;  // no barrier follows

  float m = kFloor, l = 0.f;
  v4f o[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) o[dt] = kZero4;
  for (int c = 0; c < l64; c += KC) {
    v4f s[KC / 16];
    float mc = m;
#pragma unroll
    for (int kt = 0; kt < KC / 16; ++kt) {
      v4f a = kZero4;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) a = mfma(ld8(Ks + (c + 16 * kt + r) * LD + 32 * ks + 8 * h), qf[ks], a);
      const int k0 = c + 16 * kt + 4 * h;  // the lane's 4 keys of this tile
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = k0 + e < L ? a[e] * scale : kFloor;
      mc = fmaxf(mc, fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])));
      s[kt] = a;
    }
    mc = fmaxf(mc, __shfl_xor(mc, 16));
    mc = fmaxf(mc, __shfl_xor(mc, 32));
    const float alpha = __expf(m - mc);
    m = mc;
    l *= alpha;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) o[dt] *= alpha;
#pragma unroll
    for (int kt = 0; kt < KC / 16; ++kt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pe = __expf(s[kt][e] - m);
        l += pe;
        s[kt][e] = pe;
      }
    const v8bf pb[2] = {pack8(s[0], s[1]), pack8(s[2], s[3])};
    // O^T += V^T P^T over this chunk (V rows read transposed at the chained key order)
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16* pa = Vs + (c + 32 * ks + 4 * h + q) * LD + 16 * dt + 4 * p;
        o[dt] = mfma(cat8(tr_read(pa), tr_read(pa + 16 * LD)), pb[ks], o[dt]);
      }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (!qlive) return;
  const float inv = 1.f / l;
  bf16* dst = out + (size_t)(row0 + qi) * H * D + (size_t)hh * D + 4 * h;
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) *(v4bf*)(dst + 16 * dt) = pack4(o[dt] * inv);
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
