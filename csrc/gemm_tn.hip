// Hand-written bf16 MFMA "TN" GEMM for gfx950: C[M, N] = A[T, M]^T . B[T, N] -- the weight gradient of a linear layer,
// dW = dY^T X, with the token dimension T (the reduction) as the row index of BOTH operands.
//
// BASELINE config 4 (BERT-base, 4096 tokens): the four weight-gradient GEMMs of a layer (QKV 2304x768, attention-out
// 768x768, FFN-in 3072x768, FFN-out 768x3072, all with K = 4096 tokens) were hipBLASLt's slowest products in the
// training step: 144-216 workgroups of 128x128 / 64x64 tiles on 256 CUs (one K-reduction per tile, no split), 30-46 us
// each, 160-420 TFLOP/s (profiles/archive/bert_steady_kernels_r3.md). Here every shape gets a whole wave of workgroups: the
// 96 x 96 tile puts 3072 x 768 (and 768 x 3072) on exactly 256 workgroups, and small outputs split the token range
// over gridDim.y with an fp32 partial per split, summed in split order by a second kernel (deterministic).
//
// Structure:
//  * 4 waves (2 x 2), each owning a (BM/2) x (BN/2) block of 16 x 16 MFMA tiles (mfma_f32_16x16x32_bf16);
//  * per 64-token K-tile every lane issues 16-byte global->LDS DMA loads (no VGPR round trip) of A rows [64][BM] and
//    B rows [64][BN] into a ring of NS buffers (~144 KB), NS - 1 tiles ahead of the MFMAs; one barrier per K-tile;
//  * both operands sit in LDS as the token-major rotated image of csrc/tile_index.h, so the MFMA fragments (8
//    consecutive tokens per lane) are pairs of ds_read_b64_tr_b16 transposed reads, conflict-free for every tile width
//    here (tests/test_tile_index.py);
//  * the MFMA takes the B fragment as its A operand, so the accumulator lane holds C[m][n .. n + 3]: 8-byte bf16
//    stores (or 16-byte fp32 partial stores) in the epilogue;
//  * XCD-aware tile order (xcd_tile, then grouped_tile of csrc/tile_index.h): each XCD walks a contiguous run of
//    tiles, grouped 4 m-blocks wide, so it re-reads few A and B strips per K-tile from its own L2.
#include "mfma_stage.h"

namespace {

constexpr int BK = 64;

// OUT_F32: store the fp32 partial of split blockIdx.y at P + blockIdx.y * M * N (else bf16 C directly).
// OPT bit 0: raise the wave priority around each MFMA block (bit 1 in the config table: the 8-wave gemm_tn_k2).
template <int BM, int BN, bool OUT_F32, int OPT, int NS>
__global__ __launch_bounds__(256) void gemm_tn(const bf16* __restrict__ A, const bf16* __restrict__ B,
                                                  bf16* __restrict__ C, float* __restrict__ P, int M, int N, int T,
                                                  int tps) {
  constexpr int NT = 256, WM = 2, WN = 2;
  constexpr int TM = BM / WM, TN = BN / WN, MR = TM / 16, NR = TN / 16;
  constexpr int CPA = BM / 8, CPB = BN / 8;  // 16-byte chunks per token row
  constexpr int AR = (BK * CPA + NT - 1) / NT, BR = (BK * CPB + NT - 1) / NT;  // DMA rounds per K-tile
  constexpr int ABYTES = BK * BM * 2, BBYTES = BK * BN * 2, BUF = ABYTES + BBYTES;
  static_assert(TM % 16 == 0 && TN % 16 == 0, "wave tiling");
  static_assert((BK * CPA) % NT == 0 && (BK * CPB) % NT == 0, "whole DMA rounds (counted waits)");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int wm = w / WN, wn = w % WN;
  const TileMN tl = grouped_tile(xcd_tile(blockIdx.x, gridDim.x), M / BM, N / BN);
  const int m0 = tl.m * BM, n0 = tl.n * BN;
  const int t_begin = blockIdx.y * tps, KT = tps / BK;

  // per-lane DMA source offsets (elements, relative to the K-tile's first token row)
  int aoff[AR], boff[BR];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    const int s = min(i * NT + tid, BK * CPA - 1);
    aoff[i] = tok_img_src<CPA>(s / CPA, s % CPA, M, m0);
  }
#pragma unroll
  for (int i = 0; i < BR; ++i) {
    const int s = min(i * NT + tid, BK * CPB - 1);
    boff[i] = tok_img_src<CPB>(s / CPB, s % CPB, N, n0);
  }
  auto issue = [&](int kt, int buf) {
    unsigned char* ba = lds + buf * BUF;
    unsigned char* bb = ba + ABYTES;
    const size_t t0 = (size_t)(t_begin + kt * BK);
    const bf16* a0 = A + t0 * M;
    const bf16* b0 = B + t0 * N;
#pragma unroll
    for (int i = 0; i < AR; ++i)
      if ((BK * CPA) % NT == 0 || i * NT + 64 * w < BK * CPA) glds16(a0 + aoff[i], ba + (i * NT + 64 * w) * 16);
#pragma unroll
    for (int i = 0; i < BR; ++i)
      if ((BK * CPB) % NT == 0 || i * NT + 64 * w < BK * CPB) glds16(b0 + boff[i], bb + (i * NT + 64 * w) * 16);
  };

  v4f acc[MR][NR];
#pragma unroll
  for (int a = 0; a < MR; ++a)
#pragma unroll
    for (int b = 0; b < NR; ++b) acc[a][b] = (v4f){0.f, 0.f, 0.f, 0.f};

  // fragment read geometry: lane (r, h), r = lane & 15 -> (row quad q = r >> 2, column quad p = r & 3)
  const int r = lane & 15, h = lane >> 4, q = r >> 2, p = r & 3;
  auto read_frags = [&](const unsigned char* ba, const unsigned char* bb, int ks, v8bf (&af)[MR], v8bf (&bf)[NR]) {
    const int t1 = 32 * ks + 8 * h + q;
#pragma unroll
    for (int a = 0; a < MR; ++a) af[a] = tok_frag<CPA>(ba, t1, (wm * TM + 16 * a) / 8, p);
#pragma unroll
    for (int b = 0; b < NR; ++b) bf[b] = tok_frag<CPB>(bb, t1, (wn * TN + 16 * b) / 8, p);
  };

  // NS-buffer ring (mfma_stage.h; one K-tile's MFMAs here take ~300 cycles), G DMAs per thread per tile
  constexpr int G = AR + BR;
#pragma unroll
  for (int i = 0; i < NS - 1; ++i)
    if (i < KT) issue(i, i);
  for (int kt = 0; kt < KT; ++kt) {
    const unsigned char* ba = lds + ring_next<NS, G>(kt, KT, issue) * BUF;
    const unsigned char* bb = ba + ABYTES;
    v8bf af0[MR], bf0[NR], af1[MR], bf1[NR];
    read_frags(ba, bb, 0, af0, bf0);
    read_frags(ba, bb, 1, af1, bf1);
    if (OPT & 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int a = 0; a < MR; ++a)
#pragma unroll
      for (int b = 0; b < NR; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf0[b], af0[a], acc[a][b], 0, 0, 0);
#pragma unroll
    for (int a = 0; a < MR; ++a)
#pragma unroll
      for (int b = 0; b < NR; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf1[b], af1[a], acc[a][b], 0, 0, 0);
    if (OPT & 1) __builtin_amdgcn_s_setprio(0);
  }

  // ---- epilogue: lane (r, h) holds C[m0 + wm TM + 16 a + r][n0 + wn TN + 16 b + 4 h + 0..3]
#pragma unroll
  for (int a = 0; a < MR; ++a) {
    const int m = m0 + wm * TM + 16 * a + r;
#pragma unroll
    for (int b = 0; b < NR; ++b) {
      const int n = n0 + wn * TN + 16 * b + 4 * h;
      if constexpr (OUT_F32) {
        *(v4f*)(P + (size_t)blockIdx.y * M * N + (size_t)m * N + n) = acc[a][b];
      } else {
        v4bf o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (bf16)acc[a][b][i];
        *(v4bf*)(C + (size_t)m * N + n) = o;
      }
    }
  }
}

// Measured (profiles/archive/gemm_tn_r3b_k2.jsonl): 50 us on FFN-in's dW at S = 1 against 54 for the 4-wave deep ring and
// 38 for two 4-wave workgroups per CU with a 2-way token split -- two independent barrier pipelines per CU beat one
// 8-wave pipeline, so the tuned table keeps the split; this form stays selectable (config 18).
// 8-wave form of the 96 x 96 tile (one workgroup per CU, two waves per SIMD, no token split across workgroups):
// waves w and w + 4 own the same 48 x 48 quadrant and take the two 32-token k-steps of every K-tile, so each SIMD
// runs two independent MFMA chains (the one-wave-per-SIMD 4-wave form idles at every barrier and fragment read);
// the k-step-1 waves hand their accumulators to the k-step-0 waves through LDS at the end (fixed order: k-step 0
// + k-step 1). DMA: each K-tile's 12 + 12 wave-instructions are dealt 2 + 1 / 1 + 2 to waves 0-3 / 4-7 (3 each, so
// the counted vmcnt is the same for every wave).
template <bool OUT_F32, int NS>
__global__ __launch_bounds__(512) void gemm_tn_k2(const bf16* __restrict__ A, const bf16* __restrict__ B,
                                                 bf16* __restrict__ C, float* __restrict__ P, int M, int N, int T,
                                                 int tps) {
  constexpr int BM = 96, BN = 96, TM = 48, TN = 48, MR = 3, NR = 3, CPA = 12, CPB = 12;
  constexpr int ABYTES = BK * BM * 2, BBYTES = BK * BN * 2, BUF = ABYTES + BBYTES;
  constexpr int G = 3;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int qd = w & 3, kg = w >> 2, wm = qd >> 1, wn = qd & 1;
  const TileMN tl = grouped_tile(xcd_tile(blockIdx.x, gridDim.x), M / BM, N / BN);
  const int m0 = tl.m * BM, n0 = tl.n * BN;
  const int t_begin = blockIdx.y * tps, KT = tps / BK;
  // this wave's 3 DMA wave-instructions: (operand, instruction index) -> LDS slots [64 i, 64 i + 64)
  int doff[G], dslot[G];
  bool dis_a[G];
#pragma unroll
  for (int j = 0; j < G; ++j) {
    // waves 0-3: A {w, w + 8}, B {w + 4}; waves 4-7: A {w}, B {w - 4, w + 4}
    const bool isa = kg == 0 ? j < 2 : j == 0;
    const int i = isa ? w + 8 * j : (kg == 0 ? w + 4 : (w - 4) + 8 * (j - 1));
    const int sl = 64 * i + lane, t = sl / 12, pp = sl % 12;
    dis_a[j] = isa;
    dslot[j] = 64 * i;
    int c = pp - rot<12>(t);  // (tok_img_src by hand: through the helper this kernel compiles to different code)
    c = c < 0 ? c + 12 : c;
    doff[j] = isa ? t * M + m0 + 8 * c : t * N + n0 + 8 * c;
  }
  auto issue = [&](int kt, int buf) {
    unsigned char* ba = lds + buf * BUF;
    const size_t t0 = (size_t)(t_begin + kt * BK);
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const bf16* src = dis_a[j] ? A + t0 * M + doff[j] : B + t0 * N + doff[j];
      unsigned char* dst = dis_a[j] ? ba + dslot[j] * 16 : ba + ABYTES + dslot[j] * 16;
      glds16(src, dst);
    }
  };
  v4f acc[MR][NR];
#pragma unroll
  for (int a = 0; a < MR; ++a)
#pragma unroll
    for (int b = 0; b < NR; ++b) acc[a][b] = (v4f){0.f, 0.f, 0.f, 0.f};
  const int r = lane & 15, h = lane >> 4, q = r >> 2, p = r & 3;
  const int t1 = 32 * kg + 8 * h + q, t2 = t1 + 4;  // (k-step kg of every K-tile)
  int ao1[MR], ao2[MR], bo1[NR], bo2[NR];  // byte offsets of this lane's fragment reads inside a buffer
#pragma unroll
  for (int a = 0; a < MR; ++a) {
    const int c = (wm * TM + 16 * a) / 8 + (p >> 1);
    ao1[a] = tok_frag_off<CPA>(t1, c, p);
    ao2[a] = tok_frag_off<CPA>(t2, c, p);
  }
#pragma unroll
  for (int b = 0; b < NR; ++b) {
    const int c = (wn * TN + 16 * b) / 8 + (p >> 1);
    bo1[b] = ABYTES + tok_frag_off<CPB>(t1, c, p);
    bo2[b] = ABYTES + tok_frag_off<CPB>(t2, c, p);
  }
#pragma unroll
  for (int i = 0; i < NS - 1; ++i)
    if (i < KT) issue(i, i);
  for (int kt = 0; kt < KT; ++kt) {
    const unsigned char* bf = lds + ring_next<NS, G>(kt, KT, issue) * BUF;
    v8bf af[MR], bfr[NR];
#pragma unroll
    for (int a = 0; a < MR; ++a) af[a] = cat8(tr_read(bf + ao1[a]), tr_read(bf + ao2[a]));
#pragma unroll
    for (int b = 0; b < NR; ++b) bfr[b] = cat8(tr_read(bf + bo1[b]), tr_read(bf + bo2[b]));
#pragma unroll
    for (int a = 0; a < MR; ++a)
#pragma unroll
      for (int b = 0; b < NR; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[b], af[a], acc[a][b], 0, 0, 0);
  }
  // k-step-1 waves -> LDS -> k-step-0 waves add (every buffer is free once all waves passed this barrier)
  __syncthreads();
  v4f* red = (v4f*)lds;
  if (kg == 1) {
#pragma unroll
    for (int a = 0; a < MR; ++a)
#pragma unroll
      for (int b = 0; b < NR; ++b) red[((qd * MR + a) * NR + b) * 64 + lane] = acc[a][b];
  }
  __syncthreads();
  if (kg == 1) return;
#pragma unroll
  for (int a = 0; a < MR; ++a) {
    const int m = m0 + wm * TM + 16 * a + r;
#pragma unroll
    for (int b = 0; b < NR; ++b) {
      const v4f o4 = acc[a][b] + red[((qd * MR + a) * NR + b) * 64 + lane];
      const int n = n0 + wn * TN + 16 * b + 4 * h;
      if constexpr (OUT_F32) {
        *(v4f*)(P + (size_t)blockIdx.y * M * N + (size_t)m * N + n) = o4;
      } else {
        v4bf o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (bf16)o4[i];
        *(v4bf*)(C + (size_t)m * N + n) = o;
      }
    }
  }
}

// C = bf16(sum over s of P[s]) in split order; 8 elements per thread
__global__ __launch_bounds__(256) void splits_sum(const float4* __restrict__ P, int S, long long n8, v8bf* __restrict__ C) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float4 lo = P[2 * i], hi = P[2 * i + 1];
  for (int s = 1; s < S; ++s) {
    const float4 a = P[(size_t)s * 2 * n8 + 2 * i], b = P[(size_t)s * 2 * n8 + 2 * i + 1];
    lo.x += a.x; lo.y += a.y; lo.z += a.z; lo.w += a.w;
    hi.x += b.x; hi.y += b.y; hi.z += b.z; hi.w += b.w;
  }
  C[i] = v8bf{(bf16)lo.x, (bf16)lo.y, (bf16)lo.z, (bf16)lo.w, (bf16)hi.x, (bf16)hi.y, (bf16)hi.z, (bf16)hi.w};
}

// NS0 = 0: the deepest ring within ~144 KB of LDS (one workgroup per CU); else NS0 buffers (smaller rings let 2-3
// workgroups share a CU)
template <int BM, int BN, bool OUT_F32, int OPT, int NS0>
int launch(const void* A, const void* B, void* C, float* P, int M, int N, int T, int S, hipStream_t st) {
  constexpr int BUF = (BM + BN) * BK * 2;
  constexpr int NS = NS0 ? NS0 : ((147456 / BUF) < 8 ? (147456 / BUF) : 8);
  constexpr int LDS = NS * BUF;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)gemm_tn<BM, BN, OUT_F32, OPT, NS>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    attr = true;
  }
  hipLaunchKernelGGL((gemm_tn<BM, BN, OUT_F32, OPT, NS>), dim3((M / BM) * (N / BN), S), dim3(256), LDS, st,
                     (const bf16*)A, (const bf16*)B, (bf16*)C, P, M, N, T, T / S);
  return (int)hipGetLastError();
}

template <bool OUT_F32>
int launch_k2(const void* A, const void* B, void* C, float* P, int M, int N, int T, int S, hipStream_t st) {
  constexpr int BUF = 2 * 96 * BK * 2, NS = 6, LDS = NS * BUF;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)gemm_tn_k2<OUT_F32, NS>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    attr = true;
  }
  hipLaunchKernelGGL((gemm_tn_k2<OUT_F32, NS>), dim3((M / 96) * (N / 96), S), dim3(512), LDS, st, (const bf16*)A,
                     (const bf16*)B, (bf16*)C, P, M, N, T, T / S);
  return (int)hipGetLastError();
}

int dispatch_k2(const void* A, const void* B, void* C, float* P, int M, int N, int T, int S, hipStream_t st) {
  if (S == 1) return launch_k2<false>(A, B, C, nullptr, M, N, T, 1, st);
  const int rc = launch_k2<true>(A, B, nullptr, P, M, N, T, S, st);
  if (rc != 0) return rc;
  const long long n8 = (long long)M * N / 8;
  hipLaunchKernelGGL(splits_sum, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, (const float4*)P, S, n8,
                     (v8bf*)C);
  return (int)hipGetLastError();
}

// (index = the `cfg` argument) BM x BN tile, OPT bits, ring depth NS0 (0: the deepest that fits). Written once: the
// table mifx_gemm_tn_configs reports and the dispatch both expand this list. OPT bit 1 is the 8-wave gemm_tn_k2,
// which exists for this one tile and depth only.
#define TN_CONFIGS(X)                                                                                            \
  X(96, 96, 0, 0) X(96, 96, 1, 0) X(128, 128, 0, 0) X(128, 96, 0, 0) X(96, 128, 0, 0) X(64, 64, 0, 0)            \
  X(128, 64, 0, 0) X(64, 128, 0, 0) X(96, 96, 0, 3) X(96, 96, 0, 2) X(128, 128, 0, 2) X(128, 128, 0, 3)          \
  X(64, 64, 0, 3) X(128, 64, 0, 3) X(64, 128, 0, 3) X(192, 192, 0, 3) X(192, 96, 0, 3) X(96, 192, 0, 3)          \
  X(96, 96, 2, 6) X(96, 96, 1, 2) X(128, 128, 1, 2)
struct Cfg {
  int bm, bn, opt, ns;
};
#define X(bm, bn, opt, ns) {bm, bn, opt, ns},
constexpr Cfg kCfgs[] = {TN_CONFIGS(X)};
#undef X

template <int BM, int BN, int OPT, int NS0>
int dispatch(const void* A, const void* B, void* C, float* P, int M, int N, int T, int S, hipStream_t st) {
  if constexpr (OPT & 2) {  // 8 waves, k-steps split over wave pairs
    static_assert(BM == 96 && BN == 96 && NS0 == 6, "gemm_tn_k2's tile and ring depth");
    return dispatch_k2(A, B, C, P, M, N, T, S, st);
  } else {
    if (S == 1) return launch<BM, BN, false, OPT, NS0>(A, B, C, nullptr, M, N, T, 1, st);
    const int rc = launch<BM, BN, true, OPT, NS0>(A, B, nullptr, P, M, N, T, S, st);
    if (rc != 0) return rc;
    const long long n8 = (long long)M * N / 8;
    hipLaunchKernelGGL(splits_sum, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, (const float4*)P, S, n8,
                       (v8bf*)C);
    return (int)hipGetLastError();
  }
}

}  // namespace

extern "C" {

// tile configurations: out[3 i] = BM, out[3 i + 1] = BN, out[3 i + 2] = OPT bits + 16 x ring depth (0: deepest)
int mifx_gemm_tn_configs(int* out, int n) {
  const int m = (int)(sizeof(kCfgs) / sizeof(Cfg));
  for (int i = 0; i < m && 3 * i + 2 < n; ++i) {
    out[3 * i] = kCfgs[i].bm;
    out[3 * i + 1] = kCfgs[i].bn;
    out[3 * i + 2] = kCfgs[i].opt + 16 * kCfgs[i].ns;
  }
  return m;
}

// C[M, N] (bf16) = A[T, M]^T . B[T, N] (bf16, row-major, fp32 accumulation). S > 1 splits T over S workgroup rows
// with fp32 partials P [S, M, N] summed in split order. Requires M % BM == 0, N % BN == 0, T % (64 S) == 0,
// 16-byte aligned rows (M % 8 == 0, N % 8 == 0 follow).
int mifx_gemm_tn(int cfg, const void* A, const void* B, void* C, float* P, int M, int N, int T, int S,
                 hipStream_t st) {
  const int m = (int)(sizeof(kCfgs) / sizeof(Cfg));
  if (cfg < 0 || cfg >= m || M <= 0 || N <= 0 || T <= 0 || S <= 0 || A == nullptr || B == nullptr || C == nullptr)
    return -1;
  const Cfg c = kCfgs[cfg];
  if (M % c.bm || N % c.bn || T % (BK * S)) return -1;
  if (S > 1 && P == nullptr) return -1;
  if ((uintptr_t)A % 16 || (uintptr_t)B % 16 || (uintptr_t)C % 16 || (P != nullptr && (uintptr_t)P % 16)) return -1;
  if ((long long)T * M >= (1ll << 31) || (long long)T * N >= (1ll << 31)) return -1;  // 32-bit element offsets
  int i = 0;
#define X(bm, bn, opt, ns) \
  if (cfg == i++) return dispatch<bm, bn, opt, ns>(A, B, C, P, M, N, T, S, st);
  TN_CONFIGS(X)
#undef X
  return -1;
}

}  // extern "C"
