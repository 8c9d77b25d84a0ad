// Self-attention for TRAINING over PACKED variable-length sequences on gfx950 (mifx/ops/attn_varlen.py): forward with
// attention-probability dropout and saved softmax statistics, and the two-kernel backward. The layout is the packed
// inference kernel's (csrc/bert_infer.hip): qkv [rows, 3, H, 64], out / dout [rows, H, 64] with `rows` the token
// capacity of the buffers, a cu_seqlens table (sequence b owns rows cu[b] .. cu[b + 1] - 1, 1 .. 512 of them) and a
// block table of (sequence, 128-row block) pairs, one workgroup per entry and head; entries of -1 exit at once, so
// a captured step launches the grid of its capacity and the host rewrites the tables between replays.
//
//  * attn_fwd_varlen_train: attn_fwd_varlen (ragged edge by predicated loads, zero-filled K / V staging rows, dead
//    keys selected to the running maximum's floor) plus attn_fwd_long's dropout (csrc/attention.hip: keep4 per 4-key
//    group, output scaled by 1 / (1 - p)) and the statistics of every live query row, fp32 [2, H, rows]: the row
//    maximum m, then log2 of the row sum l, indexed by packed row.
//  * attn_bwd_dq_varlen: attn_bwd_dq_long per (sequence, 128-query block, head); writes dq of its live rows and
//    dsum [H, rows] = rowsum(dO o O). A dead key (j >= L) has a zero K row, score 0, and exp2((0 - m) log2e - log2 l)
//    is not 0 (it overflows for a very negative m, and inf * 0 through the zero K row is NaN): P is selected to 0.
//  * attn_bwd_dkv_varlen: attn_bwd_dkv_long per (sequence, 128-key block, head), Q and dO staged zero-filled; writes
//    dk and dv of its live key rows. The statistics m, log2 l and D of the sequence's query rows are staged in LDS
//    beside Q and dO by predicated per-row loads (their packed rows cu[b] + i have no alignment and the last group of
//    4 runs into the next sequence, so the long kernel's float4 global loads do not carry over); P_d and dS of a dead
//    query (i >= L) are selected to 0, its statistics never read.
//
// No row at or beyond a sequence's length is read from global memory (qkv, out, dout, statistics, dsum), and none is
// written: every element of dqkv on a row owned by a sequence is written exactly once (dq by the dq kernel, dk and dv
// by the dkv kernel), rows owned by no sequence are not touched (the caller hands dqkv over zeroed). Dead query and
// key lanes compute on zero fragments; a wave with no live row leaves after the staging barrier, which is the last.
// A table entry whose sequence does not fit (L > lmax, row0 + L > rows, ...) is skipped, not trusted.
//
// Dropout: element (global head g = h0 + h, packed query row t = cu[b] + i, key j inside its sequence) takes the
// keep bit of csrc/counter_rng.h at the flat index
//
//     (g * rows + t) * 512 + j
//
// which does not depend on the head split nor on how the sequences of other packs of the same capacity are ordered,
// and is a multiple of 4 wherever j is (the 4-key groups of keep4 stay aligned). Host twin:
// mifx.ops.fused_bert.keep_mask.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "counter_rng.h"

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
constexpr float kLog2e = 1.4426950408889634f;
constexpr v4f kZero4 = {0.f, 0.f, 0.f, 0.f};

constexpr int kv_lds(int l64) { return 2 * l64 * LD * 2; }
constexpr int dkv_lds(int l64) { return 2 * l64 * LD * 2 + 3 * l64 * 4; }  // + m, log2 l, D of every query row
static_assert(dkv_lds(MAXL) <= 160 * 1024, "Q, dO and the statistics of 512 rows must fit the LDS");

__device__ __forceinline__ v4s tr_read(const bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(p));
}
__device__ __forceinline__ v8bf cat8(v4s a, v4s b) {
  v8s r = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(v8bf, r);
}
__device__ __forceinline__ v8bf ld8(const bf16* p) { return *(const v8bf*)p; }
__device__ __forceinline__ v8bf zero8() {
  const v8s z = {0, 0, 0, 0, 0, 0, 0, 0};
  return __builtin_bit_cast(v8bf, z);
}
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
__device__ __forceinline__ float prob(float sm, float l2) { return __builtin_amdgcn_exp2f(fmaf(sm, kLog2e, -l2)); }

struct Drop {
  const int64_t* rng;
  int site;
  uint32_t thr;  // 0: no dropout
  float scale;   // 1 / (1 - p)
};

// what every kernel needs of its table entry; ok false: a padding entry, or a sequence that does not fit
struct Seq {
  int row0, L, l64, blk;
  bool ok;
};

__device__ __forceinline__ Seq entry(const int* cu, const int* table, int ent, int nseq, int rows, int lmax64) {
  Seq s = {0, 0, 0, 0, false};
  const int seq = table[2 * ent];
  s.blk = table[2 * ent + 1];
  if (seq < 0 || seq >= nseq || s.blk < 0) return s;
  s.row0 = cu[seq];
  s.L = cu[seq + 1] - s.row0;
  s.l64 = (s.L + KC - 1) / KC * KC;
  s.ok = s.row0 >= 0 && s.L >= 1 && s.L <= MAXL && s.l64 <= lmax64 && s.row0 <= rows - s.L && s.blk * QB < s.L;
  return s;
}

// rows 0 .. L - 1 of one strided tensor into an LDS [l64][LD] image; rows L .. l64 - 1 zero
__device__ __forceinline__ void stage_rows(bf16* dst, const bf16* src, size_t row_stride, int L, int l64) {
#pragma unroll 4
  for (int c = threadIdx.x; c < l64 * 8; c += NT) {
    const int row = c >> 3, ch = c & 7;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row < L) v = *(const uint4*)(src + (size_t)row * row_stride + ch * 8);
    *(uint4*)(dst + row * LD + ch * 8) = v;
  }
}

__global__ __launch_bounds__(NT) void attn_fwd_varlen_train(const bf16* __restrict__ qkv, const int* __restrict__ cu,
                                                            const int* __restrict__ table, int nseq, int rows,
                                                            int lmax64, float scale, Drop dp, int H, int h0,
                                                            bf16* __restrict__ out, float* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) bf16 smem[];
  const int ent = blockIdx.x / H, hh = blockIdx.x % H;
  const Seq sq = entry(cu, table, ent, nseq, rows, lmax64);
  if (!sq.ok) return;  // uniform over the workgroup, before any barrier
  const int row0 = sq.row0, L = sq.L, l64 = sq.l64, qb = sq.blk;
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
    qf[ks] = zero8();
    if (qlive) qf[ks] = ld8(base + (size_t)qi * tok + (size_t)hh * D + 32 * ks + 8 * h);
  }
  __syncthreads();
  if (!live) return;  // no barrier follows

  const uint64_t key = dp.thr ? mifx_rng::drop_key(dp.rng, dp.site) : 0;
  const uint64_t row_base = ((uint64_t)(h0 + hh) * rows + row0 + qi) * MAXL;
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
    for (int kt = 0; kt < KC / 16; ++kt) {
      const uint32_t kbits = dp.thr ? mifx_rng::keep4(key, (row_base + c + 16 * kt + 4 * h) >> 2, dp.thr) : 0xf;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pe = __expf(s[kt][e] - m);  // exactly 0 for a dead key
        l += pe;
        s[kt][e] = (kbits >> e) & 1 ? pe : 0.f;
      }
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
  const float inv = (dp.thr ? dp.scale : 1.f) / l;
  bf16* dst = out + (size_t)(row0 + qi) * H * D + (size_t)hh * D + 4 * h;
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) *(v4bf*)(dst + 16 * dt) = pack4(o[dt] * inv);
  if (h == 0) {
    stats[(size_t)hh * rows + row0 + qi] = m;
    stats[(size_t)(H + hh) * rows + row0 + qi] = __log2f(l);
  }
}

__global__ __launch_bounds__(NT) void attn_bwd_dq_varlen(const bf16* __restrict__ qkv, const int* __restrict__ cu,
                                                         const int* __restrict__ table, int nseq, int rows, int lmax64,
                                                         const bf16* __restrict__ o, const bf16* __restrict__ dout,
                                                         const float* __restrict__ stats, float scale, Drop dp, int H,
                                                         int h0, bf16* __restrict__ dqkv, float* __restrict__ dsum) {
  extern __shared__ __attribute__((aligned(16))) bf16 smem[];
  const int ent = blockIdx.x / H, hh = blockIdx.x % H;
  const Seq sq = entry(cu, table, ent, nseq, rows, lmax64);
  if (!sq.ok) return;
  const int row0 = sq.row0, L = sq.L, l64 = sq.l64, qb = sq.blk;
  bf16* Ks = smem;
  bf16* Vs = smem + l64 * LD;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, h = lane >> 4, q = r >> 2, p = r & 3;
  const size_t tok = (size_t)3 * H * D, otok = (size_t)H * D;
  const bf16* base = qkv + (size_t)row0 * tok;
  stage_rows(Ks, base + (size_t)(H + hh) * D, tok, L, l64);
  stage_rows(Vs, base + (size_t)(2 * H + hh) * D, tok, L, l64);
  const bool live = qb * QB + 16 * w < L;
  const int qi = qb * QB + 16 * w + r;
  const bool qlive = qi < L;
  v8bf qf[2] = {zero8(), zero8()}, dof[2] = {zero8(), zero8()};
  float di = 0.f, mq = 0.f, lq = 0.f;
  if (qlive) {
    const bf16* pdo = dout + (size_t)(row0 + qi) * otok + (size_t)hh * D;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[ks] = ld8(base + (size_t)qi * tok + (size_t)hh * D + 32 * ks + 8 * h);
      dof[ks] = ld8(pdo + 32 * ks + 8 * h);
    }
    const bf16* po = o + (size_t)(row0 + qi) * otok + (size_t)hh * D + 16 * h;
    const v8bf o0 = ld8(po), o1 = ld8(po + 8), d0 = ld8(pdo + 16 * h), d1 = ld8(pdo + 16 * h + 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) di += (float)o0[e] * (float)d0[e] + (float)o1[e] * (float)d1[e];
    mq = stats[(size_t)hh * rows + row0 + qi];
    lq = stats[(size_t)(H + hh) * rows + row0 + qi];
  }
  di += __shfl_xor(di, 16);  // (the 4 lanes of a query are live or dead together)
  di += __shfl_xor(di, 32);
  if (qlive && h == 0) dsum[(size_t)hh * rows + row0 + qi] = di;
  __syncthreads();
  if (!live) return;  // no barrier follows

  const uint64_t key = dp.thr ? mifx_rng::drop_key(dp.rng, dp.site) : 0;
  const uint64_t row_base = ((uint64_t)(h0 + hh) * rows + row0 + qi) * MAXL;
  const float dsc = dp.thr ? dp.scale : 1.f;
  v4f dq[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) dq[dt] = kZero4;
  for (int c = 0; c < l64; c += KC) {
    v4f ds[KC / 16];
#pragma unroll
    for (int kt = 0; kt < KC / 16; ++kt) {
      v4f sc = kZero4, dpd = kZero4;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        sc = mfma(ld8(Ks + (c + 16 * kt + r) * LD + 32 * ks + 8 * h), qf[ks], sc);
        dpd = mfma(ld8(Vs + (c + 16 * kt + r) * LD + 32 * ks + 8 * h), dof[ks], dpd);
      }
      const int k0 = c + 16 * kt + 4 * h;
      const uint32_t kbits = dp.thr ? mifx_rng::keep4(key, (row_base + k0) >> 2, dp.thr) : 0xf;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pe = k0 + e < L ? prob(sc[e] * scale - mq, lq) : 0.f;  // dead key: exactly 0
        const float dpv = (kbits >> e) & 1 ? dpd[e] * dsc : 0.f;
        ds[kt][e] = pe * (dpv - di) * scale;
      }
    }
    const v8bf dsb[2] = {pack8(ds[0], ds[1]), pack8(ds[2], ds[3])};
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16* pa = Ks + (c + 32 * ks + 4 * h + q) * LD + 16 * dt + 4 * p;
        dq[dt] = mfma(cat8(tr_read(pa), tr_read(pa + 16 * LD)), dsb[ks], dq[dt]);
      }
  }
  if (!qlive) return;
  bf16* dst = dqkv + (size_t)(row0 + qi) * tok + (size_t)hh * D + 4 * h;
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) *(v4bf*)(dst + 16 * dt) = pack4(dq[dt]);
}

__global__ __launch_bounds__(NT) void attn_bwd_dkv_varlen(const bf16* __restrict__ qkv, const int* __restrict__ cu,
                                                          const int* __restrict__ table, int nseq, int rows,
                                                          int lmax64, const bf16* __restrict__ dout,
                                                          const float* __restrict__ stats,
                                                          const float* __restrict__ dsum, float scale, Drop dp, int H,
                                                          int h0, bf16* __restrict__ dqkv) {
  extern __shared__ __attribute__((aligned(16))) bf16 smem[];
  const int ent = blockIdx.x / H, hh = blockIdx.x % H;
  const Seq sq = entry(cu, table, ent, nseq, rows, lmax64);
  if (!sq.ok) return;
  const int row0 = sq.row0, L = sq.L, l64 = sq.l64, kb_ = sq.blk;
  bf16* Qs = smem;
  bf16* dOs = smem + l64 * LD;
  float* Ms = (float*)(smem + 2 * l64 * LD);  // m, log2 l, D of query rows 0 .. l64 - 1 (0 from L on, never used)
  float* Ls = Ms + l64;
  float* Ds = Ls + l64;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, h = lane >> 4, q = r >> 2, p = r & 3;
  const size_t tok = (size_t)3 * H * D, otok = (size_t)H * D;
  const bf16* base = qkv + (size_t)row0 * tok;
  stage_rows(Qs, base + (size_t)hh * D, tok, L, l64);
  stage_rows(dOs, dout + (size_t)row0 * otok + (size_t)hh * D, otok, L, l64);
  for (int i = tid; i < l64; i += NT) {
    float mv = 0.f, lv = 0.f, dv_ = 0.f;
    if (i < L) {
      mv = stats[(size_t)hh * rows + row0 + i];
      lv = stats[(size_t)(H + hh) * rows + row0 + i];
      dv_ = dsum[(size_t)hh * rows + row0 + i];
    }
    Ms[i] = mv;
    Ls[i] = lv;
    Ds[i] = dv_;
  }
  const bool live = kb_ * QB + 16 * w < L;
  const int kj = kb_ * QB + 16 * w + r;
  const bool klive = kj < L;
  v8bf kf[2] = {zero8(), zero8()}, vf[2] = {zero8(), zero8()};
  if (klive) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      kf[ks] = ld8(base + (size_t)kj * tok + (size_t)(H + hh) * D + 32 * ks + 8 * h);
      vf[ks] = ld8(base + (size_t)kj * tok + (size_t)(2 * H + hh) * D + 32 * ks + 8 * h);
    }
  }
  __syncthreads();
  if (!live) return;  // no barrier follows

  const uint64_t key = dp.thr ? mifx_rng::drop_key(dp.rng, dp.site) : 0;
  const uint64_t mrow = (uint64_t)(h0 + hh) * rows + row0;
  const float dsc = dp.thr ? dp.scale : 1.f;
  v4f dk[D / 16], dv[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) dk[dt] = dv[dt] = kZero4;
  for (int c = 0; c < l64; c += KC) {
    v4f pd[KC / 16], ds[KC / 16];
#pragma unroll
    for (int it = 0; it < KC / 16; ++it) {
      // lane: S[i][j], i = c + 16 it + 4h + e, j = kj
      v4f sc = kZero4, dpd = kZero4;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        sc = mfma(ld8(Qs + (c + 16 * it + r) * LD + 32 * ks + 8 * h), kf[ks], sc);
        dpd = mfma(ld8(dOs + (c + 16 * it + r) * LD + 32 * ks + 8 * h), vf[ks], dpd);
      }
      const int i0 = c + 16 * it + 4 * h;
      const float4 M = *(const float4*)(Ms + i0);  // LDS, 16-B aligned (i0 % 4 == 0)
      const float4 Lq = *(const float4*)(Ls + i0);
      const float4 Dq = *(const float4*)(Ds + i0);
      const float mv[4] = {M.x, M.y, M.z, M.w}, lv[4] = {Lq.x, Lq.y, Lq.z, Lq.w}, dv4[4] = {Dq.x, Dq.y, Dq.z, Dq.w};
      uint32_t nib = 0xf;
      if (dp.thr) nib = mifx_rng::keep4(key, ((mrow + i0 + p) * MAXL + (kj & ~3)) >> 2, dp.thr);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool kept = dp.thr ? ((__shfl(nib, (lane & ~3) | e) >> p) & 1) : true;
        // a dead query (or a dead key lane): P_d and dS exactly 0
        const float pe = (i0 + e < L && klive) ? prob(sc[e] * scale - mv[e], lv[e]) : 0.f;
        pd[it][e] = kept ? pe * dsc : 0.f;
        ds[it][e] = pe * ((kept ? dpd[e] * dsc : 0.f) - dv4[e]) * scale;
      }
    }
    const v8bf pdb[2] = {pack8(pd[0], pd[1]), pack8(pd[2], pd[3])};
    const v8bf dsb[2] = {pack8(ds[0], ds[1]), pack8(ds[2], ds[3])};
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16* pa = dOs + (c + 32 * ks + 4 * h + q) * LD + 16 * dt + 4 * p;
        dv[dt] = mfma(cat8(tr_read(pa), tr_read(pa + 16 * LD)), pdb[ks], dv[dt]);
        const bf16* pq = Qs + (c + 32 * ks + 4 * h + q) * LD + 16 * dt + 4 * p;
        dk[dt] = mfma(cat8(tr_read(pq), tr_read(pq + 16 * LD)), dsb[ks], dk[dt]);
      }
  }
  if (!klive) return;
  bf16* dst = dqkv + (size_t)(row0 + kj) * tok + 4 * h;
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    *(v4bf*)(dst + (size_t)(H + hh) * D + 16 * dt) = pack4(dk[dt]);
    *(v4bf*)(dst + (size_t)(2 * H + hh) * D + 16 * dt) = pack4(dv[dt]);
  }
}

uint32_t drop_threshold(float p) {
  if (!(p > 0.f)) return 0;
  const float t = p * 65536.f + 0.5f;
  return t >= 65536.f ? 65536u : (uint32_t)t;
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
