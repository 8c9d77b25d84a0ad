// The chunked self-attention kernels for gfx950, head dim 64, sequences of up to 512 tokens: one body each for the
// forward with online softmax, the backward's dQ pass and its dK / dV pass, and the fragment helpers they (and the
// S <= 128 kernels of csrc/attention.hip) are built from. The bodies are instantiated by thin __global__ wrappers over
// two layouts:
//  * dense  (csrc/attention.hip: attn_fwd_long, attn_bwd_dq_long, attn_bwd_dkv_long): [B, S, ...] tensors,
//    S % 64 == 0, an optional additive key bias, statistics [2, B, H, S];
//  * packed (csrc/attn_varlen_train.hip: attn_fwd_varlen_train, attn_bwd_dq_varlen, attn_bwd_dkv_varlen;
//    csrc/bert_infer.hip: attn_fwd_varlen): [rows, ...] tensors holding sequences of any length 1 .. 512 back to
//    back, found through a cu_seqlens table and a block table, statistics [2, H, rows].
//
// The whole S x S problem of such a sequence does not fit one CU's registers and LDS, so it is tiled flash-style in
// the chained MFMA orientation of the S <= 128 kernels:
//  * forward: a workgroup owns 128 queries of one (sequence, head) (8 waves x 16), the head's K and V rows resident in
//    LDS (144 B rows: 147 KB at 512 keys); keys stream in chunks of 64 with an online softmax (running max and row sum
//    per query lane, the O^T accumulators rescaled per chunk), the dropout mask drawn per chunk. S^T = K Q^T and
//    O^T = V^T P^T chain, V^T read by ds_read_tr16_b64.
//  * backward, dQ: the same partition; with the forward's statistics the probabilities of a key chunk need nothing
//    from other chunks, so dS^T is formed chunk by chunk and dQ^T = K^T dS^T accumulates in registers. It also
//    writes D_i = rowsum(dO o O) for the second kernel.
//  * backward, dK / dV: a workgroup owns 128 keys (wave = 16 keys), Q and dO resident; query chunks of 64 give
//    S = Q K^T and dP_d = dO V^T in the [query][key] orientation, so P_d and dS chain straight into
//    dV^T = dO^T P_d and dK^T = Q^T dS with dO / Q read transposed -- the forward's structure with the roles of
//    queries and keys exchanged. The lane holds 4 query rows of one key column; the dropout bits come from one
//    mask draw per lane (row 4h + lane % 4, its quad's 4 keys) exchanged within the quad.
//
// A body is templated on a geometry G (Dense, Packed below), which answers what the layouts differ in: which rows the
// workgroup owns, whether a row can be dead (G::ragged), how a score is biased or masked, where the statistics live
// and which flat index the dropout mask takes. Everything G::ragged guards is resolved at compile time: a dense
// kernel carries no row predicate, no dead-key select and no zero fragment.
//
// The ragged edge of a packed sequence of length L (l64 = L rounded up to 64):
//  * no row at or beyond L is read from global memory (qkv, out, dout, statistics, dsum), and none is written. The
//    reads are predicated, not clamped: the row after the last sequence is past the allocation;
//  * the staging rows L .. l64 - 1 are zero-filled (a garbage V row times P = 0 is NaN if it holds Inf), and dead query
//    and key lanes compute on zero8() fragments;
//  * forward: keys at or beyond L are masked by select to the running maximum's floor, -3.0e38: exp(floor - m) is
//    exactly 0, so they add nothing to l or O (every chunk holds a live key, L >= 1, so m is finite from the first
//    chunk on);
//  * backward: a dead key (j >= L) has a zero K row, score 0, and exp2((0 - m) log2e - log2 l) is not 0 (it overflows
//    for a very negative m, and inf * 0 through the zero K row is NaN): P is selected to 0. P_d and dS of a dead query
//    (i >= L) are selected to 0 as well, its statistics never read;
//  * a skipped table entry (padding, or a sequence that does not fit: L > lmax, row0 + L > rows, ...) returns before
//    any barrier; a wave with no live row returns after the staging barrier, which is the last barrier;
//  * every element of dqkv on a row owned by a listed sequence is written exactly once (dq by the dQ kernel, dk and
//    dv by the dK / dV kernel); rows owned by no sequence are not touched (the caller hands dqkv over zeroed). Dense
//    writes every element.
// Dense has no ragged edge, but at S = 192 and 320 the last 128-row block has dead waves: `live` is per wave in both
// layouts (and qlive / klive per lane where ragged).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "counter_rng.h"
#include "mfma_stage.h"

namespace {

constexpr int D = 64;      // head dim
constexpr int LD = D + 8;  // LDS row of a [token][d] image (elements): 144 B. K and V of 512 rows must fit 160 KB
// rows per workgroup (8 waves x 16), threads, rows per chunk, longest sequence
constexpr int QB = 128, NT = 512, KC = 64, MAXL = 512;
constexpr float kFloor = -3.0e38f;  // where the running maximum starts, and what a dead key's score is selected to
constexpr float kLog2e = 1.4426950408889634f;
constexpr v4f kZero4 = {0.f, 0.f, 0.f, 0.f};

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

// the backward's probability from the saved statistics of its row (the note at mifx_attn_fwd): sm = biased score minus
// the row maximum, l2 = log2 of the row sum. exp(sm) / l as one fma and one v_exp_f32 (__expf is a multiply and the
// same instruction)
__device__ __forceinline__ float prob(float sm, float l2) { return __builtin_amdgcn_exp2f(fmaf(sm, kLog2e, -l2)); }

struct Drop {
  const int64_t* rng;
  int site;
  uint32_t thr;  // 0: no dropout
  float scale;   // 1 / (1 - p)
};

inline uint32_t drop_threshold(float p) {
  if (!(p > 0.f)) return 0;
  const float t = p * 65536.f + 0.5f;
  return t >= 65536.f ? 65536u : (uint32_t)t;
}

// rows 0 .. L - 1 of one strided tensor into an LDS [l64][LD] image (16-B chunks); ragged: rows L .. l64 - 1 zero
template <bool kRagged>
__device__ __forceinline__ void stage_rows(bf16* dst, const bf16* src, size_t row_stride, int L, int l64) {
#pragma unroll 4
  for (int c = threadIdx.x; c < l64 * 8; c += NT) {
    const int row = c >> 3, ch = c & 7;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (!kRagged || row < L) v = *(const uint4*)(src + (size_t)row * row_stride + ch * 8);
    *(uint4*)(dst + row * LD + ch * 8) = v;
  }
}

// ---- geometries ------------------------------------------------------------------------------------------------
// ok (false: a skipped table entry), the sequence's first row row0 of the [rows, ...] tensors, its length L and
// l64 = L rounded up to a chunk, the workgroup's 128-row block blk and its local head hh; then
//   stat(i)      index of row i in a plane of the statistics (and in dsum); the log2 l plane is `plane` further on
//   drop_row(i)  flat dropout index of (global head, query row i, key 0); key j adds j
//   kbias4 / kbias1  the additive bias of 4 keys / one key
//   score        the forward's biased score; alive: the key is inside the sequence
//   prob_of      the backward's probability; alive: query and key are inside the sequence
//   stage_stats / stats4  m, log2 l and D of 4 query rows for the dK / dV pass (`sl`: LDS behind the two images)
// The two layouts keep their own score and probability expressions: a * scale + bias and a * scale contract to
// different FMAs, and neither result may move by a bit.

// the query (key) blocks of one head are consecutive logical blocks: keep them on one XCD (dispatch round-robins
// consecutive workgroups over the 8 XCDs), so the head's K / V (Q / dO) rows are fetched into one L2
__device__ __forceinline__ int xcd_block(int bid, int nwg) { return (nwg & 7) ? bid : (bid & 7) * (nwg >> 3) + (bid >> 3); }

// [B, S, ...] tensors, S % 64 == 0: one workgroup per (batch, head, 128-row block); kbias [B, S] or null; statistics
// [2, B, H, S], dsum [B, H, S]; dropout index ((b Htot + h0 + h) S + i) S + j
struct Dense {
  static constexpr bool ragged = false;
  static constexpr bool ok = true;
  int row0, L, l64, blk, hh;
  int bh;
  const float* kb;
  uint64_t mrow;
  size_t plane;

  __device__ __forceinline__ Dense(int S, int H, int h0, int Htot, const float* kbias) {
    const int nqb = (S + QB - 1) / QB, lb = xcd_block(blockIdx.x, gridDim.x);
    blk = lb % nqb, bh = lb / nqb;
    const int b = bh / H;
    hh = bh % H;
    row0 = b * S, L = l64 = S;
    kb = kbias ? kbias + (size_t)b * S : nullptr;
    mrow = ((uint64_t)b * Htot + h0 + hh) * S;
    plane = (size_t)(gridDim.x / nqb) * S;
  }
  __device__ __forceinline__ size_t stat(int i) const { return (size_t)bh * L + i; }
  __device__ __forceinline__ uint64_t drop_row(int i) const { return (mrow + i) * L; }
  __device__ __forceinline__ float4 kbias4(int k0) const {
    return kb ? *(const float4*)(kb + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __device__ __forceinline__ float kbias1(int kj) const { return kb ? kb[kj] : 0.f; }
  __device__ __forceinline__ float score(float a, float scale, float bias, bool) const { return a * scale + bias; }
  __device__ __forceinline__ float prob_of(float s, float scale, float bias, float m, float l2, bool) const {
    return prob(s * scale + bias - m, l2);
  }
  __device__ __forceinline__ void stage_stats(float*, const float*, const float*) const {}
  __device__ __forceinline__ void stats4(const float*, const float* stats, const float* dsum, int i0, float4& M,
                                         float4& L2, float4& Dq) const {
    M = *(const float4*)(stats + stat(i0));
    L2 = *(const float4*)(stats + plane + stat(i0));
    Dq = *(const float4*)(dsum + stat(i0));
  }
};

// [rows, ...] tensors with the sequences back to back: cu int32 [nseq + 1] (sequence b owns rows cu[b] ..
// cu[b + 1] - 1), a block table of (sequence, 128-row block) pairs, one workgroup per entry and head; no bias;
// statistics [2, H, rows], dsum [H, rows]. Dropout index ((h0 + h) rows + cu[b] + i) 512 + j, which does not depend
// on the head split nor on how the sequences of other packs of the same capacity are ordered, and is a multiple of 4
// wherever j is (the 4-key groups of keep4 stay aligned). Host twin: mifx.ops.fused_bert.keep_mask.
struct Packed {
  static constexpr bool ragged = true;
  bool ok;
  int row0, L, l64, blk, hh;
  int rows;
  uint64_t mrow;
  size_t plane;

  // rows: the row count of the allocations; lmax64: what the dynamic LDS was sized for. A table entry whose sequence
  // does not fit either is skipped, not trusted (the host validates; this keeps a bad table from reading out of bounds)
  __device__ __forceinline__ Packed(const int* cu, const int* table, int nseq, int rows_, int lmax64, int H, int h0) {
    const int ent = blockIdx.x / H;
    hh = blockIdx.x % H;
    rows = rows_;
    ok = false;
    row0 = L = l64 = 0;
    const int seq = table[2 * ent];
    blk = table[2 * ent + 1];
    if (seq < 0 || seq >= nseq || blk < 0) return;
    row0 = cu[seq];
    L = cu[seq + 1] - row0;
    l64 = (L + KC - 1) / KC * KC;
    ok = row0 >= 0 && L >= 1 && L <= MAXL && l64 <= lmax64 && row0 <= rows - L && blk * QB < L;
    mrow = (uint64_t)(h0 + hh) * rows + row0;
    plane = (size_t)H * rows;
  }
  __device__ __forceinline__ size_t stat(int i) const { return (size_t)hh * rows + row0 + i; }
  __device__ __forceinline__ uint64_t drop_row(int i) const { return (mrow + i) * MAXL; }
  __device__ __forceinline__ float4 kbias4(int) const { return make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ __forceinline__ float kbias1(int) const { return 0.f; }
  __device__ __forceinline__ float score(float a, float scale, float, bool alive) const {
    return alive ? a * scale : kFloor;
  }
  __device__ __forceinline__ float prob_of(float s, float scale, float, float m, float l2, bool alive) const {
    return alive ? prob(s * scale - m, l2) : 0.f;  // dead: exactly 0
  }
  // the statistics' packed rows cu[b] + i have no alignment and the last group of 4 runs into the next sequence, so
  // the dense float4 global loads do not carry over: predicated per-row loads into LDS (0 from L on, never used)
  __device__ __forceinline__ void stage_stats(float* sl, const float* stats, const float* dsum) const {
    for (int i = threadIdx.x; i < l64; i += NT) {
      float mv = 0.f, lv = 0.f, dv = 0.f;
      if (i < L) {
        mv = stats[stat(i)];
        lv = stats[plane + stat(i)];
        dv = dsum[stat(i)];
      }
      sl[i] = mv;
      sl[l64 + i] = lv;
      sl[2 * l64 + i] = dv;
    }
  }
  __device__ __forceinline__ void stats4(const float* sl, const float*, const float*, int i0, float4& M, float4& L2,
                                         float4& Dq) const {
    M = *(const float4*)(sl + i0);  // LDS, 16-B aligned (i0 % 4 == 0)
    L2 = *(const float4*)(sl + l64 + i0);
    Dq = *(const float4*)(sl + 2 * l64 + i0);
  }
};

// ---- bodies ----------------------------------------------------------------------------------------------------
// smem: the dynamic LDS, two [l64][LD] images (the dK / dV pass of a ragged geometry: + 3 l64 floats behind them).

// out [rows, H, 64]; kTrain: dropout dp, and the statistics m and log2 l of every live query row into `stats`
template <class G, bool kTrain>
__device__ __forceinline__ void chunked_fwd(const G& g, bf16* smem, const bf16* __restrict__ qkv, float scale, Drop dp,
                                            int H, bf16* __restrict__ out, float* __restrict__ stats) {
  if (!g.ok) return;  // uniform over the workgroup, before any barrier
  const int L = g.L, l64 = g.l64, hh = g.hh;
  bf16* Ks = smem;
  bf16* Vs = smem + l64 * LD;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, h = lane >> 4, q = r >> 2, p = r & 3;
  const size_t tok = (size_t)3 * H * D;
  const bf16* base = qkv + (size_t)g.row0 * tok;
  stage_rows<G::ragged>(Ks, base + (size_t)(H + hh) * D, tok, L, l64);
  stage_rows<G::ragged>(Vs, base + (size_t)(2 * H + hh) * D, tok, L, l64);
  const bool live = g.blk * QB + 16 * w < L;
  const int qi = g.blk * QB + 16 * w + r;
  const bool qlive = G::ragged ? qi < L : live;
  v8bf qf[2];
  if constexpr (G::ragged) qf[0] = qf[1] = zero8();
  if (qlive)  // one branch around both loads: predicated one by one, the dense kernel takes 97 VGPRs instead of 76
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = ld8(base + (size_t)qi * tok + (size_t)hh * D + 32 * ks + 8 * h);
  __syncthreads();
  if (!live) return;  // no barrier follows

  const bool drop = kTrain && dp.thr;
  const uint64_t key = drop ? mifx_rng::drop_key(dp.rng, dp.site) : 0;
  const uint64_t row_base = g.drop_row(qi);
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
      const float4 bb = g.kbias4(k0);
      const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = g.score(a[e], scale, bv[e], k0 + e < L);
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
      const uint32_t kbits = drop ? mifx_rng::keep4(key, (row_base + c + 16 * kt + 4 * h) >> 2, dp.thr) : 0xf;
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
  const float inv = (drop ? dp.scale : 1.f) / l;
  bf16* dst = out + (size_t)(g.row0 + qi) * H * D + (size_t)hh * D + 4 * h;
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) *(v4bf*)(dst + 16 * dt) = pack4(o[dt] * inv);
  if (kTrain && h == 0) {
    stats[g.stat(qi)] = m;
    stats[g.plane + g.stat(qi)] = __log2f(l);
  }
}

// o / dout [rows, H, 64], stats: the forward's; writes dq of its live rows into dqkv [rows, 3, H, 64] and
// dsum = rowsum(dO o O)
template <class G>
__device__ __forceinline__ void chunked_bwd_dq(const G& g, bf16* smem, const bf16* __restrict__ qkv,
                                               const bf16* __restrict__ o, const bf16* __restrict__ dout,
                                               const float* __restrict__ stats, float scale, Drop dp, int H,
                                               bf16* __restrict__ dqkv, float* __restrict__ dsum) {
  if (!g.ok) return;
  const int L = g.L, l64 = g.l64, hh = g.hh;
  bf16* Ks = smem;
  bf16* Vs = smem + l64 * LD;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, h = lane >> 4, q = r >> 2, p = r & 3;
  const size_t tok = (size_t)3 * H * D, otok = (size_t)H * D;
  const bf16* base = qkv + (size_t)g.row0 * tok;
  stage_rows<G::ragged>(Ks, base + (size_t)(H + hh) * D, tok, L, l64);
  stage_rows<G::ragged>(Vs, base + (size_t)(2 * H + hh) * D, tok, L, l64);
  const bool live = g.blk * QB + 16 * w < L;
  const int qi = g.blk * QB + 16 * w + r;
  const bool qlive = G::ragged ? qi < L : live;
  v8bf qf[2], dof[2];
  if constexpr (G::ragged) qf[0] = qf[1] = dof[0] = dof[1] = zero8();
  float di = 0.f, mq = 0.f, lq = 0.f;
  if (qlive) {
    const bf16* pdo = dout + (size_t)(g.row0 + qi) * otok + (size_t)hh * D;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[ks] = ld8(base + (size_t)qi * tok + (size_t)hh * D + 32 * ks + 8 * h);
      dof[ks] = ld8(pdo + 32 * ks + 8 * h);
    }
    // D_i = sum_d dO o O over the lane group's 16 d values, reduced over the 4 groups
    const bf16* po = o + (size_t)(g.row0 + qi) * otok + (size_t)hh * D + 16 * h;
    const v8bf o0 = ld8(po), o1 = ld8(po + 8), d0 = ld8(pdo + 16 * h), d1 = ld8(pdo + 16 * h + 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) di += (float)o0[e] * (float)d0[e] + (float)o1[e] * (float)d1[e];
    mq = stats[g.stat(qi)];
    lq = stats[g.plane + g.stat(qi)];
  }
  di += __shfl_xor(di, 16);  // (the 4 lanes of a query are live or dead together)
  di += __shfl_xor(di, 32);
  if (qlive && h == 0) dsum[g.stat(qi)] = di;
  __syncthreads();
  if (!live) return;  // no barrier follows

  const uint64_t key = dp.thr ? mifx_rng::drop_key(dp.rng, dp.site) : 0;
  const uint64_t row_base = g.drop_row(qi);
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
      const float4 bb = g.kbias4(k0);
      const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
      const uint32_t kbits = dp.thr ? mifx_rng::keep4(key, (row_base + k0) >> 2, dp.thr) : 0xf;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pe = g.prob_of(sc[e], scale, bv[e], mq, lq, k0 + e < L);
        const float dpv = (kbits >> e) & 1 ? dpd[e] * dsc : 0.f;  // dP = dP_d o M / (1 - p)
        ds[kt][e] = pe * (dpv - di) * scale;                      // dS (with the score scale folded in)
      }
    }
    const v8bf dsb[2] = {pack8(ds[0], ds[1]), pack8(ds[2], ds[3])};
    // dQ^T += K^T dS^T over this chunk (K rows read transposed at the chained key order)
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16* pa = Ks + (c + 32 * ks + 4 * h + q) * LD + 16 * dt + 4 * p;
        dq[dt] = mfma(cat8(tr_read(pa), tr_read(pa + 16 * LD)), dsb[ks], dq[dt]);
      }
  }
  if (!qlive) return;
  bf16* dst = dqkv + (size_t)(g.row0 + qi) * tok + (size_t)hh * D + 4 * h;
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) *(v4bf*)(dst + 16 * dt) = pack4(dq[dt]);
}

// stats and dsum: the forward's and the dQ pass's; writes dk and dv of its live key rows into dqkv
template <class G>
__device__ __forceinline__ void chunked_bwd_dkv(const G& g, bf16* smem, const bf16* __restrict__ qkv,
                                                const bf16* __restrict__ dout, const float* __restrict__ stats,
                                                const float* __restrict__ dsum, float scale, Drop dp, int H,
                                                bf16* __restrict__ dqkv) {
  if (!g.ok) return;
  const int L = g.L, l64 = g.l64, hh = g.hh;
  bf16* Qs = smem;
  bf16* dOs = smem + l64 * LD;
  float* sl = (float*)(smem + 2 * l64 * LD);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, h = lane >> 4, q = r >> 2, p = r & 3;
  const size_t tok = (size_t)3 * H * D, otok = (size_t)H * D;
  const bf16* base = qkv + (size_t)g.row0 * tok;
  stage_rows<G::ragged>(Qs, base + (size_t)hh * D, tok, L, l64);
  stage_rows<G::ragged>(dOs, dout + (size_t)g.row0 * otok + (size_t)hh * D, otok, L, l64);
  g.stage_stats(sl, stats, dsum);
  const bool live = g.blk * QB + 16 * w < L;
  const int kj = g.blk * QB + 16 * w + r;
  const bool klive = G::ragged ? kj < L : live;
  v8bf kf[2], vf[2];
  if constexpr (G::ragged) kf[0] = kf[1] = vf[0] = vf[1] = zero8();
  float bj = 0.f;
  if (klive) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      kf[ks] = ld8(base + (size_t)kj * tok + (size_t)(H + hh) * D + 32 * ks + 8 * h);
      vf[ks] = ld8(base + (size_t)kj * tok + (size_t)(2 * H + hh) * D + 32 * ks + 8 * h);
    }
    bj = g.kbias1(kj);
  }
  __syncthreads();
  if (!live) return;  // no barrier follows

  const uint64_t key = dp.thr ? mifx_rng::drop_key(dp.rng, dp.site) : 0;
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
      float4 M, L2, Dq;
      g.stats4(sl, stats, dsum, i0, M, L2, Dq);
      const float mv[4] = {M.x, M.y, M.z, M.w}, lv[4] = {L2.x, L2.y, L2.z, L2.w}, dv4[4] = {Dq.x, Dq.y, Dq.z, Dq.w};
      uint32_t nib = 0xf;
      if (dp.thr) nib = mifx_rng::keep4(key, (g.drop_row(i0 + p) + (kj & ~3)) >> 2, dp.thr);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool kept = dp.thr ? ((__shfl(nib, (lane & ~3) | e) >> p) & 1) : true;
        const float pe = g.prob_of(sc[e], scale, bj, mv[e], lv[e], i0 + e < L && klive);
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
  bf16* dst = dqkv + (size_t)(g.row0 + kj) * tok + 4 * h;
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    *(v4bf*)(dst + (size_t)(H + hh) * D + 16 * dt) = pack4(dk[dt]);
    *(v4bf*)(dst + (size_t)(2 * H + hh) * D + 16 * dt) = pack4(dv[dt]);
  }
}

}  // namespace
