// General fused Wide&Deep training step for gfx950: any DNN tower of 1..6 hidden layers, widths 2..256.
//
// The specialised kernels (csrc/wd_chain.hip, csrc/wide_deep.hip) are compiled for the padding of the taxi
// tower [100, 70, 48, 34]; this one takes the tower at run time (a small device-resident descriptor) and is the
// path for every other `hidden_units`. Same data path as wd_fused, so one emulation defines correctness: biases
// folded into the bf16 weight image through a constant-1 input column, bf16 operands (weights, activations rounded
// after ReLU, dZ rounded after the ReLU mask), fp32 MFMA accumulation, logit = deep + fp32 wide gather + wide
// bias, dl = (sigmoid(logit) - y) * grad_scale, dW = dZ^T A, dA = dZ W, the wide gradient through the chained
// kernel's fixed-point LDS histogram (order-independent). Records come through csrc/feed.h.
//
// Padding: layer l maps K_l = roundup(in_l + 1, 32) inputs (the +1 is the constant-1 column) to
// N_l = K_{l+1} outputs (the head: 32), so every image is a whole number of 32-deep MFMA k-steps and a layer's
// output image IS the next layer's input image. K_l <= 288.
//
// wdg_fused, per 64-example tile (grid-stride), 4 waves, wave w owns examples [16w, 16w + 16):
//  * forward, wave-local: Z^T = W^T . A^T with v_mfma_f32_16x16x32_bf16, the weight fragments read straight from
//    the L2-resident bf16 image W^T [N][K] (a wide tower's weights do not fit LDS: 3 x 288 x 288 x 2 B), the
//    activation fragments from a row-major LDS image. Each layer's output is kept in LDS for the next layer AND
//    written to a per-workgroup global scratch (L2-resident): six 288-wide activation images do not fit LDS.
//  * backward, layer by layer from the head: three LDS images -- A_l (reloaded from the scratch), dZ_l, dZ_{l-1}.
//    dW_l = dZ_l^T A_l over the tile's 64 examples through transposed LDS reads (ds_read_b64_tr_b16), the dW tiles
//    dealt round-robin to the waves; dZ_{l-1} = (dZ_l . W_l) masked by A_l > 0, wave-local, with the weight
//    fragments from a second, transposed image W [K][N] that the optimizer kernel keeps beside the first.
//  * dW accumulation: the choice between "accumulate into the workgroup's own slab" and "keep all activations of
//    all of the workgroup's tiles in scratch and reduce over them at the end" is the FIRST: the first tile of a
//    workgroup stores its dW tiles into the slab, every later tile feeds the slab values in as the MFMA's C operand
//    and stores the sum back. Every slab entry is read and written by one fixed lane of one fixed wave, so program
//    order is all the ordering it needs; no atomics, no zero-fill. The scratch then holds one tile only
//    (64 x sum K_l bf16 per workgroup) and the registers hold no dW state across tiles, which is what lets the
//    tower be a run-time value. Cost: one slab round trip through L2 per extra tile of a workgroup; none when the
//    grid covers the batch (batch <= 64 x grid).
//  * slab layout (this kernel's own): fp32 [grid][stride], stride = WTOT + WIDE_PAD; DNN entries in the order of
//    the W^T image (layer, n, k), so slab column == master-state index == image offset; then the wide columns.
//    The host caps the grid so that grid x stride x 4 B <= SLAB_BOUND_MB (128 MB).
//
// wdg_reduce_opt: sums the slab rows in row order 0..G-1 (fixed, deterministic), applies opt_update (csrc/wd_opt.h)
// with the DNN / wide OptHyper by column kind, writes the fp32 master state and both bf16 images. kind[col]: -1
// padding (never touched: includes the constant-1 producers), -2 wide, >= 0 DNN entry with its offset in the
// transposed image. Step from per-workgroup device slots (slot 0 is what wdg_fused reads): hipGraph-capturable.
//
// Differentially private training (wdg_fused<true, true>, per-example clipping, "ghost clipping"): the model is
// linear layers plus an embedding bag, so the L2 norm of example i's gradient factorises exactly,
//   n_i^2 = sum_l (sum_{n < out_l} dZ_l[i,n]^2) (sum_k A_l[i,k]^2) + 10 dl_i^2
// (the bias is inside A_l through the constant-1 column; column out_l of dZ_l feeds the constant-1 producer, which
// is not trained and is left out; padding columns carry A = 0; the wide part is nine one-hot columns plus the
// bias). Per tile: dl_i = sigmoid(x_i) - y_i unscaled; a wave-local NORM SWEEP walks the dZ chain once with no dW
// work (the ReLU masks read back from the scratch by the lane that wrote them, the row norms of A_l taken in the
// forward epilogue); c_i = min(1, s C / n_i); the GRADIENT SWEEP is the backward above and recomputes the same
// unscaled chain, but what enters dW_l is the row bf16(c_i dZ_l[i, :]) (Dcur scaled in place after the dA product
// has read it) and the wide histogram takes c_i dl_i. The chain is never rerun on a rescaled dl: c_i is no power of
// two, every bf16 rounding of a rescaled chain would differ from the chain whose norm was measured. Scaling the
// already rounded rows once moves each element by at most a factor 1 + 2^-8 (bf16 round-to-nearest), so the
// realised norm is <= (1 + 2^-8) c_i n_i; DP_SHRINK = s absorbs that and the fp32 rounding of n_i (see below).
// wdg_reduce_opt then adds noise_multiplier C N(0,1) (Philox4x32-10 + Box-Muller of csrc/philox.h, counter
// (column group of 4, 0, step lo, step hi), key = seed, step = the device step slot before its increment) to every
// column with kind != -1 and multiplies by grad_scale: (sum of clipped + noise) / M, as GaussianAverageQuery.
#include <hip/hip_runtime.h>
#include "feed.h"
#include <stdint.h>

namespace {

typedef __bf16 bf16;
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef __bf16 v4bf __attribute__((ext_vector_type(4)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef short v8s __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s lds_v4s;

#include "wd_opt.h"
#include "philox.h"

constexpr int T = 64;        // examples per tile
constexpr int NTHR = 256;    // 4 waves x 16 examples
constexpr int PAD = 8;       // bf16 elements of LDS row padding
constexpr int MAXH = 6;      // hidden layers
constexpr int MAXW = 256;    // hidden width
constexpr int MAXL = MAXH + 1;  // layers with the head
constexpr int KMAX = 288;    // roundup(MAXW + 1, 32)
constexpr int NWIDE = 2128;  // 2127 identity buckets + bias
constexpr int WIDE_BIAS = 2127;
constexpr int WIDE_PAD = 2176;
constexpr int SLOTS = 1024;  // optimizer step slots (one per wdg_reduce_opt workgroup)
constexpr int SLAB_BOUND_MB = 128;
// descriptor (int32): [0] layers with the head, [1] LDS row stride (max K + PAD), [2] WTOT, then per layer at
// DESC_HDR + DESC_LAYER * l: K, N, image/slab offset, live dW n tiles, live dW k tiles, scratch offset of A_l,
// trainable outputs out_l (the head: 1; read by the DP norm sweep)
constexpr int DESC_HDR = 8, DESC_LAYER = 8;
constexpr int DESC_LEN = DESC_HDR + DESC_LAYER * MAXL;
// DP clip shrink s: example i is scaled by c_i = min(1, s C / n_i). Rounding c_i dZ to bf16 (round-to-nearest, 8
// significand bits) grows an element by at most 1 + 2^-8, the wide part is scaled in fp32. n_i^2 is an fp32 sum of
// at most MAXL products of two fp32 sums of <= KMAX non-negative terms: relative error below 2 (KMAX + MAXL) 2^-24
// < 2^-14, so n_i is off by less than 2^-15; c_i (one multiply, one divide) and c_i dZ (one multiply) add 3 x 2^-24.
// s = (1 - 2^-12) / (1 + 2^-8) leaves more than a sevenfold margin on that: the realised per-example norm is
// <= C, and >= s C (1 - 2^-8) > 0.99 C for a clipped example. An example with n_i <= s C keeps c_i = 1 and is
// untouched.
constexpr float DP_SHRINK = (float)((1.0 - 1.0 / 4096.0) / (1.0 + 1.0 / 256.0));
constexpr int DP_LDS = MAXL * T * 4;  // DP: fp32 row norms^2 of A_l for the tile, [MAXL][T]

__constant__ int kWideOff[9] = {0, 1010, 2020, 2030, 2040, 2050, 2060, 2084, 2115};
__constant__ int kWideNb[9] = {1010, 1010, 10, 10, 10, 10, 24, 31, 12};

__device__ __forceinline__ v4s tr_read(const uint16_t* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(p));
}
__device__ __forceinline__ v8bf cat8(v4s a, v4s b) {
  v8s r = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(v8bf, r);
}
__device__ __forceinline__ v8bf ld8(const uint16_t* p) { return *(const v8bf*)p; }
__device__ __forceinline__ v4f mfma(v8bf a, v8bf b, v4f c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// same-wave LDS write -> read ordering: DS ops of one wave execute in order; only the compiler must not reorder
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

// Out^T[n][t] = sum_k W[n][k] B[t][k] for the 16 rows t of B (row r of the fragment = lane & 15): `ntile` 16-row
// tiles of the global bf16 matrix W (leading dimension ldw), `ksteps` 32-deep k-steps; two tiles per pass share the
// B fragments, the operand loads of four k-steps are issued before their MFMAs. epi(tile, acc): acc[i] is
// Out[t = r][n = 16 tile + 4 h + i].
template <class Epi>
__device__ __forceinline__ void rows_gemm(const uint16_t* __restrict__ W, int ldw, int ntile, int ksteps,
                                          const uint16_t* B, int ldb, int r, int h, Epi epi) {
  for (int t0 = 0; t0 < ntile; t0 += 2) {
    const bool two = t0 + 1 < ntile;
    const int t1 = two ? t0 + 1 : t0;
    v4f acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const uint16_t* w0 = W + (size_t)(16 * t0 + r) * ldw + 8 * h;
    const uint16_t* w1 = W + (size_t)(16 * t1 + r) * ldw + 8 * h;
    const uint16_t* b = B + r * ldb + 8 * h;
    for (int s0 = 0; s0 < ksteps; s0 += 4) {
      v8bf a0[4], a1[4], bb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int s = min(s0 + j, ksteps - 1);  // clamped: branch-free loads, the extra ones are not used
        a0[j] = ld8(w0 + 32 * s);
        a1[j] = ld8(w1 + 32 * s);
        bb[j] = ld8(b + 32 * s);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (s0 + j < ksteps) {
          acc0 = mfma(a0[j], bb[j], acc0);
          acc1 = mfma(a1[j], bb[j], acc1);
        }
      }
    }
    epi(t0, acc0);
    if (two) epi(t1, acc1);
  }
}

// dWt[n][k] (+)= sum_t dZ[t][n] A[t][k] over the 64 tile rows, live tiles only, dealt round-robin to the waves.
// dst = the workgroup's slab at the layer's offset, rows of K floats. first: store, else accumulate (C operand).
__device__ __forceinline__ void dw_layer(const uint16_t* dZ, const uint16_t* A, int bs, int nlive, int klive, int K,
                                         float* __restrict__ dst, bool first, int w, int r, int h) {
  const int q = r >> 2, p = r & 3;
  const int nitems = nlive * klive;
  for (int it0 = w; it0 < nitems; it0 += 8) {
    v8bf fa[2][2], fb[2][2];
    v4f acc[2];
    float* d[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int item = min(it0 + 4 * j, nitems - 1);
      const int nt = item / klive, kt = item - nt * klive;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const uint16_t* pa = dZ + (32 * s + 8 * h + q) * bs + 16 * nt + 4 * p;
        fa[j][s] = cat8(tr_read(pa), tr_read(pa + 4 * bs));
        const uint16_t* pb = A + (32 * s + 8 * h + q) * bs + 16 * kt + 4 * p;
        fb[j][s] = cat8(tr_read(pb), tr_read(pb + 4 * bs));
      }
      d[j] = dst + (size_t)(16 * nt + 4 * h) * K + 16 * kt + r;
      acc[j] = (v4f){0.f, 0.f, 0.f, 0.f};
      if (!first) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = d[j][(size_t)i * K];
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      acc[j] = mfma(fa[j][0], fb[j][0], acc[j]);
      acc[j] = mfma(fa[j][1], fb[j][1], acc[j]);
      if (it0 + 4 * j < nitems) {
#pragma unroll
        for (int i = 0; i < 4; ++i) d[j][(size_t)i * K] = acc[j][i];
      }
    }
  }
}

template <bool TRAIN, bool DP>
__global__ __launch_bounds__(NTHR, 1) void wdg_fused(
    const uint4* __restrict__ data, long long n_data, long long batch, long long start_fixed,
    const long long* __restrict__ step_ctr, const uint16_t* __restrict__ wimg, const float* __restrict__ wide,
    float* __restrict__ slab, float* __restrict__ slab_loss, float* __restrict__ logits_out, float grad_scale,
    const int* __restrict__ desc, uint16_t* __restrict__ scratch, int scratch_per_wg, MifxFeed feed, float dp_clip,
    float* __restrict__ norms_out) {
  static_assert(TRAIN || !DP, "DP is a training mode");
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, h = lane >> 4;
  const int nl = desc[0], bs = desc[1], wtot = desc[2];
  uint16_t* P0 = lds;
  uint16_t* P1 = lds + T * bs;
  uint16_t* P2 = lds + 2 * T * bs;
  float* wgrad = (float*)(lds + 3 * T * bs);
  float* red = wgrad + WIDE_PAD;
  int* wgi = (int*)wgrad;
  float* an = red + 16;  // DP only: an[l * T + row] = sum_k A_l[row][k]^2
  const uint16_t* wnk = wimg;         // W^T [N][K] per layer
  const uint16_t* wkn = wimg + wtot;  // W   [K][N] per layer
  const int stride = wtot + WIDE_PAD;
  uint16_t* scr = TRAIN ? scratch + (size_t)blockIdx.x * scratch_per_wg : nullptr;
  float* my = TRAIN ? slab + (size_t)blockIdx.x * stride : nullptr;

  if (TRAIN)
    for (int c = tid; c < WIDE_PAD; c += NTHR) wgrad[c] = 0.f;

  MifxFeed fd = feed;
  MifxFeedStep fs;
  if (step_ctr) {
    fs = mifx_feed_step(fd, step_ctr[0], n_data);
  } else {  // a fixed start (eval / predict) reads records start_fixed.. in stored order
    fd.key = 0;
    fs.e0 = 0;
    fs.i0 = start_fixed;
    fs.h = 1;
    fs.ng = 1;
    fs.ek0 = fs.ek1 = 0;
  }
  const int ntiles = (int)((batch + T - 1) / T);
  // wide gradient: 32-bit fixed-point LDS histogram (integer adds commute, so the result does not depend on the
  // order in which lanes hit a bucket); scale = the largest power of two that keeps a whole-bucket sum below 2^30
  const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  // (DP: dl enters unscaled and clipped, |c dl| <= 1; grad_scale is applied by wdg_reduce_opt)
  const float qbound = fmaxf((DP ? 1.f : fabsf(grad_scale)) * (float)(max(my_tiles, 1) * T), 1e-30f);
  const float qscale = exp2f(fminf(floorf(log2f(1073741824.f / qbound)), 100.f));
  const float qinv = 1.f / qscale;
  const float qmax = 1073741824.f / (float)(max(my_tiles, 1) * T);
  float loss_sum = 0.f, dl_sum = 0.f;
  bool first = true;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long row = (long long)tile * T + 16 * w + r;
    const bool valid = row < batch;
    // rows past the batch read a valid record; they carry dl = 0 and are left out of loss and wide gradient
    const long long di = mifx_feed_record(fd, fs, min(row, batch - 1), n_data);
    const uint4 u0 = data[2 * di], u1 = data[2 * di + 1];
    const uint32_t idw[5] = {u0.w, u1.x, u1.y, u1.z, u1.w};
    int ids[9];
    float wl = wide[WIDE_BIAS];
#pragma unroll
    for (int f = 0; f < 9; ++f) {
      int id = (f & 1) ? (idw[f >> 1] >> 16) : (idw[f >> 1] & 0xffff);
      id = id < kWideNb[f] ? id : 0;
      ids[f] = kWideOff[f] + id;
      wl += wide[ids[f]];
    }
    __syncthreads();  // the previous tile's backward is done with the LDS images (and wgrad is zeroed)
    {
      // A_0 row: dense floats, the constant 1, zeros up to K_0 = 32 (lane h writes 16-byte chunk h)
      v8bf x = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
      if (h == 0) {
        x[0] = (bf16)__uint_as_float(u0.x);
        x[1] = (bf16)__uint_as_float(u0.y);
        x[2] = (bf16)__uint_as_float(u0.z);
        x[3] = (bf16)1.0f;
      }
      *(v8bf*)(P0 + (16 * w + r) * bs + 8 * h) = x;
      if (TRAIN) *(v8bf*)(scr + desc[DESC_HDR + 5] + (16 * w + r) * 32 + 8 * h) = x;
      if (DP && h == 0) {
        const float x0 = (float)x[0], x1 = (float)x[1], x2 = (float)x[2];
        an[16 * w + r] = x0 * x0 + x1 * x1 + x2 * x2 + 1.f;
      }
    }
    wave_sync();
    // ---- forward (wave-local): A_l in P[l & 1]
    for (int l = 0; l + 1 < nl; ++l) {
      const int* dl_ = desc + DESC_HDR + DESC_LAYER * l;
      const int K = dl_[0], N = dl_[1], off = dl_[2], so = dl_[DESC_LAYER + 5];
      const uint16_t* in = (l & 1) ? P1 : P0;
      uint16_t* out = (l & 1) ? P0 : P1;
      float asq = 0.f;
      rows_gemm(wnk + off, K, N / 16, K / 32, in + 16 * w * bs, bs, r, h, [&](int t, v4f acc) {
        v4bf o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (bf16)fmaxf(acc[i], 0.f);
        *(v4bf*)(out + (16 * w + r) * bs + 16 * t + 4 * h) = o;
        if (TRAIN) *(v4bf*)(scr + so + (16 * w + r) * N + 16 * t + 4 * h) = o;
        if (DP) {
#pragma unroll
          for (int i = 0; i < 4; ++i) asq += (float)o[i] * (float)o[i];
        }
      });
      if (DP) {  // the row's four column quarters sit in lanes r, r + 16, r + 32, r + 48
        asq += __shfl_xor(asq, 16);
        asq += __shfl_xor(asq, 32);
        if (h == 0) an[(l + 1) * T + 16 * w + r] = asq;
      }
      wave_sync();
    }
    v4f z = {0.f, 0.f, 0.f, 0.f};
    {
      const int* dh = desc + DESC_HDR + DESC_LAYER * (nl - 1);
      const uint16_t* in = ((nl - 1) & 1) ? P1 : P0;
      rows_gemm(wnk + dh[2], dh[0], 1, dh[0] / 32, in + 16 * w * bs, bs, r, h, [&](int, v4f acc) { z = acc; });
    }
    // ---- logit, loss, dl (every lane recomputes for example r; lane h == 0 owns it)
    const float x = __shfl(z[0], r) + wl;
    const float y = (float)(idw[4] >> 16);
    const float lossv = fmaxf(x, 0.f) - x * y + log1pf(__expf(-fabsf(x)));
    if (!TRAIN) {
      if (h == 0 && valid) {
        logits_out[row] = x;
        loss_sum += lossv;
      }
      continue;
    }
    const float dl = valid ? (1.f / (1.f + __expf(-x)) - y) * (DP ? 1.f : grad_scale) : 0.f;
    uint16_t* Acur = ((nl - 1) & 1) ? P1 : P0;
    uint16_t* Dcur = ((nl - 1) & 1) ? P0 : P1;
    uint16_t* Dnext = P2;
    float cf = 1.f;  // DP: the example's clip factor c_i
    if (DP) {
      // ---- norm sweep (wave-local): the dZ chain of the backward below, no dW; Acur is left alone, the chain
      // alternates between Dcur and Dnext, the ReLU mask of A_l comes from the scratch (this lane's own stores)
      const float dlb = (float)(bf16)dl;
      float n2 = 10.f * dl * dl + dlb * dlb * an[(nl - 1) * T + 16 * w + r];
      uint16_t* Dc = Dcur;
      uint16_t* Dn = Dnext;
      {
        v8bf d0 = {(bf16)(h == 0 ? dl : 0.f), (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f,
                   (bf16)0.f};
        *(v8bf*)(Dc + (16 * w + r) * bs + 8 * h) = d0;
      }
      wave_sync();
      for (int l = nl - 1; l > 0; --l) {
        const int* dl_ = desc + DESC_HDR + DESC_LAYER * l;
        const int K = dl_[0], N = dl_[1], off = dl_[2], so = dl_[5], outp = dl_[-DESC_LAYER + 6];
        float dsq = 0.f;
        rows_gemm(wkn + off, N, K / 16, N / 32, Dc + 16 * w * bs, bs, r, h, [&](int t, v4f acc) {
          const uint2 m = *(const uint2*)(scr + so + (16 * w + r) * K + 16 * t + 4 * h);
          v4bf o;
          o[0] = (bf16)((m.x & 0xffffu) ? acc[0] : 0.f);
          o[1] = (bf16)((m.x >> 16) ? acc[1] : 0.f);
          o[2] = (bf16)((m.y & 0xffffu) ? acc[2] : 0.f);
          o[3] = (bf16)((m.y >> 16) ? acc[3] : 0.f);
          *(v4bf*)(Dn + (16 * w + r) * bs + 16 * t + 4 * h) = o;
#pragma unroll
          for (int i = 0; i < 4; ++i) {  // trainable outputs only: column outp feeds the constant-1 producer
            const float v = (16 * t + 4 * h + i < outp) ? (float)o[i] : 0.f;
            dsq += v * v;
          }
        });
        dsq += __shfl_xor(dsq, 16);
        dsq += __shfl_xor(dsq, 32);
        n2 += dsq * an[(l - 1) * T + 16 * w + r];
        wave_sync();
        uint16_t* t_ = Dc;
        Dc = Dn;
        Dn = t_;
      }
      const float nrm = sqrtf(n2), thr = DP_SHRINK * dp_clip;
      cf = nrm > thr ? thr / nrm : 1.f;  // rows past the batch: dl = 0, n = 0, c = 1 and nothing to scale
      if (h == 0 && valid) norms_out[row] = nrm;
    }
    const float dlc = DP ? cf * dl : dl;
    if (h == 0 && valid) {
      loss_sum += lossv;
      const int qv = __float2int_rn(fminf(fmaxf(dlc * qscale, -qmax), qmax));
#pragma unroll
      for (int f = 0; f < 9; ++f) atomicAdd(&wgi[ids[f]], qv);
      dl_sum += dlc;
    }
    // ---- backward: A_l in Acur, dZ_l in Dcur, dZ_{l-1} into Dnext
    {
      v8bf d0 = {(bf16)(h == 0 ? dl : 0.f), (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f,
                 (bf16)0.f};
      *(v8bf*)(Dcur + (16 * w + r) * bs + 8 * h) = d0;  // the head's dZ image: 32 columns, column 0 live
    }
    for (int l = nl - 1; l >= 0; --l) {
      const int* dl_ = desc + DESC_HDR + DESC_LAYER * l;
      const int K = dl_[0], N = dl_[1], off = dl_[2];
      __syncthreads();  // all 64 rows of Acur / Dcur are in place
      if (!DP) dw_layer(Dcur, Acur, bs, dl_[3], dl_[4], K, my + off, first, w, r, h);
      if (l > 0) {
        rows_gemm(wkn + off, N, K / 16, N / 32, Dcur + 16 * w * bs, bs, r, h, [&](int t, v4f acc) {
          const int o_ = (16 * w + r) * bs + 16 * t + 4 * h;
          const uint2 m = *(const uint2*)(Acur + o_);
          v4bf o;
          o[0] = (bf16)((m.x & 0xffffu) ? acc[0] : 0.f);
          o[1] = (bf16)((m.x >> 16) ? acc[1] : 0.f);
          o[2] = (bf16)((m.y & 0xffffu) ? acc[2] : 0.f);
          o[3] = (bf16)((m.y >> 16) ? acc[3] : 0.f);
          *(v4bf*)(Dnext + o_) = o;
        });
      }
      if (DP) {
        // the chain above read dZ_l unscaled; now this wave scales its own rows of the live dW columns in place,
        // dZ_l[i, :] <- bf16(c_i dZ_l[i, :]) (c_i = 1: untouched), and dW_l reads all 64 rows after the barrier
        wave_sync();
        if (cf != 1.f) {
          for (int g = h; g < 2 * dl_[3]; g += 4) {
            v8bf* pd = (v8bf*)(Dcur + (16 * w + r) * bs + 8 * g);
            v8bf d = *pd;
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = (bf16)(cf * (float)d[i]);
            *pd = d;
          }
        }
        __syncthreads();
        dw_layer(Dcur, Acur, bs, dl_[3], dl_[4], K, my + off, first, w, r, h);
      }
      if (l > 0) {
        __syncthreads();  // every wave is done reading Acur / Dcur
        const int Kp = dl_[-DESC_LAYER], so = dl_[-DESC_LAYER + 5], gpr = Kp / 8;
        for (int c = tid; c < T * gpr; c += NTHR) {
          const int rr = c / gpr, g = c - rr * gpr;
          *(uint4*)(Acur + rr * bs + 8 * g) = *(const uint4*)(scr + so + rr * Kp + 8 * g);
        }
        uint16_t* t_ = Dcur;
        Dcur = Dnext;
        Dnext = t_;
      }
    }
    first = false;
  }

  // ---- epilogue: loss, wide part of the slab
  for (int o = 32; o > 0; o >>= 1) {
    loss_sum += __shfl_xor(loss_sum, o);
    dl_sum += __shfl_xor(dl_sum, o);
  }
  __syncthreads();
  if (lane == 0) {
    red[w] = loss_sum;
    red[4 + w] = dl_sum;
  }
  __syncthreads();
  if (TRAIN) {
    for (int c = tid; c < WIDE_PAD; c += NTHR) {
      float v = (float)wgi[c] * qinv;
      if (c == WIDE_BIAS) v += red[4] + red[5] + red[6] + red[7];
      my[wtot + c] = v;
    }
  }
  if (tid == 0 && slab_loss) slab_loss[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// slab [G][stride] -> column sums in row order; out != null: the plain sum, else optimizer + both bf16 images.
// dp_mode 0: as ever. 1 / 2 (DP): the sums are the clipped per-example gradients; 2 adds noise_std N(0,1) to every
// column with kind != -1 (never to padding or the constant-1 producers: the ones must not drift), drawn at the
// step the slot holds before this pass increments it; both then multiply by gscale.
template <bool DP>  // DP = false: dp_mode is 0 and the code is the non-private pass
__global__ __launch_bounds__(256) void wdg_reduce_opt(const float4* __restrict__ slab, int G, int stride,
                                                      float4* __restrict__ out, const int* __restrict__ kind,
                                                      float* __restrict__ param, float* __restrict__ s0,
                                                      float* __restrict__ s1, uint16_t* __restrict__ wimg, int wtot,
                                                      long long* __restrict__ step_ctr, OptHyper hd, OptHyper hw,
                                                      int dp_mode, float noise_std, float gscale, uint32_t seed_lo,
                                                      uint32_t seed_hi) {
  __shared__ long long s_step;
  const bool opt = out == nullptr;
  const bool noisy = DP && dp_mode == 2;
  if ((opt || noisy) && threadIdx.x == 0)
    s_step = step_ctr[blockIdx.x] + (opt ? 1 : 0);  // the slot's only reader and writer: thread 0
  __syncthreads();
  const long long step = opt ? s_step : 0;
  const unsigned long long noff = noisy ? (unsigned long long)(opt ? s_step - 1 : s_step) : 0ull;
  const int nq = stride / 4;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < nq; c += gridDim.x * 256) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    int g = 0;
    for (; g + 4 <= G; g += 4) {
      float4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = slab[(size_t)(g + j) * nq + c];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a.x += v[j].x;
        a.y += v[j].y;
        a.z += v[j].z;
        a.w += v[j].w;
      }
    }
    for (; g < G; ++g) {
      const float4 v = slab[(size_t)g * nq + c];
      a.x += v.x;
      a.y += v.y;
      a.z += v.z;
      a.w += v.w;
    }
    float gr[4] = {a.x, a.y, a.z, a.w};
    if (DP) {
      float z[4] = {0.f, 0.f, 0.f, 0.f};
      if (noisy) {
        const U4 rn = philox(U4{(uint32_t)c, 0u, (uint32_t)noff, (uint32_t)(noff >> 32)}, seed_lo, seed_hi);
        box_muller(rn.x, rn.y, z[0], z[1]);
        box_muller(rn.z, rn.w, z[2], z[3]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (noisy && kind[4 * c + e] != -1) gr[e] += noise_std * z[e];
        gr[e] *= gscale;
      }
    }
    if (!opt) {
      out[c] = make_float4(gr[0], gr[1], gr[2], gr[3]);
      continue;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int gi = 4 * c + e;
      const int kd = kind[gi];
      if (kd == -1) continue;
      float a0 = s0[gi], a1 = s1[gi];
      const float wn = opt_update(kd >= 0 ? hd : hw, param[gi], gr[e], a0, a1, step);
      s0[gi] = a0;
      s1[gi] = a1;
      param[gi] = wn;
      if (kd >= 0) {
        const uint16_t b = __builtin_bit_cast(uint16_t, (bf16)wn);
        wimg[gi] = b;
        wimg[wtot + kd] = b;
      }
    }
  }
  if (opt && threadIdx.x == 0) step_ctr[blockIdx.x] = step;
}

// descriptor checks shared by the launchers; returns the LDS bytes (0: invalid) and the scratch elements
int desc_check(const int* d, int* scratch_elems) {
  if (d == nullptr) return 0;
  const int nl = d[0], bs = d[1], wtot = d[2];
  if (nl < 2 || nl > MAXL) return 0;
  int off = 0, so = 0, kmax = 0;
  for (int l = 0; l < nl; ++l) {
    const int* p = d + DESC_HDR + DESC_LAYER * l;
    const int K = p[0], N = p[1];
    if (K < 32 || K > KMAX || K % 32 != 0 || N < 32 || N > KMAX || N % 32 != 0) return 0;
    if (l == 0 && K != 32) return 0;
    if (l + 1 < nl ? N != p[DESC_LAYER] : N != 32) return 0;
    if (p[2] != off || p[5] != so) return 0;
    if (p[3] < 1 || p[3] > N / 16 || p[4] < 1 || p[4] > K / 16) return 0;
    if (p[6] < 1 || (p[6] + 15) / 16 != p[3] || (l + 1 == nl && p[6] != 1)) return 0;
    off += K * N;
    so += T * K;
    kmax = K > kmax ? K : kmax;
  }
  if (wtot != off || bs != kmax + PAD) return 0;
  *scratch_elems = so;
  return 3 * T * bs * 2 + WIDE_PAD * 4 + 64;
}

}  // namespace

extern "C" {

int mifx_wdg_constants(int* out, int n) {
  // DP_SHRINK goes out as the bit pattern of the float
  const int v[] = {T, NTHR, PAD, MAXH, MAXW, KMAX, NWIDE, WIDE_BIAS, WIDE_PAD, SLOTS, SLAB_BOUND_MB,
                   DESC_HDR, DESC_LAYER, DESC_LEN, __builtin_bit_cast(int, DP_SHRINK)};
  const int m = (int)(sizeof(v) / sizeof(int));
  for (int i = 0; i < n && i < m; ++i) out[i] = v[i];
  return m;
}

// desc_host / desc_dev: the same DESC_LEN int32 descriptor on the host (checked here) and on the device (read by
// the kernel). wimg: bf16 [2][WTOT]; slab: fp32 [>= grid][WTOT + WIDE_PAD]; scratch: bf16 [>= grid][sum 64 K_l].
// train: 0 eval / predict, 1 training, 2 DP training (per-example clipping to l2_norm_clip > 0; norms_out: fp32
// [>= batch], the per-example gradient norms before clipping, by position in the batch; grad_scale is then left to
// mifx_wdg_reduce_opt).
int mifx_wdg_fused(const void* data, long long n_data, long long batch, long long start_fixed,
                   const long long* step_ctr, const void* wimg, const float* wide, float* slab, float* slab_loss,
                   float* logits_out, float grad_scale, int grid, int train, const int* desc_host,
                   const int* desc_dev, void* scratch, long long feed_stride, long long feed_offset,
                   unsigned long long shuffle_key, hipStream_t stream, float l2_norm_clip, float* norms_out) {
  int scratch_elems = 0;
  int lds_bytes = desc_check(desc_host, &scratch_elems);
  if (train < 0 || train > 2) return -1;
  if (train == 2 && (!(l2_norm_clip > 0.f) || norms_out == nullptr)) return -1;
  if (lds_bytes == 0 || desc_dev == nullptr || data == nullptr || wimg == nullptr || wide == nullptr) return -1;
  if (grid <= 0 || n_data <= 0 || batch <= 0 || batch > n_data || grid > (batch + T - 1) / T) return -1;
  if (feed_stride < batch || feed_offset < 0 || feed_offset + batch > feed_stride) return -1;
  const long long stride = (long long)desc_host[2] + WIDE_PAD;
  if (train) {
    if (slab == nullptr || scratch == nullptr || step_ctr == nullptr) return -1;
    if ((long long)grid * stride * 4 > (long long)SLAB_BOUND_MB * 1024 * 1024) return -1;
  } else if (logits_out == nullptr) {
    return -1;
  }
  const MifxFeed fd{feed_stride, feed_offset, shuffle_key};
  static bool attr_done = false;  // the launch's LDS size follows the tower; the limit is the widest tower's
  if (!attr_done) {
    constexpr int MAX_LDS = 3 * T * (KMAX + PAD) * 2 + WIDE_PAD * 4 + 64;
    static_assert(MAX_LDS + DP_LDS <= 163840, "LDS budget");
    (void)hipFuncSetAttribute((const void*)wdg_fused<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              MAX_LDS);
    (void)hipFuncSetAttribute((const void*)wdg_fused<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              MAX_LDS);
    (void)hipFuncSetAttribute((const void*)wdg_fused<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              MAX_LDS + DP_LDS);
    attr_done = true;
  }
  if (train == 2) {
    lds_bytes += DP_LDS;
    hipLaunchKernelGGL((wdg_fused<true, true>), dim3(grid), dim3(NTHR), lds_bytes, stream, (const uint4*)data,
                       n_data, batch, start_fixed, step_ctr, (const uint16_t*)wimg, wide, slab, slab_loss, logits_out,
                       grad_scale, desc_dev, (uint16_t*)scratch, scratch_elems, fd, l2_norm_clip, norms_out);
  } else if (train) {
    hipLaunchKernelGGL((wdg_fused<true, false>), dim3(grid), dim3(NTHR), lds_bytes, stream, (const uint4*)data,
                       n_data, batch, start_fixed, step_ctr, (const uint16_t*)wimg, wide, slab, slab_loss, logits_out,
                       grad_scale, desc_dev, (uint16_t*)scratch, scratch_elems, fd, 0.f, (float*)nullptr);
  } else {
    hipLaunchKernelGGL((wdg_fused<false, false>), dim3(grid), dim3(NTHR), lds_bytes, stream, (const uint4*)data,
                       n_data, batch, start_fixed, step_ctr, (const uint16_t*)wimg, wide, slab, slab_loss, logits_out,
                       grad_scale, desc_dev, (uint16_t*)scratch, scratch_elems, fd, 0.f, (float*)nullptr);
  }
  return (int)hipGetLastError();
}

// slab [G][stride] summed in row order. out != null: the plain sum [stride]; else the optimizer on the
// slab-column-order state (kind / param / s0 / s1 [stride]) and both bf16 images (wimg [2][wtot]).
// step_ctr: SLOTS int64 step slots, all equal. dp_mode 0: no DP; 1: DP sums times grad_scale; 2: DP sums plus
// noise_std N(0,1) on the columns with kind != -1 (stream: seed, the step in the slots), times grad_scale; mode 2
// of the plain sum reads kind and step_ctr as well (and leaves the slots alone).
int mifx_wdg_reduce_opt(const float* slab, int G, int stride, float* out, const int* kind, float* param, float* s0,
                        float* s1, void* wimg, int wtot, long long* step_ctr, const float* hyper_dnn,
                        const float* hyper_wide, hipStream_t stream, int dp_mode, float noise_std, float grad_scale,
                        unsigned long long seed) {
  if (slab == nullptr || G <= 0 || stride <= 0 || stride % 4 != 0) return -1;
  if (dp_mode < 0 || dp_mode > 2 || (dp_mode == 2 && (kind == nullptr || step_ctr == nullptr || !(noise_std >= 0.f))))
    return -1;
  const uint32_t slo = (uint32_t)seed, shi = (uint32_t)(seed >> 32);
  if (out == nullptr && (kind == nullptr || param == nullptr || s0 == nullptr || s1 == nullptr || wimg == nullptr ||
                         step_ctr == nullptr || hyper_dnn == nullptr || hyper_wide == nullptr ||
                         wtot + WIDE_PAD != stride))
    return -1;
  int grid = (stride / 4 + 255) / 256;
  if (grid > SLOTS) grid = SLOTS;
  auto kern = dp_mode != 0 ? wdg_reduce_opt<true> : wdg_reduce_opt<false>;
  if (out != nullptr)
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, stream, (const float4*)slab, G, stride, (float4*)out,
                       dp_mode == 2 ? kind : nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                       dp_mode == 2 ? step_ctr : nullptr, OptHyper{}, OptHyper{}, dp_mode, noise_std, grad_scale, slo,
                       shi);
  else
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, stream, (const float4*)slab, G, stride, nullptr, kind,
                       param, s0, s1, (uint16_t*)wimg, wtot, step_ctr, opt_hyper(hyper_dnn), opt_hyper(hyper_wide),
                       dp_mode, noise_std, grad_scale, slo, shi);
  return (int)hipGetLastError();
}

}  // extern "C"
