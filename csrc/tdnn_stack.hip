// KFP taxi DNN with more than one hidden layer (`hidden_layer_size` = "H1,H2,..,HL"): layers 2..L and the head.
//
// The first layer (one-hot gather, sparse-row Adagrad with in-kernel row dedup, dense rows / b1) is
// csrc/embag_mlp.hip's, through its mifx_tdnn_l1_* entry points. This file holds, for an upper layer with input width
// Hin, output width Hout, batch B and row-major W [Hin, Hout] (a @ W):
//   forward         a_out = relu(a_in @ W + b)
//   input gradient  dz_in = (dz_out @ W^T) * [a_in > 0]          (W read transposed, never materialised)
//   update          g = a_in^T @ dz_out over the whole batch in registers, then acc += g^2; w -= lr g rsqrt(acc)
//                   in the epilogue: dW never reaches HBM, W and acc are read and written once per element
// and the head over a_L: logit, stable BCE, dlogit, dz_L; the w2 / b2 update is the fused update kernel on the
// [H_L, 1] "layer" w2 with dz_out = dlogit [B, 1] (its bias gradient, the column sum of dlogit, is b2's).
//
// Storage and arithmetic are fp32 (TF Adagrad semantics, the CPU oracle): the products run on the exact-f32 MFMA
// v_mfma_f32_16x16x4_f32. Per k-step of 4, lane l holds A[row l % 16][k l / 16] and B[k l / 16][col l % 16]; the
// accumulator lane holds C[4 (l / 16) + i][l % 16], i = 0..3 (as csrc/gemm_f32.hip).
//
// One wave owns one 16 x 16 output tile and walks k in ascending order with one accumulator: every output element is
// one k-ordered chain, there is no split over k (the update: no split over the batch) and there are no atomics, so a
// step is bit-reproducible, eagerly or replayed from a graph. A workgroup is 4 waves = a 16 x 64 tile (64 consecutive
// output columns = 256 B rows for the update's W / acc traffic); operands go from global memory straight to the MFMA
// (each is used by one wave once; the 16-row reuse is the cache's), kInFlight k-steps of loads in flight per wave: a
// wave's k walk is one dependent chain, so at the reference batch its length in load round trips is the kernel's
// time. Edges in every dimension are zero-filled on load and masked on store. At the reference batch of 32 the
// products are tiny and the update's 16 B per parameter is the cost: the tile is small so that even a 200 x 100 layer
// spreads over many CUs.
#include <hip/hip_runtime.h>
#include "tdnn_common.h"
#include <stdint.h>

namespace {

constexpr int kMaxLayers = 8;
constexpr int kMaxBatch = 8192;  // the first layer's bound (embag_mlp.hip kMaxList)
constexpr int kTile = 16;
constexpr int kWaves = kThreads / 64;  // waves per workgroup of the layer kernels (each wave: its own 16 x 16 tile)
constexpr int kInFlight = 32;  // k-steps (of 4) whose operand loads a wave issues before it waits: 2 x 32 VGPRs

typedef float f32x4 __attribute__((ext_vector_type(4)));

// C[16 x 16] = sum_k A[m][k] B[k][n] for this wave's tile, k = 0..K-1 ascending. la(k) / lb(k) load this lane's
// operand A[m = lane % 16][k] / B[k][n = lane % 16] for 0 <= k < K; a lane whose row m / column n lies outside the
// matrix loads a clamped (valid) address and passes va / vb = false, and the last, partial round clamps k: what is
// outside is zeroed by a select after the load, so the loads are straight-line code (a predicated load per operand
// compiled to a branch each, and a lone wave per SIMD spent its time issuing them).
template <class LA, class LB>
__device__ __forceinline__ f32x4 wave_tile(int K, bool va, bool vb, LA la, LB lb) {
  const int kq = (threadIdx.x & 63) >> 4;
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  constexpr int U = kInFlight;
  float a[U], b[U];
  int k0 = 0;
  for (; k0 + 4 * U <= K; k0 += 4 * U) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      a[u] = la(k0 + 4 * u + kq);
      b[u] = lb(k0 + 4 * u + kq);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(va ? a[u] : 0.f, vb ? b[u] : 0.f, c, 0, 0, 0);
  }
  if (k0 < K) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = min(k0 + 4 * u + kq, K - 1);
      a[u] = la(k);
      b[u] = lb(k);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (k0 + 4 * u < K) {  // (wave-uniform)
        const bool in = k0 + 4 * u + kq < K;
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(va && in ? a[u] : 0.f, vb && in ? b[u] : 0.f, c, 0, 0, 0);
      }
  }
  return c;
}

// grid (ceil(Hout/64), ceil(B/16)): a_out = relu(a_in @ W + b)
__global__ __launch_bounds__(64 * kWaves) void tdnn_layer_fwd(const float* __restrict__ a_in,
                                                          const float* __restrict__ W, const float* __restrict__ b,
                                                          float* __restrict__ a_out, int B, int Hin, int Hout) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * kWaves + w) * kTile, m0 = blockIdx.y * kTile;
  if (n0 >= Hout) return;
  const int m = m0 + (lane & 15), n = n0 + (lane & 15);
  const int mc = min(m, B - 1), nc = min(n, Hout - 1);
  const f32x4 c = wave_tile(
      Hin, m < B, n < Hout, [&](int k) { return a_in[(size_t)mc * Hin + k]; },
      [&](int k) { return W[(size_t)k * Hout + nc]; });
  if (n >= Hout) return;
  const float bias = b[n];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = m0 + 4 * (lane >> 4) + i;
    if (r < B) a_out[(size_t)r * Hout + n] = fmaxf(c[i] + bias, 0.f);
  }
}

// grid (ceil(Hin/64), ceil(B/16)): dz_in = (dz_out @ W^T) * [a_in > 0]
__global__ __launch_bounds__(64 * kWaves) void tdnn_layer_dgrad(const float* __restrict__ dz_out,
                                                            const float* __restrict__ W,
                                                            const float* __restrict__ a_in,
                                                            float* __restrict__ dz_in, int B, int Hin, int Hout) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * kWaves + w) * kTile, m0 = blockIdx.y * kTile;
  if (n0 >= Hin) return;
  const int m = m0 + (lane & 15), n = n0 + (lane & 15);
  const int mc = min(m, B - 1), nc = min(n, Hin - 1);
  const f32x4 c = wave_tile(
      Hout, m < B, n < Hin, [&](int k) { return dz_out[(size_t)mc * Hout + k]; },
      [&](int k) { return W[(size_t)nc * Hout + k]; });  // B[k][n] = W[n][k]
  if (n >= Hin) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = m0 + 4 * (lane >> 4) + i;
    if (r < B) dz_in[(size_t)r * Hin + n] = a_in[(size_t)r * Hin + n] > 0.f ? c[i] : 0.f;
  }
}

// grid (ceil(Hout/64), ceil(Hin/16)): the wave's 16 x 16 tile of W. g = a_in^T @ dz_out over the batch (ascending b,
// in registers), then Adagrad on W / acc in place. The waves of tile row 0 also take the bias gradient, the column
// sum of dz_out, as a second product with an all-ones A (the same ascending-b chain), and update b / accb.
__global__ __launch_bounds__(64 * kWaves) void tdnn_layer_wgrad_adagrad(const float* __restrict__ a_in,
                                                                    const float* __restrict__ dz_out,
                                                                    float* __restrict__ W, float* __restrict__ accW,
                                                                    float* __restrict__ b, float* __restrict__ accb,
                                                                    int B, int Hin, int Hout, float lr) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * kWaves + w) * kTile, m0 = blockIdx.y * kTile;
  if (n0 >= Hout) return;
  const int m = m0 + (lane & 15), n = n0 + (lane & 15);
  const int mc = min(m, Hin - 1), nc = min(n, Hout - 1);
  const auto ldz = [&](int k) { return dz_out[(size_t)k * Hout + nc]; };
  const f32x4 c = wave_tile(B, m < Hin, n < Hout, [&](int k) { return a_in[(size_t)k * Hin + mc]; }, ldz);
  if (n < Hout) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = m0 + 4 * (lane >> 4) + i;
      if (r < Hin) {
        const size_t e = (size_t)r * Hout + n;
        adagrad_one(W + e, accW + e, c[i], lr);
      }
    }
  }
  if (blockIdx.y == 0) {
    const f32x4 s = wave_tile(B, true, n < Hout, [&](int) { return 1.f; }, ldz);  // every row of s is the column sum
    if (lane < 16 && n < Hout) adagrad_one(b + n, accb + n, s[0], lr);
  }
}

// grid (B): logit_b = a_L[b] . w2 + b2 (fixed order: strided per-thread partials, then block_sum), BCE, dlogit and
// dz_L = dlogit * w2 * [a_L > 0] (tdnn_head_bwd of embag_mlp.hip for a last layer of any width)
__global__ __launch_bounds__(kThreads) void tdnn_stack_head(const float* __restrict__ a, const float* __restrict__ w2,
                                                           const float* __restrict__ b2, const float* __restrict__ y,
                                                           BatchSel sel, int H, float grad_scale, int train,
                                                           float* __restrict__ dz_out, float* __restrict__ logit_out,
                                                           float* __restrict__ dlogit_out,
                                                           float* __restrict__ loss_out) {
  __shared__ float red[kThreads / 64];
  const int b = blockIdx.x;
  float p = 0.f;
  for (int h = threadIdx.x; h < H; h += kThreads) p += a[(size_t)b * H + h] * w2[h];
  const float logit = b2[0] + block_sum(p, red);
  if (threadIdx.x == 0) logit_out[b] = logit;
  if (!train) return;
  const float yy = y[sel.rec(sel.start(), b)];
  const float dl = (1.f / (1.f + expf(-logit)) - yy) * grad_scale;
  if (threadIdx.x == 0) {
    // stable BCE with logits: max(l,0) - l*y + log1p(exp(-|l|))
    loss_out[b] = fmaxf(logit, 0.f) - logit * yy + log1pf(expf(-fabsf(logit)));
    dlogit_out[b] = dl;
  }
  for (int h = threadIdx.x; h < H; h += kThreads)
    dz_out[(size_t)b * H + h] = a[(size_t)b * H + h] > 0.f ? dl * w2[h] : 0.f;
}

bool stack_ok(int L, const int* widths, int B) {
  if (L < 1 || L > kMaxLayers || B < 1 || B > kMaxBatch || widths == nullptr) return false;
  for (int k = 0; k < L; ++k)
    if (widths[k] < 1 || widths[k] > kMaxH) return false;
  return true;
}

dim3 tile_grid(int cols, int rows) { return dim3((cols + kWaves * kTile - 1) / (kWaves * kTile), (rows + kTile - 1) / kTile); }

}  // namespace

extern "C" {

int mifx_tdnn_stack_limits(int* out) {
  out[0] = kMaxLayers;
  out[1] = kMaxH;
  out[2] = kMaxBatch;
  return 0;
}

// widths [L] = H1..HL; act [L] = a_1..a_L ([B, H_k], a_1 filled by mifx_tdnn_l1_fwd); Wh / bh [L - 1] = layers 2..L.
// The pointer arrays are host arrays of device pointers.
int mifx_tdnn_stack_fwd(int L, const int* widths, int B, float* const* act, const float* const* Wh,
                        const float* const* bh, hipStream_t st) {
  if (!stack_ok(L, widths, B)) return -1;
  for (int k = 1; k < L; ++k)
    hipLaunchKernelGGL(tdnn_layer_fwd, tile_grid(widths[k], B), dim3(64 * kWaves), 0, st, act[k - 1], Wh[k - 1],
                       bh[k - 1], act[k], B, widths[k - 1], widths[k]);
  return (int)hipGetLastError();
}

// The head over a_L [B, H]: logit (always); with train: loss, dlogit, dz_L, then the w2 / b2 Adagrad update. y [n]
// and the record selection are mifx_tdnn_fwd_bwd's.
int mifx_tdnn_stack_head(const float* aL, float* w2, float* accw2, float* b2, float* accb2, const float* y,
                         long long n, const long long* step_ctr, long long start_fixed, int B, int H,
                         float grad_scale, int train, float lr, float* dz_out, float* logit_out, float* dlogit_out,
                         float* loss_out, long long feed_stride, long long feed_offset,
                         unsigned long long shuffle_key, hipStream_t st) {
  if (H < 1 || H > kMaxH || B < 1 || B > kMaxBatch) return -1;
  if (train && (n < B || start_fixed < 0 || start_fixed >= n || feed_stride < B || feed_offset < 0 ||
                feed_offset + B > feed_stride))
    return -1;
  const BatchSel sel{n, step_ctr, start_fixed, B, MifxFeed{feed_stride, feed_offset, shuffle_key}, nullptr};
  hipLaunchKernelGGL(tdnn_stack_head, dim3(B), dim3(kThreads), 0, st, aL, w2, b2, y, sel, H, grad_scale, train,
                     dz_out, logit_out, dlogit_out, loss_out);
  if (train)  // after tdnn_stack_head, which read w2 for dz_L
    hipLaunchKernelGGL(tdnn_layer_wgrad_adagrad, tile_grid(1, H), dim3(64 * kWaves), 0, st, aL, dlogit_out, w2,
                       accw2, b2, accb2, B, H, 1, lr);
  return (int)hipGetLastError();
}

// For k = L..2: dz_{k-1} from dz_k and Wh (before the update overwrites it), then the fused update of layer k.
// dz [L] = dz_1..dz_L ([B, H_k]; dz_L filled by mifx_tdnn_stack_head, dz_1 goes to mifx_tdnn_l1_adagrad).
int mifx_tdnn_stack_bwd(int L, const int* widths, int B, const float* const* act, float* const* dz,
                        float* const* Wh, float* const* accWh, float* const* bh, float* const* accbh, float lr,
                        hipStream_t st) {
  if (!stack_ok(L, widths, B)) return -1;
  for (int k = L - 1; k >= 1; --k) {
    const int Hin = widths[k - 1], Hout = widths[k];
    hipLaunchKernelGGL(tdnn_layer_dgrad, tile_grid(Hin, B), dim3(64 * kWaves), 0, st, dz[k], Wh[k - 1], act[k - 1],
                       dz[k - 1], B, Hin, Hout);
    hipLaunchKernelGGL(tdnn_layer_wgrad_adagrad, tile_grid(Hout, Hin), dim3(64 * kWaves), 0, st, act[k - 1], dz[k],
                       Wh[k - 1], accWh[k - 1], bh[k - 1], accbh[k - 1], B, Hin, Hout, lr);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
