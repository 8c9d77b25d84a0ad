// Image input pipeline kernels for gfx950: random-crop + horizontal flip + normalize, uint8 NHWC -> bf16 NHWC
// (crop_flip_norm), and scale + aspect-ratio augmentation / eval resize: a sampled or given box per image resized
// bilinearly to the output (rrc_boxes + resample_flip_norm, below).
//
// BASELINE config 5 (ResNet-50 image pipeline, DP=8): the dataset lives in HBM as uint8 NHWC
// (288 GB per GPU holds ~1.9M 256x256x3 images), so the per-step input work is a gather of the
// batch's images fused with augmentation and normalisation into the bf16 channels_last tensor
// the first convolution consumes — one read of B*256*256*3 bytes and one write of B*224*224*3*2.
//
// grid (ceil(W_out*C / (kThreads*kVec)), H_out, B): block row = one output row of one image;
// each thread writes kVec consecutive channel-interleaved elements (16-byte bf16 stores).
// Per-image crop offsets and the flip bit come from an in-kernel Philox4x32-10 keyed by
// (seed) with counter (image slot, step), so augmentation is reproducible and needs no host RNG.
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kThreads = 128;
constexpr int kVec = 8;

struct U4 {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
    c = U4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

template <typename TOut>
__device__ __forceinline__ TOut cvt(float v);
template <>
__device__ __forceinline__ float cvt<float>(float v) {
  return v;
}
template <>
__device__ __forceinline__ __hip_bfloat16 cvt<__hip_bfloat16>(float v) {
  return __float2bfloat16(v);
}

template <typename TOut>
__global__ __launch_bounds__(kThreads) void crop_flip_norm(const uint8_t* __restrict__ src, const int* __restrict__ idx,
                                                          int Hin, int Win, int C, int Hout, int Wout, int train,
                                                          uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                                                          const long long* __restrict__ step_dev,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ inv_std,
                                                          TOut* __restrict__ out) {
  const int b = blockIdx.z, y = blockIdx.y;
  int oy, ox, flip;
  if (train) {
    if (step_dev) step = (uint32_t)step_dev[0];  // device step counter (captured hipGraph steps)
    const U4 r = philox(U4{(uint32_t)b, step, 0x1234u, 0u}, seed_lo, seed_hi);
    oy = (int)(r.x % (uint32_t)(Hin - Hout + 1));
    ox = (int)(r.y % (uint32_t)(Win - Wout + 1));
    flip = (int)(r.z & 1u);
  } else {
    oy = (Hin - Hout) / 2;
    ox = (Win - Wout) / 2;
    flip = 0;
  }
  const uint8_t* row = src + ((size_t)idx[b] * Hin + (oy + y)) * (size_t)Win * C;
  TOut* orow = out + ((size_t)b * Hout + y) * (size_t)Wout * C;
  const int rowlen = Wout * C;
  const int e0 = (blockIdx.x * kThreads + threadIdx.x) * kVec;
#pragma unroll
  for (int k = 0; k < kVec; ++k) {
    const int e = e0 + k;
    if (e < rowlen) {
      const int x = e / C, c = e - x * C;
      const int sx = ox + (flip ? (Wout - 1 - x) : x);
      const float v = (float)row[sx * C + c] * (1.0f / 255.0f);
      orow[e] = cvt<TOut>((v - mean[c]) * inv_std[c]);
    }
  }
}

// ---- random-resized-crop boxes + bilinear resample ---------------------------------------------------------------
// Box table: int32 [B, 5] = (x0, y0, w, h, flip) in device memory; rrc_boxes samples it, resample_flip_norm reads it
// (sampled, or given by the caller: the eval box, tests).

// fp32 with every operation rounded on its own, so the numpy twin (mifx.ops.image_ops.rrc_params) reproduces the
// boxes bit for bit: only + - * / sqrt, which hipcc rounds correctly by default (no exp / log / pow), written as
// plain operators under `fp contract(off)` -- hipcc otherwise fuses a * b + c into an FMA, and it does so through
// the __fmul_rn / __fadd_rn intrinsics too (their bodies carry the contract flag).
__device__ __forceinline__ float u01_24(uint32_t v) {  // [0, 1), exact
  return (float)(v >> 8) * (1.0f / 16777216.0f);
}

// One thread per batch slot. Up to 10 attempts, attempt k on Philox counter (b, step, 0x1235, k): area fraction
// uniform in [scale_lo, scale_hi] from word x; aspect ratio "mirrored" from word y (low bit: landscape
// q = 1 + (ratio_hi - 1) t, w^2 = area q, h^2 = area / q; or portrait q = 1 + (1 / ratio_lo - 1) t with the roles
// swapped), x0 / y0 from words z / w. After 10 misses the central crop with the image's ratio clamped into
// [ratio_lo, ratio_hi] (torchvision's fallback). flip: bit 0 of word z of crop_flip_norm's stream (b, step, 0x1234, 0).
__global__ __launch_bounds__(64) void rrc_boxes(int B, int Hin, int Win, uint32_t seed_lo, uint32_t seed_hi,
                                                uint32_t step, const long long* __restrict__ step_dev, float scale_lo,
                                                float scale_hi, float ratio_lo, float ratio_hi,
                                                int* __restrict__ boxes) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  if (step_dev) step = (uint32_t)step_dev[0];
  const float full = (float)(Hin * Win);  // (exact: the entry point bounds Hin * Win by 2^24)
  const float dscale = scale_hi - scale_lo;
  const float qhi = ratio_hi - 1.0f, qlo = 1.0f / ratio_lo - 1.0f;
  int x0 = 0, y0 = 0, w = 0, h = 0;
  bool ok = false;
  for (uint32_t k = 0; k < 10u && !ok; ++k) {
    const U4 r = philox(U4{(uint32_t)b, step, 0x1235u, k}, seed_lo, seed_hi);
    const float du = dscale * u01_24(r.x);
    const float area = (scale_lo + du) * full;
    const bool portrait = (r.y & 1u) != 0u;
    const float qt = (portrait ? qlo : qhi) * u01_24(r.y);
    const float q = 1.0f + qt;
    const float s_mul = sqrtf(area * q), s_div = sqrtf(area / q);
    const int a = (int)(s_mul + 0.5f), c = (int)(s_div + 0.5f);  // round: floor(v + 0.5), v >= 0
    w = portrait ? c : a;
    h = portrait ? a : c;
    if (w >= 1 && w <= Win && h >= 1 && h <= Hin) {
      ok = true;
      x0 = (int)(r.z % (uint32_t)(Win - w + 1));
      y0 = (int)(r.w % (uint32_t)(Hin - h + 1));
    }
  }
  if (!ok) {
    const float in_ratio = (float)Win / (float)Hin;
    w = Win;
    h = Hin;
    if (in_ratio < ratio_lo) {
      const float hf = (float)Win / ratio_lo;
      h = (int)(hf + 0.5f);
    } else if (in_ratio > ratio_hi) {
      const float wf = (float)Hin * ratio_hi;
      w = (int)(wf + 0.5f);
    }
    w = min(max(w, 1), Win);
    h = min(max(h, 1), Hin);
    x0 = (Win - w) / 2;
    y0 = (Hin - h) / 2;
  }
  const U4 f = philox(U4{(uint32_t)b, step, 0x1234u, 0u}, seed_lo, seed_hi);
  int* o = boxes + (size_t)b * 5;
  o[0] = x0;
  o[1] = y0;
  o[2] = w;
  o[3] = h;
  o[4] = (int)(f.z & 1u);
}

// Bilinear tap of output o along an axis of n_in box pixels and n_out outputs, half-pixel centres: source position
// ((2o + 1) n_in - n_out) / (2 n_out), split in integers so that the fraction is exact up to one rounding. Taps are
// clamped inside the box; the fraction is 0 left of the first pixel. rden = 1 / (2 n_out): the quotient
// (<= 2^14, numerator <= 2^29: the entry point's bounds) comes from one fp32 multiply, off by at most 1, and one
// correction step on the integer remainder instead of an integer division per pixel.
__device__ __forceinline__ void tap(int o, int n_in, int n_out, float rden, int& i0, int& i1, float& frac) {
  const int num = (2 * o + 1) * n_in - n_out, den = 2 * n_out;
  int i = (int)floorf((float)num * rden);
  int rem = num - i * den;
  if (rem < 0) {
    --i;
    rem += den;
  } else if (rem >= den) {
    ++i;
    rem -= den;
  }
  frac = i < 0 ? 0.0f : (float)rem / (float)den;
  i0 = min(max(i, 0), n_in - 1);
  i1 = min(max(i + 1, 0), n_in - 1);
}

// The 4 bytes at byte offset a of a staged row, from the two aligned dwords around them: byte and unaligned 16-bit
// LDS reads (what the compiler makes of per-channel byte loads) stall the LDS on every odd address, measured as
// SQ_LDS_UNALIGNED_STALL and 1.7x the kernel's time on boxes other than 224 or 112 wide.
__device__ __forceinline__ uint32_t bytes4(const uint32_t* row, int a) {
  const uint32_t* p = row + (a >> 2);
  return (uint32_t)((((uint64_t)p[1] << 32) | p[0]) >> (8 * (a & 3)));
}

constexpr int kMaxRowBytes = 4096;  // Win * C of the entry point
constexpr int kRsThreads = 64;      // one wave per block

// pixels per thread: a thread owns whole pixels (one tap computation per pixel, channels unrolled) and its
// P * C elements are a whole number of 16-byte (bf16, C = 3: 8-byte) stores
template <int C>
constexpr int kPix = C == 1 ? 8 : C == 4 ? 2 : 4;

__host__ __device__ constexpr int rs_row_stride(int row_bytes) {  // LDS bytes per staged row (16-byte chunks)
  return (row_bytes + 30 + 15) & ~15;
}

// grid (ceil(W_out / (kRsThreads * P)), H_out, B): one wave = (part of) one output row of one image. The two source
// rows it needs are two contiguous w * C byte segments: staged into LDS in aligned 16-byte chunks (one load per
// lane covers a 256 x 3 row), then every pixel gathers its four taps from LDS (bytes4). A chunk may reach past the
// row's ends into the neighbouring rows of the dataset (valid memory, never used); only a chunk crossing the ends
// of the dataset itself is read byte by byte.
// No antialiasing: fine for the 256^2 -> 224^2 geometry (box side / output side <= 1.14); downscaling by more than
// about 2x would alias without a prefilter.
template <typename TOut, int C>
__global__ __launch_bounds__(kRsThreads) void resample_flip_norm(const uint8_t* __restrict__ src,
                                                                const int* __restrict__ idx,
                                                                const int* __restrict__ boxes, int box_stride, int N,
                                                                int Hin, int Win, int Hout, int Wout,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ inv_std,
                                                                TOut* __restrict__ out) {
  extern __shared__ __align__(16) uint8_t lds[];
  constexpr int P = kPix<C>, E = P * C;
  constexpr int SB = (E * sizeof(TOut)) % 16 == 0 ? 16 : 8;  // bytes per store
  const int b = blockIdx.z, y = blockIdx.y;
  const int* bx = boxes + (size_t)b * box_stride;
  // a box from the caller is clamped into the image: nothing is read outside it whatever the table holds
  const int x0 = min(max(bx[0], 0), Win - 1), y0 = min(max(bx[1], 0), Hin - 1);
  const int w = min(max(bx[2], 1), Win - x0), h = min(max(bx[3], 1), Hin - y0);
  const int flip = bx[4] & 1;
  const int img = min(max(idx[b], 0), N - 1);
  int r0, r1;
  float fy;
  tap(y, h, Hout, 1.0f / (float)(2 * Hout), r0, r1, fy);
  const int seg = w * C, stride = rs_row_stride(Win * C);
  const uintptr_t lo = (uintptr_t)src, hi = lo + (size_t)N * Hin * Win * C;  // the dataset: what may be read
  int lead[2];  // byte offset of each segment inside its first staged chunk
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const uintptr_t s0 = lo + (((size_t)img * Hin + (y0 + (r ? r1 : r0))) * Win + x0) * C;
    const uintptr_t al = s0 & ~(uintptr_t)15;
    lead[r] = (int)(s0 - al);
    const int nc = (lead[r] + seg + 15) >> 4;
    for (int j = threadIdx.x; j < nc; j += kRsThreads) {
      const uintptr_t a = al + 16u * (uintptr_t)j;
      uint4 v;
      if (a >= lo && a + 16 <= hi) {
        v = *(const uint4*)a;
      } else {
        uint32_t q[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
        for (int t = 0; t < 16; ++t)
          if (a + t >= lo && a + t < hi) q[t >> 2] |= (uint32_t)(*(const uint8_t*)(a + t)) << (8 * (t & 3));
        v = uint4{q[0], q[1], q[2], q[3]};
      }
      *(uint4*)(lds + r * stride + 16 * j) = v;
    }
  }
  __syncthreads();
  const int px0 = (blockIdx.x * kRsThreads + threadIdx.x) * P;
  if (px0 >= Wout) return;
  const uint32_t* top = (const uint32_t*)lds;
  const uint32_t* bot = (const uint32_t*)(lds + stride);
  float m[C], s[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    m[c] = mean[c];
    s[c] = inv_std[c];
  }
  const float rden = 1.0f / (float)(2 * Wout);
  alignas(16) TOut vals[E];  // (pixels past the row's end read clamped taps and are not stored)
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int x = px0 + p;
    int c0, c1;
    float fx;
    tap(flip ? (Wout - 1 - x) : x, w, Wout, rden, c0, c1, fx);
    // a tap's C <= 4 channels (the dword after a row's last pixel lies inside the row's LDS slack: rs_row_stride)
    const uint32_t q00 = bytes4(top, lead[0] + c0 * C), q01 = bytes4(top, lead[0] + c1 * C);
    const uint32_t q10 = bytes4(bot, lead[1] + c0 * C), q11 = bytes4(bot, lead[1] + c1 * C);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float t0 = (float)((q00 >> (8 * c)) & 0xffu), t1 = (float)((q01 >> (8 * c)) & 0xffu);
      const float b0 = (float)((q10 >> (8 * c)) & 0xffu), b1 = (float)((q11 >> (8 * c)) & 0xffu);
      const float tv = t0 + fx * (t1 - t0), bv = b0 + fx * (b1 - b0);
      const float v = (tv + fy * (bv - tv)) * (1.0f / 255.0f);
      vals[p * C + c] = cvt<TOut>((v - m[c]) * s[c]);
    }
  }
  const int rowlen = Wout * C, e0 = px0 * C;
  TOut* orow = out + ((size_t)b * Hout + y) * (size_t)rowlen;
  // whole stores: all P pixels inside the row, and the row's start a multiple of the store size (out itself is)
  if (px0 + P <= Wout && (rowlen * sizeof(TOut)) % SB == 0) {
#pragma unroll
    for (int k = 0; k < (int)(E * sizeof(TOut)); k += SB) {
      if constexpr (SB == 16)
        *(uint4*)((char*)(orow + e0) + k) = *(const uint4*)((const char*)vals + k);
      else
        *(uint2*)((char*)(orow + e0) + k) = *(const uint2*)((const char*)vals + k);
    }
  } else {
#pragma unroll
    for (int k = 0; k < E; ++k)
      if (e0 + k < rowlen) orow[e0 + k] = vals[k];
  }
}

template <typename TOut, int C>
void launch_resample(const uint8_t* src, const int* idx, const int* boxes, int box_stride, int N, int B, int Hin,
                     int Win, int Hout, int Wout, const float* mean, const float* inv_std, void* out,
                     hipStream_t st) {
  const dim3 grid((Wout + kRsThreads * kPix<C> - 1) / (kRsThreads * kPix<C>), Hout, B);
  hipLaunchKernelGGL((resample_flip_norm<TOut, C>), grid, dim3(kRsThreads), 2 * rs_row_stride(Win * C), st, src, idx,
                     boxes, box_stride, N, Hin, Win, Hout, Wout, mean, inv_std, (TOut*)out);
}

}  // namespace

extern "C" {

// src: [N, Hin, Win, C] uint8; idx: [B] int32 image ids; out: [B, Hout, Wout, C] (dtype 0 fp32, 1 bf16).
// step_dev (optional): device int64 read by the kernel in place of `step` (a graph replayed every step)
int mifx_img_crop_flip_norm(const uint8_t* src, const int* idx, int B, int Hin, int Win, int C, int Hout, int Wout,
                            int train, unsigned long long seed, unsigned int step, const long long* step_dev,
                            const float* mean,
                            const float* inv_std, int dtype, void* out, hipStream_t st) {
  if (B <= 0 || Hout > Hin || Wout > Win || C <= 0 || C > 4) return -1;
  const dim3 grid((Wout * C + kThreads * kVec - 1) / (kThreads * kVec), Hout, B);
  if (dtype)
    hipLaunchKernelGGL(crop_flip_norm<__hip_bfloat16>, grid, dim3(kThreads), 0, st, src, idx, Hin, Win, C, Hout, Wout,
                       train, (uint32_t)seed, (uint32_t)(seed >> 32), step, step_dev, mean, inv_std, (__hip_bfloat16*)out);
  else
    hipLaunchKernelGGL(crop_flip_norm<float>, grid, dim3(kThreads), 0, st, src, idx, Hin, Win, C, Hout, Wout, train,
                       (uint32_t)seed, (uint32_t)(seed >> 32), step, step_dev, mean, inv_std, (float*)out);
  return (int)hipGetLastError();
}

// boxes: int32 [B, 5] (x0, y0, w, h, flip), written for training step `step` (step_dev as above). Requires
// 0 < scale_lo <= scale_hi <= 1 and 0 < ratio_lo <= 1 <= ratio_hi.
int mifx_img_rrc_boxes(int B, int Hin, int Win, unsigned long long seed, unsigned int step, const long long* step_dev,
                       float scale_lo, float scale_hi, float ratio_lo, float ratio_hi, int* boxes, hipStream_t st) {
  if (B <= 0 || Hin <= 0 || Win <= 0 || (long long)Hin * Win > (1 << 24)) return -1;
  if (!(scale_lo > 0.0f && scale_lo <= scale_hi && scale_hi <= 1.0f && ratio_lo > 0.0f && ratio_lo <= 1.0f &&
        ratio_hi >= 1.0f))
    return -1;
  hipLaunchKernelGGL(rrc_boxes, dim3((B + 63) / 64), dim3(64), 0, st, B, Hin, Win, (uint32_t)seed,
                     (uint32_t)(seed >> 32), step, step_dev, scale_lo, scale_hi, ratio_lo, ratio_hi, boxes);
  return (int)hipGetLastError();
}

// src: [N, Hin, Win, C] uint8; idx: [B]; boxes: int32 box table, slot b at boxes + b * box_stride (5: one box per
// slot; 0: one box for the whole batch); out: [B, Hout, Wout, C] (dtype 0 fp32, 1 bf16), box resized bilinearly
// (half-pixel centres, taps clamped inside the box), flipped and normalised as crop_flip_norm does.
int mifx_img_resample_flip_norm(const uint8_t* src, const int* idx, const int* boxes, int box_stride, int N, int B,
                                int Hin, int Win, int C, int Hout, int Wout, const float* mean, const float* inv_std,
                                int dtype, void* out, hipStream_t st) {
  if (B <= 0 || N <= 0 || C <= 0 || C > 4 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0) return -1;
  if (Win * C > kMaxRowBytes || Hin > 16384 || Hout > 16384 || Wout > 16384 || B > 65535 || Hout > 65535) return -1;
  if (box_stride != 0 && box_stride != 5) return -1;
  switch (C * 2 + (dtype ? 1 : 0)) {
#define MIFX_RS(CC)                                                                                                  \
  case CC * 2:                                                                                                       \
    launch_resample<float, CC>(src, idx, boxes, box_stride, N, B, Hin, Win, Hout, Wout, mean, inv_std, out, st);     \
    break;                                                                                                           \
  case CC * 2 + 1:                                                                                                   \
    launch_resample<__hip_bfloat16, CC>(src, idx, boxes, box_stride, N, B, Hin, Win, Hout, Wout, mean, inv_std, out, \
                                        st);                                                                         \
    break;
    MIFX_RS(1) MIFX_RS(2) MIFX_RS(3) MIFX_RS(4)
#undef MIFX_RS
  }
  return (int)hipGetLastError();
}

}  // extern "C"
