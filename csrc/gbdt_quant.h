// The quantise stage of the device GBDT growers: ONE copy, included by the depth-wise grower (csrc/gbdt_gpu.hip) and by
// the leaf-wise one (csrc/gbdt_lossguide.hip). Largest magnitudes of g and h, one exponent each (gbdt_split.h), the
// rows as int64, the identity permutation and the root's sums and row count; with subsample < 1 the same over the rows
// that gbdt_sample.h keeps, compacted into perm0[0, n_s). Also the workspace carver and the 64-bit atomic add.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gbdt_sample.h"
#include "gbdt_split.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

typedef unsigned long long u64;

struct Quant {  // what the stage reads and writes; a grower's init kernel zeroes amax [2], nsamp [2], *root_g, *root_h
  long long *qg, *qh;  // [n] by row id
  int* perm0;          // [n] the root's rows
  unsigned* amax;      // [2] bit patterns of max |g|, max |h|
  int* exps;           // [2]
  int* nsamp;          // [2] sampled rows: their count (k_amax_s), the compaction cursor (k_quant_s)
  long long *root_g, *root_h;
  int* root_end;  // the root is [0, *root_end)
};

struct Carver {
  char* base;
  size_t used = 0;
  template <class T>
  T* take(size_t count) {
    T* r = base ? reinterpret_cast<T*>(base + used) : nullptr;
    used += (count * sizeof(T) + 255) & ~(size_t)255;
    return r;
  }
};

__device__ __forceinline__ void add64(long long* p, long long v) { atomicAdd(reinterpret_cast<u64*>(p), (u64)v); }

int grid_for(long n, int cap = 4096) { return (int)std::max<long>(1, std::min<long>((n + kThreads - 1) / kThreads, cap)); }

// max |g|, max |h| as bit patterns: non-negative floats order like their bits, and a NaN sorts above infinity
__global__ void k_amax(const float* g, const float* h, long n, unsigned* amax) {
  unsigned mg = 0, mh = 0;
  for (long i = blockIdx.x * (long)kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    mg = max(mg, __float_as_uint(fabsf(g[i])));
    mh = max(mh, __float_as_uint(fabsf(h[i])));
  }
  for (int o = 32; o; o >>= 1) {
    mg = max(mg, (unsigned)__shfl_xor((int)mg, o));
    mh = max(mh, (unsigned)__shfl_xor((int)mh, o));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(amax, mg);
    atomicMax(amax + 1, mh);
  }
}

__global__ void k_quant(const float* g, const float* h, long n, Quant w) {
  const int eg = mifx_gb_quant_exp((double)__uint_as_float(w.amax[0]), n);
  const int eh = mifx_gb_quant_exp((double)__uint_as_float(w.amax[1]), n);
  long long sg = 0, sh = 0;
  for (long i = blockIdx.x * (long)kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    const long long a = mifx_gb_quantise(g[i], eg), b = mifx_gb_quantise(h[i], eh);
    w.qg[i] = a;
    w.qh[i] = b;
    w.perm0[i] = (int)i;
    sg += a;
    sh += b;
  }
  for (int o = 32; o; o >>= 1) {
    sg += __shfl_xor(sg, o);
    sh += __shfl_xor(sh, o);
  }
  if ((threadIdx.x & 63) == 0) {
    add64(w.root_g, sg);
    add64(w.root_h, sh);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    w.exps[0] = eg;
    w.exps[1] = eh;
    *w.root_end = (int)n;
  }
}

// ---- subsample < 1: the quantise stage over the sampled rows only. Row i is sampled iff mifx_gs_keep_row(key, i,
// thr); both kernels hash (a few integer multiplies per row) instead of storing a mask. One atomic per workgroup and
// word: the per-wave form of k_amax / k_quant runs at the same-address atomic rate (profiles/gbdt_gpu.md).
__global__ __launch_bounds__(kThreads) void k_amax_s(const float* g, const float* h, long n, u64 key, u64 thr,
                                                     unsigned* amax, int* nsamp) {
  __shared__ unsigned s_g[kWaves], s_h[kWaves];
  __shared__ int s_c[kWaves];
  unsigned mg = 0, mh = 0;
  int c = 0;
  for (long i = blockIdx.x * (long)kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads)
    if (mifx_gs_keep_row(key, (u64)i, thr)) {
      mg = max(mg, __float_as_uint(fabsf(g[i])));
      mh = max(mh, __float_as_uint(fabsf(h[i])));
      ++c;
    }
  for (int o = 32; o; o >>= 1) {
    mg = max(mg, (unsigned)__shfl_xor((int)mg, o));
    mh = max(mh, (unsigned)__shfl_xor((int)mh, o));
    c += __shfl_xor(c, o);
  }
  if ((threadIdx.x & 63) == 0) {
    s_g[threadIdx.x >> 6] = mg;
    s_h[threadIdx.x >> 6] = mh;
    s_c[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int v = 1; v < kWaves; ++v) {
    mg = max(mg, s_g[v]);
    mh = max(mh, s_h[v]);
    c += s_c[v];
  }
  if (c == 0) return;
  atomicMax(amax, mg);
  atomicMax(amax + 1, mh);
  atomicAdd(nsamp, c);
}

__global__ __launch_bounds__(kThreads) void k_quant_s(const float* g, const float* h, long n, u64 key, u64 thr, Quant w,
                                                      int* leaf_of_row) {
  __shared__ int s_c[kWaves], s_base;
  __shared__ long long s_g[kWaves], s_h[kWaves];
  const int ns = w.nsamp[0];
  const int eg = mifx_gb_quant_exp((double)__uint_as_float(w.amax[0]), ns);
  const int eh = mifx_gb_quant_exp((double)__uint_as_float(w.amax[1]), ns);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the workgroup's sampled rows over its grid-stride share, then ONE returning atomic for its range of perm0
  int c = 0;
  for (long i = blockIdx.x * (long)kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads)
    c += mifx_gs_keep_row(key, (u64)i, thr);
  for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) s_c[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int v = 0; v < kWaves; ++v) tot += s_c[v];
    s_base = tot ? atomicAdd(&w.nsamp[1], tot) : 0;
  }
  __syncthreads();
  int cur = s_base;  // uniform over the wave: where this wave's next sampled row goes
  for (int v = 0; v < wave; ++v) cur += s_c[v];
  long long sg = 0, sh = 0;
  // the same rows as above, a wave at a time (the trip count is uniform over the wave: every lane reaches the ballot)
  for (long i0 = blockIdx.x * (long)kThreads + wave * 64; i0 < n; i0 += (long)gridDim.x * kThreads) {
    const long i = i0 + lane;
    const bool kp = i < n && mifx_gs_keep_row(key, (u64)i, thr);
    const u64 m = __ballot(kp);
    if (kp) {
      const long long a = mifx_gb_quantise(g[i], eg), b = mifx_gb_quantise(h[i], eh);
      w.qg[i] = a;
      w.qh[i] = b;
      const int pos = cur + __popcll(m & (((u64)1 << lane) - 1));
      if ((unsigned)pos < (unsigned long)n) w.perm0[pos] = (int)i;
      sg += a;
      sh += b;
    } else if (i < n) {
      leaf_of_row[i] = -1;
    }
    cur += __popcll(m);
  }
  for (int o = 32; o; o >>= 1) {
    sg += __shfl_xor(sg, o);
    sh += __shfl_xor(sh, o);
  }
  if (lane == 0) {
    s_g[wave] = sg;
    s_h[wave] = sh;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < kWaves; ++v) {
      sg += s_g[v];
      sh += s_h[v];
    }
    if (sg) add64(w.root_g, sg);
    if (sh) add64(w.root_h, sh);
    if (blockIdx.x == 0) {
      w.exps[0] = eg;
      w.exps[1] = eh;
      *w.root_end = ns;
    }
  }
}

// the stage on `stream`: thr < 2^32 samples the rows of (seed, round) (leaf_of_row = -1 for the others)
void launch_quant(const float* g, const float* h, long n, unsigned long long seed, unsigned long long round,
                  unsigned long long thr, const Quant& q, int* leaf_of_row, hipStream_t stream) {
  if (thr < MIFX_GS_KEEP_ALL) {
    const u64 key = mifx_gs_key(seed, round, MIFX_GS_SITE_ROWS);
    k_amax_s<<<grid_for(n), kThreads, 0, stream>>>(g, h, n, key, thr, q.amax, q.nsamp);
    k_quant_s<<<grid_for(n), kThreads, 0, stream>>>(g, h, n, key, thr, q, leaf_of_row);
  } else {
    k_amax<<<grid_for(n), kThreads, 0, stream>>>(g, h, n, q.amax);
    k_quant<<<grid_for(n), kThreads, 0, stream>>>(g, h, n, q);
  }
}

}  // namespace
