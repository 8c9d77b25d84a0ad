// Shared by the taxi-DNN kernels (csrc/embag_mlp.hip: first layer and the one-layer step; csrc/tdnn_stack.hip: layers
// 2..L and their head): block reduction, the device-side batch selection and the TF-Adagrad update of one element.
#pragma once
#include <hip/hip_runtime.h>
#include "feed.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxH = 4096;

__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) red[w] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < kThreads / 64; ++i) t += red[i];
  __syncthreads();
  return t;
}

// record of example b of this step (see the header): the record feed of csrc/feed.h at step step_ctr[0] (global
// stream stride / offset, optional per-epoch shuffle), or records start_fixed.. in stored order
struct BatchSel {
  long long n;
  const long long* ctr;
  long long start_fixed;
  int B;
  MifxFeed feed;
  long long* rec_out;  // nullable: tdnn_head_bwd records which record each example of the step was
  __device__ __forceinline__ MifxFeedStep start() const {
    if (ctr) return mifx_feed_step(feed, ctr[0], n);
    MifxFeedStep s;
    s.e0 = 0;
    s.i0 = start_fixed;
    s.h = 1;
    return s;
  }
  __device__ __forceinline__ long long rec(const MifxFeedStep& st, int b) const {
    if (!ctr) {
      const long long e = st.i0 + b;
      return e >= n ? e - n : e;  // host guarantees B <= n
    }
    return mifx_feed_record(feed, st, b, n);
  }
};

// TF Adagrad: acc += g^2; w -= lr * g / sqrt(acc) (a zero gradient leaves both bit-unchanged)
__device__ __forceinline__ void adagrad_one(float* w, float* acc, float g, float lr) {
  const float s = *acc + g * g;
  *acc = s;
  *w -= lr * g * rsqrtf(s);
}

}  // namespace
