// Multi-tensor SGD (weight decay, momentum, dampening, Nesterov) for gfx950: one launch updates every fp32 parameter
// of a model in place from its own gradient and momentum tensors.
//
// Why (profiles/archive/resnet_steady_r5za.md, ResNet-50 B=256): torch.optim.SGD's captured update is six _foreach
// passes per parameter group (wd add, momentum mul, momentum add, Nesterov add, lr mul, param add) -- 14
// multi_tensor_apply launches, ~280 us per step -- each re-reading and re-writing the 25.6 M fp32 values. Here each
// element is read once (param, grad, momentum: 12 B) and written once (param, momentum: 8 B), in one launch.
//
// Semantics (torch.optim.SGD, foreach path): g' = g + wd p; buf = mom buf + (1 - damp) g';
// u = nesterov ? g' + mom buf : buf; p += neg_lr u, with neg_lr = -lr read from device memory (a replayed graph
// follows the learning-rate schedule). fp32 throughout; results match the foreach reference to fp32 rounding (FMA
// contraction may differ), not bit for bit.
//
// Workgroup b updates chunk b: tensor tp[b], elements [to[b], to[b] + tn[b]); per tensor: param / grad / momentum
// device addresses and its weight decay.
//
// The large-batch recipe (LARS trust ratios, learning-rate schedule from a device step counter) is a second entry
// point with kernels of its own further down (mifx_sgd_step_ex); the plain update above it is untouched by it.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = kThreads * 8;  // 2048 fp32 per workgroup: two float4 per thread

struct SgdArgs {
  const unsigned long long *pp, *gp, *bp;  // [P] param / grad / momentum addresses
  const float* wd;                         // [P]
  const int *tp, *to, *tn;                 // [nblocks] chunk -> (tensor, offset, length)
  const float* neg_lr;                     // device scalar: -lr
  float mom, damp;
  int nesterov;
};

__device__ __forceinline__ void sgd1(float& p, float g, float& b, float wd, float mom, float damp, bool nest,
                                     float nlr) {
  const float gg = g + wd * p;
  b = mom * b + (1.f - damp) * gg;
  const float u = nest ? gg + mom * b : b;
  p = p + nlr * u;
}

__global__ __launch_bounds__(kThreads) void sgd_chunks(const SgdArgs a) {
  const int ti = a.tp[blockIdx.x];
  float* p = (float*)a.pp[ti];
  const float* g = (const float*)a.gp[ti];
  float* b = (float*)a.bp[ti];
  const int o0 = a.to[blockIdx.x], n = a.tn[blockIdx.x];
  p += o0;
  g += o0;
  b += o0;
  const float wd = a.wd[ti], nlr = *a.neg_lr, mom = a.mom, damp = a.damp;
  const bool nest = a.nesterov != 0;
  const bool vec = (((unsigned long long)p | (unsigned long long)g | (unsigned long long)b) & 15) == 0;
  const int nv = vec ? n / 4 : 0;
  float4 pv[2], gv[2], bv[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {  // both vectors' loads in flight before the first update
    const int i = threadIdx.x + u * kThreads;
    if (i < nv) {
      pv[u] = ((const float4*)p)[i];
      gv[u] = ((const float4*)g)[i];
      bv[u] = ((const float4*)b)[i];
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = threadIdx.x + u * kThreads;
    if (i >= nv) break;
    sgd1(pv[u].x, gv[u].x, bv[u].x, wd, mom, damp, nest, nlr);
    sgd1(pv[u].y, gv[u].y, bv[u].y, wd, mom, damp, nest, nlr);
    sgd1(pv[u].z, gv[u].z, bv[u].z, wd, mom, damp, nest, nlr);
    sgd1(pv[u].w, gv[u].w, bv[u].w, wd, mom, damp, nest, nlr);
    ((float4*)p)[i] = pv[u];
    ((float4*)b)[i] = bv[u];
  }
  for (int i = nv * 4 + threadIdx.x; i < n; i += kThreads) {  // tail / unaligned tensor
    float pp = p[i], bb = b[i];
    sgd1(pp, g[i], bb, wd, mom, damp, nest, nlr);
    p[i] = pp;
    b[i] = bb;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Large-batch recipe, all of it evaluated on the device so that a captured step replays it: LARS trust ratios
// (apex-LARC-style scaling in front of the SGD update above) and the learning-rate schedule, read from the step
// counter the graph already holds. Three launches over the update's own chunk tables:
//   sqnorm2_chunks   workgroup b: sums of squares of its chunk of p and of g -> pw[b], pg[b];
//   lars_finalize    workgroup i: tensor i's partials summed in double -> ratio[i], {wn, gn}[i]; workgroup 0 also
//                    writes {-lr_t, lr_t} from the schedule at *step;
//   sgd_chunks_ex    sgd_chunks with g' = (g + wd p) * ratio[tensor] and -lr_t from the scalar written above.
// r_i = eta wn / (gn + wd_i wn + eps) for an adapted tensor with wn != 0 and gn != 0 (with clip: min(r_i / lr_t, 1)),
// else exactly 1. Without LARS (first == null) the finalize is one workgroup that only evaluates the schedule.

// Sum over the 16 lanes of a DPP row, left in every lane of the row: a butterfly of lane exchanges (xor 1, xor 2,
// mirror within 8, mirror within 16) on the VALU, no LDS traffic. Both partners add the same two values, so the
// order is fixed. (The helpers of csrc/adamw.hip's sqnorm_chunks.)
template <int CTRL>
__device__ inline float dpp_add(float x) {
  return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}

__device__ inline float row16_sum(float x) {
  x = dpp_add<0xB1>(x);   // quad_perm:[1,0,3,2]
  x = dpp_add<0x4E>(x);   // quad_perm:[2,3,0,1]
  x = dpp_add<0x141>(x);  // row_half_mirror
  x = dpp_add<0x140>(x);  // row_mirror
  return x;
}

__device__ inline float lane_value(float x, int lane) {  // lane's x, uniform over the wave
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}

__device__ inline float wave_sum(float s) {  // the wave's four rows, the same value in every lane
  s = row16_sum(s);
  return (lane_value(s, 0) + lane_value(s, 16)) + (lane_value(s, 32) + lane_value(s, 48));
}

__device__ __forceinline__ float sq4(float4 v, float s) {
  s = fmaf(v.x, v.x, s);
  s = fmaf(v.y, v.y, s);
  s = fmaf(v.z, v.z, s);
  return fmaf(v.w, v.w, s);
}

// fp32, in a fixed order: up to 8 squares per thread (two float4 of p and two of g, all four loads in flight), the DPP
// butterfly over each row, the wave's four rows, then the four waves through LDS. No atomics, and pw[b] / pg[b] are
// written on every launch, so the result is bit-reproducible and nothing stale survives a graph replay.
__global__ __launch_bounds__(kThreads) void sqnorm2_chunks(const unsigned long long* __restrict__ pp,
                                                          const unsigned long long* __restrict__ gp,
                                                          const int* __restrict__ tp, const int* __restrict__ to,
                                                          const int* __restrict__ tn, float* __restrict__ pw,
                                                          float* __restrict__ pg) {
  __shared__ float part[2][kThreads / 64];
  const int ti = tp[blockIdx.x];
  const int o0 = to[blockIdx.x], n = tn[blockIdx.x];
  const float* p = (const float*)pp[ti] + o0;
  const float* g = (const float*)gp[ti] + o0;
  const bool vec = (((unsigned long long)p | (unsigned long long)g) & 15) == 0;
  const int nv = vec ? n / 4 : 0;
  float4 pv[2], gv[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = threadIdx.x + u * kThreads;
    pv[u] = gv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < nv) {
      pv[u] = ((const float4*)p)[i];
      gv[u] = ((const float4*)g)[i];
    }
  }
  float sw = sq4(pv[1], sq4(pv[0], 0.f)), sg = sq4(gv[1], sq4(gv[0], 0.f));
  for (int i = nv * 4 + threadIdx.x; i < n; i += kThreads) {  // tail / unaligned tensor
    sw = fmaf(p[i], p[i], sw);
    sg = fmaf(g[i], g[i], sg);
  }
  sw = wave_sum(sw);
  sg = wave_sum(sg);
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = sw;
    part[1][threadIdx.x >> 6] = sg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    pw[blockIdx.x] = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
    pg[blockIdx.x] = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
  }
}

// Learning rate of the update that follows t completed ones, in double (mifx.ops.sgd.scheduled_lr is the twin):
// kind 0 constant, 1 cosine, 2 poly (power 2), each after a linear warmup base * min(1, (t + 1) / max(1, warmup)).
struct LrSched {
  int kind;
  long long warmup, total;
  double base, end;
};

__device__ inline double lr_at(const LrSched s, long long t) {
#pragma clang fp contract(off)  // the operations of the Python twin, one rounding each
  if (s.kind == 0 || t < s.warmup) {
    const double f = (double)(t + 1) / (s.warmup > 1 ? (double)s.warmup : 1.0);
    return s.base * (f < 1.0 ? f : 1.0);
  }
  if (t >= s.total) return s.end;
  const double x = (double)(t - s.warmup) / (double)(s.total - s.warmup);
  if (s.kind == 1) return s.end + (s.base - s.end) * 0.5 * (1.0 + cos(3.141592653589793 * x));
  const double q = 1.0 - x;
  return s.end + (s.base - s.end) * (q * q);
}

// One workgroup per tensor: thread j adds the partials first[i] + j, + 256, ... of its tensor in double (a loop: the
// largest ResNet-50 tensor has 1152 chunks), then an LDS tree; both orders are fixed.
__global__ __launch_bounds__(kThreads) void lars_finalize(const float* __restrict__ pw, const float* __restrict__ pg,
                                                         const int* __restrict__ first, const int* __restrict__ adapt,
                                                         const float* __restrict__ wd,
                                                         const long long* __restrict__ step, const LrSched sched,
                                                         double eta, double eps, int clip, float* __restrict__ ratio,
                                                         float* __restrict__ norms, float* __restrict__ lr_out) {
  __shared__ double acc[2][kThreads];
  float lr = 0.f;
  if (threadIdx.x == 0) {
    lr = (float)lr_at(sched, *step);  // the one rounding to fp32
    if (blockIdx.x == 0) {
      lr_out[0] = -lr;
      lr_out[1] = lr;
    }
  }
  if (first == nullptr) return;  // schedule only
  const int ti = blockIdx.x;
  double sw = 0.0, sg = 0.0;
  for (int i = first[ti] + threadIdx.x; i < first[ti + 1]; i += kThreads) {
    sw += (double)pw[i];
    sg += (double)pg[i];
  }
  acc[0][threadIdx.x] = sw;
  acc[1][threadIdx.x] = sg;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      acc[0][threadIdx.x] += acc[0][threadIdx.x + w];
      acc[1][threadIdx.x] += acc[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double wn = sqrt(acc[0][0]), gn = sqrt(acc[1][0]);
    float r = 1.f;
    if (adapt[ti] != 0 && wn != 0.0 && gn != 0.0) {
      double q = eta * wn / (gn + (double)wd[ti] * wn + eps);
      if (clip) {
        q = q / (double)lr;
        if (q > 1.0) q = 1.0;  // (not fmin: a NaN must stay a NaN)
      }
      r = (float)q;
    }
    ratio[ti] = r;
    norms[2 * ti] = (float)wn;
    norms[2 * ti + 1] = (float)gn;
  }
}

__device__ __forceinline__ void sgd1_ex(float& p, float g, float& b, float wd, float r, float mom, float damp,
                                        bool nest, float nlr) {
  const float gg = (g + wd * p) * r;
  b = mom * b + (1.f - damp) * gg;
  const float u = nest ? gg + mom * b : b;
  p = p + nlr * u;
}

// sgd_chunks with the gradient scaled by its tensor's trust ratio (ratio null: 1) and -lr_t from lars_finalize.
__global__ __launch_bounds__(kThreads) void sgd_chunks_ex(const SgdArgs a, const float* __restrict__ ratio) {
  const int ti = a.tp[blockIdx.x];
  float* p = (float*)a.pp[ti];
  const float* g = (const float*)a.gp[ti];
  float* b = (float*)a.bp[ti];
  const int o0 = a.to[blockIdx.x], n = a.tn[blockIdx.x];
  p += o0;
  g += o0;
  b += o0;
  const float wd = a.wd[ti], nlr = *a.neg_lr, mom = a.mom, damp = a.damp;
  const float r = ratio != nullptr ? ratio[ti] : 1.f;
  const bool nest = a.nesterov != 0;
  const bool vec = (((unsigned long long)p | (unsigned long long)g | (unsigned long long)b) & 15) == 0;
  const int nv = vec ? n / 4 : 0;
  float4 pv[2], gv[2], bv[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {  // both vectors' loads in flight before the first update
    const int i = threadIdx.x + u * kThreads;
    if (i < nv) {
      pv[u] = ((const float4*)p)[i];
      gv[u] = ((const float4*)g)[i];
      bv[u] = ((const float4*)b)[i];
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = threadIdx.x + u * kThreads;
    if (i >= nv) break;
    sgd1_ex(pv[u].x, gv[u].x, bv[u].x, wd, r, mom, damp, nest, nlr);
    sgd1_ex(pv[u].y, gv[u].y, bv[u].y, wd, r, mom, damp, nest, nlr);
    sgd1_ex(pv[u].z, gv[u].z, bv[u].z, wd, r, mom, damp, nest, nlr);
    sgd1_ex(pv[u].w, gv[u].w, bv[u].w, wd, r, mom, damp, nest, nlr);
    ((float4*)p)[i] = pv[u];
    ((float4*)b)[i] = bv[u];
  }
  for (int i = nv * 4 + threadIdx.x; i < n; i += kThreads) {  // tail / unaligned tensor
    float pp = p[i], bb = b[i];
    sgd1_ex(pp, g[i], bb, wd, r, mom, damp, nest, nlr);
    p[i] = pp;
    b[i] = bb;
  }
}

}  // namespace

extern "C" {

int mifx_sgd_chunk_size() { return kChunk; }

// One update with the recipe evaluated on the device (see above). first [ntensors + 1] (chunk range of each tensor)
// and adapt [ntensors] select LARS: then pw / pg [nblocks] are scratch (fully rewritten), ratio [ntensors] and norms
// [2 ntensors] = {wn, gn} are outputs; first == null is the schedule alone. lr_out [2] = {-lr_t, lr_t}; step is the
// device int64 count of completed updates (read, not advanced). sched_kind 0 constant / 1 cosine / 2 poly.
int mifx_sgd_step_ex(const unsigned long long* pp, const unsigned long long* gp, const unsigned long long* bp,
                     const float* wd, const int* tp, const int* to, const int* tn, int nblocks, const int* first,
                     const int* adapt, int ntensors, float* pw, float* pg, float* ratio, float* norms,
                     const long long* step, float* lr_out, int sched_kind, long long warmup, long long total,
                     double base, double end, double eta, double eps, int clip, float mom, float damp, int nesterov,
                     hipStream_t st) {
  if (nblocks <= 0 || pp == nullptr || gp == nullptr || bp == nullptr || wd == nullptr || step == nullptr ||
      lr_out == nullptr || sched_kind < 0 || sched_kind > 2 || (sched_kind != 0 && total <= warmup))
    return -1;
  const bool lars = first != nullptr;
  if (lars && (ntensors <= 0 || adapt == nullptr || pw == nullptr || pg == nullptr || ratio == nullptr ||
               norms == nullptr))
    return -1;
  const LrSched sched{sched_kind, warmup, total, base, end};
  if (lars)
    hipLaunchKernelGGL(sqnorm2_chunks, dim3((unsigned)nblocks), dim3(kThreads), 0, st, pp, gp, tp, to, tn, pw, pg);
  hipLaunchKernelGGL(lars_finalize, dim3(lars ? (unsigned)ntensors : 1u), dim3(kThreads), 0, st, (const float*)pw,
                     (const float*)pg, first, adapt, wd, step, sched, eta, eps, clip, ratio, norms, lr_out);
  const SgdArgs a{pp, gp, bp, wd, tp, to, tn, lr_out, mom, damp, nesterov};
  hipLaunchKernelGGL(sgd_chunks_ex, dim3((unsigned)nblocks), dim3(kThreads), 0, st, a,
                     lars ? (const float*)ratio : (const float*)nullptr);
  return (int)hipGetLastError();
}

int mifx_sgd_chunks(const unsigned long long* pp, const unsigned long long* gp, const unsigned long long* bp,
                    const float* wd, const int* tp, const int* to, const int* tn, int nblocks, const float* neg_lr,
                    float mom, float damp, int nesterov, hipStream_t st) {
  if (nblocks <= 0 || pp == nullptr || gp == nullptr || bp == nullptr || wd == nullptr || neg_lr == nullptr) return -1;
  const SgdArgs a{pp, gp, bp, wd, tp, to, tn, neg_lr, mom, damp, nesterov};
  hipLaunchKernelGGL(sgd_chunks, dim3((unsigned)nblocks), dim3(kThreads), 0, st, a);
  return (int)hipGetLastError();
}

}  // extern "C"
