// Device learner of mifx.gbdt (XGBRegressor / XGBClassifier with device="gpu"): one boosting round's gradients, tree
// and margin updates on the GPU, nothing read back inside a tree.
// MIFX_HIPCC_FLAGS: -ffp-contract=off
//
// Semantics: the fixed-point learner of gbdt_split.h (the one copy of the split rule, shared with the host twin
// mifx_gbdt_grow_fixed in gbdt.cpp). Gradients are quantised to int64 with one exponent per tree and quantity, so
// histograms, node sums and prefix sums are integer sums: the tree cannot depend on launch geometry, on the order of
// atomics or on the order of rows inside a node, and the host twin reproduces it bit for bit.
//
// Data: bins row-major [n, f] uint16 (one row's features share a cache line: the rows of a deep node are a gather);
// a value >= nbins[j] (0xFFFF or anything else) is "missing", so every index taken from bins is in bounds. Rows of a
// node are a contiguous range [begin, end) of a permutation array; a split partitions its range into the children's
// ranges in a second array (ping-pong). Rows of a node that turned leaf keep their place and are never read again.
//
// Per level d (every kernel is launched for the worst case 2^d nodes and reads the live count on the device; a dead
// level costs empty launches, never a host synchronisation):
//   k_hist      per (row chunk, feature tile) workgroup, per node segment inside the chunk: LDS histograms
//               (int64 g, int64 h, int32 rows) by LDS atomics, non-empty slots flushed with 64-bit global atomics
//   k_split     one wave per (node, feature): lanes own runs of 4 bins, integer prefix scan across the wave,
//               mifx_gb_scan per lane, lanes merged with ties to the lowest (bin, direction)
//   k_decide    one workgroup: per node the features in order (1e-12 rule), leaf test, leaf value (and, when asked
//               for, the node's gain and cover: mifx_gbdt_gpu_grow_stats); then one thread
//               numbers the children in the host learner's order (breadth first, in the order of their parents)
//   k_partition per row position: a leaf's rows get leaf_of_row and margin += value; a split's rows move to their
//               child's range through wave-aggregated atomic cursors. The order of rows INSIDE a child is therefore
//               not deterministic; nothing downstream depends on it (integer sums, per-row writes).
//
// Stochastic boosting (mifx_gbdt_gpu_grow_ex; the draws are gbdt_sample.h's, the host twin is mifx_gbdt_grow_fixed_ex):
//   rows      with subsample < 1 the quantise stage is a compaction: k_amax_s takes the maxima over the sampled rows
//             and counts them, k_quant_s derives the exponents from that device-side count, writes the sampled rows
//             as perm[0][0, n_s) (each workgroup counts its share, draws ONE cursor range, then places) and
//             leaf_of_row = -1 for the others; the root is [0, n_s). The level kernels are still launched for n rows
//             and find no node beyond n_s. Rows outside the sample get their margin from a walk of the finished tree
//             over the training bins (k_apply_rest).
//   features  a [max_depth, f] uint8 mask computed by the host: k_split gives no candidate for a masked (level,
//             feature), k_hist skips a feature tile that is masked entirely.
//
// Multi-class (multi:softprob, K >= 3 classes): k_grad_softmax computes all K gradient pairs of a round in one launch
// from class-major [K, n] margins; the round then grows K trees with the grower above, tree k on row k of g, h and
// the margins. The grower itself knows nothing about classes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gbdt_sample.h"
#include "gbdt_split.h"

namespace {

constexpr int kMaxBins = 256;          // bins per feature
constexpr int kSlots = kMaxBins + 1;   // LDS slots per feature: the bins and "missing"
constexpr int kMaxDepth = 12;
constexpr int kMaxFeatTile = 12;       // 12 * 257 * 20 B = 61,680 B of LDS
constexpr int kThreads = 256;

typedef unsigned long long u64;

struct Level {  // the nodes of one depth, in the host learner's order (= ascending row ranges)
  int *id, *begin, *end;
  long long *qg, *qh;
};

struct Decision {  // per node of the current level
  int *feat, *bin, *dl, *cl;  // feat < 0: leaf
  long long *gl, *hl;
  double* val;
};

struct TreeOut {
  int *feature, *split_bin;
  uint8_t* default_left;
  int *left, *right;
  double* value;
  double *gain, *cover;  // (nullable) node statistics: the split's gain (0.0 at a leaf), the node's hessian sum
};

struct Ws {
  long long *qg, *qh;
  int* perm[2];
  unsigned* amax;  // [2] bit patterns of max |g|, max |h|
  int *exps, *lcount, *ncount;
  Level lv[2];
  Decision dec;
  int* cur;
  MifxGbSplit* cand;
  long long *hg, *hh;
  int* hc;
  int* nsamp;  // [2] sampled rows: their count (k_amax_s), the compaction cursor (k_quant_s)
  size_t bytes;
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

Ws carve(void* base, long n, int f, int max_depth, int hsize) {
  Carver c{static_cast<char*>(base)};
  const size_t maxl = (size_t)1 << max_depth, maxh = max_depth > 0 ? (size_t)1 << (max_depth - 1) : 1;
  Ws w;
  w.qg = c.take<long long>(n);
  w.qh = c.take<long long>(n);
  w.perm[0] = c.take<int>(n);
  w.perm[1] = c.take<int>(n);
  w.amax = c.take<unsigned>(2);
  w.exps = c.take<int>(2);
  w.lcount = c.take<int>(max_depth + 2);
  w.ncount = c.take<int>(1);
  for (int i = 0; i < 2; ++i) {
    w.lv[i].id = c.take<int>(maxl);
    w.lv[i].begin = c.take<int>(maxl);
    w.lv[i].end = c.take<int>(maxl);
    w.lv[i].qg = c.take<long long>(maxl);
    w.lv[i].qh = c.take<long long>(maxl);
  }
  w.dec.feat = c.take<int>(maxl);
  w.dec.bin = c.take<int>(maxl);
  w.dec.dl = c.take<int>(maxl);
  w.dec.cl = c.take<int>(maxl);
  w.dec.gl = c.take<long long>(maxl);
  w.dec.hl = c.take<long long>(maxl);
  w.dec.val = c.take<double>(maxl);
  w.cur = c.take<int>(2 * maxl);
  w.cand = c.take<MifxGbSplit>(maxh * f);
  w.hg = c.take<long long>(maxh * hsize);
  w.hh = c.take<long long>(maxh * hsize);
  w.hc = c.take<int>(maxh * hsize);
  w.nsamp = c.take<int>(2);
  w.bytes = c.used;
  return w;
}

__device__ __forceinline__ void add64(long long* p, long long v) { atomicAdd(reinterpret_cast<u64*>(p), (u64)v); }

// ---- gradients: the formulas of XGBRegressor / XGBClassifier._grad_hess
// wt (nullable): instance weights; the float32 pair times the float32 weight, one IEEE multiply each
__global__ void k_grad(int objective, const double* margin, const double* y, const float* wt, long n, float* g,
                       float* h) {
  const long i = blockIdx.x * (long)kThreads + threadIdx.x;
  if (i >= n) return;
  float gi, hi;
  if (objective == 0) {
    gi = (float)(margin[i] - y[i]);
    hi = 1.0f;
  } else {
    const double p = 1.0 / (1.0 + exp(-margin[i]));
    gi = (float)(p - y[i]);
    hi = (float)fmax(p * (1.0 - p), 1e-16);
  }
  if (wt) {
    gi = gi * wt[i];
    hi = hi * wt[i];
  }
  g[i] = gi;
  h[i] = hi;
}

// ---- multi:softprob: the K pairs of every row from the margins at the start of the round (XGBClassifier._grad_hess
// for K >= 3 is the specification). margin, g, h: class-major [K, n]; y: the class index as a double. One row per
// thread, so a wave reads and writes 64 consecutive elements of one class at a time. Everything up to the two casts is
// double: the maximum, e_k = exp(m_k - mx), their sum in class order, p_k = e_k / s. exp is evaluated twice per element
// (K is a run-time value: the e_k cannot wait in registers) from the same expression, so p_k comes from the e_k that
// entered s; the second and third pass re-read margins that the first one has just brought in.
__global__ void k_grad_softmax(const double* margin, const double* y, const float* wt, long n, int K, float* g,
                               float* h) {
  const long i = blockIdx.x * (long)kThreads + threadIdx.x;
  if (i >= n) return;
  const double* m = margin + i;
  double mx = m[0];
  for (int k = 1; k < K; ++k) mx = fmax(mx, m[(size_t)k * n]);
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += exp(m[(size_t)k * n] - mx);
  const int yi = (int)y[i];
  const float w = wt ? wt[i] : 1.0f;
  for (int k = 0; k < K; ++k) {
    const double p = exp(m[(size_t)k * n] - mx) / s;
    float gi = (float)(p - (k == yi ? 1.0 : 0.0));
    float hi = (float)fmax(2.0 * p * (1.0 - p), 1e-16);
    if (wt) {
      gi = gi * w;
      hi = hi * w;
    }
    g[(size_t)k * n + i] = gi;
    h[(size_t)k * n + i] = hi;
  }
}

__global__ void k_init(Ws w) {
  if (threadIdx.x < 2) w.amax[threadIdx.x] = 0u;
  if (threadIdx.x == 2) w.lv[0].qg[0] = 0;
  if (threadIdx.x == 3) w.lv[0].qh[0] = 0;
  if (threadIdx.x == 4 || threadIdx.x == 5) w.nsamp[threadIdx.x - 4] = 0;
}

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

__global__ void k_quant(const float* g, const float* h, long n, Ws w) {
  const int eg = mifx_gb_quant_exp((double)__uint_as_float(w.amax[0]), n);
  const int eh = mifx_gb_quant_exp((double)__uint_as_float(w.amax[1]), n);
  long long sg = 0, sh = 0;
  for (long i = blockIdx.x * (long)kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    const long long a = mifx_gb_quantise(g[i], eg), b = mifx_gb_quantise(h[i], eh);
    w.qg[i] = a;
    w.qh[i] = b;
    w.perm[0][i] = (int)i;
    sg += a;
    sh += b;
  }
  for (int o = 32; o; o >>= 1) {
    sg += __shfl_xor(sg, o);
    sh += __shfl_xor(sh, o);
  }
  if ((threadIdx.x & 63) == 0) {
    add64(w.lv[0].qg, sg);
    add64(w.lv[0].qh, sh);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    w.exps[0] = eg;
    w.exps[1] = eh;
    w.lv[0].id[0] = 0;
    w.lv[0].begin[0] = 0;
    w.lv[0].end[0] = (int)n;
    w.lcount[0] = 1;
    *w.ncount = 1;
  }
}

// ---- subsample < 1: the quantise stage over the sampled rows only. Row i is sampled iff mifx_gs_keep_row(key, i,
// thr); both kernels hash (a few integer multiplies per row) instead of storing a mask. One atomic per workgroup and
// word: the per-wave form of k_amax / k_quant runs at the same-address atomic rate (profiles/gbdt_gpu.md).
constexpr int kWaves = kThreads / 64;

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

__global__ __launch_bounds__(kThreads) void k_quant_s(const float* g, const float* h, long n, u64 key, u64 thr, Ws w,
                                                      int* leaf_of_row) {
  __shared__ int s_c[kWaves], s_base;
  __shared__ long long s_g[kWaves], s_h[kWaves];
  const int ns = w.nsamp[0];
  const int eg = mifx_gb_quant_exp((double)__uint_as_float(w.amax[0]), ns);
  const int eh = mifx_gb_quant_exp((double)__uint_as_float(w.amax[1]), ns);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the workgroup's sampled rows over its grid-stride share, then ONE returning atomic for its range of perm[0]
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
      if ((unsigned)pos < (unsigned long)n) w.perm[0][pos] = (int)i;
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
    if (sg) add64(w.lv[0].qg, sg);
    if (sh) add64(w.lv[0].qh, sh);
    if (blockIdx.x == 0) {
      w.exps[0] = eg;
      w.exps[1] = eh;
      w.lv[0].id[0] = 0;
      w.lv[0].begin[0] = 0;
      w.lv[0].end[0] = ns;
      w.lcount[0] = 1;
      *w.ncount = 1;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_hist(Level lv, const int* lcount, int d, const uint16_t* bins,
                                                   const int* perm, const long long* qg, const long long* qh, long n,
                                                   int f, const int* nbins, const int* hoff, int hsize, long long* hg,
                                                   long long* hh, int* hc, int rows_per_wg, int ft,
                                                   const uint8_t* lmask) {
  extern __shared__ long long smem[];
  long long* sg = smem;
  long long* sh = smem + ft * kSlots;
  int* sc = reinterpret_cast<int*>(smem + 2 * ft * kSlots);
  const int cnt = min(lcount[d], 1 << d);
  const long p0 = (long)blockIdx.x * rows_per_wg, p1 = min(n, p0 + rows_per_wg);
  const int j0 = blockIdx.y * ft, nf = min(ft, f - j0), tid = threadIdx.x;
  if (lmask) {  // (nullable) the level's feature mask: a tile without a live feature is never searched
    bool live = false;
    for (int jj = 0; jj < nf; ++jj) live |= lmask[j0 + jj] != 0;
    if (!live) return;  // uniform over the workgroup
  }
  int lo = 0, hi = cnt;  // first node that ends after p0 (ranges ascend)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (lv.end[mid] > p0) hi = mid;
    else lo = mid + 1;
  }
  for (int k = lo; k < cnt; ++k) {  // every branch on k is uniform over the workgroup
    const int b = lv.begin[k], e = lv.end[k];
    if (b >= p1) break;
    if (e - b < 2) continue;  // a leaf whatever its histogram
    const long s0 = max((long)b, p0), s1 = min((long)e, p1);
    if (s0 >= s1) continue;
    for (int i = tid; i < nf * kSlots; i += kThreads) {
      sg[i] = 0;
      sh[i] = 0;
      sc[i] = 0;
    }
    __syncthreads();
    const long items = (s1 - s0) * nf;
    for (long it = tid; it < items; it += kThreads) {
      const int jj = (int)(it % nf);
      const int r = perm[s0 + it / nf];
      if ((unsigned)r >= (unsigned long)n) continue;
      const int nb = min(nbins[j0 + jj], kMaxBins);
      const int bv = bins[(size_t)r * f + j0 + jj];
      const int s = jj * kSlots + (bv < nb ? bv : nb);
      add64(&sg[s], qg[r]);
      add64(&sh[s], qh[r]);
      atomicAdd(&sc[s], 1);
    }
    __syncthreads();
    for (int i = tid; i < nf * kSlots; i += kThreads) {
      const int jj = i / kSlots, sl = i % kSlots;
      if (sc[i] != 0 && sl <= min(nbins[j0 + jj], kMaxBins)) {
        const size_t o = (size_t)k * hsize + hoff[j0 + jj] + sl;
        add64(&hg[o], sg[i]);
        add64(&hh[o], sh[i]);
        atomicAdd(&hc[o], sc[i]);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void k_split(Level lv, const int* lcount, int d, int f, const int* nbins,
                                                    const int* hoff, int hsize, const long long* hg,
                                                    const long long* hh, const int* hc, const int* exps,
                                                    MifxGbParams prm, MifxGbSplit* cand, const uint8_t* lmask) {
  const long wave = (blockIdx.x * (long)kThreads + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const int cnt = min(lcount[d], 1 << d);
  const int k = (int)(wave / f), j = (int)(wave % f);
  if (k >= cnt) return;  // uniform over the wave
  MifxGbSplit bs = mifx_gb_no_split();
  if (lv.end[k] - lv.begin[k] >= 2 && (!lmask || lmask[j])) {  // a masked feature yields no candidate at this level
    const int nb = min(nbins[j], kMaxBins);
    const size_t o = (size_t)k * hsize + hoff[j];
    const long long *g0 = hg + o, *h0 = hh + o;
    const int* c0 = hc + o;
    const int b0 = lane * 4;  // 64 lanes x 4 bins = kMaxBins
    long long lg = 0, lh = 0;
    int lc = 0;
    for (int b = b0; b < b0 + 4 && b < nb; ++b) {
      lg += g0[b];
      lh += h0[b];
      lc += c0[b];
    }
    long long ig = lg, ih = lh;  // inclusive prefix over the lanes
    int ic = lc;
    for (int s = 1; s < 64; s <<= 1) {
      const long long tg = __shfl_up(ig, s), th = __shfl_up(ih, s);
      const int tc = __shfl_up(ic, s);
      if (lane >= s) {
        ig += tg;
        ih += th;
        ic += tc;
      }
    }
    const int eg = exps[0], eh = exps[1];
    const long long Qg = lv.qg[k], Qh = lv.qh[k];
    const double parent = mifx_gb_parent_score(Qg, Qh, eg, eh, prm);
    mifx_gb_scan(g0, h0, c0, nb, b0, b0 + 4, ig - lg, ih - lh, ic - lc, Qg, Qh, eg, eh, j, prm, parent, &bs);
    for (int s = 32; s; s >>= 1) {
      MifxGbSplit ot;
      ot.gain = __shfl_xor(bs.gain, s);
      ot.feature = __shfl_xor(bs.feature, s);
      ot.bin = __shfl_xor(bs.bin, s);
      ot.default_left = __shfl_xor(bs.default_left, s);
      ot.gl = __shfl_xor(bs.gl, s);
      ot.hl = __shfl_xor(bs.hl, s);
      ot.cl = __shfl_xor(bs.cl, s);
      if (!mifx_gb_lower_wins(bs, ot)) bs = ot;
    }
  }
  if (lane == 0) cand[(size_t)k * f + j] = bs;
}

__global__ __launch_bounds__(kThreads) void k_decide(Level lv, Level nx, int* lcount, int d, int force_leaf, int f,
                                                     const MifxGbSplit* cand, const int* exps, MifxGbParams prm,
                                                     Decision dec, int* cur, TreeOut t, int cap, int* ncount) {
  const int cnt = min(lcount[d], 1 << d);
  for (int k = threadIdx.x; k < cnt; k += kThreads) {
    MifxGbSplit best = mifx_gb_no_split();
    if (!force_leaf)
      for (int j = 0; j < f; ++j) {
        const MifxGbSplit c = cand[(size_t)k * f + j];
        if (mifx_gb_feature_wins(c, best)) best = c;
      }
    const bool leaf = force_leaf || mifx_gb_is_leaf(best);
    dec.feat[k] = leaf ? -1 : best.feature;
    dec.bin[k] = best.bin;
    dec.dl[k] = best.default_left;
    dec.cl[k] = best.cl;
    dec.gl[k] = best.gl;
    dec.hl[k] = best.hl;
    // the root of an empty sample: +0.0, no division (no other node is ever empty: d is uniform, so levels below
    // the root do not even load the range)
    const bool empty = d == 0 && lv.end[k] <= lv.begin[k];
    dec.val[k] = leaf && !empty ? mifx_gb_leaf_value(lv.qg[k], lv.qh[k], exps[0], exps[1], prm) : 0.0;
    const int nid = lv.id[k];
    if (t.gain && nid >= 0 && nid < cap) {  // what the host twin records (mifx_gbdt_grow_fixed_stats)
      t.gain[nid] = leaf ? 0.0 : best.gain;
      t.cover[nid] = mifx_gb_dequant(lv.qh[k], exps[1]);
    }
    cur[2 * k] = 0;
    cur[2 * k + 1] = 0;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int base = *ncount;
  int s = 0;  // splits so far in this level: children are numbered in the order of their parents
  for (int k = 0; k < cnt; ++k) {
    const int id = lv.id[k];
    if (id < 0 || id >= cap) continue;
    if (dec.feat[k] >= 0 && base + 2 * s + 1 >= cap) {  // cannot happen with cap = 2^(max_depth + 1)
      dec.feat[k] = -1;
      dec.val[k] = mifx_gb_leaf_value(lv.qg[k], lv.qh[k], exps[0], exps[1], prm);
      if (t.gain) t.gain[id] = 0.0;
    }
    const bool leaf = dec.feat[k] < 0;
    const int li = leaf ? -1 : base + 2 * s, ri = leaf ? -1 : li + 1;
    t.feature[id] = dec.feat[k];
    t.split_bin[id] = leaf ? -1 : dec.bin[k];
    t.default_left[id] = leaf ? 0 : (uint8_t)dec.dl[k];
    t.left[id] = li;
    t.right[id] = ri;
    t.value[id] = dec.val[k];
    if (leaf) continue;
    const int b = lv.begin[k], e = lv.end[k], mid = min(e, b + max(dec.cl[k], 0));
    dec.cl[k] = mid - b;
    nx.id[2 * s] = li;
    nx.begin[2 * s] = b;
    nx.end[2 * s] = mid;
    nx.qg[2 * s] = dec.gl[k];
    nx.qh[2 * s] = dec.hl[k];
    nx.id[2 * s + 1] = ri;
    nx.begin[2 * s + 1] = mid;
    nx.end[2 * s + 1] = e;
    nx.qg[2 * s + 1] = lv.qg[k] - dec.gl[k];
    nx.qh[2 * s + 1] = lv.qh[k] - dec.hl[k];
    ++s;
  }
  lcount[d + 1] = 2 * s;
  *ncount = base + 2 * s;
}

__global__ __launch_bounds__(kThreads) void k_partition(Level lv, const int* lcount, int d, Decision dec, int* cur,
                                                        const uint16_t* bins, const int* nbins, long n, int f,
                                                        const int* perm_in, int* perm_out, int* leaf_of_row,
                                                        double* margin) {
  const long p = blockIdx.x * (long)kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int cnt = min(lcount[d], 1 << d);
  int k = -1;
  if (p < n) {
    int lo = 0, hi = cnt;  // the last node that begins at or before p
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (lv.begin[mid] <= p) lo = mid + 1;
      else hi = mid;
    }
    k = lo - 1;
    if (k >= 0 && p >= lv.end[k]) k = -1;  // a row of a node that turned leaf at an earlier level
  }
  int r = 0, feat = -1;
  if (k >= 0) {
    r = perm_in[p];
    feat = dec.feat[k];
    if ((unsigned)r >= (unsigned long)n) k = -1, feat = -1;
  }
  if (k >= 0 && feat < 0) {
    leaf_of_row[r] = lv.id[k];
    if (margin) margin[r] += dec.val[k];
  }
  const bool split = k >= 0 && feat >= 0;
  bool goleft = false;
  if (split) {
    const int nb = min(nbins[feat], kMaxBins);
    const int bv = bins[(size_t)r * f + feat];
    goleft = bv < nb ? bv <= dec.bin[k] : dec.dl[k] != 0;
  }
  // every lane reaches the wave operations below; a wave whose 64 rows all belong to one split node draws its
  // places with two atomics, any other wave with one per row
  const int k0 = __shfl(k, 0);
  const bool uniform = __all(k == k0) && k0 >= 0;
  int off = -1;
  if (uniform && split) {  // (split is uniform where uniform holds)
    const u64 ml = __ballot(goleft);
    const int nl = __popcll(ml), nr = 64 - nl;
    int bl = 0, br = 0;
    if (lane == 0) {
      if (nl) bl = atomicAdd(&cur[2 * k0], nl);
      if (nr) br = atomicAdd(&cur[2 * k0 + 1], nr);
    }
    bl = __shfl(bl, 0);
    br = __shfl(br, 0);
    const int rl = __popcll(ml & (((u64)1 << lane) - 1));
    off = goleft ? bl + rl : dec.cl[k] + br + (lane - rl);
  } else if (split) {
    off = goleft ? atomicAdd(&cur[2 * k], 1) : dec.cl[k] + atomicAdd(&cur[2 * k + 1], 1);
  }
  if (split) {
    const long dst = (long)lv.begin[k] + off;
    if (off >= 0 && dst < lv.end[k]) perm_out[dst] = r;
  }
}

// margin[i] += the new tree's output for row i of a binned matrix (the eval set): bin <= split_bin  <=>  x < cut
// rest (nullable): leaf_of_row of a sampled tree; only its -1 rows, the rows outside the sample, are walked
__global__ void k_apply(const uint16_t* bins, long m, int f, const int* nbins, TreeOut t, int cap, int max_depth,
                        double* margin, const int* rest) {
  const long i = blockIdx.x * (long)kThreads + threadIdx.x;
  if (i >= m) return;
  if (rest && rest[i] >= 0) return;
  int k = 0;
  for (int step = 0; step <= max_depth; ++step) {
    const int feat = t.feature[k];
    if (feat < 0 || feat >= f) break;
    const int nb = min(nbins[feat], kMaxBins);
    const int bv = bins[(size_t)i * f + feat];
    const bool l = bv < nb ? bv <= t.split_bin[k] : t.default_left[k] != 0;
    const int c = l ? t.left[k] : t.right[k];
    if (c <= 0 || c >= cap) break;
    k = c;
  }
  margin[i] += t.value[k];
}

int grid_for(long n, int cap = 4096) { return (int)std::max<long>(1, std::min<long>((n + kThreads - 1) / kThreads, cap)); }

}  // namespace

extern "C" {

int mifx_gbdt_gpu_max_depth() { return kMaxDepth; }
int mifx_gbdt_gpu_max_bins() { return kMaxBins; }
int mifx_gbdt_gpu_max_feat_tile() { return kMaxFeatTile; }

// bytes of workspace for mifx_gbdt_gpu_grow; hsize = sum over features of nbins + 1; -1 on arguments out of range
long long mifx_gbdt_gpu_ws_bytes(long n, int f, int max_depth, int hsize) {
  if (n < 1 || n >= (1L << 31) || f < 1 || max_depth < 0 || max_depth > kMaxDepth || hsize < 2 * f ||
      hsize > f * kSlots)
    return -1;
  return (long long)carve(nullptr, n, f, max_depth, hsize).bytes;
}

int mifx_gbdt_gpu_grad(int objective, const double* margin, const double* y, long n, float* g, float* h,
                       hipStream_t stream) {
  if (n < 1 || objective < 0 || objective > 1) return -1;
  k_grad<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, stream>>>(objective, margin, y, nullptr, n, g, h);
  return (int)hipGetLastError();
}

// the same with instance weights (float32 [n], nullable): g, h = the pair above times the weight
int mifx_gbdt_gpu_grad_w(int objective, const double* margin, const double* y, const float* weight, long n, float* g,
                         float* h, hipStream_t stream) {
  if (n < 1 || objective < 0 || objective > 1) return -1;
  k_grad<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, stream>>>(objective, margin, y, weight, n, g, h);
  return (int)hipGetLastError();
}

// multi:softprob, one launch per round: margin [num_class, n] (class-major) and y [n] (class indices 0 .. num_class - 1
// as doubles) to g, h [num_class, n]; weight (float32 [n], nullable) as above. num_class has no upper limit here.
int mifx_gbdt_gpu_grad_softmax(const double* margin, const double* y, const float* weight, long n, int num_class,
                               float* g, float* h, hipStream_t stream) {
  if (n < 1 || n >= (1L << 31) || num_class < 1) return -1;
  k_grad_softmax<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, stream>>>(margin, y, weight, n, num_class,
                                                                                      g, h);
  return (int)hipGetLastError();
}

// Grow one tree. bins: row-major [n, f]; nbins [f] and hoff [f] (exclusive prefix of nbins + 1) on the device, the
// tree arrays (cap = 2^(max_depth + 1) entries each) and node_count too. leaf_of_row [n]; margin (nullable) [n]
// receives margin[row] += value[leaf of row]. rows_per_wg / feat_tile: launch geometry of the histogram kernel.
//
// Sampling: thr < 2^32 grows the tree on the rows that mifx_gs_keep_row(key(seed, round, rows), i, thr) keeps, as if
// the table held only them (leaf_of_row = -1 for the others; thr >= 2^32 keeps every row and hashes nothing).
// level_mask (device, nullable): [max_depth, f] uint8, the features each level may split on. With sampling every
// row's margin still receives the tree's output; margin_route 0: the partition updates the sampled rows and a walk of
// the tree covers the others, 1: one walk over all rows. Both add the same double to the same margin.
// node_gain / node_cover (device, cap doubles each, both or neither): per node the gain of its split (0.0 at a leaf)
// and its hessian sum over the rows the tree was grown on, the values of the host's mifx_gbdt_grow_fixed_stats.
int mifx_gbdt_gpu_grow_stats(const uint16_t* bins, long n, int f, const int* nbins, const int* hoff, int hsize,
                             const float* g, const float* h, int max_depth, double min_child_weight, double lambda,
                             double gamma, double eta, void* ws, long long ws_bytes, int* feature, int* split_bin,
                             uint8_t* default_left, int* left, int* right, double* value, int* node_count,
                             int* leaf_of_row, double* margin, int rows_per_wg, int feat_tile, unsigned long long seed,
                             unsigned long long round, unsigned long long thr, const uint8_t* level_mask,
                             int margin_route, double* node_gain, double* node_cover, hipStream_t stream) {
  if ((node_gain == nullptr) != (node_cover == nullptr)) return -1;
  const long long need = mifx_gbdt_gpu_ws_bytes(n, f, max_depth, hsize);
  if (need < 0 || ws_bytes < need || rows_per_wg < 1 || feat_tile < 1 || feat_tile > kMaxFeatTile) return -1;
  if (margin_route < 0 || margin_route > 1) return -1;
  const bool sampled = thr < MIFX_GS_KEEP_ALL;
  double* part_margin = sampled && margin_route == 1 ? nullptr : margin;
  Ws w = carve(ws, n, f, max_depth, hsize);
  const MifxGbParams prm{lambda, gamma, min_child_weight, eta};
  const TreeOut t{feature, split_bin, default_left, left, right, value, node_gain, node_cover};
  const int cap = 1 << (max_depth + 1);
  k_init<<<1, 64, 0, stream>>>(w);
  if (sampled) {
    const u64 key = mifx_gs_key(seed, round, MIFX_GS_SITE_ROWS);
    k_amax_s<<<grid_for(n), kThreads, 0, stream>>>(g, h, n, key, thr, w.amax, w.nsamp);
    k_quant_s<<<grid_for(n), kThreads, 0, stream>>>(g, h, n, key, thr, w, leaf_of_row);
  } else {
    k_amax<<<grid_for(n), kThreads, 0, stream>>>(g, h, n, w.amax);
    k_quant<<<grid_for(n), kThreads, 0, stream>>>(g, h, n, w);
  }
  const unsigned row_blocks = (unsigned)((n + kThreads - 1) / kThreads);
  const dim3 hist_grid((unsigned)((n + rows_per_wg - 1) / rows_per_wg), (unsigned)((f + feat_tile - 1) / feat_tile));
  const size_t lds = (size_t)feat_tile * kSlots * (2 * sizeof(long long) + sizeof(int));
  for (int d = 0; d <= max_depth; ++d) {
    Level &lv = w.lv[d & 1], &nx = w.lv[(d + 1) & 1];
    if (d < max_depth) {
      const uint8_t* lmask = level_mask ? level_mask + (size_t)d * f : nullptr;
      const size_t cells = ((size_t)1 << d) * hsize;
      hipError_t e = hipMemsetAsync(w.hg, 0, cells * sizeof(long long), stream);
      if (e == hipSuccess) e = hipMemsetAsync(w.hh, 0, cells * sizeof(long long), stream);
      if (e == hipSuccess) e = hipMemsetAsync(w.hc, 0, cells * sizeof(int), stream);
      if (e != hipSuccess) return (int)e;
      k_hist<<<hist_grid, kThreads, lds, stream>>>(lv, w.lcount, d, bins, w.perm[d & 1], w.qg, w.qh, n, f, nbins, hoff,
                                                   hsize, w.hg, w.hh, w.hc, rows_per_wg, feat_tile, lmask);
      const long waves = ((long)1 << d) * f;
      k_split<<<(unsigned)((waves + 3) / 4), kThreads, 0, stream>>>(lv, w.lcount, d, f, nbins, hoff, hsize, w.hg, w.hh,
                                                                    w.hc, w.exps, prm, w.cand, lmask);
    }
    k_decide<<<1, kThreads, 0, stream>>>(lv, nx, w.lcount, d, d == max_depth, f, w.cand, w.exps, prm, w.dec, w.cur, t,
                                         cap, w.ncount);
    k_partition<<<row_blocks, kThreads, 0, stream>>>(lv, w.lcount, d, w.dec, w.cur, bins, nbins, n, f, w.perm[d & 1],
                                                     w.perm[(d + 1) & 1], leaf_of_row, part_margin);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  if (sampled && margin) {  // the tree is complete: the rows that no leaf has updated
    k_apply<<<row_blocks, kThreads, 0, stream>>>(bins, n, f, nbins, t, cap, max_depth, margin,
                                                 margin_route == 1 ? nullptr : leaf_of_row);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return (int)hipMemcpyAsync(node_count, w.ncount, sizeof(int), hipMemcpyDeviceToDevice, stream);
}

int mifx_gbdt_gpu_grow_ex(const uint16_t* bins, long n, int f, const int* nbins, const int* hoff, int hsize,
                          const float* g, const float* h, int max_depth, double min_child_weight, double lambda,
                          double gamma, double eta, void* ws, long long ws_bytes, int* feature, int* split_bin,
                          uint8_t* default_left, int* left, int* right, double* value, int* node_count,
                          int* leaf_of_row, double* margin, int rows_per_wg, int feat_tile, unsigned long long seed,
                          unsigned long long round, unsigned long long thr, const uint8_t* level_mask,
                          int margin_route, hipStream_t stream) {
  return mifx_gbdt_gpu_grow_stats(bins, n, f, nbins, hoff, hsize, g, h, max_depth, min_child_weight, lambda, gamma, eta,
                                  ws, ws_bytes, feature, split_bin, default_left, left, right, value, node_count,
                                  leaf_of_row, margin, rows_per_wg, feat_tile, seed, round, thr, level_mask,
                                  margin_route, nullptr, nullptr, stream);
}

int mifx_gbdt_gpu_grow(const uint16_t* bins, long n, int f, const int* nbins, const int* hoff, int hsize,
                       const float* g, const float* h, int max_depth, double min_child_weight, double lambda,
                       double gamma, double eta, void* ws, long long ws_bytes, int* feature, int* split_bin,
                       uint8_t* default_left, int* left, int* right, double* value, int* node_count, int* leaf_of_row,
                       double* margin, int rows_per_wg, int feat_tile, hipStream_t stream) {
  return mifx_gbdt_gpu_grow_ex(bins, n, f, nbins, hoff, hsize, g, h, max_depth, min_child_weight, lambda, gamma, eta,
                               ws, ws_bytes, feature, split_bin, default_left, left, right, value, node_count,
                               leaf_of_row, margin, rows_per_wg, feat_tile, 0, 0, MIFX_GS_KEEP_ALL, nullptr, 0, stream);
}

// margin[i] += tree(row i) for a binned row-major [m, f] matrix (the eval set's margins)
int mifx_gbdt_gpu_apply(const uint16_t* bins, long m, int f, const int* nbins, const int* feature,
                        const int* split_bin, const uint8_t* default_left, const int* left, const int* right,
                        const double* value, int max_depth, double* margin, hipStream_t stream) {
  if (m < 1 || f < 1 || max_depth < 0 || max_depth > kMaxDepth) return -1;
  const TreeOut t{const_cast<int*>(feature), const_cast<int*>(split_bin), const_cast<uint8_t*>(default_left),
                  const_cast<int*>(left), const_cast<int*>(right), const_cast<double*>(value), nullptr, nullptr};
  k_apply<<<(unsigned)((m + kThreads - 1) / kThreads), kThreads, 0, stream>>>(bins, m, f, nbins, t,
                                                                               1 << (max_depth + 1), max_depth, margin,
                                                                               nullptr);
  return (int)hipGetLastError();
}

}  // extern "C"
