// MIFX_HIPCC_FLAGS: -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops
// The absolute-error and quantile objectives of mifx.gbdt on the device: their gradient pair and the exact leaf
// refresh of gbdt_quantile.h, a segmented weighted radix select over the leaves of one finished tree. Input: leaf_of_row
// [n] (-1: a row outside the sample), the tree's value array, the margins from before the tree, y and the float32
// hessians the tree was grown from. Output: value[l] = eta * quantile_l for every leaf l of total weight > 0. Everything
// stays on the device and on the caller's stream, nothing is read back, and the number of launches depends only on
// whether n exceeds the small-segment capacity.
//
//   k_q_init     clears the per-leaf row counts and the scalars (kernels, not memsets: the sequence can be captured).
//   k_q_count    per-leaf row counts in LDS-privatised counters (one int per node id, <= 32 KB), flushed with integer
//                atomics; the largest |h| (as its bit pattern) and the number of rows that have a leaf, for the
//                exponent of the integer weights.
//   k_q_scan     one workgroup: exclusive scan of the counts into segment offsets and scatter cursors; the exponent;
//                the list of LARGE segments (more rows than one workgroup selects from LDS), each with a slot, and
//                the table of their row chunks (slot, first position).
//   k_q_scatter  a tile of 2048 rows per workgroup and trip: every row draws its rank among the tile's rows of its leaf
//                from an LDS counter, the tile then draws one range per leaf from the leaf's global cursor, and the
//                rows store (key, weight) -- key = mifx_sort_key(y - margin), weight = the quantised hessian -- at
//                range + rank. The order inside a segment depends on the atomics; the selection below does not.
//   k_q_small    one workgroup per node id whose segment fits in LDS (<= 4096 rows: 64 KB of keys and weights, staged
//                once). OR and AND of the keys give the bits that vary inside the segment; the select walks the 8-bit
//                digits from the top and runs a pass only for a digit that holds a varying bit (a near-constant leaf
//                varies in its low digits only; float32-widened residuals of ONE sign have 29 constant low bits, but
//                a negative value's key is its complement, so a leaf of mixed signs varies in every digit). A pass is
//                a 256-bucket int64 weight histogram over the keys that match the digits chosen so far (LDS atomics on
//                integers), then one wave scans it for the bucket where the running weight reaches the remaining T.
//   large segments, cut into chunks of rows_per_wg rows over several workgroups:
//     k_q_lstats   OR / AND / total weight per segment (integer atomics on the slot)
//     k_q_lnarrow  one wave per slot. First call: T from the total, the selection starts from the AND word. After each
//                  histogram pass: scan the slot's 256 global buckets, fix the digit, reduce T, clear the buckets. The
//                  call after the lowest digit writes the leaf value.
//     k_q_lhist    per chunk: the LDS histogram of the digit over the matching keys, flushed with integer atomics into
//                  the slot's global buckets. A chunk whose segment does not vary in the digit returns at once.
//
// No floating-point atomics: every sum is int64 (|q_i| <= 2^(60 - bitlen(ns)), so any subset sums below 2^61) and every
// comparison is on integers, so rows_per_wg, grid sizes and the order of atomics change no bit of the result, and the
// host's mifx_gbdt_leaf_refresh (csrc/gbdt.cpp), a plain sort per leaf, gives the same values bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gbdt_quantile.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxNodes = 8192;   // node ids of a tree: 2^13 (depth-wise, depth 12) or 2 * 4096 - 1 (leaf-wise)
constexpr int kSmall = 4096;      // rows of a segment that one workgroup selects from LDS
constexpr int kPer = 8;           // rows per thread of a scatter tile
constexpr int kTile = kThreads * kPer;
constexpr int kRowsPerWg = 8192;  // default chunk of a large segment
constexpr int kMaxGrid = 2048;

typedef unsigned long long u64;

enum { M_AMAX = 0, M_NSAMP, M_EH, M_NLARGE, M_NCHUNK, M_PASSES, M_LEAVES, M_COUNT };

struct Ws {
  u64* keys;       // [n] the rows' keys, segment by segment
  long long* qs;   // [n] their weights
  int* count;      // [nodes] rows per leaf
  int* off;        // [nodes + 1] segment starts
  int* cur;        // [nodes] scatter cursors
  int* meta;       // [M_COUNT]
  int* s_leaf;     // [S] large slots: the leaf,
  u64 *s_or, *s_and, *s_sel;  // OR / AND of its keys, the key selected so far,
  long long *s_q, *s_t;       // its total weight, the weight still to reach
  long long* ghist;           // [S, 256]
  int *c_slot, *c_begin;      // [C] chunks of the large segments
  int S, C;
  size_t bytes;
};

Ws carve(char* base, long n, int nodes, int small_cap, int chunk) {
  Ws w;
  size_t used = 0;
  const auto take = [&](size_t bytes) {
    char* r = base ? base + used : nullptr;
    used += (bytes + 255) & ~(size_t)255;
    return r;
  };
  w.S = (int)(n / ((long)small_cap + 1)) + 1;
  w.C = (int)(n / chunk) + w.S + 1;
  w.keys = (u64*)take((size_t)n * 8);
  w.qs = (long long*)take((size_t)n * 8);
  w.count = (int*)take((size_t)nodes * 4);
  w.off = (int*)take((size_t)(nodes + 1) * 4);
  w.cur = (int*)take((size_t)nodes * 4);
  w.meta = (int*)take(M_COUNT * 4);
  w.s_leaf = (int*)take((size_t)w.S * 4);
  w.s_or = (u64*)take((size_t)w.S * 8);
  w.s_and = (u64*)take((size_t)w.S * 8);
  w.s_sel = (u64*)take((size_t)w.S * 8);
  w.s_q = (long long*)take((size_t)w.S * 8);
  w.s_t = (long long*)take((size_t)w.S * 8);
  w.ghist = (long long*)take((size_t)w.S * 256 * 8);
  w.c_slot = (int*)take((size_t)w.C * 4);
  w.c_begin = (int*)take((size_t)w.C * 4);
  w.bytes = used;
  return w;
}

__device__ __forceinline__ void add64(long long* p, long long v) { atomicAdd(reinterpret_cast<u64*>(p), (u64)v); }

__device__ __forceinline__ u64 shfl_xor64(u64 v, int o) { return (u64)__shfl_xor((long long)v, o); }

// ---- gradients: mifx_gq_grad times the float32 weight, one IEEE multiply each (XGBRegressor._grad_hess)
__global__ void k_q_grad(const double* margin, const double* y, const float* wt, long n, double alpha, float* g,
                         float* h) {
  const long i = blockIdx.x * (long)kThreads + threadIdx.x;
  if (i >= n) return;
  float gi = mifx_gq_grad(margin[i], y[i], alpha), hi = 1.0f;
  if (wt) {
    gi = gi * wt[i];
    hi = hi * wt[i];
  }
  g[i] = gi;
  h[i] = hi;
}

// ---- counts
__global__ void k_q_init(Ws w, int nodes) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < nodes) w.count[i] = 0;
  if (i < M_COUNT) w.meta[i] = 0;
}

__global__ __launch_bounds__(kThreads) void k_q_count(const int* leaf_of_row, const float* h, long n, int nodes, Ws w) {
  __shared__ int s_cnt[kMaxNodes];
  for (int l = threadIdx.x; l < nodes; l += kThreads) s_cnt[l] = 0;
  __syncthreads();
  unsigned mh = 0;
  int c = 0;
  for (long i = blockIdx.x * (long)kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    const int l = leaf_of_row[i];
    if (l < 0 || l >= nodes) continue;
    atomicAdd(&s_cnt[l], 1);
    mh = max(mh, __float_as_uint(fabsf(h[i])));
    ++c;
  }
  for (int o = 32; o; o >>= 1) {
    mh = max(mh, (unsigned)__shfl_xor((int)mh, o));
    c += __shfl_xor(c, o);
  }
  if ((threadIdx.x & 63) == 0 && c) {
    atomicMax(reinterpret_cast<unsigned*>(w.meta + M_AMAX), mh);
    atomicAdd(w.meta + M_NSAMP, c);
  }
  __syncthreads();
  for (int l = threadIdx.x; l < nodes; l += kThreads) {
    const int v = s_cnt[l];
    if (v) atomicAdd(&w.count[l], v);
  }
}

// ---- segments: offsets, cursors, the large segments' slots and chunks
__global__ __launch_bounds__(kThreads) void k_q_scan(Ws w, int nodes, int small_cap, int chunk) {
  __shared__ int s_a[kThreads], s_b[kThreads], s_c[kThreads];
  __shared__ int carry[3];
  const int t = threadIdx.x;
  if (t < 3) carry[t] = 0;
  __syncthreads();
  for (int base = 0; base < nodes; base += kThreads) {
    const int l = base + t;
    const int c = l < nodes ? w.count[l] : 0;
    const int big = c > small_cap;
    const int nch = big ? (int)(((long)c + chunk - 1) / chunk) : 0;
    s_a[t] = c;
    s_b[t] = big;
    s_c[t] = nch;
    __syncthreads();
    for (int o = 1; o < kThreads; o <<= 1) {  // inclusive scans of the three
      const int a = t >= o ? s_a[t - o] : 0, b = t >= o ? s_b[t - o] : 0, d = t >= o ? s_c[t - o] : 0;
      __syncthreads();
      s_a[t] += a;
      s_b[t] += b;
      s_c[t] += d;
      __syncthreads();
    }
    const int eo = carry[0] + s_a[t] - c, es = carry[1] + s_b[t] - big, ec = carry[2] + s_c[t] - nch;
    if (l < nodes) {
      w.off[l] = eo;
      w.cur[l] = eo;
      if (big && es < w.S) {
        w.s_leaf[es] = l;
        w.s_or[es] = 0;
        w.s_and[es] = ~(u64)0;
        w.s_q[es] = 0;
        for (int j = 0; j < nch && ec + j < w.C; ++j) {
          w.c_slot[ec + j] = es;
          w.c_begin[ec + j] = eo + j * chunk;
        }
      }
    }
    __syncthreads();
    if (t == kThreads - 1) {
      carry[0] += s_a[t];
      carry[1] += s_b[t];
      carry[2] += s_c[t];
    }
    __syncthreads();
  }
  if (t == 0) {
    w.off[nodes] = carry[0];
    w.meta[M_NLARGE] = min(carry[1], w.S);
    w.meta[M_NCHUNK] = min(carry[2], w.C);
    w.meta[M_EH] = mifx_gq_exp((double)__uint_as_float((unsigned)w.meta[M_AMAX]), w.meta[M_NSAMP]);
  }
}

__global__ __launch_bounds__(kThreads) void k_q_scatter(const int* leaf_of_row, const double* margin, const double* y,
                                                        const float* h, long n, int nodes, Ws w) {
  __shared__ int s_cnt[kMaxNodes];
  const int eh = w.meta[M_EH];
  const long tiles = (n + kTile - 1) / kTile;
  for (long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    for (int l = threadIdx.x; l < nodes; l += kThreads) s_cnt[l] = 0;
    __syncthreads();
    int lf[kPer], rank[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const long i = tl * kTile + j * kThreads + threadIdx.x;
      int l = i < n ? leaf_of_row[i] : -1;
      if (l >= nodes) l = -1;
      lf[j] = l;
      rank[j] = l >= 0 ? atomicAdd(&s_cnt[l], 1) : 0;
    }
    __syncthreads();
    for (int l = threadIdx.x; l < nodes; l += kThreads) {  // the tile's range of every leaf it holds rows of
      const int c = s_cnt[l];
      if (c) s_cnt[l] = atomicAdd(&w.cur[l], c);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (lf[j] < 0) continue;
      const long i = tl * kTile + j * kThreads + threadIdx.x;
      const long pos = (long)s_cnt[lf[j]] + rank[j];
      if (pos < 0 || pos >= n) continue;
      w.keys[pos] = mifx_gq_key(y[i], margin[i]);
      w.qs[pos] = mifx_gq_weight(h[i], eh);
    }
    __syncthreads();
  }
}

// ---- select
// OR, AND and sum over the workgroup; every thread receives them
__device__ __forceinline__ void block_stats(u64& vor, u64& vand, long long& q, u64* s_or, u64* s_and, long long* s_q) {
  for (int o = 32; o; o >>= 1) {
    vor |= shfl_xor64(vor, o);
    vand &= shfl_xor64(vand, o);
    q += __shfl_xor(q, o);
  }
  if ((threadIdx.x & 63) == 0) {
    s_or[threadIdx.x >> 6] = vor;
    s_and[threadIdx.x >> 6] = vand;
    s_q[threadIdx.x >> 6] = q;
  }
  __syncthreads();
  vor = 0, vand = ~(u64)0, q = 0;
  for (int v = 0; v < kWaves; ++v) {
    vor |= s_or[v];
    vand &= s_and[v];
    q += s_q[v];
  }
}

// One wave: the first of 256 buckets at which the running sum reaches t (1 <= t <= the buckets' total); *before
// receives the sum of the buckets below it. Lane i holds buckets 4 i .. 4 i + 3. Every lane returns the result.
__device__ __forceinline__ int pick_bucket(const long long* hist, long long t, long long* before) {
  const int lane = threadIdx.x & 63;
  long long s[4], tot = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) tot += s[j] = hist[4 * lane + j];
  long long incl = tot;
  for (int o = 1; o < 64; o <<= 1) {
    const long long up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  long long run = incl - tot;
  const bool mine = run < t && t <= incl;
  int b = 0;
  if (mine) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (run + s[j] >= t) {
        b = 4 * lane + j;
        break;
      }
      run += s[j];
    }
  }
  const u64 m = __ballot(mine);
  const int src = m ? __ffsll((long long)m) - 1 : 0;  // (m is never empty for a t in range)
  *before = __shfl(run, src);
  return __shfl(b, src);
}

__device__ __forceinline__ bool digit_varies(u64 vary, int d) { return ((vary >> (8 * d)) & 0xFF) != 0; }

// does key k agree with the selection in every digit above d
__device__ __forceinline__ bool matches(u64 k, u64 sel, int d) { return d == 7 || ((k ^ sel) >> (8 * (d + 1))) == 0; }

__device__ __forceinline__ u64 set_digit(u64 sel, int d, int b) {
  return (sel & ~((u64)0xFF << (8 * d))) | ((u64)b << (8 * d));
}

__global__ __launch_bounds__(kThreads) void k_q_small(Ws w, int small_cap, double alpha, double eta, double* value) {
  extern __shared__ u64 lds[];  // keys [small_cap], weights [small_cap]
  __shared__ long long hist[256];
  __shared__ u64 s_or[kWaves], s_and[kWaves];
  __shared__ long long s_q[kWaves], s_t;
  __shared__ int s_b;
  const int l = blockIdx.x, t = threadIdx.x;
  const int c = w.count[l];
  if (c <= 0 || c > small_cap) return;
  u64* keys = lds;
  long long* qs = reinterpret_cast<long long*>(lds + small_cap);
  const int begin = w.off[l];
  u64 vor = 0, vand = ~(u64)0;
  long long Q = 0;
  for (int i = t; i < c; i += kThreads) {
    const u64 k = w.keys[begin + i];
    const long long q = w.qs[begin + i];
    keys[i] = k;
    qs[i] = q;
    vor |= k;
    vand &= k;
    Q += q;
  }
  block_stats(vor, vand, Q, s_or, s_and, s_q);
  if (Q <= 0) return;
  long long T = mifx_gq_threshold(alpha, Q);
  u64 sel = vand;
  const u64 vary = vor ^ vand;
  int passes = 0;
  for (int d = 7; d >= 0; --d) {
    if (!digit_varies(vary, d)) continue;
    ++passes;
    hist[t] = 0;
    __syncthreads();
    for (int i = t; i < c; i += kThreads) {
      const u64 k = keys[i];
      const long long q = qs[i];
      if (q != 0 && matches(k, sel, d)) add64(&hist[(k >> (8 * d)) & 0xFF], q);
    }
    __syncthreads();
    if (t < 64) {
      long long before;
      const int b = pick_bucket(hist, T, &before);
      if (t == 0) {
        s_b = b;
        s_t = T - before;
      }
    }
    __syncthreads();
    sel = set_digit(sel, d, s_b);
    T = s_t;
    __syncthreads();
  }
  if (t == 0) {
    value[l] = mifx_gq_value(sel, eta);
    atomicAdd(w.meta + M_PASSES, passes);
    atomicAdd(w.meta + M_LEAVES, 1);
  }
}

// the chunk of this workgroup: false if there is none
__device__ __forceinline__ bool chunk_of(const Ws& w, int chunk, int* slot, int* begin, int* end) {
  const int idx = blockIdx.x;
  if (idx >= w.meta[M_NCHUNK]) return false;
  *slot = w.c_slot[idx];
  *begin = w.c_begin[idx];
  const int leaf = w.s_leaf[*slot];
  *end = (int)min((long)*begin + chunk, (long)w.off[leaf + 1]);
  return true;
}

__global__ __launch_bounds__(kThreads) void k_q_lstats(Ws w, int chunk) {
  __shared__ u64 s_or[kWaves], s_and[kWaves];
  __shared__ long long s_q[kWaves];
  int slot, begin, end;
  if (!chunk_of(w, chunk, &slot, &begin, &end)) return;
  u64 vor = 0, vand = ~(u64)0;
  long long Q = 0;
  for (int i = begin + threadIdx.x; i < end; i += kThreads) {
    const u64 k = w.keys[i];
    vor |= k;
    vand &= k;
    Q += w.qs[i];
  }
  block_stats(vor, vand, Q, s_or, s_and, s_q);
  if (threadIdx.x == 0) {
    atomicOr(&w.s_or[slot], vor);
    atomicAnd(&w.s_and[slot], vand);
    if (Q) add64(&w.s_q[slot], Q);
  }
}

// one wave per slot; d = 8: before the first pass, d in [0, 8): after the histogram pass of digit d
__global__ __launch_bounds__(64) void k_q_lnarrow(Ws w, int d, double alpha, double eta, double* value) {
  const int slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= w.meta[M_NLARGE]) return;
  const long long Q = w.s_q[slot];
  long long* hist = w.ghist + (size_t)slot * 256;
  if (d == 8) {
    if (lane == 0) {
      w.s_t[slot] = Q > 0 ? mifx_gq_threshold(alpha, Q) : 0;
      w.s_sel[slot] = w.s_and[slot];
    }
    for (int j = 0; j < 4; ++j) hist[4 * lane + j] = 0;
    return;
  }
  if (Q <= 0) return;
  u64 sel = w.s_sel[slot];
  const bool ran = digit_varies(w.s_or[slot] ^ w.s_and[slot], d);
  if (ran) {
    long long before;
    const int b = pick_bucket(hist, w.s_t[slot], &before);
    sel = set_digit(sel, d, b);
    for (int j = 0; j < 4; ++j) hist[4 * lane + j] = 0;  // (every lane has read its buckets inside pick_bucket)
    if (lane == 0) {
      w.s_sel[slot] = sel;
      w.s_t[slot] -= before;
      atomicAdd(w.meta + M_PASSES, 1);
    }
  }
  if (d == 0 && lane == 0) {
    value[w.s_leaf[slot]] = mifx_gq_value(sel, eta);
    atomicAdd(w.meta + M_LEAVES, 1);
  }
}

__global__ __launch_bounds__(kThreads) void k_q_lhist(Ws w, int chunk, int d) {
  __shared__ long long hist[256];
  int slot, begin, end;
  if (!chunk_of(w, chunk, &slot, &begin, &end)) return;
  if (w.s_q[slot] <= 0 || !digit_varies(w.s_or[slot] ^ w.s_and[slot], d)) return;
  const u64 sel = w.s_sel[slot];
  hist[threadIdx.x] = 0;
  __syncthreads();
  for (int i = begin + threadIdx.x; i < end; i += kThreads) {
    const u64 k = w.keys[i];
    if (!matches(k, sel, d)) continue;
    const long long q = w.qs[i];
    if (q != 0) add64(&hist[(k >> (8 * d)) & 0xFF], q);
  }
  __syncthreads();
  const long long v = hist[threadIdx.x];
  if (v) add64(&w.ghist[(size_t)slot * 256 + threadIdx.x], v);
}

bool args_ok(long n, int nodes, int rows_per_wg) {
  return n >= 1 && n < (1L << 31) && nodes >= 1 && nodes <= kMaxNodes && rows_per_wg >= 1;
}

}  // namespace

extern "C" {

int mifx_gbdt_q_max_nodes() { return kMaxNodes; }
int mifx_gbdt_q_rows_per_wg() { return kRowsPerWg; }

// bytes of workspace for mifx_gbdt_q_refresh (16 n and small change); -1 on arguments out of range
long long mifx_gbdt_q_ws_bytes(long n, int nodes, int rows_per_wg) {
  if (!args_ok(n, nodes, rows_per_wg)) return -1;
  return (long long)carve(nullptr, n, nodes, std::min(kSmall, rows_per_wg), rows_per_wg).bytes;
}

// g, h of reg:absoluteerror (alpha < 0) or reg:quantileerror (alpha in (0, 1)); weight (float32 [n], nullable)
int mifx_gbdt_q_grad(const double* margin, const double* y, const float* weight, long n, double alpha, float* g,
                     float* h, hipStream_t stream) {
  if (n < 1 || !(alpha < 1.0)) return -1;
  k_q_grad<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, stream>>>(margin, y, weight, n, alpha, g, h);
  return (int)hipGetLastError();
}

// The leaf refresh: value [nodes] of the tree that left leaf_of_row [n]; margin [n] from before the tree. rows_per_wg:
// launch geometry (the chunk of a large segment; a segment of more than min(4096, rows_per_wg) rows is large): the
// result does not depend on it.
int mifx_gbdt_q_refresh(const int* leaf_of_row, double* value, const double* margin, const double* y, const float* h,
                        long n, int nodes, double alpha, double eta, void* ws, long long ws_bytes, int rows_per_wg,
                        hipStream_t stream) {
  if (!args_ok(n, nodes, rows_per_wg) || !(alpha > 0.0 && alpha < 1.0) || !ws) return -1;
  const int small_cap = std::min(kSmall, rows_per_wg);
  const Ws w = carve((char*)ws, n, nodes, small_cap, rows_per_wg);
  if (ws_bytes < (long long)w.bytes) return -1;
  const size_t lds = (size_t)small_cap * 16;
  if (lds > 32768) (void)hipFuncSetAttribute((const void*)k_q_small, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const int row_grid = (int)std::min<long>((n + kThreads - 1) / kThreads, kMaxGrid);
  const int tile_grid = (int)std::min<long>((n + kTile - 1) / kTile, kMaxGrid);
  k_q_init<<<(nodes + kThreads - 1) / kThreads, kThreads, 0, stream>>>(w, nodes);
  k_q_count<<<row_grid, kThreads, 0, stream>>>(leaf_of_row, h, n, nodes, w);
  k_q_scan<<<1, kThreads, 0, stream>>>(w, nodes, small_cap, rows_per_wg);
  k_q_scatter<<<tile_grid, kThreads, 0, stream>>>(leaf_of_row, margin, y, h, n, nodes, w);
  k_q_small<<<nodes, kThreads, lds, stream>>>(w, small_cap, alpha, eta, value);
  if (n > small_cap) {  // a large segment can exist
    k_q_lstats<<<w.C, kThreads, 0, stream>>>(w, rows_per_wg);
    k_q_lnarrow<<<w.S, 64, 0, stream>>>(w, 8, alpha, eta, value);
    for (int d = 7; d >= 0; --d) {
      k_q_lhist<<<w.C, kThreads, 0, stream>>>(w, rows_per_wg, d);
      k_q_lnarrow<<<w.S, 64, 0, stream>>>(w, d, alpha, eta, value);
    }
  }
  return (int)hipGetLastError();
}

// what the last refresh on `ws` did, for measurements (synchronises): out[0] select passes run, out[1] leaves refreshed
int mifx_gbdt_q_stats(const void* ws, long n, int nodes, int rows_per_wg, int* out, hipStream_t stream) {
  if (!args_ok(n, nodes, rows_per_wg)) return -1;
  const Ws w = carve((char*)ws, n, nodes, std::min(kSmall, rows_per_wg), rows_per_wg);
  hipError_t e = hipMemcpyAsync(out, w.meta + M_PASSES, 2 * sizeof(int), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  return (int)e;
}

}  // extern "C"
