// Feature preparation and prediction of mifx.gbdt on the device: quantile cuts from a sorted column, binning of the
// raw table, and forest prediction on raw features. Each is bit-identical to its host function in gbdt.cpp
// (mifx_gbdt_cuts under ==, mifx_gbdt_bin, mifx_gbdt_predict); nothing here depends on launch geometry.
// MIFX_HIPCC_FLAGS: -ffp-contract=off
//
//   cuts     The host rule is a serial state machine over the distinct values of the sorted column v[0..m). Its
//            equivalent without serial state: with D distinct values, D <= max_bins keeps every distinct value but the
//            first; otherwise cut k (k = 1 .. max_bins - 1) is v[p], p = upper_bound(v, v[r - 1]),
//            r = max(1, ceil(k m / max_bins)), if p < m, repeats of one p dropped.
//            k_cut_mark counts the positions that start a run of equal values (wave-aggregated integer atomics) and
//            records the first kCutSlots of them, in whatever order the atomics land; k_cut_pick (one workgroup)
//            either ranks the recorded positions (D <= max_bins: all of them were recorded, and a set has one sorted
//            order) or runs the max_bins - 1 independent binary searches.
//   bins     k_bin: one workgroup per (row chunk, feature tile); the tile's cut tables are staged in LDS
//            (32 features x 255 cuts x 8 B = 65,280 B), bin = number of cuts <= x by binary search, NaN -> 0xFFFF.
//            Output row-major [n, f] uint16, the layout the learner (gbdt_gpu.hip) reads.
//   predict  k_predict: one row per thread; the forest is walked in tree order from packed 24-byte nodes, staged
//            through LDS in chunks of whole consecutive trees (a tree larger than a chunk is walked from global
//            memory). One double per row, additions only, in the host's order.
//            k_predict_multi: the same walk for a multi-class forest (tree t belongs to class t % K), one launch for
//            all K classes, one double per (class, row), per class the host's order.
//   contribs k_contribs: per-row feature contributions (path-dependent TreeSHAP) from the path table of gbdt_shap.h,
//            one row per thread, the table staged through LDS in chunks of whole leaves; mifx_gbdt_contribs bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gbdt_shap.h"

namespace {

constexpr int kMaxBins = 256;               // cuts: max_bins <= 256, so at most 255 cuts per feature
constexpr int kMaxCuts = kMaxBins - 1;
constexpr int kCutSlots = kMaxBins + 1;     // run starts recorded per column: enough to tell D <= max_bins apart
constexpr int kMaxFeatTile = 32;            // 32 * 255 * 8 B = 65,280 B of LDS
constexpr int kMaxRowsPerWg = 1 << 20;
constexpr int kMarkThreads = 256;
constexpr int kBinThreads = 512;
constexpr int kPredictThreads = 256;
constexpr int kMaxChunkNodes = 2730;        // 2730 * 24 B = 65,520 B of LDS

typedef unsigned long long u64;

struct PackedNode {  // 24 bytes; built once per model (mifx/ops/gbdt_prep.py)
  double v;          // inner node: the threshold (left iff x < v); leaf: the value
  int feature;       // < 0: leaf
  int left, right;   // local to the tree
  int default_left;
};

// ---- cuts

// state[0] = D, the number of run starts in v[0, m); pos[s] for s < min(D, kCutSlots): run-start positions, unordered
__global__ __launch_bounds__(kMarkThreads) void k_cut_mark(const double* v, long n, const long long* nan_count,
                                                           u64* state, long long* pos) {
  const long m = n - (long)*nan_count;
  const int lane = threadIdx.x & 63;
  // Slots matter only while the count is below kCutSlots, and it never falls: a wave that has seen it there stops
  // drawing slots and adds its own count once at the end (a column of distinct values would otherwise send one
  // atomic per wave and 64 rows to a single word). Every quantity below but `start` and `i` is wave-uniform.
  bool slots = true;
  u64 pending = 0;
  for (long base = (long)blockIdx.x * kMarkThreads; base < m; base += (long)gridDim.x * kMarkThreads) {
    const long i = base + threadIdx.x;
    const bool start = i < m && (i == 0 || v[i] != v[i - 1]);
    const u64 mask = __ballot(start);
    if (mask == 0) continue;
    if (!slots) {
      pending += __popcll(mask);
      continue;
    }
    const int leader = __ffsll((long long)mask) - 1;
    u64 first = 0;
    if (lane == leader) first = atomicAdd(&state[0], (u64)__popcll(mask));
    first = __shfl(first, leader);
    const u64 slot = first + __popcll(mask & (((u64)1 << lane) - 1));
    if (start && slot < (u64)kCutSlots) pos[slot] = i;
    slots = first + __popcll(mask) < (u64)kCutSlots;
  }
  if (pending && lane == 0) atomicAdd(&state[0], pending);
}

// one workgroup of kMaxBins threads: cuts[0 .. count) and *count from the state k_cut_mark left
__global__ __launch_bounds__(kMaxBins) void k_cut_pick(const double* v, long n, const long long* nan_count,
                                                       int max_bins, const u64* state, const long long* pos,
                                                       double* cuts, int* count) {
  __shared__ long long sp[kCutSlots];
  __shared__ int keep[kMaxBins];
  const long m = n - (long)*nan_count;
  const u64 D = state[0];
  const int t = threadIdx.x;
  if (m <= 0) {
    if (t == 0) *count = 0;
    return;
  }
  if (D <= (u64)max_bins) {  // one bin per distinct value: the run starts in ascending order, without the first
    const int d = (int)D;
    for (int s = t; s < d; s += kMaxBins) sp[s] = pos[s];
    __syncthreads();
    for (int s = t; s < d; s += kMaxBins) {
      const long long p = sp[s];
      int rank = 0;
      for (int q = 0; q < d; ++q) rank += sp[q] < p;
      if (rank > 0 && p >= 0 && p < m) cuts[rank - 1] = v[p];
    }
    if (t == 0) *count = d - 1;
    return;
  }
  // count quantiles: thread k - 1 searches for cut k
  const int k = t + 1;
  long p = m;
  if (k < max_bins) {
    const double total = (double)m;
    const double q = k * total / max_bins;  // the host's expression, in its operation order
    long r = (long)ceil(q);
    r = r < 1 ? 1 : (r > m ? m : r);
    const double a = v[r - 1];
    long lo = r, hi = m;  // upper_bound(v, a): the first index holding a greater value; v[r - 1] == a, so it is >= r
    while (lo < hi) {
      const long mid = lo + (hi - lo) / 2;
      if (v[mid] <= a) lo = mid + 1; else hi = mid;
    }
    p = lo;
  }
  sp[t] = p;
  __syncthreads();
  const bool kept = k < max_bins && p < m && (t == 0 || sp[t - 1] != p);
  keep[t] = kept;
  __syncthreads();
  int rank = 0;
  for (int q = 0; q < t; ++q) rank += keep[q];
  if (kept) cuts[rank] = v[p];
  if (t == kMaxBins - 1) *count = rank + (kept ? 1 : 0);
}

// ---- bins

template <class T>
__global__ __launch_bounds__(kBinThreads) void k_bin(const T* X, long n, int f, const double* cut_flat,
                                                     const int* cut_off, const int* ncut, uint16_t* bins,
                                                     int rows_per_wg, int feat_tile) {
  extern __shared__ double lds_cuts[];  // the tile's tables back to back
  __shared__ int loff[kMaxFeatTile + 1];
  const int j0 = blockIdx.y * feat_tile;
  const int tw = min(feat_tile, f - j0);
  if (threadIdx.x == 0) {
    int o = 0;
    for (int jj = 0; jj < tw; ++jj) {
      loff[jj] = o;
      o += min(max(ncut[j0 + jj], 0), kMaxCuts);
    }
    loff[tw] = o;
  }
  __syncthreads();
  for (int jj = 0; jj < tw; ++jj) {
    const double* src = cut_flat + cut_off[j0 + jj];
    const int c = loff[jj + 1] - loff[jj];
    for (int q = threadIdx.x; q < c; q += kBinThreads) lds_cuts[loff[jj] + q] = src[q];
  }
  __syncthreads();
  const long r0 = (long)blockIdx.x * rows_per_wg;
  const int rows = (int)min((long)rows_per_wg, n - r0);
  const int cells = rows * tw;  // rows_per_wg <= kMaxRowsPerWg: no overflow
  for (int e = threadIdx.x; e < cells; e += kBinThreads) {
    const long row = r0 + e / tw;
    const int jj = e % tw;
    const size_t at = (size_t)row * f + j0 + jj;
    const double a = (double)X[at];
    const double* c = lds_cuts + loff[jj];
    int lo = 0, hi = loff[jj + 1] - loff[jj];
    while (lo < hi) {  // the number of cuts <= a (std::upper_bound)
      const int mid = (lo + hi) >> 1;
      if (c[mid] <= a) lo = mid + 1; else hi = mid;
    }
    bins[at] = a != a ? (uint16_t)0xFFFF : (uint16_t)lo;
  }
}

// ---- predict

template <class T>
__device__ inline double walk(const PackedNode* nodes, int cnt, const T* xi) {
  int k = 0;
  PackedNode nd = nodes[0];
  for (int step = 1; step < cnt && nd.feature >= 0; ++step) {  // children have larger indices: < cnt steps
    const double a = (double)xi[nd.feature];
    const bool l = a != a ? nd.default_left != 0 : a < nd.v;
    k = l ? nd.left : nd.right;
    if ((unsigned)k >= (unsigned)cnt) return 0.0;  // refused on the host (validate_forest); never read past the tree
    nd = nodes[k];
  }
  return nd.v;
}

template <class T>
__global__ __launch_bounds__(kPredictThreads) void k_predict(const T* X, long n, int f, const PackedNode* nodes,
                                                             const int* tree_off, int n_trees, double base,
                                                             int nodes_per_chunk, double* out) {
  extern __shared__ double lds_raw[];
  PackedNode* lds = reinterpret_cast<PackedNode*>(lds_raw);
  const long i = (long)blockIdx.x * kPredictThreads + threadIdx.x;
  const T* xi = X + (size_t)(i < n ? i : 0) * f;
  double s = base;
  int t0 = 0;
  while (t0 < n_trees) {  // every quantity that steers this loop is uniform over the workgroup
    const int o0 = tree_off[t0];
    int t1 = t0;
    while (t1 < n_trees && tree_off[t1 + 1] - o0 <= nodes_per_chunk) ++t1;
    if (t1 == t0) {  // one tree larger than a chunk: from global memory
      if (i < n) s += walk(nodes + o0, tree_off[t0 + 1] - o0, xi);
      t0 += 1;
      continue;
    }
    const int total = tree_off[t1] - o0;
    __syncthreads();  // the previous chunk has been walked
    for (int q = threadIdx.x; q < total; q += kPredictThreads) lds[q] = nodes[o0 + q];
    __syncthreads();
    if (i < n)
      for (int t = t0; t < t1; ++t) s += walk(lds + (tree_off[t] - o0), tree_off[t + 1] - tree_off[t], xi);
    t0 = t1;
  }
  if (i < n) out[i] = s;
}

// Multi-class (multi:softprob): tree t belongs to class t % K, and class k's margin is base plus the outputs of trees
// k, k + K, k + 2K, ... below n_trees, added in that order: per class the additions of k_predict over the class's own
// trees, so the host's per-class mifx_gbdt_predict bit for bit. The forest is walked ONCE, with the chunk staging of
// k_predict. out is class-major [K, n]: a wave's 64 rows are 64 consecutive doubles of one class (coalesced), and it is
// the layout of the training margins. The class of a tree is uniform over the grid, so choosing its sum is a scalar
// branch. KT > 0 (K <= KT): the K sums stay in registers; acc[] is indexed by unrolled constants only, and the tree
// loop is unrolled over the classes so that tree t's output is added straight to acc[t % K]. They are stored once.
// KT == 0 (any K): the thread accumulates into its own K elements of out, initialised to base; no other thread
// touches them, so plain loads and stores.
constexpr int kRegClasses = 16;

// adds the outputs of trees [t0, t1) for one row, tree t to class t % K; nd: where node tree_off[t] - o0 lives
template <class T, int KT>
__device__ inline void add_trees(double* acc, double* out, long n, long i, const PackedNode* nd, int o0,
                                 const int* tree_off, int t0, int t1, int K, const T* xi) {
  int t = t0, c = t0 % K;
  if constexpr (KT > 0) {
    while (t < t1) {  // one pass adds up to K trees, classes ascending; the pass that starts at class c adds tree t
#pragma unroll
      for (int k = 0; k < KT; ++k)
        if (c == k && t < t1) {
          acc[k] += walk(nd + (tree_off[t] - o0), tree_off[t + 1] - tree_off[t], xi);
          ++t;
          c = k + 1 == K ? 0 : k + 1;
        }
    }
  } else {
    for (; t < t1; ++t) {
      out[(size_t)c * n + i] += walk(nd + (tree_off[t] - o0), tree_off[t + 1] - tree_off[t], xi);
      c = c + 1 == K ? 0 : c + 1;
    }
  }
}

template <class T, int KT>
__global__ __launch_bounds__(kPredictThreads) void k_predict_multi(const T* X, long n, int f, const PackedNode* nodes,
                                                                   const int* tree_off, int n_trees, int K,
                                                                   double base, int nodes_per_chunk, double* out) {
  extern __shared__ double lds_raw[];
  PackedNode* lds = reinterpret_cast<PackedNode*>(lds_raw);
  const long i = (long)blockIdx.x * kPredictThreads + threadIdx.x;
  const bool live = i < n;  // a thread past the table only helps staging: it never touches out
  const T* xi = X + (size_t)(live ? i : 0) * f;
  double acc[KT > 0 ? KT : 1];
#pragma unroll
  for (int k = 0; k < (KT > 0 ? KT : 1); ++k) acc[k] = base;
  if (KT == 0 && live)
    for (int k = 0; k < K; ++k) out[(size_t)k * n + i] = base;
  int t0 = 0;
  while (t0 < n_trees) {  // every quantity that steers this loop is uniform over the workgroup
    const int o0 = tree_off[t0];
    int t1 = t0;
    while (t1 < n_trees && tree_off[t1 + 1] - o0 <= nodes_per_chunk) ++t1;
    if (t1 == t0) {  // one tree larger than a chunk: from global memory
      if (live) add_trees<T, KT>(acc, out, n, i, nodes + o0, o0, tree_off, t0, t0 + 1, K, xi);
      t0 += 1;
      continue;
    }
    const int total = tree_off[t1] - o0;
    __syncthreads();  // the previous chunk has been walked
    for (int q = threadIdx.x; q < total; q += kPredictThreads) lds[q] = nodes[o0 + q];
    __syncthreads();
    if (live) add_trees<T, KT>(acc, out, n, i, lds, o0, tree_off, t0, t1, K, xi);
    t0 = t1;
  }
  if (KT > 0 && live) {
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (k < K) out[(size_t)k * n + i] = acc[k];
  }
}

template <class T>
void launch_predict_multi(const T* X, long n, int f, const PackedNode* nd, const int* tree_off, int n_trees, int K,
                          double base, int nodes_per_chunk, double* out, int in_registers, hipStream_t stream) {
  const unsigned grid = (unsigned)((n + kPredictThreads - 1) / kPredictThreads);
  const size_t lds = (size_t)nodes_per_chunk * sizeof(PackedNode);
  if (in_registers && K <= 8)
    k_predict_multi<T, 8><<<grid, kPredictThreads, lds, stream>>>(X, n, f, nd, tree_off, n_trees, K, base,
                                                                  nodes_per_chunk, out);
  else if (in_registers)
    k_predict_multi<T, kRegClasses><<<grid, kPredictThreads, lds, stream>>>(X, n, f, nd, tree_off, n_trees, K, base,
                                                                            nodes_per_chunk, out);
  else
    k_predict_multi<T, 0><<<grid, kPredictThreads, lds, stream>>>(X, n, f, nd, tree_off, n_trees, K, base,
                                                                  nodes_per_chunk, out);
}

// ---- contributions (path-dependent TreeSHAP in path form; gbdt_shap.h holds the one copy of the arithmetic)
//
// One row per thread. The path table is staged through LDS in chunks of whole leaves (a leaf is at most
// 1 + MIFX_SHAP_MAX_PATH records, so any chunk of that many records makes progress); every lane of the workgroup is at
// the same leaf at the same time, so m, every z and every feature index are uniform (LDS broadcasts, scalar branch on
// m) and only the o bits and the permutation weights differ per lane. The weights are registers: mifx_shap_leaf<M>
// indexes them by constants only. A row's f contributions accumulate in the thread's own slots, in the table's order:
//   ACC_LDS   slot j of thread t is lds[j * blockDim.x + t] (consecutive lanes, consecutive words); stored once. The
//             workgroup is 256, 128 or 64 threads, the largest whose f sums per thread fit beside the chunk
//   otherwise the thread's own output row (plain loads and stores: no other thread touches it)
// The same thread adds the same doubles in the same order either way, and in the order of the host's
// mifx_gbdt_contribs: the three agree bit for bit whatever the chunk size or the grid. The bias is one register.
constexpr int kContribThreads = 256;
constexpr int kMinContribChunk = 1 + MIFX_SHAP_MAX_PATH;
constexpr int kMaxContribLds = 65536;  // chunk records and, on the LDS route, the accumulators

template <class T, bool ACC_LDS>
__global__ __launch_bounds__(kContribThreads) void k_contribs(const T* X, long n, int f, const MifxShapRec* recs,
                                                              const int* leaf_off, int n_leaves, double base,
                                                              int chunk, double* out, long stride) {
  extern __shared__ double lds_raw[];
  MifxShapRec* lds = reinterpret_cast<MifxShapRec*>(lds_raw);
  double* acc = lds_raw + (size_t)chunk * (sizeof(MifxShapRec) / sizeof(double)) + threadIdx.x;
  const int nt = blockDim.x;
  const long i = (long)blockIdx.x * nt + threadIdx.x;
  const bool live = i < n;  // a thread past the table only helps staging: it never touches out
  const T* xi = X + (size_t)(live ? i : 0) * f;
  double* phi = out + (size_t)(live ? i : 0) * stride;
  if (ACC_LDS) {
    for (int j = 0; j < f; ++j) acc[(size_t)j * nt] = 0.0;
  } else if (live) {
    for (int j = 0; j < f; ++j) phi[j] = 0.0;
  }
  double bias = base;
  int l0 = 0;
  while (l0 < n_leaves) {  // every quantity that steers this loop is uniform over the workgroup
    const int o0 = leaf_off[l0];
    int lo = l0 + 1, hi = n_leaves;  // the last leaf boundary within a chunk of o0; l0 + 1 always is (validated)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (leaf_off[mid] - o0 <= chunk) lo = mid; else hi = mid - 1;
    }
    const int total = min(leaf_off[lo] - o0, chunk);
    __syncthreads();  // the previous chunk has been walked
    for (int q = threadIdx.x; q < total; q += nt) lds[q] = recs[o0 + q];
    __syncthreads();
    if (live) {
      int pos = 0;
      while (pos < total) {
        const int m = lds[pos].i;
        if (m < 0 || m > MIFX_SHAP_MAX_PATH || pos + 1 + m > total) break;  // refused on the host; never read past
        bias += lds[pos].b;
        if (m > 0) {
          const MifxShapRec* e = lds + pos + 1;
          unsigned obits = 0;
          for (int k = 0; k < m; ++k) {
            const int j = min(max(e[k].i, 0), f - 1);
            obits |= (unsigned)mifx_shap_passes(e[k], (double)xi[j]) << k;
          }
          const double v = lds[pos].a;
          if (ACC_LDS)
            mifx_shap_leaf_m(m, e, obits, v, [&](int j, double x) {
              if ((unsigned)j < (unsigned)f) acc[(size_t)j * nt] += x;
            });
          else
            mifx_shap_leaf_m(m, e, obits, v, [&](int j, double x) {
              if ((unsigned)j < (unsigned)f) phi[j] += x;
            });
        }
        pos += 1 + m;
      }
    }
    l0 = lo;
  }
  if (!live) return;
  if (ACC_LDS)
    for (int j = 0; j < f; ++j) phi[j] = acc[(size_t)j * nt];
  phi[f] = bias;
}

}  // namespace

extern "C" {

int mifx_gbdt_prep_contrib_rec_bytes() { return (int)sizeof(MifxShapRec); }
int mifx_gbdt_prep_contrib_min_chunk() { return kMinContribChunk; }
int mifx_gbdt_prep_contrib_max_lds() { return kMaxContribLds; }
int mifx_gbdt_prep_contrib_threads() { return kContribThreads; }

// Contributions of the first n_leaves leaves of a path table (mifx_gbdt_paths_build, validated on the host) for a
// row-major [n, f] table: out[i * stride + j], j < f, is feature j's contribution and out[i * stride + f] the bias
// (base plus every leaf's share), the bits of the host's mifx_gbdt_contribs. leaf_off [>= n_leaves + 1] on the device.
// chunk: records staged in LDS at a time; threads: 64, 128 or 256 per workgroup; acc_lds: 1 accumulates in LDS (needs
// chunk * 32 + f * threads * 8 bytes <= mifx_gbdt_prep_contrib_max_lds()), 0 in the output rows. None of the three
// changes a bit of the result.
int mifx_gbdt_prep_contribs(const void* X, int is_f64, long n, int f, const void* recs, const int* leaf_off,
                            int n_leaves, double base, int chunk, int threads, int acc_lds, double* out, long stride,
                            hipStream_t stream) {
  if (n < 1 || n >= (1L << 31) || f < 1 || n_leaves < 0 || chunk < kMinContribChunk || stride < f + 1 ||
      acc_lds < 0 || acc_lds > 1 || (threads != 64 && threads != 128 && threads != kContribThreads))
    return -1;
  const size_t lds = (size_t)chunk * sizeof(MifxShapRec) + (acc_lds ? (size_t)f * threads * sizeof(double) : 0);
  if (lds > (size_t)kMaxContribLds) return -1;
  const unsigned grid = (unsigned)((n + threads - 1) / threads);
  const MifxShapRec* r = static_cast<const MifxShapRec*>(recs);
#define MIFX_CONTRIBS(T, A) \
  k_contribs<T, A><<<grid, threads, lds, stream>>>(static_cast<const T*>(X), n, f, r, leaf_off, n_leaves, \
                                                           base, chunk, out, stride)
  if (is_f64 && acc_lds) MIFX_CONTRIBS(double, true);
  else if (is_f64) MIFX_CONTRIBS(double, false);
  else if (acc_lds) MIFX_CONTRIBS(float, true);
  else MIFX_CONTRIBS(float, false);
#undef MIFX_CONTRIBS
  return (int)hipGetLastError();
}

int mifx_gbdt_prep_max_bins() { return kMaxBins; }
int mifx_gbdt_prep_max_feat_tile() { return kMaxFeatTile; }
int mifx_gbdt_prep_max_chunk_nodes() { return kMaxChunkNodes; }
int mifx_gbdt_prep_node_bytes() { return (int)sizeof(PackedNode); }
int mifx_gbdt_prep_cut_scratch_bytes() { return (int)((1 + kCutSlots) * sizeof(long long)); }

// Cuts of one column. sorted: the column's n values ascending with the NaNs last (device); nan_count: their number
// (device, int64). Writes up to max_bins - 1 ascending cuts and their count (device). scratch: cut_scratch_bytes.
int mifx_gbdt_prep_cuts(const double* sorted, long n, const long long* nan_count, int max_bins, double* cuts,
                        int* count, void* scratch, int blocks, hipStream_t stream) {
  if (n < 1 || n >= (1L << 31) || max_bins < 2 || max_bins > kMaxBins || blocks < 1 || blocks > 65535) return -1;
  u64* state = static_cast<u64*>(scratch);
  long long* pos = static_cast<long long*>(scratch) + 1;
  const hipError_t e = hipMemsetAsync(state, 0, sizeof(u64), stream);
  if (e != hipSuccess) return (int)e;
  k_cut_mark<<<(unsigned)blocks, kMarkThreads, 0, stream>>>(sorted, n, nan_count, state, pos);
  k_cut_pick<<<1, kMaxBins, 0, stream>>>(sorted, n, nan_count, max_bins, state, pos, cuts, count);
  return (int)hipGetLastError();
}

// Bins of a row-major [n, f] table (is_f64: double, else float) into row-major [n, f] uint16. cut_flat / cut_off /
// ncut on the device; every ncut[j] <= 255 and every table inside cut_flat (checked by the caller on the host).
int mifx_gbdt_prep_bin(const void* X, int is_f64, long n, int f, const double* cut_flat, const int* cut_off,
                       const int* ncut, uint16_t* bins, int rows_per_wg, int feat_tile, hipStream_t stream) {
  if (n < 1 || n >= (1L << 31) || f < 1 || rows_per_wg < 1 || rows_per_wg > kMaxRowsPerWg || feat_tile < 1 ||
      feat_tile > kMaxFeatTile)
    return -1;
  const long tiles = ((long)f + feat_tile - 1) / feat_tile;
  if (tiles > 65535) return -1;
  const dim3 grid((unsigned)((n + rows_per_wg - 1) / rows_per_wg), (unsigned)tiles);
  const size_t lds = (size_t)feat_tile * kMaxCuts * sizeof(double);
  if (is_f64)
    k_bin<double><<<grid, kBinThreads, lds, stream>>>(static_cast<const double*>(X), n, f, cut_flat, cut_off, ncut,
                                                      bins, rows_per_wg, feat_tile);
  else
    k_bin<float><<<grid, kBinThreads, lds, stream>>>(static_cast<const float*>(X), n, f, cut_flat, cut_off, ncut,
                                                     bins, rows_per_wg, feat_tile);
  return (int)hipGetLastError();
}

// out[i] = base + the first n_trees trees' outputs for row i of a row-major [n, f] table. nodes: the packed forest;
// tree_off [trees + 1]: node offsets (both validated on the host before upload).
int mifx_gbdt_prep_predict(const void* X, int is_f64, long n, int f, const void* nodes, const int* tree_off,
                           int n_trees, double base, int nodes_per_chunk, double* out, hipStream_t stream) {
  if (n < 1 || n >= (1L << 31) || f < 1 || n_trees < 0 || nodes_per_chunk < 1 || nodes_per_chunk > kMaxChunkNodes)
    return -1;
  const unsigned grid = (unsigned)((n + kPredictThreads - 1) / kPredictThreads);
  const size_t lds = (size_t)nodes_per_chunk * sizeof(PackedNode);
  const PackedNode* nd = static_cast<const PackedNode*>(nodes);
  if (is_f64)
    k_predict<double><<<grid, kPredictThreads, lds, stream>>>(static_cast<const double*>(X), n, f, nd, tree_off,
                                                              n_trees, base, nodes_per_chunk, out);
  else
    k_predict<float><<<grid, kPredictThreads, lds, stream>>>(static_cast<const float*>(X), n, f, nd, tree_off,
                                                             n_trees, base, nodes_per_chunk, out);
  return (int)hipGetLastError();
}

int mifx_gbdt_prep_reg_classes() { return kRegClasses; }

// Multi-class margins in one launch: out [num_class, n] (class-major); out[k, i] = base + the outputs for row i of
// trees k, k + num_class, ... below n_trees, in that order. in_registers: 1 keeps the class sums in registers (needs
// num_class <= mifx_gbdt_prep_reg_classes()), 0 accumulates in out itself (any num_class). The same bits either way.
int mifx_gbdt_prep_predict_multi(const void* X, int is_f64, long n, int f, const void* nodes, const int* tree_off,
                                 int n_trees, int num_class, double base, int nodes_per_chunk, double* out,
                                 int in_registers, hipStream_t stream) {
  if (n < 1 || n >= (1L << 31) || f < 1 || n_trees < 0 || nodes_per_chunk < 1 || nodes_per_chunk > kMaxChunkNodes ||
      num_class < 1 || in_registers < 0 || in_registers > 1 || (in_registers && num_class > kRegClasses))
    return -1;
  const PackedNode* nd = static_cast<const PackedNode*>(nodes);
  if (is_f64)
    launch_predict_multi(static_cast<const double*>(X), n, f, nd, tree_off, n_trees, num_class, base, nodes_per_chunk,
                         out, in_registers, stream);
  else
    launch_predict_multi(static_cast<const float*>(X), n, f, nd, tree_off, n_trees, num_class, base, nodes_per_chunk,
                         out, in_registers, stream);
  return (int)hipGetLastError();
}

}  // extern "C"
