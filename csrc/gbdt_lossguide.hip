// Leaf-wise device grower of mifx.gbdt (grow_policy="lossguide", max_leaves): always split the open leaf with the
// largest gain, stop at a leaf budget. One node per expansion, nothing read back inside a tree.
// MIFX_HIPCC_FLAGS: -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops
//
// Semantics: the fixed-point learner of gbdt_split.h, as csrc/gbdt_gpu.hip; the host twin is
// mifx_gbdt_grow_fixed_lossguide_stats (csrc/gbdt.cpp), which this file reproduces bit for bit. The rule: the root is
// node 0; a node is closed as a leaf if it has fewer than two rows, if mifx_gb_is_leaf holds for its candidate, or if
// its depth equals max_depth (> 0; 0 = no limit). While fewer than max_leaves leaves exist and a node is open, the
// open node with the largest gain (ties: lowest id) is split and its children take the next two ids, left then right.
//
// State on the device:
//   node table  per node (2 * max_leaves - 1 of them): row range [begin, end), which of the two permutation arrays
//               holds it (a split writes both children into the OTHER array at the same offsets: ping-pong per node),
//               depth, quantised sums, histogram slot, its stored candidate, its state (closed / open / split /
//               pending = created by this expansion, candidate not yet known)
//   pool        max_leaves histogram slots of hsize entries (int64 g, int64 h, int32 rows). The smaller child of a
//               split (by rows, ties: left) gets a fresh slot and is built from its rows; the parent's slot becomes the
//               larger child's by in-place subtraction. In int64 built and subtracted histograms are identical.
//   ctrl        counters and the current expansion (parent, smaller and larger child), written by k_pick
//
// The host enqueues max_leaves - 1 expansions of four kernels; every kernel reads what to do from ctrl, and after the
// tree is finished (budget reached or nothing open) the remaining launches return at once:
//   k_pick   one workgroup: argmax over the open nodes (gain descending, id ascending); writes the parent's tree entry,
//            creates the children (ranges from the stored left count, sums, slots, their leaf entries) and zeroes the
//            fresh slot. Children that can never be split (depth limit, or the budget is reached by this split) are
//            closed here and the expansion's histogram and split kernels return at once.
//   k_part   a fixed grid of waves striding over the parent's range only: ballots, two atomics per wave for the
//            children's cursors. Row order inside a child is not deterministic; nothing depends on it.
//   k_hist   a fixed grid of (row chunk x feature tile) workgroups striding over the smaller child's range: one LDS
//            histogram per workgroup over ALL its chunks (a subset of the rows sums below 2^61), non-empty slots flushed
//            once with 64-bit global atomics
//   k_split  one workgroup per child, a wave per feature at a time: the wave stages the feature's histogram in LDS (for
//            the larger child it forms parent - smaller on the way and writes it back), lanes own runs of 4 bins,
//            integer prefix scan, mifx_gb_scan, lanes merged with mifx_gb_lower_wins; then one thread walks the
//            features in order (1e-12 rule), applies the leaf test and stores candidate and state in the table
// The root goes through the quantise stage of gbdt_quant.h (with the row compaction of subsample < 1), k_root, and the
// same k_hist and k_split with "smaller child" = root. k_finish gives every row of a leaf its leaf_of_row and
// margin += value; rows outside the sample are walked through the finished tree (k_walk), at most the tree's real
// depth steps. colsample_bytree reaches k_hist / k_split as one [f] uint8 mask per tree.
//
// monotone_constraints (mifx_gbdt_lg_grow_mono; the rule is gbdt_split.h's, the host twin
// mifx_gbdt_grow_fixed_lossguide_mono): the node table holds every node's weight interval (two doubles more per node);
// k_root and k_pick write it and clamp the leaf entries, k_split_mono takes k_split's place.
//
// interaction_constraints / colsample_bynode (mifx_gbdt_lg_grow_nodeset; the rule is gbdt_nodeset.h's, the host twin
// mifx_gbdt_grow_lossguide_nodeset): the node table holds every node's path set and mask row; k_root and k_pick write
// the sets, k_nodeset (a wave per child) the rows. A row has two bits per feature: the histogram set (the level set and
// A(S): it only shrinks down the tree, so the parent's slot serves the larger child by subtraction) decides what k_hist
// builds and what k_split stages and subtracts, the split set (the by-node draw too) what a wave searches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gbdt_nodeset.h"
#include "gbdt_quant.h"
#include "gbdt_sample.h"
#include "gbdt_split.h"
#include "gbdt_wave.h"

namespace {

constexpr int kMaxBins = 256;         // bins per feature
constexpr int kSlots = kMaxBins + 1;  // LDS slots per feature: the bins and "missing"
constexpr int kMaxDepth = 12;         // the limit on a max_depth > 0 (the depth-wise grower's)
constexpr int kMaxLeaves = 4096;
constexpr int kMaxFeatTile = 12;  // 12 * 257 * 20 B = 61,680 B of LDS
constexpr int kSplitWaves = 8;    // k_split: 8 * 257 * 20 B = 41,120 B of LDS

enum State { CLOSED = 0, OPEN = 1, SPLIT = 2, PENDING = 3 };
enum Ctrl { C_DONE, C_NODES, C_LEAVES, C_SLOTS, C_DEPTH, C_CUR_L, C_CUR_R, C_PARENT, C_SMALL, C_LARGE, C_COUNT };

struct TreeOut {
  int *feature, *split_bin;
  uint8_t* default_left;
  int *left, *right;
  double* value;
  double *gain, *cover;  // (nullable) node statistics: the split's gain (0.0 at a leaf), the node's hessian sum
};

struct Nodes {
  int *begin, *end, *side, *depth, *slot, *state;
  long long *qg, *qh;
  MifxGbSplit* cand;
  double *lo, *hi;  // monotone_constraints: the node's weight interval (null in an unconstrained tree)
  uint64_t* sset;   // node sets (gbdt_nodeset.h): the node's path set, words = ceil(f / 64) per node (null without)
  uint8_t* nmask;   // node sets: the node's mask row [f], made by k_nodeset before the node's histogram and search
};

struct Ws {
  long long *qg, *qh;
  int* perm[2];
  unsigned* amax;
  int *exps, *nsamp, *ctrl;
  Nodes nd;
  MifxGbSplit* fcand;  // [2, f] the per-feature candidates of the expansion's two children
  long long *hg, *hh;  // the pool
  int* hc;
  size_t bytes;
  Quant quant() const { return Quant{qg, qh, perm[0], amax, exps, nsamp, nd.qg, nd.qh, nd.end}; }
};

Ws carve(void* base, long n, int f, int max_leaves, int hsize, bool mono = false, bool nodeset = false) {
  Carver c{static_cast<char*>(base)};
  const size_t cap = 2 * (size_t)max_leaves - 1, pool = (size_t)max_leaves * hsize;
  Ws w;
  w.qg = c.take<long long>(n);
  w.qh = c.take<long long>(n);
  w.perm[0] = c.take<int>(n);
  w.perm[1] = c.take<int>(n);
  w.amax = c.take<unsigned>(2);
  w.exps = c.take<int>(2);
  w.nsamp = c.take<int>(2);
  w.ctrl = c.take<int>(C_COUNT);
  w.nd.begin = c.take<int>(cap);
  w.nd.end = c.take<int>(cap);
  w.nd.side = c.take<int>(cap);
  w.nd.depth = c.take<int>(cap);
  w.nd.slot = c.take<int>(cap);
  w.nd.state = c.take<int>(cap);
  w.nd.qg = c.take<long long>(cap);
  w.nd.qh = c.take<long long>(cap);
  w.nd.cand = c.take<MifxGbSplit>(cap);
  w.fcand = c.take<MifxGbSplit>(2 * (size_t)f);
  w.hg = c.take<long long>(pool);
  w.hh = c.take<long long>(pool);
  w.hc = c.take<int>(pool);
  w.nd.lo = mono ? c.take<double>(cap) : nullptr;  // after everything the unconstrained grower lays out
  w.nd.hi = mono ? c.take<double>(cap) : nullptr;
  w.nd.sset = nodeset ? c.take<uint64_t>(cap * mifx_ns_words(f)) : nullptr;
  w.nd.nmask = nodeset ? c.take<uint8_t>(cap * f) : nullptr;
  w.bytes = c.used;
  return w;
}

__global__ void k_init(Ws w) {
  if (threadIdx.x < 2) w.amax[threadIdx.x] = 0u, w.nsamp[threadIdx.x] = 0;
  if (threadIdx.x == 2) w.nd.qg[0] = 0, w.nd.qh[0] = 0;
  if (threadIdx.x < C_COUNT) w.ctrl[threadIdx.x] = 0;
}

// node k enters the tree as a leaf; a later split of it overwrites the entry
__device__ void leaf_entry(const Ws& w, const TreeOut& t, int k, const MifxGbParams& prm) {
  const bool empty = w.nd.end[k] <= w.nd.begin[k];  // the root of an empty sample only: +0.0, no division
  t.feature[k] = -1;
  t.split_bin[k] = -1;
  t.default_left[k] = 0;
  t.left[k] = -1;
  t.right[k] = -1;
  if (w.nd.lo)  // constrained: eta times the weight clamped into the node's interval
    t.value[k] = empty ? 0.0 : mifx_gb_mono_leaf_value(w.nd.qg[k], w.nd.qh[k], w.exps[0], w.exps[1], prm, w.nd.lo[k],
                                                       w.nd.hi[k]);
  else
    t.value[k] = empty ? 0.0 : mifx_gb_leaf_value(w.nd.qg[k], w.nd.qh[k], w.exps[0], w.exps[1], prm);
  if (t.gain) {
    t.gain[k] = 0.0;
    t.cover[k] = mifx_gb_dequant(w.nd.qh[k], w.exps[1]);
  }
}

__device__ void zero_slot(const Ws& w, int slot, int hsize) {
  const size_t o = (size_t)slot * hsize;
  for (int i = threadIdx.x; i < hsize; i += kThreads) {
    w.hg[o + i] = 0;
    w.hh[o + i] = 0;
    w.hc[o + i] = 0;
  }
}

// after the quantise stage (which left the root's sums and its row count in the table): node 0
__global__ __launch_bounds__(kThreads) void k_root(Ws w, TreeOut t, MifxGbParams prm, int max_leaves, int hsize,
                                                   int words) {
  const bool grow = w.nd.end[0] >= 2 && max_leaves >= 2;  // (read before thread 0 writes anything but the entry)
  if (w.nd.sset)  // the root's path set is empty
    for (int i = threadIdx.x; i < words; i += kThreads) w.nd.sset[i] = 0;
  if (threadIdx.x == 0) {
    w.nd.begin[0] = 0;
    w.nd.side[0] = 0;
    w.nd.depth[0] = 0;
    w.nd.slot[0] = 0;
    w.nd.state[0] = grow ? PENDING : CLOSED;
    w.nd.cand[0] = mifx_gb_no_split();
    if (w.nd.lo) w.nd.lo[0] = -INFINITY, w.nd.hi[0] = INFINITY;
    leaf_entry(w, t, 0, prm);
    w.ctrl[C_DONE] = !grow;
    w.ctrl[C_NODES] = 1;
    w.ctrl[C_LEAVES] = 1;
    w.ctrl[C_SLOTS] = 1;
    w.ctrl[C_PARENT] = -1;
    w.ctrl[C_SMALL] = grow ? 0 : -1;
    w.ctrl[C_LARGE] = -1;
  }
  if (grow) zero_slot(w, 0, hsize);
}

// mono (nullable): the constraint vector; the children then inherit their intervals here, before their leaf entries.
// With node sets both children's path sets are the parent's with the split feature's bit set (words per node).
__global__ __launch_bounds__(kThreads) void k_pick(Ws w, TreeOut t, MifxGbParams prm, int max_depth, int max_leaves,
                                                   int hsize, const int* mono, int words) {
  __shared__ double s_gain[kWaves];
  __shared__ int s_id[kWaves], s_fresh;
  int* ctrl = w.ctrl;
  const int nn = ctrl[C_NODES], leaves = ctrl[C_LEAVES];
  if (ctrl[C_DONE]) {  // uniform: the tree is finished, the expansion's other kernels find nothing to do
    if (threadIdx.x == 0) ctrl[C_PARENT] = ctrl[C_SMALL] = ctrl[C_LARGE] = -1;
    return;
  }
  double bg = 0.0;
  int bid = -1;  // an open node's gain is > 1e-6, so -1 loses against any
  for (int k = threadIdx.x; k < nn; k += kThreads)  // ascending ids per thread: strict > keeps the lowest
    if (w.nd.state[k] == OPEN && (bid < 0 || w.nd.cand[k].gain > bg)) bg = w.nd.cand[k].gain, bid = k;
  for (int o = 32; o; o >>= 1) {
    const double og = __shfl_xor(bg, o);
    const int oi = __shfl_xor(bid, o);
    if (oi >= 0 && (bid < 0 || og > bg || (og == bg && oi < bid))) bg = og, bid = oi;
  }
  if ((threadIdx.x & 63) == 0) s_gain[threadIdx.x >> 6] = bg, s_id[threadIdx.x >> 6] = bid;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < kWaves; ++v)
      if (s_id[v] >= 0 && (bid < 0 || s_gain[v] > bg || (s_gain[v] == bg && s_id[v] < bid))) bg = s_gain[v], bid = s_id[v];
    s_fresh = -1;
    if (bid < 0 || leaves >= max_leaves || nn + 2 > 2 * max_leaves - 1 || ctrl[C_SLOTS] >= max_leaves) {
      ctrl[C_DONE] = 1;
      ctrl[C_PARENT] = ctrl[C_SMALL] = ctrl[C_LARGE] = -1;
    } else {
      const int p = bid, li = nn, ri = nn + 1, d = w.nd.depth[p] + 1;
      const MifxGbSplit c = w.nd.cand[p];
      const int b = w.nd.begin[p], e = w.nd.end[p], mid = min(e, b + max(c.cl, 0));
      // can a child ever be split: not at the depth limit, and not when this split reaches the budget
      const bool more = (max_depth == 0 || d < max_depth) && leaves + 1 < max_leaves;
      const int small = mid - b <= e - mid ? li : ri, large = li + ri - small;
      w.nd.state[p] = SPLIT;
      t.feature[p] = c.feature;
      t.split_bin[p] = c.bin;
      t.default_left[p] = (uint8_t)c.default_left;
      t.left[p] = li;
      t.right[p] = ri;
      t.value[p] = 0.0;
      if (t.gain) t.gain[p] = c.gain;
      double bd[4];
      if (mono)
        mifx_gb_mono_children_q(c, w.nd.qg[p], w.nd.qh[p], w.exps[0], w.exps[1], prm, mono[c.feature], w.nd.lo[p],
                                w.nd.hi[p], bd);
      for (int s = 0; s < 2; ++s) {
        const int k = li + s;
        if (mono) w.nd.lo[k] = bd[2 * s], w.nd.hi[k] = bd[2 * s + 1];
        if (w.nd.sset)
          for (int i = 0; i < words; ++i)
            w.nd.sset[(size_t)k * words + i] =
                w.nd.sset[(size_t)p * words + i] | (i == c.feature >> 6 ? (uint64_t)1 << (c.feature & 63) : 0);
        w.nd.begin[k] = s ? mid : b;
        w.nd.end[k] = s ? e : mid;
        w.nd.side[k] = 1 - w.nd.side[p];
        w.nd.depth[k] = d;
        w.nd.qg[k] = s ? w.nd.qg[p] - c.gl : c.gl;
        w.nd.qh[k] = s ? w.nd.qh[p] - c.hl : c.hl;
        w.nd.state[k] = more ? PENDING : CLOSED;
        w.nd.cand[k] = mifx_gb_no_split();
        leaf_entry(w, t, k, prm);
      }
      if (more) {
        s_fresh = ctrl[C_SLOTS];
        w.nd.slot[small] = s_fresh;
        w.nd.slot[large] = w.nd.slot[p];
        ctrl[C_SLOTS] = s_fresh + 1;
      }
      ctrl[C_NODES] = nn + 2;
      ctrl[C_LEAVES] = leaves + 1;
      ctrl[C_DEPTH] = max(ctrl[C_DEPTH], d);
      ctrl[C_CUR_L] = ctrl[C_CUR_R] = 0;
      ctrl[C_PARENT] = p;
      ctrl[C_SMALL] = more ? small : -1;
      ctrl[C_LARGE] = more ? large : -1;
    }
  }
  __syncthreads();
  if (s_fresh >= 0) zero_slot(w, s_fresh, hsize);
}

__global__ __launch_bounds__(kThreads) void k_part(Ws w, TreeOut t, const uint16_t* bins, const int* nbins, long n,
                                                   int f) {
  const int p = w.ctrl[C_PARENT];
  if (p < 0) return;
  const int lane = threadIdx.x & 63;
  const long b = w.nd.begin[p], e = w.nd.end[p], mid = w.nd.end[t.left[p]];
  const int* in = w.perm[w.nd.side[p]];
  int* out = w.perm[1 - w.nd.side[p]];
  const int feat = t.feature[p], sb = t.split_bin[p];
  const bool dl = t.default_left[p] != 0;
  if (feat < 0 || feat >= f) return;
  const int nb = min(nbins[feat], kMaxBins);
  const long wave = (blockIdx.x * (long)kThreads + threadIdx.x) >> 6, waves = (long)gridDim.x * kWaves;
  for (long i0 = b + wave * 64; i0 < e; i0 += waves * 64) {  // i0 is uniform over the wave: every lane reaches the ballots
    const long i = i0 + lane;
    int r = i < e ? in[i] : -1;
    const bool ok = (unsigned)r < (unsigned long)n;
    bool goleft = false;
    if (ok) {
      const int bv = bins[(size_t)r * f + feat];
      goleft = bv < nb ? bv <= sb : dl;
    }
    const u64 ml = __ballot(ok && goleft), mr = __ballot(ok && !goleft);
    int bl = 0, br = 0;
    if (lane == 0) {
      if (ml) bl = atomicAdd(&w.ctrl[C_CUR_L], __popcll(ml));
      if (mr) br = atomicAdd(&w.ctrl[C_CUR_R], __popcll(mr));
    }
    bl = __shfl(bl, 0);
    br = __shfl(br, 0);
    if (!ok) continue;
    const u64 below = ((u64)1 << lane) - 1;
    const long dst = goleft ? b + bl + __popcll(ml & below) : mid + br + __popcll(mr & below);
    if (dst < (goleft ? mid : e)) out[dst] = r;
  }
}

// kPerNode (node sets): the masks are the nodes' own rows (w.nd.nmask), not the tree's one row
template <bool kPerNode>
__global__ __launch_bounds__(kThreads) void k_hist(Ws w, const uint16_t* bins, long n, int f, const int* nbins,
                                                   const int* hoff, int hsize, int rows_per_wg, int ft,
                                                   const uint8_t* mask) {
  extern __shared__ long long smem[];
  long long* sg = smem;
  long long* sh = smem + ft * kSlots;
  int* sc = reinterpret_cast<int*>(smem + 2 * ft * kSlots);
  const int k = w.ctrl[C_SMALL];
  if (k < 0) return;
  const long b = w.nd.begin[k], e = w.nd.end[k];
  const long first = b + (long)blockIdx.x * rows_per_wg, stride = (long)gridDim.x * rows_per_wg;
  if (first >= e) return;  // uniform over the workgroup
  const int j0 = blockIdx.y * ft, nf = min(ft, f - j0), tid = threadIdx.x;
  if (kPerNode) {  // the tile holds nothing that the node's histogram keeps (its larger sibling keeps the same set)
    bool live = false;
    for (int jj = 0; jj < nf; ++jj) live |= (w.nd.nmask[(size_t)k * f + j0 + jj] & MIFX_NS_HIST) != 0;
    if (!live) return;
  } else if (mask) {  // (nullable) the tree's feature mask: a tile without a live feature is never searched
    bool live = false;
    for (int jj = 0; jj < nf; ++jj) live |= mask[j0 + jj] != 0;
    if (!live) return;
  }
  const int* perm = w.perm[w.nd.side[k]];
  for (int i = tid; i < nf * kSlots; i += kThreads) {
    sg[i] = 0;
    sh[i] = 0;
    sc[i] = 0;
  }
  __syncthreads();
  for (long c0 = first; c0 < e; c0 += stride) {
    const long items = (min(e, c0 + rows_per_wg) - c0) * nf;
    for (long it = tid; it < items; it += kThreads) {
      const int jj = (int)(it % nf);
      const int r = perm[c0 + it / nf];
      if ((unsigned)r >= (unsigned long)n) continue;
      const int nb = min(nbins[j0 + jj], kMaxBins);
      const int bv = bins[(size_t)r * f + j0 + jj];
      const int s = jj * kSlots + (bv < nb ? bv : nb);
      add64(&sg[s], w.qg[r]);
      add64(&sh[s], w.qh[r]);
      atomicAdd(&sc[s], 1);
    }
  }
  __syncthreads();
  const size_t slot = (size_t)w.nd.slot[k] * hsize;
  for (int i = tid; i < nf * kSlots; i += kThreads) {
    const int jj = i / kSlots, sl = i % kSlots;
    if (sc[i] != 0 && sl <= min(nbins[j0 + jj], kMaxBins)) {
      const size_t o = slot + hoff[j0 + jj] + sl;
      add64(&w.hg[o], sg[i]);
      add64(&w.hh[o], sh[i]);
      atomicAdd(&w.hc[o], sc[i]);
    }
  }
}

// workgroup 0: the smaller child (or the root), workgroup 1: the larger one
template <bool kPerNode>
__global__ __launch_bounds__(kSplitWaves * 64) void k_split(Ws w, int f, const int* nbins, const int* hoff, int hsize,
                                                            MifxGbParams prm, const uint8_t* mask) {
  __shared__ long long s_g[kSplitWaves][kSlots], s_h[kSplitWaves][kSlots];
  __shared__ int s_c[kSplitWaves][kSlots];
  const int small = w.ctrl[C_SMALL], k = blockIdx.x == 0 ? small : w.ctrl[C_LARGE];
  if (k < 0) return;  // uniform over the workgroup
  const bool subtract = blockIdx.x == 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool scan = w.nd.end[k] - w.nd.begin[k] >= 2;  // fewer rows: a leaf whatever its histogram
  const int eg = w.exps[0], eh = w.exps[1];
  const long long Qg = w.nd.qg[k], Qh = w.nd.qh[k];
  const double parent = mifx_gb_parent_score(Qg, Qh, eg, eh, prm);
  const size_t mine = (size_t)w.nd.slot[k] * hsize, other = (size_t)w.nd.slot[small] * hsize;
  MifxGbSplit* fc = w.fcand + (size_t)blockIdx.x * f;
  long long* g0 = s_g[wave];
  long long* h0 = s_h[wave];
  int* c0 = s_c[wave];
  for (int jb = 0; jb < f; jb += kSplitWaves) {  // every thread takes every trip: the barriers are uniform
    const int j = jb + wave;
    // uniform over the wave. With node sets `live` is "the histogram holds the feature" (staged, and subtracted for the
    // larger child, whose descendants may draw it) and `search` "this node may split on it"; without, they are one.
    const int nm = kPerNode && j < f ? w.nd.nmask[(size_t)k * f + j] : MIFX_NS_HIST | MIFX_NS_SPLIT;
    const bool live = scan && j < f && (kPerNode ? (nm & MIFX_NS_HIST) != 0 : !mask || mask[j]);
    const bool search = live && (nm & MIFX_NS_SPLIT);
    const int nb = live ? min(nbins[j], kMaxBins) : 0;
    if (live)
      for (int s = lane; s <= nb; s += 64) {
        const size_t o = mine + hoff[j] + s;
        long long a = w.hg[o], b = w.hh[o];
        int c = w.hc[o];
        if (subtract) {  // this slot still holds the parent: parent - smaller, kept for the child's own descendants
          const size_t q = other + hoff[j] + s;
          w.hg[o] = a -= w.hg[q];
          w.hh[o] = b -= w.hh[q];
          w.hc[o] = c -= w.hc[q];
        }
        g0[s] = a;
        h0[s] = b;
        c0[s] = c;
      }
    __syncthreads();
    if (search) {
      MifxGbSplit bs = mifx_gb_no_split();
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
      if (lane == 0) fc[j] = bs;
    } else if (j < f && lane == 0) {
      fc[j] = mifx_gb_no_split();
    }
    __syncthreads();  // the staging rows are rewritten by the next trip; fc is complete after the last one
  }
  if (threadIdx.x != 0) return;
  MifxGbSplit best = mifx_gb_no_split();
  for (int j = 0; j < f; ++j)
    if (mifx_gb_feature_wins(fc[j], best)) best = fc[j];
  w.nd.cand[k] = best;
  w.nd.state[k] = mifx_gb_is_leaf(best) ? CLOSED : OPEN;
}

// k_split under monotone_constraints (the rule is gbdt_split.h's, the wave search gbdt_wave.h's): the same two
// workgroups, staging and in-place subtraction; the child's interval comes from the node table (k_pick wrote it), once
// per workgroup, and every wave searches its feature with the feature's direction.
template <bool kPerNode>
__global__ __launch_bounds__(kSplitWaves * 64) void k_split_mono(Ws w, int f, const int* nbins, const int* hoff,
                                                                 int hsize, MifxGbParams prm, const uint8_t* mask,
                                                                 const int* mono) {
  __shared__ long long s_g[kSplitWaves][kSlots], s_h[kSplitWaves][kSlots];
  __shared__ int s_c[kSplitWaves][kSlots];
  const int small = w.ctrl[C_SMALL], k = blockIdx.x == 0 ? small : w.ctrl[C_LARGE];
  if (k < 0) return;  // uniform over the workgroup
  const bool subtract = blockIdx.x == 1;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool scan = w.nd.end[k] - w.nd.begin[k] >= 2;  // fewer rows: a leaf whatever its histogram
  const int eg = w.exps[0], eh = w.exps[1];
  const long long Qg = w.nd.qg[k], Qh = w.nd.qh[k];
  const double lo = w.nd.lo[k], hi = w.nd.hi[k];
  const size_t mine = (size_t)w.nd.slot[k] * hsize, other = (size_t)w.nd.slot[small] * hsize;
  MifxGbSplit* fc = w.fcand + (size_t)blockIdx.x * f;
  for (int jb = 0; jb < f; jb += kSplitWaves) {  // every thread takes every trip: the barriers are uniform
    const int j = jb + wave;
    // uniform over the wave. With node sets `live` is "the histogram holds the feature" (staged, and subtracted for the
    // larger child, whose descendants may draw it) and `search` "this node may split on it"; without, they are one.
    const int nm = kPerNode && j < f ? w.nd.nmask[(size_t)k * f + j] : MIFX_NS_HIST | MIFX_NS_SPLIT;
    const bool live = scan && j < f && (kPerNode ? (nm & MIFX_NS_HIST) != 0 : !mask || mask[j]);
    const bool search = live && (nm & MIFX_NS_SPLIT);
    const int nb = live ? min(nbins[j], kMaxBins) : 0;
    if (live)
      for (int s = lane; s <= nb; s += 64) {
        const size_t o = mine + hoff[j] + s;
        long long a = w.hg[o], b = w.hh[o];
        int c = w.hc[o];
        if (subtract) {  // this slot still holds the parent: parent - smaller, kept for the child's own descendants
          const size_t q = other + hoff[j] + s;
          w.hg[o] = a -= w.hg[q];
          w.hh[o] = b -= w.hh[q];
          w.hc[o] = c -= w.hc[q];
        }
        s_g[wave][s] = a;
        s_h[wave][s] = b;
        s_c[wave][s] = c;
      }
    __syncthreads();
    if (search) {
      const MifxGbSplit bs = wave_search_mono(s_g[wave], s_h[wave], s_c[wave], nb, lane, Qg, Qh, eg, eh, j, prm, mono[j],
                                              lo, hi);
      if (lane == 0) fc[j] = bs;
    } else if (j < f && lane == 0) {
      fc[j] = mifx_gb_no_split();
    }
    __syncthreads();  // the staging rows are rewritten by the next trip; fc is complete after the last one
  }
  if (threadIdx.x != 0) return;
  MifxGbSplit best = mifx_gb_no_split();
  for (int j = 0; j < f; ++j)
    if (mifx_gb_feature_wins(fc[j], best)) best = fc[j];
  w.nd.cand[k] = best;
  w.nd.state[k] = mifx_gb_is_leaf(best) ? CLOSED : OPEN;
}

// ---- node sets (interaction_constraints, colsample_bynode; the rule and the wave's work are gbdt_nodeset.h's): the
// mask rows of the nodes whose histograms and candidates come next -- the root (one wave), or the expansion's two children,
// a wave each. Nothing to do once the tree is finished or when the children were closed by k_pick. tree_set (nullable):
// the tree's colsample_bytree set, every node's level set.
__global__ __launch_bounds__(128) void k_nodeset(Ws w, MifxNsSpec ns, int f, const uint8_t* tree_set, int root) {
  extern __shared__ uint64_t ns_hash[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w.ctrl[C_SMALL] < 0 || (root && wave != 0)) return;  // uniform over the wave
  const int k = root ? 0 : w.ctrl[C_NODES] - 2 + wave;
  nodeset_wave(ns, f, k, w.nd.sset + (size_t)k * mifx_ns_words(f), tree_set, w.nd.nmask + (size_t)k * f,
               ns_hash + (size_t)wave * f, threadIdx.x & 63);
}

// every row of a leaf: leaf_of_row and margin += value. y strides over the nodes, x over a node's rows.
__global__ __launch_bounds__(kThreads) void k_finish(Ws w, TreeOut t, long n, int* leaf_of_row, double* margin,
                                                     int* node_count) {
  const int nn = w.ctrl[C_NODES];
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    node_count[0] = nn;
    node_count[1] = w.ctrl[C_DEPTH];
  }
  for (int k = blockIdx.y; k < nn; k += gridDim.y) {
    if (w.nd.state[k] == SPLIT) continue;
    const int* perm = w.perm[w.nd.side[k]];
    const long e = w.nd.end[k];
    const double v = t.value[k];
    for (long p = w.nd.begin[k] + blockIdx.x * (long)kThreads + threadIdx.x; p < e; p += (long)gridDim.x * kThreads) {
      const int r = perm[p];
      if ((unsigned)r >= (unsigned long)n) continue;
      leaf_of_row[r] = k;
      if (margin) margin[r] += v;
    }
  }
}

// margin[i] += the tree's output for row i of a binned matrix: bin <= split_bin  <=>  x < cut. node_count: the tree's
// node count and its depth (k_finish), which bounds the walk. rest (nullable): leaf_of_row of a sampled tree; only its
// -1 rows, the rows outside the sample, are walked.
__global__ void k_walk(const uint16_t* bins, long m, int f, const int* nbins, TreeOut t, const int* node_count,
                       double* margin, const int* rest) {
  const long i = blockIdx.x * (long)kThreads + threadIdx.x;
  if (i >= m) return;
  if (rest && rest[i] >= 0) return;
  const int cap = node_count[0], depth = node_count[1];
  int k = 0;
  for (int step = 0; step < depth; ++step) {
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

// the grower behind mifx_gbdt_lg_grow and mifx_gbdt_lg_grow_mono; mono (device, null = unconstrained): [f] directions,
// the workspace then has the constrained layout
int grow_tree(const uint16_t* bins, long n, int f, const int* nbins, const int* hoff, int hsize, const float* g,
              const float* h, int max_depth, int max_leaves, double min_child_weight, double lambda, double gamma,
              double eta, void* ws, long long ws_bytes, int* feature, int* split_bin, uint8_t* default_left, int* left,
              int* right, double* value, int* node_count, int* leaf_of_row, double* margin, int rows_per_wg,
              int feat_tile, int grid_x, unsigned long long seed, unsigned long long round, unsigned long long thr,
              const uint8_t* feature_mask, double* node_gain, double* node_cover, const int* mono,
              const MifxNsSpec* ns, hipStream_t stream);

}  // namespace

extern "C" {

int mifx_gbdt_lg_max_leaves() { return kMaxLeaves; }
int mifx_gbdt_lg_max_depth() { return kMaxDepth; }
int mifx_gbdt_lg_max_feat_tile() { return kMaxFeatTile; }

// Bytes of workspace for mifx_gbdt_lg_grow; hsize = sum over features of nbins + 1; -1 on arguments out of range.
// With every array rounded up to 256 bytes:
//   24 n                        the quantised rows (int64 g, h) and the two permutation arrays
// + (2 max_leaves - 1) * 80     the node table (six ints, two int64, one 40-byte candidate per node)
// + 2 f * 40                    the per-feature candidates of one expansion
// + max_leaves * hsize * 20     the histogram pool (int64 g, int64 h, int32 rows per entry)
// + four small arrays.
long long mifx_gbdt_lg_ws_bytes(long n, int f, int max_leaves, int hsize) {
  if (n < 1 || n >= (1L << 31) || f < 1 || max_leaves < 2 || max_leaves > kMaxLeaves || hsize < 2 * f ||
      hsize > f * kSlots)
    return -1;
  return (long long)carve(nullptr, n, f, max_leaves, hsize).bytes;
}

// the same for mifx_gbdt_lg_grow_mono: (2 max_leaves - 1) * 16 more, the node table's two doubles per node
long long mifx_gbdt_lg_ws_bytes_mono(long n, int f, int max_leaves, int hsize) {
  if (mifx_gbdt_lg_ws_bytes(n, f, max_leaves, hsize) < 0) return -1;
  return (long long)carve(nullptr, n, f, max_leaves, hsize, true).bytes;
}

// Grow one tree leaf-wise. bins: row-major [n, f]; nbins [f] and hoff [f] (exclusive prefix of nbins + 1) on the
// device, the tree arrays (2 * max_leaves - 1 entries each) too. node_count [2] (device) receives the node count and
// the tree's depth. leaf_of_row [n]; margin (nullable) [n] receives margin[row] += the tree's output, for every row.
// max_depth: 0 = no limit, else a node at that depth is a leaf (<= mifx_gbdt_lg_max_depth()).
// rows_per_wg / feat_tile / grid_x: launch geometry (rows per chunk and features per workgroup of k_hist, workgroups
// along the rows of k_hist and k_part); the tree does not depend on it.
// Sampling: thr < 2^32 grows the tree on the rows that mifx_gs_keep_row(key(seed, round, rows), i, thr) keeps, as if
// the table held only them (leaf_of_row = -1 for the others, whose margins come from a walk of the finished tree).
// feature_mask (device, nullable): [f] uint8, the features the tree may split on.
// node_gain / node_cover (device, nullable, both or neither): as in mifx_gbdt_gpu_grow_stats.
int mifx_gbdt_lg_grow(const uint16_t* bins, long n, int f, const int* nbins, const int* hoff, int hsize, const float* g,
                      const float* h, int max_depth, int max_leaves, double min_child_weight, double lambda,
                      double gamma, double eta, void* ws, long long ws_bytes, int* feature, int* split_bin,
                      uint8_t* default_left, int* left, int* right, double* value, int* node_count, int* leaf_of_row,
                      double* margin, int rows_per_wg, int feat_tile, int grid_x, unsigned long long seed,
                      unsigned long long round, unsigned long long thr, const uint8_t* feature_mask, double* node_gain,
                      double* node_cover, hipStream_t stream) {
  return grow_tree(bins, n, f, nbins, hoff, hsize, g, h, max_depth, max_leaves, min_child_weight, lambda, gamma, eta, ws,
                   ws_bytes, feature, split_bin, default_left, left, right, value, node_count, leaf_of_row, margin,
                   rows_per_wg, feat_tile, grid_x, seed, round, thr, feature_mask, node_gain, node_cover, nullptr,
                   nullptr, stream);
}

// mifx_gbdt_lg_grow under monotone_constraints: mono (device) [f] ints in {-1, 0, +1}, the rule of gbdt_split.h; ws
// holds mifx_gbdt_lg_ws_bytes_mono bytes. The host twin is mifx_gbdt_grow_fixed_lossguide_mono. Every node's interval
// is in the node table: k_root and k_pick write it and clamp the leaf entries, k_split_mono searches under it.
int mifx_gbdt_lg_grow_mono(const uint16_t* bins, long n, int f, const int* nbins, const int* hoff, int hsize,
                           const float* g, const float* h, int max_depth, int max_leaves, double min_child_weight,
                           double lambda, double gamma, double eta, void* ws, long long ws_bytes, int* feature,
                           int* split_bin, uint8_t* default_left, int* left, int* right, double* value, int* node_count,
                           int* leaf_of_row, double* margin, int rows_per_wg, int feat_tile, int grid_x,
                           unsigned long long seed, unsigned long long round, unsigned long long thr,
                           const uint8_t* feature_mask, double* node_gain, double* node_cover, const int* mono,
                           hipStream_t stream) {
  if (!mono) return -1;
  return grow_tree(bins, n, f, nbins, hoff, hsize, g, h, max_depth, max_leaves, min_child_weight, lambda, gamma, eta, ws,
                   ws_bytes, feature, split_bin, default_left, left, right, value, node_count, leaf_of_row, margin,
                   rows_per_wg, feat_tile, grid_x, seed, round, thr, feature_mask, node_gain, node_cover, mono, nullptr,
                   stream);
}

// the workspace of mifx_gbdt_lg_grow_nodeset: the (mono: constrained) layout, then per node its path set
// (ceil(f / 64) * 8 bytes) and its mask row (f bytes)
long long mifx_gbdt_lg_ws_bytes_nodeset(long n, int f, int max_leaves, int hsize, int mono) {
  if (mifx_gbdt_lg_ws_bytes(n, f, max_leaves, hsize) < 0) return -1;
  return (long long)carve(nullptr, n, f, max_leaves, hsize, mono != 0, true).bytes;
}

// mifx_gbdt_lg_grow / mifx_gbdt_lg_grow_mono (mono nullable) with per-node feature sets, the rule of gbdt_nodeset.h:
// groups (device, nullable) [n_groups, ceil(f / 64)] uint64 bitsets, bynode the colsample_bynode rate (1.0: no draw;
// < 1 needs f <= 2048), keyed by (seed, round, node id). k_pick hands the children their path sets, k_nodeset makes
// their mask rows (feature_mask, nullable, is every node's level set); k_hist skips the tiles outside the smaller
// child's histogram set and the split kernels search the split set only. ws holds mifx_gbdt_lg_ws_bytes_nodeset bytes.
// The host twin is mifx_gbdt_grow_lossguide_nodeset with fixed = 1.
int mifx_gbdt_lg_grow_nodeset(const uint16_t* bins, long n, int f, const int* nbins, const int* hoff, int hsize,
                              const float* g, const float* h, int max_depth, int max_leaves, double min_child_weight,
                              double lambda, double gamma, double eta, void* ws, long long ws_bytes, int* feature,
                              int* split_bin, uint8_t* default_left, int* left, int* right, double* value,
                              int* node_count, int* leaf_of_row, double* margin, int rows_per_wg, int feat_tile,
                              int grid_x, unsigned long long seed, unsigned long long round, unsigned long long thr,
                              const uint8_t* feature_mask, double* node_gain, double* node_cover, const int* mono,
                              const uint64_t* groups, int n_groups, double bynode, hipStream_t stream) {
  if (!(bynode > 0.0 && bynode <= 1.0) || (groups && n_groups < 1) || (bynode < 1.0 && f > kNsMaxDrawFeat)) return -1;
  const MifxNsSpec ns{groups, groups ? n_groups : 0, bynode, seed, round};
  return grow_tree(bins, n, f, nbins, hoff, hsize, g, h, max_depth, max_leaves, min_child_weight, lambda, gamma, eta, ws,
                   ws_bytes, feature, split_bin, default_left, left, right, value, node_count, leaf_of_row, margin,
                   rows_per_wg, feat_tile, grid_x, seed, round, thr, feature_mask, node_gain, node_cover, mono, &ns,
                   stream);
}

}  // extern "C"

namespace {

int grow_tree(const uint16_t* bins, long n, int f, const int* nbins, const int* hoff, int hsize, const float* g,
              const float* h, int max_depth, int max_leaves, double min_child_weight, double lambda, double gamma,
              double eta, void* ws, long long ws_bytes, int* feature, int* split_bin, uint8_t* default_left, int* left,
              int* right, double* value, int* node_count, int* leaf_of_row, double* margin, int rows_per_wg,
              int feat_tile, int grid_x, unsigned long long seed, unsigned long long round, unsigned long long thr,
              const uint8_t* feature_mask, double* node_gain, double* node_cover, const int* mono,
              const MifxNsSpec* ns, hipStream_t stream) {
  if ((node_gain == nullptr) != (node_cover == nullptr)) return -1;
  const long long need = ns     ? mifx_gbdt_lg_ws_bytes_nodeset(n, f, max_leaves, hsize, mono != nullptr)
                         : mono ? mifx_gbdt_lg_ws_bytes_mono(n, f, max_leaves, hsize)
                                : mifx_gbdt_lg_ws_bytes(n, f, max_leaves, hsize);
  if (need < 0 || ws_bytes < need || max_depth < 0 || max_depth > kMaxDepth) return -1;
  if (rows_per_wg < 1 || feat_tile < 1 || feat_tile > kMaxFeatTile || grid_x < 1 || grid_x > 65535) return -1;
  Ws w = carve(ws, n, f, max_leaves, hsize, mono != nullptr, ns != nullptr);
  const int words = mifx_ns_words(f);
  const MifxGbParams prm{lambda, gamma, min_child_weight, eta};
  const TreeOut t{feature, split_bin, default_left, left, right, value, node_gain, node_cover};
  const dim3 hist_grid((unsigned)std::min<long>((n + rows_per_wg - 1) / rows_per_wg, grid_x),
                       (unsigned)((f + feat_tile - 1) / feat_tile));
  const size_t lds = (size_t)feat_tile * kSlots * (2 * sizeof(long long) + sizeof(int));
  const unsigned part_grid = (unsigned)grid_for(n, grid_x);
  k_init<<<1, 64, 0, stream>>>(w);
  launch_quant(g, h, n, seed, round, thr, w.quant(), leaf_of_row, stream);
  k_root<<<1, kThreads, 0, stream>>>(w, t, prm, max_leaves, hsize, words);
  for (int x = 0; x < max_leaves; ++x) {  // x = 0: the root's candidate; then max_leaves - 1 expansions
    if (x > 0) {
      k_pick<<<1, kThreads, 0, stream>>>(w, t, prm, max_depth, max_leaves, hsize, mono, words);
      k_part<<<part_grid, kThreads, 0, stream>>>(w, t, bins, nbins, n, f);
    }
    if (x + 1 < max_leaves) {  // the last expansion's children are never split
      if (ns) k_nodeset<<<1, 128, ns_lds_bytes(*ns, f, 2), stream>>>(w, *ns, f, feature_mask, x == 0);
      (ns ? k_hist<true> : k_hist<false>)<<<hist_grid, kThreads, lds, stream>>>(w, bins, n, f, nbins, hoff, hsize,
                                                                                 rows_per_wg, feat_tile, feature_mask);
      if (mono)
        (ns ? k_split_mono<true> : k_split_mono<false>)<<<2, kSplitWaves * 64, 0, stream>>>(w, f, nbins, hoff, hsize,
                                                                                             prm, feature_mask, mono);
      else
        (ns ? k_split<true> : k_split<false>)<<<2, kSplitWaves * 64, 0, stream>>>(w, f, nbins, hoff, hsize, prm,
                                                                                   feature_mask);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  k_finish<<<dim3(128, 8), kThreads, 0, stream>>>(w, t, n, leaf_of_row, margin, node_count);
  if (thr < MIFX_GS_KEEP_ALL && margin)  // the rows that no leaf holds
    k_walk<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, stream>>>(bins, n, f, nbins, t, node_count, margin,
                                                                               leaf_of_row);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// margin[i] += tree(row i) for a binned row-major [m, f] matrix (the eval set's margins); node_count: the [2] that
// mifx_gbdt_lg_grow wrote for this tree
int mifx_gbdt_lg_apply(const uint16_t* bins, long m, int f, const int* nbins, const int* feature, const int* split_bin,
                       const uint8_t* default_left, const int* left, const int* right, const double* value,
                       const int* node_count, double* margin, hipStream_t stream) {
  if (m < 1 || f < 1) return -1;
  const TreeOut t{const_cast<int*>(feature), const_cast<int*>(split_bin), const_cast<uint8_t*>(default_left),
                  const_cast<int*>(left), const_cast<int*>(right), const_cast<double*>(value), nullptr, nullptr};
  k_walk<<<(unsigned)((m + kThreads - 1) / kThreads), kThreads, 0, stream>>>(bins, m, f, nbins, t, node_count, margin,
                                                                             nullptr);
  return (int)hipGetLastError();
}

}  // extern "C"
