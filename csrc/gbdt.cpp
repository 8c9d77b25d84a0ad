// Histogram gradient-boosted trees (host C++): the tree learner behind mifx.gbdt's XGBRegressor / XGBClassifier.
//
// Reference workload: the fairing XGBoost sample (`kubeflow-pipelines/fairing/fairing_xgboost.py:69-87`: 1000
// estimators, learning rate 0.1, early stopping 50 on an eval set) and notebook N12 (CPU scope, the
// Ames housing table is ~1.5k rows x 37 numeric columns -- far below the size where a GPU launch pays). The learner
// is XGBoost's second-order one on quantised features:
//  * binning: per feature, the sorted distinct values give the cut points (value < cut goes left); more than
//    max_bins distinct values are thinned to count quantiles. NaN is "missing" (bin 0xFFFF) and each split learns
//    the direction missing values take (both tried, the better kept), as XGBoost's sparsity-aware split does.
//  * growth: depth-wise to max_depth; a node's histogram of (sum g, sum h) per bin is built for the smaller child
//    only and the larger one is the parent's minus it; the best split maximises
//    G_L^2 / (H_L + lambda) + G_R^2 / (H_R + lambda) - G^2 / (H + lambda) (halved, minus gamma) subject to
//    H_L, H_R >= min_child_weight; leaves take -eta G / (H + lambda).
//  * determinism: ties go to the lowest feature, then the lowest cut; histograms are summed in row order, so a
//    model is bit-reproducible for any thread count (threads split the features, never the rows of one feature).
// Rows of a node are a contiguous range of one permutation array, partitioned in place after each split.
//
// mifx_gbdt_grow_fixed is the same learner on fixed-point (int64) histograms with the split rule of gbdt_split.h:
// the host twin of the device learner in gbdt_gpu.hip (larger tables, device="gpu"), which it reproduces bit for bit.
//
// Leaf-wise growth (the *_lossguide_stats entries): the open leaf with the largest gain is split next until a leaf
// budget is reached; one driver over the double and the fixed-point arithmetic, the latter the host twin of
// csrc/gbdt_lossguide.hip.
//
// Stochastic boosting (the *_ex entries): a tree is grown on a list of sampled rows as if the table held only them,
// and a [max_depth, f] mask names the features each level may split on; the draws themselves are gbdt_sample.h's.
//
// Node statistics (the *_stats entries): every grower can also record each node's gain and cover (hessian sum), which
// feature importances and feature contributions need. mifx_gbdt_paths_build turns a forest with covers into the path
// table of gbdt_shap.h and mifx_gbdt_contribs evaluates path-dependent TreeSHAP from it (the device twin is k_contribs
// in gbdt_prep.hip); mifx_gbdt_interactions gives the interaction values, one conditioned pass per feature over the
// leaves that hold it (the device twin is k_interactions in gbdt_interactions.hip).
//
// Absolute / quantile error: mifx_gbdt_leaf_refresh replaces a finished tree's leaf values by exact weighted quantiles
// of the residuals of each leaf's rows (the rule of gbdt_quantile.h; the device twin is gbdt_quantile.hip).
//
// Ranking: mifx_gbdt_rank_grad is the LambdaMART gradient pair of rank:pairwise / rank:ndcg over contiguous query
// groups (the rule of gbdt_rank.h; the device twin is gbdt_rank.hip).
//
// eval_metric="auc": mifx_gbdt_auc gives the exact integer pair counts of the one-vs-rest AUC per class (the rule of
// gbdt_auc.h; the device twin is gbdt_auc.hip).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "gbdt_auc.h"
#include "gbdt_nodeset.h"
#include "gbdt_quantile.h"
#include "gbdt_rank.h"
#include "gbdt_sample.h"
#include "gbdt_shap.h"
#include "gbdt_split.h"

namespace {

constexpr uint16_t kMissing = 0xFFFF;

struct Hist {
  double g, h;
};

struct Split {
  double gain = 0.0;
  int feature = -1;
  int bin = -1;  // rows with bin <= this go left
  bool default_left = false;
  double gl = 0, hl = 0, gr = 0, hr = 0;
};

struct Node {
  int begin, end, depth, id;
  double g, h;
  std::vector<Hist> hist;  // [features][nbins + 1], the last slot is "missing"
  double lo, hi;           // the weight interval of monotone_constraints (gbdt_split.h)
  std::vector<uint64_t> S;  // the path set of gbdt_nodeset.h (kept only under a node-set spec)
};

template <class F>
void parallel_for(int n, int threads, F&& fn) {
  if (threads <= 1 || n <= 1) {
    for (int i = 0; i < n; ++i) fn(i);
    return;
  }
  threads = std::min(threads, n);
  std::vector<std::thread> pool;
  pool.reserve(threads);
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&, t] {
      for (int i = t; i < n; i += threads) fn(i);
    });
  for (auto& th : pool) th.join();
}

// the *_ex entries' row list: ascending ids inside [0, n)
bool rows_ok(const int* rows, long n_rows, long n) {
  if (!rows) return true;
  if (n_rows < 0 || n_rows > n) return false;
  for (long k = 0; k < n_rows; ++k)
    if (rows[k] < 0 || rows[k] >= n || (k > 0 && rows[k] <= rows[k - 1])) return false;
  return true;
}

// the *_mono entries' directions: one of -1, 0, +1 per feature
bool mono_ok(const int* mono, int f) {
  if (!mono) return false;
  for (int j = 0; j < f; ++j)
    if (mono[j] < -1 || mono[j] > 1) return false;
  return true;
}

// the *_nodeset entries' spec: a rate in (0, 1], groups over [0, f) only (the bits past f clear)
bool nodeset_ok(const MifxNsSpec& ns, int f) {
  if (!(ns.bynode > 0.0 && ns.bynode <= 1.0) || (ns.groups && ns.n_groups < 1)) return false;
  const int words = mifx_ns_words(f);
  for (int g = 0; ns.groups && g < ns.n_groups; ++g)
    if ((f & 63) && ns.groups[(size_t)g * words + words - 1] >> (f & 63)) return false;
  return true;
}

// a child's path set: the parent's and the split feature
std::vector<uint64_t> child_set(const std::vector<uint64_t>& S, int feature) {
  std::vector<uint64_t> c = S;
  c[feature >> 6] |= (uint64_t)1 << (feature & 63);
  return c;
}

}  // namespace

extern "C" {

// ---- the draws of gbdt_sample.h, for the estimators and for the tests that compare them with the numpy twin and
// with the device. keep [n]: 1 for a sampled row; returns their count.
long mifx_gbdt_sample_rows(uint64_t seed, uint64_t round, double subsample, long n, uint8_t* keep) {
  const uint64_t thr = mifx_gs_row_thr(subsample);
  if (thr >= MIFX_GS_KEEP_ALL) {
    std::memset(keep, 1, (size_t)n);
    return n;
  }
  const uint64_t key = mifx_gs_key(seed, round, MIFX_GS_SITE_ROWS);
  long cnt = 0;
  for (long i = 0; i < n; ++i) cnt += keep[i] = mifx_gs_keep_row(key, (uint64_t)i, thr);
  return cnt;
}

// one feature draw at `site` among cand (null: all f); out [f]; returns k
int mifx_gbdt_sample_features(uint64_t seed, uint64_t round, uint64_t site, double rate, const uint8_t* cand, int f,
                              uint8_t* out) {
  return mifx_gs_choose(mifx_gs_key(seed, round, site), rate, cand, f, out);
}

// the [max_depth, f] level mask of a round (and the tree's set [f])
int mifx_gbdt_level_mask(uint64_t seed, uint64_t round, int f, int max_depth, double colsample_bytree,
                         double colsample_bylevel, uint8_t* tree_set, uint8_t* mask) {
  if (f < 1 || max_depth < 0) return -1;
  mifx_gs_level_mask(seed, round, f, max_depth, colsample_bytree, colsample_bylevel, tree_set, mask);
  return 0;
}

// Cut points of one feature column (n values, stride `stride` doubles apart): writes up to max_bins - 1 ascending
// cuts into `cuts` and returns their count.
int mifx_gbdt_cuts(const double* x, long n, long stride, int max_bins, double* cuts) {
  if (max_bins < 2 || max_bins > 65535) return -1;
  std::vector<double> v;
  v.reserve(n);
  for (long i = 0; i < n; ++i) {
    const double a = x[i * stride];
    if (!std::isnan(a)) v.push_back(a);
  }
  if (v.empty()) return 0;
  std::sort(v.begin(), v.end());
  // distinct values with their counts
  std::vector<double> u;
  std::vector<long> cnt;
  for (size_t i = 0; i < v.size(); ++i) {
    if (u.empty() || v[i] != u.back()) {
      u.push_back(v[i]);
      cnt.push_back(1);
    } else {
      ++cnt.back();
    }
  }
  int nc = 0;
  if ((long)u.size() <= max_bins) {
    for (size_t i = 1; i < u.size(); ++i) cuts[nc++] = u[i];  // one bin per distinct value
    return nc;
  }
  // count quantiles: a cut before the distinct value at which the running count crosses k n / max_bins
  const double total = (double)v.size();
  long run = 0;
  int k = 1;
  for (size_t i = 0; i < u.size() && nc < max_bins - 1; ++i) {
    if (i > 0 && (double)run >= k * total / max_bins) {
      cuts[nc++] = u[i];
      while (k * total / max_bins <= (double)run) ++k;
    }
    run += cnt[i];
  }
  return nc;
}

// Bin a row-major [n, f] matrix into a column-major [f, n] uint16 matrix with the per-feature cuts
// (cuts + cut_off[j], ncut[j] of them): bin = number of cuts <= x, NaN -> 0xFFFF.
int mifx_gbdt_bin(const double* X, long n, int f, const double* cuts, const int* cut_off, const int* ncut,
                  uint16_t* bins, int threads) {
  parallel_for(f, n * (long)f > 200000 ? threads : 1, [&](int j) {
    const double* c = cuts + cut_off[j];
    const int m = ncut[j];
    uint16_t* out = bins + (size_t)j * n;
    for (long i = 0; i < n; ++i) {
      const double a = X[(size_t)i * f + j];
      out[i] = std::isnan(a) ? kMissing : (uint16_t)(std::upper_bound(c, c + m, a) - c);
    }
  });
  return 0;
}

// Grow one tree on binned features. nbins[j] = ncut[j] + 1. g / h: per-row gradients and hessians. The tree is
// written as parallel arrays of at most max_nodes entries: feature (-1 = leaf), split bin, default_left, left,
// right, value (leaf output, eta applied). leaf_of_row[i] receives the leaf id of row i (for the caller's
// prediction update). Returns the node count, or -1 if max_nodes is too small.
//
// sample (null = all rows): n_rows ascending row ids; the tree is grown on exactly these rows as if the table held
// only them, leaf_of_row is -1 for the others, and an empty list gives the one-node tree of value +0.0.
// level_mask (null = all features): [max_depth, f], a feature with level_mask[d * f + j] == 0 yields no candidate
// at depth d, as nbins[j] == 1 does. -2: a row list that is not ascending inside [0, n).
//
// node_gain / node_cover (nullable, max_nodes doubles each): per node the gain the learner maximised,
// 0.5 * (score_L + score_R - score_parent) - gamma (0.0 at a leaf), and the node's hessian sum over the rows the tree
// was grown on. The tree does not depend on whether they are asked for.
//
// mono (null = unconstrained, and then every expression is the one it always was): [f] directions in {-1, 0, +1}, the
// monotone_constraints rule of gbdt_split.h; every node carries its weight interval.
// nsp (null = none): the per-node feature sets of gbdt_nodeset.h; every node carries its path set, and a feature
// outside the node's split set yields no candidate, as a masked one.
static int grow_double(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                       int max_depth, double min_child_weight, double lambda, double gamma, double eta, int threads,
                       int max_nodes, int* feature, int* split_bin, uint8_t* default_left, int* left, int* right,
                       double* value, int* leaf_of_row, const int* sample, long n_rows, const uint8_t* level_mask,
                       double* node_gain, double* node_cover, const int* mono, const MifxNsSpec* nsp = nullptr) {
  if (!rows_ok(sample, n_rows, n)) return -2;
  const MifxGbParams prm{lambda, gamma, min_child_weight, eta};
  std::vector<int> off(f + 1, 0);
  for (int j = 0; j < f; ++j) off[j + 1] = off[j] + nbins[j] + 1;
  const int hsize = off[f];
  const long ns = sample ? n_rows : n;
  std::vector<int> rows(ns);
  for (long i = 0; i < ns; ++i) rows[i] = sample ? sample[i] : (int)i;
  if (sample)
    for (long i = 0; i < n; ++i) leaf_of_row[i] = -1;
  const int th = ns * (long)f > 200000 ? threads : 1;

  auto build = [&](Node& nd) {
    nd.hist.assign(hsize, Hist{0.0, 0.0});
    parallel_for(f, th, [&](int j) {
      Hist* hj = nd.hist.data() + off[j];
      const uint16_t* bj = bins + (size_t)j * n;
      const int nb = nbins[j];
      for (int k = nd.begin; k < nd.end; ++k) {
        const int r = rows[k];
        const uint16_t b = bj[r];
        Hist& e = hj[b == kMissing ? nb : b];
        e.g += g[r];
        e.h += h[r];
      }
    });
  };
  auto score = [&](double G, double H) { return G * G / (H + lambda); };
  auto best_split = [&](const Node& nd) {
    std::vector<Split> per(f);
    const double parent = mono ? mifx_gb_mono_parent(nd.g, nd.h, lambda, nd.lo, nd.hi) : score(nd.g, nd.h);
    const uint8_t* lrow = level_mask ? level_mask + (size_t)nd.depth * f : nullptr;
    std::vector<uint8_t> allow;  // the node's mask row
    if (nsp) {
      allow.resize(f);
      mifx_ns_node_mask(*nsp, f, (uint64_t)nd.id, nd.S.data(), lrow, allow.data());
    }
    parallel_for(f, th, [&](int j) {
      const Hist* hj = nd.hist.data() + off[j];
      const int nb = (nsp ? !(allow[j] & MIFX_NS_SPLIT) : lrow && !lrow[j]) ? 1 : nbins[j];
      const double gm = hj[nbins[j]].g, hm = hj[nbins[j]].h;
      Split bs;
      double gl = 0, hl = 0;
      for (int b = 0; b + 1 < nb; ++b) {  // cut after bin b
        gl += hj[b].g;
        hl += hj[b].h;
        for (int dir = 0; dir < 2; ++dir) {  // dir 0: missing right, 1: missing left
          if (dir == 1 && hm == 0.0 && gm == 0.0) break;
          const double GL = gl + (dir ? gm : 0.0), HL = hl + (dir ? hm : 0.0);
          const double GR = nd.g - GL, HR = nd.h - HL;
          if (HL < min_child_weight || HR < min_child_weight) continue;
          double gain;
          if (!mono) gain = 0.5 * (score(GL, HL) + score(GR, HR) - parent) - gamma;
          else if (!mifx_gb_mono_gain(GL, HL, GR, HR, prm, parent, mono[j], nd.lo, nd.hi, &gain)) continue;
          if (gain > bs.gain) {
            bs.gain = gain;
            bs.feature = j;
            bs.bin = b;
            bs.default_left = dir == 1;
            bs.gl = GL, bs.hl = HL, bs.gr = GR, bs.hr = HR;
          }
        }
      }
      per[j] = bs;
    });
    Split best;
    for (int j = 0; j < f; ++j)
      if (per[j].feature >= 0 && per[j].gain > best.gain + 1e-12 * std::fabs(best.gain)) best = per[j];
    return best;
  };

  int count = 0;
  auto new_node = [&]() -> int {
    if (count >= max_nodes) return -1;
    feature[count] = -1;
    split_bin[count] = -1;
    default_left[count] = 0;
    left[count] = right[count] = -1;
    value[count] = 0.0;
    if (node_gain) node_gain[count] = 0.0;
    if (node_cover) node_cover[count] = 0.0;
    return count++;
  };
  Node root{0, (int)ns, 0, new_node(), 0.0, 0.0, {}, -INFINITY, INFINITY, {}};
  if (nsp) root.S.assign(mifx_ns_words(f), 0);
  if (root.id < 0) return -1;
  if (ns == 0) return count;  // nothing sampled: the root alone, value +0.0
  for (long i = 0; i < ns; ++i) {
    root.g += g[rows[i]];
    root.h += h[rows[i]];
  }
  build(root);
  std::vector<Node> level;
  level.push_back(std::move(root));
  auto make_leaf = [&](const Node& nd) {
    value[nd.id] = mono ? eta * mifx_gb_mono_weight(nd.g, nd.h, lambda, nd.lo, nd.hi) : -eta * nd.g / (nd.h + lambda);
    for (int k = nd.begin; k < nd.end; ++k) leaf_of_row[rows[k]] = nd.id;
  };
  while (!level.empty()) {
    std::vector<Node> next;
    for (Node& nd : level) {
      Split s;
      if (nd.depth < max_depth && nd.end - nd.begin >= 2) s = best_split(nd);
      if (node_cover) node_cover[nd.id] = nd.h;
      if (s.feature < 0 || s.gain <= 1e-6) {
        make_leaf(nd);
        continue;
      }
      if (node_gain) node_gain[nd.id] = s.gain;
      // partition rows: left = bin <= s.bin (or missing with default_left)
      const uint16_t* bj = bins + (size_t)s.feature * n;
      auto goes_left = [&](int r) {
        const uint16_t b = bj[r];
        return b == kMissing ? s.default_left : (int)b <= s.bin;
      };
      const int mid = (int)(std::stable_partition(rows.begin() + nd.begin, rows.begin() + nd.end, goes_left) -
                            rows.begin());
      const int li = new_node(), ri = new_node();
      if (li < 0 || ri < 0) return -1;
      feature[nd.id] = s.feature;
      split_bin[nd.id] = s.bin;
      default_left[nd.id] = s.default_left;
      left[nd.id] = li;
      right[nd.id] = ri;
      double b[4] = {nd.lo, nd.hi, nd.lo, nd.hi};  // the children's intervals
      if (mono) mifx_gb_mono_children(s.gl, s.hl, s.gr, s.hr, lambda, mono[s.feature], nd.lo, nd.hi, b);
      Node L{nd.begin, mid, nd.depth + 1, li, s.gl, s.hl, {}, b[0], b[1], {}};
      Node R{mid, nd.end, nd.depth + 1, ri, s.gr, s.hr, {}, b[2], b[3], {}};
      if (nsp) L.S = R.S = child_set(nd.S, s.feature);
      const bool grow_more = nd.depth + 1 < max_depth;
      if (grow_more) {  // smaller child built, larger = parent - smaller
        Node& small = (L.end - L.begin) <= (R.end - R.begin) ? L : R;
        Node& large = &small == &L ? R : L;
        build(small);
        large.hist = std::move(nd.hist);
        for (int k = 0; k < hsize; ++k) {
          large.hist[k].g -= small.hist[k].g;
          large.hist[k].h -= small.hist[k].h;
        }
      }
      next.push_back(std::move(L));
      next.push_back(std::move(R));
    }
    level = std::move(next);
  }
  return count;
}

int mifx_gbdt_grow_stats(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                         int max_depth, double min_child_weight, double lambda, double gamma, double eta, int threads,
                         int max_nodes, int* feature, int* split_bin, uint8_t* default_left, int* left, int* right,
                         double* value, int* leaf_of_row, const int* sample, long n_rows, const uint8_t* level_mask,
                         double* node_gain, double* node_cover) {
  return grow_double(bins, n, f, nbins, g, h, max_depth, min_child_weight, lambda, gamma, eta, threads, max_nodes,
                     feature, split_bin, default_left, left, right, value, leaf_of_row, sample, n_rows, level_mask,
                     node_gain, node_cover, nullptr);
}

// mifx_gbdt_grow_stats under monotone_constraints: mono [f] in {-1, 0, +1} (-3: anything else, or null)
int mifx_gbdt_grow_mono(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                        int max_depth, double min_child_weight, double lambda, double gamma, double eta, int threads,
                        int max_nodes, int* feature, int* split_bin, uint8_t* default_left, int* left, int* right,
                        double* value, int* leaf_of_row, const int* sample, long n_rows, const uint8_t* level_mask,
                        double* node_gain, double* node_cover, const int* mono) {
  if (!mono_ok(mono, f)) return -3;
  return grow_double(bins, n, f, nbins, g, h, max_depth, min_child_weight, lambda, gamma, eta, threads, max_nodes,
                     feature, split_bin, default_left, left, right, value, leaf_of_row, sample, n_rows, level_mask,
                     node_gain, node_cover, mono);
}

int mifx_gbdt_grow_ex(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                      int max_depth, double min_child_weight, double lambda, double gamma, double eta, int threads,
                      int max_nodes, int* feature, int* split_bin, uint8_t* default_left, int* left, int* right,
                      double* value, int* leaf_of_row, const int* sample, long n_rows, const uint8_t* level_mask) {
  return mifx_gbdt_grow_stats(bins, n, f, nbins, g, h, max_depth, min_child_weight, lambda, gamma, eta, threads,
                              max_nodes, feature, split_bin, default_left, left, right, value, leaf_of_row, sample,
                              n_rows, level_mask, nullptr, nullptr);
}

int mifx_gbdt_grow(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                   int max_depth, double min_child_weight, double lambda, double gamma, double eta, int threads,
                   int max_nodes, int* feature, int* split_bin, uint8_t* default_left, int* left, int* right,
                   double* value, int* leaf_of_row) {
  return mifx_gbdt_grow_ex(bins, n, f, nbins, g, h, max_depth, min_child_weight, lambda, gamma, eta, threads,
                           max_nodes, feature, split_bin, default_left, left, right, value, leaf_of_row, nullptr, 0,
                           nullptr);
}

// ---- fixed-point twin of mifx_gbdt_grow (gbdt_split.h): int64 histograms, so the tree cannot depend on the order
// of any sum -- the host reference that the device learner (csrc/gbdt_gpu.hip) reproduces bit for bit.

int mifx_gbdt_quant_exp(double amax, long n) { return mifx_gb_quant_exp(amax, n); }

// mifx_gbdt_grow's signature and outputs; the semantics are the fixed-point ones of gbdt_split.h. On gradients that
// quantise exactly and sum exactly in double (small dyadic rationals) it grows exactly mifx_gbdt_grow's tree.
// sample / level_mask: as in mifx_gbdt_grow_ex; the exponents come from the sampled rows alone (their largest
// magnitudes and their count).
// node_gain / node_cover: as in mifx_gbdt_grow_stats; the gain is MifxGbSplit::gain, the cover mifx_gb_dequant(Qh, eh).
// mono (null = unconstrained): as in grow_double, the scan is then mifx_gb_scan_mono.
static int grow_fixed(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                      int max_depth, double min_child_weight, double lambda, double gamma, double eta, int threads,
                      int max_nodes, int* feature, int* split_bin, uint8_t* default_left, int* left, int* right,
                      double* value, int* leaf_of_row, const int* sample, long n_rows, const uint8_t* level_mask,
                      double* node_gain, double* node_cover, const int* mono, const MifxNsSpec* nsp = nullptr) {
  if (!rows_ok(sample, n_rows, n)) return -2;
  struct QNode {
    int begin, end, depth, id;
    long long g, h;
    std::vector<long long> hg, hh;  // [features][nbins + 1], the last slot is "missing"
    std::vector<int> hc;            // rows per slot
    double lo, hi;                  // the weight interval of monotone_constraints
    std::vector<uint64_t> S;        // the path set of gbdt_nodeset.h (kept only under a node-set spec, nsp)
  };
  const MifxGbParams prm{lambda, gamma, min_child_weight, eta};
  std::vector<int> off(f + 1, 0);
  for (int j = 0; j < f; ++j) off[j + 1] = off[j] + nbins[j] + 1;
  const int hsize = off[f];
  const long ns = sample ? n_rows : n;
  std::vector<int> rows(ns);
  for (long i = 0; i < ns; ++i) rows[i] = sample ? sample[i] : (int)i;
  if (sample)
    for (long i = 0; i < n; ++i) leaf_of_row[i] = -1;
  const int th = ns * (long)f > 200000 ? threads : 1;

  // quantisation: the largest magnitudes (max is order-independent), one exponent each, then the rows
  auto amax = [&](const float* v) {
    double a = 0.0;
    for (long i = 0; i < ns; ++i) {
      const double x = std::fabs((double)v[rows[i]]);
      if (!(x <= a)) a = x;  // a NaN sticks: the exponent is then 0
      if (std::isnan(x)) return x;
    }
    return a;
  };
  const int eg = mifx_gb_quant_exp(amax(g), ns), eh = mifx_gb_quant_exp(amax(h), ns);
  std::vector<long long> qg(n), qh(n);  // indexed by row id; rows outside the sample are never read
  for (long i = 0; i < ns; ++i) {
    const int r = rows[i];
    qg[r] = mifx_gb_quantise(g[r], eg);
    qh[r] = mifx_gb_quantise(h[r], eh);
  }

  auto build = [&](QNode& nd) {
    nd.hg.assign(hsize, 0);
    nd.hh.assign(hsize, 0);
    nd.hc.assign(hsize, 0);
    parallel_for(f, th, [&](int j) {
      const uint16_t* bj = bins + (size_t)j * n;
      const int nb = nbins[j];
      for (int k = nd.begin; k < nd.end; ++k) {
        const int r = rows[k];
        const uint16_t b = bj[r];
        const int s = off[j] + ((int)b < nb ? (int)b : nb);  // 0xFFFF, or anything past the bins: missing
        nd.hg[s] += qg[r];
        nd.hh[s] += qh[r];
        nd.hc[s] += 1;
      }
    });
  };
  auto best_split = [&](const QNode& nd) {
    std::vector<MifxGbSplit> per(f);
    const double parent = mono ? mifx_gb_mono_parent(mifx_gb_dequant(nd.g, eg), mifx_gb_dequant(nd.h, eh), lambda,
                                                     nd.lo, nd.hi)
                               : mifx_gb_parent_score(nd.g, nd.h, eg, eh, prm);
    const uint8_t* lrow = level_mask ? level_mask + (size_t)nd.depth * f : nullptr;
    std::vector<uint8_t> allow;  // the node's mask row
    if (nsp) {
      allow.resize(f);
      mifx_ns_node_mask(*nsp, f, (uint64_t)nd.id, nd.S.data(), lrow, allow.data());
    }
    parallel_for(f, th, [&](int j) {
      MifxGbSplit bs = mifx_gb_no_split();
      const bool live = nsp ? (allow[j] & MIFX_NS_SPLIT) != 0 : !lrow || lrow[j];
      if (live && mono)
        mifx_gb_scan_mono(nd.hg.data() + off[j], nd.hh.data() + off[j], nd.hc.data() + off[j], nbins[j], 0, nbins[j],
                          0, 0, 0, nd.g, nd.h, eg, eh, j, prm, parent, mono[j], nd.lo, nd.hi, &bs);
      else if (live)
        mifx_gb_scan(nd.hg.data() + off[j], nd.hh.data() + off[j], nd.hc.data() + off[j], nbins[j], 0, nbins[j], 0,
                     0, 0, nd.g, nd.h, eg, eh, j, prm, parent, &bs);
      per[j] = bs;
    });
    MifxGbSplit best = mifx_gb_no_split();
    for (int j = 0; j < f; ++j)
      if (mifx_gb_feature_wins(per[j], best)) best = per[j];
    return best;
  };

  int count = 0;
  auto new_node = [&]() -> int {
    if (count >= max_nodes) return -1;
    feature[count] = -1;
    split_bin[count] = -1;
    default_left[count] = 0;
    left[count] = right[count] = -1;
    value[count] = 0.0;
    if (node_gain) node_gain[count] = 0.0;
    if (node_cover) node_cover[count] = 0.0;
    return count++;
  };
  QNode root{0, (int)ns, 0, new_node(), 0, 0, {}, {}, {}, -INFINITY, INFINITY, {}};
  if (nsp) root.S.assign(mifx_ns_words(f), 0);
  if (root.id < 0) return -1;
  if (ns == 0) return count;  // nothing sampled: the root alone, value +0.0
  for (long i = 0; i < ns; ++i) {
    root.g += qg[rows[i]];
    root.h += qh[rows[i]];
  }
  if (max_depth > 0) build(root);
  std::vector<QNode> level;
  level.push_back(std::move(root));
  while (!level.empty()) {
    std::vector<QNode> next;
    for (QNode& nd : level) {
      MifxGbSplit s = mifx_gb_no_split();
      if (nd.depth < max_depth && nd.end - nd.begin >= 2) s = best_split(nd);
      if (node_cover) node_cover[nd.id] = mifx_gb_dequant(nd.h, eh);
      if (mifx_gb_is_leaf(s)) {
        value[nd.id] = mono ? mifx_gb_mono_leaf_value(nd.g, nd.h, eg, eh, prm, nd.lo, nd.hi)
                            : mifx_gb_leaf_value(nd.g, nd.h, eg, eh, prm);
        for (int k = nd.begin; k < nd.end; ++k) leaf_of_row[rows[k]] = nd.id;
        continue;
      }
      const uint16_t* bj = bins + (size_t)s.feature * n;
      const int nb = nbins[s.feature];
      auto goes_left = [&](int r) {
        const int b = bj[r];
        return b < nb ? b <= s.bin : s.default_left != 0;
      };
      const int mid = (int)(std::stable_partition(rows.begin() + nd.begin, rows.begin() + nd.end, goes_left) -
                            rows.begin());
      const int li = new_node(), ri = new_node();
      if (li < 0 || ri < 0) return -1;
      if (node_gain) node_gain[nd.id] = s.gain;
      feature[nd.id] = s.feature;
      split_bin[nd.id] = s.bin;
      default_left[nd.id] = (uint8_t)s.default_left;
      left[nd.id] = li;
      right[nd.id] = ri;
      double b[4] = {nd.lo, nd.hi, nd.lo, nd.hi};  // the children's intervals
      if (mono) mifx_gb_mono_children_q(s, nd.g, nd.h, eg, eh, prm, mono[s.feature], nd.lo, nd.hi, b);
      QNode L{nd.begin, mid, nd.depth + 1, li, s.gl, s.hl, {}, {}, {}, b[0], b[1], {}};
      QNode R{mid, nd.end, nd.depth + 1, ri, nd.g - s.gl, nd.h - s.hl, {}, {}, {}, b[2], b[3], {}};
      if (nsp) L.S = R.S = child_set(nd.S, s.feature);
      if (nd.depth + 1 < max_depth) {  // smaller child built, larger = parent - smaller (identical in integers)
        QNode& small = (L.end - L.begin) <= (R.end - R.begin) ? L : R;
        QNode& large = &small == &L ? R : L;
        build(small);
        large.hg = std::move(nd.hg);
        large.hh = std::move(nd.hh);
        large.hc = std::move(nd.hc);
        for (int k = 0; k < hsize; ++k) {
          large.hg[k] -= small.hg[k];
          large.hh[k] -= small.hh[k];
          large.hc[k] -= small.hc[k];
        }
      }
      next.push_back(std::move(L));
      next.push_back(std::move(R));
    }
    level = std::move(next);
  }
  return count;
}

int mifx_gbdt_grow_fixed_stats(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                               int max_depth, double min_child_weight, double lambda, double gamma, double eta,
                               int threads, int max_nodes, int* feature, int* split_bin, uint8_t* default_left,
                               int* left, int* right, double* value, int* leaf_of_row, const int* sample, long n_rows,
                               const uint8_t* level_mask, double* node_gain, double* node_cover) {
  return grow_fixed(bins, n, f, nbins, g, h, max_depth, min_child_weight, lambda, gamma, eta, threads, max_nodes,
                    feature, split_bin, default_left, left, right, value, leaf_of_row, sample, n_rows, level_mask,
                    node_gain, node_cover, nullptr);
}

// mifx_gbdt_grow_fixed_stats under monotone_constraints: the host twin of mifx_gbdt_gpu_grow_mono
int mifx_gbdt_grow_fixed_mono(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                              int max_depth, double min_child_weight, double lambda, double gamma, double eta,
                              int threads, int max_nodes, int* feature, int* split_bin, uint8_t* default_left,
                              int* left, int* right, double* value, int* leaf_of_row, const int* sample, long n_rows,
                              const uint8_t* level_mask, double* node_gain, double* node_cover, const int* mono) {
  if (!mono_ok(mono, f)) return -3;
  return grow_fixed(bins, n, f, nbins, g, h, max_depth, min_child_weight, lambda, gamma, eta, threads, max_nodes,
                    feature, split_bin, default_left, left, right, value, leaf_of_row, sample, n_rows, level_mask,
                    node_gain, node_cover, mono);
}

int mifx_gbdt_grow_fixed_ex(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                            int max_depth, double min_child_weight, double lambda, double gamma, double eta,
                            int threads, int max_nodes, int* feature, int* split_bin, uint8_t* default_left, int* left,
                            int* right, double* value, int* leaf_of_row, const int* sample, long n_rows,
                            const uint8_t* level_mask) {
  return mifx_gbdt_grow_fixed_stats(bins, n, f, nbins, g, h, max_depth, min_child_weight, lambda, gamma, eta, threads,
                                    max_nodes, feature, split_bin, default_left, left, right, value, leaf_of_row,
                                    sample, n_rows, level_mask, nullptr, nullptr);
}

int mifx_gbdt_grow_fixed(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                         int max_depth, double min_child_weight, double lambda, double gamma, double eta, int threads,
                         int max_nodes, int* feature, int* split_bin, uint8_t* default_left, int* left, int* right,
                         double* value, int* leaf_of_row) {
  return mifx_gbdt_grow_fixed_ex(bins, n, f, nbins, g, h, max_depth, min_child_weight, lambda, gamma, eta, threads,
                                 max_nodes, feature, split_bin, default_left, left, right, value, leaf_of_row, nullptr,
                                 0, nullptr);
}

// The depth-wise growers with per-node feature sets (interaction_constraints, colsample_bynode: the rule of
// gbdt_nodeset.h): the arguments of mifx_gbdt_grow_mono with a nullable mono, in front of them `fixed` (0: the double
// learner, 1: the fixed-point one, the host twin of mifx_gbdt_gpu_grow_nodeset), and after them groups (nullable)
// [n_groups, ceil(f / 64)] uint64 bitsets, the colsample_bynode rate (1.0: no draw) and the draw's (seed, round).
// level_mask is then every node's level set. -3: directions or a spec out of range.
int mifx_gbdt_grow_nodeset(int fixed, const uint16_t* bins, long n, int f, const int* nbins, const float* g,
                           const float* h, int max_depth, double min_child_weight, double lambda, double gamma,
                           double eta, int threads, int max_nodes, int* feature, int* split_bin, uint8_t* default_left,
                           int* left, int* right, double* value, int* leaf_of_row, const int* sample, long n_rows,
                           const uint8_t* level_mask, double* node_gain, double* node_cover, const int* mono,
                           const uint64_t* groups, int n_groups, double bynode, uint64_t seed, uint64_t round) {
  const MifxNsSpec ns{groups, groups ? n_groups : 0, bynode, seed, round};
  if ((mono && !mono_ok(mono, f)) || !nodeset_ok(ns, f)) return -3;
  return (fixed ? grow_fixed : grow_double)(bins, n, f, nbins, g, h, max_depth, min_child_weight, lambda, gamma, eta,
                                            threads, max_nodes, feature, split_bin, default_left, left, right, value,
                                            leaf_of_row, sample, n_rows, level_mask, node_gain, node_cover, mono, &ns);
}

// ---- the leaf refresh of reg:absoluteerror / reg:quantileerror (gbdt_quantile.h has the rule): value[l] of every leaf
// l < nodes that holds rows becomes eta times the weighted lower alpha-quantile of resid over the rows with
// leaf_of_row == l (-1: a row outside the sample). h [n]: the float32 hessians the tree was grown from; their integer
// weights use the exponent of the rows with a leaf. A leaf of total weight 0 keeps its value. The leaves are
// independent: the same bits for any thread count. Returns 0, or -1 for a leaf id outside [-1, nodes).
int mifx_gbdt_leaf_refresh(const double* resid, const float* h, const int* leaf_of_row, long n, int nodes, double alpha,
                           double eta, double* value, int threads) {
  if (n < 0 || nodes < 1) return -1;
  std::vector<long> off(nodes + 1, 0);
  double amax = 0.0;
  long ns = 0;
  for (long i = 0; i < n; ++i) {
    const int l = leaf_of_row[i];
    if (l < -1 || l >= nodes) return -1;
    if (l < 0) continue;
    ++off[l + 1];
    ++ns;
    amax = std::max(amax, std::fabs((double)h[i]));
  }
  const int eh = mifx_gq_exp(amax, ns);
  for (int l = 0; l < nodes; ++l) off[l + 1] += off[l];
  struct Row {
    uint64_t key;
    long long q;
  };
  std::vector<Row> rows(ns);
  std::vector<long> cur(off.begin(), off.end() - 1);
  for (long i = 0; i < n; ++i)
    if (leaf_of_row[i] >= 0) rows[cur[leaf_of_row[i]]++] = Row{mifx_sort_key(resid[i]), mifx_gq_weight(h[i], eh)};
  parallel_for(nodes, ns > 100000 ? threads : 1, [&](int l) {
    Row *b = rows.data() + off[l], *e = rows.data() + off[l + 1];
    long long Q = 0;
    for (Row* r = b; r < e; ++r) Q += r->q;
    if (Q <= 0) return;
    std::sort(b, e, [](const Row& x, const Row& y) { return x.key < y.key; });
    long long left = mifx_gq_threshold(alpha, Q);
    for (Row* r = b; r < e; ++r)
      if ((left -= r->q) <= 0) {  // equal keys are adjacent: the first row that reaches T carries the selected key
        value[l] = mifx_gq_value(r->key, eta);
        return;
      }
  });
  return 0;
}

// ---- the LambdaMART pair of rank:pairwise (objective 0) / rank:ndcg (objective 1), gbdt_rank.h has the rule. margin
// [n], y [n] (integer labels in [0, 31] as doubles), gptr [G + 1] the groups' row offsets, D and P the discount table
// and its prefix sums (each longer than the largest group), topk 0 for every pair. A plain sort per group, then every
// row walks its partners in rank order. The groups are independent: the same bits for any thread count. Returns 0, or
// -1 for offsets that do not cover [0, n] in order or a label outside [0, 31].
int mifx_gbdt_rank_grad(int objective, const double* margin, const double* y, const long* gptr, long G, const double* D,
                        const double* P, int topk, float* g, float* h, int threads) {
  if (objective < 0 || objective > 1 || G < 0 || topk < 0 || gptr[0] != 0) return -1;
  for (long q = 0; q < G; ++q)
    if (gptr[q + 1] < gptr[q] || gptr[q + 1] - gptr[q] > 0x7FFFFFFF) return -1;
  for (long i = 0; i < gptr[G]; ++i)
    if (!(y[i] >= 0.0 && y[i] < (double)kMifxRankLabels) || y[i] != (double)(int)y[i]) return -1;
  parallel_for((int)std::min<long>(G, 0x7FFFFFFF), gptr[G] > 2000 ? threads : 1, [&](int q) {
    const long b = gptr[q];
    const int m = (int)(gptr[q + 1] - b);
    std::vector<uint64_t> key(m);
    std::vector<int> at(m), label(m), cnt(kMifxRankLabels, 0);
    for (int i = 0; i < m; ++i) {
      key[i] = mifx_sort_key(margin[b + i]);
      at[i] = i;
      ++cnt[label[i] = (int)y[b + i]];
    }
    std::sort(at.begin(), at.end(), [&](int i, int j) { return mifx_rk_before(key[i], i, key[j], j); });
    const double idcg = objective ? mifx_rk_idcg(cnt.data(), P) : 0.0;
    for (int ra = 0; ra < m; ++ra) {
      const int a = at[ra], end = mifx_rk_partner_end(ra, m, topk);
      double gs = 0.0, hs = 0.0;
      for (int r = 0; r < end; ++r)
        if (label[at[r]] != label[a])
          mifx_rk_accum(objective != 0, idcg, margin[b + a], label[a], D[ra], margin[b + at[r]], label[at[r]], D[r],
                        &gs, &hs);
      g[b + a] = (float)gs;
      h[b + a] = (float)hs;
    }
  });
  return 0;
}

// ---- the integers of eval_metric="auc", gbdt_auc.h has the rule. margin [K, m] class-major, y [m] the class index as
// a double (K = 1: 0.0 / 1.0, class 0's margins scored against y == 1; K >= 2: row k against y == k). out [K, 3]:
// (U2, P, N) per class. The 2 K (class, side) lists sort side by side, then one merge walk per class: integer counts,
// the same for any thread count. Returns 0, -1 for bad arguments, -2 for a margin that is not finite.
int mifx_gbdt_auc(const double* margin, const double* y, long m, int K, long long* out, int threads) {
  if (m < 0 || m >= (1L << 31) || K < 1) return -1;
  for (long i = 0; i < (long)K * m; ++i)
    if (!std::isfinite(margin[i])) return -2;
  std::vector<std::vector<double>> side(2 * (size_t)K);
  parallel_for(2 * K, (long)K * m > 20000 ? threads : 1, [&](int s) {
    const int k = s >> 1;
    const double want = K == 1 ? 1.0 : (double)k;
    std::vector<double>& v = side[s];
    for (long i = 0; i < m; ++i)
      if ((y[i] == want) == (bool)(s & 1)) v.push_back(margin[(size_t)k * m + i]);
    std::sort(v.begin(), v.end());
  });
  parallel_for(K, (long)K * m > 20000 ? threads : 1, [&](int k) {
    const std::vector<double>&neg = side[2 * k], &pos = side[2 * k + 1];
    out[3 * k + 0] = mifx_auc_merge(neg.data(), (long)neg.size(), pos.data(), (long)pos.size());
    out[3 * k + 1] = (long long)pos.size();
    out[3 * k + 2] = (long long)neg.size();
  });
  return 0;
}

}  // extern "C"

// ---- leaf-wise growth (grow_policy="lossguide"): the open node with the largest gain is split next (ties: the lowest
// id), until max_leaves leaves exist or no node is open; children take the next two ids, left then right. A node's
// candidate is its depth-wise one (same histograms, same scan), so the tree is the best-first prefix of the depth-wise
// tree with the same depth limit. One driver; a Core supplies the arithmetic of one learner.
namespace {

struct LgArgs {
  const uint16_t* bins;
  long n;
  int f;
  const int* nbins;
  const float *g, *h;
  int max_depth, max_leaves;  // max_depth 0: no limit
  double min_child_weight, lambda, gamma, eta;
  int threads, max_nodes;
  int *feature, *split_bin;
  uint8_t* default_left;
  int *left, *right;
  double* value;
  int* leaf_of_row;
  const int* sample;
  long n_rows;
  const uint8_t* feature_mask;  // [f], null = all
  double *node_gain, *node_cover;
  const int* mono = nullptr;  // [f] monotone_constraints (gbdt_split.h), null = unconstrained
  const MifxNsSpec* ns = nullptr;  // per-node feature sets (gbdt_nodeset.h), null = none; feature_mask is the level set
};

struct LgCand {  // a node's candidate in either arithmetic
  double gain = 0.0;
  int feature = -1, bin = -1, default_left = 0;
  bool leaf = true;
};

// the double learner of mifx_gbdt_grow_stats: smaller child built in row order, larger = parent - smaller
struct DoubleCore {
  struct Node {
    int begin, end, depth, id;
    LgCand cand;
    double g = 0, h = 0, gl = 0, hl = 0;  // sums; the candidate's left sums
    std::vector<Hist> hist;
    double lo = -INFINITY, hi = INFINITY;  // the weight interval of monotone_constraints
    std::vector<uint64_t> S;               // the path set of gbdt_nodeset.h (kept only under a spec)
  };
  const LgArgs& a;
  const std::vector<int>& off;
  const std::vector<int>& rows;
  int th;
  void start(Node& root) {
    for (int r : rows) {
      root.g += a.g[r];
      root.h += a.h[r];
    }
  }
  void build(Node& nd) {
    nd.hist.assign(off[a.f], Hist{0.0, 0.0});
    parallel_for(a.f, th, [&](int j) {
      Hist* hj = nd.hist.data() + off[j];
      const uint16_t* bj = a.bins + (size_t)j * a.n;
      for (int k = nd.begin; k < nd.end; ++k) {
        const uint16_t b = bj[rows[k]];
        Hist& e = hj[b == kMissing ? a.nbins[j] : b];
        e.g += a.g[rows[k]];
        e.h += a.h[rows[k]];
      }
    });
  }
  void inherit(Node& large, Node& parent, const Node& small) {
    large.hist = std::move(parent.hist);
    for (size_t k = 0; k < large.hist.size(); ++k) {
      large.hist[k].g -= small.hist[k].g;
      large.hist[k].h -= small.hist[k].h;
    }
  }
  void release(Node& nd) { std::vector<Hist>().swap(nd.hist); }
  void search(Node& nd, const uint8_t* allow) {  // allow (nullable): the node's mask row of gbdt_nodeset.h
    std::vector<Split> per(a.f);
    auto score = [&](double G, double H) { return G * G / (H + a.lambda); };
    const MifxGbParams prm{a.lambda, a.gamma, a.min_child_weight, a.eta};
    const double parent = a.mono ? mifx_gb_mono_parent(nd.g, nd.h, a.lambda, nd.lo, nd.hi) : score(nd.g, nd.h);
    parallel_for(a.f, th, [&](int j) {
      const Hist* hj = nd.hist.data() + off[j];
      const int nb = (allow ? !(allow[j] & MIFX_NS_SPLIT) : a.feature_mask && !a.feature_mask[j]) ? 1 : a.nbins[j];
      const double gm = hj[a.nbins[j]].g, hm = hj[a.nbins[j]].h;
      Split bs;
      double gl = 0, hl = 0;
      for (int b = 0; b + 1 < nb; ++b) {
        gl += hj[b].g;
        hl += hj[b].h;
        for (int dir = 0; dir < 2; ++dir) {
          if (dir == 1 && hm == 0.0 && gm == 0.0) break;
          const double GL = gl + (dir ? gm : 0.0), HL = hl + (dir ? hm : 0.0);
          const double GR = nd.g - GL, HR = nd.h - HL;
          if (HL < a.min_child_weight || HR < a.min_child_weight) continue;
          double gain;
          if (!a.mono) gain = 0.5 * (score(GL, HL) + score(GR, HR) - parent) - a.gamma;
          else if (!mifx_gb_mono_gain(GL, HL, GR, HR, prm, parent, a.mono[j], nd.lo, nd.hi, &gain)) continue;
          if (gain > bs.gain) {
            bs.gain = gain, bs.feature = j, bs.bin = b, bs.default_left = dir == 1;
            bs.gl = GL, bs.hl = HL, bs.gr = GR, bs.hr = HR;
          }
        }
      }
      per[j] = bs;
    });
    Split best;
    for (int j = 0; j < a.f; ++j)
      if (per[j].feature >= 0 && per[j].gain > best.gain + 1e-12 * std::fabs(best.gain)) best = per[j];
    nd.cand = LgCand{best.gain, best.feature, best.bin, best.default_left, best.feature < 0 || best.gain <= 1e-6};
    nd.gl = best.gl, nd.hl = best.hl;
  }
  bool goes_left(const LgCand& c, int r) const {
    const uint16_t b = a.bins[(size_t)c.feature * a.n + r];
    return b == kMissing ? c.default_left != 0 : (int)b <= c.bin;
  }
  void children(const Node& p, Node& L, Node& R) const {
    L.g = p.gl, L.h = p.hl;
    R.g = p.g - p.gl, R.h = p.h - p.hl;  // (the depth-wise learner's GR, HR)
    if (!a.mono) return;
    double b[4];
    mifx_gb_mono_children(L.g, L.h, R.g, R.h, a.lambda, a.mono[p.cand.feature], p.lo, p.hi, b);
    L.lo = b[0], L.hi = b[1], R.lo = b[2], R.hi = b[3];
  }
  double value(const Node& nd) const {
    return a.mono ? a.eta * mifx_gb_mono_weight(nd.g, nd.h, a.lambda, nd.lo, nd.hi) : -a.eta * nd.g / (nd.h + a.lambda);
  }
  double cover(const Node& nd) const { return nd.h; }
};

// the fixed-point learner of mifx_gbdt_grow_fixed_stats (gbdt_split.h): the device twin
struct FixedCore {
  struct Node {
    int begin, end, depth, id;
    LgCand cand;
    long long g = 0, h = 0, gl = 0, hl = 0;
    std::vector<long long> hg, hh;
    std::vector<int> hc;
    double lo = -INFINITY, hi = INFINITY;  // the weight interval of monotone_constraints
    std::vector<uint64_t> S;               // the path set of gbdt_nodeset.h (kept only under a spec)
  };
  const LgArgs& a;
  const std::vector<int>& off;
  const std::vector<int>& rows;
  int th;
  MifxGbParams prm{a.lambda, a.gamma, a.min_child_weight, a.eta};
  int eg = 0, eh = 0;
  std::vector<long long> qg, qh;  // by row id; rows outside the sample are never read
  void start(Node& root) {
    const long ns = (long)rows.size();
    auto amax = [&](const float* v) {
      double m = 0.0;
      for (int r : rows) {
        const double x = std::fabs((double)v[r]);
        if (!(x <= m)) m = x;  // a NaN sticks: the exponent is then 0
        if (std::isnan(x)) return x;
      }
      return m;
    };
    eg = mifx_gb_quant_exp(amax(a.g), ns), eh = mifx_gb_quant_exp(amax(a.h), ns);
    qg.assign(a.n, 0), qh.assign(a.n, 0);
    for (int r : rows) {
      root.g += qg[r] = mifx_gb_quantise(a.g[r], eg);
      root.h += qh[r] = mifx_gb_quantise(a.h[r], eh);
    }
  }
  void build(Node& nd) {
    nd.hg.assign(off[a.f], 0), nd.hh.assign(off[a.f], 0), nd.hc.assign(off[a.f], 0);
    parallel_for(a.f, th, [&](int j) {
      const uint16_t* bj = a.bins + (size_t)j * a.n;
      const int nb = a.nbins[j];
      for (int k = nd.begin; k < nd.end; ++k) {
        const int r = rows[k], b = bj[r], s = off[j] + (b < nb ? b : nb);  // anything past the bins: missing
        nd.hg[s] += qg[r];
        nd.hh[s] += qh[r];
        nd.hc[s] += 1;
      }
    });
  }
  void inherit(Node& large, Node& parent, const Node& small) {
    large.hg = std::move(parent.hg), large.hh = std::move(parent.hh), large.hc = std::move(parent.hc);
    for (size_t k = 0; k < large.hg.size(); ++k) {
      large.hg[k] -= small.hg[k];
      large.hh[k] -= small.hh[k];
      large.hc[k] -= small.hc[k];
    }
  }
  void release(Node& nd) {
    std::vector<long long>().swap(nd.hg);
    std::vector<long long>().swap(nd.hh);
    std::vector<int>().swap(nd.hc);
  }
  void search(Node& nd, const uint8_t* allow) {  // allow (nullable): the node's mask row of gbdt_nodeset.h
    std::vector<MifxGbSplit> per(a.f);
    const double parent = a.mono ? mifx_gb_mono_parent(mifx_gb_dequant(nd.g, eg), mifx_gb_dequant(nd.h, eh), a.lambda,
                                                       nd.lo, nd.hi)
                                 : mifx_gb_parent_score(nd.g, nd.h, eg, eh, prm);
    parallel_for(a.f, th, [&](int j) {
      MifxGbSplit bs = mifx_gb_no_split();
      const bool live = allow ? (allow[j] & MIFX_NS_SPLIT) != 0 : !a.feature_mask || a.feature_mask[j];
      if (live && a.mono)
        mifx_gb_scan_mono(nd.hg.data() + off[j], nd.hh.data() + off[j], nd.hc.data() + off[j], a.nbins[j], 0,
                          a.nbins[j], 0, 0, 0, nd.g, nd.h, eg, eh, j, prm, parent, a.mono[j], nd.lo, nd.hi, &bs);
      else if (live)
        mifx_gb_scan(nd.hg.data() + off[j], nd.hh.data() + off[j], nd.hc.data() + off[j], a.nbins[j], 0, a.nbins[j], 0,
                     0, 0, nd.g, nd.h, eg, eh, j, prm, parent, &bs);
      per[j] = bs;
    });
    MifxGbSplit best = mifx_gb_no_split();
    for (int j = 0; j < a.f; ++j)
      if (mifx_gb_feature_wins(per[j], best)) best = per[j];
    nd.cand = LgCand{best.gain, best.feature, best.bin, best.default_left, mifx_gb_is_leaf(best)};
    nd.gl = best.gl, nd.hl = best.hl;
  }
  bool goes_left(const LgCand& c, int r) const {
    const int b = a.bins[(size_t)c.feature * a.n + r];
    return b < a.nbins[c.feature] ? b <= c.bin : c.default_left != 0;
  }
  void children(const Node& p, Node& L, Node& R) const {
    L.g = p.gl, L.h = p.hl;
    R.g = p.g - p.gl, R.h = p.h - p.hl;
    if (!a.mono) return;
    MifxGbSplit s = mifx_gb_no_split();
    s.gl = p.gl, s.hl = p.hl;
    double b[4];
    mifx_gb_mono_children_q(s, p.g, p.h, eg, eh, prm, a.mono[p.cand.feature], p.lo, p.hi, b);
    L.lo = b[0], L.hi = b[1], R.lo = b[2], R.hi = b[3];
  }
  double value(const Node& nd) const {
    return a.mono ? mifx_gb_mono_leaf_value(nd.g, nd.h, eg, eh, prm, nd.lo, nd.hi)
                  : mifx_gb_leaf_value(nd.g, nd.h, eg, eh, prm);
  }
  double cover(const Node& nd) const { return mifx_gb_dequant(nd.h, eh); }
};

template <class Core>
int grow_lossguide(const LgArgs& a) {
  using Node = typename Core::Node;
  if (a.max_leaves < 1 || a.max_depth < 0) return -1;
  if (!rows_ok(a.sample, a.n_rows, a.n)) return -2;
  std::vector<int> off(a.f + 1, 0);
  for (int j = 0; j < a.f; ++j) off[j + 1] = off[j] + a.nbins[j] + 1;
  const long ns = a.sample ? a.n_rows : a.n;
  std::vector<int> rows(ns);
  for (long i = 0; i < ns; ++i) rows[i] = a.sample ? a.sample[i] : (int)i;
  if (a.sample)
    for (long i = 0; i < a.n; ++i) a.leaf_of_row[i] = -1;
  Core core{a, off, rows, ns * (long)a.f > 200000 ? a.threads : 1};

  std::vector<Node> nodes;  // by id; a node's histogram lives until the node is split or closed
  std::vector<int> open;
  auto add = [&](int begin, int end, int depth) -> Node* {
    const int id = (int)nodes.size();
    if (id >= a.max_nodes) return nullptr;
    a.feature[id] = a.split_bin[id] = a.left[id] = a.right[id] = -1;
    a.default_left[id] = 0;
    a.value[id] = 0.0;
    if (a.node_gain) a.node_gain[id] = 0.0;
    if (a.node_cover) a.node_cover[id] = 0.0;
    nodes.push_back(Node{begin, end, depth, id});
    return &nodes.back();
  };
  auto can_split = [&](const Node& nd) {  // before any histogram: rows, the depth limit
    return nd.end - nd.begin >= 2 && (a.max_depth == 0 || nd.depth < a.max_depth);
  };
  auto settle = [&](Node& nd) {  // the node's sums are known: its entry as a leaf
    a.value[nd.id] = nd.end > nd.begin ? core.value(nd) : 0.0;
    if (a.node_cover) a.node_cover[nd.id] = core.cover(nd);
  };
  std::vector<uint8_t> allow(a.ns ? a.f : 0);
  auto search = [&](Node& nd) {  // under a spec the node's mask row comes first: its draw is keyed by its id
    if (a.ns) mifx_ns_node_mask(*a.ns, a.f, (uint64_t)nd.id, nd.S.data(), a.feature_mask, allow.data());
    core.search(nd, a.ns ? allow.data() : nullptr);
  };
  nodes.reserve(2 * (size_t)a.max_leaves);  // (pointers into it stay valid)
  Node* root = add(0, (int)ns, 0);
  if (!root) return -1;
  if (a.ns) root->S.assign(mifx_ns_words(a.f), 0);
  core.start(*root);
  settle(*root);
  int leaves = 1;
  if (can_split(*root) && a.max_leaves >= 2) {
    core.build(*root);
    search(*root);
    if (!root->cand.leaf) open.push_back(0);
  }
  while (leaves < a.max_leaves && !open.empty()) {
    size_t at = 0;  // open holds ascending ids: strict > keeps the lowest id among equal gains
    for (size_t i = 1; i < open.size(); ++i)
      if (nodes[open[i]].cand.gain > nodes[open[at]].cand.gain) at = i;
    Node& p = nodes[open[at]];
    open.erase(open.begin() + at);
    const LgCand c = p.cand;
    const int mid = (int)(std::stable_partition(rows.begin() + p.begin, rows.begin() + p.end,
                                                [&](int r) { return core.goes_left(c, r); }) - rows.begin());
    Node *L = add(p.begin, mid, p.depth + 1), *R = add(mid, p.end, p.depth + 1);
    if (!L || !R) return -1;
    ++leaves;
    a.feature[p.id] = c.feature;
    a.split_bin[p.id] = c.bin;
    a.default_left[p.id] = (uint8_t)c.default_left;
    a.left[p.id] = L->id;
    a.right[p.id] = R->id;
    a.value[p.id] = 0.0;
    if (a.node_gain) a.node_gain[p.id] = c.gain;
    core.children(p, *L, *R);
    if (a.ns) L->S = R->S = child_set(p.S, c.feature);
    settle(*L);
    settle(*R);
    // candidates only where a child can still be split (both children share the depth; the last split of the budget
    // needs none): smaller child built, larger = parent - smaller
    if ((a.max_depth == 0 || L->depth < a.max_depth) && leaves < a.max_leaves) {
      Node& small = (L->end - L->begin) <= (R->end - R->begin) ? *L : *R;
      Node& large = &small == L ? *R : *L;
      core.build(small);
      core.inherit(large, p, small);
      for (Node* ch : {L, R})
        if (can_split(*ch)) {
          search(*ch);
          if (!ch->cand.leaf) open.push_back(ch->id);
        }
      for (Node* ch : {L, R})
        if (ch->cand.leaf) core.release(*ch);  // closed: its histogram is never read again
    }
    core.release(p);
  }
  for (const Node& nd : nodes)
    if (a.feature[nd.id] < 0)
      for (int k = nd.begin; k < nd.end; ++k) a.leaf_of_row[rows[k]] = nd.id;
  return (int)nodes.size();
}

}  // namespace

extern "C" {

// Leaf-wise twins of mifx_gbdt_grow_stats / mifx_gbdt_grow_fixed_stats: the same arguments, and max_leaves (>= 1);
// max_depth 0 means no depth limit; the tree arrays hold max_nodes >= 2 * max_leaves - 1 entries; feature_mask
// (null = all): [f], the features the tree may split on. mifx_gbdt_grow_fixed_lossguide_stats is the host twin of
// the device grower in csrc/gbdt_lossguide.hip.
int mifx_gbdt_grow_lossguide_stats(const uint16_t* bins, long n, int f, const int* nbins, const float* g,
                                   const float* h, int max_depth, int max_leaves, double min_child_weight,
                                   double lambda, double gamma, double eta, int threads, int max_nodes, int* feature,
                                   int* split_bin, uint8_t* default_left, int* left, int* right, double* value,
                                   int* leaf_of_row, const int* sample, long n_rows, const uint8_t* feature_mask,
                                   double* node_gain, double* node_cover) {
  return grow_lossguide<DoubleCore>(LgArgs{bins, n, f, nbins, g, h, max_depth, max_leaves, min_child_weight, lambda,
                                           gamma, eta, threads, max_nodes, feature, split_bin, default_left, left,
                                           right, value, leaf_of_row, sample, n_rows, feature_mask, node_gain,
                                           node_cover});
}

int mifx_gbdt_grow_fixed_lossguide_stats(const uint16_t* bins, long n, int f, const int* nbins, const float* g,
                                         const float* h, int max_depth, int max_leaves, double min_child_weight,
                                         double lambda, double gamma, double eta, int threads, int max_nodes,
                                         int* feature, int* split_bin, uint8_t* default_left, int* left, int* right,
                                         double* value, int* leaf_of_row, const int* sample, long n_rows,
                                         const uint8_t* feature_mask, double* node_gain, double* node_cover) {
  return grow_lossguide<FixedCore>(LgArgs{bins, n, f, nbins, g, h, max_depth, max_leaves, min_child_weight, lambda,
                                          gamma, eta, threads, max_nodes, feature, split_bin, default_left, left,
                                          right, value, leaf_of_row, sample, n_rows, feature_mask, node_gain,
                                          node_cover});
}

// The two leaf-wise growers under monotone_constraints: the arguments above and mono [f] in {-1, 0, +1} (-3: anything
// else, or null). mifx_gbdt_grow_fixed_lossguide_mono is the host twin of mifx_gbdt_lg_grow_mono.
int mifx_gbdt_grow_lossguide_mono(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                                  int max_depth, int max_leaves, double min_child_weight, double lambda, double gamma,
                                  double eta, int threads, int max_nodes, int* feature, int* split_bin,
                                  uint8_t* default_left, int* left, int* right, double* value, int* leaf_of_row,
                                  const int* sample, long n_rows, const uint8_t* feature_mask, double* node_gain,
                                  double* node_cover, const int* mono) {
  if (!mono_ok(mono, f)) return -3;
  return grow_lossguide<DoubleCore>(LgArgs{bins, n, f, nbins, g, h, max_depth, max_leaves, min_child_weight, lambda,
                                           gamma, eta, threads, max_nodes, feature, split_bin, default_left, left,
                                           right, value, leaf_of_row, sample, n_rows, feature_mask, node_gain,
                                           node_cover, mono});
}

int mifx_gbdt_grow_fixed_lossguide_mono(const uint16_t* bins, long n, int f, const int* nbins, const float* g,
                                        const float* h, int max_depth, int max_leaves, double min_child_weight,
                                        double lambda, double gamma, double eta, int threads, int max_nodes,
                                        int* feature, int* split_bin, uint8_t* default_left, int* left, int* right,
                                        double* value, int* leaf_of_row, const int* sample, long n_rows,
                                        const uint8_t* feature_mask, double* node_gain, double* node_cover,
                                        const int* mono) {
  if (!mono_ok(mono, f)) return -3;
  return grow_lossguide<FixedCore>(LgArgs{bins, n, f, nbins, g, h, max_depth, max_leaves, min_child_weight, lambda,
                                          gamma, eta, threads, max_nodes, feature, split_bin, default_left, left,
                                          right, value, leaf_of_row, sample, n_rows, feature_mask, node_gain,
                                          node_cover, mono});
}

// The leaf-wise growers with per-node feature sets: mifx_gbdt_grow_nodeset's arguments with max_leaves after max_depth,
// feature_mask [f] in the level mask's place. fixed = 1 is the host twin of mifx_gbdt_lg_grow_nodeset.
int mifx_gbdt_grow_lossguide_nodeset(int fixed, const uint16_t* bins, long n, int f, const int* nbins, const float* g,
                                     const float* h, int max_depth, int max_leaves, double min_child_weight,
                                     double lambda, double gamma, double eta, int threads, int max_nodes, int* feature,
                                     int* split_bin, uint8_t* default_left, int* left, int* right, double* value,
                                     int* leaf_of_row, const int* sample, long n_rows, const uint8_t* feature_mask,
                                     double* node_gain, double* node_cover, const int* mono, const uint64_t* groups,
                                     int n_groups, double bynode, uint64_t seed, uint64_t round) {
  const MifxNsSpec ns{groups, groups ? n_groups : 0, bynode, seed, round};
  if ((mono && !mono_ok(mono, f)) || !nodeset_ok(ns, f)) return -3;
  const LgArgs a{bins, n, f, nbins, g, h, max_depth, max_leaves, min_child_weight, lambda, gamma, eta, threads, max_nodes,
                 feature, split_bin, default_left, left, right, value, leaf_of_row, sample, n_rows, feature_mask,
                 node_gain, node_cover, mono, &ns};
  return fixed ? grow_lossguide<FixedCore>(a) : grow_lossguide<DoubleCore>(a);
}

// Sum of the first n_trees trees' outputs for each row of a row-major [n, f] matrix of raw values. Trees are
// concatenated: tree t's nodes are [tree_off[t], tree_off[t + 1]) with child indices local to the tree; thr is
// the split's cut value (go left iff x < thr, NaN follows default_left).
int mifx_gbdt_predict(const double* X, long n, int f, int n_trees, const int* tree_off, const int* feature,
                      const double* thr, const uint8_t* default_left, const int* left, const int* right,
                      const double* value, double base, double* out, int threads) {
  const int chunks = n > 4096 ? std::max(1, threads) : 1;
  parallel_for(chunks, chunks, [&](int c) {
    const long lo = n * c / chunks, hi = n * (c + 1) / chunks;
    for (long i = lo; i < hi; ++i) {
      const double* xi = X + (size_t)i * f;
      double s = base;
      for (int t = 0; t < n_trees; ++t) {
        const int o = tree_off[t];
        int k = 0;
        while (feature[o + k] >= 0) {
          const double a = xi[feature[o + k]];
          const bool l = std::isnan(a) ? default_left[o + k] != 0 : a < thr[o + k];
          k = l ? left[o + k] : right[o + k];
        }
        s += value[o + k];
      }
      out[i] = s;
    }
  });
  return 0;
}

// ---- feature contributions (path-dependent TreeSHAP in path form, gbdt_shap.h)

// The path table of a forest (trees concatenated as for mifx_gbdt_predict, tree_off [n_trees + 1]; cover: the nodes'
// hessian sums). recs == null counts only. info [3] receives the records, the leaves and, on an error, the tree.
// leaf_off [leaves + 1]: record offset of every leaf's header; tree_leaf [n_trees + 1]: first leaf of every tree.
// Everything the walkers trust is checked here: -1 a tree that is not one (an empty tree, a child outside
// (node, count), a node with two parents or none), -2 a feature outside [0, nfeat), -3 an inner node or a child of
// one whose cover is not finite and > 0 (UNWIND divides by the ratios), -4 a path with more than MIFX_SHAP_MAX_PATH
// distinct features, -5 an output too small or 2^31 records, -6 a NaN threshold.
int mifx_gbdt_paths_build(int n_trees, const int* tree_off, const int* feature, const double* thr,
                          const uint8_t* default_left, const int* left, const int* right, const double* value,
                          const double* cover, int nfeat, MifxShapRec* recs, long rec_cap, int* leaf_off, long leaf_cap,
                          int* tree_leaf, long* info) {
  long n_recs = 0, n_leaves = 0;
  info[0] = info[1] = 0;
  info[2] = -1;
  if (n_trees < 0 || nfeat < 1) return -1;
  std::vector<int> parent, path;
  auto good = [](double c) { return c > 0.0 && c <= 1.7976931348623157e308; };
  for (int t = 0; t < n_trees; ++t) {
    info[2] = t;
    const int o = tree_off[t], c = tree_off[t + 1] - o;
    if (o < 0 || c < 1) return -1;
    const int *fe = feature + o, *le = left + o, *ri = right + o;
    const double *th = thr + o, *cv = cover + o, *val = value + o;
    const uint8_t* dl = default_left + o;
    parent.assign(c, -1);
    for (int k = 0; k < c; ++k) {
      if (fe[k] < 0) continue;
      if (fe[k] >= nfeat) return -2;
      const int l = le[k], r = ri[k];
      if (l <= k || l >= c || r <= k || r >= c || l == r || parent[l] >= 0 || parent[r] >= 0) return -1;
      if (th[k] != th[k]) return -6;
      if (!good(cv[k]) || !good(cv[l]) || !good(cv[r])) return -3;
      parent[l] = parent[r] = k;
    }
    for (int k = 1; k < c; ++k)
      if (parent[k] < 0) return -1;
    if (recs) tree_leaf[t] = (int)n_leaves;
    for (int k = 0; k < c; ++k) {
      if (fe[k] >= 0) continue;
      path.clear();
      for (int a = k; a >= 0; a = parent[a]) path.push_back(a);  // parents have smaller indices: it ends at the root
      MifxShapRec el[MIFX_SHAP_MAX_PATH];
      int m = 0;
      for (size_t s = path.size() - 1; s > 0; --s) {
        const int p = path[s], ch = path[s - 1];
        int e = 0;
        while (e < m && el[e].i != fe[p]) ++e;
        if (e == m) {
          if (m == MIFX_SHAP_MAX_PATH) return -4;
          el[m++] = MifxShapRec{1.0, -INFINITY, 0.0, fe[p], MIFX_SHAP_NAN_OK};
        }
        el[e].a = el[e].a * (cv[ch] / cv[p]);
        if (ch == le[p]) {
          el[e].c = (el[e].j & MIFX_SHAP_HAS_HI) && el[e].c < th[p] ? el[e].c : th[p];
          el[e].j |= MIFX_SHAP_HAS_HI;
          if (!dl[p]) el[e].j &= ~MIFX_SHAP_NAN_OK;
        } else {
          if (th[p] > el[e].b) el[e].b = th[p];
          if (dl[p]) el[e].j &= ~MIFX_SHAP_NAN_OK;
        }
      }
      if (n_recs + 1 + m >= (1L << 31)) return -5;
      if (recs) {
        if (n_recs + 1 + m > rec_cap || n_leaves + 1 > leaf_cap) return -5;
        double pz = 1.0;
        for (int e = 0; e < m; ++e) pz = pz * el[e].a;
        leaf_off[n_leaves] = (int)n_recs;
        recs[n_recs] = MifxShapRec{val[k], m ? val[k] * pz : val[k], 0.0, m, 0};
        for (int e = 0; e < m; ++e) recs[n_recs + 1 + e] = el[e];
      }
      n_recs += 1 + m;
      n_leaves += 1;
    }
  }
  if (recs) {
    tree_leaf[n_trees] = (int)n_leaves;
    leaf_off[n_leaves] = (int)n_recs;
  }
  info[0] = n_recs;
  info[1] = n_leaves;
  info[2] = -1;
  return 0;
}

// is recs[0, n_recs) whole leaves of at most MIFX_SHAP_MAX_PATH elements with features in [0, f)
static bool shap_table_fits(const MifxShapRec* recs, long n_recs, int f) {
  for (long pos = 0; pos < n_recs;) {
    const int m = recs[pos].i;
    if (m < 0 || m > MIFX_SHAP_MAX_PATH || pos + 1 + m > n_recs) return false;
    for (int e = 0; e < m; ++e)
      if (recs[pos + 1 + e].i < 0 || recs[pos + 1 + e].i >= f) return false;
    pos += 1 + m;
  }
  return true;
}

// one row's contributions phi[0 .. f) and bias phi[f], the table walked in order; obits (or null) receives every
// leaf's o bits
static void shap_contribs_row(const double* xi, int f, const MifxShapRec* recs, long n_recs, double base, double* phi,
                              uint16_t* leaf_obits) {
  for (int j = 0; j < f; ++j) phi[j] = 0.0;
  double bias = base;
  for (long pos = 0; pos < n_recs;) {
    const MifxShapRec& hd = recs[pos];
    const int m = hd.i;
    bias += hd.b;
    unsigned obits = 0;
    if (m > 0) {
      const MifxShapRec* e = recs + pos + 1;
      for (int k = 0; k < m; ++k) obits |= (unsigned)mifx_shap_passes(e[k], xi[e[k].i]) << k;
      mifx_shap_leaf_m(m, e, obits, hd.a, [&](int j, double x) { phi[j] += x; });
    }
    if (leaf_obits) *leaf_obits++ = (uint16_t)obits;
    pos += 1 + m;
  }
  phi[f] = bias;
}

// Contributions of the leaves in recs[0, n_recs) (a prefix of a path table that ends at a leaf boundary) for every
// row of a row-major [n, f] table: out[i * stride + j] for j < f is feature j's contribution, out[i * stride + f]
// the bias, base plus every leaf's share. One accumulator row per data row, the table walked in order, so the result
// does not depend on the thread count. -1: a table that is not one for f features (checked before any row).
int mifx_gbdt_contribs(const double* X, long n, int f, const MifxShapRec* recs, long n_recs, double base, double* out,
                       long stride, int threads) {
  if (n < 0 || f < 1 || n_recs < 0 || stride < f + 1) return -1;
  if (!shap_table_fits(recs, n_recs, f)) return -1;
  const int chunks = n > 64 ? (int)std::min<long>(std::max(1, threads), n) : 1;
  parallel_for(chunks, chunks, [&](int c) {
    const long lo = n * c / chunks, hi = n * (c + 1) / chunks;
    for (long i = lo; i < hi; ++i)
      shap_contribs_row(X + (size_t)i * f, f, recs, n_recs, base, out + (size_t)i * stride, nullptr);
  });
  return 0;
}

// Interaction values (XGBoost's pred_interactions) of the first n_leaves leaves of a path table for every row of a
// row-major [n, f] table: out[r * stride + i * (f + 1) + j] is Phi[i][j] of row r, an (f + 1) x (f + 1) matrix.
// leaf_off [n_leaves + 1]: the leaves' record offsets. feat_off [f + 1], feat_leaf, feat_pos: per feature the
// ascending leaves whose path holds it and its element index there (mifx/gbdt/shap.py builds them); entries of
// leaves >= n_leaves end a list. Cell (i, j), i != j < f, sums mifx_shap_leaf_skip's shares over feature i's
// leaves in that order from 0; the diagonal is mifx_shap_diagonal of the row's contribution (the arithmetic of
// mifx_gbdt_contribs); row and column f are zero but for the bias in (f, f). One matrix per data row and thread, so
// the result does not depend on the thread count. -1: a table or an index that does not fit (checked before any row).
int mifx_gbdt_interactions(const double* X, long n, int f, const MifxShapRec* recs, const int* leaf_off, int n_leaves,
                           const int* feat_off, const int* feat_leaf, const int* feat_pos, double base, double* out,
                           long stride, int threads) {
  if (n < 0 || f < 1 || n_leaves < 0 || stride < (long)(f + 1) * (f + 1) || leaf_off[0] != 0) return -1;
  for (int l = 0; l < n_leaves; ++l)  // leaf_off is the walk of the headers
    if (leaf_off[l + 1] <= leaf_off[l] || recs[leaf_off[l]].i != leaf_off[l + 1] - leaf_off[l] - 1) return -1;
  const long n_recs = leaf_off[n_leaves];
  if (!shap_table_fits(recs, n_recs, f)) return -1;
  std::vector<int> feat_end(f);  // the end of every list under this leaf limit
  for (int i = 0; i < f; ++i) {
    if (feat_off[i] < 0 || feat_off[i + 1] < feat_off[i]) return -1;
    int q = feat_off[i], last = -1;
    for (; q < feat_off[i + 1] && feat_leaf[q] < n_leaves; ++q) {
      const int l = feat_leaf[q], c = feat_pos[q];
      if (l <= last || c < 0 || c >= recs[leaf_off[l]].i || recs[leaf_off[l] + 1 + c].i != i) return -1;
      last = l;
    }
    feat_end[i] = q;
  }
  const int w = f + 1;
  const int chunks = (int)std::max<long>(1, std::min<long>(threads, n));
  parallel_for(chunks, chunks, [&](int t) {
    const long lo = n * t / chunks, hi = n * (t + 1) / chunks;
    std::vector<double> phi(w);
    std::vector<uint16_t> obits(std::max(1, n_leaves));  // every leaf's o bits of the row, taken once
    for (long r = lo; r < hi; ++r) {
      double* M = out + (size_t)r * stride;
      shap_contribs_row(X + (size_t)r * f, f, recs, n_recs, base, phi.data(), obits.data());
      for (int i = 0; i < f; ++i) {
        double* row = M + (size_t)i * w;
        for (int j = 0; j < w; ++j) row[j] = 0.0;
        for (int q = feat_off[i]; q < feat_end[i]; ++q) {
          const MifxShapRec* hd = recs + leaf_off[feat_leaf[q]];
          mifx_shap_leaf_skip_m(hd->i, hd + 1, feat_pos[q], obits[feat_leaf[q]], hd->a,
                                [&](int j, double x) { row[j] += x; });
        }
        row[i] = mifx_shap_diagonal(phi[i], f, i, [&](int j) { return row[j]; });
      }
      for (int j = 0; j < f; ++j) M[(size_t)f * w + j] = 0.0;
      M[(size_t)f * w + f] = phi[f];
    }
  });
  return 0;
}

}  // extern "C"
