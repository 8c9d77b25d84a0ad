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
// Stochastic boosting (the *_ex entries): a tree is grown on a list of sampled rows as if the table held only them,
// and a [max_depth, f] mask names the features each level may split on; the draws themselves are gbdt_sample.h's.
//
// Node statistics (the *_stats entries): every grower can also record each node's gain and cover (hessian sum), which
// feature importances and feature contributions need. mifx_gbdt_paths_build turns a forest with covers into the path
// table of gbdt_shap.h and mifx_gbdt_contribs evaluates path-dependent TreeSHAP from it (the device twin is k_contribs
// in gbdt_prep.hip).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

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
int mifx_gbdt_grow_stats(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                         int max_depth, double min_child_weight, double lambda, double gamma, double eta, int threads,
                         int max_nodes, int* feature, int* split_bin, uint8_t* default_left, int* left, int* right,
                         double* value, int* leaf_of_row, const int* sample, long n_rows, const uint8_t* level_mask,
                         double* node_gain, double* node_cover) {
  if (!rows_ok(sample, n_rows, n)) return -2;
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
    const double parent = score(nd.g, nd.h);
    parallel_for(f, th, [&](int j) {
      const Hist* hj = nd.hist.data() + off[j];
      const int nb = level_mask && !level_mask[(size_t)nd.depth * f + j] ? 1 : nbins[j];
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
          const double gain = 0.5 * (score(GL, HL) + score(GR, HR) - parent) - gamma;
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
  Node root{0, (int)ns, 0, new_node(), 0.0, 0.0, {}};
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
    value[nd.id] = -eta * nd.g / (nd.h + lambda);
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
      Node L{nd.begin, mid, nd.depth + 1, li, s.gl, s.hl, {}};
      Node R{mid, nd.end, nd.depth + 1, ri, s.gr, s.hr, {}};
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
int mifx_gbdt_grow_fixed_stats(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                               int max_depth, double min_child_weight, double lambda, double gamma, double eta,
                               int threads, int max_nodes, int* feature, int* split_bin, uint8_t* default_left,
                               int* left, int* right, double* value, int* leaf_of_row, const int* sample, long n_rows,
                               const uint8_t* level_mask, double* node_gain, double* node_cover) {
  if (!rows_ok(sample, n_rows, n)) return -2;
  struct QNode {
    int begin, end, depth, id;
    long long g, h;
    std::vector<long long> hg, hh;  // [features][nbins + 1], the last slot is "missing"
    std::vector<int> hc;            // rows per slot
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
    const double parent = mifx_gb_parent_score(nd.g, nd.h, eg, eh, prm);
    parallel_for(f, th, [&](int j) {
      MifxGbSplit bs = mifx_gb_no_split();
      if (!level_mask || level_mask[(size_t)nd.depth * f + j])
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
  QNode root{0, (int)ns, 0, new_node(), 0, 0, {}, {}, {}};
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
        value[nd.id] = mifx_gb_leaf_value(nd.g, nd.h, eg, eh, prm);
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
      QNode L{nd.begin, mid, nd.depth + 1, li, s.gl, s.hl, {}, {}, {}};
      QNode R{mid, nd.end, nd.depth + 1, ri, nd.g - s.gl, nd.h - s.hl, {}, {}, {}};
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

// Contributions of the leaves in recs[0, n_recs) (a prefix of a path table that ends at a leaf boundary) for every
// row of a row-major [n, f] table: out[i * stride + j] for j < f is feature j's contribution, out[i * stride + f]
// the bias, base plus every leaf's share. One accumulator row per data row, the table walked in order, so the result
// does not depend on the thread count. -1: a table that is not one for f features (checked before any row).
int mifx_gbdt_contribs(const double* X, long n, int f, const MifxShapRec* recs, long n_recs, double base, double* out,
                       long stride, int threads) {
  if (n < 0 || f < 1 || n_recs < 0 || stride < f + 1) return -1;
  for (long pos = 0; pos < n_recs;) {
    const int m = recs[pos].i;
    if (m < 0 || m > MIFX_SHAP_MAX_PATH || pos + 1 + m > n_recs) return -1;
    for (int e = 0; e < m; ++e)
      if (recs[pos + 1 + e].i < 0 || recs[pos + 1 + e].i >= f) return -1;
    pos += 1 + m;
  }
  const int chunks = n > 64 ? (int)std::min<long>(std::max(1, threads), n) : 1;
  parallel_for(chunks, chunks, [&](int c) {
    const long lo = n * c / chunks, hi = n * (c + 1) / chunks;
    for (long i = lo; i < hi; ++i) {
      const double* xi = X + (size_t)i * f;
      double* phi = out + (size_t)i * stride;
      for (int j = 0; j < f; ++j) phi[j] = 0.0;
      double bias = base;
      for (long pos = 0; pos < n_recs;) {
        const MifxShapRec& hd = recs[pos];
        const int m = hd.i;
        bias += hd.b;
        if (m > 0) {
          const MifxShapRec* e = recs + pos + 1;
          unsigned obits = 0;
          for (int k = 0; k < m; ++k) obits |= (unsigned)mifx_shap_passes(e[k], xi[e[k].i]) << k;
          mifx_shap_leaf_m(m, e, obits, hd.a, [&](int j, double x) { phi[j] += x; });
        }
        pos += 1 + m;
      }
      phi[f] = bias;
    }
  });
  return 0;
}

}  // extern "C"
