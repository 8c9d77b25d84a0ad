// Host sanitizer harness for the sampled tree growers (mifx_gbdt_grow_ex / mifx_gbdt_grow_fixed_ex in csrc/gbdt.cpp:
// a row list and a per-level feature mask; the draws of csrc/gbdt_sample.h). A stand-alone program, built twice by
// tests/test_gbdt_sample_cpu.py: AddressSanitizer + UBSan, and ThreadSanitizer (features are split over std::threads
// when sampled rows * f > 200k).
//
// Per trial: random bins as in gbdt_fixed_fuzz.cpp, a row list drawn by the rule itself at a random rate (so empty and
// single-row lists occur; the first trials force them), a random level mask (colsample_bytree x colsample_bylevel).
// Asserted: the trees grown with 1, 2, 3 and 8 threads are the SAME bit for bit (fixed point on any gradients, the
// double learner too: its sums are in row order per feature); leaf_of_row is -1 exactly off the list and a node id on
// it; every split feature lies inside its level's mask; an empty list gives one node of value +0.0. Exact-size heap
// buffers everywhere, so any over-read / over-write is an ASan report.
//   g++ -O1 -g -fsanitize=address,undefined -std=c++17 -pthread tools/sanitize/gbdt_sample_fuzz.cpp csrc/gbdt.cpp
//   g++ -O1 -g -fsanitize=thread -std=c++17 -pthread tools/sanitize/gbdt_sample_fuzz.cpp csrc/gbdt.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

extern "C" {
int mifx_gbdt_grow_ex(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                      int max_depth, double min_child_weight, double lambda, double gamma, double eta, int threads,
                      int max_nodes, int* feature, int* split_bin, uint8_t* default_left, int* left, int* right,
                      double* value, int* leaf_of_row, const int* sample, long n_rows, const uint8_t* level_mask);
int mifx_gbdt_grow_fixed_ex(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                            int max_depth, double min_child_weight, double lambda, double gamma, double eta,
                            int threads, int max_nodes, int* feature, int* split_bin, uint8_t* default_left, int* left,
                            int* right, double* value, int* leaf_of_row, const int* sample, long n_rows,
                            const uint8_t* level_mask);
long mifx_gbdt_sample_rows(uint64_t seed, uint64_t round, double subsample, long n, uint8_t* keep);
int mifx_gbdt_level_mask(uint64_t seed, uint64_t round, int f, int max_depth, double colsample_bytree,
                         double colsample_bylevel, uint8_t* tree_set, uint8_t* mask);
}

struct Tree {
  std::vector<int> feature, split_bin, left, right, leaf;
  std::vector<uint8_t> dl;
  std::vector<double> value;
  int count = 0;
};

struct Case {
  long n;
  int f, depth;
  double mcw, gamma;
  std::vector<uint16_t> bins;
  std::vector<int> nbins, rows;
  std::vector<float> g, h;
  std::vector<uint8_t> keep, mask;  // keep [n]; mask [depth, f] (empty: none)
  bool use_rows, use_mask;
};

static Tree grow(const Case& c, bool fixed, int threads) {
  const int max_nodes = (1 << (c.depth + 1)) - 1;
  Tree t;
  t.feature.resize(max_nodes);
  t.split_bin.resize(max_nodes);
  t.left.resize(max_nodes);
  t.right.resize(max_nodes);
  t.dl.resize(max_nodes);
  t.value.resize(max_nodes);
  t.leaf.assign(c.n, -7);
  // an exact-size copy of the list (an empty one is a valid non-null pointer to nothing)
  std::vector<int> rows(c.rows);
  static int nothing;
  const int* rp = c.use_rows ? (rows.empty() ? &nothing : rows.data()) : nullptr;
  t.count = (fixed ? mifx_gbdt_grow_fixed_ex : mifx_gbdt_grow_ex)(
      c.bins.data(), c.n, c.f, c.nbins.data(), c.g.data(), c.h.data(), c.depth, c.mcw, 1.0, c.gamma, 0.3, threads,
      max_nodes, t.feature.data(), t.split_bin.data(), t.dl.data(), t.left.data(), t.right.data(), t.value.data(),
      t.leaf.data(), rp, (long)rows.size(), c.use_mask && c.depth > 0 ? c.mask.data() : nullptr);
  return t;
}

static bool same(const Tree& a, const Tree& b, long n) {
  if (a.count != b.count || a.count <= 0) return false;
  for (int k = 0; k < a.count; ++k)
    if (a.feature[k] != b.feature[k] || a.split_bin[k] != b.split_bin[k] || a.left[k] != b.left[k] ||
        a.right[k] != b.right[k] || a.dl[k] != b.dl[k] || std::memcmp(&a.value[k], &b.value[k], sizeof(double)))
      return false;
  for (long i = 0; i < n; ++i)
    if (a.leaf[i] != b.leaf[i]) return false;
  return true;
}

// leaf_of_row and the masks of one grown tree; returns the number of violated properties
static int check(const Case& c, const Tree& t, int trial, const char* which) {
  int bad = 0;
  for (long i = 0; i < c.n; ++i) {
    const bool in = !c.use_rows || c.keep[i];
    const int l = t.leaf[i];
    if (in ? (l < 0 || l >= t.count || t.feature[l] >= 0) : l != -1) {
      if (!bad)
        std::printf("trial %d %s: leaf_of_row[%ld] = %d (row %s the list)\n", trial, which, i, l, in ? "on" : "off");
      ++bad;
    }
  }
  std::vector<int> depth(t.count, 0);
  for (int k = 0; k < t.count; ++k) {
    if (t.feature[k] < 0) continue;
    if (t.left[k] <= k || t.left[k] >= t.count || t.right[k] <= k || t.right[k] >= t.count) {
      std::printf("trial %d %s: node %d has children out of range\n", trial, which, k);
      return bad + 1;
    }
    depth[t.left[k]] = depth[t.right[k]] = depth[k] + 1;
    if (t.feature[k] >= c.f || depth[k] >= c.depth ||
        (c.use_mask && !c.mask[(size_t)depth[k] * c.f + t.feature[k]])) {
      std::printf("trial %d %s: node %d (depth %d) splits on feature %d outside its level's mask\n", trial, which, k,
                  depth[k], t.feature[k]);
      ++bad;
    }
  }
  if (c.use_rows && c.rows.empty() && (t.count != 1 || t.value[0] != 0.0 || std::signbit(t.value[0]))) {
    std::printf("trial %d %s: an empty sample must give one node of value +0.0\n", trial, which);
    ++bad;
  }
  return bad;
}

int main() {
  std::mt19937_64 rng(20261021);
  int failures = 0, trees = 0, empty = 0, single = 0;
  const int kinds[5] = {5, 256, 1, 2, 64};
  const double mcws[3] = {0.0, 1.0, 5.0};
  const double rates[5] = {1.0, 0.8, 0.5, 0.1, 0.01};
  for (int trial = 0; trial < 36; ++trial) {
    const bool big = trial % 12 == 5;  // sampled rows * f > 200000: features over threads
    Case c;
    c.n = trial < 4 ? 1 + trial : big ? 24000 + (long)(rng() % 4000) : 1 + (long)(rng() % 3000);
    c.f = big ? 10 + (int)(rng() % 3) : 1 + (int)(rng() % 12);
    c.depth = (int)(rng() % 7);
    c.mcw = mcws[rng() % 3];
    c.gamma = rng() % 2 ? 0.25 : 0.0;
    c.bins.resize((size_t)c.n * c.f);
    c.nbins.resize(c.f);
    for (int j = 0; j < c.f; ++j) {
      const bool all_missing = c.f >= 3 && j == c.f - 1;
      const int nb = all_missing ? 1 : kinds[(j + trial) % 5];
      c.nbins[j] = nb;
      for (long i = 0; i < c.n; ++i)
        c.bins[(size_t)j * c.n + i] = all_missing || rng() % 10 == 0 ? 0xFFFF : (uint16_t)(rng() % nb);
    }
    c.g.resize(c.n);
    c.h.resize(c.n);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::uniform_real_distribution<float> ud(0.1f, 1.f);
    const float scale = trial % 8 == 3 ? 1e30f : trial % 8 == 7 ? 1e-30f : 1.f;
    for (long i = 0; i < c.n; ++i) {
      c.g[i] = nd(rng) * scale;
      c.h[i] = ud(rng) * scale;
    }
    // rows: the rule's own draw; trials 0-3 (n = 1..4) at a rate that leaves them empty or nearly so
    c.use_rows = trial % 7 != 6;
    const double sub = big ? 0.9 : trial < 4 ? 0.3 : rates[rng() % 5];
    c.keep.resize(c.n);
    const long ns = mifx_gbdt_sample_rows(rng(), (uint64_t)trial, sub, c.n, c.keep.data());
    for (long i = 0; i < c.n; ++i)
      if (c.keep[i]) c.rows.push_back((int)i);
    if ((long)c.rows.size() != ns) {
      std::printf("trial %d: mifx_gbdt_sample_rows counted %ld of %zu rows\n", trial, ns, c.rows.size());
      ++failures;
    }
    if (c.use_rows) empty += c.rows.empty(), single += c.rows.size() == 1;
    c.use_mask = trial % 5 != 4;
    c.mask.resize((size_t)c.depth * c.f);
    std::vector<uint8_t> tree_set(c.f);
    if (mifx_gbdt_level_mask(rng(), (uint64_t)trial, c.f, c.depth, rates[rng() % 4], rates[rng() % 4], tree_set.data(),
                             c.mask.data()) != 0)
      ++failures;

    for (int fixed = 0; fixed < 2; ++fixed) {
      const char* which = fixed ? "fixed" : "double";
      const Tree t1 = grow(c, fixed != 0, 1);
      ++trees;
      if (t1.count <= 0) {
        std::printf("trial %d %s: grow failed: %d\n", trial, which, t1.count);
        ++failures;
        continue;
      }
      failures += check(c, t1, trial, which) != 0;
      for (int th : {2, 3, 8}) {
        ++trees;
        if (!same(t1, grow(c, fixed != 0, th), c.n)) {
          std::printf("trial %d %s: %d threads grew a different tree\n", trial, which, th);
          ++failures;
        }
      }
    }
  }
  // hand-made lists: empty and single-row, on a table of several rows
  for (int k = 0; k < 2; ++k) {
    Case c;
    c.n = 9, c.f = 2, c.depth = 3, c.mcw = 0.0, c.gamma = 0.0;
    c.bins.resize(18);
    c.nbins = {4, 4};
    for (auto& b : c.bins) b = (uint16_t)(rng() % 4);
    c.g.assign(9, 0.5f);
    c.h.assign(9, 1.f);
    c.keep.assign(9, 0);
    c.use_rows = true, c.use_mask = false;
    if (k == 1) c.rows = {4}, c.keep[4] = 1;
    empty += k == 0, single += k == 1;
    for (int fixed = 0; fixed < 2; ++fixed) {
      const Tree t = grow(c, fixed != 0, 2);
      ++trees;
      failures += t.count != 1 || check(c, t, 100 + k, fixed ? "fixed" : "double") != 0;
    }
  }
  if (!empty || !single) {
    std::printf("no empty (%d) or no single-row (%d) list was tried\n", empty, single);
    ++failures;
  }
  std::printf("%d trees, %d empty and %d single-row lists, %d failures\n", trees, empty, single, failures);
  return failures != 0;
}
