// Host sanitizer harness for the fixed-point twin of the tree learner (mifx_gbdt_grow_fixed in csrc/gbdt.cpp, the
// split rule of csrc/gbdt_split.h). A stand-alone program, built twice by tests/test_gbdt_fixed.py: AddressSanitizer +
// UBSan, and ThreadSanitizer (features are split over std::threads when n * f > 200k).
//
// Per trial: random bins (mixed bin counts, a constant feature, ~10 % missing, an all-missing column; n from 1 to
// ~3000, or 20k-40k rows x 10-12 features so the threaded paths run). On general float gradients the trees grown with
// 1, 2, 3 and 8 threads must be the SAME bit for bit; on dyadic gradients (g = k / 256, h = k / 64: every double sum
// and every quantisation exact) the twin must also grow exactly mifx_gbdt_grow's tree. Exact-size heap buffers
// everywhere, so any over-read / over-write is an ASan report; int64 overflow would be a UBSan report.
//   g++ -O1 -g -fsanitize=address,undefined -std=c++17 -pthread tools/sanitize/gbdt_fixed_fuzz.cpp csrc/gbdt.cpp
//   g++ -O1 -g -fsanitize=thread -std=c++17 -pthread tools/sanitize/gbdt_fixed_fuzz.cpp csrc/gbdt.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

extern "C" {
int mifx_gbdt_grow(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                   int max_depth, double min_child_weight, double lambda, double gamma, double eta, int threads,
                   int max_nodes, int* feature, int* split_bin, uint8_t* default_left, int* left, int* right,
                   double* value, int* leaf_of_row);
int mifx_gbdt_grow_fixed(const uint16_t* bins, long n, int f, const int* nbins, const float* g, const float* h,
                         int max_depth, double min_child_weight, double lambda, double gamma, double eta, int threads,
                         int max_nodes, int* feature, int* split_bin, uint8_t* default_left, int* left, int* right,
                         double* value, int* leaf_of_row);
int mifx_gbdt_quant_exp(double amax, long n);
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
  std::vector<int> nbins;
  std::vector<float> g, h;
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
  t.leaf.resize(c.n);
  t.count = (fixed ? mifx_gbdt_grow_fixed : mifx_gbdt_grow)(
      c.bins.data(), c.n, c.f, c.nbins.data(), c.g.data(), c.h.data(), c.depth, c.mcw, 1.0, c.gamma, 0.3, threads,
      max_nodes, t.feature.data(), t.split_bin.data(), t.dl.data(), t.left.data(), t.right.data(), t.value.data(),
      t.leaf.data());
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

int main() {
  std::mt19937_64 rng(20261020);
  int failures = 0, trees = 0;
  if (mifx_gbdt_quant_exp(0.0, 10) != 0 || mifx_gbdt_quant_exp(1.0, 1) != 58 || mifx_gbdt_quant_exp(4.0, 4096) != 44) {
    std::printf("quant_exp: wrong exponent\n");
    ++failures;
  }
  const int kinds[5] = {5, 256, 1, 2, 64};
  const double mcws[3] = {0.0, 1.0, 5.0};
  for (int trial = 0; trial < 48; ++trial) {
    const bool big = trial % 6 == 5;  // n * f > 200000: features over threads
    Case c;
    c.n = trial < 4 ? 1 + trial : big ? 20000 + (long)(rng() % 20000) : 1 + (long)(rng() % 3000);
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
    const bool dyadic = trial % 2 == 0;
    std::normal_distribution<float> nd(0.f, 1.f);
    std::uniform_real_distribution<float> ud(0.1f, 1.f);
    const float scale = trial % 8 == 3 ? 1e30f : trial % 8 == 7 ? 1e-30f : 1.f;
    for (long i = 0; i < c.n; ++i) {
      c.g[i] = dyadic ? (float)((long)(rng() % 2049) - 1024) / 256.f : nd(rng) * scale;
      c.h[i] = dyadic ? (float)(1 + rng() % 64) / 64.f : ud(rng) * scale;
    }
    const Tree t1 = grow(c, true, 1);
    ++trees;
    if (t1.count <= 0) {
      std::printf("trial %d: grow_fixed failed: %d\n", trial, t1.count);
      ++failures;
      continue;
    }
    for (int th : {2, 3, 8}) {
      ++trees;
      if (!same(t1, grow(c, true, th), c.n)) {
        std::printf("trial %d: %d threads grew a different tree\n", trial, th);
        ++failures;
      }
    }
    if (dyadic) {
      ++trees;
      if (!same(t1, grow(c, false, 4), c.n)) {
        std::printf("trial %d: the twin differs from mifx_gbdt_grow on dyadic gradients\n", trial);
        ++failures;
      }
    }
  }
  std::printf("%d trees, %d failures\n", trees, failures);
  return failures != 0;
}
