// Host sanitizer harness for feature contributions (mifx_gbdt_paths_build and mifx_gbdt_contribs in csrc/gbdt.cpp, the
// arithmetic of csrc/gbdt_shap.h). A stand-alone program, built by tests/test_gbdt_contribs_cpu.py under
// AddressSanitizer + UBSan.
//
// Per trial a random forest (random shapes up to depth 14, features repeated along paths, thresholds that include
// +-inf, random default directions, covers that are consistent sums of random leaf weights), then:
//   * the count pass and the fill pass agree; the table is well formed (every leaf 1 + m records, m <= 12, the z of a
//     leaf multiply to cover(leaf) / cover(root));
//   * contributions of random rows (NaN, +-inf) with 1 and 3 threads are the same bits, and every row sums to the
//     forest's prediction within 1e-12 * S;
//   * malformed forests (a child index out of range or not larger than its parent, a shared child, a feature out of
//     range, a zero / negative / NaN / infinite cover, a NaN threshold, an orphan node, an empty tree, a path with more
//     than 12 distinct features, outputs that are too small) are refused with the documented code, and a table with a
//     broken header or feature is refused by mifx_gbdt_contribs.
// Exact-size heap buffers everywhere, so any over-read / over-write is an ASan report.
//   g++ -O1 -g -fsanitize=address,undefined -std=c++17 -pthread tools/sanitize/gbdt_contribs_fuzz.cpp csrc/gbdt.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../csrc/gbdt_shap.h"

extern "C" {
int mifx_gbdt_paths_build(int n_trees, const int* tree_off, const int* feature, const double* thr,
                          const uint8_t* default_left, const int* left, const int* right, const double* value,
                          const double* cover, int nfeat, MifxShapRec* recs, long rec_cap, int* leaf_off, long leaf_cap,
                          int* tree_leaf, long* info);
int mifx_gbdt_contribs(const double* X, long n, int f, const MifxShapRec* recs, long n_recs, double base, double* out,
                       long stride, int threads);
int mifx_gbdt_predict(const double* X, long n, int f, int n_trees, const int* tree_off, const int* feature,
                      const double* thr, const uint8_t* default_left, const int* left, const int* right,
                      const double* value, double base, double* out, int threads);
}

struct Forest {
  int nfeat = 0;
  std::vector<int> off{0}, fe, le, ri;
  std::vector<double> thr, val, cov;
  std::vector<uint8_t> dl;
  int trees() const { return (int)off.size() - 1; }
};

static int failures = 0;
#define CHECK(c, ...)                        \
  do {                                       \
    if (!(c)) {                              \
      ++failures;                            \
      std::printf("FAIL %s: ", #c);          \
      std::printf(__VA_ARGS__);              \
      std::printf("\n");                     \
    }                                        \
  } while (0)

// breadth-first like the growers: children are appended, so they have larger indices than their parent
static void add_tree(Forest& F, std::mt19937_64& r, int max_depth, double p_split) {
  const int o = (int)F.fe.size();
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::normal_distribution<double> nrm;
  std::vector<int> depth{0};
  auto push = [&] {
    F.fe.push_back(-1), F.le.push_back(-1), F.ri.push_back(-1), F.dl.push_back(0);
    F.thr.push_back(0.0), F.val.push_back(nrm(r)), F.cov.push_back(0.0);
  };
  push();
  for (int k = 0; k < (int)depth.size(); ++k) {
    if (depth[k] >= max_depth || u(r) > p_split) continue;
    F.fe[o + k] = (int)(r() % F.nfeat);
    const double pick = u(r);
    F.thr[o + k] = pick < 0.03 ? INFINITY : pick < 0.06 ? -INFINITY : nrm(r);
    F.dl[o + k] = r() & 1;
    F.le[o + k] = (int)depth.size();
    F.ri[o + k] = (int)depth.size() + 1;
    for (int c = 0; c < 2; ++c) push(), depth.push_back(depth[k] + 1);
  }
  const int c = (int)depth.size();
  for (int k = c - 1; k >= 0; --k)  // covers: random leaf weights, summed upward
    F.cov[o + k] = F.fe[o + k] < 0 ? 0.25 + u(r) * 8 : F.cov[o + F.le[o + k]] + F.cov[o + F.ri[o + k]];
  F.off.push_back(o + c);
}

struct Table {
  int rc = 0;
  long info[3] = {0, 0, 0};
  std::vector<MifxShapRec> recs;
  std::vector<int> leaf_off, tree_leaf;
};

static Table build(const Forest& F, long shrink_recs = 0, long shrink_leaves = 0) {
  Table T;
  T.rc = mifx_gbdt_paths_build(F.trees(), F.off.data(), F.fe.data(), F.thr.data(), F.dl.data(), F.le.data(),
                               F.ri.data(), F.val.data(), F.cov.data(), F.nfeat, nullptr, 0, nullptr, 0, nullptr,
                               T.info);
  if (T.rc != 0) return T;
  const long nr = T.info[0] - shrink_recs, nl = T.info[1] - shrink_leaves;
  T.recs.resize(nr);  // exact sizes: one record or one leaf too many is an ASan report
  T.leaf_off.resize(nl + 1);
  T.tree_leaf.resize(F.trees() + 1);
  long info2[3];
  T.rc = mifx_gbdt_paths_build(F.trees(), F.off.data(), F.fe.data(), F.thr.data(), F.dl.data(), F.le.data(),
                               F.ri.data(), F.val.data(), F.cov.data(), F.nfeat, T.recs.data(), nr, T.leaf_off.data(),
                               nl, T.tree_leaf.data(), info2);
  if (T.rc == 0) CHECK(info2[0] == T.info[0] && info2[1] == T.info[1], "count and fill pass disagree");
  return T;
}

static int build_rc(const Forest& F) { return build(F).rc; }

int main() {
  std::mt19937_64 r(20240607);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::normal_distribution<double> nrm;
  int refused = 0, deep = 0;
  for (int trial = 0; trial < 160; ++trial) {
    Forest F;
    F.nfeat = 1 + (int)(r() % 9);
    const int trees = (int)(r() % 5);
    const int max_depth = trial % 4 == 0 ? 14 : 1 + (int)(r() % 7);
    for (int t = 0; t < trees; ++t)  // (deep trees stay thin: the harness runs under a sanitizer)
      add_tree(F, r, trial % 7 == 0 ? 0 : max_depth, trial % 4 == 0 ? 0.62 : 0.55 + 0.4 * u(r));
    Table T = build(F);
    CHECK(T.rc == 0, "trial %d: a valid forest refused (%d, tree %ld)", trial, T.rc, T.info[2]);
    if (T.rc != 0) continue;
    // the table's shape
    long pos = 0, leaves = 0;
    double S = 0;
    for (int t = 0; t < trees; ++t) {
      double big = 0;
      for (int k = F.off[t]; k < F.off[t + 1]; ++k)
        if (F.fe[k] < 0) big = std::fmax(big, std::fabs(F.val[k]));
      S += big;
    }
    while (pos < T.info[0]) {
      CHECK(T.leaf_off[leaves] == pos, "trial %d: leaf_off", trial);
      const int m = T.recs[pos].i;
      CHECK(m >= 0 && m <= MIFX_SHAP_MAX_PATH && pos + 1 + m <= T.info[0], "trial %d: header m = %d", trial, m);
      if (m >= 8) ++deep;
      pos += 1 + m;
      ++leaves;
    }
    CHECK(leaves == T.info[1] && T.leaf_off[leaves] == T.info[0] && T.tree_leaf[trees] == leaves, "trial %d: counts",
          trial);
    // rows
    const long n = 1 + (long)(r() % 150);
    const int f = F.nfeat;
    std::vector<double> X(n * f), a(n * (f + 1)), b(n * (f + 1)), pred(n);
    for (auto& x : X) {
      const double pick = u(r);
      x = pick < 0.1 ? NAN : pick < 0.13 ? INFINITY : pick < 0.16 ? -INFINITY : nrm(r);
    }
    const double base = nrm(r);
    const int used = trees ? (int)(r() % (trees + 1)) : 0;
    const long used_recs = T.leaf_off[T.tree_leaf[used]];
    CHECK(mifx_gbdt_contribs(X.data(), n, f, T.recs.data(), used_recs, base, a.data(), f + 1, 1) == 0, "contribs");
    CHECK(mifx_gbdt_contribs(X.data(), n, f, T.recs.data(), used_recs, base, b.data(), f + 1, 3) == 0, "contribs");
    CHECK(std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0, "trial %d: threads change the bits", trial);
    mifx_gbdt_predict(X.data(), n, f, used, F.off.data(), F.fe.data(), F.thr.data(), F.dl.data(), F.le.data(),
                      F.ri.data(), F.val.data(), base, pred.data(), 1);
    for (long i = 0; i < n; ++i) {
      double s = 0;
      for (int j = 0; j <= f; ++j) s += a[i * (f + 1) + j];
      CHECK(std::fabs(s - pred[i]) <= 1e-12 * (S + std::fabs(base)) + 1e-300, "trial %d row %ld: sum %.17g margin %.17g",
            trial, i, s, pred[i]);
    }
    if (!trees) continue;
    // malformed variants of this forest: each must be refused with its code, none may read or write out of bounds
    const int t = (int)(r() % trees), o = F.off[t], c = F.off[t + 1] - o;
    int inner = -1;
    for (int k = 0; k < c && inner < 0; ++k)
      if (F.fe[o + k] >= 0) inner = o + k;
    auto expect = [&](Forest G, int code, const char* what) {
      const int rc = build_rc(G);
      CHECK(rc == code, "trial %d: %s gave %d, expected %d", trial, what, rc, code);
      ++refused;
    };
    if (T.info[0] > 0) {
      // (a table of one record has no shorter buffer: a null record pointer asks for the count pass)
      CHECK(T.info[0] == 1 || build(F, 1, 0).rc == -5, "trial %d: a record buffer one short", trial);
      CHECK(build(F, 0, 1).rc == -5, "trial %d: a leaf buffer one short", trial);
      std::vector<MifxShapRec> bad(T.recs.begin(), T.recs.begin() + used_recs);
      if (!bad.empty()) {
        bad[0].i = 13;
        CHECK(mifx_gbdt_contribs(X.data(), n, f, bad.data(), used_recs, base, a.data(), f + 1, 1) == -1, "m = 13");
        bad[0].i = (int)used_recs;  // a leaf that runs past the table
        CHECK(mifx_gbdt_contribs(X.data(), n, f, bad.data(), used_recs, base, a.data(), f + 1, 1) == -1, "long leaf");
        bad[0].i = T.recs[0].i;
        if (bad[0].i > 0) {
          bad[1].i = f;
          CHECK(mifx_gbdt_contribs(X.data(), n, f, bad.data(), used_recs, base, a.data(), f + 1, 1) == -1, "feature");
        }
      }
    }
    if (inner >= 0) {
      Forest G = F;
      G.le[inner] = c, expect(G, -1, "left child == count");
      G = F, G.ri[inner] = inner - o, expect(G, -1, "right child == node");
      G = F, G.le[inner] = -5, expect(G, -1, "negative child");
      G = F, G.le[inner] = G.ri[inner], expect(G, -1, "one child twice");
      G = F, G.fe[inner] = F.nfeat, expect(G, -2, "feature == nfeat");
      G = F, G.cov[inner] = 0.0, expect(G, -3, "zero cover");
      G = F, G.cov[o + F.le[inner]] = -1.0, expect(G, -3, "negative child cover");
      G = F, G.cov[o + F.ri[inner]] = NAN, expect(G, -3, "NaN child cover");
      G = F, G.cov[inner] = INFINITY, expect(G, -3, "infinite cover");
      G = F, G.thr[inner] = NAN, expect(G, -6, "NaN threshold");
      G = F, G.fe[inner] = -1, expect(G, -1, "orphans");  // its children lose their parent
    }
    {
      Forest G = F;  // an empty tree in the middle
      G.off.insert(G.off.begin() + t + 1, G.off[t + 1]);
      G.off[t + 1] = G.off[t];
      expect(G, -1, "empty tree");
    }
  }
  {  // a chain through 13 distinct features
    Forest G;
    G.nfeat = 13;
    for (int d = 0; d < 13; ++d) {
      G.fe.insert(G.fe.end(), {d, -1}), G.le.insert(G.le.end(), {2 * d + 2, -1}), G.ri.insert(G.ri.end(), {2 * d + 1, -1});
      G.dl.insert(G.dl.end(), {0, 0}), G.thr.insert(G.thr.end(), {0.0, 0.0}), G.val.insert(G.val.end(), {0.0, 1.0});
      G.cov.insert(G.cov.end(), {14.0 - d, 1.0});
    }
    G.fe.push_back(-1), G.le.push_back(-1), G.ri.push_back(-1), G.dl.push_back(0), G.thr.push_back(0.0);
    G.val.push_back(2.0), G.cov.push_back(1.0);
    G.off.push_back((int)G.fe.size());
    CHECK(build_rc(G) == -4, "13 distinct features on a path gave %d", build_rc(G));
    G.fe[24] = 0;  // the last split repeats feature 0: 12 distinct features, allowed
    CHECK(build_rc(G) == 0, "12 distinct features on a path gave %d", build_rc(G));
  }
  CHECK(refused > 500 && deep > 0, "the trials did not cover what they should (%d refusals, %d long paths)", refused,
        deep);
  std::printf("%d refusals checked, %d leaves with 8 or more elements\n%d failures\n", refused, deep, failures);
  return failures != 0;
}
