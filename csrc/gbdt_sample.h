// The sampling rule of the GBDT learners (subsample, colsample_bytree, colsample_bylevel): ONE copy, included by the
// host learners (csrc/gbdt.cpp) and by the device learner (csrc/gbdt_gpu.hip); mifx/gbdt/sample.py is the numpy twin.
//
// Counter-based and integer-only, so a draw is a pure function of (random_state, round, site, index): independent of
// thread count, launch geometry and the order in which rows are visited, and equal on host and device.
//   G = 0x9E3779B97F4A7C15, mix64 = murmur3's fmix64 (the one of csrc/counter_rng.h)
//   key(seed, round, site) = mix64(seed ^ mix64(round * G + site))                     (uint64 wrap-around)
//  * rows (site 1): row i is in the round's sample iff (mix64(key + i * G) >> 32) < thr with
//    thr = (uint64)(subsample * 4294967296.0): the one floating-point product of the rule. thr = 2^32 keeps every
//    row, and callers do not hash at all then.
//  * features (site 2 per tree over all features; site 3 + d for level d over the tree's set): from the candidates c
//    the k = max(1, (int)(rate * len(c))) with the smallest (mix64(key + j * G), j), j the feature index. A rate of
//    1.0 skips the draw.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MIFX_GS_HD __host__ __device__ __forceinline__
#else
#define MIFX_GS_HD inline
#endif

#define MIFX_GS_GOLDEN 0x9E3779B97F4A7C15ULL
#define MIFX_GS_SITE_ROWS 1
#define MIFX_GS_SITE_TREE 2
#define MIFX_GS_SITE_LEVEL0 3
#define MIFX_GS_KEEP_ALL 4294967296ULL  // the row threshold of subsample = 1

MIFX_GS_HD uint64_t mifx_gs_mix64(uint64_t z) {
  z ^= z >> 33;
  z *= 0xff51afd7ed558ccdULL;
  z ^= z >> 33;
  z *= 0xc4ceb9fe1a85ec53ULL;
  z ^= z >> 33;
  return z;
}

MIFX_GS_HD uint64_t mifx_gs_key(uint64_t seed, uint64_t round, uint64_t site) {
  return mifx_gs_mix64(seed ^ mifx_gs_mix64(round * MIFX_GS_GOLDEN + site));
}

MIFX_GS_HD uint64_t mifx_gs_row_thr(double subsample) { return (uint64_t)(subsample * 4294967296.0); }

MIFX_GS_HD bool mifx_gs_keep_row(uint64_t key, uint64_t i, uint64_t thr) {
  return (mifx_gs_mix64(key + i * MIFX_GS_GOLDEN) >> 32) < thr;
}

// out[j] = 1 for the chosen features among the candidates (cand[j] != 0; cand null = all f), 0 elsewhere. A feature
// is chosen iff fewer than k candidates come before it in (hash, index) order: f is small, so no sort is needed.
// cand and out must not overlap (out is written while cand is read); returns k (0 without a candidate).
inline int mifx_gs_choose(uint64_t key, double rate, const uint8_t* cand, int f, uint8_t* out) {
  int len = 0;
  for (int j = 0; j < f; ++j) len += !cand || cand[j];
  int k = (int)(rate * len);
  if (k < 1) k = 1;
  if (k > len) k = len;
  for (int j = 0; j < f; ++j) {
    out[j] = 0;
    if (cand && !cand[j]) continue;
    const uint64_t hj = mifx_gs_mix64(key + (uint64_t)j * MIFX_GS_GOLDEN);
    int before = 0;
    for (int i = 0; i < f; ++i) {
      if (i == j || (cand && !cand[i])) continue;
      const uint64_t hi = mifx_gs_mix64(key + (uint64_t)i * MIFX_GS_GOLDEN);
      before += hi < hj || (hi == hj && i < j);
    }
    out[j] = before < k;
  }
  return k;
}

// The [max_depth, f] mask of one round: row d holds the features that level d may split on. tree_set [f] receives
// the tree's own set (the candidates of every level).
inline void mifx_gs_level_mask(uint64_t seed, uint64_t round, int f, int max_depth, double bytree, double bylevel,
                               uint8_t* tree_set, uint8_t* mask) {
  if (bytree < 1.0) {
    mifx_gs_choose(mifx_gs_key(seed, round, MIFX_GS_SITE_TREE), bytree, nullptr, f, tree_set);
  } else {
    for (int j = 0; j < f; ++j) tree_set[j] = 1;
  }
  for (int d = 0; d < max_depth; ++d) {
    uint8_t* row = mask + (size_t)d * f;
    if (bylevel < 1.0) {
      mifx_gs_choose(mifx_gs_key(seed, round, MIFX_GS_SITE_LEVEL0 + (uint64_t)d), bylevel, tree_set, f, row);
    } else {
      for (int j = 0; j < f; ++j) row[j] = tree_set[j];
    }
  }
}
