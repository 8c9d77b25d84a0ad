// The per-node feature sets of the GBDT learners (interaction_constraints, colsample_bynode): ONE copy of the rule,
// included by the host learners (csrc/gbdt.cpp) and by both device growers (csrc/gbdt_gpu.hip,
// csrc/gbdt_lossguide.hip); mifx/gbdt/sample.py has the numpy twin of the draw.
//
// Every node has a path set S, the features its ancestors split on, kept as a bitset of words = ceil(f / 64) 64-bit
// words (feature j is bit j & 63 of word j >> 6); the root's is empty and both children of a split on j get S | {j}.
//  * interaction_constraints: groups [n_groups, words] bitsets. With S empty every feature is allowed, otherwise
//    A(S) = S | union of the groups g with S a subset of g. Without groups (null) every feature is allowed.
//  * colsample_bynode = rate < 1: from the node's level set (the tree's colsample_bytree set, narrowed by the level's
//    colsample_bylevel set depth-wise) the k = max(1, (int)(rate * len)) features with the smallest
//    (mix64(key + j * G), j), key = mifx_gs_key(seed, round, 2^32 + node), node the index in the tree arrays: the rule of
//    mifx_gs_choose at a site beyond every level's. The draw does not look at the constraints.
//  * a node may split on the drawn set intersected with A(S); an empty set makes it a leaf.
// A(S | {j}) is a subset of A(S) for every j in A(S), so a histogram built over A(S) serves every descendant; the drawn
// sets of a parent and its child are unrelated. The masks therefore hold two bits per (node, feature):
//   MIFX_NS_SPLIT  the node may split on the feature      (level set & drawn & A(S))
//   MIFX_NS_HIST   the node's histogram holds the feature (level set & A(S))
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gbdt_sample.h"

#define MIFX_NS_SITE_NODE0 4294967296ULL  // the draw of node k is keyed by site 2^32 + k
#define MIFX_NS_SPLIT 1
#define MIFX_NS_HIST 2

struct MifxNsSpec {
  const uint64_t* groups;  // [n_groups, words] (host learners: host memory, device growers: device memory), nullable
  int n_groups;
  double bynode;  // 1.0 skips the draw
  uint64_t seed, round;
};

MIFX_GS_HD int mifx_ns_words(int f) { return (f + 63) >> 6; }

// the host learners: out [f] receives the node's mask (the two bits above). S [words]; lset [f] (null = all features).
inline void mifx_ns_node_mask(const MifxNsSpec& ns, int f, uint64_t node, const uint64_t* S, const uint8_t* lset,
                              uint8_t* out) {
  const int words = mifx_ns_words(f);
  if (ns.bynode < 1.0) {
    mifx_gs_choose(mifx_gs_key(ns.seed, ns.round, MIFX_NS_SITE_NODE0 + node), ns.bynode, lset, f, out);
  } else {
    for (int j = 0; j < f; ++j) out[j] = 1;
  }
  bool empty = true;
  for (int w = 0; w < words; ++w) empty &= S[w] == 0;
  for (int j = 0; j < f; ++j) {
    bool adm = !lset || lset[j];
    if (adm && ns.groups && !empty) {
      adm = (S[j >> 6] >> (j & 63)) & 1;
      for (int g = 0; g < ns.n_groups && !adm; ++g) {
        const uint64_t* G = ns.groups + (size_t)g * words;
        if (!((G[j >> 6] >> (j & 63)) & 1)) continue;
        bool fits = true;
        for (int w = 0; w < words; ++w) fits &= (S[w] & ~G[w]) == 0;
        adm = fits;
      }
    }
    out[j] = adm ? (uint8_t)(MIFX_NS_HIST | (out[j] ? MIFX_NS_SPLIT : 0)) : 0;
  }
}

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace {

constexpr int kNsWaves = 4;          // waves (= nodes) per workgroup of the node-set kernels
constexpr int kNsMaxDrawFeat = 2048; // colsample_bynode < 1: kNsWaves images of f 8-byte hashes in 64 KB of LDS

// bytes of dynamic LDS of a node-set kernel with `waves` waves per workgroup
inline size_t ns_lds_bytes(const MifxNsSpec& ns, int f, int waves) {
  return ns.bynode < 1.0 ? (size_t)waves * f * sizeof(uint64_t) : 0;
}

// One wave makes the mask row of one node: out [f]. The lanes own features, lane l takes j = l, l + 64, ...
// S (null = empty, the root) [words]; lset (nullable) [f] the node's level set, its bit 0 counts; hash: the wave's own
// LDS image [f] (unused when the draw is off). Every argument but the lane is uniform over the wave.
//  (1) out[j] = MIFX_NS_HIST for the features of lset that S holds (all of lset when nothing constrains the node)
//  (2) per group: is S a subset of it? One pass over the words, lanes striding, folded by a wave vote -- the answer is
//      the wave's, held in a scalar; in a group that fits every lane then marks its own features
//  (3) the draw: every lane hashes its features into the LDS image; a feature's rank is the number of candidates before
//      it in (hash, index) order, counted 64 at a time: each lane loads one hash of the chunk, and the wave walks the
//      chunk's candidates by cross-lane reads. A feature is drawn iff its rank is < k.
__device__ __forceinline__ void nodeset_wave(const MifxNsSpec& ns, int f, int node, const uint64_t* S,
                                             const uint8_t* lset, uint8_t* out, volatile uint64_t* hash, int lane) {
  typedef unsigned long long u64;
  const int words = mifx_ns_words(f);
  bool nz = false;
  if (S && ns.groups)
    for (int w = lane; w < words; w += 64) nz |= S[w] != 0;
  const bool constrained = __any(nz);
  for (int j = lane; j < f; j += 64) {
    const bool in = !lset || (lset[j] & 1);
    out[j] = in && (!constrained || ((S[j >> 6] >> (j & 63)) & 1)) ? MIFX_NS_HIST : 0;
  }
  if (constrained)
    for (int g = 0; g < ns.n_groups; ++g) {
      const uint64_t* G = ns.groups + (size_t)g * words;
      bool inside = true;
      for (int w = lane; w < words; w += 64) inside &= (S[w] & ~G[w]) == 0;
      if (!__all(inside)) continue;  // uniform
      for (int j = lane; j < f; j += 64)
        if ((!lset || (lset[j] & 1)) && ((G[j >> 6] >> (j & 63)) & 1)) out[j] = MIFX_NS_HIST;
    }
  if (!(ns.bynode < 1.0)) {  // no draw: every feature the histogram holds may split
    for (int j = lane; j < f; j += 64)
      if (out[j]) out[j] = MIFX_NS_HIST | MIFX_NS_SPLIT;
    return;
  }
  const u64 key = mifx_gs_key(ns.seed, ns.round, MIFX_NS_SITE_NODE0 + (u64)node);
  int len = 0;
  for (int j0 = 0; j0 < f; j0 += 64) {  // j0 is uniform: every lane reaches the ballot
    const int j = j0 + lane;
    if (j < f) hash[j] = mifx_gs_mix64(key + (u64)j * MIFX_GS_GOLDEN);
    len += __popcll(__ballot(j < f && (!lset || (lset[j] & 1))));
  }
  int k = (int)(ns.bynode * len);
  if (k < 1) k = 1;
  __builtin_amdgcn_wave_barrier();  // the image is the wave's own: its writes are ordered before its reads
  for (int j0 = 0; j0 < f; j0 += 64) {
    const int j = j0 + lane;
    const u64 hj = j < f ? hash[j] : 0;
    int before = 0;
    for (int i0 = 0; i0 < f; i0 += 64) {
      const int i = i0 + lane;
      const u64 hi = i < f ? hash[i] : 0;
      const u64 cm = __ballot(i < f && (!lset || (lset[i] & 1)));  // the chunk's candidates
      for (int b = 0; b < 64; ++b) {
        if (!((cm >> b) & 1)) continue;  // uniform
        const u64 hb = (u64)__shfl((long long)hi, b);
        before += hb < hj || (hb == hj && i0 + b < j);
      }
    }
    if (j < f && out[j] && before < k) out[j] = MIFX_NS_HIST | MIFX_NS_SPLIT;
  }
}

}  // namespace
#endif
