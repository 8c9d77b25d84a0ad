// The split rule of the fixed-point GBDT learners: ONE copy, included by the host twin (csrc/gbdt.cpp,
// mifx_gbdt_grow_fixed) and by the device learner (csrc/gbdt_gpu.hip).
//
// Fixed point: per tree and per quantity (g, h) one exponent e = 60 - bitlen(n) - (ilogb(amax) + 1), rows are
// q_i = llrint(ldexp(g_i, e)) (round half even), so |q_i| <= 2^(60 - bitlen(n)) and any subset of the n < 2^bitlen(n)
// rows sums to less than 2^61: histograms, node sums and prefix sums are int64 and therefore independent of the
// order of summation (threads, atomics, launch geometry, built versus subtracted child). Sums go back to double
// (ldexp(Q, -e)) only where csrc/gbdt.cpp's mifx_gbdt_grow evaluates doubles: the gain, the min_child_weight tests
// and the leaf value, with exactly its expressions and its tie rules:
//  * within a feature, candidates in (bin, direction) order, direction 0 (missing right) first, strict >; the
//    missing-left direction is skipped when no row of the node is missing in the feature;
//  * across features in feature order, a later feature wins only above best + 1e-12 |best|;
//  * a node is a leaf at gain <= 1e-6 (or without a candidate); leaf value -eta G / (H + lambda).
// Nothing here may be contracted into FMAs (the host build has no FMA ISA; the device build passes
// -ffp-contract=off and the pragma below says it again). No dependency on the build's force-included header.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MIFX_GB_HD __host__ __device__ __forceinline__
#else
#define MIFX_GB_HD inline
#endif

#ifdef __clang__
#pragma clang fp contract(off)
#endif

struct MifxGbParams {
  double lambda, gamma, min_child_weight, eta;
};

struct MifxGbSplit {
  double gain;
  int feature;  // -1: no candidate
  int bin;      // rows with bin <= this go left
  int default_left;
  long long gl, hl;  // quantised sums of the left child
  int cl;            // rows of the left child
};

MIFX_GB_HD MifxGbSplit mifx_gb_no_split() {
  MifxGbSplit s;
  s.gain = 0.0;
  s.feature = -1;
  s.bin = -1;
  s.default_left = 0;
  s.gl = s.hl = 0;
  s.cl = 0;
  return s;
}

// quantisation exponent for n rows whose largest magnitude is amax (0 for amax zero, infinite or NaN)
MIFX_GB_HD int mifx_gb_quant_exp(double amax, long long n) {
  if (!(amax > 0.0) || !(amax <= 1.7976931348623157e308)) return 0;
  int bitlen = 0;
  for (unsigned long long m = n > 0 ? (unsigned long long)n : 0ull; m; m >>= 1) ++bitlen;
  int ex;  // amax = m 2^ex with m in [0.5, 1): ex = ilogb(amax) + 1
  (void)frexp(amax, &ex);
  return 60 - bitlen - ex;
}

// one row's quantised value; a row that is not finite (or, with e = 0 after a non-finite amax, beyond int64) carries 0
MIFX_GB_HD long long mifx_gb_quantise(float v, int e) {
  const double s = ldexp((double)v, e);
  if (!(fabs(s) < 4611686018427387904.0)) return 0;  // 2^62
  return llrint(s);
}

MIFX_GB_HD double mifx_gb_dequant(long long q, int e) { return ldexp((double)q, -e); }

MIFX_GB_HD double mifx_gb_score(double G, double H, double lambda) { return G * G / (H + lambda); }

MIFX_GB_HD double mifx_gb_leaf_value(long long Qg, long long Qh, int eg, int eh, const MifxGbParams& p) {
  return -p.eta * mifx_gb_dequant(Qg, eg) / (mifx_gb_dequant(Qh, eh) + p.lambda);
}

MIFX_GB_HD double mifx_gb_parent_score(long long Qg, long long Qh, int eg, int eh, const MifxGbParams& p) {
  return mifx_gb_score(mifx_gb_dequant(Qg, eg), mifx_gb_dequant(Qh, eh), p.lambda);
}

// Candidates "cut after bin b" for b in [b0, b1) of one feature with nb bins (slot nb of hg / hh / hc is "missing"),
// in (bin, direction) order, folded into *bs with strict >. pg / ph / pc: sums of the bins below b0. The host scans
// [0, nb) in one call; the device gives each lane a run of bins and merges the lanes with mifx_gb_lower_wins.
MIFX_GB_HD void mifx_gb_scan(const long long* hg, const long long* hh, const int* hc, int nb, int b0, int b1,
                             long long pg, long long ph, int pc, long long Qg, long long Qh, int eg, int eh,
                             int feature, const MifxGbParams& p, double parent, MifxGbSplit* bs) {
  const long long mg = hg[nb], mh = hh[nb];
  const int mc = hc[nb];
  for (int b = b0; b < b1 && b + 1 < nb; ++b) {
    pg += hg[b];
    ph += hh[b];
    pc += hc[b];
    for (int dir = 0; dir < 2; ++dir) {  // dir 0: missing right, 1: missing left
      if (dir == 1 && mc == 0) break;
      const long long qgl = pg + (dir ? mg : 0), qhl = ph + (dir ? mh : 0);
      const double GL = mifx_gb_dequant(qgl, eg), HL = mifx_gb_dequant(qhl, eh);
      const double GR = mifx_gb_dequant(Qg - qgl, eg), HR = mifx_gb_dequant(Qh - qhl, eh);
      if (HL < p.min_child_weight || HR < p.min_child_weight) continue;
      const double gain = 0.5 * (mifx_gb_score(GL, HL, p.lambda) + mifx_gb_score(GR, HR, p.lambda) - parent) - p.gamma;
      if (gain > bs->gain) {
        bs->gain = gain;
        bs->feature = feature;
        bs->bin = b;
        bs->default_left = dir;
        bs->gl = qgl;
        bs->hl = qhl;
        bs->cl = pc + (dir ? mc : 0);
      }
    }
  }
}

// merging two partial scans of ONE feature: what a single in-order scan with strict > would have kept
MIFX_GB_HD bool mifx_gb_lower_wins(const MifxGbSplit& a, const MifxGbSplit& b) {  // true: keep a
  if (b.feature < 0) return true;
  if (a.feature < 0) return false;
  if (a.gain != b.gain) return a.gain > b.gain;
  return a.bin != b.bin ? a.bin < b.bin : a.default_left <= b.default_left;
}

// walking the features in order: does feature candidate c replace the best so far
MIFX_GB_HD bool mifx_gb_feature_wins(const MifxGbSplit& c, const MifxGbSplit& best) {
  return c.feature >= 0 && c.gain > best.gain + 1e-12 * fabs(best.gain);
}

MIFX_GB_HD bool mifx_gb_is_leaf(const MifxGbSplit& s) { return s.feature < 0 || s.gain <= 1e-6; }
