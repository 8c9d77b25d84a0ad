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

// ---- monotone_constraints: the rule of the constrained growers, entered only when some feature's direction c_j is
// not 0 (so nothing here needs to equal the expressions above, and nothing above changes). Every node carries an
// interval [lo, hi] of weights (before eta), the root [-inf, +inf]:
//  * weight w(G, H) = -G / (H + lambda) clamped into the node's interval; leaf value eta * w;
//  * score with a weight: -(2 G w + (H + lambda) w w), for the parent and for both children;
//  * a candidate on a feature with c = +1 is dropped when wl > wr, with c = -1 when wl < wr;
//  * after a split on a feature with c != 0 and mid = 0.5 (wl + wr): c = +1 gives the left child [lo, mid] and the right
//    [mid, hi], c = -1 the other way round; c = 0 hands [lo, hi] to both.
// Candidate order, the strict >, the 1e-12 feature rule and the leaf test are the ones above. All of it takes doubles,
// so the double learner of gbdt.cpp calls the same functions as the fixed-point ones.
MIFX_GB_HD double mifx_gb_mono_weight(double G, double H, double lambda, double lo, double hi) {
  const double w = -G / (H + lambda);
  return w < lo ? lo : (w > hi ? hi : w);
}

MIFX_GB_HD double mifx_gb_mono_score(double G, double H, double lambda, double w) {
  return -(2.0 * G * w + (H + lambda) * w * w);
}

MIFX_GB_HD double mifx_gb_mono_parent(double G, double H, double lambda, double lo, double hi) {
  return mifx_gb_mono_score(G, H, lambda, mifx_gb_mono_weight(G, H, lambda, lo, hi));
}

// one candidate: false when the direction drops it, else its gain
MIFX_GB_HD bool mifx_gb_mono_gain(double GL, double HL, double GR, double HR, const MifxGbParams& p, double parent, int c,
                                  double lo, double hi, double* gain) {
  const double wl = mifx_gb_mono_weight(GL, HL, p.lambda, lo, hi), wr = mifx_gb_mono_weight(GR, HR, p.lambda, lo, hi);
  if ((c > 0 && wl > wr) || (c < 0 && wl < wr)) return false;
  *gain = 0.5 * (mifx_gb_mono_score(GL, HL, p.lambda, wl) + mifx_gb_mono_score(GR, HR, p.lambda, wr) - parent) - p.gamma;
  return true;
}

// the children's intervals after the chosen split: b = {left lo, left hi, right lo, right hi}
MIFX_GB_HD void mifx_gb_mono_children(double GL, double HL, double GR, double HR, double lambda, int c, double lo,
                                      double hi, double* b) {
  b[0] = b[2] = lo;
  b[1] = b[3] = hi;
  if (c == 0) return;
  const double wl = mifx_gb_mono_weight(GL, HL, lambda, lo, hi), wr = mifx_gb_mono_weight(GR, HR, lambda, lo, hi);
  const double mid = 0.5 * (wl + wr);
  if (c > 0) b[1] = b[2] = mid;
  else b[0] = b[3] = mid;
}

// the fixed-point forms: quantised sums in, the functions above on their doubles
MIFX_GB_HD double mifx_gb_mono_leaf_value(long long Qg, long long Qh, int eg, int eh, const MifxGbParams& p, double lo,
                                          double hi) {
  return p.eta * mifx_gb_mono_weight(mifx_gb_dequant(Qg, eg), mifx_gb_dequant(Qh, eh), p.lambda, lo, hi);
}

MIFX_GB_HD void mifx_gb_mono_children_q(const MifxGbSplit& s, long long Qg, long long Qh, int eg, int eh,
                                        const MifxGbParams& p, int c, double lo, double hi, double* b) {
  mifx_gb_mono_children(mifx_gb_dequant(s.gl, eg), mifx_gb_dequant(s.hl, eh), mifx_gb_dequant(Qg - s.gl, eg),
                        mifx_gb_dequant(Qh - s.hl, eh), p.lambda, c, lo, hi, b);
}

// mifx_gb_scan under a constraint: the same candidates in the same order; parent is mifx_gb_mono_parent of the node
MIFX_GB_HD void mifx_gb_scan_mono(const long long* hg, const long long* hh, const int* hc, int nb, int b0, int b1,
                                  long long pg, long long ph, int pc, long long Qg, long long Qh, int eg, int eh,
                                  int feature, const MifxGbParams& p, double parent, int c, double lo, double hi,
                                  MifxGbSplit* bs) {
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
      double gain;
      if (!mifx_gb_mono_gain(GL, HL, GR, HR, p, parent, c, lo, hi, &gain)) continue;
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
