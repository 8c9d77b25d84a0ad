// The leaf refresh of the absolute-error and quantile objectives of mifx.gbdt: ONE copy of its rule, included by the
// host function (csrc/gbdt.cpp, mifx_gbdt_leaf_refresh) and by the device kernels (csrc/gbdt_quantile.hip).
//
// After a tree is grown, every leaf's value becomes eta times the weighted lower alpha-quantile of the residuals
// r_i = y_i - margin_i (double, margins from BEFORE the tree) of the leaf's rows. The weights are integers: row i
// carries q_i = mifx_gb_quantise(h_i, eh), the fixed-point hessian of gbdt_split.h, with eh the exponent of the rows
// the tree was grown on (leaf_of_row >= 0): their largest |h| and their count. With Q the sum of a leaf's q_i and
// T = ceil(alpha * (double)Q) clamped to [1, Q], the quantile is the smallest residual r of the leaf with
// sum of q_i over r_i <= r  >=  T, in the order of gbdt_sort_key.h (numeric, -0.0 before +0.0). A leaf with Q = 0
// keeps the grower's value. Everything compared or summed is an integer, so the result depends on no order of
// evaluation: threads, launch geometry and atomics change no bit of it.
#pragma once
#include <stdint.h>

#include "gbdt_sort_key.h"
#include "gbdt_split.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

// the residual's radix key
MIFX_GB_HD uint64_t mifx_gq_key(double y, double margin) { return mifx_sort_key(y - margin); }

// the exponent of the integer weights: amax the largest |h| over the ns rows the tree was grown on
MIFX_GB_HD int mifx_gq_exp(double amax, long long ns) { return mifx_gb_quant_exp(amax, ns); }

MIFX_GB_HD long long mifx_gq_weight(float h, int eh) { return mifx_gb_quantise(h, eh); }

// the weight the selected residual's running sum must reach, for a leaf of total weight Q >= 1
MIFX_GB_HD long long mifx_gq_threshold(double alpha, long long Q) {
  const double t = ceil(alpha * (double)Q);
  if (!(t >= 1.0)) return 1;
  if (t >= (double)Q) return Q;  // (also where (double)Q rounded Q up)
  return (long long)t;
}

// the leaf value of a selected key: one double multiply
MIFX_GB_HD double mifx_gq_value(uint64_t key, double eta) { return eta * mifx_sort_value(key); }

// The gradient pair of the two objectives from d = margin - y (double). alpha < 0: reg:absoluteerror, the sign of d;
// else reg:quantileerror, (float)(1 - alpha) for d >= 0 and (float)(-alpha) below. The hessian is 1.0f in both.
MIFX_GB_HD float mifx_gq_grad(double margin, double y, double alpha) {
  const double d = margin - y;
  if (alpha < 0.0) return d > 0.0 ? 1.0f : d < 0.0 ? -1.0f : 0.0f;
  return d >= 0.0 ? (float)(1.0 - alpha) : (float)(-alpha);
}
