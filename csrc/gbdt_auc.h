// The pair count of mifx.gbdt's eval_metric="auc": ONE copy of its rule, included by the host function (csrc/gbdt.cpp,
// mifx_gbdt_auc) and by the device kernels (csrc/gbdt_auc.hip).
//
// Unweighted binary AUC over m rows, P of them positive and N negative. Margins are compared numerically as doubles, so
// -0.0 == +0.0 is a tie. A positive with margin v scores twice the negatives below it plus the negatives equal to it:
//   U2 = sum over positives i of (2 * #{neg j : m_j < m_i} + #{neg j : m_j == m_i}),
// an int64 with U2 <= 2 P N < 2^62 for m < 2^31. With lower(v) = #{neg < v} and upper(v) = #{neg <= v} over the sorted
// negatives, a positive's term is 2 * lower + (upper - lower) = lower + upper. Counts add over disjoint pieces of the
// negatives, so the term may be taken piece by piece (the device's LDS chunks) and the sum over positives in any order
// (integer adds): U2 is a pure function of the data. The score, U2 / (2 P N) correctly rounded, is formed by one Python
// function from the integers (mifx.gbdt.xgb.auc_score) for both learners, so equal integers give equal bits.
// Margins are finite: a NaN compares false with everything and the counts then mean nothing (the host refuses it).
#pragma once

#if defined(__HIPCC__)
#define MIFX_AUC_HD __host__ __device__ __forceinline__
#else
#define MIFX_AUC_HD inline
#endif

// #{a[i] < v} over the ascending a[0 .. n)
MIFX_AUC_HD long mifx_auc_lower(const double* a, long n, double v) {
  long lo = 0, hi = n;
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// #{a[i] <= v} over the ascending a[0 .. n), given `from` <= that count with a[0 .. from) <= v (0 is always valid)
MIFX_AUC_HD long mifx_auc_upper(const double* a, long n, double v, long from) {
  long lo = from, hi = n;
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// one positive's term over a piece of the negatives: 2 * lower + (upper - lower)
MIFX_AUC_HD long long mifx_auc_term(long lower, long upper) { return (long long)lower + (long long)upper; }

// U2 of ascending positives against ascending negatives by one merge walk (the host's route): both bounds only move up
inline long long mifx_auc_merge(const double* neg, long N, const double* pos, long P) {
  long long u2 = 0;
  long lower = 0, upper = 0;
  for (long i = 0; i < P; ++i) {
    while (lower < N && neg[lower] < pos[i]) ++lower;
    if (upper < lower) upper = lower;
    while (upper < N && neg[upper] <= pos[i]) ++upper;
    u2 += mifx_auc_term(lower, upper);
  }
  return u2;
}
