// The LambdaMART gradient pair of mifx.gbdt's XGBRanker (rank:pairwise, rank:ndcg): ONE copy of its rule, included by
// the host function (csrc/gbdt.cpp, mifx_gbdt_rank_grad) and by the device kernels (csrc/gbdt_rank.hip).
//
// The rows of a query group are contiguous (gptr[G + 1] are the row offsets). Inside a group the rows are ranked by
// margin, descending, on the order-preserving integer key of gbdt_sort_key.h (+0.0 above -0.0), ties to the lower row
// index; rank r is 0-based. Labels are integers in [0, 31], the gain of label l is 2^l - 1 (exact), the discount of
// rank r is D[r] = 1 / log2(r + 2), and P[r] = D[0] + ... + D[r - 1]; D and P are tables computed once by the host, so
// that host and device read the same bits. With c_l rows of label l and b_l rows of a label above l,
//   IDCG = sum over l = 31 ... 1 of gain(l) * (P[b_l + c_l] - P[b_l]), in that order, in double.
// A pair is (i, j) of one group with label_i > label_j; under "topk" (topk = k >= 1; 0 means every pair) only pairs
// with min(r_i, r_j) < k count. With s = m_i - m_j (higher label minus lower):
//   rho = 1 / (1 + exp(s)), delta = 1 (rank:pairwise) or |(gain_i - gain_j) * (D[r_i] - D[r_j])| / IDCG (rank:ndcg;
//   0 where IDCG is 0), lambda = rho * delta, eta = 2 * max(rho * (1 - rho), 1e-16) * delta;
//   row i takes g -= lambda, h += eta and row j takes g += lambda, h += eta.
// A row's g and h start from 0 and are summed in double over its partners in ascending partner rank, partners of equal
// label skipped, then cast to float32: a pure function of the group's data that no thread count or launch geometry
// can change. Only exp differs between a host and a device evaluation (a few double ulps per term), and with all
// margins equal exp(0) = 1 makes them agree bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gbdt_sort_key.h"
#include "gbdt_split.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

constexpr int kMifxRankLabels = 32;  // labels are 0 ... 31

// row a (key ka, index ia inside the group) ranks before row b
MIFX_GB_HD bool mifx_rk_before(uint64_t ka, int ia, uint64_t kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

MIFX_GB_HD double mifx_rk_gain(int label) { return (double)((1u << label) - 1u); }

// IDCG from the group's label counts cnt[32] and the prefix sums P
template <class Cnt>
MIFX_GB_HD double mifx_rk_idcg(const Cnt* cnt, const double* P) {
  double idcg = 0.0;
  int above = 0;
  for (int l = kMifxRankLabels - 1; l >= 1; --l) {
    const int c = (int)cnt[l];
    idcg += mifx_rk_gain(l) * (P[above + c] - P[above]);
    above += c;
  }
  return idcg;
}

// The partner ranks of a row at rank r in a group of m rows are 0 ... end - 1: under topk a row at or below rank k
// pairs only with the ranks above k.
MIFX_GB_HD int mifx_rk_partner_end(int r, int m, int topk) { return topk > 0 && r >= topk && topk < m ? topk : m; }

// One partner's term added to a row's sums. (m, l, d): margin, label and discount D[rank], of the row itself and of the
// partner; the labels differ and the pair counts. idcg is unused for rank:pairwise.
MIFX_GB_HD void mifx_rk_accum(bool ndcg, double idcg, double m_self, int l_self, double d_self, double m_other,
                              int l_other, double d_other, double* g, double* h) {
  const bool hi = l_self > l_other;
  const double s = hi ? m_self - m_other : m_other - m_self;
  const double rho = 1.0 / (1.0 + exp(s));
  double delta = 1.0;
  if (ndcg)
    delta = idcg > 0.0 ? fabs((mifx_rk_gain(l_self) - mifx_rk_gain(l_other)) * (d_self - d_other)) / idcg : 0.0;
  const double lambda = rho * delta;
  const double eta = 2.0 * fmax(rho * (1.0 - rho), 1e-16) * delta;
  *g = hi ? *g - lambda : *g + lambda;
  *h = *h + eta;
}
