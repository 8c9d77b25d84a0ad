// Path-dependent TreeSHAP in path form: ONE copy of the per-(row, leaf) arithmetic, included by the host function
// (csrc/gbdt.cpp, mifx_gbdt_contribs) and by the device kernel (csrc/gbdt_prep.hip, k_contribs), which therefore
// agree bit for bit: + - * / and comparisons only, nothing contracted into FMAs.
//
// The path table (built once per model by mifx_gbdt_paths_build in gbdt.cpp) is a flat array of 32-byte records.
// Every leaf, trees in order and leaves in node order, is one header record followed by its m element records, one
// per DISTINCT feature on the root-to-leaf path, in the order the path first meets them:
//   header   a = leaf value v, b = v * (product of the elements' z) = the leaf's share of the bias, i = m
//   element  a = z, the product of cover(child) / cover(node) over the path's nodes of this feature (path order);
//            [b, c) = the interval of x that passes every test of this feature toward the leaf: b = the largest
//            threshold passed to the right (-inf: none), c = the smallest passed to the left (flag HAS_HI);
//            i = feature, j = flags (NAN_OK: every node of the feature on the path defaults toward the path)
// o(x) reproduces the walk of mifx_gbdt_predict: "left" is x < thr, "right" is !(x < thr) for a non-NaN x.
//
// Per (row, leaf): Lundberg's EXTEND over the m elements (after the root's dummy element z = o = 1) gives the m + 1
// permutation weights w; for element j UNWIND sums them without j, and phi[feature_j] += sum * (o_j - z_j) * v.
// Because o is 0 or 1, EXTEND needs no multiply by o and UNWIND divides only by z (once per element, as 1 / z).
// The weight array is indexed by compile-time constants only (M is a template argument and every loop unrolls), so
// on the device it lives in registers.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MIFX_SHAP_HD __host__ __device__ __forceinline__
#else
#define MIFX_SHAP_HD inline
#endif

#ifdef __clang__
#pragma clang fp contract(off)
#define MIFX_SHAP_UNROLL _Pragma("unroll")
#else
#define MIFX_SHAP_UNROLL _Pragma("GCC unroll 16")
#endif

#define MIFX_SHAP_MAX_PATH 12  // distinct features on one path
#define MIFX_SHAP_NAN_OK 1
#define MIFX_SHAP_HAS_HI 2

struct MifxShapRec {
  double a, b, c;
  int i, j;
};

// does x pass every test of element e toward the leaf
MIFX_SHAP_HD bool mifx_shap_passes(const MifxShapRec& e, double x) {
  if (x != x) return (e.j & MIFX_SHAP_NAN_OK) != 0;
  return !(x < e.b) && (!(e.j & MIFX_SHAP_HAS_HI) || x < e.c);
}

// One leaf with M elements e[0 .. M) for one row: bit k of obits is o of element k, v the leaf value.
// add(feature, x) receives the M contributions in element order.
template <int M, class Add>
MIFX_SHAP_HD void mifx_shap_leaf(const MifxShapRec* e, unsigned obits, double v, Add&& add) {
  double w[M + 1];
  w[0] = 1.0;
MIFX_SHAP_UNROLL
  for (int l = 1; l <= M; ++l) {  // EXTEND by element l - 1; the path then holds l + 1 elements
    const double z = e[l - 1].a;
    const bool o = (obits >> (l - 1)) & 1u;
    w[l] = 0.0;
MIFX_SHAP_UNROLL
    for (int i = l - 1; i >= 0; --i) {
      const double wi = w[i];
      if (o) w[i + 1] += wi * ((double)(i + 1) / (double)(l + 1));
      w[i] = (z * wi) * ((double)(l - i) / (double)(l + 1));
    }
  }
MIFX_SHAP_UNROLL
  for (int k = 0; k < M; ++k) {  // UNWIND element k: the sum of the weights of the path without it
    const double z = e[k].a;
    const bool o = (obits >> k) & 1u;
    double total = 0.0;
    if (o) {
      double next = w[M];
MIFX_SHAP_UNROLL
      for (int i = M - 1; i >= 0; --i) {
        const double t = next * ((double)(M + 1) / (double)(i + 1));
        total += t;
        next = w[i] - (t * z) * ((double)(M - i) / (double)(M + 1));
      }
    } else {
      const double rz = 1.0 / z;
MIFX_SHAP_UNROLL
      for (int i = M - 1; i >= 0; --i) total += (w[i] * rz) * ((double)(M + 1) / (double)(M - i));
    }
    add(e[k].i, (total * ((o ? 1.0 : 0.0) - z)) * v);
  }
}

// the same for a run-time m in [1, MIFX_SHAP_MAX_PATH] (uniform over a workgroup on the device: a scalar branch)
template <class Add>
MIFX_SHAP_HD void mifx_shap_leaf_m(int m, const MifxShapRec* e, unsigned obits, double v, Add&& add) {
  switch (m) {
    case 1: mifx_shap_leaf<1>(e, obits, v, add); break;
    case 2: mifx_shap_leaf<2>(e, obits, v, add); break;
    case 3: mifx_shap_leaf<3>(e, obits, v, add); break;
    case 4: mifx_shap_leaf<4>(e, obits, v, add); break;
    case 5: mifx_shap_leaf<5>(e, obits, v, add); break;
    case 6: mifx_shap_leaf<6>(e, obits, v, add); break;
    case 7: mifx_shap_leaf<7>(e, obits, v, add); break;
    case 8: mifx_shap_leaf<8>(e, obits, v, add); break;
    case 9: mifx_shap_leaf<9>(e, obits, v, add); break;
    case 10: mifx_shap_leaf<10>(e, obits, v, add); break;
    case 11: mifx_shap_leaf<11>(e, obits, v, add); break;
    case 12: mifx_shap_leaf<12>(e, obits, v, add); break;
    default: break;
  }
}
