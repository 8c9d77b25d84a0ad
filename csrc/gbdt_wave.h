// The wave-level pieces of the constrained split kernels (k_split_mono of csrc/gbdt_gpu.hip and of
// csrc/gbdt_lossguide.hip): ONE copy. A wave searches one feature of one node: lane l owns the run of bins
// [4 l, 4 l + 4), the runs' integer sums are prefix-scanned across the wave, every lane folds its own candidates with
// mifx_gb_scan_mono, and the lanes' partial results merge with mifx_gb_lower_wins (ties to the lowest (bin, direction):
// what one in-order scan keeps).
#pragma once
#include <hip/hip_runtime.h>

#include "gbdt_split.h"

namespace {

constexpr int kRun = 4;  // bins per lane: 64 lanes x 4 = the 256 bins of a feature

// g0 / h0 / c0: one feature's histogram of nb <= 256 bins (global or LDS). The best candidate of the whole feature under
// direction c and the node's interval [lo, hi], in every lane. Uniform arguments but for the lane.
__device__ __forceinline__ MifxGbSplit wave_search_mono(const long long* g0, const long long* h0, const int* c0, int nb,
                                                        int lane, long long Qg, long long Qh, int eg, int eh, int j,
                                                        const MifxGbParams& prm, int c, double lo, double hi) {
  const int b0 = lane * kRun;
  long long lg = 0, lh = 0;
  int lc = 0;
  for (int b = b0; b < b0 + kRun && b < nb; ++b) {
    lg += g0[b];
    lh += h0[b];
    lc += c0[b];
  }
  long long ig = lg, ih = lh;  // inclusive prefix over the lanes
  int ic = lc;
  for (int s = 1; s < 64; s <<= 1) {
    const long long tg = __shfl_up(ig, s), th = __shfl_up(ih, s);
    const int tc = __shfl_up(ic, s);
    if (lane >= s) {
      ig += tg;
      ih += th;
      ic += tc;
    }
  }
  // the parent's clamped weight and score are the wave's, not the candidate's: once, outside the lanes' loops
  const double parent = mifx_gb_mono_parent(mifx_gb_dequant(Qg, eg), mifx_gb_dequant(Qh, eh), prm.lambda, lo, hi);
  MifxGbSplit bs = mifx_gb_no_split();
  mifx_gb_scan_mono(g0, h0, c0, nb, b0, b0 + kRun, ig - lg, ih - lh, ic - lc, Qg, Qh, eg, eh, j, prm, parent, c, lo, hi,
                    &bs);
  for (int s = 32; s; s >>= 1) {
    MifxGbSplit ot;
    ot.gain = __shfl_xor(bs.gain, s);
    ot.feature = __shfl_xor(bs.feature, s);
    ot.bin = __shfl_xor(bs.bin, s);
    ot.default_left = __shfl_xor(bs.default_left, s);
    ot.gl = __shfl_xor(bs.gl, s);
    ot.hl = __shfl_xor(bs.hl, s);
    ot.cl = __shfl_xor(bs.cl, s);
    if (!mifx_gb_lower_wins(bs, ot)) bs = ot;
  }
  return bs;
}

}  // namespace
