// MIFX_HIPCC_FLAGS: -ffp-contract=off
// eval_metric="auc" of mifx.gbdt on the device: the exact integer pair counts of gbdt_auc.h from the eval set's
// margins, without reading them back. The wrapper (mifx/ops/gbdt_auc.py: AucPlan) runs, per group of G classes,
//
//   k_auc_fill    the class-major [K, m] float64 margins and the label bytes into a row-major [m, 2 G] table: column
//                 2 c is class c's margin where the row is a negative of that class, else NaN, column 2 c + 1 the same
//                 for its positives. A workgroup takes tiles of 128 rows x up to 16 classes: a wave reads 64 consecutive
//                 margins of one class (coalesced along the class's row), both columns go to LDS, and the tile is stored
//                 along the table's rows (a row's 2 G cells are contiguous). The first workgroup also clears the
//                 group's counters, so nothing needs a memset.
//   the batched radix sort of csrc/gbdt_sort.hip over all 2 G columns in the same launches, NaNs last: class c's N
//                 negatives ascend in the first N cells of row 2 c of its [2 G, m] result, its P positives in row 2 c + 1.
//   k_auc_count   one workgroup per (tile of sorted positives, class). The tile's first and last value bound a span of
//                 the sorted negatives by two binary searches in global memory: the `lo` negatives below the span are
//                 below every positive of the tile and count 2 each, arithmetically, without being read; those above it
//                 count nothing. A tile whose positives are all equal (the common case while the trees still give few
//                 distinct margins) is settled by the two searches alone: each positive scores lo + hi. Otherwise the
//                 span goes through LDS in chunks; every thread takes the tile's positives t, t + threads, ... and finds
//                 each one's lower and upper bound inside the chunk by binary search in LDS, adding
//                 2 * lower + (upper - lower). The partial sums are reduced over the wave with cross-lane adds, over the
//                 workgroup through LDS, and one 64-bit integer atomicAdd per workgroup goes to U2[class].
//
// There is no floating-point sum anywhere: values are only compared. An integer sum does not depend on its order, so
// the tile, the threads, the LDS chunk and the grouping of classes change no bit, and U2 equals the host's merge walk.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gbdt_auc.h"

namespace {

constexpr int kFillRows = 128;      // fill tile: 128 rows x 32 columns x 8 B = 32 KB of LDS (+ padding)
constexpr int kFillClasses = 16;
constexpr int kFillCols = 2 * kFillClasses;
constexpr int kFillBlocks = 2048;   // row workgroups of the fill pass (grid-stride over the row tiles)
constexpr int kThreads = 256;
constexpr int kMaxChunk = 4096;     // doubles of negatives staged at a time: 32 KB of LDS
constexpr int kMaxGroup = 32767;    // classes of one group: 2 G columns are the sort's grid dimension y

typedef unsigned long long u64;

// classes [c0, c0 + G) of margin [K, m]; label [m] holds the class index (K = 1: 0 / 1, positive = 1)
__global__ __launch_bounds__(kThreads) void k_auc_fill(const double* margin, const uint8_t* label, long m, int K,
                                                       int c0, int G, double* table, long long* u2) {
  __shared__ double tile[kFillRows * (kFillCols + 1)];
  const int t = threadIdx.x;
  const int g0 = blockIdx.y * kFillClasses;          // first class of this workgroup inside the group
  const int gw = min(kFillClasses, G - g0);
  if (blockIdx.x == 0)
    for (int c = t; c < gw; c += kThreads) u2[c0 + g0 + c] = 0;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  const long tiles = (m + kFillRows - 1) / kFillRows;
  for (long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const long r0 = tl * kFillRows;
    const int rows = (int)min((long)kFillRows, m - r0);
    __syncthreads();  // the previous tile has been stored
    for (int e = t; e < gw * kFillRows; e += kThreads) {  // a wave: 64 consecutive rows of one class
      const int c = e / kFillRows, r = e % kFillRows;
      if (r < rows) {
        const int cls = c0 + g0 + c;
        const double v = margin[(size_t)cls * m + r0 + r];
        const bool pos = label[r0 + r] == (K == 1 ? 1 : cls);
        tile[r * (kFillCols + 1) + 2 * c] = pos ? nan : v;
        tile[r * (kFillCols + 1) + 2 * c + 1] = pos ? v : nan;
      }
    }
    __syncthreads();
    const int cw = 2 * gw;
    for (int e = t; e < rows * cw; e += kThreads) {
      const int r = e / cw, c = e - r * cw;
      table[(size_t)(r0 + r) * (2 * G) + 2 * g0 + c] = tile[r * (kFillCols + 1) + c];
    }
  }
}

// sorted [2 G, m]: the sort's result for classes [c0, c0 + G); pn [K, 2]: (P, N) per class
__global__ void k_auc_count(const double* sorted, long m, int c0, const long long* pn, int tile, int chunk,
                            long long* u2) {
  extern __shared__ double s_neg[];
  __shared__ u64 s_part[kThreads / 64];
  const int t = threadIdx.x, c = blockIdx.y, cls = c0 + c;
  const long P = (long)pn[2 * cls], N = (long)pn[2 * cls + 1];
  const long p0 = (long)blockIdx.x * tile;
  if (p0 >= P || P > m || N > m) return;  // (uniform over the workgroup: no barrier is skipped by a part of it)
  const long p1 = min(P, p0 + tile);
  const double* neg = sorted + (size_t)(2 * c) * m;
  const double* pos = sorted + (size_t)(2 * c + 1) * m;
  const double first = pos[p0], last = pos[p1 - 1];
  const long lo = mifx_auc_lower(neg, N, first);
  const long hi = mifx_auc_upper(neg, N, last, lo);
  u64 acc = 0;
  if (first == last) {  // every positive of the tile sees the same bounds
    if (t == 0) acc = (u64)(p1 - p0) * (u64)mifx_auc_term(lo, hi);
  } else {
    if (t == 0) acc = (u64)(p1 - p0) * 2 * (u64)lo;  // the negatives below the span
    for (long s = lo; s < hi; s += chunk) {
      const int len = (int)min((long)chunk, hi - s);
      __syncthreads();  // the previous chunk has been searched
      for (int i = t; i < len; i += blockDim.x) s_neg[i] = neg[s + i];
      __syncthreads();
      for (long i = p0 + t; i < p1; i += blockDim.x) {
        const double v = pos[i];
        const long lower = mifx_auc_lower(s_neg, len, v);
        acc += (u64)mifx_auc_term(lower, mifx_auc_upper(s_neg, len, v, lower));
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((t & 63) == 0) s_part[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) acc += s_part[w];
    atomicAdd(reinterpret_cast<u64*>(u2) + cls, acc);
  }
}

}  // namespace

extern "C" {

int mifx_gbdt_auc_max_chunk() { return kMaxChunk; }
int mifx_gbdt_auc_max_threads() { return kThreads; }
int mifx_gbdt_auc_max_group() { return kMaxGroup; }

// table [m, 2 G] of classes [c0, c0 + G) from margin [K, m] and label [m]; clears u2[c0 .. c0 + G)
int mifx_gbdt_auc_fill(const double* margin, const uint8_t* label, long m, int K, int c0, int G, double* table,
                       long long* u2, hipStream_t stream) {
  if (m < 1 || m >= (1L << 31) || K < 1 || K > 256 || c0 < 0 || G < 1 || G > kMaxGroup || c0 + G > K) return -1;
  const long tiles = (m + kFillRows - 1) / kFillRows;
  const dim3 grid((unsigned)(tiles < kFillBlocks ? tiles : kFillBlocks), (unsigned)((G + kFillClasses - 1) / kFillClasses));
  k_auc_fill<<<grid, kThreads, 0, stream>>>(margin, label, m, K, c0, G, table, u2);
  return (int)hipGetLastError();
}

// adds the pair counts of classes [c0, c0 + G) to u2 from their sorted [2 G, m] columns; pn [K, 2] = (P, N) on the
// device, max_pos the largest P among the group's classes. Geometry: `tile` positives per workgroup, `threads` (a
// multiple of 64 up to 256), `chunk` negatives in LDS at a time (up to mifx_gbdt_auc_max_chunk()).
int mifx_gbdt_auc_count(const double* sorted, long m, int K, int c0, int G, const long long* pn, long max_pos, int tile,
                        int threads, int chunk, long long* u2, hipStream_t stream) {
  if (m < 1 || m >= (1L << 31) || c0 < 0 || G < 1 || G > kMaxGroup || c0 + G > K || max_pos < 1 || max_pos > m ||
      tile < 1 || threads < 64 || threads > kThreads || threads % 64 || chunk < 1 || chunk > kMaxChunk)
    return -1;
  const long tiles = (max_pos + tile - 1) / tile;
  if (tiles > 0x7FFFFFFFL) return -1;
  const dim3 grid((unsigned)tiles, (unsigned)G);
  k_auc_count<<<grid, threads, (size_t)chunk * sizeof(double), stream>>>(sorted, m, c0, pn, tile, chunk, u2);
  return (int)hipGetLastError();
}

}  // extern "C"
