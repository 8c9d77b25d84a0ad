// Interaction values of mifx.gbdt on the device (XGBoost's pred_interactions, path-dependent, margin space): per
// row an (f + 1) x (f + 1) matrix Phi, bit for bit the host's mifx_gbdt_interactions (gbdt.cpp) whatever the launch
// geometry. gbdt_shap.h holds the one copy of the per-leaf arithmetic (mifx_shap_leaf_skip).
// MIFX_HIPCC_FLAGS: -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops
//
// Work split. The grid is (row tiles) x (f + 1 matrix rows) and one thread owns one output row Phi[row][i][0 .. f]:
// f + 1 contiguous doubles, the accumulator shape of k_contribs (gbdt_prep.hip), and f + 1 times its workgroups,
// which is what a table of 10^4 rows needs to fill the device. Matrix row i < f is one conditioned pass: feature i
// is taken off every path that holds it, so only those leaves matter, and the workgroup walks feature i's leaf list
// (mifx/gbdt/shap.py: PathTable.feature_leaves) instead of the table.
//
// Staging. The list is walked in chunks of whole leaves. The workgroup gathers a chunk's leaves from the path table
// into LDS, packed one after the other, one thread per (list entry, record slot); the header's unused field j takes
// the entry's element index c. Every lane is then at the same leaf at the same time: m, c, every z and every feature
// index are uniform (m and c are made scalars, so the dispatch on m is a scalar branch; the records are LDS
// broadcasts) and only the o bits and the permutation weights differ per lane. The weights are registers:
// mifx_shap_leaf_at<M> indexes them by constants, c only addresses the records.
//
// Accumulators: the two routes of k_contribs and its LDS budget.
//   ACC_LDS   cell j of thread t is lds[j * blockDim.x + t] (consecutive lanes, consecutive words), stored once; the
//             workgroup is 256, 128 or 64 threads, the largest whose f sums per thread fit beside the chunk
//   otherwise the thread's own output row (plain loads and stores: no other thread touches it)
// A cell adds its leaves' shares in list order from 0 on either route, as the host does.
//
// Epilogue. phi[row][i] comes from a [n, f + 1] contributions buffer that k_contribs filled on the same stream; the
// diagonal is mifx_shap_diagonal over the row's cells, column f is 0. The workgroups of matrix row f write zeros and
// the bias. A feature with an empty list goes straight to the epilogue. No atomics, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gbdt_shap.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSlots = 1 + MIFX_SHAP_MAX_PATH;  // records of the largest leaf: the smallest chunk
constexpr int kMaxLds = 65536;                  // mifx_gbdt_prep_contrib_max_lds: the chunk and the LDS sums

template <class T, bool ACC_LDS>
__global__ __launch_bounds__(kThreads) void k_interactions(const T* X, long n, int f, const MifxShapRec* recs,
                                                           const int* leaf_off, int n_leaves, const int* feat_off,
                                                           const int* feat_leaf, const int* feat_pos,
                                                           const int* feat_rec, const double* phi, long phi_stride,
                                                           int chunk, double* out, long stride) {
  extern __shared__ double lds_raw[];
  MifxShapRec* lds = reinterpret_cast<MifxShapRec*>(lds_raw);
  double* acc = lds_raw + (size_t)chunk * (sizeof(MifxShapRec) / sizeof(double)) + threadIdx.x;
  const int nt = blockDim.x, i = blockIdx.y, w = f + 1;
  const long r = (long)blockIdx.x * nt + threadIdx.x;
  const bool live = r < n;  // a thread past the table only helps staging: it never touches out
  double* row = out + (size_t)(live ? r : 0) * stride + (size_t)i * w;
  if (i == f) {  // the bias row
    if (live) {
      for (int j = 0; j < f; ++j) row[j] = 0.0;
      row[f] = phi[(size_t)r * phi_stride + f];
    }
    return;
  }
  const T* xi = X + (size_t)(live ? r : 0) * f;
  if (ACC_LDS) {
    for (int j = 0; j < f; ++j) acc[(size_t)j * nt] = 0.0;
  } else if (live) {
    for (int j = 0; j < f; ++j) row[j] = 0.0;
  }
  // feature i's entries of leaves below n_leaves: [q0, qe). Everything that steers the loops is uniform.
  int q0 = feat_off[i], qe = feat_off[i + 1];
  for (int lo = q0; lo < qe;) {
    const int mid = (lo + qe) >> 1;
    if (feat_leaf[mid] < n_leaves) lo = mid + 1; else qe = mid;
  }
  while (q0 < qe) {
    const int r0 = feat_rec[q0];
    int lo = q0 + 1, hi = qe;  // the last entry boundary within a chunk of r0; q0 + 1 always is (chunk >= kSlots)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (feat_rec[mid] - r0 <= chunk) lo = mid; else hi = mid - 1;
    }
    const int total = min(feat_rec[lo] - r0, chunk);
    __syncthreads();  // the previous chunk has been walked
    for (int s = threadIdx.x; s < (lo - q0) * kSlots; s += nt) {
      const int q = q0 + s / kSlots, k = s % kSlots;
      const int at = feat_rec[q] - r0;
      if (k < feat_rec[q + 1] - feat_rec[q] && at + k < total) {
        MifxShapRec rec = recs[leaf_off[feat_leaf[q]] + k];
        if (k == 0) rec.j = feat_pos[q];
        lds[at + k] = rec;
      }
    }
    __syncthreads();
    if (live) {
      int pos = 0;
      while (pos < total) {
        const int m = __builtin_amdgcn_readfirstlane(lds[pos].i), c = __builtin_amdgcn_readfirstlane(lds[pos].j);
        if (m < 1 || m > MIFX_SHAP_MAX_PATH || c < 0 || c >= m || pos + 1 + m > total) break;  // refused on the host
        const MifxShapRec* e = lds + pos + 1;
        unsigned obits = 0;
        for (int k = 0; k < m; ++k) {
          const int j = min(max(e[k].i, 0), f - 1);
          obits |= (unsigned)mifx_shap_passes(e[k], (double)xi[j]) << k;
        }
        const double v = lds[pos].a;
        if (ACC_LDS)
          mifx_shap_leaf_skip_m(m, e, c, obits, v, [&](int j, double x) {
            if ((unsigned)j < (unsigned)f) acc[(size_t)j * nt] += x;
          });
        else
          mifx_shap_leaf_skip_m(m, e, c, obits, v, [&](int j, double x) {
            if ((unsigned)j < (unsigned)f) row[j] += x;
          });
        pos += 1 + m;
      }
    }
    q0 = lo;
  }
  if (!live) return;
  const double phi_i = phi[(size_t)r * phi_stride + i];
  if (ACC_LDS) {
    for (int j = 0; j < f; ++j) row[j] = acc[(size_t)j * nt];
    row[i] = mifx_shap_diagonal(phi_i, f, i, [&](int j) { return acc[(size_t)j * nt]; });
  } else {
    row[i] = mifx_shap_diagonal(phi_i, f, i, [&](int j) { return row[j]; });
  }
  row[f] = 0.0;
}

}  // namespace

extern "C" {

int mifx_gbdt_interactions_min_chunk() { return kSlots; }
int mifx_gbdt_interactions_max_lds() { return kMaxLds; }

// Interaction values of the first n_leaves leaves of a path table (validated on the host) for a row-major [n, f]
// table: out[r * stride + i * (f + 1) + j] = Phi[i][j] of row r, the bits of the host's mifx_gbdt_interactions.
// recs, leaf_off and the per-feature lists feat_off [f + 1], feat_leaf, feat_pos, feat_rec [entries + 1] (the running
// record count of the listed leaves) are on the device. phi [n, >= f + 1] with row stride phi_stride: the rows'
// contributions and bias for the same leaves, complete on `stream` before this launch. chunk, threads, acc_lds:
// as for mifx_gbdt_prep_contribs; none changes a bit of the result.
int mifx_gbdt_interactions_launch(const void* X, int is_f64, long n, int f, const void* recs, const int* leaf_off,
                                  int n_leaves, const int* feat_off, const int* feat_leaf, const int* feat_pos,
                                  const int* feat_rec, const double* phi, long phi_stride, int chunk, int threads,
                                  int acc_lds, double* out, long stride, hipStream_t stream) {
  if (n < 1 || n >= (1L << 31) || f < 1 || f >= 65535 || n_leaves < 0 || chunk < kSlots || phi_stride < f + 1 ||
      stride < (long)(f + 1) * (f + 1) || acc_lds < 0 || acc_lds > 1 ||
      (threads != 64 && threads != 128 && threads != kThreads))
    return -1;
  const size_t lds = (size_t)chunk * sizeof(MifxShapRec) + (acc_lds ? (size_t)f * threads * sizeof(double) : 0);
  if (lds > (size_t)kMaxLds) return -1;
  const dim3 grid((unsigned)((n + threads - 1) / threads), (unsigned)(f + 1));
  const MifxShapRec* rc = static_cast<const MifxShapRec*>(recs);
#define MIFX_INTERACTIONS(T, A) \
  k_interactions<T, A><<<grid, threads, lds, stream>>>(static_cast<const T*>(X), n, f, rc, leaf_off, n_leaves, \
                                                       feat_off, feat_leaf, feat_pos, feat_rec, phi, phi_stride, \
                                                       chunk, out, stride)
  if (is_f64 && acc_lds) MIFX_INTERACTIONS(double, true);
  else if (is_f64) MIFX_INTERACTIONS(double, false);
  else if (acc_lds) MIFX_INTERACTIONS(float, true);
  else MIFX_INTERACTIONS(float, false);
#undef MIFX_INTERACTIONS
  return (int)hipGetLastError();
}

}  // extern "C"
