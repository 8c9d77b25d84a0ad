// MIFX_HIPCC_FLAGS: -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops
// The LambdaMART gradient pair of XGBRanker (rank:pairwise, rank:ndcg) on the device: the rule of gbdt_rank.h over
// contiguous query groups. Input: margins [n] (double), labels [n] (uint8 or double, integers in [0, 31]), gptr [G + 1],
// the discount table D and its prefix sums P, and a work list: the group ids sorted by size, descending, built once per
// fit (groups do not change between rounds). Output: g, h [n] float32. Everything stays on the caller's stream; no
// global atomics, no library sort, nothing read back. A group takes one of two routes by its size m:
//
//   k_rank_wave, m <= 64: one wave per group, several groups per workgroup (4 by default), one row per lane. Key, label
//     and margin stay in registers. The rank is counted: r_i = #{j : row j before row i} over m cross-lane reads of the
//     key. The label counts for IDCG are 31 wave ballots, so every lane holds the same IDCG without a reduction. For
//     the pair loop the wave writes a private 64-entry LDS image (margin, label) in rank order and every lane walks it:
//     each step is one broadcast LDS read for the whole wave. (The other way -- no LDS, cross-lane reads in rank order
//     -- needs the inverse permutation first and then three cross-lane moves per step, which go through the LDS
//     crossbar anyway; the image costs 576 bytes a wave and one read of each kind per step.)
//
//   k_rank_wg, 64 < m <= kCap: one workgroup per group, its LDS image sized for the largest group of the launch.
//     (key uint64, row uint16) are staged, padded to a power of two with entries that rank last, and sorted by a
//     bitonic network in LDS. Then the key becomes the margin again in place, the label is gathered through the sorted
//     row index, rank_of[row] is written, the labels are counted into wave-private LDS histograms (integer LDS adds) and
//     one lane evaluates the 31-term IDCG. After that LDS holds, in rank order, margin[r], label[r] and D[r]. Thread t
//     owns the ORIGINAL rows t, t + threads, ..., so the stores of g and h are coalesced; it finds its rank through
//     rank_of and walks r = 0 ... end - 1, every lane reading the same LDS address (a broadcast, no bank conflict).
//     The gain 2^l - 1 is a shift and a conversion from the label, so no gain table is kept.
//
// Every pair is evaluated twice, once from each of its rows: that doubles the number of exp calls, and it is the price
// of no atomics and of a sum order fixed by the rule alone. Launch geometry (groups per workgroup, threads) therefore
// changes no bit. LDS per row of the workgroup route: 8 (key / margin) + 2 (row) + 2 (rank_of) + 1 (label) + 8 (D) =
// 21 B; kCap = 4096 takes 86 KB of gfx950's 160 KB, above the 64 KB default, so the kernel opts in with
// hipFuncSetAttribute. Groups are launched in two size classes (up to 512 rows, and above) so that small groups are
// not held to the occupancy of the largest image.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gbdt_rank.h"

namespace {

constexpr int kCap = 4096;          // rows of the largest group (a power of two: the bitonic network's size)
constexpr int kMid = 512;           // the size-class boundary of the workgroup route
constexpr int kMaxThreads = 256;
constexpr int kMaxWaves = kMaxThreads / 64;

typedef uint64_t u64;

__device__ __forceinline__ int label_at(const void* y, int y_f64, long i) {
  const int l = y_f64 ? (int)static_cast<const double*>(y)[i] : (int)static_cast<const uint8_t*>(y)[i];
  return l & (kMifxRankLabels - 1);  // (validated by the host; the mask keeps a histogram index inside its table)
}

// ---- m <= 64: one wave per group; list[k] is the k-th group of this route
__global__ __launch_bounds__(kMaxThreads) void k_rank_wave(int ndcg, int topk, const double* margin, const void* y,
                                                           int y_f64, const long* gptr, const int* list, int count,
                                                           const double* D, const double* P, float* g, float* h) {
  __shared__ double s_m[kMaxWaves][64];
  __shared__ uint8_t s_l[kMaxWaves][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = blockIdx.x * (blockDim.x >> 6) + wave;
  long base = 0;
  int m = 0;
  if (k < count) {
    const int q = list[k];
    base = gptr[q];
    m = (int)(gptr[q + 1] - base);
    if (m > 64) m = 0;  // (not this route's: the host never lists one here)
  }
  const bool active = lane < m;
  const double mine = active ? margin[base + lane] : 0.0;
  const int label = active ? label_at(y, y_f64, base + lane) : -1;
  const u64 key = mifx_sort_key(mine);
  int rank = 0;
  for (int j = 0; j < m; ++j) {
    const u64 kj = (u64)__shfl((long long)key, j);
    rank += mifx_rk_before(kj, j, key, lane) ? 1 : 0;
  }
  double idcg = 0.0;
  if (ndcg) {
    int above = 0;
    for (int l = kMifxRankLabels - 1; l >= 1; --l) {  // mifx_rk_idcg with the counts taken from ballots
      const int c = __popcll(__ballot(label == l));
      idcg += mifx_rk_gain(l) * (P[above + c] - P[above]);
      above += c;
    }
  }
  if (active) {
    s_m[wave][rank] = mine;
    s_l[wave][rank] = (uint8_t)label;
  }
  __syncthreads();
  if (!active) return;
  const int end = mifx_rk_partner_end(rank, m, topk);
  const double d_self = D[rank];
  double gs = 0.0, hs = 0.0;
  for (int r = 0; r < end; ++r) {
    const int lr = s_l[wave][r];
    if (lr != label) mifx_rk_accum(ndcg != 0, idcg, mine, label, d_self, s_m[wave][r], lr, D[r], &gs, &hs);
  }
  g[base + lane] = (float)gs;
  h[base + lane] = (float)hs;
}

// ---- 64 < m <= cap (cap a power of two, the launch's largest group rounded up): one workgroup per group
struct WgImage {
  u64* key;           // [cap] keys, then the margins in rank order (the same 8 bytes)
  double* disc;       // [cap] D[r]
  uint16_t* row;      // [cap] the row (inside the group) at rank r
  uint16_t* rank_of;  // [cap] the rank of row i
  uint8_t* label;     // [cap] the label at rank r
};

__host__ __device__ inline size_t wg_image_bytes(int cap) { return (size_t)cap * 21; }

__device__ __forceinline__ WgImage wg_image(char* lds, int cap) {
  WgImage im;
  im.key = reinterpret_cast<u64*>(lds);
  im.disc = reinterpret_cast<double*>(lds + (size_t)cap * 8);
  im.row = reinterpret_cast<uint16_t*>(lds + (size_t)cap * 16);
  im.rank_of = reinterpret_cast<uint16_t*>(lds + (size_t)cap * 18);
  im.label = reinterpret_cast<uint8_t*>(lds + (size_t)cap * 20);
  return im;
}

__global__ __launch_bounds__(kMaxThreads) void k_rank_wg(int ndcg, int topk, const double* margin, const void* y,
                                                         int y_f64, const long* gptr, const int* list, int cap,
                                                         const double* D, const double* P, float* g, float* h) {
  extern __shared__ __align__(16) char lds[];
  __shared__ int s_cnt[kMaxWaves][kMifxRankLabels];
  __shared__ double s_idcg;
  const WgImage im = wg_image(lds, cap);
  const int tid = threadIdx.x, T = blockDim.x;
  const int q = list[blockIdx.x];
  const long base = gptr[q];
  const int m = (int)(gptr[q + 1] - base);
  if (m > cap || m < 1) return;  // (uniform; the host sizes cap from the launch's largest group)
  int mp = 64;
  while (mp < m) mp <<= 1;  // the network's size, <= cap
  for (int i = tid; i < mp; i += T) {
    im.key[i] = i < m ? mifx_sort_key(margin[base + i]) : 0ull;  // key 0 is no double's image: padding ranks last
    im.row[i] = (uint16_t)(i < m ? i : 0xFFFF);
    if (i < m) im.disc[i] = D[i];
  }
  for (int i = tid; i < kMaxWaves * kMifxRankLabels; i += T) (&s_cnt[0][0])[i] = 0;
  __syncthreads();
  for (int k = 2; k <= mp; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < mp; i += T) {
        const int p = i ^ j;
        if (p > i) {
          const u64 ki = im.key[i], kp = im.key[p];
          const int ri = im.row[i], rp = im.row[p];
          const bool up = (i & k) == 0;  // this pair ends in rank order (or in the reverse, for the merge above)
          if (mifx_rk_before(kp, rp, ki, ri) == up) {
            im.key[i] = kp, im.key[p] = ki;
            im.row[i] = (uint16_t)rp, im.row[p] = (uint16_t)ri;
          }
        }
      }
      __syncthreads();
    }
  for (int r = tid; r < m; r += T) {
    const int row = im.row[r];
    const int l = label_at(y, y_f64, base + row);
    reinterpret_cast<double*>(im.key)[r] = mifx_sort_value(im.key[r]);
    im.label[r] = (uint8_t)l;
    im.rank_of[row] = (uint16_t)r;
    if (ndcg) atomicAdd(&s_cnt[tid >> 6][l], 1);
  }
  __syncthreads();
  if (tid == 0) {
    if (ndcg)
      for (int l = 0; l < kMifxRankLabels; ++l)
        for (int w = 1; w < kMaxWaves; ++w) s_cnt[0][l] += s_cnt[w][l];
    s_idcg = ndcg ? mifx_rk_idcg(&s_cnt[0][0], P) : 0.0;
  }
  __syncthreads();
  const double idcg = s_idcg;
  const double* s_m = reinterpret_cast<const double*>(im.key);
  for (int a = tid; a < m; a += T) {
    const int ra = im.rank_of[a];
    const double mine = s_m[ra], d_self = im.disc[ra];
    const int label = im.label[ra];
    const int end = mifx_rk_partner_end(ra, m, topk);
    double gs = 0.0, hs = 0.0;
    for (int r = 0; r < end; ++r) {
      const int lr = im.label[r];
      if (lr != label) mifx_rk_accum(ndcg != 0, idcg, mine, label, d_self, s_m[r], lr, im.disc[r], &gs, &hs);
    }
    g[base + a] = (float)gs;
    h[base + a] = (float)hs;
  }
}

int launch_wg(int ndcg, int topk, const double* margin, const void* y, int y_f64, const long* gptr, const int* list,
              int count, int largest, int threads, const double* D, const double* P, float* g, float* h,
              hipStream_t stream) {
  if (count <= 0) return 0;
  int cap = 64;
  while (cap < largest) cap <<= 1;
  const size_t bytes = wg_image_bytes(cap);
  if (bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_rank_wg),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
  }
  k_rank_wg<<<count, threads, bytes, stream>>>(ndcg, topk, margin, y, y_f64, gptr, list, cap, D, P, g, h);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int mifx_gbdt_rank_max_group() { return kCap; }
int mifx_gbdt_rank_mid_group() { return kMid; }

// The gradient pair of every row. objective: 0 rank:pairwise, 1 rank:ndcg; topk: 0 for every pair. list [G]: the group
// ids by size, descending, of which the first n_large have more than kMid rows (the largest `largest` rows), the next
// n_mid more than 64 (the largest of them `largest_mid`), and the last n_small at most 64. D, P: device copies of the
// tables, longer than the largest group. groups_per_wg in [1, 4] is the wave route's geometry, threads (a multiple of
// 64 up to 256) the workgroup route's. Returns a HIP error code, or -1 for arguments outside the limits.
int mifx_gbdt_rank_grad_gpu(int objective, int topk, const double* margin, const void* y, int y_f64, const long* gptr,
                            const int* list, int n_large, int largest, int n_mid, int largest_mid, int n_small,
                            const double* D, const double* P, float* g, float* h, int groups_per_wg, int threads,
                            hipStream_t stream) {
  if (objective < 0 || objective > 1 || topk < 0 || largest > kCap || largest_mid > kMid) return -1;
  if (groups_per_wg < 1 || groups_per_wg > kMaxWaves || threads < 64 || threads > kMaxThreads || threads % 64) return -1;
  if (n_large < 0 || n_mid < 0 || n_small < 0) return -1;
  int rc = launch_wg(objective, topk, margin, y, y_f64, gptr, list, n_large, largest, threads, D, P, g, h, stream);
  if (rc) return rc;
  rc = launch_wg(objective, topk, margin, y, y_f64, gptr, list + n_large, n_mid, largest_mid, threads, D, P, g, h, stream);
  if (rc) return rc;
  if (n_small > 0) {
    const int grid = (n_small + groups_per_wg - 1) / groups_per_wg;
    k_rank_wave<<<grid, 64 * groups_per_wg, 0, stream>>>(objective, topk, margin, y, y_f64, gptr,
                                                        list + n_large + n_mid, n_small, D, P, g, h);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
