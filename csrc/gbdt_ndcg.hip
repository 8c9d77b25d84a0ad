// MIFX_HIPCC_FLAGS: -ffp-contract=off
// XGBRanker's eval metric "ndcg" / "ndcg@k" on the device: one double per query group, scored where the eval margins
// live. The rule is mifx.gbdt.xgb.ndcg's. Inside a group the rows are ranked by mifx_rk_before of gbdt_rank.h (margin
// descending on the integer key of gbdt_sort_key.h, ties to the lower row). With kk = m for "ndcg" and min(k, m) for
// "ndcg@k", and t_r = gain(label at rank r) * D[r] (gain = 2^l - 1, D the host's discount table: no log2 here),
//   DCG = ((0.0 + t_0) + t_1) + ... + t_{kk - 1}, one IEEE multiply per term and one IEEE add per term in rank order,
//   score = idcg > 0 ? DCG / idcg : 1.0, idcg [G] computed once per fit by the host (labels and groups only).
// No contraction (the flag above), no transcendental, no library sort, no global atomics: every bit is the host's, and
// launch geometry cannot change one. Input: margins [n] (double), labels [n] (uint8, 0 ... 31), gptr [G + 1], D, idcg
// and work lists built once per fit. Output: score [G]. A group takes one of two routes by its size m:
//
//   k_ndcg_wave, m <= 64: one wave per group, several groups per workgroup, one row per lane; key and label stay in
//     registers. The rank is counted over m cross-lane reads of the key. A lane with rank < kk writes its term into a
//     wave-private 64-double LDS image at slot `rank`; then every lane folds slots 0 ... kk - 1 in order (broadcast
//     reads) and lane 0 writes the score. One launch, no scratch.
//
//   k_ndcg_tile + k_ndcg_fold, m > 64, any size: ranks are COUNTED, not sorted, so no LDS image bounds the group. The
//     work list holds tiles (group, first row) of 256 rows; one workgroup per tile, one row per thread. The workgroup
//     streams the keys of the whole group through LDS in chunks of CHUNK keys, double-buffered: the next chunk's
//     global loads are issued before the current chunk is consumed and land in the other buffer after it, one barrier
//     per chunk. Every thread counts the rows that rank before its own; all lanes read the same LDS address (a
//     broadcast). A chunk that lies wholly below the tile's rows counts `key_j >= key` and one wholly above `key_j >
//     key` (the tie rule with the row order known); only the chunks that overlap the tile compare row indices, on a
//     key tie. Ranks are a permutation of 0 ... m - 1, so a thread with rank < kk stores terms[base + rank] and every
//     slot that is read later is written exactly once; nothing is initialised. Under "ndcg@k" a wave stops counting as
//     soon as all its lanes have counted kk rows before them (their terms are not wanted): one __all per chunk. Such
//     a wave still loads and stages its share of the next chunk, and the barrier at the end of a chunk votes
//     (__syncthreads_and), so a tile whose waves have all stopped leaves the loop. Only the waves that hold one of the
//     group's kk best rows walk the whole group: O(m kk) compares a group instead of O(m^2).
//     k_ndcg_fold then takes one wave per tiled group: 64 terms per step, coalesced and loaded one step ahead, folded
//     in rank order by lane reads (every lane carries the same running sum), stopping at kk.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gbdt_rank.h"

namespace {

constexpr int kTile = 256;          // rows of a tile = threads of its workgroup
constexpr int kMaxWaves = 4;        // groups per workgroup of the wave route and of the fold
constexpr int kChunk = 2048;        // keys of an LDS chunk (2 x 16 KB); kChunkSmall is the tests' second geometry
constexpr int kChunkSmall = 512;
// Rows of the largest eval group XGBRanker scores here (the kernels themselves have no limit). Counting is O(m^2), so
// a single-group eval set was timed at 2^12 ... 2^20 rows against the read-back plus the host function: the device
// step was faster at every size, so the limit is the largest size tried (no crossover found; profiles/gbdt_ndcg.md).
constexpr int kMaxGroup = 1 << 20;

typedef uint64_t u64;

__device__ __forceinline__ int cutoff(int k, int m) { return k > 0 && k < m ? k : m; }
__device__ __forceinline__ double term(const uint8_t* label, long i, const double* D, int rank) {
  return mifx_rk_gain(label[i] & (kMifxRankLabels - 1)) * D[rank];
}
// lane j's v for the whole wave, j wave-uniform: two lane reads into scalar registers, no trip through the LDS crossbar
// (the fold's adds form one dependent chain, so a step's latency is the fold's time)
__device__ __forceinline__ double lane_value(double v, int j) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j),
                          __builtin_amdgcn_readlane(__double2loint(v), j));
}
__device__ __forceinline__ double group_score(double dcg, double idcg) { return idcg > 0.0 ? dcg / idcg : 1.0; }

// ---- m <= 64: one wave per group; list[g] is the g-th group of this route
__global__ __launch_bounds__(64 * kMaxWaves) void k_ndcg_wave(int k, const double* margin, const uint8_t* label,
                                                              const long* gptr, const int* list, int count,
                                                              const double* D, const double* idcg, double* score) {
  __shared__ double s_t[kMaxWaves][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = blockIdx.x * (blockDim.x >> 6) + wave;
  int q = -1, m = 0;
  long base = 0;
  if (g < count) {
    q = list[g];
    base = gptr[q];
    m = (int)(gptr[q + 1] - base);
    if (m > 64) q = -1, m = 0;  // (not this route's: the host never lists one here)
  }
  const bool active = lane < m;
  const u64 key = mifx_sort_key(active ? margin[base + lane] : 0.0);
  int rank = 0;
  for (int j = 0; j < m; ++j) {
    const u64 kj = (u64)__shfl((long long)key, j);
    rank += mifx_rk_before(kj, j, key, lane) ? 1 : 0;
  }
  const int kk = cutoff(k, m);
  if (active && rank < kk) s_t[wave][rank] = term(label, base + lane, D, rank);
  __syncthreads();
  double dcg = 0.0;
  for (int r = 0; r < kk; ++r) dcg += s_t[wave][r];
  if (lane == 0 && q >= 0) score[q] = group_score(dcg, idcg[q]);
}

// ---- m > 64: one workgroup per tile (group, first row) of kTile rows
template <int CHUNK>
__global__ __launch_bounds__(kTile) void k_ndcg_tile(int k, const double* margin, const uint8_t* label,
                                                     const long* gptr, const int2* tiles, const double* D,
                                                     double* terms) {
  constexpr int kPer = CHUNK / kTile;  // keys a thread stages per chunk
  __shared__ u64 s_key[2][CHUNK];
  const int tid = threadIdx.x;
  const int2 tile = tiles[blockIdx.x];
  const long base = gptr[tile.x];
  const int m = (int)(gptr[tile.x + 1] - base);
  const int row = tile.y + tid;
  const bool active = row < m;
  const int kk = cutoff(k, m);
  const u64 key = active ? mifx_sort_key(margin[base + row]) : 0ull;
  double next[kPer];
  auto load = [&](int c0) {  // the chunk's margins into registers; rows past the group's end are never consumed
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int j = c0 + i * kTile + tid;
      next[i] = j < m ? margin[base + j] : 0.0;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) s_key[buf][i * kTile + tid] = mifx_sort_key(next[i]);
  };
  load(0);
  stage(0);
  __syncthreads();
  int count = 0;
  bool done = __all(!active);  // wave-uniform from here on
  for (int c0 = 0, buf = 0;; c0 += CHUNK, buf ^= 1) {
    const bool more = c0 + CHUNK < m;
    if (more) load(c0 + CHUNK);
    if (!done) {
      const int len = min(CHUNK, m - c0);
      const u64* s = s_key[buf];
      if (c0 + len <= tile.y) {  // every row of the chunk is a lower row than the tile's: a tie ranks it before
#pragma unroll 8
        for (int j = 0; j < len; ++j) count += s[j] >= key ? 1 : 0;
      } else if (c0 >= tile.y + kTile) {  // every row is a higher one: a tie ranks it after
#pragma unroll 8
        for (int j = 0; j < len; ++j) count += s[j] > key ? 1 : 0;
      } else {
#pragma unroll 8
        for (int j = 0; j < len; ++j) count += mifx_rk_before(s[j], c0 + j, key, row) ? 1 : 0;
      }
      if (k > 0) done = __all(!active || count >= kk);
    }
    if (!more) break;
    stage(buf ^ 1);  // (its last readers passed the barrier that ended the chunk before this one)
    if (k > 0) {
      if (__syncthreads_and(done)) break;
    } else {
      __syncthreads();
    }
  }
  if (active && count < kk) terms[base + count] = term(label, base + row, D, count);
}

// ---- one wave per tiled group: the terms in rank order, 64 per step
__global__ __launch_bounds__(64 * kMaxWaves) void k_ndcg_fold(int k, const long* gptr, const int* list, int count,
                                                              const double* terms, const double* idcg,
                                                              double* score) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (g >= count) return;  // (a whole wave; the kernel has no barrier)
  const int q = list[g];
  const long base = gptr[q];
  const int kk = cutoff(k, (int)(gptr[q + 1] - base));
  double dcg = 0.0;
  double t = lane < kk ? terms[base + lane] : 0.0;
  for (int r0 = 0; r0 < kk; r0 += 64) {
    const double cur = t;
    if (r0 + 64 + lane < kk) t = terms[base + r0 + 64 + lane];  // the next step's terms, under this step's adds
    if (kk - r0 >= 64) {
#pragma unroll
      for (int j = 0; j < 64; ++j) dcg += lane_value(cur, j);
    } else {
      for (int j = 0; j < kk - r0; ++j) dcg += lane_value(cur, j);
    }
  }
  if (lane == 0) score[q] = group_score(dcg, idcg[q]);
}

}  // namespace

extern "C" {

int mifx_gbdt_ndcg_max_group() { return kMaxGroup; }
int mifx_gbdt_ndcg_max_groups_per_wg() { return kMaxWaves; }
int mifx_gbdt_ndcg_tile() { return kTile; }
// 1 if `chunk` is one of the tile kernel's compiled chunk sizes
int mifx_gbdt_ndcg_chunk_ok(int chunk) { return chunk == kChunk || chunk == kChunkSmall; }

// score [G] of the margins. k: 0 for "ndcg", the cutoff of "ndcg@k". list_small [n_small]: the groups of up to 64
// rows; tiles [n_tiles] (group, first row) and list_big [n_big]: the tiles of 256 rows and the ids of the larger
// groups; terms [n]: scratch of the tiled route (may be null without tiles). groups_per_wg in [1, 4] and chunk (0:
// the default) are launch geometry. Returns a HIP error code, or -1 for arguments outside the limits.
int mifx_gbdt_ndcg_gpu(int k, const double* margin, const uint8_t* label, const long* gptr, const double* D,
                       const double* idcg, const int* list_small, int n_small, const int* tiles, int n_tiles,
                       const int* list_big, int n_big, double* terms, double* score, int groups_per_wg, int chunk,
                       hipStream_t stream) {
  if (chunk == 0) chunk = kChunk;
  if (k < 0 || n_small < 0 || n_tiles < 0 || n_big < 0 || (n_tiles > 0 && (!terms || n_big < 1))) return -1;
  if (groups_per_wg < 1 || groups_per_wg > kMaxWaves || !mifx_gbdt_ndcg_chunk_ok(chunk)) return -1;
  if (n_small > 0) {
    const int grid = (n_small + groups_per_wg - 1) / groups_per_wg;
    k_ndcg_wave<<<grid, 64 * groups_per_wg, 0, stream>>>(k, margin, label, gptr, list_small, n_small, D, idcg, score);
  }
  if (n_tiles > 0) {
    const int2* t2 = reinterpret_cast<const int2*>(tiles);
    if (chunk == kChunk)
      k_ndcg_tile<kChunk><<<n_tiles, kTile, 0, stream>>>(k, margin, label, gptr, t2, D, terms);
    else
      k_ndcg_tile<kChunkSmall><<<n_tiles, kTile, 0, stream>>>(k, margin, label, gptr, t2, D, terms);
    const int grid = (n_big + groups_per_wg - 1) / groups_per_wg;
    k_ndcg_fold<<<grid, 64 * groups_per_wg, 0, stream>>>(k, gptr, list_big, n_big, terms, idcg, score);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
