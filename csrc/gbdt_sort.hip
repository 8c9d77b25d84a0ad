// Batched keys-only radix sort of a group of columns of a row-major [n, f] float32 / float64 device table, for the
// quantile cuts of mifx.gbdt (mifx/ops/gbdt_prep.py: device_sort_columns). All G columns of the group sort in the same
// launches: the column is grid dimension y of every kernel. The result is what mifx_gbdt_prep_cuts consumes: sorted
// [G, n] float64 (per column ascending, -0.0 before +0.0, the NaNs last) and nan_count [G] int64.
// MIFX_HIPCC_FLAGS: -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops
//
// Keys (gbdt_sort_key.h) are 64-bit for a float64 table and 32-bit for a float32 one (widening is monotone and exact,
// so a float32 column sorts in half the passes on half the bytes and is widened in the last scatter only).
//
//   k_sort_load     one pass over the table. A workgroup reads tiles of 128 rows x up to 32 columns along the rows of
//                   the table (a row's cells of the group are contiguous), turns them into keys, transposes them
//                   through LDS and stores them column-major with one wave on 64 consecutive keys of one column. A
//                   thread reads the same column in every tile, so the column's NaN count and the OR and the AND of
//                   its keys are three registers per thread; a workgroup combines them in LDS and writes one partial
//                   per column -- no global atomics, nothing to clear beforehand.
//   k_sort_plan     one workgroup: combines the partials into nan_count and into the set of 8-bit digits to sort by.
//                   Every key of a column has the same value in a digit exactly when OR and AND agree on its bits; a
//                   digit in which that holds for every column of the group is a stable pass that moves nothing, and
//                   is skipped (the occupancy of single bins, from two words instead of 256 counters per digit and
//                   column). The top digit is never skipped, so the pass that writes the float64 result always runs.
//   per digit       k_sort_count   per (tile, column): the tile's 256 digit counts, to cnt[column][digit][tile]
//                   k_sort_scan    one wave per (column, digit): exclusive scan over the tiles, in place, and the
//                                  digit's total
//                   k_sort_scatter per (tile, column): digit starts (a 256-entry scan of the totals) plus the tile's
//                                  scanned counts give the tile's first position per digit; the tile is walked in
//                                  chunks of 256 x kKpt keys held in registers
//                   The three kernels of a skipped digit return at once; which of the two key buffers holds the
//                   current order is the parity of the passes that ran, which every kernel derives from the plan word.
//
// The in-tile rank is stable: a wave takes 64 consecutive keys at a time; eight ballots give each lane the set of
// lanes holding its digit, its rank is the number of those below it, and the lowest of them advances the wave's
// counter of that digit in LDS by the size of the set and hands the old value to the others. After the chunk, thread d
// turns the four waves' counts of digit d into positions in wave order and advances the tile's running position.
//
// Every dependency between workgroups is a kernel boundary; there is no atomic on global memory. Positions inside a
// column are 32-bit (n < 2^31). The output is a pure function of the input: tile size, grid sizes, the grouping of
// columns and the skipped passes change no bit of it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gbdt_sort_key.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kKpt = 4;                    // keys per thread and chunk, in registers
constexpr int kChunk = kThreads * kKpt;    // a tile is a whole number of chunks
constexpr int kMaxTile = 1 << 16;
constexpr int kLoadRows = 128;             // load tile: 128 rows x 32 columns x 8 B = 32 KB of LDS (+ padding)
constexpr int kLoadCols = 32;
constexpr int kLoadBlocks = 512;           // row workgroups of the load pass: each leaves one partial per column
constexpr int kMaxGroup = 65535;           // grid dimension y

typedef unsigned long long u64;

struct Layout {  // the scratch buffer, every part 256-byte aligned
  size_t keys_a, keys_b, cnt, total, p_or, p_and, p_nan, plan, bytes;
  int nt, ntp, blocks;
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

Layout layout(long n, int G, int tile, int key_bytes) {
  Layout L;
  L.nt = (int)((n + tile - 1) / tile);
  L.ntp = (L.nt + 3) & ~3;  // rows of cnt start 16-byte aligned: k_sort_scan moves four counts at a time
  const long row_tiles = (n + kLoadRows - 1) / kLoadRows;
  L.blocks = (int)(row_tiles < kLoadBlocks ? row_tiles : kLoadBlocks);
  size_t at = 0;
  const auto take = [&at](size_t bytes) {
    const size_t here = at;
    at = align256(at + bytes);
    return here;
  };
  L.keys_a = take((size_t)G * n * key_bytes);
  L.keys_b = take((size_t)G * n * key_bytes);
  L.cnt = take((size_t)G * 256 * L.ntp * sizeof(unsigned));
  L.total = take((size_t)G * 256 * sizeof(unsigned));
  L.p_or = take((size_t)L.blocks * G * sizeof(u64));
  L.p_and = take((size_t)L.blocks * G * sizeof(u64));
  L.p_nan = take((size_t)L.blocks * G * sizeof(unsigned));
  L.plan = take(sizeof(unsigned));
  L.bytes = at;
  return L;
}

// ---- load

template <class T, class K>
__global__ __launch_bounds__(kThreads) void k_sort_load(const T* X, long n, int f, int j0, int G, int lg_cw, K* keys,
                                                        u64* p_or, u64* p_and, unsigned* p_nan) {
  __shared__ K tile[kLoadCols * (kLoadRows + 1)];
  __shared__ u64 l_or[kLoadCols], l_and[kLoadCols];
  __shared__ unsigned l_nan[kLoadCols];
  const int t = threadIdx.x;
  const int c0 = blockIdx.y * kLoadCols;
  const int gw = min(kLoadCols, G - c0);
  // reading: 2^lg_cw >= gw column slots side by side, the rest of the workgroup down the rows
  const int c = t & ((1 << lg_cw) - 1), rs = t >> lg_cw, rstep = kThreads >> lg_cw;
  if (t < kLoadCols) {
    l_or[t] = 0;
    l_and[t] = ~(u64)0;
    l_nan[t] = 0;
  }
  K vor = 0, vand = ~(K)0;
  unsigned nan = 0;
  const long tiles = (n + kLoadRows - 1) / kLoadRows;
  for (long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const long r0 = tl * kLoadRows;
    const int rows = (int)min((long)kLoadRows, n - r0);
    __syncthreads();  // the previous tile has been stored
    if (c < gw)
      for (int r = rs; r < rows; r += rstep) {
        const K k = mifx_sort_key(X[(size_t)(r0 + r) * f + j0 + c0 + c]);
        nan += k == ~(K)0;
        vor |= k;
        vand &= k;
        tile[c * (kLoadRows + 1) + r] = k;
      }
    __syncthreads();
    for (int e = t; e < gw * kLoadRows; e += kThreads) {
      const int cc = e / kLoadRows, r = e % kLoadRows;
      if (r < rows) keys[(size_t)(c0 + cc) * n + r0 + r] = tile[cc * (kLoadRows + 1) + r];
    }
  }
  if (c < gw) {  // a 32-bit key leaves the upper halves of OR and AND equal (zero)
    atomicOr(&l_or[c], (u64)vor);
    atomicAnd(&l_and[c], (u64)vand);
    atomicAdd(&l_nan[c], nan);
  }
  __syncthreads();
  if (t < gw) {
    const size_t at = (size_t)blockIdx.x * G + c0 + t;
    p_or[at] = l_or[t];
    p_and[at] = l_and[t];
    p_nan[at] = l_nan[t];
  }
}

// plan[0]: bit d set = sort by digit d. One workgroup: 4 slices of the partials x 64 columns at a time.
__global__ __launch_bounds__(kThreads) void k_sort_plan(const u64* p_or, const u64* p_and, const unsigned* p_nan,
                                                        int blocks, int G, int digits, long long* nan_count,
                                                        unsigned* plan) {
  __shared__ u64 s_or[kThreads], s_and[kThreads], s_nan[kThreads];
  const int t = threadIdx.x, cl = t & 63, sl = t >> 6;
  u64 diff = 0;
  for (int cb = 0; cb < G; cb += 64) {
    const int c = cb + cl;
    u64 o = 0, a = ~(u64)0, nn = 0;
    if (c < G)
      for (int b = sl; b < blocks; b += kWaves) {
        const size_t at = (size_t)b * G + c;
        o |= p_or[at];
        a &= p_and[at];
        nn += p_nan[at];
      }
    s_or[t] = o;
    s_and[t] = a;
    s_nan[t] = nn;
    __syncthreads();
    if (sl == 0 && c < G) {
      for (int s = 1; s < kWaves; ++s) {
        o |= s_or[s * 64 + cl];
        a &= s_and[s * 64 + cl];
        nn += s_nan[s * 64 + cl];
      }
      nan_count[c] = (long long)nn;
      diff |= o ^ a;
    }
    __syncthreads();
  }
  if (sl == 0) {
    for (int off = 32; off > 0; off >>= 1) diff |= __shfl_xor(diff, off);
    if (t == 0) {
      unsigned mask = 1u << (digits - 1);
      for (int d = 0; d < digits; ++d)
        if ((diff >> (8 * d)) & 255) mask |= 1u << d;
      plan[0] = mask;
    }
  }
}

// ---- one digit

__device__ inline bool pass_runs(unsigned mask, int dig) { return (mask >> dig) & 1; }
// the passes below `dig` that ran, odd: the current order is in the second buffer
__device__ inline bool pass_from_b(unsigned mask, int dig) { return __popc(mask & ((1u << dig) - 1)) & 1; }

__device__ inline unsigned wave_inclusive_scan(unsigned v, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}

template <class K>
__global__ __launch_bounds__(kThreads) void k_sort_count(const K* A, const K* B, long n, int tile, int ntp, int dig,
                                                         const unsigned* plan, unsigned* cnt) {
  __shared__ unsigned h[256];
  const unsigned mask = plan[0];
  if (!pass_runs(mask, dig)) return;
  const int t = threadIdx.x, c = blockIdx.y;
  const K* col = (pass_from_b(mask, dig) ? B : A) + (size_t)c * n;
  h[t] = 0;
  __syncthreads();
  const long b0 = (long)blockIdx.x * tile, b1 = min(n, b0 + tile);
  for (long i = b0 + t; i < b1; i += kThreads) atomicAdd(&h[(unsigned)(col[i] >> (8 * dig)) & 255], 1u);
  __syncthreads();
  cnt[((size_t)c * 256 + t) * ntp + blockIdx.x] = h[t];
}

// wave w of workgroup (x, c) scans the nt tile counts of digit 4 x + w of column c, four per lane and step
__global__ __launch_bounds__(kThreads) void k_sort_scan(unsigned* cnt, unsigned* total, int nt, int ntp, int dig,
                                                        const unsigned* plan) {
  if (!pass_runs(plan[0], dig)) return;
  const int lane = threadIdx.x & 63, d = blockIdx.x * kWaves + (threadIdx.x >> 6), c = blockIdx.y;
  unsigned* row = cnt + ((size_t)c * 256 + d) * ntp;
  unsigned carry = 0;
  for (int base = 0; base < ntp; base += 256) {
    const int i = base + lane * 4;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (i < ntp) v = *reinterpret_cast<const uint4*>(row + i);  // ntp is a multiple of 4: all four are inside the row
    if (i + 0 >= nt) v.x = 0;  // the row's padding was never written
    if (i + 1 >= nt) v.y = 0;
    if (i + 2 >= nt) v.z = 0;
    if (i + 3 >= nt) v.w = 0;
    const unsigned s = v.x + v.y + v.z + v.w;
    const unsigned inc = wave_inclusive_scan(s, lane);
    const unsigned ex = carry + inc - s;
    if (i < ntp) *reinterpret_cast<uint4*>(row + i) = make_uint4(ex, ex + v.x, ex + v.x + v.y, ex + v.x + v.y + v.z);
    carry += __shfl(inc, 63);
  }
  if (lane == 0) total[c * 256 + d] = carry;
}

template <class K, bool LAST>
__global__ __launch_bounds__(kThreads) void k_sort_scatter(K* A, K* B, double* out, long n, int tile, int ntp, int dig,
                                                           const unsigned* plan, const unsigned* cnt,
                                                           const unsigned* total) {
  __shared__ unsigned base[256];          // where the tile's next key of each digit goes
  __shared__ unsigned wcnt[kWaves][256];  // per wave and digit: the chunk's count, then the wave's first position
  __shared__ unsigned wsum[kWaves];
  const unsigned mask = plan[0];
  if (!pass_runs(mask, dig)) return;
  const bool from_b = pass_from_b(mask, dig);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, c = blockIdx.y;
  const K* col = (from_b ? B : A) + (size_t)c * n;
  K* dst = (from_b ? A : B) + (size_t)c * n;
  double* res = out + (size_t)c * n;

  const unsigned tot = total[c * 256 + t];
  const unsigned inc = wave_inclusive_scan(tot, lane);
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  unsigned start = inc - tot;
  for (int q = 0; q < w; ++q) start += wsum[q];
  base[t] = start + cnt[((size_t)c * 256 + t) * ntp + blockIdx.x];

  const long b0 = (long)blockIdx.x * tile, b1 = min(n, b0 + tile);
  for (long ch = b0; ch < b1; ch += kChunk) {
    for (int q = 0; q < kWaves; ++q) wcnt[q][t] = 0;
    __syncthreads();
    K key[kKpt];
    unsigned off[kKpt];
#pragma unroll
    for (int k = 0; k < kKpt; ++k) {  // wave w: keys [w * 64 kKpt, (w + 1) * 64 kKpt) of the chunk, 64 at a time
      const long i = ch + (w * kKpt + k) * 64 + lane;
      const bool valid = i < b1;
      key[k] = valid ? col[i] : (K)0;
      const unsigned d = (unsigned)(key[k] >> (8 * dig)) & 255;
      u64 same = __ballot(valid);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1;
        const u64 bal = __ballot(bit);
        same &= bit ? bal : ~bal;
      }
      // a valid lane is in its own set; the lanes past the column's end come last and take no part
      const int leader = valid ? __ffsll((long long)same) - 1 : lane;
      unsigned old = 0;
      if (valid && lane == leader) {
        old = wcnt[w][d];
        wcnt[w][d] = old + __popcll(same);
      }
      old = __shfl(old, leader);
      off[k] = old + __popcll(same & (((u64)1 << lane) - 1));
    }
    __syncthreads();
    {
      unsigned run = base[t];
      for (int q = 0; q < kWaves; ++q) {
        const unsigned own = wcnt[q][t];
        wcnt[q][t] = run;
        run += own;
      }
      base[t] = run;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kKpt; ++k) {
      const long i = ch + (w * kKpt + k) * 64 + lane;
      const unsigned d = (unsigned)(key[k] >> (8 * dig)) & 255;
      const unsigned pos = wcnt[w][d] + off[k];
      if (i < b1 && (long)pos < n) {  // pos < n by construction; never store past the column
        if (LAST) res[pos] = mifx_sort_value(key[k]);
        else dst[pos] = key[k];
      }
    }
    __syncthreads();  // wcnt has been read
  }
}

template <class T, class K>
int sort_group(const T* X, long n, int f, int j0, int G, int tile, char* scratch, double* out, long long* nan_count,
               hipStream_t stream) {
  const Layout L = layout(n, G, tile, (int)sizeof(K));
  K* A = reinterpret_cast<K*>(scratch + L.keys_a);
  K* B = reinterpret_cast<K*>(scratch + L.keys_b);
  unsigned* cnt = reinterpret_cast<unsigned*>(scratch + L.cnt);
  unsigned* total = reinterpret_cast<unsigned*>(scratch + L.total);
  u64* p_or = reinterpret_cast<u64*>(scratch + L.p_or);
  u64* p_and = reinterpret_cast<u64*>(scratch + L.p_and);
  unsigned* p_nan = reinterpret_cast<unsigned*>(scratch + L.p_nan);
  unsigned* plan = reinterpret_cast<unsigned*>(scratch + L.plan);
  const int digits = (int)sizeof(K);
  int lg_cw = 0;
  while ((1 << lg_cw) < (G < kLoadCols ? G : kLoadCols)) ++lg_cw;
  const dim3 load_grid((unsigned)L.blocks, (unsigned)((G + kLoadCols - 1) / kLoadCols));
  k_sort_load<T, K><<<load_grid, kThreads, 0, stream>>>(X, n, f, j0, G, lg_cw, A, p_or, p_and, p_nan);
  k_sort_plan<<<1, kThreads, 0, stream>>>(p_or, p_and, p_nan, L.blocks, G, digits, nan_count, plan);
  const dim3 tiles((unsigned)L.nt, (unsigned)G), rows(256 / kWaves, (unsigned)G);
  for (int dig = 0; dig < digits; ++dig) {
    k_sort_count<K><<<tiles, kThreads, 0, stream>>>(A, B, n, tile, L.ntp, dig, plan, cnt);
    k_sort_scan<<<rows, kThreads, 0, stream>>>(cnt, total, L.nt, L.ntp, dig, plan);
    if (dig + 1 < digits)
      k_sort_scatter<K, false><<<tiles, kThreads, 0, stream>>>(A, B, out, n, tile, L.ntp, dig, plan, cnt, total);
    else
      k_sort_scatter<K, true><<<tiles, kThreads, 0, stream>>>(A, B, out, n, tile, L.ntp, dig, plan, cnt, total);
  }
  return (int)hipGetLastError();
}

bool geometry_ok(long n, int G, int tile) {
  return n >= 1 && n < (1L << 31) && G >= 1 && G <= kMaxGroup && tile >= kChunk && tile <= kMaxTile &&
         tile % kChunk == 0;
}

}  // namespace

extern "C" {

int mifx_gbdt_sort_key_bytes(int is_f64) { return is_f64 ? 8 : 4; }
int mifx_gbdt_sort_tile_step() { return kChunk; }  // a tile is a multiple of this, at least one
int mifx_gbdt_sort_max_tile() { return kMaxTile; }
int mifx_gbdt_sort_max_group() { return kMaxGroup; }

// bytes of scratch for sorting G columns of n rows with `tile` keys per workgroup; -1: geometry out of range
long mifx_gbdt_sort_scratch_bytes(long n, int G, int tile, int is_f64) {
  if (!geometry_ok(n, G, tile)) return -1;
  return (long)layout(n, G, tile, is_f64 ? 8 : 4).bytes;
}

// Sorts columns [j0, j0 + G) of the row-major [n, f] table X (is_f64: double, else float), all in the same launches.
// out [G, n] float64: per column the non-NaN values ascending (-0.0 before +0.0), then the NaNs; nan_count [G] int64.
// scratch: mifx_gbdt_sort_scratch_bytes(n, G, tile, is_f64) bytes, 256-byte aligned; nothing in it needs clearing.
int mifx_gbdt_sort_launch(const void* X, int is_f64, long n, int f, int j0, int G, int tile, void* scratch,
                          double* out, long long* nan_count, hipStream_t stream) {
  if (!geometry_ok(n, G, tile) || f < 1 || j0 < 0 || (long)j0 + G > f) return -1;
  char* s = static_cast<char*>(scratch);
  if (is_f64)
    return sort_group<double, uint64_t>(static_cast<const double*>(X), n, f, j0, G, tile, s, out, nan_count, stream);
  return sort_group<float, uint32_t>(static_cast<const float*>(X), n, f, j0, G, tile, s, out, nan_count, stream);
}

}  // extern "C"
