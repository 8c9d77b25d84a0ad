// Step tail of the Wide&Deep trainers: gradient-slab reductions, optimizer kernels and the xGMI exchange (device
// code; the launchers are in csrc/wide_deep.hip). Included inside that translation unit's anonymous namespace.
#pragma once
#include "wd_opt.h"

// partial[sp][e] = sum_{g in split sp} slab[g][e]   (float4 granules, 4 loads in flight)
__global__ __launch_bounds__(256) void wd_reduce(const float4* __restrict__ slab, int G, int gchunk,
                                                 float4* __restrict__ partial, int stride) {
  const int S4 = stride / 4;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= S4) return;
  const int g0 = blockIdx.y * gchunk;
  const int g1 = min(G, g0 + gchunk);
  float4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = make_float4(0, 0, 0, 0);
  int g = g0;
  for (; g + 3 < g1; g += 4) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = slab[(size_t)(g + u) * S4 + e];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc[u].x += v[u].x; acc[u].y += v[u].y; acc[u].z += v[u].z; acc[u].w += v[u].w;
    }
  }
  for (; g < g1; ++g) {
    const float4 v = slab[(size_t)g * S4 + e];
    acc[0].x += v.x; acc[0].y += v.y; acc[0].z += v.z; acc[0].w += v.w;
  }
  partial[(size_t)blockIdx.y * S4 + e] =
      make_float4(acc[0].x + acc[1].x + acc[2].x + acc[3].x, acc[0].y + acc[1].y + acc[2].y + acc[3].y,
                  acc[0].z + acc[1].z + acc[2].z + acc[3].z, acc[0].w + acc[1].w + acc[2].w + acc[3].w);
}

// Step counters: the optimizer step is needed by every workgroup (Adam bias correction) and the next fused
// launch derives its data offset from it. A single counter bumped by one workgroup races with the others'
// reads, and a last-workgroup-done atomic costs an agent-scope fence (L2 writeback) per workgroup, so each
// workgroup owns a slot: step_ctr[blockIdx.x] is read and bumped by that workgroup only; slot 0 is the
// canonical step the fused kernel reads. All STEP_SLOTS slots start equal (host set_step). The exchange epochs
// (xep, xctr) are slot arrays of the same kind.

// One workgroup of NT threads keeps the slots that no workgroup of its grid owns, [first_free, STEP_SLOTS), equal to
// the value its own slot moves to, so a later launch with a larger grid finds every slot in step.
// With TWO, a second slot array of the same grid moves in the same pass.
template <int NT, bool TWO = false>
__device__ __forceinline__ void fan_out_slots(long long* __restrict__ slots, unsigned int first_free, long long value,
                                              long long* __restrict__ slots2 = nullptr, long long value2 = 0) {
  for (int i = first_free + threadIdx.x; i < STEP_SLOTS; i += NT) {
    slots[i] = value;
    if (TWO) slots2[i] = value2;
  }
}

// One thread per canonical parameter. DNN segment [0, WTOT) then wide segment [WTOT, WTOT+NWIDE).
__global__ __launch_bounds__(256) void wd_optimizer(
    const float* __restrict__ partial, int nparts, const int* __restrict__ gidx, const uint8_t* __restrict__ mask,
    float* __restrict__ param, float* __restrict__ s0, float* __restrict__ s1, uint16_t* __restrict__ wt_out,
    long long* __restrict__ step_ctr, OptHyper hd, OptHyper hw, int stride) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  __shared__ long long s_step;
  if (threadIdx.x == 0) s_step = step_ctr[blockIdx.x] + 1;  // the slot's only reader and writer: thread 0
  __syncthreads();
  const long long step = s_step;
  if (c < WTOT + NWIDE) {
    const bool dnn = c < WTOT;
    float w = param[c];
    if (mask[c]) {
      const int gi = gidx[c];
      float gs[4] = {0.f, 0.f, 0.f, 0.f};
      int pidx = 0;
      for (; pidx + 3 < nparts; pidx += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) gs[u] += partial[(size_t)(pidx + u) * stride + gi];
      }
      for (; pidx < nparts; ++pidx) gs[0] += partial[(size_t)pidx * stride + gi];
      const float g = (gs[0] + gs[1]) + (gs[2] + gs[3]);
      float a0 = s0[c], a1 = s1[c];
      w = opt_update(dnn ? hd : hw, w, g, a0, a1, step);
      s0[c] = a0;
      s1[c] = a1;
      param[c] = w;
    }
    if (dnn) wt_out[c] = __builtin_bit_cast(uint16_t, (bf16)w);
  }
  if (threadIdx.x == 0) step_ctr[blockIdx.x] = step;
}

// Fused slab reduction + optimizer: one workgroup owns RQ float4 columns (4*RQ gradient entries) of the
// compact slab and sums ALL G rows of them (row groups of 256/RQ threads, fixed order -> deterministic), so
// the full per-column gradient is available in one workgroup and the optimizer runs right there through
// the inverse map inv[slab column] -> canonical parameter (-1 = padding). Replaces wd_reduce + wd_optimizer
// (two launches, a [nsplit, stride] round trip) on the single-rank step; with OPT=false it is the local
// full reduction feeding the DP all-reduce.
constexpr int RQ = 16;               // float4 columns per workgroup
constexpr int RG = 256 / RQ;         // row groups
constexpr int RU = 8;            // slab rows in flight per thread (G=256: 322 workgroups x 256 threads x
                                     // 8 x 16 B = the whole 21 MB slab requested in two rounds; RU 16, all of
                                     // it in one round, measured 2 us slower per step: profiles/archive/wd_ab_r2s.txt)

// Column sums of the slab: float4 column q = blockIdx.x * RQ + threadIdx.x % RQ over rows [0, G), row groups of
// RG threads, fixed order (deterministic). The full sum is returned to threads threadIdx.x < RQ. (A chunk-major
// slab layout -- this workgroup's columns one contiguous [G][RQ] block -- measured no faster: profiles/archive/wd_ab_r2s.txt)
__device__ __forceinline__ float4 slab_column_sum(const float4* __restrict__ slab, int G, int S4,
                                                  float4 (&part)[RG][RQ]) {
  const int lq = threadIdx.x % RQ, r = threadIdx.x / RQ;
  const int q = blockIdx.x * RQ + lq;
  float4 acc[RU];
#pragma unroll
  for (int u = 0; u < RU; ++u) acc[u] = make_float4(0, 0, 0, 0);
  if (q < S4) {
    const float4* base = slab + q;
    const size_t rs = S4;
    int g = r;
    for (; g + (RU - 1) * RG < G; g += RU * RG) {
      float4 v[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) v[u] = base[(size_t)(g + u * RG) * rs];
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        acc[u].x += v[u].x; acc[u].y += v[u].y; acc[u].z += v[u].z; acc[u].w += v[u].w;
      }
    }
    for (; g < G; g += RG) {
      const float4 v = base[(size_t)g * rs];
      acc[0].x += v.x; acc[0].y += v.y; acc[0].z += v.z; acc[0].w += v.w;
    }
  }
#pragma unroll
  for (int h = RU / 2; h >= 1; h /= 2)
#pragma unroll
    for (int u = 0; u < h; ++u) {
      acc[u].x += acc[u + h].x; acc[u].y += acc[u + h].y; acc[u].z += acc[u + h].z; acc[u].w += acc[u + h].w;
    }
  part[r][lq] = acc[0];
  __syncthreads();
  float4 s = make_float4(0, 0, 0, 0);
  if (threadIdx.x < RQ) {
    s = part[0][lq];
#pragma unroll
    for (int k = 1; k < RG; ++k) {
      const float4 v = part[k][lq];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  return s;
}

template <bool OPT>
__global__ __launch_bounds__(256) void wd_reduce_opt(
    const float4* __restrict__ slab, int G, int stride, float4* __restrict__ out, const int* __restrict__ inv,
    float* __restrict__ param, float* __restrict__ s0, float* __restrict__ s1, uint16_t* __restrict__ wt_out,
    const int* __restrict__ wmap, long long* __restrict__ step_ctr, OptHyper hd, OptHyper hw) {
  __shared__ float4 part[RG][RQ];
  __shared__ float gsum[4 * RQ];
  __shared__ long long s_step;
  if (OPT && threadIdx.x == 0) s_step = step_ctr[blockIdx.x] + 1;  // slot read and written by thread 0 only
  const int S4 = stride / 4;
  const int lq = threadIdx.x % RQ;
  const int q = blockIdx.x * RQ + lq;
  const float4 s = slab_column_sum(slab, G, S4, part);
  if (threadIdx.x < RQ) {
    if (!OPT) {
      if (q < S4) out[q] = s;
    } else {
      gsum[4 * lq + 0] = s.x; gsum[4 * lq + 1] = s.y; gsum[4 * lq + 2] = s.z; gsum[4 * lq + 3] = s.w;
    }
  }
  if (!OPT) return;
  __syncthreads();
  const long long step = s_step;
  if (threadIdx.x < 4 * RQ) {
    const int gi = blockIdx.x * 4 * RQ + threadIdx.x;
    const int c = gi < stride ? inv[gi] : -1;
    if (c >= 0) {
      const bool dnn = c < WTOT;
      float a0 = s0[c], a1 = s1[c];
      const float w = opt_update(dnn ? hd : hw, param[c], gsum[threadIdx.x], a0, a1, step);
      s0[c] = a0;
      s1[c] = a1;
      param[c] = w;
      // bf16 weight image: canonical order, or through wmap (canonical -> image offset) for the
      // register-chained kernel's C-ordered LDS image (csrc/wd_chain.hip)
      if (dnn) wt_out[wmap != nullptr ? wmap[c] : c] = __builtin_bit_cast(uint16_t, (bf16)w);
    }
  }
  if (threadIdx.x == 0) step_ctr[blockIdx.x] = step;
}

// Slab-column-order optimizer state (the register-chained trainer): param / s0 / s1 are indexed by slab column and
// wsc[col] says what the column is (-1 padding, -2 wide weight, >= 0 DNN weight with that bf16 weight-image offset).
// No indirection: a thread's state needs no other load's result for its address (the canonical-order kernel above must
// wait for the gradient's inv[] entry, then for param/s0/s1 at that index, then for wmap). sc_load issues its four
// loads unconditionally; what keeps them in front of the gradient's arrival differs by kernel: in wd_reduce_opt_sc the
// reduction's loop and barriers stand between the loads and their use, so they stay where the source has them; in the
// straight-line kernels (wd_opt1_sc, wd_res_opt_sc) nothing does -- the compiler used to sink them into the branch of
// sc_update that uses them, behind the wait for the gradient -- so those consume everything at one point, sc_landed
// (csrc/wd_opt.h), placed behind the last load.
__global__ __launch_bounds__(256) void wd_reduce_opt_sc(const float4* __restrict__ slab, int G, int stride,
                                                        const int* __restrict__ wsc, float* __restrict__ param,
                                                        float* __restrict__ s0, float* __restrict__ s1,
                                                        uint16_t* __restrict__ wt_out, long long* __restrict__ step_ctr,
                                                        OptHyper hd, OptHyper hw) {
  __shared__ float4 part[RG][RQ];
  __shared__ float gsum[4 * RQ];
  __shared__ long long s_step;
  if (threadIdx.x == 0) s_step = step_ctr[blockIdx.x] + 1;
  const int gi = blockIdx.x * 4 * RQ + threadIdx.x;
  ScState st{-1, 0.f, 0.f, 0.f};
  if (threadIdx.x < 4 * RQ) st = sc_load(gi, stride, wsc, param, s0, s1);  // in flight during the reduction
  const int lq = threadIdx.x % RQ;
  const float4 s = slab_column_sum(slab, G, stride / 4, part);
  if (threadIdx.x < RQ) {
    gsum[4 * lq + 0] = s.x; gsum[4 * lq + 1] = s.y; gsum[4 * lq + 2] = s.z; gsum[4 * lq + 3] = s.w;
  }
  __syncthreads();
  if (threadIdx.x < 4 * RQ) sc_update(gi, st, gsum[threadIdx.x], hd, hw, s_step, param, s0, s1, wt_out);
  if (threadIdx.x == 0) step_ctr[blockIdx.x] = s_step;
}

// One slab row (the reference batch's single fused workgroup, or the data-parallel all-reduced gradient): nothing
// to reduce, so one thread per column and a quarter of wd_reduce_opt_sc's workgroups (93 vs 370). Bit-identical:
// the general kernel's column sum of one row adds only zeros to it. Each workgroup owns step slot blockIdx.x, as
// there; a trainer always takes the same path (its slab height is fixed), so the slots it reads stay in step.
// Argument order: everything the first loads need (slab .. s1, step_ctr) is within the 14 preloaded argument dwords
// (csrc/wide_deep.hip), wt_out and the hyper-parameters come by a load issued beside the data loads. The slab entry,
// the state and the step slot are all issued before sc_landed's single wait.
__global__ __launch_bounds__(256) void wd_opt1_sc(const float* __restrict__ slab, int stride,
                                                  const int* __restrict__ wsc, float* __restrict__ param,
                                                  float* __restrict__ s0, float* __restrict__ s1,
                                                  long long* __restrict__ step_ctr, uint16_t* __restrict__ wt_out,
                                                  OptHyper hd, OptHyper hw) {
  __shared__ long long s_step;
  const int gi = blockIdx.x * 256 + threadIdx.x;
  ScState st = sc_load(gi, stride, wsc, param, s0, s1);
  float g[1] = {slab[min(gi, stride - 1)]};
  long long slot = step_ctr[blockIdx.x];  // wave-uniform (a scalar load); thread 0's copy is the one that counts
  sc_landed(st, g, slot, wt_out, hd, hw);
  if (threadIdx.x == 0) s_step = slot + 1;
  __syncthreads();
  if (gi < stride) sc_update(gi, st, g[0], hd, hw, s_step, param, s0, s1, wt_out);
  if (threadIdx.x == 0) step_ctr[blockIdx.x] = s_step;
}

// system-scope (write-through / cache-bypassing) 32-bit stores and loads, for data another XCD or GPU reads
__device__ __forceinline__ void st_sys(float* p, float v) {
  __hip_atomic_store((unsigned int*)p, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ float ld_sys(const float* p) {
  return __uint_as_float(__hip_atomic_load((const unsigned int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
}

// ---- xGMI exchange synchronisation (release / acquire at system scope; bounded, sticky failure)
// A rank publishes epoch e for a chunk with a RELEASE store of the flag (its partial stores are ordered before it:
// they are write-through system-scope stores, drained by the s_waitcnt before the workgroup barrier, and the
// release orders everything the workgroup did before the barrier), and a waiter re-reads the flag with relaxed
// loads and then issues an ACQUIRE fence before loading the partials. The wait is bounded by WALL-CLOCK time
// (s_memrealtime, 100 MHz): a peer that never arrives sets the rank's sticky err flag instead of hanging the
// GPU; every exchange kernel reads err first and does nothing once it is set (no publish, no parameter update,
// no counter advance) -- the peers then time out too, so every rank stops with its weights untouched by
// garbage and the host raises at its next check (FusedWideDeepTrainer._check_exchange).
constexpr long long XG_TIMEOUT_TICKS = 1000ll * 1000 * 1000;  // 10 s at the 100 MHz real-time clock

__device__ __forceinline__ bool xg_failed(const int* err) {
  return __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
}

__device__ __forceinline__ void xg_publish(unsigned int* flag, unsigned int e) {
  __hip_atomic_store(flag, e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// wait until *f reaches epoch e (wrapping compare); false on timeout or when another workgroup already failed
__device__ __forceinline__ bool xg_wait(const unsigned int* f, unsigned int e, int* err) {
  const long long t0 = wall_clock64();
  while ((int)(__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - e) < 0) {
    __builtin_amdgcn_s_sleep(2);
    if (xg_failed(err)) return false;
    if (wall_clock64() - t0 > XG_TIMEOUT_TICKS) {
      __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return false;
    }
  }
  return true;
}

// xGMI exchange peers (see the data-parallel section below)
constexpr int XG_MAXW = 8;
constexpr int XB_THR = 64;               // kernel B: one wave, one float4 column per thread
constexpr int XB_CHUNKS = XB_THR / RQ;   // chunks per kernel-B workgroup
struct XgPeers {
  const float* part[XG_MAXW];  // peer p's [2][stride] partial buffer (p == rank: our own)
  unsigned int* sig[XG_MAXW];   // peer p's flag array [chunks][XG_MAXW] (uncached)
};

// ---- XCD-local slab reduction + optimizer (the register-chained trainer's step on one GPU).
// The fused kernel's workgroups write their 82 KB slab rows into the L2 of the XCD they run on (8 XCDs, 4 MB L2
// each; 32 rows per XCD at grid 256). A one-pass reduction reads every row from every XCD: measured, the fused
// kernel then runs 29-30 us instead of 23 us (its slab writes pay for the lines the previous reduction pulled
// across XCDs), whatever cache policy the reduction's loads use (plain, nontemporal or agent-scope:
// profiles/archive/wd_ab_r2s.txt), and a standalone write + read-back of 21 MB costs 12 us against 3.6 us for re-reading
// a clean slab (tools/micro/launch_floor.hip). So:
//   level 1 (wd_reduce_xcd, 8 x 81 workgroups): workgroup (chunk c = blockIdx / 8) sums, for its 256 columns, only
//     the rows written on ITS OWN XCD (the fused kernel records each workgroup's XCD in xcd_of), ascending -- L2
//     hits -- into the per-XCD partial part[xcd], and stamps ok[xcd][c] with the epoch;
//   level 2 (wd_xcd_opt_sc, one thread per column): sums the per-XCD partials and runs the optimizer.
// Determinism: the dispatcher hands out workgroups round-robin over the XCDs but the starting XCD rotates with
// launch history, so level 2 adds the partials in the order of each XCD's FIRST row, not of XCD id: the same
// association for every rotation. Completeness: an XCD holding rows that no level-1 workgroup of a chunk ran on
// (another placement; XCC ids >= 8) is seen through the epoch stamps and summed from the slab by level 2 itself.
// (One kernel with a last-arriver finalizer measured slower, 12.9 us vs 5.0 + 6.0: its chain of write-through
// stores, counter atomic and partial loads is longer than a kernel boundary.)
constexpr int XMAX = 16;  // XCC_ID range
constexpr int X1C = 64;   // float4 columns per level-1 workgroup (1 KB of each slab row): one per lane of a wave
static_assert(X1C == 64, "wd_reduce_xcd maps lane -> float4 column of its chunk");

// The 4 waves' float4 per lane, summed in wave order: the result is wave 0's (one barrier; red is free again after
// the workgroup's next barrier).
__device__ __forceinline__ float4 fold_waves(float4 a, float4 (&red)[4][X1C]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  red[w][lane] = a;
  __syncthreads();
  float4 sm = red[0][lane];
#pragma unroll
  for (int k2 = 1; k2 < 4; ++k2) {
    sm.x += red[k2][lane].x; sm.y += red[k2][lane].y; sm.z += red[k2][lane].z; sm.w += red[k2][lane].w;
  }
  return sm;
}

__global__ __launch_bounds__(256) void wd_reduce_xcd(const float4* __restrict__ slab, int G, int stride,
                                                     const int* __restrict__ xcd_of, float4* __restrict__ part,
                                                     int* __restrict__ ok, const long long* __restrict__ xep) {
  __shared__ int rows[256];
  __shared__ int wcnt[4];
  __shared__ float4 red[4][X1C];
  const int x = mifx_xcc_id();
  const int S4 = stride / 4, nc1 = (S4 + X1C - 1) / X1C;
  const int c = blockIdx.x / 8;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  // ascending list of the rows written on this XCD
  const bool sel = t < G && xcd_of[t] == x;
  const unsigned long long m = __ballot(sel);
  if (lane == 0) wcnt[w] = __popcll(m);
  __syncthreads();
  int base = 0;
  for (int i = 0; i < w; ++i) base += wcnt[i];
  if (sel) rows[base + __popcll(m & ((1ull << lane) - 1))] = t;
  const int n = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
  __syncthreads();
  if (c >= nc1) return;
  const int q = c * X1C + lane;
  float4 a = make_float4(0, 0, 0, 0);
  if (q < S4) {  // rows w, w + 4, ... of the list, 8 loads in flight (32 rows per XCD at grid 256: one round)
    constexpr int U = 8;
    for (int i0 = w; i0 < n; i0 += 4 * U) {
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + 4 * u;
        v[u] = i < n ? slab[(size_t)rows[i] * S4 + q] : make_float4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w;
      }
    }
  }
  const float4 sm = fold_waves(a, red);
  if (w == 0 && q < S4) part[(size_t)x * S4 + q] = sm;
  if (t == 0) ok[x * nc1 + c] = (int)(xep[0] + 1);
}

// ---- residue-class two-level reduction (the register-chained trainer's default step tail on one GPU).
// Level 1 (wd_reduce_res, 8 x nchunks workgroups): workgroup j sums, for its 256 columns (chunk j / 8), the slab rows
// b == j (mod 8), ascending, into part[j % 8]. Level 2 (wd_res_opt_sc, one thread per column): part[0] + ... +
// part[7] in that order, then the optimizer. Both sums run over fixed row sets in a fixed order whatever the
// placement, so the step is deterministic with no record of where anything ran, and neither kernel has a dependent
// load before its data loads (wd_reduce_xcd first reads xcd_of, wd_xcd_opt_sc orders the XCDs and checks epoch
// stamps). Locality: the dispatcher hands workgroups to the XCDs round-robin from a pointer that carries over between
// launches, and both the fused kernel's grid (256) and this one's (8 x nchunks) are multiples of 8, so fused
// workgroup b and level-1 workgroup j with j == b (mod 8) run on the same XCD and the rows are L2 hits -- as in
// wd_reduce_xcd. A placement that breaks this only costs cross-XCD reads, never a different result.

// Level 1: float4 column q summed over the slab rows == k (mod 8), ascending; wave w takes rows k + 8 (w + 4 i) and
// the waves are folded in order. The sum is returned to wave 0.
__device__ __forceinline__ float4 res_column_sum(const float4* __restrict__ slab, int G, int S4, int k, int q,
                                                 float4 (&red)[4][X1C]) {
  const int w = threadIdx.x >> 6;
  float4 a = make_float4(0, 0, 0, 0);
  if (q < S4) {  // rows k + 8 (w + 4 i): 8 loads in flight per thread (32 rows per residue at G = 256: one round)
    constexpr int U = 8;
    for (int i0 = k + 8 * w; i0 < G; i0 += 32 * U) {
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int r = i0 + 32 * u;
        v[u] = r < G ? slab[(size_t)r * S4 + q] : make_float4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w;
      }
    }
  }
  return fold_waves(a, red);
}

__global__ __launch_bounds__(256) void wd_reduce_res(const float4* __restrict__ slab, int G, int stride,
                                                     float4* __restrict__ part) {
  __shared__ float4 red[4][X1C];
  const int S4 = stride / 4;
  const int k = blockIdx.x & 7, c = blockIdx.x >> 3;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int q = c * X1C + lane;
  const float4 sm = res_column_sum(slab, G, S4, k, q, red);
  if (w == 0 && q < S4) part[(size_t)k * S4 + q] = sm;
}

// Level 2 for column gi: part[0][gi] + ... + part[7][gi] in residue order. load(p) reads one partial: a plain load
// after a kernel boundary, an agent-scope load inside wd_reduce_res_fused.
// The loads are unconditional at the column clamped into [0, stride) (straight-line code, issued back to back; a
// thread past the last column stores nothing), and separate from the fold so that a kernel can issue its other
// loads between the two.
template <class Load>
__device__ __forceinline__ void res_partial_load(Load load, const float* part, int gi, int stride, float (&pv)[8]) {
  const int gc = min(gi, stride - 1);
#pragma unroll
  for (int x = 0; x < 8; ++x) pv[x] = load(part + (size_t)x * stride + gc);
}
__device__ __forceinline__ float res_partial_fold(const float (&pv)[8]) {
  float g = pv[0];
#pragma unroll
  for (int x = 1; x < 8; ++x) g += pv[x];
  return g;
}

// level 2 of the residue-class reduction, one thread per column
__global__ __launch_bounds__(256) void wd_res_opt_sc(const float* __restrict__ part, int stride,
                                                     const int* __restrict__ wsc, float* __restrict__ param,
                                                     float* __restrict__ s0, float* __restrict__ s1,
                                                     long long* __restrict__ step_ctr, uint16_t* __restrict__ wt_out,
                                                     OptHyper hd, OptHyper hw) {
  // One round trip: part .. s1 and step_ctr are preloaded argument dwords (wt_out and the hyper-parameters are loaded
  // beside the data), and the 8 partials, the state and the step slot are all issued before sc_landed's wait.
  const int t = threadIdx.x, gi = blockIdx.x * 256 + t;
  long long slot = step_ctr[blockIdx.x];
  float pv[8];
  res_partial_load([](const float* p) { return *p; }, part, gi, stride, pv);
  ScState st = sc_load(gi, stride, wsc, param, s0, s1);
  sc_landed(st, pv, slot, wt_out, hd, hw);
  const long long step = slot + 1;
  const float g = res_partial_fold(pv);
  if (gi < stride) sc_update(gi, st, g, hd, hw, step, param, s0, s1, wt_out);
  if (t == 0) step_ctr[blockIdx.x] = step;
  if (blockIdx.x == 0) fan_out_slots<256>(step_ctr, gridDim.x, step);
}

// Both levels in ONE launch (opt-in, MIFX_WD_RES_FUSED=1): level 1 exactly as wd_reduce_res; the LAST of a
// chunk's 8 residue workgroups to finish (a per-chunk ticket) then adds the chunk's 8 partials in residue order and
// applies the optimizer to its 256 columns -- wd_res_opt_sc's sums and state updates, bit for bit, without the
// second launch. The partials are stored and loaded at agent scope (coherent across the XCDs' L2s) and completed
// before the ticket increment; the last arriver resets the ticket. No workgroup ever waits for another.
__global__ __launch_bounds__(256) void wd_reduce_res_fused(const float4* __restrict__ slab, int G, int stride,
                                                           float* __restrict__ part, int* __restrict__ ticket,
                                                           const int* __restrict__ wsc, float* __restrict__ param,
                                                           float* __restrict__ s0, float* __restrict__ s1,
                                                           uint16_t* __restrict__ wt_out,
                                                           long long* __restrict__ step_ctr, OptHyper hd, OptHyper hw) {
  __shared__ float4 red[4][X1C];
  __shared__ int last;
  const int S4 = stride / 4, nc1 = (S4 + X1C - 1) / X1C;
  const int k = blockIdx.x & 7, c = blockIdx.x >> 3;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int q = c * X1C + lane;
  const float4 sm = res_column_sum(slab, G, S4, k, q, red);
  if (w == 0 && q < S4) {
    float* dst = part + (size_t)k * stride + 4 * q;
    __hip_atomic_store(dst + 0, sm.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(dst + 1, sm.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(dst + 2, sm.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(dst + 3, sm.w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (t == 0) {
    // wave 0 made the partial stores; they are agent-scope (coherent across the XCDs' L2s), so completing them
    // (vmcnt 0) before the increment orders them -- a release fence here (an L2 writeback) measured ~5 us slower
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    __builtin_amdgcn_s_waitcnt(0);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    const int old = __hip_atomic_fetch_add(ticket + c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = old == 7;
  }
  __syncthreads();
  if (!last) return;
  const int gi = c * 256 + t;
  const long long step = step_ctr[c] + 1;
  const auto ld_agent = [](const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  float pv[8];
  res_partial_load(ld_agent, part, gi, stride, pv);
  const ScState st = sc_load(gi, stride, wsc, param, s0, s1);
  const float g = res_partial_fold(pv);
  if (gi < stride) sc_update(gi, st, g, hd, hw, step, param, s0, s1, wt_out);
  if (t == 0) {
    step_ctr[c] = step;
    __hip_atomic_store(ticket + c, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (c == 0) fan_out_slots<256>(step_ctr, nc1, step);
}

// Publish half of the xGMI exchange for wd_xcd_opt_sc's 256 columns: store the local sum g of column gi into half
// (epoch & 1) of this rank's IPC buffer, then -- the stores acknowledged, the workgroup past its barrier -- stamp the
// flags of the 4 RQ-float4 exchange chunks the columns make up, in every peer. Returns the exchange epoch.
__device__ __forceinline__ long long xcd_publish(float g, int gi, int stride, const XgPeers& peers, int world, int rank,
                                                 const long long* xctr) {
  const int t = threadIdx.x;
  const long long ex = xctr[blockIdx.x] + 1;
  if (gi < stride) {
    st_sys((float*)peers.part[rank] + (size_t)(ex & 1) * stride + gi, g);
    __builtin_amdgcn_s_waitcnt(0);  // acknowledged before the chunk flags below
  }
  __syncthreads();
  const int nch = (stride / 4 + RQ - 1) / RQ;
  if (t < 4 * world) {
    const int cc = 4 * blockIdx.x + t / world, p = t % world;
    if (cc < nch) xg_publish(peers.sig[p] + cc * XG_MAXW + rank, (unsigned int)ex);
  }
  return ex;
}

// level 2: one thread per slab column. MODE 0: plain sum into out; 1: optimizer on slab-order state; 2: xGMI data
// parallelism, publish half -- store the local sum into half (epoch & 1) of this rank's IPC buffer and stamp the 4
// RQ-float4 chunks' flags in every peer, no wait (wd_xgmi_gather_opt waits, gathers and applies the optimizer in
// one-wave workgroups); 3: the same with the wait, the gather over xGMI and the optimizer in this kernel (opt-in,
// MIFX_XGMI_FUSED_WAIT=1: one launch fewer, but 256-thread workgroups spin on the peers).
template <int MODE>
__global__ __launch_bounds__(256) void wd_xcd_opt_sc(const float* __restrict__ part, const int* __restrict__ ok,
                                                     const float* __restrict__ slab, int G, int stride,
                                                     const int* __restrict__ xcd_of, long long* __restrict__ xep,
                                                     float* __restrict__ out, const int* __restrict__ wsc,
                                                     float* __restrict__ param, float* __restrict__ s0,
                                                     float* __restrict__ s1, uint16_t* __restrict__ wt_out,
                                                     long long* __restrict__ step_ctr, OptHyper hd, OptHyper hw,
                                                     XgPeers peers, int world, int rank,
                                                     long long* __restrict__ xctr,
                                                     const unsigned int* __restrict__ my_sig,
                                                     int* __restrict__ err) {
  __shared__ int first[XMAX];
  __shared__ int order[XMAX];
  __shared__ int nord;
  __shared__ long long s_e, s_step;
  __shared__ int s_bad;
  const int t = threadIdx.x;
  constexpr bool opt = MODE == 1 || MODE == 3;
  if (MODE >= 2) {  // the exchange already failed on this rank: touch nothing (see xg_wait)
    if (t == 0) s_bad = xg_failed(err) ? 1 : 0;
    __syncthreads();
    if (s_bad) return;
  }
  if (t < XMAX) first[t] = 1 << 30;
  if (t == 0) {
    s_e = xep[blockIdx.x] + 1;
    if (opt) s_step = step_ctr[blockIdx.x] + 1;
  }
  const int gi = blockIdx.x * 256 + t;
  const int S4 = stride / 4, nc1 = (S4 + X1C - 1) / X1C;
  const int c1 = min(gi, stride - 1) / 4 / X1C;
  // everything in flight at once: the row XCDs, the 8 stamps and 8 partials of this column, the optimizer state
  const int xo = t < G ? xcd_of[t] : -1;
  int okv[8];
  float pv[8];
#pragma unroll
  for (int x = 0; x < 8; ++x) {
    okv[x] = ok[x * nc1 + c1];
    pv[x] = gi < stride ? part[(size_t)x * stride + gi] : 0.f;
  }
  ScState st{-1, 0.f, 0.f, 0.f};
  if (opt) st = sc_load(gi, stride, wsc, param, s0, s1);
  __syncthreads();
  if (xo >= 0) atomicMin(&first[xo], t);
  __syncthreads();
  if (t < XMAX) {  // XCDs holding rows, by first row: lane t's rank among the distinct valid first rows (a serial
                   // insertion sort by one lane cost ~1.5 us of dependent LDS round trips per workgroup)
    const int f = first[t];
    const bool valid = f < (1 << 30);
    int rank = 0;
#pragma unroll
    for (int y = 0; y < XMAX; ++y) rank += first[y] < f ? 1 : 0;
    if (valid) order[rank] = t;
    const unsigned long long vm = __ballot(valid);
    if (t == 0) nord = __popcll(vm);
  }
  __syncthreads();
  const int e = (int)s_e;
  float g = 0.f;
  if (gi < stride) {
    for (int k2 = 0; k2 < nord; ++k2) {
      const int xx = order[k2];
      float v = 0.f;
#pragma unroll
      for (int x = 0; x < 8; ++x)
        if (x == xx) v = pv[x];
      if (!(xx < 8 && okv[xx & 7] == e)) {  // no level-1 workgroup ran on XCD xx for this chunk: its rows, here
        v = 0.f;
        for (int r = 0; r < G; ++r)
          if (xcd_of[r] == xx) v += slab[(size_t)r * stride + gi];
      }
      g += v;
    }
    if (MODE == 0) out[gi] = g;
    if (MODE == 1) sc_update(gi, st, g, hd, hw, s_step, param, s0, s1, wt_out);
  }
  if (MODE == 2)  // publish only: the wait, gather and optimizer run in wd_xgmi_gather_opt (one-wave waiters); the
                  // exchange epoch slot b is advanced by the gather kernel's block b
    xcd_publish(g, gi, stride, peers, world, rank, xctr);
  if (MODE == 3) {
    const long long ex = xcd_publish(g, gi, stride, peers, world, rank, xctr);  // exchange epoch (own slot)
    const unsigned int uex = (unsigned int)ex;
    const size_t hoff = (size_t)(ex & 1) * stride;
    // then wait for every peer's stamp of each of the 4 chunks
    const int nch = (stride / 4 + RQ - 1) / RQ;
    if (t < 4 * world) {
      const int cc = 4 * blockIdx.x + t / world, p = t % world;
      if (cc < nch && !xg_wait(my_sig + cc * XG_MAXW + p, uex, err)) s_bad = 1;
    }
    __syncthreads();
    if (s_bad) return;  // a peer never arrived: no update, no counter advance (err is set)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // the peers' partials published before their flags
    if (gi < stride) {
      float pv2[XG_MAXW];
#pragma unroll
      for (int p = 0; p < XG_MAXW; ++p) pv2[p] = p < world ? ld_sys(peers.part[p] + hoff + gi) : 0.f;
      float gs = pv2[0];
#pragma unroll
      for (int p = 1; p < XG_MAXW; ++p)
        if (p < world) gs += pv2[p];
      sc_update(gi, st, gs, hd, hw, s_step, param, s0, s1, wt_out);
    }
    __syncthreads();
    if (t == 0) xctr[blockIdx.x] = ex;
    if (blockIdx.x == 0) fan_out_slots<256>(xctr, gridDim.x, ex);
  }
  __syncthreads();
  if (t == 0) {
    xep[blockIdx.x] = s_e;
    if (opt) step_ctr[blockIdx.x] = s_step;
  }
  if (blockIdx.x == 0) fan_out_slots<256, opt>(xep, gridDim.x, s_e, step_ctr, s_step);
}

// ---- data parallelism over xGMI: one-shot cross-GPU exchange of the local gradient, no host collective
// (mifx/parallel/xgmi.py). Two kernels per step after the fused fwd/bwd:
//   A wd_reduce_xgmi_publish (322 workgroups): workgroup c sums its RQ float4 columns ("chunk c") over the G slab
//     rows (as wd_reduce_opt, fixed order), stores the chunk into half (epoch & 1) of this rank's IPC-shared
//     partial buffer with system-scope (write-through) stores, waits for their completion and publishes epoch e
//     for chunk c into every peer's flag array (uncached memory): sig[c][rank] = e. No waiting.
//   B wd_xgmi_gather_opt (81 one-wave workgroups, 4 chunks each): waits until all ranks published e for its
//     chunks (bounded spin: a peer that never arrives sets err, no wave can hang), loads the world partials from
//     the peers' HBM over xGMI with system-scope loads, sums them in rank order -- identical on every rank, so
//     the replicas stay bit-identical -- and runs the optimizer on its columns.
// No cache-wide writeback or invalidate anywhere. The waiting kernel is small on purpose: it never holds the CUs
// another rank's fused kernel needs (ranks sharing a GPU in tests, or anything else running on the node).
// Double buffering by epoch parity makes one flag per epoch enough: rank r rewrites half e & 1 of chunk c only in
// epoch e + 2, after its epoch e + 1 kernel B saw every peer's e + 1 flag for chunk c, which that peer published
// after its epoch-e kernel B (its reads of chunk c) completed. The W&D gradient is one 82 KB bucket: every GPU
// reads 7 x 82 KB over 7 point-to-point xGMI links in one round.


// epoch of the coming exchange: xctr holds the last completed one (per-workgroup slots of kernel B; kernel A
// reads slot 0, written by kernel B's workgroup 0 of the previous step)
__global__ __launch_bounds__(256) void wd_reduce_xgmi_publish(const float4* __restrict__ slab, int G, int stride,
                                                              XgPeers peers, int world, int rank,
                                                              const long long* __restrict__ xctr,
                                                              const int* __restrict__ err) {
  __shared__ float4 part[RG][RQ];
  __shared__ int s_bad;
  if (threadIdx.x == 0) s_bad = xg_failed(err) ? 1 : 0;
  __syncthreads();
  if (s_bad) return;  // failed exchange: publish nothing (the peers time out and stop too)
  const int S4 = stride / 4;
  const int q = blockIdx.x * RQ + threadIdx.x % RQ;
  const long long e = xctr[0] + 1;
  const float4 s = slab_column_sum(slab, G, S4, part);
  if (threadIdx.x < RQ && q < S4) {
    float* dst = (float*)peers.part[rank] + (size_t)(e & 1) * stride + 4 * q;
    st_sys(dst + 0, s.x);
    st_sys(dst + 1, s.y);
    st_sys(dst + 2, s.z);
    st_sys(dst + 3, s.w);
    __builtin_amdgcn_s_waitcnt(0);  // the chunk's stores acknowledged before the flag below
  }
  __syncthreads();
  if (threadIdx.x < world) xg_publish(peers.sig[threadIdx.x] + blockIdx.x * XG_MAXW + rank, (unsigned int)e);
}

template <bool OPT>
__global__ __launch_bounds__(XB_THR) void wd_xgmi_gather_opt(
    int stride, XgPeers peers, int world, const unsigned int* __restrict__ my_sig, int* __restrict__ err,
    long long* __restrict__ xctr, float4* __restrict__ out, const int* __restrict__ wsc, float* __restrict__ param,
    float* __restrict__ s0, float* __restrict__ s1, uint16_t* __restrict__ wt_out,
    long long* __restrict__ step_ctr, OptHyper hd, OptHyper hw) {
  const int t = threadIdx.x;
  // one wave: a lane-uniform early exit needs no barrier
  if (xg_failed(err)) return;
  const int q0 = blockIdx.x * XB_THR + t;
  ScState st[4];
  if (OPT) {  // slab-order optimizer state, in flight during the wait
#pragma unroll
    for (int j = 0; j < 4; ++j) st[j] = sc_load(4 * q0 + j, stride, wsc, param, s0, s1);
  }
  const long long e = xctr[blockIdx.x] + 1;  // one wave: every lane reads the slot, no LDS broadcast needed
  const long long step = OPT ? step_ctr[blockIdx.x] + 1 : 0;
  const unsigned int ue = (unsigned int)e;
  const int nchunks = (stride / 4 + RQ - 1) / RQ;
  bool ok = true;
  {  // lane t waits for flag (chunk XB_CHUNKS * blockIdx.x + t / world, rank t % world)
    const int c = XB_CHUNKS * blockIdx.x + t / max(world, 1);
    if (t < XB_CHUNKS * world && c < nchunks) ok = xg_wait(my_sig + c * XG_MAXW + t % world, ue, err);
  }
  // any lane's timeout stops the whole wave: no update, no counter advance (err is set)
  if (__ballot(!ok) != 0ull) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // the peers' partials published before their flags
  const int S4 = stride / 4;
  const int q = blockIdx.x * XB_THR + t;
  if (q < S4) {
    const size_t off = (size_t)(e & 1) * stride + 4 * q;
    float v[XG_MAXW][4];
#pragma unroll
    for (int p = 0; p < XG_MAXW; ++p)
      if (p < world) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[p][j] = ld_sys(peers.part[p] + off + j);
      }
    float g4[4] = {v[0][0], v[0][1], v[0][2], v[0][3]};
#pragma unroll
    for (int p = 1; p < XG_MAXW; ++p)
      if (p < world) {
#pragma unroll
        for (int j = 0; j < 4; ++j) g4[j] += v[p][j];
      }
    if (!OPT) {
      out[q] = make_float4(g4[0], g4[1], g4[2], g4[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) sc_update(4 * q + j, st[j], g4[j], hd, hw, step, param, s0, s1, wt_out);
    }
  }
  __syncthreads();  // every lane read its slots before lane 0 moves them on
  if (t == 0) {
    xctr[blockIdx.x] = e;
    if (OPT) step_ctr[blockIdx.x] = step;
  }
  if (blockIdx.x == 0) fan_out_slots<XB_THR, OPT>(xctr, gridDim.x, e, step_ctr, step);
}
