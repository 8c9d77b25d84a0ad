// Integer geometry shared by the MFMA GEMM kernels: which output tile a workgroup owns, where a 16-byte chunk of an
// operand sits in its LDS image, and the s_waitcnt immediate of a counted wait. Pure integer functions, host and
// device: the kernels include this through mfma_stage.h, and tests/test_tile_index.py compiles it with a plain C++
// compiler and checks every property stated below exhaustively.
#pragma once

#ifdef __HIPCC__
#define MIFX_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MIFX_HD inline
#endif

namespace {

// XCD-aware bijective tile order (CDNA guide section 5, "XCD swizzle"): workgroups are dispatched round-robin over
// the 8 XCDs, so workgroup `bid` of `nwg` is remapped such that each XCD walks a contiguous run of tiles (sharing
// operand panels in its own L2). The first nwg % 8 XCDs take one tile more; a bijection of [0, nwg) for every nwg.
MIFX_HD constexpr int xcd_tile(int bid, int nwg) {
  const int xcd = bid % 8, q = nwg / 8, r = nwg % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
}

// Grouped tile order: runs of GM m-blocks x all n-blocks, m fastest (the last group may be shorter), so a run of
// consecutive tiles covers a GM x (run / GM) block of the output and re-reads few operand strips per K-tile.
struct TileMN {
  int m, n;  // m-block, n-block
};
template <int GM = 4>
MIFX_HD constexpr TileMN grouped_tile(int tile, int nb_m, int nb_n) {
  const int per_group = GM * nb_n, group = tile / per_group, first_m = group * GM;
  const int gsz = nb_m - first_m < GM ? nb_m - first_m : GM, wi = tile - group * per_group;
  return {first_m + wi % gsz, wi / gsz};
}

// ---- row-major image: [rows][64] bf16, 128-byte rows, the 16-byte chunk index XOR-swizzled by (row >> 1) & 7. The
// 16 rows of an MFMA fragment read (ds_read_b128, lanes l & 15) then hit 16 distinct 16-byte slots of the 256-byte
// bank row. DMA destinations are lane-linear (slot s = 8 row + physical chunk), so the swizzle is applied to each
// lane's SOURCE address and to the fragment reads.
MIFX_HD constexpr int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }
// element offset, in a row-major operand of leading dimension ld whose image starts at row row0, of the chunk that
// lands at physical chunk pc of image row `row` (DMA slot s: row = s >> 3, pc = s & 7)
MIFX_HD constexpr int row_img_src(int row, int pc, int row0, int ld) { return (row0 + row) * ld + 8 * swz(row, pc); }

// ---- token-major image: [64 token rows][CPR 16-byte chunks], the reduction index is the ROW. MFMA fragments (8
// consecutive tokens of one column per lane) are read with ds_read_b64_tr_b16: a 16-lane group supplies 4 token rows x
// 16 columns and each lane receives one column's 4 tokens; two reads, 4 rows apart, make the 8-token fragment. The
// chunks of row t sit rotated by rot(t) inside their row (again applied to the DMA SOURCE address), chosen so that
// every 32-lane half of every fragment read touches 64 distinct banks (found by tools/lds_banks_tn.py).
template <int CPR>
MIFX_HD constexpr int rot(int t) {
  static_assert(CPR == 4 || CPR == 8 || CPR == 12 || CPR == 16 || CPR == 24, "chunks per token row");
  if constexpr (CPR == 4) return 2 * ((t >> 3) & 1);  // 64-byte rows: the 16-lane groups of a half read tokens 8
                                                      // apart, shifted 8 banks
  if constexpr (CPR == 8) return ((t & 3) + 4 * ((t >> 3) & 3)) & 7;
  if constexpr (CPR == 12) return (2 * ((t >> 3) & 3)) % 12;
  if constexpr (CPR == 24) return (6 * (t & 3) + 6 * ((t >> 3) & 3)) % 24;
  return (2 * (t & 3) + 8 * ((t >> 3) & 3)) & 15;
}
template <int CPR>
MIFX_HD constexpr int slot_of(int t, int c) {  // physical chunk of logical chunk c in row t
  const int p = c + rot<CPR>(t);
  return p >= CPR ? p - CPR : p;
}
// The inverse of slot_of, as the DMA needs it: element offset, in a token-major operand of leading dimension ld whose
// image starts at column col0, of the chunk that lands at physical chunk p of token row t (DMA slot s: t = s / CPR,
// p = s % CPR), relative to the K-tile's first token row. ld = 0, col0 = 0 gives 8 x the logical chunk.
template <int CPR>
MIFX_HD constexpr int tok_img_src(int t, int p, int ld, int col0) {
  int c = p - rot<CPR>(t);
  c = c < 0 ? c + CPR : c;
  return t * ld + col0 + 8 * c;
}
// 16-byte slot, counted from the image's start, of logical chunk c of token row t
template <int CPR>
MIFX_HD constexpr int tok_slot(int t, int c) { return t * CPR + slot_of<CPR>(t, c); }
// Transposed fragment read of the 16 columns from chunk c0 (= column / 8): lane (r = lane & 15, h = lane >> 4) of
// 32-deep k-step ks addresses token row t = 32 ks + 8 h + (r >> 2) -- and t + 4 in the second read -- and there the 8
// bytes p & 1 of chunk c = c0 + (p >> 1), p = r & 3. Byte offset inside the image:
template <int CPR>
MIFX_HD constexpr int tok_frag_off(int t, int c, int p) { return tok_slot<CPR>(t, c) * 16 + 8 * (p & 1); }

// s_waitcnt immediate (gfx9 encoding) that waits for vmcnt <= n only: vmcnt is split over bits [3:0] and [15:14],
// expcnt (bits [6:4]) and lgkmcnt (bits [11:8]) are left at their maxima, i.e. not waited on. Outside the counter's
// range the trap is not a constant expression, so the build fails where the immediate is formed.
MIFX_HD constexpr int vm_wait(int n) {
  if (n < 0 || n >= 64) __builtin_trap();
  return (n & 15) | (7 << 4) | (15 << 8) | ((n >> 4) << 14);
}

}  // namespace
