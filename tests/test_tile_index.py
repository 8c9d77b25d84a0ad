"""csrc/tile_index.h, the integer geometry of the MFMA GEMM kernels (tile order, LDS image layouts, the counted-wait
immediate), compiled for the host and checked exhaustively. This is the check of the formulas the kernels run;
tools/lds_banks_tn.py is the search that found the rotations."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include "tile_index.h"
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

static bool xcd_bijective() {
  for (int nwg = 1; nwg <= 600; ++nwg) {
    std::vector<int> seen(nwg, 0);
    for (int bid = 0; bid < nwg; ++bid) {
      const int t = xcd_tile(bid, nwg);
      if (t < 0 || t >= nwg || seen[t]++) return false;
    }
  }
  return true;
}

static bool grouped_bijective() {
  for (int nb_m = 1; nb_m <= 9; ++nb_m)
    for (int nb_n = 1; nb_n <= 9; ++nb_n) {
      std::set<std::pair<int, int>> seen;
      for (int tile = 0; tile < nb_m * nb_n; ++tile) {
        const TileMN t = grouped_tile(tile, nb_m, nb_n);
        if (t.m < 0 || t.m >= nb_m || t.n < 0 || t.n >= nb_n || !seen.insert({t.m, t.n}).second) return false;
      }
    }
  return true;
}

// slot_of<CPR>(t, .) permutes [0, CPR) and tok_img_src (ld = 0, col0 = 0: 8 x the logical chunk) undoes it
template <int CPR>
static bool rotation_invertible() {
  for (int t = 0; t < 64; ++t) {
    std::set<int> seen;
    for (int c = 0; c < CPR; ++c) {
      const int p = slot_of<CPR>(t, c);
      if (p < 0 || p >= CPR || !seen.insert(p).second) return false;
      if (tok_img_src<CPR>(t, p, 0, 0) != 8 * c) return false;
      if (tok_img_src<CPR>(t, p, 1000, 40) != 1000 * t + 40 + 8 * c) return false;
      if (tok_slot<CPR>(t, c) != t * CPR + p) return false;
    }
  }
  return true;
}

// every 32-lane half of every transposed fragment read touches 64 distinct 4-byte banks: lane (r = lane & 15,
// h = lane >> 4) reads 8 bytes (two banks) at tok_frag_off of token row 32 ks + 8 h + (r >> 2) (+ 4: second read),
// chunk c0 + (p >> 1), p = r & 3, for each pair of chunks c0 of the row (the access pattern of tools/lds_banks_tn.py)
template <int CPR>
static bool banks_distinct() {
  for (int ks = 0; ks < 2; ++ks)
    for (int second = 0; second < 2; ++second)
      for (int half = 0; half < 2; ++half)
        for (int c0 = 0; c0 + 1 < CPR; c0 += 2) {
          std::set<int> banks;
          for (int lane = 32 * half; lane < 32 * half + 32; ++lane) {
            const int r = lane & 15, h = lane >> 4, p = r & 3;
            const int t = 32 * ks + 8 * h + (r >> 2) + 4 * second;
            const int off = tok_frag_off<CPR>(t, c0 + (p >> 1), p);
            if (off % 8 != 0 || off < 0 || off + 8 > 64 * CPR * 16) return false;
            banks.insert((off / 4) % 64);
            banks.insert((off / 4 + 1) % 64);
          }
          if (banks.size() != 64) return false;
        }
  return true;
}

template <int CPR>
static void report() {
  std::printf("perm %d %d\n", CPR, (int)rotation_invertible<CPR>());
  std::printf("banks %d %d\n", CPR, (int)banks_distinct<CPR>());
}

static bool vm_wait_decodes() {
  for (int n = 0; n < 64; ++n) {
    const int imm = vm_wait(n);
    const int vmcnt = (imm & 15) | (((imm >> 14) & 3) << 4), expcnt = (imm >> 4) & 7, lgkmcnt = (imm >> 8) & 15;
    if (vmcnt != n || expcnt != 7 || lgkmcnt != 15 || (imm & ~0xcf7f) != 0) return false;
  }
  return true;
}
static_assert(vm_wait(0) == 0x0f70 && vm_wait(63) == 0xcf7f, "constant expression");

int main() {
  std::printf("xcd %d\n", (int)xcd_bijective());
  std::printf("grouped %d\n", (int)grouped_bijective());
  report<4>();
  report<8>();
  report<12>();
  report<16>();
  report<24>();
  std::printf("vm_wait %d\n", (int)vm_wait_decodes());
  bool swz_ok = true;  // swz(row, .) permutes the 8 chunks of a row and is its own inverse
  for (int row = 0; row < 256; ++row)
    for (int c = 0; c < 8; ++c) {
      swz_ok = swz_ok && swz(row, swz(row, c)) == c && swz(row, c) >= 0 && swz(row, c) < 8;
      swz_ok = swz_ok && row_img_src(row, swz(row, c), 512, 768) == (512 + row) * 768 + 8 * c;
    }
  std::printf("swz %d\n", (int)swz_ok);
  return 0;
}
'''

WIDTHS = (4, 8, 12, 16, 24)  # 16-byte chunks per token row the kernels instantiate


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_index")
    src, exe = d / "tile_index_check.cpp", d / "tile_index_check"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "csrc"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    rep = {}
    for line in out.splitlines():
        *key, val = line.split()
        rep[tuple(key)] = int(val)
    return rep


def test_xcd_tile_is_a_bijection_for_every_grid_size(report):
    assert report[("xcd",)] == 1


def test_grouped_order_covers_the_tile_grid_once(report):
    assert report[("grouped",)] == 1


def test_swizzle_is_an_involution_and_the_dma_source_applies_it(report):
    assert report[("swz",)] == 1


@pytest.mark.parametrize("cpr", WIDTHS)
def test_rotation_is_a_permutation_and_the_dma_source_inverts_it(report, cpr):
    assert report[("perm", str(cpr))] == 1


@pytest.mark.parametrize("cpr", WIDTHS)
def test_transposed_fragment_reads_are_bank_conflict_free(report, cpr):
    assert report[("banks", str(cpr))] == 1


def test_vm_wait_encodes_vmcnt_only(report):
    assert report[("vm_wait",)] == 1
