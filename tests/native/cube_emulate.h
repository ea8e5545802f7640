// The device grid builders' enumeration (csrc/rt_gridbuild.h gb_bin_quarter)
// on the CPU, host only: the per-lane functions of csrc/rt_cgbuild.h run lane
// by lane in the kernels' order -- the block's quarters, each quarter's tiles
// ascending, each tile's cells by lane.  The one copy the device-builder
// checks (cg_device_check.cpp, sg_device_check.cpp) share.
#pragma once

#include <vector>

#include "rt_cgbuild.h"

namespace cube_emulate {

// The patch tables of one N on the host, and the view the lane functions take.
struct Tables {
  std::vector<rtk::CubePatch> faces, blocks, tiles;
  std::vector<double> cell;
  rtk::CubeTables view{};
  explicit Tables(int N) {
    int NT = 0, NB = 0;
    rtk::cube_tables(N, faces, blocks, tiles, cell, NT, NB);
    view = rtk::CubeTables{faces.data(), blocks.data(), tiles.data(), cell.data(), N, NT, NB};
  }
  Tables(const Tables &) = delete;
  int nblocks() const { return 6 * view.NB * view.NB; }
};

// fn(cell) for every cell the disk k lists in block b (which it meets, cg_block).
template <class F>
void block_cells(const rtk::CgDisk &k, const rtk::CubeTables &T, int b, F fn) {
  const bool wide = rtk::cg_wide(k);
  const int f = b / (T.NB * T.NB), bj = (b / T.NB) % T.NB, bi = b % T.NB;
  unsigned long long tmask = 0, imask = 0;
  for (int lane = 0; lane < 64; lane++) {
    bool tm, inside;
    rtk::cg_tile(k, T, f, bi, bj, lane, tm, inside);
    if (tm) tmask |= 1ull << lane;
    if (inside) imask |= 1ull << lane;
  }
  for (int q = 0; q < 4; q++) {  // quarter items: tiles of rows 2q, 2q + 1 of the block
    unsigned long long qmask = tmask & (0xffffull << (16 * q));
    while (qmask) {
      const int tl = __builtin_ctzll(qmask);
      qmask &= qmask - 1;
      for (int lane = 0; lane < 64; lane++) {
        const int gc = rtk::cg_cell(k, wide, T, f, bi, bj, tl, lane, (imask >> tl) & 1ull);
        if (gc >= 0) fn(gc);
      }
    }
  }
}

}  // namespace cube_emulate
