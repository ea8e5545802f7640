// rt_gridbuild.h -- the device builders of the cube-map direction grids:
// camera grids (per launch), sphere grids and light grids (at upload).
// Included by rt_kernel.hip only, after rt_device.h and rt_cgbuild.h.
//
// Every grid lists, per cell, the spheres whose grown disk seen from the
// grid's point meets the cell -- build_point_grid / build_sphere_grids /
// build_light_grid (rt_lightgrid.cpp) on the GPU, by the host builder's patch
// hierarchy and tests (faces, blocks of 8 x 8 tiles, tiles of 8 x 8 cells -- a
// tile well inside a disk takes all its cells untested -- cells against the
// per-(i, j) table), the same patches and margins (rt_cgbuild.h, per lane).
// Both builders run the same two passes over a GridJob:
//   pass 1 (gb_list_disks)   a wave per (grid, sphere): its disks and the
//                            (disk, block) pairs they meet
//   pass 2 (gb_bin_quarter)  a wave per quarter of a pair: tiles, cells, and
//                            for every listed cell the builder's sink (the
//                            camera grids 4 tiles a round, the others 1)
// and then sort each list (gb_insertion_sort).  They differ in where a grid's
// point comes from, in which spheres count as global, and in the sink: a slot
// of ent[cell][K] (camera grids) or a CSR list counted, scanned, then filled
// (sphere and light grids).
#pragma once

#include "rt_cgbuild.h"
#include "rt_device.h"

namespace rtk {

// What the passes work on: the spheres, the patch tables, and pass 1's output
// (pass 2's input) for the ng grids in flight.
struct GridJob {
  const SphGeo *geo;
  const double *rad;
  CubeTables tab;
  CgDisk *disks;     // [grid][sphere][side]
  int2 *pairs;       // [grid][maxp] (disk, block) pairs whose block the disk meets
  unsigned *npairs;  // [grid * stride] their counts, dropped pairs included (a line of its own per grid)
  int n, ng, maxp;
};

// Pass 1 body, one wave: the disks of sphere s seen from grid `grid` (v its
// view; `sides` of them, one for a global sphere), and every (disk, block)
// pair whose face and block patches the disk meets (a lane per block, one
// atomic on the grid's pair count `cnt` per wave and side).  A grid whose
// pairs exceed maxp keeps the first maxp; its count says so.
__device__ __forceinline__ void gb_list_disks(const GridJob &j, const CgView &v, int sides, int grid, int s, int lane,
                                              unsigned *cnt) {
  const int nb = 6 * j.tab.NB * j.tab.NB;
  for (int side = 0; side < (v.global ? 1 : sides); ++side) {
    const CgDisk k = cg_side(v, side, s);
    const int di = 2 * (grid * j.n + s) + side;
    if (lane == 0) j.disks[RT_CK(kCkCgBuild, di, 2LL * j.n * j.ng)] = k;
    for (int b0 = 0; b0 < nb; b0 += 64) {
      const int b = b0 + lane;
      const bool m = b < nb && cg_block(k, j.tab, b);
      const unsigned long long bm = __ballot(m);
      if (!bm) continue;
      unsigned q0 = 0;
      if (lane == 0) q0 = atomicAdd(cnt, (unsigned)__builtin_popcountll(bm));
      q0 = (unsigned)__builtin_amdgcn_readfirstlane((int)q0);
      const unsigned qi = q0 + (unsigned)__builtin_popcountll(bm & ((1ull << lane) - 1));
      if (m && qi < (unsigned)j.maxp)
        j.pairs[RT_CK(kCkCgBuild, (size_t)grid * j.maxp + qi, (long long)j.ng * j.maxp)] = make_int2(di, b);
    }
  }
}

// Pass 2 body, one wave: quarter `item & 3` of grid `grid`'s pair `item >> 2`
// -- the block's 64 tiles (a lane each), then the cells (a lane each) of every
// tile of the quarter the disk meets.  A listed cell goes to the sink in two
// steps, slot = sink.take(cell) and sink.put(cell, slot, sphere, tlo), up to
// kRound tiles a round: their cells' slot atomics are in flight together
// before the first entry waits for its slot.  kRound = 4 for the camera grids
// (their build is inside every moving launch); the point grids' sinks, which
// go through the CSR offsets, are 7 % slower that way than tile by tile
// (synth200's sphere grids 353 -> 378 us count, 386 -> 413 us fill,
// profiles/r13a), so they take 1.
template <int kRound, class Sink>
__device__ __forceinline__ void gb_bin_quarter(const GridJob &j, int grid, unsigned item, int lane, const Sink &sink) {
  const int2 pr = j.pairs[RT_CK(kCkCgBuild, (size_t)grid * j.maxp + (item >> 2), (long long)j.ng * j.maxp)];
  const CgDisk k = j.disks[RT_CK(kCkCgBuild, pr.x, 2LL * j.n * j.ng)];
  const bool wide = cg_wide(k);
  const int bb = pr.y, NB = j.tab.NB;
  const int f = bb / (NB * NB), bj = (bb / NB) % NB, bi = bb % NB;
  bool tm, inside;
  cg_tile(k, j.tab, f, bi, bj, lane, tm, inside);
  unsigned long long tmask = __ballot(tm) & (0xffffull << (16 * (item & 3)));
  const unsigned long long imask = __ballot(inside);
  while (tmask) {
    int gcs[kRound];
#pragma unroll
    for (int u = 0; u < kRound; ++u) {
      gcs[u] = -1;
      if (!tmask) continue;
      const int tl = __builtin_ctzll(tmask);
      tmask &= tmask - 1;
      gcs[u] = cg_cell(k, wide, j.tab, f, bi, bj, tl, lane, (imask >> tl) & 1ull);
    }
    int slots[kRound];
#pragma unroll
    for (int u = 0; u < kRound; ++u) slots[u] = gcs[u] >= 0 ? sink.take(gcs[u]) : 0;
#pragma unroll
    for (int u = 0; u < kRound; ++u)
      if (gcs[u] >= 0) sink.put(gcs[u], slots[u], k.s, k.tlo);
  }
}

// A list of cnt elements sorted in place, ascending by before(key(a), key(b))
// (lists are short: insertion sort; the key of the element being placed is
// formed once).
template <class T, class Key, class Before>
__device__ __forceinline__ void gb_insertion_sort(T *e, int cnt, Key key, Before before) {
  for (int k = 1; k < cnt; ++k) {
    const T x = e[k];
    const auto kx = key(x);
    int m = k - 1;
    while (m >= 0 && before(kx, key(e[m]))) {
      e[m + 1] = e[m];
      --m;
    }
    e[m + 1] = x;
  }
}
// (sphere, tlo bits) entries: ascending (tlo, sphere index)
__device__ __forceinline__ void gb_sort_entries(int2 *e, int cnt) {
  gb_insertion_sort(e, cnt, [](int2 x) { return x; },
                    [](int2 a, int2 b) { return cg_before(__int_as_float(a.y), a.x, __int_as_float(b.y), b.x); });
}

// ---------------------------------------------------------------------------
// The camera grid, built for each camera position of a launch.  Every
// sphere's two disks seen from the grid's point P -- along +u with tlo =
// (D - R)(1 - 1e-9), along -u (the negative tangent root, sphere.h:43-47)
// with -(D + R)(1 + 1e-9), R the light grids' grown radius, each disk's
// angular radius asin(R / D) + kLgSlack -- are listed in every cell they
// meet; a sphere that contains (or nearly contains) P, or has non-finite data,
// is one disk of every direction with tlo = -inf (on every list).  A cell
// keeps K entries; one that overflows is marked by its count, and its rays
// sweep.  Passes: cg_disk_kernel (pass 1), cg_bin_kernel (pass 2: a fixed
// grid of waves walks the grids' pair lists), cg_sort_kernel (a thread per
// cell: (tlo, index) order).
struct CgBuild {
  GridJob j;       // npairs: [grid * kCgCntStride] (a 256-byte line per grid's counter)
  int32_t *count;  // [grid][cell] the lists' lengths
  int2 *ent;       // [grid][cell][K] the lists
  int K;
  double px[RT_MAX_FRAMES], py[RT_MAX_FRAMES], pz[RT_MAX_FRAMES], diam[RT_MAX_FRAMES];
};
static_assert(sizeof(CgBuild) <= 4096, "CgBuild exceeds the kernel-argument segment");

constexpr int kCgCntStride = 64;
__global__ __launch_bounds__(256) void cg_disk_kernel(const CgBuild a) {
  const int t = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = (int)(threadIdx.x & 63);
  if (t >= a.j.n * a.j.ng) return;
  const int grid = t / a.j.n, s = t - grid * a.j.n;
  const SphGeo sp = a.j.geo[s];
  const CgView v = cg_view(sp.cx, sp.cy, sp.cz, a.j.rad[s], a.px[grid], a.py[grid], a.pz[grid], a.diam[grid]);
  // a grid whose pairs exceed maxp: cg_sort_kernel marks all its cells overflowed (its rays sweep)
  gb_list_disks(a.j, v, 2, grid, s, lane, &a.j.npairs[grid * kCgCntStride]);
}

// a listed cell takes a slot (count) and, below K, the entry (sphere, tlo)
struct CgSink {
  const CgBuild &a;
  long long c0, cells;  // the grid's first cell; cells per grid
  __device__ int take(int cell) const { return atomicAdd(&a.count[RT_CK(kCkCgBuild, c0 + cell, a.j.ng * cells)], 1); }
  __device__ void put(int cell, int slot, int s, float tlo) const {
    if (slot < a.K)
      a.ent[RT_CK(kCkCgBuild, (c0 + cell) * a.K + slot, a.j.ng * cells * a.K)] = make_int2(s, __float_as_int(tlo));
  }
};
__global__ __launch_bounds__(64) void cg_bin_kernel(const CgBuild a) {
  const int lane = (int)(threadIdx.x & 63);
  const long long cells = 6LL * a.j.tab.N * a.j.tab.N;
  // work items per grid (4 per stored pair; the host keeps 4 ngrid maxp < 2^32), then their prefix
  unsigned incl = lane < a.j.ng ? 4u * min(a.j.npairs[lane * kCgCntStride], (unsigned)a.j.maxp) : 0u;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  const unsigned total = __shfl(incl, 63, 64);
  for (unsigned v = blockIdx.x; v < total; v += gridDim.x) {
    const int grid = __builtin_popcountll(__ballot(incl <= v));
    const unsigned item = v - (grid ? __shfl(incl, grid - 1, 64) : 0u);
    gb_bin_quarter<4>(a.j, grid, item, lane, CgSink{a, grid * cells, cells});
  }
}

// Pass 3, a thread per cell: its list sorted in place (an overflowed cell's
// rays sweep, its list unread).
__global__ __launch_bounds__(256) void cg_sort_kernel(const CgBuild a) {
  const long long cells = 6LL * a.j.tab.N * a.j.tab.N;
  const long long gc = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gc >= cells * a.j.ng) return;
  if (a.j.npairs[(gc / cells) * kCgCntStride] > (unsigned)a.j.maxp) {  // pass 1 dropped pairs: the grid is incomplete
    a.count[gc] = a.K + 1;                                               // every cell overflowed, its rays sweep
    return;
  }
  const int cnt = a.count[gc];
  if (cnt > a.K) return;
  gb_sort_entries(a.ent + gc * a.K, cnt);
}

// ---------------------------------------------------------------------------
// Point grids built at upload: the sphere grids (build_sphere_grids,
// rt_lightgrid.cpp) -- one cube-map grid per reflective sphere s, seen from
// the ball B(C_s, rho_s) that holds the origins of the reflection rays leaving
// s (main.cpp:46), both disks of every sphere, the spheres within reach of
// the ball (global) on every list, entries (sphere, tlo) ascending by (tlo,
// index) -- and the light grids (build_light_grid) -- one grid per light, seen
// from the light (rho = 0), the disk ahead only, global spheres on a separate
// list (the grid's slot `cells`), ids ascending.  The host builders' CSR
// layouts.  Grids go through in batches (their disks and pair lists are
// scratch); passes:
//   pg_disk_kernel   pass 1 (pairs past maxp and global spheres counted per
//                    grid: the host refuses a sphere grid with more than
//                    kSgMaxGlobal globals or dropped pairs, as
//                    build_sphere_grids refuses it); a light grid's global
//                    sphere goes to its global list (counted, then filled)
//   pg_bin_kernel    pass 2 over the host's work offsets: <count> adds 1 per
//                    listed cell, <fill> takes a slot there and writes the
//                    entry at the cell's CSR offset
//   scan_*           the exclusive prefix of the counts (CSR offsets)
//   sg_sort_kernel / ids_sort_kernel   a thread per list: (tlo, index) / (nearest distance, index) order
//   sg_start_kernel / lg_start_kernel  the host builders' start arrays
struct GridPt {  // a grid's point and origin-ball radius
  double x, y, z, rho;
};
struct SgBuild {
  GridJob j;                     // the batch's grids; npairs: [grid * kSgCntStride] (one 64-B line each)
  const GridPt *pts;             // [ng] the batch's grids
  const unsigned char *allglob;  // [ng] or nullptr: 1 = every sphere global (a non-finite light)
  unsigned *nglob;       // [ng * 16]: global spheres per grid
  const unsigned *woff;  // [ng + 1]: work items (4 per kept pair) before grid j; refused grids have none
  int *cnt;              // [ng][row] (count pass: list lengths; fill pass: slots taken)
  const int *off;        // [(g0 + j) row + c]: the CSR offset of the batch's grid j's list c
  int2 *ent;             // sphere grids: (sphere, tlo bits)
  int32_t *ids;          // light grids: sphere ids
  long long nent;        // entries of all grids (the fill pass's bound)
  int g0;                // the batch's first grid
  int row;               // lists per grid: 6 N^2 cells (+ 1 global list: light grids)
  int sides;             // 2: both disks (sphere grids), 1: the disk ahead (light grids)
  int globlist;          // 1: global spheres on the grid's list `row - 1`, not in every cell
  int fill;              // the pass: 0 count, 1 fill
  double diam;
};
static_assert(sizeof(SgBuild) <= 4096, "SgBuild exceeds the kernel-argument segment");
constexpr int kSgCntStride = 16;

// a list entry: at the CSR offset of list ci (batch-local) plus its slot
__device__ __forceinline__ void pg_put(const SgBuild &a, long long ci, int slot, int s, float tlo) {
  const long long e = RT_CK(kCkCgBuild, (long long)a.off[(long long)a.g0 * a.row + ci] + slot, a.nent);
  if (a.ids)
    a.ids[e] = s;
  else
    a.ent[e] = make_int2(s, __float_as_int(tlo));
}
// list `cell` of a grid (l0: its first list, batch-local): counted, or (fill) a slot taken and filled
struct PgSink {
  const SgBuild &a;
  long long l0;
  __device__ int take(int cell) const {
    return atomicAdd(&a.cnt[RT_CK(kCkCgBuild, l0 + cell, (long long)a.j.ng * a.row)], 1);
  }
  __device__ void put(int cell, int slot, int s, float tlo) const {
    if (a.fill) pg_put(a, l0 + cell, slot, s, tlo);
  }
};

__global__ __launch_bounds__(256) void pg_disk_kernel(const SgBuild a) {
  const int t = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = (int)(threadIdx.x & 63);
  if (t >= a.j.n * a.j.ng) return;
  const int j = t / a.j.n, i = t - j * a.j.n;
  const GridPt P = a.pts[j];
  const SphGeo sp = a.j.geo[i];
  // light grids (one side): spheres within a shadow ray's overshoot of the light are global (kLgOvershoot)
  CgView v = cg_view(sp.cx, sp.cy, sp.cz, a.j.rad[i], P.x, P.y, P.z, a.diam, P.rho, a.sides == 1 ? kLgOvershoot : 0.0);
  if (a.allglob && a.allglob[j]) v = cg_view(0.0, 0.0, 0.0, __builtin_inf(), 0.0, 0.0, 0.0, 0.0);  // global
  if (v.global && lane == 0) {
    atomicAdd(&a.nglob[j * kSgCntStride], 1u);
    if (a.globlist) {  // the grid's global list
      const PgSink sink{a, (long long)j * a.row};
      sink.put(a.row - 1, sink.take(a.row - 1), i, -__builtin_inff());
    }
  }
  if (v.global && a.globlist) return;
  gb_list_disks(a.j, v, a.sides, j, i, lane, &a.j.npairs[j * kSgCntStride]);
}

__global__ __launch_bounds__(64) void pg_bin_kernel(const SgBuild a) {
  const int lane = (int)(threadIdx.x & 63);
  const unsigned total = a.woff[a.j.ng];
  for (unsigned v = blockIdx.x; v < total; v += gridDim.x) {
    int lo = 0, hi = a.j.ng;  // the grid of work item v: woff[j] <= v < woff[j + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.woff[mid] <= v) lo = mid; else hi = mid;
    }
    gb_bin_quarter<1>(a.j, lo, v - a.woff[lo], lane, PgSink{a, (long long)lo * a.row});
  }
}

// Exclusive prefix sum of n ints (x -> y, y[n] = the total), in chunks of
// kScanChunk per 256-thread block: chunk sums, their prefix (one block), then
// each chunk's prefix from its base.
constexpr int kScanChunk = 4096;
__device__ __forceinline__ int block_excl_scan256(int x, int *sh, int &total) {
  const int t = (int)threadIdx.x;
  sh[t] = x;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = t >= o ? sh[t - o] : 0;
    __syncthreads();
    sh[t] += v;
    __syncthreads();
  }
  total = sh[255];
  const int incl = sh[t];
  __syncthreads();
  return incl - x;
}
__global__ __launch_bounds__(256) void scan_chunk_sums(const int *x, long long n, long long *bsum) {
  __shared__ long long sh[256];
  const long long b0 = (long long)blockIdx.x * kScanChunk;
  long long s = 0;
  for (int k = threadIdx.x; k < kScanChunk; k += 256)
    if (b0 + k < n) s += x[b0 + k];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) bsum[blockIdx.x] = sh[0];
}
// in place, exclusive, in 64 bits (bsum[nb] = the total: the caller refuses
// totals past 32 bits before using the offsets); a few thousand chunk sums at
// most, serially in one thread
__global__ __launch_bounds__(64) void scan_sums(long long *bsum, int nb) {
  if (threadIdx.x != 0) return;
  long long run = 0;
  for (int k = 0; k < nb; ++k) {
    const long long v = bsum[k];
    bsum[k] = run;
    run += v;
  }
  bsum[nb] = run;
}
__global__ __launch_bounds__(256) void scan_apply(const int *x, long long n, const long long *bsum, int *y) {
  __shared__ int sh[256];
  constexpr int kPer = kScanChunk / 256;
  const long long b0 = (long long)blockIdx.x * kScanChunk + (long long)threadIdx.x * kPer;
  int v[kPer], s = 0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    v[k] = b0 + k < n ? x[b0 + k] : 0;
    s += v[k];
  }
  int tot;
  int run = (int)bsum[blockIdx.x] + block_excl_scan256(s, sh, tot);
#pragma unroll
  for (int k = 0; k < kPer; ++k)
    if (b0 + k < n) {
      y[b0 + k] = run;
      run += v[k];
    }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) y[n] = (int)bsum[gridDim.x];
}

// Sphere s's row of CSR starts (every sphere has one, as on the host): its
// grid's offsets, or an empty list everywhere (no grid / refused).
__global__ __launch_bounds__(256) void sg_start_kernel(const int *gidx, const unsigned char *ok, const int *off,
                                                       int n, long long cells, int *start) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x, row = cells + 1;
  if (k >= (long long)n * row) return;
  const int s = (int)(k / row);
  const long long c = k - (long long)s * row;
  const int j = gidx[s];
  start[k] = (j >= 0 && ok[j]) ? off[(long long)j * cells + c] : 0;
}

// A light grid's start row (build_light_grid: stride 6N^2 + 2, the global
// list last): the CSR offsets of its 6N^2 + 1 lists and their end.
__global__ __launch_bounds__(256) void lg_start_kernel(const int *off, int nl, long long cells, int *start) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x, row = cells + 2;
  if (k >= (long long)nl * row) return;
  const long long l = k / row, c = k - l * row;
  start[k] = off[l * (cells + 1) + c];  // c = cells + 1: the next light's first offset (or the total)
}

// A thread per list: ascending ids; with `near` (light grids) ascending by
// the sphere's nearest distance from the grid's point (|C - P| - |r|, then the
// id; a NaN distance ties with every other), so a shadow query meets the
// spheres between its point and the light before those beyond it -- the
// lists' order is free: a shadow query is an any-hit test (scene.h:78-82).
__device__ __forceinline__ double near_key(const SphGeo *geo, const GridPt &p, int i) {
  const SphGeo s = geo[i];
  const double dx = s.cx - p.x, dy = s.cy - p.y, dz = s.cz - p.z;
  return __builtin_sqrt(dx * dx + dy * dy + dz * dz) - __builtin_sqrt(s.rr);
}
__global__ __launch_bounds__(256) void ids_sort_kernel(const int *off, long long nlists, int32_t *ids,
                                                       const SphGeo *geo, const GridPt *pts, long long row, int near) {
  const long long gc = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gc >= nlists) return;
  const GridPt p = near ? pts[gc / row] : GridPt{};
  struct Key {
    double d;
    int32_t i;
  };
  gb_insertion_sort(ids + off[gc], off[gc + 1] - off[gc],
                    [&](int32_t i) { return Key{near ? near_key(geo, p, i) : 0.0, i}; },
                    [](const Key &a, const Key &b) { return a.d < b.d || (!(b.d < a.d) && a.i < b.i); });
}

// A thread per cell of every grid: its list in (tlo, index) order.
__global__ __launch_bounds__(256) void sg_sort_kernel(const int *off, long long ncells, int2 *ent) {
  const long long gc = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gc >= ncells) return;
  gb_sort_entries(ent + off[gc], off[gc + 1] - off[gc]);
}

}  // namespace rtk
