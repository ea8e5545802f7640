// rt_kernel.hip -- gfx950 (MI355X / CDNA4) render loop + device half of the C-ABI.
//
// One lane per pixel, wave64 over an 8x8 pixel tile, one-wave workgroups; a
// wave takes four tiles (merge_tiles; the heaviest and the last tiles of a
// launch one each) in the host's heavy-first order.  The scene (spheres as
// cx,cy,cz,r*r in fp64, lights, 4-wide BVH, light / camera / sphere / behind
// grids) is read through L1/L2.  Reflections are walked iteratively: the rays
// of a level are merged across the wave's tiles into full passes (an LDS
// queue), deep levels of multi-frame launches go to a second kernel
// (render_deferred), and each level's (shade*(1-refl), refl) is unwound at the
// end, which reproduces the reference recursion's rounding exactly.
// RT_HIP_LDS_SCENE=1 is the first design: 2x2-wave workgroups, scene in LDS.
// The ray queries (rt_trace_rays, rt_camera_rays: rt_query.h) ask the same
// sweeps and walks for the closest hit / an occluder of rays the caller supplies,
// the path queries (rt_trace_paths: rt_paths.h) for a ray's whole reflection
// path with its shadow masks, and the radiance queries (rt_trace_radiance:
// rt_radiance.h) shade and composite that path into trace_ray's colour.
//
// Numerics follow the serial fp64 path operation by operation:
// vec3.h:13-33, ray.h:12, camera.h:17-25, sphere.h:26-64, scene.h:41-121,
// main.cpp:16-58 and the quantiser main.cpp:85-87.  Build with
// -ffp-contract=off (also forced below): no FMA contraction, IEEE division and
// sqrt, so the output bytes equal ray_serial's.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <string>

#include "rt_hip.h"
#include "rt_internal.h"

#pragma clang fp contract(off)

#include "rt_device.h"
#include "rt_cgbuild.h"
#include "rt_gridbuild.h"
#include "rt_query.h"
#include "rt_paths.h"
#include "rt_radiance.h"
#include "rt_sched.h"

#include <chrono>
#include <cmath>
#include <vector>

namespace rtk {

#ifdef RT_STAMPS
// Diagnostic timeline: per wave {start, end} (s_memrealtime, 100 MHz) and
// {HW_ID, XCC_ID}; dumped by rt_render_stats when RT_HIP_STAMPS_FILE is set.
constexpr int kTimelineWaves = 1 << 17;
constexpr int kTl = 16;  // u64 per wave
__device__ unsigned long long g_timeline[kTimelineWaves * kTl];
#endif


// Output of a launch.  RT_FB_RGB8 with full = 0: rows.count x W RGB8 (the
// rows of `rows`, rt_render); RT_FB_RGB8 with full = 1: a W x H RGB8 image in
// PPM row order; RT_FB_F32X3 / RT_FB_F64X3: the reference's framebuffer,
// index j*W + x with j = 0 the bottom row (src/main.cpp:156, kernel.cu:112),
// unquantised.  Pixels x0 <= x < x0 + xw are written.  Frame f of a
// multi-frame launch (RT_FB_RGB8, full = 0) starts fstride bytes after frame f-1.
struct OutDesc {
  void *ptr;
  int fmt, full, x0, xw;
  long long fstride;
};

// A queued ray of the merged levels (merge_tiles' LDS queue, render_deferred's
// global queue): origin, direction, stack level, depth left, the sphere it
// leaves, and its pixel.
struct QRay {  // 64 B
  double ox, oy, oz, dx, dy, dz;
  int orig, dleft, key, pix;
};
// All arguments of render_kernel in one struct: its only kernel parameter, so
// it sits at offset 0 of the kernarg segment and a member can be re-read from
// there by offsetof (kernarg_late).
struct RenderArgs {
  const SphGeo *geo;
  const double *radius;
  const SphMat *mat;
  const LightD *lights;
  int n, nl;
  D3 amb;
  Cam cam[RT_MAX_FRAMES];  // frame f's camera (rt_render_frames_async); cam[0] otherwise
  int frames;              // frames of this launch: launch slot b renders frame b % frames of tile slot b / frames
  int W, H, depth;
  Rows rows;
  BvhArgs bv;
  LgArgs lg;
  CgArgs cg;  // camera grid of the launch's (shared) camera position; cg.on = 0: none
  SgArgs sg;  // sphere grids (reflection rays); sg.on = 0: none
  OutDesc od;
  StackEnt *gstack;               // kStackGlobal: [depth-1][launch pixels]
  StackEnt *homes;                // kStackMerge: [home][depth-1][kMergeTiles * 64] (a wave's group of tiles)
  unsigned long long *home_bits;  // kStackMerge: the homes taken (a bit each)
  int home_words;                 // kStackMerge: 64-bit words of home_bits
  StackEnt *dstack;               // kStackMerge: deferred rays' stacks, [depth-1][kShards * dq_cap]
  unsigned long long *counters;
  int ntx, ntiles;
  int nslots;                     // wave slots per frame: kStackMerge tile groups, kStackGlobal with perm
                                  // the listed blocks, else ntiles
  const int *perm;
  unsigned long long *zero_next;  // counters of the next launch, zeroed by workgroup 0 (or nullptr)
  QRay *dq;                       // kStackMerge: deferred deep rays, [kShards][dq_cap] (render_deferred)
  int dq_cap;                     // entries per shard segment; 0 = no deferral
  int merge_q;                    // kStackMerge: LDS ray-queue entries per wave (16..64)
  int nsingle;                    // kStackMerge: the first nsingle tile slots (heaviest class) get a wave each
  int merge_end;                  // kStackMerge: slots [nsingle, merge_end) go kMergeTiles per wave, the rest
                                  // (the launch's tail: its lightest tiles) one per wave again
  int pix_off;                    // kStackMerge: LDS offset of the wave's finished pixels (flush_tile)
  int rows_dword;                 // kStackMerge: every 8-pixel tile row starts dword aligned (flush_tile)
  int defer_level;                // kStackMerge: rays of this reflection level and deeper are deferred
  int xcd_frames;                 // multi-frame launches: every frame of a tile group on one XCD (render_kernel)
  const double *dirs;             // kStackMerge: the launch's ray table (ray_table_kernel), or nullptr: rays formed inline
};
// The ray table: per tile (its unpermuted index) the planes x, y, z of the 64
// lanes' camera-ray directions, 512 B each -- a wave's load of one plane is one
// contiguous run at a scalar tile base plus the lane's offset.
constexpr int kRayTileDoubles = 3 * 64;
constexpr size_t kRayTileBytes = kRayTileDoubles * sizeof(double);
// the whole struct is the kernel's argument block (kernarg segment, at most 4 KiB)
static_assert(sizeof(RenderArgs) <= 4096, "RenderArgs exceeds the kernel-argument segment");

// Member `x` (at offset kOff of RenderArgs) re-read from the kernarg segment
// here.  Kernel arguments are otherwise loaded into SGPRs at entry and live
// for the whole kernel; the big loop-invariant ones (BVH and light-grid
// descriptors) then spill to VGPR lanes, paid for with v_readlane /
// v_writelane in the level and light loops.  The empty asm makes the kernarg
// pointer opaque, so the scalar loads happen at this point and their
// registers are free again afterwards.  kLate = false returns x itself.
template <bool kLate, size_t kOff, class T>
__device__ __forceinline__ const T &kernarg_late(const T &x);

// Frame f's camera, read from the kernarg segment (a dynamic index into the
// by-value kernel argument would copy the array to scratch).
__device__ __forceinline__ const Cam &kernarg_cam(int f) {
  typedef const __attribute__((address_space(4))) unsigned char KB;
  KB *p = (KB *)__builtin_amdgcn_kernarg_segment_ptr();
  return *(const Cam *)(p + offsetof(RenderArgs, cam) + (size_t)f * sizeof(Cam));
}

template <bool kLate, size_t kOff, class T>
__device__ __forceinline__ const T &kernarg_late(const T &x) {
  if constexpr (!kLate) {
    return x;
  } else {
    typedef const __attribute__((address_space(4))) unsigned char KB;
    KB *p = (KB *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const T *)(p + kOff);
  }
}

// One bounce of trace_ray (src/main.cpp:16-58) for the wave's `alive` lanes:
// closest hit, sky on a miss, Phong shading with per-light shadow queries,
// and the reflection decision (main.cpp:43-55).  Outcome per alive lane:
// kEnded (colour = the level's final colour: sky, shade, or shade*(1-refl)
// when no depth is left) or kSpawned (colour = shade*(1-refl), refl, and the
// reflection ray no/nd leaving sphere nkey).  Wave-uniform control flow.
enum { kEnded = 1, kSpawned = 2 };

// kArgMem: bv and lg are the kernel's own arguments (kernarg segment), so they
// are re-read where needed (kernarg_late) instead of held in SGPRs throughout.
// kFast: only the default paths (ordered 4-wide BVH walk, light-grid shadow
// queries) are compiled in; the host picks it when the scene uses them.
// The part of bounce() after the closest hit (bi, bt) is known: sky or
// shading with the shadow queries, and the reflection decision.  Lanes with
// alive = false take no part; it has no wave-wide operation that needs every
// lane active (render_deferred_walk calls it for the lanes whose walk ended).
// Position of the k-th (from 0) set bit of m (k < popcount(m)).
__device__ __forceinline__ int nth_set_bit(unsigned long long m, int k) {
  int pos = 0;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned long long low = m & ((1ull << s) - 1ull);
    const int c = __popcll(low);
    if (k >= c) {
      k -= c;
      m >>= s;
      pos += s;
    } else {
      m = low;
    }
  }
  return pos;
}

// kWide (one-frame launches): a wave whose hit lanes are at most half of it
// spreads the light loop over the lanes -- in passes of lpp = 64 / hits lights,
// lane j handles light l0 + j % lpp of the (j / lpp)-th hit lane: its shadow
// query and Phong terms, computed with the same operands and operations as the
// loop below (the hit lane's normal and view direction passed over) -- and each
// hit lane then adds its lights' terms in file order (scene.h:117): the same
// bits, in ceil(lights / lpp) passes instead of one per light.
// kTwoForms (kFast, the lane-per-ray loop): each light's shadow query has a
// straight-line form for the waves whose lanes all pass the light's guards
// (rt_device.h light_common, shadow_cells_row<true>) beside the general one.  The
// render kernel has it (synth200 0.186 -> 0.181 ms per frame); the deferred
// kernels and the wide loop do not: there it measured no faster, and in the
// wide loop it costs 16 more VGPR spills.  The flag
// also tells the wide loop which kernel it is in: the render kernel's takes
// the list's exact test in its predicated form (shadow_cells' kPred), the
// deferred kernels' keeps the chain form.
template <bool kCull, bool kArgMem = false, bool kFast = false, bool kWide = false, bool kTwoForms = true>
__device__ __forceinline__ void shade_hit(const SphGeo *__restrict__ g, const double *__restrict__ rad,
                                          const SphMat *__restrict__ mat, const LightD *__restrict__ slight, int n,
                                          int nl, D3 amb, const BvhArgs &bv, const LgArgs &lg_arg, bool alive, D3 o,
                                          D3 d, int key, int dleft, int bi, double bt, Work &work, unsigned &c_shadow,
                                          int &outcome, D3 &color, double &refl, D3 &no, D3 &nd, int &nkey) {
  outcome = 0;
  const bool hit = alive && bi >= 0;
  if (alive && !hit) {  // sky, main.cpp:26-30
    const double st = 0.5 * (d.y + 1.0);
    color = add(scale(mk(1.0, 1.0, 1.0), 1.0 - st), scale(mk(0.5, 0.7, 1.0), st));
    outcome = kEnded;
  }
  const int hi = RT_CK(kCkSphere, hit ? bi : 0, n > 0 ? n : 1);
  const D3 hp = add(o, scale(d, bt));                            // main.cpp:32
  D3 col;
  {
    const SphMat m0 = mat[hi];
    col = mul(amb, mk(m0.cr, m0.cg, m0.cb));                   // scene.h:91
  }
  // the normal (sphere.h:62-64), used by the shading and by the reflection
  // (main.cpp:44-46: the same expression, formed once), and the view direction
  D3 nrm = mk(0.0, 0.0, 0.0), view = nrm;
  if (hit) {
    const SphGeo sg = g[hi];
    nrm = normalized(sub(hp, mk(sg.cx, sg.cy, sg.cz)));
    view = normalized(sub(o, hp));  // main.cpp:38
  }
    // scene.h:94-120: per light in file order, the shadow query then (if lit)
    // the Phong terms with the same ldir -- skipped by a wave (or the active
    // lanes of one) whose rays all left the scene
    bool wide_done = false;
    if constexpr (kWide && kFast) {
      const unsigned long long hm = __ballot(hit);
      const int nh = __popcll(hm);
      const LgArgs &lgw = kernarg_late<kArgMem, offsetof(RenderArgs, lg)>(lg_arg);
      const int lpp = nh ? (64 / nh < nl ? 64 / nh : nl) : 0;  // lights per pass
      if (nl >= 2 && lpp >= 2 && lgw.on) {                   // wave-uniform
        const int lane = (int)(threadIdx.x & 63);
        const int rank = (int)__popcll(hm & ((1ull << lane) - 1ull));
        for (int l0 = 0; l0 < nl; l0 += lpp) {  // lights l0 .. l0 + cnt - 1 in this pass
          const int cnt = nl - l0 < lpp ? nl - l0 : lpp;
          const bool helper = lane < nh * cnt;
          const int r = helper ? lane / cnt : 0, lh = l0 + (helper ? lane - r * cnt : 0);
          const int src = nth_set_bit(hm, r);
          // the owner's hit point, sphere, normal and view direction
          const D3 hq = mk(__shfl(hp.x, src, 64), __shfl(hp.y, src, 64), __shfl(hp.z, src, 64));
          const D3 nq = mk(__shfl(nrm.x, src, 64), __shfl(nrm.y, src, 64), __shfl(nrm.z, src, 64));
          const D3 vq = mk(__shfl(view.x, src, 64), __shfl(view.y, src, 64), __shfl(view.z, src, 64));
          const int hq_i = RT_CK(kCkSphere, __shfl(hi, src, 64), n > 0 ? n : 1);
          D3 t = mk(0.0, 0.0, 0.0);
          bool lit = false;
          {
            const SphMat m = mat[hq_i];
            const D3 mc = mk(m.cr, m.cg, m.cb);
            const LightD L = slight[lh];
            const D3 lp = mk(L.px, L.py, L.pz);
            const LgRange cell = lg_range(lgw, lh, hq, lp, helper);
            const int id0 = lg_first(lgw, cell);
            const D3 to_light = sub(lp, hq);
            const double dist = length(to_light);
            const D3 ldir = normalized(to_light);
            const D3 so = add(hq, scale(ldir, kEps)), sd = renormalized(ldir);
            // the list's exact test in its predicated form, except in the
            // deferred kernels (no kTwoForms): there it costs 4 VGPR spills
            const bool occ =
                shadow_cells<kTwoForms>(g, n, helper, so, sd, lp, dist, lgw, lh, cell, id0, work, hq_i);
            if (helper && !occ) {  // the terms of the loop below, same operands and order
              const double ndl = max0(dot(nq, ldir));
              const D3 diffuse = scale(scale(mc, 1.0 - m.refl), ndl);
              const D3 nl2 = scale(ldir, -1.0);
              const D3 rdir = sub(nl2, scale(scale(nq, 2.0), dot(nl2, nq)));
              const double rdv = max0(dot(rdir, vq));
              double spec = 0.0;
              int ipow = 0;
              if (!(rdv == 0.0 && m.shin > 0.0))
                spec = int_pow_ok(rdv, m.shin, ipow) ? int_pow(rdv, ipow) : pow_call(rdv, m.shin);
              const D3 specular = scale(scale(mk(L.cr, L.cg, L.cb), kSpec), spec);
              t = add(specular, diffuse);
              lit = true;
            }
          }
          // each hit lane adds this pass's lights' terms in file order (scene.h:117)
          const unsigned long long litm = __ballot(lit);
          for (int l = 0; l < cnt; ++l) {
            const int sl = hit ? rank * cnt + l : 0;
            const D3 tl = mk(__shfl(t.x, sl, 64), __shfl(t.y, sl, 64), __shfl(t.z, sl, 64));
            if (hit && ((litm >> sl) & 1ull)) col = add(tl, col);
          }
        }
        wide_done = true;
      }
    }
    if (!wide_done && __ballot(hit)) {
      const SphMat m = mat[hi];
      const D3 mc = mk(m.cr, m.cg, m.cb);
      // kRow (the render kernel's loop, the one with two forms): the light
      // grid's descriptor is read once per call, and what a light's iteration
      // needs of it is carried in scalar registers -- the light's row of
      // lg.start, advanced by the row stride (6 N^2 + 2 entries) per light.
      // The next light's cell range is loaded from the next row one light
      // ahead; this light's global-list range is loaded through the scalar path
      // (lg_global_uniform) and the lane's own sphere, for the query's pre-test,
      // through the vector path, both where the iteration starts, so they
      // arrive during the setup arithmetic.  The deferred kernels keep the loop
      // that re-reads the descriptor where it is used: with the carried row they
      // measured no faster (profiles/r14a).
      // kRow has no test of lg.on: launch_tiles sets `sel.fast = merge &&
      // bv.ordered && bv.wide && ra.lg.on`, and render_kernel_fn picks a kFast
      // kernel only from sel.fast (sel.wide implies it), so the test is
      // constant in this loop.  What is wave-uniform per call is decided
      // once here: off_free, as the width of light_common's range test.
      constexpr bool kRow = kFast && kTwoForms;
      LgArgs lgv{};  // kRow: the fields the straight-line form reads; the rest stay in the kernarg segment
      int cells = 0;
      const int32_t *row = nullptr;
      [[maybe_unused]] long long room = 0;  // RT_CHECK: entries of lg.start from `row` on, less one
      LgRange next{0, 0};
      [[maybe_unused]] double common_width = 0.0;
      if constexpr (kRow) {
        const LgArgs &lgk = kernarg_late<kArgMem, offsetof(RenderArgs, lg)>(lg_arg);
        lgv.start = lgk.start, lgv.ids = lgk.ids, lgv.N = lgk.N, lgv.on = lgk.on, lgv.off_free = lgk.off_free;
#ifdef RT_CHECK
        lgv.nstart = lgk.nstart, lgv.nids = lgk.nids;
#endif
        cells = 6 * lgv.N * lgv.N;
        row = lgv.start;
        room = lgv.nstart - 1;
        common_width = light_common_width(lgv.off_free != 0);
        if (nl > 0) next = lg_range_row(row, lgv.N, room, hp, mk(slight[0].px, slight[0].py, slight[0].pz), hit);
      } else {
        const LgArgs &lg0 = kernarg_late<kArgMem, offsetof(RenderArgs, lg)>(lg_arg);
        if (lg0.on && nl > 0) next = lg_range(lg0, 0, hp, mk(slight[0].px, slight[0].py, slight[0].pz), hit);
      }
      for (int l = 0; l < nl; ++l) {
        const LgArgs &lg = kernarg_late<kArgMem && !kRow, offsetof(RenderArgs, lg)>(lg_arg);
        RT_T0(t_setup);
        // this light's first list id, and the next light's cell range, are
        // loaded now and consumed after the setup arithmetic below
        const LgRange cell = next;
        int id0;
        [[maybe_unused]] LgRange glob{0, 0};
        [[maybe_unused]] SphGeo own{};
        if constexpr (kRow) {
          id0 = lg_first(lgv, cell);
          glob = lg_global_uniform(row, cells, room);
          if (l + 1 < nl)
            next = lg_range_row(row + (cells + 2), lgv.N, room - (cells + 2), hp,
                                mk(slight[l + 1].px, slight[l + 1].py, slight[l + 1].pz), hit);
          own = g[hi];
        } else {
          id0 = lg.on ? lg_first(lg, cell) : 0;
          if (lg.on && l + 1 < nl) next = lg_range(lg, l + 1, hp, mk(slight[l + 1].px, slight[l + 1].py, slight[l + 1].pz), hit);
        }
        const LightD L = slight[l];
        const D3 lp = mk(L.px, L.py, L.pz);
        const D3 to_light = sub(lp, hp);
        const double dist = length(to_light);
        const D3 ldir = normalized(to_light);
        const bool need = hit;
        RT_ACC(work, 3, t_setup);
        RT_T0(t_sh);
        bool occ = false;
        if (__ballot(need)) {
          const D3 so = add(hp, scale(ldir, kEps));
          if constexpr (kRow) {
            // a wave with no rare lane for this light (light_common) takes the
            // query's straight-line form; any other wave the general one, with
            // the descriptor read from the kernarg segment there, where it is rare
            auto global_range = [&] { return glob; };
            double rt;
            const bool common = light_common(common_width, cell, dist, ldir, rt);
            if (__ballot(need && !common) == 0)
              occ = shadow_cells_row<true>(g, n, need, so, renorm_near_one_quot(ldir, rt), lp, dist, lgv, cell, id0, work,
                                           hi, own, global_range);
            else
              occ = shadow_cells_row(g, n, need, so, renormalized(ldir), lp, dist,
                                     kernarg_late<kArgMem, offsetof(RenderArgs, lg)>(lg_arg), cell, id0, work, hi, own,
                                     global_range);
          } else if constexpr (kFast) {
            occ = shadow_cells(g, n, need, so, renormalized(ldir), lp, dist, lg, l, cell, id0, work, hi);
          } else {
            const D3 sd = renormalized(ldir);
            occ = lg.on ? shadow_cells(g, n, need, so, sd, lp, dist, lg, l, cell, id0, work, hi)
                        : sweep_shadow<kCull>(g, rad, n, need, so, sd, lp, hi, dist,
                                              kernarg_late<kArgMem, offsetof(RenderArgs, bv)>(bv), work);
          }
        }
        RT_ACC(work, 9, t_sh);
        RT_T0(t_shade);
        if (hit && !occ) {
          const double ndl = max0(dot(nrm, ldir));
          const D3 diffuse = scale(scale(mc, 1.0 - m.refl), ndl);
          const D3 nl2 = scale(ldir, -1.0);
          const D3 rdir = sub(nl2, scale(scale(nrm, 2.0), dot(nl2, nrm)));  // reflect(), vec3.h:31-33
          const double rdv = max0(dot(rdir, view));
          // pow(+0, y > 0) is +0 exactly (C99 F.10.4.4), so most lanes skip ocml's pow.
          double spec = 0.0;
          int ipow = 0;
          if (!(rdv == 0.0 && m.shin > 0.0))
            spec = int_pow_ok(rdv, m.shin, ipow) ? int_pow(rdv, ipow) : pow_call(rdv, m.shin);
          const D3 specular = scale(scale(mk(L.cr, L.cg, L.cb), kSpec), spec);
          col = add(add(specular, diffuse), col);                  // scene.h:117
        }
        RT_ACC(work, 4, t_shade);
        if constexpr (kRow) {
          row += cells + 2;
          room -= cells + 2;
        }
      }
    }
  if (hit) {
    c_shadow += (unsigned)nl;
    const SphMat m = mat[hi];
    if (m.refl > 0.0) {                                         // main.cpp:43-55
      const double w = 1.0 - m.refl;
      const D3 A = mk(col.x * w, col.y * w, col.z * w);
      color = A;  // with no depth left trace_ray(depth 0) is black: A + (0,0,0)*refl == A
      outcome = kEnded;
      if (dleft - 1 >= 1) {
        const D3 rd = sub(d, scale(scale(nrm, 2.0), dot(d, nrm)));
        no = add(hp, scale(nrm, kEps));
        nd = renormalized(rd);
        nkey = hi;
        refl = m.refl;
        outcome = kSpawned;
      }
    } else {
      color = col;
      outcome = kEnded;
    }
  }
}

// The closest hit of bounce() (scene.h:41-61) for the `alive` lanes: sphere
// index (-1: none) and t.  Wave-uniform control flow.
template <bool kCull, bool kArgMem = false, bool kFast = false>
__device__ __forceinline__ int closest_hit(const SphGeo *__restrict__ g, const double *__restrict__ rad, int n,
                                           const BvhArgs &bv, bool alive, D3 o, D3 d, int key, Work &work,
                                           double &bt_out, bool cam_pass = false, int frame = 0) {
  double bt = kInf;
  RT_T0(t_cl);
  int bi = -1;
  // cam_pass (kFast merged kernels, wave-uniform): every alive lane holds a
  // camera ray of a frame whose position is the camera grid's point.  The
  // lanes a grid cannot serve (`rest`) take the one sweep below.
  bool rest = alive;
  if constexpr (kFast && kArgMem) {
    if (cam_pass) {
      const CgArgs &cg = kernarg_late<true, offsetof(RenderArgs, cg)>(CgArgs{});
      bi = cam_closest(g, n, alive, o, d, cg, cg.per_frame ? frame : 0, rest, bt, work);
    } else if (kernarg_late<true, offsetof(RenderArgs, sg)>(SgArgs{}).on) {
      // reflection rays through the sphere grid of the sphere they leave; the
      // lanes whose origin fails the grid's check sweep as before
      bool grid;
      {
        const SgArgs &sg = kernarg_late<true, offsetof(RenderArgs, sg)>(SgArgs{});
        grid = sg_usable(g, sg, alive, o, key);
      }
      if (__ballot(grid)) {
        const SgArgs &sg = kernarg_late<true, offsetof(RenderArgs, sg)>(SgArgs{});
        bi = grid_closest(g, n, grid, o, d, sg.start, sg.ent, sg.N, grid ? key * (6 * sg.N * sg.N + 1) : 0, sg.nstart,
                          sg.nent, bt, work);
      }
      rest = alive && !grid;
    }
  }
  if (__ballot(rest)) {
    double bt2 = kInf;
    const int bi2 = sweep_closest<kCull, kFast>(g, rad, n, rest, o, d, key,
                                                kernarg_late<kArgMem, offsetof(RenderArgs, bv)>(bv), bt2, work);
    if (rest) {
      bi = bi2;
      bt = bt2;
    }
  }
  RT_ACC(work, 8, t_cl);
  bt_out = bt;
  return bi;
}

template <bool kCull, bool kArgMem = false, bool kFast = false, bool kWide = false, bool kTwoForms = true>
__device__ __forceinline__ void bounce(const SphGeo *__restrict__ g, const double *__restrict__ rad,
                                       const SphMat *__restrict__ mat, const LightD *__restrict__ slight, int n,
                                       int nl, D3 amb, const BvhArgs &bv, const LgArgs &lg_arg, bool alive, D3 o, D3 d,
                                       int key, int dleft, Work &work, unsigned &c_shadow, int &outcome, D3 &color,
                                       double &refl, D3 &no, D3 &nd, int &nkey, bool cam_pass = false) {
  double bt;
  const int bi = closest_hit<kCull, kArgMem, kFast>(g, rad, n, bv, alive, o, d, key, work, bt, cam_pass);
  shade_hit<kCull, kArgMem, kFast, kWide, kTwoForms>(g, rad, mat, slight, n, nl, amb, bv, lg_arg, alive, o, d, key, dleft, bi, bt,
                                          work, c_shadow, outcome, color, refl, no, nd, nkey);
}

// trace_ray for one camera ray per lane, the wave walking the levels together
// (lanes masked by `alive`); the lane's reflection stack entries are
// sbase[sidx + level * sstride] (depth - 1 levels), unwound innermost first.
// The wave-uniform base and a 32-bit lane index (not a per-lane 64-bit
// pointer) keep the stack address out of the registers that spill.
// kPark: a lane's final colour is parked in LDS (park[lane], this wave's
// slice) when its chain ends instead of being held in registers while the
// wave's other lanes keep bouncing (6 VGPRs fewer in the level loop).
template <bool kCull, bool kArgMem = false, bool kPark = false>
__device__ __forceinline__ D3 trace_wave(const SphGeo *__restrict__ g, const double *__restrict__ rad,
                                         const SphMat *__restrict__ mat, const LightD *__restrict__ slight, int n,
                                         int nl, D3 amb, int depth, const BvhArgs &bv, const LgArgs &lg, bool live,
                                         D3 o, D3 d, StackEnt *sbase, unsigned sidx, unsigned sstride, Work &work, unsigned &c_prim,
                                         unsigned &c_shadow, unsigned &c_reflect, D3 *park = nullptr) {
  int lev = 0;
  int dleft = depth;
  D3 res = mk(0.0, 0.0, 0.0);     // depth <= 0 -> black (main.cpp:17-18)
  bool alive = live && depth >= 1;
  const bool traced = alive;
  int key = -1;  // sphere the current ray leaves (-1: camera), groups lanes in sweeps
  c_prim += alive ? 1u : 0u;
  while (__ballot(alive)) {
    int outcome, nkey = 0;
    D3 color = kPark ? mk(0.0, 0.0, 0.0) : res, no = o, nd = d;
    double refl = 0.0;
    bounce<kCull, kArgMem>(g, rad, mat, slight, n, nl, amb, bv, lg, alive, o, d, key, dleft, work, c_shadow, outcome,
                           color, refl, no, nd, nkey);
    if (alive) {
      if (outcome == kSpawned) {
        sbase[RT_CK(kCkStack, sidx + (unsigned)lev * sstride, (long long)(depth - 1) * sstride)] =
            StackEnt{color.x, color.y, color.z, refl};
        ++lev;
        o = no;
        d = nd;
        key = nkey;
        --dleft;
        ++c_reflect;
      } else {
        if (kPark) park[threadIdx.x & 63] = color;
        else res = color;
        alive = false;
      }
    }
  }
  if (kPark && traced) res = park[threadIdx.x & 63];
  while (lev > 0) {  // unwind: shade*(1-refl) + reflected*refl, innermost first
    --lev;
    const StackEnt e = sbase[RT_CK(kCkStack, sidx + (unsigned)lev * sstride, (long long)(depth - 1) * sstride)];
    res = mk(e.ax + res.x * e.refl, e.ay + res.y * e.refl, e.az + res.z * e.refl);
  }
  return res;
}

// One 8x8 tile of pixels, one lane per pixel; `samples` = 1 (the serial
// path) or 4 (main_gpu.cu:249-333's antialias offsets, in fp64 serial
// semantics: samples summed in order, then * 0.25).  Adds the tile's ray
// counts to the wave sums.
struct CompactArgs {
  D3 *park;          // kStackGlobal with kernarg-resident arguments: this wave's parked colours (LDS)
  StackEnt *gstack;  // [depth-1][npx]
  size_t npx;        // level stride: pixels of all frames of the launch
  unsigned fpx;      // this wave's frame's first stack entry (frame * pixels per frame)
};

// Reflection stack placement: kStackGlobal = [level][pixel] in global memory
// (any depth, one tile per wave: trace_wave); kStackMerge = the same stack with
// merged reflection levels (merge_tiles, below).
enum { kStackGlobal = 1, kStackMerge = 4 };
template <bool kCull, int kSamples, int kStack, bool kArgMem = false>
__device__ __forceinline__ void trace_tile(const SphGeo *__restrict__ g, const double *__restrict__ rad,
                                           const SphMat *__restrict__ mat, const LightD *__restrict__ slight, int n,
                                           int nl, D3 amb, const Cam &cam, int W_arg, int H_arg, int depth,
                                           const Rows &rows_arg, const BvhArgs &bv, const LgArgs &lg,
                                           const OutDesc &od_arg, int x0, int k0, const CompactArgs &ca, Work &work,
                                           unsigned long long (&sums)[4], int frame = 0) {
  const int W = W_arg, H = H_arg;
  const Rows &rows = rows_arg;
  const OutDesc &od = od_arg;
  const int lane = threadIdx.x & 63;
  const int x = x0 + (lane & 7);
  const int k = k0 + (lane >> 3);
  const bool in_tile = x < W && x < od.x0 + od.xw && k < rows.count;
  const long long y = (long long)(k / rows.band) * rows.band * rows.stride + (long long)rows.first * rows.band +
                      (k % rows.band);
  const bool in_img = in_tile && y < H;
  const int j = H - 1 - (int)(in_img ? y : 0);  // reference row (main.cpp:74)
  unsigned c_prim = 0, c_shadow = 0, c_reflect = 0, c_neg = 0;
  D3 acc = mk(0.0, 0.0, 0.0);
#pragma unroll 1
  for (int s = 0; s < kSamples; ++s) {
    // Camera ray, camera.h:17-25 and main.cpp:151-154: ((u-0.5)*scale)*aspect,
    // aspect = 1.0; antialias offsets main_gpu.cu:253-256 (x + 0.0 == x exactly)
    const double ox = (double)(s & 1) * 0.5, oy = s >= 2 ? 0.5 : 0.0;
    const D3 dir = camera_dir(cam, (double)x + ox, (double)j + oy, W, H);
    const D3 d = renormalized(normalized(dir));  // get_ray normalises, Ray() normalises again
    const D3 o = mk(cam.px, cam.py, cam.pz);
    const int pix = k * od.xw + (x - od.x0);
    const D3 c = trace_wave<kCull, kArgMem, kArgMem>(g, rad, mat, slight, n, nl, amb, depth, bv, lg, in_img, o, d,
                                                     ca.gstack, (unsigned)pix + ca.fpx, (unsigned)ca.npx, work,
                                                     c_prim, c_shadow, c_reflect, ca.park);
    acc = kSamples == 1 ? c : add(acc, c);  // serial: the colour itself; AA: from 0 in sample order (main_gpu.cu:250, 327)
  }
  const D3 res = kSamples == 4 ? scale(acc, 0.25) : acc;  // main_gpu.cu:331, 1/4 is exact
  // The pixel's coordinates are recomputed from the lane id (mbcnt) rather
  // than kept live across the trace, which would spill them to scratch; the
  // output descriptors are re-read from the kernarg segment (kArgMem).
  {
    const OutDesc &od = kernarg_late<kArgMem, offsetof(RenderArgs, od)>(od_arg);
    const Rows &rows = kernarg_late<kArgMem, offsetof(RenderArgs, rows)>(rows_arg);
    const int W = kernarg_late<kArgMem, offsetof(RenderArgs, W)>(W_arg);
    const int H = kernarg_late<kArgMem, offsetof(RenderArgs, H)>(H_arg);
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int x = x0 + (lane & 7);
    const int k = k0 + (lane >> 3);
    const bool in_tile = x < W && x < od.x0 + od.xw && k < rows.count;
    const long long y = (long long)(k / rows.band) * rows.band * rows.stride + (long long)rows.first * rows.band +
                        (k % rows.band);
    const bool in_img = in_tile && y < H;
    const int j = H - 1 - (int)(in_img ? y : 0);
  if (od.fmt == RT_FB_RGB8) {
    // RGB8: a tile row of 8 pixels is 24 contiguous bytes.  When the whole row
    // is written and dword aligned, lanes 0-5 of the row store it as 6 dwords
    // assembled with two shuffles; otherwise every lane stores its 3 bytes.
    unsigned v = 0;  // r | g << 8 | b << 16
    if (in_img) {
      const int q0 = quantize(res.x), q1 = quantize(res.y), q2 = quantize(res.z);
      c_neg = (q0 < 0) + (q1 < 0) + (q2 < 0);
      v = (unsigned)(q0 < 0 ? 0 : q0) | (unsigned)(q1 < 0 ? 0 : q1) << 8 | (unsigned)(q2 < 0 ? 0 : q2) << 16;
    }
    const bool put = in_tile && (in_img || !od.full);  // padding rows of a shard are zero-filled
    const int c = lane & 7, rb = lane & ~7;
    const unsigned long long rowmask = 0xFFull << rb;
    const bool whole = (__ballot(put) & rowmask) == rowmask;
    uint8_t *row = static_cast<uint8_t *>(od.ptr) + (size_t)frame * (size_t)od.fstride +
                   ((size_t)(od.full ? y : k) * W + (x - c)) * 3;
    const bool packed = whole && ((reinterpret_cast<uintptr_t>(row) & 3u) == 0);
    const int p0 = (4 * c) / 3;  // dword c holds bytes 4c..4c+3: pixels p0, p0+1
    const unsigned v0 = __shfl(v, rb + (p0 < 7 ? p0 : 7), 64), v1 = __shfl(v, rb + (p0 + 1 < 7 ? p0 + 1 : 7), 64);
    if (packed) {
      if (c < 6) {
        const unsigned long long both = (unsigned long long)v0 | (unsigned long long)v1 << 24;
        reinterpret_cast<unsigned *>(row)[c] = (unsigned)(both >> (8 * (4 * c - 3 * p0)));
      }
    } else if (put) {
      uint8_t *px = row + c * 3;
      px[0] = (uint8_t)v;
      px[1] = (uint8_t)(v >> 8);
      px[2] = (uint8_t)(v >> 16);
    }
  } else if (in_tile && in_img) {
    const size_t i = ((size_t)j * W + x) * 3;
    if (od.fmt == RT_FB_F64X3) {
      double *f = static_cast<double *>(od.ptr) + i;
      f[0] = res.x;
      f[1] = res.y;
      f[2] = res.z;
    } else {
      float *f = static_cast<float *>(od.ptr) + i;
      f[0] = (float)res.x;
      f[1] = (float)res.y;
      f[2] = (float)res.z;
    }
  }
  }
  sums[0] += wave_sum(c_prim);
  sums[1] += wave_sum(c_shadow);
  sums[2] += wave_sum(c_reflect);
  sums[3] += wave_sum(c_neg);
}

// kStackMerge: one wave traces kMergeTiles tiles and merges their reflection
// rays before tracing them.  Level 0 runs tile by tile (one lane per pixel,
// coherent); a pixel whose chain ends there is stored at once.  The rays it
// spawns (typically a handful per tile: 0.34 M reflection rays for 2.07 M
// pixels on synth200) wait in a per-wave LDS queue (< 64 entries) until a
// tile's spawns and the queue fill a wave: then those 64 rays run their
// remaining levels together (chain), each lane unwinding its own pixel's
// [level][pixel] stack and storing it.  So the incoherent levels cost one
// wave pass per 64 rays instead of one per tile that has any: measured per
// reflection level, level 2 of synth200 (41 K rays) cost 0.047 ms and level 3
// (8 K rays) 0.021 ms with one tile per wave.  No barriers: the wave is its
// own workgroup.  RGB8 row-compact output, one sample per pixel.
#ifndef RT_MERGE_TILES
#define RT_MERGE_TILES 4
#endif
constexpr int kMergeTiles = RT_MERGE_TILES;
// Rays of reflection level >= kDeferLevel leave the merged megakernel for
// render_deferred, a second kernel over all deferred rays of the launch; the
// per-shard count lives in u64 slot kDeferSlot of the launch's counter shards.
#ifndef RT_DEFER_LEVEL
#define RT_DEFER_LEVEL 2
#endif
constexpr int kDeferLevel = RT_DEFER_LEVEL;
#ifndef RT_DEFER_WGS
#define RT_DEFER_WGS 48  // render_deferred workgroups (one wave each) per shard segment
#endif
#ifndef RT_DEFER_CAP_DIV
#define RT_DEFER_CAP_DIV 8  // deferred-queue room: 1 / RT_DEFER_CAP_DIV of the launch's pixels
#endif
constexpr int kDeferSlot = 7;
// merge_tiles' LDS: the finished pixels (RGB8, 192 B per tile), then the tile ids
constexpr size_t kPixbufIds = (size_t)kMergeTiles * 64 * 3;
constexpr size_t kPixbufBytes = kPixbufIds + (size_t)kMergeTiles * 8;  // + (tile id, row-0 offset) per tile
// u64 slot of a counter shard: the deferred kernels' next queue entry of that
// shard segment (lanes take entries dynamically; zeroed with the launch's counters)
constexpr int kFetchSlot = 24;
constexpr long long kSchedMinTiles = 1024;  // launches with fewer 8x8 tiles keep scanline order

// A pixel's final colour quantised as write_ppm (main.cpp:85), packed r | g << 8 | b << 16.
__device__ __forceinline__ unsigned pack_px(D3 c, unsigned &c_neg) {
  const int q0 = quantize(c.x), q1 = quantize(c.y), q2 = quantize(c.z);
  c_neg += (q0 < 0) + (q1 < 0) + (q2 < 0);
  return (unsigned)(q0 < 0 ? 0 : q0) | (unsigned)(q1 < 0 ? 0 : q1) << 8 | (unsigned)(q2 < 0 ? 0 : q2) << 16;
}

// A deferred ray's pixel (render_deferred*): its 3 bytes at out + 3 pix are
// OR-ed into the one or two dwords that hold them.  merge_tiles stored the
// pixel's tile as dword rows with zero bytes in this pixel's place, and the
// neighbours in those dwords may be other deferred pixels being OR-ed at the
// same time: a dword atomic OR per covered dword, no byte stores.
__device__ __forceinline__ void or_px(uint8_t *out, unsigned pix, unsigned v) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(out) + (uintptr_t)pix * 3;
  unsigned *d = reinterpret_cast<unsigned *>(a & ~(uintptr_t)3);
  const unsigned sh = (unsigned)(a & 3) * 8;
  const unsigned long long w = (unsigned long long)v << sh;  // bytes sh/8 .. sh/8 + 2 of a dword pair
  if ((unsigned)w) atomicOr(d, (unsigned)w);
  if (sh > 8 && (unsigned)(w >> 32)) atomicOr(d + 1, (unsigned)(w >> 32));
}

// kMergeTiles tiles of one frame for one wave (see kStackMerge).  Every lane
// holds at most one ray: (o, d, key = the sphere it leaves, dleft = depth
// left, pix, lev = stack entries its pixel has).  One bounce() per iteration
// for all lanes holding a ray:
//   * a tile pass loads the next tile's camera rays into all lanes (level 0);
//     the reflection rays it spawns join the queue unless they and the queue
//     fill the wave (or no tile is left), then the queued rays fill the lanes
//     that spawned none;
//   * a chain pass bounces the lanes' rays (any level >= 1) and refills the
//     lanes whose chain ended from the queue.
// A chain that ends unwinds its pixel's stack (sbase[sidx + level * sstride],
// innermost first, main.cpp:54) and stores the pixel.
// One pixel's 3 bytes at p (any alignment) written with dword atomics: its
// bytes of each covering dword cleared (AND), then set (OR); the other bytes,
// other pixels', are untouched whoever writes them meanwhile.
__device__ __forceinline__ void put_px(uint8_t *p, unsigned v) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  unsigned *d = reinterpret_cast<unsigned *>(a & ~(uintptr_t)3);
  const unsigned sh = (unsigned)(a & 3) * 8;
  const unsigned long long m = 0xFFFFFFull << sh, w = (unsigned long long)v << sh;
  atomicAnd(d, ~(unsigned)m);
  if ((unsigned)w) atomicOr(d, (unsigned)w);
  if (sh > 8) {
    atomicAnd(d + 1, ~(unsigned)(m >> 32));
    if ((unsigned)(w >> 32)) atomicOr(d + 1, (unsigned)(w >> 32));
  }
}

// The finished pixels of a merge_tiles group wait in LDS as RGB8 bytes laid
// out like the tiles' rows (tile slot t, row y, pixel x at t * 192 + y * 24 +
// x * 3) until every pixel of their tile is final, then go out as the tile's
// 24-byte rows, one dword per lane (flush_tile); a deferred pixel's bytes stay
// 0 for render_deferred's or_px.
typedef __attribute__((address_space(3))) unsigned char LdsU8;
typedef __attribute__((address_space(3))) unsigned LdsU32;
__device__ __forceinline__ void flush_tile(const RenderArgs &a, int tile, int frame, const LdsU8 *pb) {
  const int lane = (int)(threadIdx.x & 63);
  const OutDesc &od = kernarg_late<true, offsetof(RenderArgs, od)>(a.od);
  const Rows &rows = kernarg_late<true, offsetof(RenderArgs, rows)>(a.rows);
  const int W = kernarg_late<true, offsetof(RenderArgs, W)>(a.W);
  const int ntx = kernarg_late<true, offsetof(RenderArgs, ntx)>(a.ntx);
  const int rows_dword = kernarg_late<true, offsetof(RenderArgs, rows_dword)>(a.rows_dword);
  uint8_t *out = static_cast<uint8_t *>(od.ptr) + (size_t)frame * (size_t)od.fstride;
  const int x0 = (tile % ntx) * 8, ty = tile / ntx;
  // a row of 8 pixels is 24 bytes = 6 dwords when it is whole and dword aligned
  auto row_at = [&](int r) { return out + ((size_t)(ty * 8 + r) * W + x0) * 3; };
  if (rows_dword && x0 + 8 <= W && ty * 8 + 8 <= rows.count) {  // wave-uniform: the usual case
    if (lane < 48) {  // lane: row lane / 6, dword lane % 6 = LDS dword lane
      const unsigned v = reinterpret_cast<const LdsU32 *>(pb)[lane];
      *reinterpret_cast<unsigned *>(row_at(0) + (unsigned)(lane / 6) * (unsigned)W * 3u +
                                    4u * (unsigned)(lane - 6 * (lane / 6))) = v;
    }
    return;
  }
  auto whole = [&](int r) {
    return ty * 8 + r < rows.count && x0 + 8 <= W && (reinterpret_cast<uintptr_t>(row_at(r)) & 3) == 0;
  };
  {
    const int r = lane / 6, c = lane - 6 * (lane / 6);  // lanes 0..47: row r, dword c = LDS dword lane
    if (lane < 48 && whole(r)) reinterpret_cast<unsigned *>(row_at(r))[c] = reinterpret_cast<const LdsU32 *>(pb)[lane];
  }
  {
    // rows that are not whole (the image's right edge, odd widths): the
    // lane's own pixel into the dwords it shares with its neighbours (which
    // other waves may be writing): its bytes cleared and set by dword atomics
    const int r = lane >> 3, x = x0 + (lane & 7);
    if (!whole(r) && ty * 8 + r < rows.count && x < W) {
      const LdsU8 *p = pb + lane * 3;
      put_px(row_at(r) + (lane & 7) * 3, (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16);
    }
  }
}

// A merged wave's reflection stack lives in a "home": [depth-1][kMergeTiles *
// 64] entries, one per pixel of its group (lidx) and level, taken from the
// context's pool when the wave's first reflection ray spawns and returned
// when the wave ends.  The pool has twice as many homes as waves can be
// resident on the device (the host sizes it by the occupancy API), so a free
// one exists whenever a wave asks; the bitmap is searched from a word picked
// by the workgroup id, one atomic OR per try.  The stack memory of a launch
// is bounded by the pool, not by its pixels (kStackGlobal keeps the
// per-pixel stack).
constexpr int kHomePx = kMergeTiles * 64;
__device__ __forceinline__ int home_acquire(unsigned long long *bits, int nwords) {
  int h = -1;
  if ((threadIdx.x & 63) == 0) {
    int w = (int)(blockIdx.x % (unsigned)nwords);
    // the first try: a bit picked by the workgroup id as well (a half-full word
    // then takes one atomic, not two); it learns the word.  (Lowest-free-bit
    // first, to keep the homes in use few and L2-resident, measured the same
    // HBM writes and frame time: profiles/r7f/.)
    unsigned long long cur = ~(1ull << ((blockIdx.x / (unsigned)nwords) & 63u));
#ifdef RT_CHECK
    long long spins = 0;
#endif
    while (h < 0) {
      while (~cur) {
        const int bit = __builtin_ctzll(~cur);
        const unsigned long long old = atomicOr(bits + w, 1ull << bit);
        if (!((old >> bit) & 1ull)) {
          h = w * 64 + bit;
          break;
        }
        cur = old | (1ull << bit);
      }
      if (h < 0) {
        w = w + 1 == nwords ? 0 : w + 1;
        cur = 0ull;
#ifdef RT_CHECK
        // the pool holds twice the resident waves, so a wave finds a home
        // within a sweep or two; a wave still spinning after kHomeSweeps full
        // sweeps means a leaked home or an under-sized pool: record it and
        // share home 0 (wrong pixels, RT_ERR_CHECK) so the launch drains
        // instead of hanging
        constexpr long long kHomeSweeps = 4096;
        if (++spins >= kHomeSweeps * nwords) {
          ck_fail(kCkHome, spins, kHomeSweeps * nwords);
          h = 0;
        }
#endif
      }
    }
  }
  return __shfl(h, 0, 64);
}
__device__ __forceinline__ void home_release(unsigned long long *bits, int h) {
  if ((threadIdx.x & 63) == 0) atomicAnd(bits + (h >> 6), ~(1ull << (h & 63)));
}

template <bool kCull, bool kFast, bool kWide = false>
__device__ __forceinline__ void merge_tiles(const SphGeo *__restrict__ g, const double *__restrict__ rad,
                                            const SphMat *__restrict__ mat, const LightD *__restrict__ slight,
                                            const RenderArgs &a, int group, int frame, const CompactArgs &ca,
                                            QRay *q, Work &work, unsigned long long (&sums)[4]) {
  const int lane = (int)(threadIdx.x & 63);
  const unsigned long long lt = (1ull << lane) - 1ull;
  unsigned c_prim = 0, c_shadow = 0, c_reflect = 0, c_neg = 0;
  // the finished pixels (flush_tile), at an LDS offset the host placed after the walk stacks
  auto pixbuf = [&]() { return (LdsU8 *)rt_dyn_lds + kernarg_late<true, offsetof(RenderArgs, pix_off)>(a.pix_off); };
#pragma unroll
  for (int i = 0; i < (int)((kPixbufIds + 255) / 256); ++i)  // padding, depth 0 and deferred pixels: 0
    if ((size_t)(i * 256 + lane * 4) < kPixbufIds) reinterpret_cast<LdsU32 *>(pixbuf())[i * 64 + lane] = 0u;
  const int depth = a.depth;
  int qn = 0;        // queued rays q[0 .. qn), wave-uniform, < Q between passes
  const int Q = kernarg_late<true, offsetof(RenderArgs, merge_q)>(a.merge_q);
  int next = 0;      // next tile of the group
  bool act = false;  // this lane holds a ray
  D3 o = mk(0.0, 0.0, 0.0), d = o;
  int key = -1, dleft = 0, lev = 0;
  unsigned pix = 0;
  int lidx = 0;  // the pixel's place in the group: tile slot * 64 + y * 8 + x (pixbuf byte 3 * lidx)
  int home = -1;  // the group's stack home (home_acquire), once a reflection ray spawned
  auto hs = [&]() {
    return kernarg_late<true, offsetof(RenderArgs, homes)>(a.homes) + (size_t)home * (size_t)(depth - 1) * kHomePx;
  };
  auto hslot = [&](int l) {
    return RT_CK(kCkStack, (size_t)l * kHomePx + (size_t)lidx, (long long)(depth - 1) * kHomePx);
  };
  // pops queued rays into the lanes without one (lanes ranked by lane id)
  auto refill = [&](unsigned long long busy) {
    const int take = (64 - __popcll(busy)) < qn ? (64 - __popcll(busy)) : qn;
    const int r = (int)__popcll(~busy & lt);
    if (!act && r < take) {
      const QRay &e = q[RT_CK(kCkLdsQueue, qn - 1 - r, Q)];
      o = mk(e.ox, e.oy, e.oz);
      d = mk(e.dx, e.dy, e.dz);
      key = e.key;
      dleft = e.dleft;
      pix = (unsigned)e.pix;
      lidx = e.orig;
      lev = 1;
      act = true;
    }
    qn -= take;
  };
  while (true) {
    // the group's tile slots: [base, base + nt) -- one slot for the first nsingle
    // groups (the heaviest tiles: their own reflection rays fill the wave, and
    // a frame's critical path is its slowest wave), kMergeTiles up to
    // merge_end, then one slot per group again (the launch's last, lightest
    // tiles: the waves that end a launch are short, so fewer slots idle while
    // the last ones finish)
    const int ns = kernarg_late<true, offsetof(RenderArgs, nsingle)>(a.nsingle);
    const int me = kernarg_late<true, offsetof(RenderArgs, merge_end)>(a.merge_end);
    const int nm = (me - ns + kMergeTiles - 1) / kMergeTiles;
    int base, nt;
    if (group < ns) {
      base = group, nt = 1;
    } else if (group < ns + nm) {
      base = ns + (group - ns) * kMergeTiles, nt = me - base < kMergeTiles ? me - base : kMergeTiles;
    } else {
      base = me + (group - ns - nm), nt = 1;
    }
    bool tile_pass = false;
    if (__ballot(act) == 0) {
      if (next < nt) {  // camera rays of the next tile: camera.h:17-25, main.cpp:151-154 (as trace_tile)
        const int *perm = kernarg_late<true, offsetof(RenderArgs, perm)>(a.perm);
        const int slot = base + next;
        const int tile = RT_CK(kCkTile, perm ? perm[RT_CK(kCkTile, slot, a.ntiles)] : slot, a.ntiles);
        const int ntx = kernarg_late<true, offsetof(RenderArgs, ntx)>(a.ntx);
        const int tx = tile % ntx, ty = tile / ntx;
        const OutDesc &od = kernarg_late<true, offsetof(RenderArgs, od)>(a.od);
        const Rows &rows = kernarg_late<true, offsetof(RenderArgs, rows)>(a.rows);
        const int W = kernarg_late<true, offsetof(RenderArgs, W)>(a.W);
        const int H = kernarg_late<true, offsetof(RenderArgs, H)>(a.H);
        const int x = tx * 8 + (lane & 7);
        const int k = ty * 8 + (lane >> 3);
        const bool in_tile = x < W && k < rows.count;
        const long long y = (long long)(k / rows.band) * rows.band * rows.stride +
                            (long long)rows.first * rows.band + (k % rows.band);
        const bool in_img = in_tile && y < H;
        const int j = H - 1 - (int)(in_img ? y : 0);  // reference row (main.cpp:74)
        const Cam &cam = kernarg_cam(frame);
        // the launch's ray table (the frames share the orientation, the image and the rows): this tile's
        // directions as ray_table_kernel formed them, with these same expressions
        if (const double *dirs = kernarg_late<true, offsetof(RenderArgs, dirs)>(a.dirs)) {
          const double *tb = dirs + (size_t)tile * kRayTileDoubles;
          d = mk(tb[lane], tb[64 + lane], tb[128 + lane]);
        } else {
          const D3 dir = camera_dir(cam, (double)x, (double)j, W, H);
          d = renormalized(normalized(dir));
        }
        o = mk(cam.px, cam.py, cam.pz);
        pix = (unsigned)(k * W + x);
        lidx = next * 64 + lane;
        key = -1;
        dleft = depth;
        lev = 0;
        act = in_img && depth >= 1;
        c_prim += act ? 1u : 0u;
        // depth <= 0 -> black (main.cpp:17-18), padding rows -> zeros: pixbuf's 0
        (void)od;
        // for the flush at the group's end: the tile id and, when the tile is
        // whole and its rows dword aligned, the byte offset of its first row in
        // the frame (else ~0: flush_tile's general path)
        if (lane == 0) {
          const size_t off = ((size_t)ty * 8 * W + (size_t)tx * 8) * 3;
          const bool whole = kernarg_late<true, offsetof(RenderArgs, rows_dword)>(a.rows_dword) && tx * 8 + 8 <= W &&
                             ty * 8 + 8 <= rows.count && off < 0xFFFFFFFFull;
          LdsU32 *ids = reinterpret_cast<LdsU32 *>(pixbuf() + kPixbufIds);
          ids[2 * next] = (unsigned)tile;
          ids[2 * next + 1] = whole ? (unsigned)off : 0xFFFFFFFFu;
        }
        ++next;
        tile_pass = true;
        if (__ballot(act) == 0) continue;
      } else if (qn > 0) {
        refill(0ull);
      } else {
        break;
      }
    }
    int outcome = 0, nkey = 0;
    D3 color = mk(0.0, 0.0, 0.0), no = o, nd = d;
    double refl = 0.0;
    double bt;
    const int bi = closest_hit<kCull, true, kFast>(g, rad, a.n, a.bv, act, o, d, key, work, bt,
                                             kFast && tile_pass && kernarg_late<true, offsetof(RenderArgs, cg)>(a.cg).on,
                                             frame);
    shade_hit<kCull, true, kFast, kWide>(g, rad, mat, slight, a.n, a.nl, a.amb, a.bv, a.lg, act, o, d, key, dleft, bi, bt,
                                  work, c_shadow, outcome, color, refl, no, nd, nkey);
    const unsigned sidx = pix + ca.fpx;
    bool defer = false;
    if (home < 0 && __ballot(act && outcome == kSpawned))
      home = home_acquire(kernarg_late<true, offsetof(RenderArgs, home_bits)>(a.home_bits),
                          kernarg_late<true, offsetof(RenderArgs, home_words)>(a.home_words));
    if (act) {
      if (outcome == kSpawned) {
        hs()[hslot(lev)] = StackEnt{color.x, color.y, color.z, refl};
        ++lev;
        o = no;
        d = nd;
        key = nkey;
        --dleft;
        ++c_reflect;
        defer = lev >= kernarg_late<true, offsetof(RenderArgs, defer_level)>(a.defer_level);
      } else {  // the chain ends: unwind its pixel's stack and store it
        D3 res = color;
        while (lev > 0) {
          --lev;
          const StackEnt e = hs()[hslot(lev)];
          res = mk(e.ax + res.x * e.refl, e.ay + res.y * e.refl, e.az + res.z * e.refl);
        }
        {
          const unsigned v = pack_px(res, c_neg);
          LdsU8 *p = pixbuf() + 3 * RT_CK(kCkPixbuf, lidx, kMergeTiles * 64);
          p[0] = (unsigned char)v;
          p[1] = (unsigned char)(v >> 8);
          p[2] = (unsigned char)(v >> 16);
        }
        act = false;
      }
    }
    // rays of level >= kDeferLevel go to the launch's deferred queue (render_deferred),
    // as far as its shard segment has room; the others continue here
    const unsigned long long dm = __ballot(defer);
    if (dm) {
      const int cap = kernarg_late<true, offsetof(RenderArgs, dq_cap)>(a.dq_cap);
      if (cap > 0) {
        unsigned long long base = 0;
        const int first = __builtin_ctzll(dm);
        if (lane == first) base = atomicAdd(&counter_shard(kernarg_late<true, offsetof(RenderArgs, counters)>(a.counters))[kDeferSlot],
                                            (unsigned long long)__popcll(dm));
        base = __shfl(base, first, 64);
        const unsigned long long slot = base + (unsigned long long)__popcll(dm & lt);
        if (defer && slot < (unsigned long long)cap) {
          QRay *dq = kernarg_late<true, offsetof(RenderArgs, dq)>(a.dq);
          const unsigned wg = blockIdx.x;
          const size_t gslot = RT_CK(kCkDeferQ, (size_t)(wg % kShards) * (size_t)cap + slot, (long long)kShards * cap);
          dq[gslot] = QRay{o.x, o.y, o.z, d.x, d.y, d.z, lev, dleft, key, (int)sidx};
          // its stack entries so far go with it: render_deferred continues the chain at its queue slot
          StackEnt *ds = kernarg_late<true, offsetof(RenderArgs, dstack)>(a.dstack);
          const size_t dtot = (size_t)kShards * (size_t)cap;
          for (int l = 0; l < lev; ++l)
            ds[RT_CK(kCkStack, (size_t)l * dtot + gslot, (long long)(depth - 1) * (long long)dtot)] = hs()[hslot(l)];
          act = false;
        }
      }
    }
    const unsigned long long busy = __ballot(act);
    if (tile_pass && next < nt && __popcll(busy) + qn < Q) {
      // this tile's reflection rays wait for the next tiles' (queue < Q entries)
      if (act)
        q[RT_CK(kCkLdsQueue, qn + (int)__popcll(busy & lt), Q)] =
            QRay{o.x, o.y, o.z, d.x, d.y, d.z, lidx, dleft, key, (int)pix};
      qn += __popcll(busy);
      act = false;
    } else if (qn > 0 && busy != ~0ull) {
      refill(busy);  // lanes without a ray take queued ones
    }
  }
  // every pixel of the group is final (or deferred, 0 bytes): its tiles go
  // out, a whole aligned tile as 48 dword stores at its recorded offset
  {
    const OutDesc &od = kernarg_late<true, offsetof(RenderArgs, od)>(a.od);
    const int W = kernarg_late<true, offsetof(RenderArgs, W)>(a.W);
    uint8_t *out = static_cast<uint8_t *>(od.ptr) + (size_t)frame * (size_t)od.fstride;
    const unsigned roff = (unsigned)(lane / 6) * (unsigned)W * 3u + 4u * (unsigned)(lane - 6 * (lane / 6));
    const LdsU32 *ids = reinterpret_cast<const LdsU32 *>(pixbuf() + kPixbufIds);
#pragma unroll
    for (int t = 0; t < kMergeTiles; ++t) {
      if (t >= next) break;
      const unsigned off = __builtin_amdgcn_readfirstlane(ids[2 * t + 1]);
      if (off != 0xFFFFFFFFu) {
        if (lane < 48) {
          const unsigned v = reinterpret_cast<const LdsU32 *>(pixbuf() + 192 * t)[lane];
          *reinterpret_cast<unsigned *>(
              out + RT_CK(kCkOut, (size_t)off + roff,
                          (long long)(kernarg_late<true, offsetof(RenderArgs, rows)>(a.rows).count) * W * 3 - 3)) = v;
        }
      } else {
        flush_tile(a, (int)__builtin_amdgcn_readfirstlane(ids[2 * t]), frame, pixbuf() + 192 * t);
      }
    }
  }
  if (home >= 0) home_release(kernarg_late<true, offsetof(RenderArgs, home_bits)>(a.home_bits), home);
  sums[0] += wave_sum(c_prim);
  sums[1] += wave_sum(c_shadow);
  sums[2] += wave_sum(c_reflect);
  sums[3] += wave_sum(c_neg);
}

// Flushes a wave's ray counts and work counters into its counter shard.
// Called with every lane of the wave active (the per-lane work counters are
// summed over the wave here).
__device__ __forceinline__ void flush_counts(unsigned long long *counters, const unsigned long long (&sums)[4],
                                             const Work &work) {
  const unsigned long long exact = wave_sum64(work.exact), cull = wave_sum64(work.cull);
#ifdef RT_STAMPS
  const unsigned long long trip_sh = wave_sum64(work.trip_sh), trip_scan = wave_sum64(work.trip_scan),
                           trip_leaf = wave_sum64(work.trip_leaf);
#endif
  if ((threadIdx.x & 63) == 0) {
    unsigned long long *sc = counter_shard(counters);
#ifdef RT_STAMPS
    atomicAdd(&sc[25], trip_sh);
    atomicAdd(&sc[26], trip_scan);
    atomicAdd(&sc[27], trip_leaf);
    for (int q = 0; q < 6; q++) atomicAdd(&sc[8 + q], work.st[q]);
    atomicAdd(&sc[20], work.st[6]);
    atomicAdd(&sc[21], work.st[8]);  // closest hits
    atomicAdd(&sc[22], work.st[9]);  // shadow queries
    atomicAdd(&sc[14], 1ull);
    atomicAdd(&sc[15], work.iters);
    atomicAdd(&sc[16], work.sweeps);
    atomicAdd(&sc[17], work.it_closest);
    atomicAdd(&sc[18], work.sw_closest);
    atomicAdd(&sc[19], work.it_prim);
#endif
    for (int q = 0; q < 4; q++)
      if (sums[q]) atomicAdd(&sc[q], sums[q]);
    if (exact) atomicAdd(&sc[4], exact);
    if (cull) atomicAdd(&sc[5], cull);
  }
}

#ifdef RT_STAMPS
__device__ __forceinline__ void record_timeline(unsigned wave_id, unsigned long long t_real0, const Work &work) {
  const int lane = threadIdx.x & 63;
  const unsigned long long bvh_steps_max = (unsigned long long)wmax((double)work.st[7]);
  const unsigned long long wave_trips = wave_sum((unsigned)work.st[10]);
  if (lane == 0) {
    const unsigned wid = wave_id;
    if (wid < (unsigned)kTimelineWaves) {
      unsigned long long *tl = g_timeline + (size_t)kTl * wid;
      tl[0] = t_real0;
      tl[1] = __builtin_amdgcn_s_memrealtime();
      const unsigned hw = __builtin_amdgcn_s_getreg(4 | (31 << 11));
      const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11));
      tl[2] = ((unsigned long long)xcc << 32) | hw;
      tl[3] = work.st[0];  // bound cycles
      tl[4] = work.st[1];  // cull
      tl[5] = work.st[2];  // candidates
      tl[6] = work.st[4];  // shading
      tl[7] = work.st[5];  // total
      tl[8] = work.iters | (work.sweeps << 32);
      tl[10] = work.st[6];  // bvh walks
      tl[11] = work.st[3];  // per-light setup
      tl[12] = work.st[8];  // closest sweeps
      tl[13] = work.st[9];  // shadow sweeps
      tl[14] = wave_trips;  // bvh loop trips of the wave
      tl[9] = bvh_steps_max;  // most BVH node visits of one lane
    }
  }
}
#endif

#ifndef RT_MIN_WAVES_PER_EU
#define RT_MIN_WAVES_PER_EU 3  // caps VGPRs at 168: three waves per SIMD
#endif
// Waves per render_kernel workgroup: 4 (2x2 tiles of 8x8 pixels) when the
// workgroup shares a scene staged in LDS; 1 otherwise, so no wave's slot
// waits for its slowest neighbour.
template <bool kLdsGeo>
constexpr int wg_waves() {
  return kLdsGeo ? 4 : 1;
}

template <bool kLdsGeo, bool kCull, int kSamples, int kStack, bool kFast = false, bool kWide = false>
__global__ __launch_bounds__((64 * wg_waves<kLdsGeo>()), RT_MIN_WAVES_PER_EU) void render_kernel(
    const RenderArgs a) {
  // Workgroups are dealt to the 8 XCDs round robin (b % 8), so every image
  // region is spread over all XCDs.  perm: the host's launch order (rt_sched.h).
  const int b = blockIdx.x;
  if (b == 0 && a.zero_next)
    for (int i = (int)threadIdx.x; i < kShards * kShardStride; i += (int)blockDim.x) a.zero_next[i] = 0ull;
  // the frames of a multi-frame launch share the tile order, so every frame's
  // copy of a heavy tile starts early.  Workgroups are dealt to the 8 XCDs
  // round robin (b % 8); with xcd_frames the k-th workgroup of XCD x renders
  // frame k % F of tile group 8 (k / F) + x, so all F copies of a group run on
  // the XCD whose L2 holds that group's scene lists and nodes (the grid is
  // padded to a multiple of 8 groups; the padding exits); otherwise the F
  // copies of a group are adjacent (b / F, b % F) and spread over the XCDs
  const int nf = a.frames;
  int slot = b, frame = 0;
  if (nf > 1) {
    if (a.xcd_frames) {
      const int k = b >> 3;
      slot = (k / nf) * 8 + (b & 7);
      frame = k - (k / nf) * nf;
    } else {
      slot = b / nf;
      frame = b - slot * nf;
    }
  }
  int tile = slot;
  if constexpr (kStack == kStackMerge) {
    if (slot >= a.nslots) return;  // slot = this wave's group of tile slots (merge_tiles)
  } else {
    if (a.perm) {
      if (slot >= a.nslots) return;
      tile = a.perm[RT_CK(kCkTile, slot, a.nslots)];  // heaviest predicted tiles first, or a batch's listed blocks
    }
    if (tile >= a.ntiles) return;  // workgroup-uniform, before any barrier
  }
  const int tx = tile % a.ntx, ty = tile / a.ntx;
  extern __shared__ __attribute__((aligned(32))) unsigned char smem[];
  const SphGeo *g;
  const double *rad;
  const LightD *slight;
  const SphMat *sm;
  // With the scene staged in LDS the BVH arguments are a modified local copy;
  // otherwise the kernel argument itself is used (re-read from the kernarg
  // segment where needed: kernarg_late) and the ordered walk finds its LDS
  // stacks at bv.ostk_off (set by the host).
  BvhArgs bv_local = a.bv;
  stage_scene<kLdsGeo>(smem, a.geo, a.radius, a.mat, a.lights, a.n, a.nl, bv_local, g, rad, sm, slight);
  const size_t stack_off = (lds_layout(kLdsGeo, a.n, a.nl, a.bv.nnodes).end + 31) & ~(size_t)31;
  // the ordered BVH walk's per-lane stacks, [wave][entry][lane], after the scene
  if (kLdsGeo && bv_local.ordered)
    bv_local.ostk = reinterpret_cast<int2 *>(smem + stack_off) + (size_t)(threadIdx.x >> 6) * bv_local.odepth * 64;
  const BvhArgs &bv = kLdsGeo ? bv_local : a.bv;
  constexpr int kWg = wg_waves<kLdsGeo>();
  constexpr int kWx = kWg == 4 ? 2 : 1;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: keeps tile coordinates in SGPRs
  CompactArgs ca;
  ca.park = nullptr;
  if (!kLdsGeo)  // after the ordered walk's stacks (launch_tiles sizes both)
    ca.park = reinterpret_cast<D3 *>(smem + stack_off + (a.bv.ordered ? (size_t)kWg * a.bv.odepth * 64 * sizeof(int2) : 0)) +
              (size_t)wave * 64;
  ca.gstack = a.gstack;
  ca.npx = (size_t)a.rows.count * a.od.xw * nf;
  ca.fpx = (unsigned)((size_t)a.rows.count * a.od.xw * frame);
  Work work;
  unsigned long long sums[4] = {0, 0, 0, 0};
  RT_T0(t_wave);
#ifdef RT_STAMPS
  const unsigned long long t_real0 = __builtin_amdgcn_s_memrealtime();
#endif
  if constexpr (kStack == kStackMerge && !kLdsGeo && kSamples == 1) {
    // the wave's ray queue sits where trace_wave parks colours, after the
    // finished-pixel bytes (launch_tiles)
    QRay *q = reinterpret_cast<QRay *>(reinterpret_cast<unsigned char *>(ca.park) + kPixbufBytes);
    merge_tiles<kCull, kFast, kWide>(g, rad, sm, slight, a, slot, frame, ca, q, work, sums);
  } else {
    trace_tile<kCull, kSamples, kStack, !kLdsGeo>(g, rad, sm, slight, a.n, a.nl, a.amb, kernarg_cam(frame), a.W, a.H,
                                                  a.depth, a.rows, bv, a.lg, a.od,
                                                  a.od.x0 + tx * (8 * kWx) + (wave % kWx) * 8,
                                                  ty * (8 * (kWg / kWx)) + (wave / kWx) * 8, ca, work,
                                                  sums, frame);
  }
  RT_ACC(work, 5, t_wave);
#ifdef RT_STAMPS
  // merged kernels: one entry per workgroup of the launch (slot b = group b / F of frame b % F)
  record_timeline(kStack == kStackMerge ? (unsigned)blockIdx.x : (unsigned)(tile * kWg + wave), t_real0, work);
#endif
  flush_counts(kernarg_late<!kLdsGeo, offsetof(RenderArgs, counters)>(a.counters), sums, work);
}

// The deferred rays of a kStackMerge launch (level >= kDeferLevel, typically
// 2-3 % of its rays but the least coherent): one wave per workgroup,
// workgroup b serves shard segment b % kShards and takes its chunks of 64
// rays b / kShards, + gridDim / kShards, ...  Each lane runs its ray's chain
// to the end exactly as merge_tiles would have (bounce, stack entries at its
// queue slot's [level][slot] entries of dstack), unwinds the chain's whole
// stack -- the levels merge_tiles copied there at the deferral first -- and
// stores the pixel.
template <bool kCull, bool kFast = false, bool kWide = false>
__global__ __launch_bounds__(64, RT_MIN_WAVES_PER_EU) void render_deferred(const RenderArgs a) {
  const unsigned shard = blockIdx.x % kShards, first = blockIdx.x / kShards;
  const int cap = a.dq_cap;
  const unsigned long long cnt = a.counters[(size_t)shard * kShardStride + kDeferSlot];
  const unsigned n_dq = (unsigned)(cnt < (unsigned long long)cap ? cnt : (unsigned long long)cap);
  if (first * 64u >= n_dq) return;
  const int lane = (int)(threadIdx.x & 63);
  const unsigned npx_frame = (unsigned)((size_t)a.rows.count * a.od.xw);
  const unsigned sstride = (unsigned)kShards * (unsigned)cap;  // the chain's stack: dstack[level][queue slot]
  Work work;
  unsigned c_shadow = 0, c_reflect = 0, c_neg = 0;
  // Lanes without a ray take the shard segment's next entries (one
  // wave-aggregated atomic on its fetch slot), so the wave stays full until
  // the segment runs out and the workgroups of a segment finish together
  // instead of each finishing its own static stream's longest chains.
  const unsigned long long lt = (1ull << lane) - 1ull;
  bool act = false, more = true;
  D3 o = mk(0.0, 0.0, 0.0), d = o;
  int key = -1, dleft = 0, lev = 0;
  unsigned pixg = 0, qslot = 0;  // the ray's output pixel (launch index) and queue slot
  unsigned long long *fetch = kernarg_late<true, offsetof(RenderArgs, counters)>(a.counters) +
                              (size_t)shard * kShardStride + kFetchSlot;
  while (true) {
    const unsigned long long idle = ~__ballot(act);
    if (idle && more) {
      const int fi = __builtin_ctzll(idle);
      unsigned long long base = 0;
      if (lane == fi) base = atomicAdd(fetch, (unsigned long long)__popcll(idle));
      base = __shfl(base, fi, 64);
      const unsigned long long i = base + (unsigned long long)__popcll(idle & lt);
      more = base + (unsigned long long)__popcll(idle) < n_dq;
      if (!act && i < n_dq) {
        const QRay &e = kernarg_late<true, offsetof(RenderArgs, dq)>(a.dq)[RT_CK(kCkDeferQ, (size_t)shard * (size_t)cap + i, (long long)kShards * cap)];
        o = mk(e.ox, e.oy, e.oz);
        d = mk(e.dx, e.dy, e.dz);
        lev = e.orig;
        dleft = e.dleft;
        key = e.key;
        pixg = (unsigned)e.pix;
        qslot = shard * (unsigned)cap + (unsigned)i;
        act = true;
      }
    }
    if (__ballot(act) == 0) break;
    {
      int outcome = 0, nkey = 0;
      D3 color = mk(0.0, 0.0, 0.0), no = o, nd = d;
      double refl = 0.0;
      bounce<kCull, true, kFast, kWide, false>(a.geo, a.radius, a.mat, a.lights, a.n, a.nl, a.amb, a.bv, a.lg, act, o, d, key,
                                        dleft, work, c_shadow, outcome, color, refl, no, nd, nkey);
      if (act) {
        StackEnt *gs = kernarg_late<true, offsetof(RenderArgs, dstack)>(a.dstack);
        if (outcome == kSpawned) {
          gs[RT_CK(kCkStack, qslot + (unsigned)lev * sstride, (long long)(a.depth - 1) * sstride)] =
              StackEnt{color.x, color.y, color.z, refl};
          ++lev;
          o = no;
          d = nd;
          key = nkey;
          --dleft;
          ++c_reflect;
        } else {
          D3 res = color;
          while (lev > 0) {  // main.cpp:54, innermost first
            --lev;
            const StackEnt e = gs[RT_CK(kCkStack, qslot + (unsigned)lev * sstride, (long long)(a.depth - 1) * sstride)];
            res = mk(e.ax + res.x * e.refl, e.ay + res.y * e.refl, e.az + res.z * e.refl);
          }
          const OutDesc &od = kernarg_late<true, offsetof(RenderArgs, od)>(a.od);
          const unsigned f = pixg / npx_frame;
          or_px(static_cast<uint8_t *>(od.ptr) + (size_t)RT_CK(kCkOut, f, a.frames) * (size_t)od.fstride, pixg - f * npx_frame,
                pack_px(res, c_neg));
          act = false;
        }
      }
    }
  }
  unsigned long long sums[4] = {0ull, wave_sum(c_shadow), wave_sum(c_reflect), wave_sum(c_neg)};
  flush_counts(kernarg_late<true, offsetof(RenderArgs, counters)>(a.counters), sums, work);
}

// render_deferred for scenes with a BVH, with the walks decoupled from the
// shading (kFast configuration).  A lane's closest-hit walk advances one node
// or leaf per step (walk4_step); a lane whose walk ended waits, and the wave
// shades once kShadeAt lanes are ready (or no lane is walking): shade_hit for
// the ready lanes only, after which a spawned reflection ray starts its walk
// and an ended chain stores its pixel and takes the next queued ray.  In
// render_deferred a wave's walk lasts as long as its longest one (the
// level >= 2 rays' walks are long-tailed: scripts/bvh_sim.cpp models 0.36 of
// the lanes busy); here the lanes whose walks end early start the next ray's.
// Same tests, same per-ray results: the closest hit of each ray is its
// lexicographic (t, index) minimum (walk4_step, closest_test), shading and
// the stack unwinding are render_deferred's.
#ifndef RT_SHADE_AT
#define RT_SHADE_AT 40
#endif
constexpr int kShadeAt = RT_SHADE_AT;
__global__ __launch_bounds__(64, RT_MIN_WAVES_PER_EU) void render_deferred_walk(const RenderArgs a) {
  const unsigned shard = blockIdx.x % kShards, first = blockIdx.x / kShards;
  const int cap = a.dq_cap;
  const unsigned long long cnt = a.counters[(size_t)shard * kShardStride + kDeferSlot];
  const unsigned n_dq = (unsigned)(cnt < (unsigned long long)cap ? cnt : (unsigned long long)cap);
  if (first * 64u >= n_dq) return;
  const int lane = (int)(threadIdx.x & 63);
  const unsigned npx_frame = (unsigned)((size_t)a.rows.count * a.od.xw);
  const unsigned sstride = (unsigned)kShards * (unsigned)cap;  // the chain's stack: dstack[level][queue slot]
  Work work;
  unsigned c_shadow = 0, c_reflect = 0, c_neg = 0;
  const unsigned long long lt = (1ull << lane) - 1ull;
  bool act = false, walking = false, more = true;
  unsigned long long *fetch = kernarg_late<true, offsetof(RenderArgs, counters)>(a.counters) +
                              (size_t)shard * kShardStride + kFetchSlot;  // as render_deferred
  D3 o = mk(0.0, 0.0, 0.0), d = o;
  int key = -1, dleft = 0, lev = 0;
  unsigned pixg = 0, qslot = 0;  // the ray's output pixel (launch index) and queue slot
  // the walk of this lane's ray: pending reference and stack depth, the best
  // hit so far (t, numerator, sphere) and the fp32 prune bound
  int ref = 0, sp = 0, bi = -1;
  double bt = kInf, bn = __builtin_inf();
  float tmf = 0.0f;
  auto prune = [&](const BvhArgs &bv) { return float_up(bt + 2e-6 * (bv.diam + __builtin_fabs(bt))); };
  auto begin = [&](const BvhArgs &bv) {  // a new ray: an empty best, the root box
    bt = kInf;
    bn = __builtin_inf();
    bi = -1;
    tmf = prune(bv);
    walking = walk4_begin(bv, walk4_ray(bv, o, d), tmf, ref, sp);
  };
  while (true) {
    {
      const unsigned long long idle = ~__ballot(act);
      if (idle && more) {
        const int fi = __builtin_ctzll(idle);
        unsigned long long base = 0;
        if (lane == fi) base = atomicAdd(fetch, (unsigned long long)__popcll(idle));
        base = __shfl(base, fi, 64);
        const unsigned long long i = base + (unsigned long long)__popcll(idle & lt);
        more = base + (unsigned long long)__popcll(idle) < n_dq;
        if (!act && i < n_dq) {
          const QRay &e = kernarg_late<true, offsetof(RenderArgs, dq)>(a.dq)[RT_CK(kCkDeferQ, (size_t)shard * (size_t)cap + i, (long long)kShards * cap)];
          o = mk(e.ox, e.oy, e.oz);
          d = mk(e.dx, e.dy, e.dz);
          lev = e.orig;
          dleft = e.dleft;
          key = e.key;
          pixg = (unsigned)e.pix;
          qslot = shard * (unsigned)cap + (unsigned)i;
          act = true;
          begin(kernarg_late<true, offsetof(RenderArgs, bv)>(a.bv));
        }
      }
    }
    if (__ballot(act) == 0) break;
    // walk until enough lanes are ready to shade (or no lane walks)
    if (__ballot(walking)) {
      const BvhArgs &bv = kernarg_late<true, offsetof(RenderArgs, bv)>(a.bv);
      const Walk4Ray r = walk4_ray(bv, o, d);
      const double a4 = 4.0 * dot(d, d), a2 = 0.5 * a4;
      const bool fast = a2_ok(a2);
      const SphGeo *__restrict__ g = a.geo;
      while (true) {
        const unsigned long long wm = __ballot(walking);
        if (wm == 0 || __popcll(__ballot(act) & ~wm) >= kShadeAt) break;
        if (walking) {
          auto leaf = [&](int i) {
            work.exact += 1;
            closest_test(g[RT_CK(kCkSphere, i, a.n)], i, o, d, a4, a2, fast, bt, bn, bi);
          };
          walking = walk4_step(bv, r, [&] { return prune(bv); }, work, leaf, ref, sp, tmf);
        }
      }
    }
    const bool ready = act && !walking;
    if (__ballot(ready)) {
      {
        // the line's part behind its origin (the walk skipped boxes wholly behind it)
        const BvhArgs &bv = kernarg_late<true, offsetof(RenderArgs, bv)>(a.bv);
        if (bv.ug.on && ready) {
          const double a4 = 4.0 * dot(d, d), a2 = 0.5 * a4;
          const bool fast = a2_ok(a2);
          const SphGeo *__restrict__ g = a.geo;
          behind_cells(bv, o, d, work, [&](int i) { closest_test(g[RT_CK(kCkSphere, i, a.n)], i, o, d, a4, a2, fast, bt, bn, bi); });
        }
      }
      int outcome = 0, nkey = 0;
      D3 color = mk(0.0, 0.0, 0.0), no = o, nd = d;
      double refl = 0.0;
      shade_hit<true, true, true, false, false>(a.geo, a.radius, a.mat, a.lights, a.n, a.nl, a.amb, a.bv, a.lg, ready, o, d, key,
                                   dleft, bi, bt, work, c_shadow, outcome, color, refl, no, nd, nkey);
      bool spawned = false;
      if (ready) {
        StackEnt *gs = kernarg_late<true, offsetof(RenderArgs, dstack)>(a.dstack);
        if (outcome == kSpawned) {
          gs[RT_CK(kCkStack, qslot + (unsigned)lev * sstride, (long long)(a.depth - 1) * sstride)] =
              StackEnt{color.x, color.y, color.z, refl};
          ++lev;
          o = no;
          d = nd;
          key = nkey;
          --dleft;
          ++c_reflect;
          spawned = true;
        } else {
          D3 res = color;
          while (lev > 0) {  // main.cpp:54, innermost first
            --lev;
            const StackEnt e = gs[RT_CK(kCkStack, qslot + (unsigned)lev * sstride, (long long)(a.depth - 1) * sstride)];
            res = mk(e.ax + res.x * e.refl, e.ay + res.y * e.refl, e.az + res.z * e.refl);
          }
          const OutDesc &od = kernarg_late<true, offsetof(RenderArgs, od)>(a.od);
          const unsigned f = pixg / npx_frame;
          or_px(static_cast<uint8_t *>(od.ptr) + (size_t)RT_CK(kCkOut, f, a.frames) * (size_t)od.fstride, pixg - f * npx_frame,
                pack_px(res, c_neg));
          act = false;
        }
      }
      if (spawned) begin(kernarg_late<true, offsetof(RenderArgs, bv)>(a.bv));
    }
  }
  unsigned long long sums[4] = {0ull, wave_sum(c_shadow), wave_sum(c_reflect), wave_sum(c_neg)};
  flush_counts(kernarg_late<true, offsetof(RenderArgs, counters)>(a.counters), sums, work);
}

// The build pass of a launch's ray table (RenderArgs::dirs): a wave per 8x8
// tile, a lane per pixel, with merge_tiles' own expressions for the pixel, its
// image row and its ray (camera.h:17-25, main.cpp:151-154), so the bits are
// the ones a tile pass would form; a padding lane (x >= W, a row past the
// launch's or the image's) holds what the inline code forms for it.
struct RayBuild {
  Cam cam;  // the orientation and scale (the position is not read)
  int W, H;
  Rows rows;
  int ntx, ntiles;
  double *out;  // [ntiles][kRayTileDoubles]
};
__global__ __launch_bounds__(256) void ray_table_kernel(const RayBuild b) {
  const int lane = (int)(threadIdx.x & 63);
  const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= b.ntiles) return;
  const int tx = (int)(tile % b.ntx), ty = (int)(tile / b.ntx);
  const Rows &rows = b.rows;
  const int W = b.W, H = b.H;
  const int x = tx * 8 + (lane & 7);
  const int k = ty * 8 + (lane >> 3);
  const bool in_tile = x < W && k < rows.count;
  const long long y = (long long)(k / rows.band) * rows.band * rows.stride +
                      (long long)rows.first * rows.band + (k % rows.band);
  const bool in_img = in_tile && y < H;
  const int j = H - 1 - (int)(in_img ? y : 0);
  const D3 dir = camera_dir(b.cam, (double)x, (double)j, W, H);
  const D3 d = renormalized(normalized(dir));
  double *tb = b.out + (size_t)tile * kRayTileDoubles;
  tb[lane] = d.x;
  tb[64 + lane] = d.y;
  tb[128 + lane] = d.z;
}

// Reassemble rank-major shards into PPM row order (one workgroup per row).
__global__ __launch_bounds__(kBlock) void unpermute_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                           int W, int H, int band, int G, int R) {
  const int y = blockIdx.x;
  if (y >= H) return;
  const int b = y / band;
  const int r = b % G;
  const int k = (b / G) * band + (y % band);
  const uint8_t *s = src + ((size_t)r * R + k) * (size_t)W * 3;
  uint8_t *d = dst + (size_t)y * W * 3;
  const int nb = W * 3;
  // 16-byte (else 4-byte) vector copies when both rows allow it (1080p: a row
  // is 360 x 16 B), bytes otherwise; the condition is uniform per row
  if (((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d) | (uintptr_t)nb) & 15) == 0) {
    const uint4 *s4 = reinterpret_cast<const uint4 *>(s);
    uint4 *d4 = reinterpret_cast<uint4 *>(d);
    for (int i = threadIdx.x; i < nb / 16; i += kBlock) d4[i] = s4[i];
  } else if (((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d) | (uintptr_t)nb) & 3) == 0) {
    const unsigned *s1 = reinterpret_cast<const unsigned *>(s);
    unsigned *d1 = reinterpret_cast<unsigned *>(d);
    for (int i = threadIdx.x; i < nb / 4; i += kBlock) d1[i] = s1[i];
  } else {
    for (int i = threadIdx.x; i < nb; i += kBlock) d[i] = s[i];
  }
}

}  // namespace rtk

using namespace rtk;

constexpr int kBvhAlwaysAbove = 1024;
constexpr size_t kUgMaxEntries = size_t(64) << 20;  // behind-grid list entries (20 B each)

// The one owner of an allocation: move-only, freed exactly once.  bytes() is
// the size asked for (a 0-byte request still allocates, so get() is never
// null after a successful alloc).
template <class T, class Alloc>
class OwnedBuf {
 public:
  OwnedBuf() = default;
  OwnedBuf(OwnedBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
  OwnedBuf &operator=(OwnedBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, bytes_ = o.bytes_;
      o.p_ = nullptr, o.bytes_ = 0;
    }
    return *this;
  }
  ~OwnedBuf() { reset(); }
  T *get() const { return p_; }
  size_t bytes() const { return bytes_; }
  void reset() {
    if (p_) Alloc::release(p_);
    p_ = nullptr;
    bytes_ = 0;
  }
  hipError_t alloc(size_t bytes) {
    reset();
    void *q = nullptr;
    const hipError_t e = Alloc::acquire(&q, bytes ? bytes : 1);
    if (e == hipSuccess) p_ = static_cast<T *>(q), bytes_ = bytes;
    return e;
  }

 private:
  T *p_ = nullptr;
  size_t bytes_ = 0;
};
struct DevAlloc {
  static hipError_t acquire(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void *p) { (void)hipFree(p); }
};
struct PinnedAlloc {
  static hipError_t acquire(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void release(void *p) { (void)hipHostFree(p); }
};
template <class T>
using PinnedBuf = OwnedBuf<T, PinnedAlloc>;
template <class T>
struct DevBuf : OwnedBuf<T, DevAlloc> {
  // room for v.size() + pad elements, the first v.size() of them copied from v
  hipError_t upload(const std::vector<T> &v, size_t pad = 0) {
    const hipError_t e = this->alloc(sizeof(T) * (v.size() + pad));
    if (e != hipSuccess || v.empty()) return e;
    return hipMemcpy(this->get(), v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
  }
};

// What rt_upload_scene builds and free_scene releases: the scene's device
// arrays with their sizes, and the flags saying which of them a launch may use.
struct Scene {
  bool has_scene = false;
  DevBuf<SphGeo> geo;
  DevBuf<double> rad;  // |radius|, for the conservative cull only
  DevBuf<SphMat> mat;
  DevBuf<LightD> lights;
  std::vector<LightD> lights_host;  // the uploaded records: what rt_set_light_samples shifts
  int nsph = 0, nlight = 0;
  double amb[3] = {0, 0, 0};
  double c0[3] = {0, 0, 0};
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // bounds of spheres and lights
  double rmax = 0;
  // the query region R of rt_trace_rays (lo..hi grown on every side by its own
  // diagonal) and R's diagonal: ray origins inside it keep the walks' margins sound
  double q_lo[3] = {0, 0, 0}, q_hi[3] = {0, 0, 0}, q_diam = 0;
  std::vector<SchedSphere> refl;  // reflective spheres of the scene (rt_sched.h)
  // BVH over the spheres (fallback for incoherent groups)
  DevBuf<BvhNode> bvh;
  DevBuf<int32_t> prims;
  DevBuf<float4> pf;
  DevBuf<BvhNode2> bvh2;
  DevBuf<BvhNode4> bvh4;  // 4-wide nodes for the ordered walk (RT_HIP_BVH4=0: two-child walk)
  int bvh2_root = -1, bvh_depth = 0, bvh4_root = -1, bvh4_stack = 0;
  int bvh_nodes = 0;
  int bvh2_nodes = 0, bvh4_nodes = 0, bvh_prims = 0;  // sizes the RT_CHECK build checks node / leaf indices against
  int bvh_leaf = 4;  // spheres per leaf it was built with (Knobs::bvh_leaf_opt, rt_upload_scene)
  // per-light direction grids for shadow rays (rt_lightgrid.h)
  DevBuf<int32_t> lg_start, lg_ids;
  long long lg_nstart = 0, lg_nids = 0;
  int lg_n = 128;  // their cells per cube-map face edge (Knobs::lg_n_opt, rt_upload_scene)
  double lg_max_off = 0.0;
  bool lg_off_free = false;  // shadow queries skip the per-ray max_off check (light_grids)
  // sphere grids (rt_lightgrid.h build_sphere_grids): the closest hit of
  // reflection rays in the kFast kernels, for the reflective spheres
  DevBuf<int32_t> sg_start;
  DevBuf<int2> sg_ent;  // (sphere, tlo bits)
  DevBuf<double> sg_rho2;
  int sg_n = 0, sg_grids = 0;
  long long sg_nstart = 0, sg_nent = 0;
  bool sg_ok = false;
  size_t sg_entries = 0;
  // RT_HIP_SPHERE_GRID auto: the grids are built by the scene's first launch
  // of more than one frame, or its second launch -- not by rt_upload_scene: a
  // one-image render (the drop-in ray_serial) spends ~1.8 ms building 143
  // grids (synth200) that save it ~0.05 ms of kernel time
  std::vector<rt_sphere> sg_src;  // the uploaded spheres, held only until sphere_grids has run
  double sg_diam = 0.0;
  bool sg_pending = false;
  long long launches = 0;  // render launches since the scene was uploaded
  // behind grid (rt_bvh.h build_ugrid): the backward half of the ordered
  // walks' closest-hit lines (rt_device.h behind_cells)
  DevBuf<int32_t> ug_rid, ug_ids, ug_glob;
  DevBuf<UgRec> ug_rec, ug_q;
  UgArgs ug{};  // its device arguments (on = 0 until a launch allows it)
  float ug_reg_margin = 0.0f, ug_extent = 0.0f;
  bool ug_ok = false;
  size_t ug_entries = 0;
};

// What rt_create reads from the environment (read_knobs), constant afterwards.
// The product build reads RT_HIP_LDS_SCENE and RT_HIP_CAM_GRID; the tuning build
// (-DRT_TUNING: variants/librt_hip_tuning.so) also the layout and grid knobs that the parity
// tests sweep and the A/B scripts measured.  Every default is the measured optimum.
struct Knobs {
  int bvh_ordered = 1;  // RT_HIP_BVH_ORDERED
  int bvh_wide = 1;     // RT_HIP_BVH4
  int lg_on = 1;        // RT_HIP_SHADOW_GRID
  int lg_n_opt = 0;     // RT_HIP_SHADOW_GRID_N; 0 = 128, or 768 above kBvhAlwaysAbove spheres
  int cg_mode = 1;    // RT_HIP_CAM_GRID: 0 off, 1 auto (a one-frame launch at a new position sweeps), 2 every launch
  int cg_n_opt = 0;   // RT_HIP_CAM_GRID_N (tuning build); 0 = kCgNStatic / kCgNMoving
  long long cg_budget_opt = -1;  // RT_HIP_CAM_GRID_BUDGET (tuning build): bytes for a launch's grids; -1 = kCgBudgetBytes
  long long cg_maxp_opt = -1;    // RT_HIP_CAM_GRID_MAXP (tuning build): pairs per grid kept; -1 = the pair budget
  // sphere grids (Scene::sg_*)
  int sg_mode = -1;  // RT_HIP_SPHERE_GRID: -1 auto (scenes of up to kSgMaxSpheres spheres), 0 off, 1 on
  int sg_n_opt = 0;  // RT_HIP_SPHERE_GRID_N; 0 = kSgN
  // behind grid (Scene::ug_*), built at upload
  int ug_mode = -1;  // RT_HIP_BEHIND_GRID: -1 auto (scenes above kBvhAlwaysAbove spheres), 0 off, 1 on
  // RT_HIP_GRID_CLOSEST: 1 (default) = with the grid, closest hits walk it along the whole line instead of the
  // BVH (rt_device.h grid_closest_line; synth10k 3.03 -> 2.93 ms per frame, profiles/r3u); 0 = the ordered BVH
  // walk ahead of the origin + behind_cells behind it (3.15 ms: the grid walk behind the origin costs more than
  // the BVH boxes it replaces)
  int ug_closest = 1;
  double ug_cells = 2.0;  // RT_HIP_GRID_CELLS: cells per listed sphere
  int bvh_min = 24, bvh_on = 1, bvh_groups = 2;  // RT_HIP_BVH_MIN, RT_HIP_BVH, RT_HIP_BVH_GROUPS
  // RT_HIP_BVH_LEAF; 0 = 2, or 1 above kBvhAlwaysAbove spheres (rt_upload_scene)
  int bvh_leaf_opt = 0;
  // RT_HIP_BVH_ALWAYS; -1 (auto): every group walks the BVH when the scene has
  // more than kBvhAlwaysAbove spheres (a linear cull sweep is O(n) per group)
  int bvh_always = -1;
  int stack_mode = 4;  // RT_HIP_STACK: 4 merged reflection levels (default), 1 per-pixel global stack (one tile per wave)
  // RT_HIP_DEFER: kStackMerge defers rays of level >= kDeferLevel to render_deferred
  // (-1, default: in multi-frame launches only; 0 never; 1 always).  A one-frame
  // launch ends on its slowest chains either way, and the second kernel's own
  // ramp and tail come after them (synth200 single frame 0.455 -> 0.384 ms
  // without it, profiles/r3n/ab_knobs.log; 32-frame launches are 13 % slower
  // per frame without it)
  int defer = -1;
  bool defer_walk = true;  // RT_HIP_DEFER_WALK: deferred rays of a scene whose closest hits always walk the BVH use render_deferred_walk
  int merge_q_max = 64;       // RT_HIP_MERGE_Q: longest LDS ray queue per wave tried (8, 16, 32 or 64; launch_render)
  int defer_level = kDeferLevel;  // RT_HIP_DEFER_LEVEL (>= 1)
  int defer_div = RT_DEFER_CAP_DIV;  // RT_HIP_DEFER_DIV (tuning build): queue room = launch pixels / defer_div
  // RT_HIP_LDS_SCENE=1: stage scenes that fit (<= kLdsBudget) in LDS, 4-wave
  // workgroups.  Off by default: one-wave workgroups reading the scene through
  // L2 free each wave's slot as soon as its own tile is done (synth200:
  // 0.473 -> 0.428 ms), which beats the LDS latency advantage.
  int lds_scene = 0;
  // Launch order of the tiles (rt_sched.h), rebuilt when the view or the
  // scene changes; RT_HIP_SCHED=0 dispatches in scanline order.
  int sched = 1;
  // kStackMerge: tiles of this class and above get a wave each (RT_HIP_SINGLE_CLASS
  // for every launch; kSchedClasses = none).  Default: every tile (class >= 0)
  // in one-frame launches, whose end is their slowest wave -- with no deferred
  // kernel after them (defer, above): synth200 0.780 -> 0.372 ms, complex
  // 0.652 -> 0.332 ms (profiles/r3r/ab_knobs.log); none in multi-frame
  // launches, where the other frames fill that tail and four tiles per wave
  // share their reflection rays' passes (class >= 1 there: 0.2285 -> 0.2364 ms
  // per frame, profiles/r3c/ab_single.log)
  int single_class = -1;
  // RT_HIP_TAIL: launches give their last tiles (the lightest, about one per
  // wave slot of the chip: tail_waves per CU over the frames) a wave each
  // (merge_end); 0: four per wave to the end.  RT_HIP_TAIL_WAVES (tuning build)
  int tail = 1;
  int tail_waves = 12;
  // RT_HIP_WIDE (tuning build): the render kernel whose sparse waves spread
  // their light loop over the lanes (shade_hit kWide).  3 (default): the
  // render and the deferred kernels of every fp64 launch; 2: the render kernel
  // only; 1: one-frame launches only; 0: the lane-per-ray loop (synth200 one
  // frame 0.297 -> 0.279 ms, 20 frames 0.1965 -> 0.1932 ms per frame; complex
  // 0.1797 -> 0.1755; profiles/r5o, profiles/r5p/ab_wide.log)
  int wide_mode = 3;
  // RT_HIP_XCD_FRAMES: multi-frame launches put every frame of a tile group on
  // one XCD (render_kernel).  -1 (default): for scenes with the uniform grid
  // (large scenes, whose lists and nodes outgrow an XCD's L2: synth10k 2.58 ->
  // 2.49 ms per frame); synth200 keeps the adjacent order (0.1943 vs 0.1958
  // ms per frame at 32 frames, equal at 20; profiles/r3u/ab_xcd_frames.log)
  int xcd_frames = -1;
};

static Knobs read_knobs() {
  Knobs k;
  if (const char *e = std::getenv("RT_HIP_LDS_SCENE")) k.lds_scene = std::atoi(e) != 0;
  if (const char *e = std::getenv("RT_HIP_CAM_GRID")) k.cg_mode = std::max(0, std::min(2, std::atoi(e)));
#ifdef RT_TUNING
  if (const char *e = std::getenv("RT_HIP_BVH")) k.bvh_on = std::atoi(e) != 0;
  if (const char *e = std::getenv("RT_HIP_BVH_MIN")) k.bvh_min = std::atoi(e);
  if (const char *e = std::getenv("RT_HIP_BVH_ALWAYS")) k.bvh_always = std::atoi(e) != 0;
  if (const char *e = std::getenv("RT_HIP_BVH_GROUPS")) k.bvh_groups = std::max(1, std::atoi(e));
  if (const char *e = std::getenv("RT_HIP_SHADOW_GRID")) k.lg_on = std::atoi(e) != 0;
  if (const char *e = std::getenv("RT_HIP_SCHED")) k.sched = std::atoi(e) != 0;
  if (const char *e = std::getenv("RT_HIP_STACK")) k.stack_mode = std::atoi(e) == kStackGlobal ? kStackGlobal : kStackMerge;
  if (const char *e = std::getenv("RT_HIP_BVH_ORDERED")) k.bvh_ordered = std::atoi(e) != 0;
  if (const char *e = std::getenv("RT_HIP_BVH4")) k.bvh_wide = std::atoi(e) != 0;
  if (const char *e = std::getenv("RT_HIP_BVH_LEAF")) k.bvh_leaf_opt = std::max(1, std::min(15, std::atoi(e)));
  if (const char *e = std::getenv("RT_HIP_DEFER")) k.defer = std::atoi(e) != 0 ? 1 : 0;
  if (const char *e = std::getenv("RT_HIP_DEFER_WALK")) k.defer_walk = std::atoi(e) != 0;
  if (const char *e = std::getenv("RT_HIP_DEFER_LEVEL")) k.defer_level = std::max(1, std::min(RT_MAX_DEPTH, std::atoi(e)));
  if (const char *e = std::getenv("RT_HIP_MERGE_Q")) k.merge_q_max = std::max(8, std::min(64, std::atoi(e)));
  if (const char *e = std::getenv("RT_HIP_SHADOW_GRID_N")) k.lg_n_opt = std::max(1, std::min(1024, std::atoi(e)));
  if (const char *e = std::getenv("RT_HIP_CAM_GRID_N")) k.cg_n_opt = std::max(1, std::min(1024, std::atoi(e)));
  if (const char *e = std::getenv("RT_HIP_CAM_GRID_BUDGET")) k.cg_budget_opt = std::max(0LL, std::atoll(e));
  if (const char *e = std::getenv("RT_HIP_CAM_GRID_MAXP")) k.cg_maxp_opt = std::max(1LL, std::atoll(e));
  if (const char *e = std::getenv("RT_HIP_SPHERE_GRID")) k.sg_mode = std::max(-1, std::min(1, std::atoi(e)));
  if (const char *e = std::getenv("RT_HIP_SPHERE_GRID_N")) k.sg_n_opt = std::max(1, std::min(256, std::atoi(e)));
  if (const char *e = std::getenv("RT_HIP_BEHIND_GRID")) k.ug_mode = std::max(-1, std::min(1, std::atoi(e)));
  if (const char *e = std::getenv("RT_HIP_GRID_CLOSEST")) k.ug_closest = std::atoi(e) != 0 ? 1 : 0;
  if (const char *e = std::getenv("RT_HIP_XCD_FRAMES")) k.xcd_frames = std::max(-1, std::min(1, std::atoi(e)));
  if (const char *e = std::getenv("RT_HIP_TAIL")) k.tail = std::atoi(e) != 0;
  if (const char *e = std::getenv("RT_HIP_TAIL_WAVES")) k.tail_waves = std::max(1, std::min(64, std::atoi(e)));
  if (const char *e = std::getenv("RT_HIP_WIDE")) k.wide_mode = std::max(0, std::min(3, std::atoi(e)));
  if (const char *e = std::getenv("RT_HIP_DEFER_DIV")) k.defer_div = std::max(1, std::min(1024, std::atoi(e)));
  if (const char *e = std::getenv("RT_HIP_GRID_CELLS")) k.ug_cells = std::max(0.05, std::min(64.0, std::atof(e)));
  if (const char *e = std::getenv("RT_HIP_SINGLE_CLASS"))
    k.single_class = std::max(0, std::min(kSchedClasses, std::atoi(e)));
#endif
  return k;
}

// Camera grids (rt_device.h CgArgs), built on the device per camera position
// of a launch (cg_bin_kernel / cg_sort_kernel) and kept while the positions
// and the scene stay the same.
struct CgTables {  // the cube map's patch tables of one N on the device: their owners and the kernels' view
  CubeTables view{};
  DevBuf<CubePatch> faces, blocks, tiles;
  DevBuf<double> cell;
};
struct CamGrids {
  DevBuf<int32_t> count;
  DevBuf<int2> ent, pairs;
  DevBuf<CgDisk> disks;
  DevBuf<unsigned> npairs;
  size_t bytes() const { return count.bytes() + ent.bytes() + disks.bytes() + pairs.bytes() + npairs.bytes(); }
  int n = 0, ngrid = 0;
  std::vector<double> pos;   // the grids' points (3 per grid)
  std::vector<double> seen;  // the previous launch's camera positions
  unsigned long long seen_gen = ~0ull;
  unsigned long long gen = ~0ull;  // scene_gen they were built for
  CgTables tab[2];
  int tab_next = 0;
};

// The ray table (RenderArgs::dirs, ray_table_kernel) and what it was built for; it does not depend on the
// scene, so an upload leaves it.
struct RayTable {
  DevBuf<double> buf;
  RayKey key{}, seen{};  // the table's key; the previous merged launch's key
  bool valid = false, seen_valid = false;
  // rt_set_ray_table: the policy's mode (rt_sched.h ray_table_policy: 0 never, 1 launches of two frames or
  // more, a kept table's key and a key's second one-frame launch, 2 every launch of one key) and the bytes a
  // table may take (-1: kRayBudgetBytes)
  int mode = 1;
  long long budget = -1;
  size_t bytes() const { return buf.bytes(); }
};

// The cached launch order of the tiles (tile_perm) and the view it was built for.
struct TileOrder {
  SchedView view{};
  unsigned long long gen = ~0ull;
  DevBuf<int> perm;
  PinnedBuf<int> h_perm;
  long long cls[kSchedClasses] = {};  // tiles per class of the cached order
};

// Counters: two halves of one allocation, alternating by launch; cur is the
// half of the latest launch (what rt_render_stats reads).  A render_kernel
// launch zeroes the other half for the next launch, so the default path needs
// no separate memset (a fill kernel per frame).
struct Counters {
  unsigned long long *cur = nullptr;  // into base
  DevBuf<unsigned long long> base;
  bool clean[2] = {true, true};
  PinnedBuf<unsigned long long> host;
};

// In-stream HIP events around every render launch (a ring), so a caller can
// time a whole region of launches and read the per-launch durations after.
struct LaunchTiming {
  static constexpr int kRing = 256;
  hipEvent_t ev0[kRing] = {}, ev1[kRing] = {};
  long long launches = 0, hist_begin = 0;
  int slot() const { return (int)(launches % kRing); }  // of the launch being enqueued
};

// The occupancy of the last kernel asked (blocks per CU at lds).
struct OccCache {
  const void *kernel = nullptr;
  size_t lds = 0;
  int blocks = 0;
};

// What rt_get_info reports of the builds made by uploads and render calls.
// None of it is reset by an upload: each figure is that of its latest build.
struct BuildInfo {
  bool cg_last = false, ug_last = false;  // the most recent launch used camera grids / the behind grid
  int cg_last_n = 0;
  unsigned long long cg_builds = 0, perm_builds = 0;
  double cg_build_ms = 0.0, perm_build_ms = 0.0, upload_ms = 0.0, sg_build_ms = 0.0, ug_build_ms = 0.0;
  double bvh_build_ms = 0.0, lg_build_ms = 0.0;  // rt_upload_scene's host builds
  // rt_get_ray_table_info: the ray table's builds, and whether the most recent launch read one
  bool rays_last = false;
  unsigned long long rays_builds = 0;
  double rays_build_ms = 0.0;
};

// The launch state of one family of caller-ray queries.  rt_ctx keeps one per
// family -- the ray queries (rt_trace_rays), the path queries (rt_trace_paths)
// and the radiance queries (rt_trace_radiance, rt_trace_radiance_resolve,
// rt_render_samples, rt_render_samples_async, rt_render_lens_samples[_async])
// -- and nothing of one is shared with another or with the
// renders: each has its own counters, its own most recent launch and its own
// staging.  Created by the family's first launch of a context (trace_state).
struct TraceState {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool launched = false;
  DevBuf<unsigned long long> ctr;      // [kShards][kShardStride], zeroed ahead of every launch
  PinnedBuf<unsigned long long> host;
  DevBuf<StackEnt> stack;              // radiance only, grow-only: [depth - 1][grid * 64] of the largest launch seen
  // the synchronous calls from host memory: the batch on the device, and what it
  // answers (hits; vertices and surfaces; colour records)
  DevBuf<uint8_t> rays, out[2];
  // radiance only: the light table of the resolving launches (rt_set_light_samples), [area_samples][nlight]
  // shifted copies of the scene's light records; area_samples == 0: no table.  Replaced or cleared only with
  // the stream idle (the setter, rt_upload_scene).
  DevBuf<LightD> area;
  int area_samples = 0;
  // radiance only: the gloss table of the resolving launches (rt_set_gloss_samples), [gloss_samples]
  // [gloss_bounces] points, and the scene's spheres' roughness; gloss_samples == 0: no table.  Replaced or
  // cleared as the light table is.
  DevBuf<D3> gloss;
  DevBuf<double> rough;
  int gloss_samples = 0, gloss_bounces = 0;
};

struct rt_ctx {
  explicit rt_ctx(int dev, const Knobs &k) : device(dev), knobs(k) {}
  const int device;
  int n_cu = 256;
  hipStream_t own_stream = nullptr, stream = nullptr;
  hipEvent_t switch_ev = nullptr;  // rt_set_stream: orders the new stream after the old one
  const Knobs knobs;
  // the caller's settings
  bool cull = true;  // rt_set_culling
  int samples = 1;   // 4: the antialias mode (rt_set_antialias)
  Scene scene;
  unsigned long long scene_gen = 0;  // counts the uploads: what the caches below were built for
  CamGrids cg;
  RayTable rays;
  TileOrder order;
  Counters ctr;
  LaunchTiming timing;
  OccCache occ;
  BuildInfo info;
  TraceState query, paths, radiance;
  // grow-only scratch of the launches
  DevBuf<uint8_t> tmp;      // rt_render to host memory: the image on the device
  DevBuf<QRay> dq;          // kStackMerge: the deferred queue (and its slots' stacks)
  // kStackMerge: the merged waves' stack homes (merge_tiles, home_acquire), twice as many
  // as the render kernel can have resident, and their bitmap (one bit per home)
  DevBuf<StackEnt> homes;
  DevBuf<unsigned long long> home_bits;
  DevBuf<int> bperm;        // rt_render_tiles: the launch-order buffer of the blocks covering the tiles
  PinnedBuf<int> h_bperm;
  DevBuf<StackEnt> gstack;  // kStackGlobal: the per-pixel reflection stack
  std::string err;
};

namespace {
double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int fail(rt_ctx *c, hipError_t e, const char *what) {
  if (c) c->err = std::string(what) + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP;
}

#define RT_TRY(ctx, call)                           \
  do {                                              \
    hipError_t e_ = (call);                         \
    if (e_ != hipSuccess) return fail(ctx, e_, #call); \
  } while (0)

// One render launch as its entry point asked for it; validate checks it and
// enqueue passes it down: nothing of a launch's arguments is kept in rt_ctx.
struct LaunchReq {
  const rt_camera *cams;  // nframes of them (more than one: rt_render_frames_async)
  int nframes;
  int W, H, depth;
  Rows rows;
  OutDesc od;
  const rt_tile *tiles = nullptr;  // rt_render_tiles: only the blocks covering these are rendered
  int ntiles = 0;
};

void free_scene(rt_ctx *c) {
  c->scene = Scene{};
  c->cg.gen = ~0ull;
}

// The diameter of the scene's bounds extended by the point p.
double extent_with(const Scene &sc, const double *p) {
  double d2 = 0.0;
  for (int k = 0; k < 3; k++) {
    const double l = std::min(sc.lo[k], p[k]), h = std::max(sc.hi[k], p[k]);
    d2 += (h - l) * (h - l);
  }
  return std::sqrt(d2);
}

// BVH arguments for rays whose origins lie within `diam` (a diameter of the
// scene's bounds extended by them); margin = 1e-6 * (diameter + largest
// radius).  behind_grid = false: the walks cover the whole line themselves.
BvhArgs bvh_args_within(const rt_ctx *c, double diam, bool behind_grid) {
  const Scene &sc = c->scene;
  BvhArgs b{};
  b.nodes = sc.bvh.get();
  b.prims = sc.prims.get();
  b.pf = sc.pf.get();
  b.n2 = sc.bvh2.get();
  b.root_ref = sc.bvh2_root;
  b.nnodes = (c->knobs.bvh_on && c->cull) ? sc.bvh_nodes : 0;
  b.nn2 = sc.bvh2_nodes;
  b.nn4 = sc.bvh4_nodes;
  b.nprims = sc.bvh_prims;
  b.n4 = sc.bvh4.get();
  b.root4 = sc.bvh4_root;
  b.wide = (c->knobs.bvh_wide && b.n4 && sc.bvh4_stack <= kOrderedStack) ? 1 : 0;
  b.ordered = (c->knobs.bvh_ordered && b.nnodes > 0 && (b.wide || (b.n2 && sc.bvh_depth <= kOrderedStack))) ? 1 : 0;
  if (!b.ordered) b.wide = 0;
  b.odepth = std::max(1, b.wide ? sc.bvh4_stack : sc.bvh_depth);
  b.ostk = nullptr;  // set in the kernel (LDS), or found at ostk_off
  b.ostk_off = -1;
  b.c0x = sc.c0[0], b.c0y = sc.c0[1], b.c0z = sc.c0[2];
  b.diam = diam;
  const double m = 1e-6 * (b.diam + sc.rmax);
  b.margin = std::isfinite(m) ? (float)(m * (1.0 + 1e-6)) : INFINITY;
  b.pmargin = 4.0f * b.margin;
  if (!std::isfinite(b.diam)) b.diam = INFINITY;
  b.min_cands = c->knobs.bvh_min;
  b.always = c->knobs.bvh_always >= 0 ? c->knobs.bvh_always : (sc.nsph > kBvhAlwaysAbove ? 1 : 0);
  b.max_groups = c->knobs.bvh_groups;
  // the behind grid, when its listing margin covers this view's prefilter
  // margin plus the DDA's error bound (rt_device.h behind_cells); the ordered
  // walks then skip boxes wholly behind the origin
  b.tf_min = -INFINITY;
  b.ug = UgArgs{};
  if (behind_grid && sc.ug_ok && b.nnodes > 0 && b.ordered && b.wide && std::isfinite(b.pmargin) &&
      (double)b.pmargin + 1e-4 * (double)sc.ug_extent <= (double)sc.ug_reg_margin) {
    b.ug = sc.ug;
    b.ug.on = 1;
    b.ug.closest = c->knobs.ug_closest;
    b.tf_min = 0.0f;
    // no closest hit walks the BVH then (the shadow queries use the light
    // grids or the stackless walk): no LDS stacks for the ordered walk, so
    // merge_tiles keeps its longest ray queue
    if (b.ug.closest) b.odepth = 0;
  }
  return b;
}

// BVH arguments for one render: the scene extent includes the camera (the
// origin of primary rays).
BvhArgs bvh_args(const rt_ctx *c, const Cam &cam) {
  const double cp[3] = {cam.px, cam.py, cam.pz};
  return bvh_args_within(c, extent_with(c->scene, cp) + 0.01, true);  // + the 0.001 origin offsets of secondary rays
}

// BVH arguments for a ray query: origins anywhere in the query region
// (Scene::q_lo..q_hi), no behind grid.
BvhArgs query_bvh_args(const rt_ctx *c) { return bvh_args_within(c, c->scene.q_diam + 0.01, false); }

LgArgs lg_args(const rt_ctx *c) {
  LgArgs g{};
  g.start = c->scene.lg_start.get(), g.ids = c->scene.lg_ids.get(), g.N = c->scene.lg_n;
  g.on = (c->knobs.lg_on && c->cull && g.start) ? 1 : 0;
  g.max_off = c->scene.lg_max_off, g.off_free = c->scene.lg_off_free ? 1 : 0;
  g.nstart = c->scene.lg_nstart, g.nids = c->scene.lg_nids;
  return g;
}

// camera grid cells per cube-map face edge (profiles/r4e/ab_camgrid_n.log,
// per frame of 32-frame launches at one position, synth200 / complex: 512
// 0.1914 / 0.1761 ms, 256 0.1914 / 0.1766, 128 0.1925 / 0.1770, 64 0.1950 /
// 0.1791, no grid 0.2177 / 0.1980): 256 for a launch at one position, 128 for
// a grid per frame (a quarter of the cells to build)
constexpr int kCgNStatic = 256, kCgNMoving = 128;

int upload_tables(rt_ctx *c, int N, CgTables &t);

// The device patch tables of the cube map with N cells per face edge (two
// kept; replacing one waits for the launches in flight).
int cg_tables(rt_ctx *c, int N, const CgTables *&out) {
  for (const auto &t : c->cg.tab)
    if (t.view.N == N) {
      out = &t;
      return RT_OK;
    }
  CgTables &t = c->cg.tab[c->cg.tab_next];
  c->cg.tab_next ^= 1;
  RT_TRY(c, hipStreamSynchronize(c->stream));
  t = CgTables{};
  const int rc = upload_tables(c, N, t);
  if (rc != RT_OK) return rc;
  out = &t;
  return RT_OK;
}

// The cube map's patch tables for N cells per face edge, on the device.
int upload_tables(rt_ctx *c, int N, CgTables &t) {
  std::vector<CubePatch> faces, blocks, tiles;
  std::vector<double> cell;
  int NT = 0, NB = 0;
  cube_tables(N, faces, blocks, tiles, cell, NT, NB);
  RT_TRY(c, t.faces.upload(faces));
  RT_TRY(c, t.blocks.upload(blocks));
  RT_TRY(c, t.tiles.upload(tiles));
  RT_TRY(c, t.cell.upload(cell));
  t.view = CubeTables{t.faces.get(), t.blocks.get(), t.tiles.get(), t.cell.get(), N, NT, NB};
  return RT_OK;
}

// grow-only buffer (device or pinned)
template <class B>
int grow(rt_ctx *c, B &b, size_t bytes) {
  if (b.bytes() >= bytes) return RT_OK;
  RT_TRY(c, hipStreamSynchronize(c->stream));  // launches in flight may read the old one
  b.reset();
  RT_TRY(c, b.alloc(bytes));
  return RT_OK;
}

// grow-only buffer that may fail softly: false (error cleared, buffer freed)
// when the memory is not there -- for optional structures
template <class B>
bool grow_soft(rt_ctx *c, B &b, size_t bytes) {
  if (b.bytes() >= bytes) return true;
  if (hipStreamSynchronize(c->stream) != hipSuccess) return false;
  b.reset();
  if (b.alloc(bytes) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}

// Camera-grid memory: the (disk, block) pair lists of one launch's grids take
// at most kCgPairBytes (a grid with more pairs is marked overflowed on the
// device and its rays sweep), and all of a launch's grid buffers at most
// kCgBudgetBytes and half the device's free memory -- the grid is a speed-up,
// so past that (or when an allocation fails) the launch sweeps (RT_OK).
constexpr size_t kCgPairBytes = size_t(128) << 20;
constexpr size_t kCgBudgetBytes = size_t(2) << 30;

// What cam_grid_prepare decided for a launch.
struct CgPlan {
  bool use = false;    // the launch scans grids
  bool build = false;  // ... built by cam_grid_enqueue first
  int N = 0, ngrid = 0, maxp = 0;
  long long nblocks = 0;
  std::vector<double> pos;
  const CgTables *tab = nullptr;
};

// The camera grids of this launch (plan.use = false: the launch sweeps as
// before): one grid when every frame shares the camera position, else one per
// frame; kept while the positions and the scene stay the same.  The host part
// -- policy, tables, buffers (which may wait for the stream) -- runs before
// the launch's start event; cam_grid_enqueue puts the device passes on the
// stream ahead of the render kernel.
int cam_grid_prepare(rt_ctx *c, const LaunchReq &q, CgPlan &p) {
  p = CgPlan{};
  const int nsph = c->scene.nsph, nf = q.nframes;
  if (c->knobs.cg_mode == 0 || !c->cull || nsph == 0) return RT_OK;
  std::vector<double> pos(q.cams[0].position, q.cams[0].position + 3);
  bool same = true;
  for (int f = 1; f < nf; f++) same = same && std::memcmp(q.cams[f].position, pos.data(), 3 * sizeof(double)) == 0;
  const int ngrid = same ? 1 : nf;
  for (int f = 1; f < ngrid; f++) pos.insert(pos.end(), q.cams[f].position, q.cams[f].position + 3);
  const int N = c->knobs.cg_n_opt ? c->knobs.cg_n_opt : (same ? kCgNStatic : kCgNMoving);
  const size_t cells = 6 * (size_t)N * N;
  if (ngrid * cells * kCgSlots >= (size_t(1) << 31)) return RT_OK;  // the scan's 32-bit slot index: no grid
  const bool cached = c->cg.gen == c->scene_gen && c->cg.n == N && c->cg.ngrid == ngrid && c->cg.pos == pos;
  if (!cached && nf == 1 && c->knobs.cg_mode == 1 && !(c->cg.seen_gen == c->scene_gen && c->cg.seen == pos)) {
    // one frame from a position the previous launch did not use: the build
    // (~0.05 ms) costs more than the grid saves that frame (profiles/r4j/);
    // the position's next launch gets the grid
    c->cg.seen = pos;
    c->cg.seen_gen = c->scene_gen;
    return RT_OK;
  }
  c->cg.seen = pos;
  c->cg.seen_gen = c->scene_gen;
  if (cached) {
    p.use = true;
    p.N = N;
    p.ngrid = ngrid;
    return RT_OK;
  }
  // from here the buffers change: the cached grids are gone whatever happens
  c->cg.gen = ~0ull;
  const CgTables *tab = nullptr;
  int rc = cg_tables(c, N, tab);
  if (rc != RT_OK) return rc;
  const long long nblocks = 6LL * tab->view.NB * tab->view.NB;
  // pairs per grid: every (disk, block) pair at most, within the pair budget
  // (a grid past it is marked overflowed on the device), and 4 work items per
  // pair of all grids countable in 32 bits (cg_bin_kernel)
  const unsigned long long worst = 2ull * (unsigned long long)nsph * (unsigned long long)nblocks;
  const unsigned long long cap32 = ((1ull << 32) - 1) / (4ull * (unsigned long long)ngrid);
  const unsigned long long budget = std::max<unsigned long long>(1, kCgPairBytes / sizeof(int2) / ngrid);
  int maxp = (int)std::min({worst, cap32, budget, (unsigned long long)INT32_MAX});
  if (c->knobs.cg_maxp_opt >= 0) maxp = (int)std::max<long long>(1, std::min<long long>(maxp, c->knobs.cg_maxp_opt));
  const size_t b_count = ngrid * cells * sizeof(int32_t), b_ent = ngrid * cells * kCgSlots * sizeof(int2),
               b_np = (size_t)ngrid * kCgCntStride * sizeof(unsigned),
               b_disks = 2 * (size_t)nsph * ngrid * sizeof(CgDisk), b_pairs = (size_t)ngrid * maxp * sizeof(int2);
  const size_t total = b_count + b_ent + b_np + b_disks + b_pairs;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void)hipGetLastError();
    free_b = 0;
  }
  // what the grids hold now counts as available: growing frees it first
  const size_t held = c->cg.bytes();
  const size_t limit = c->knobs.cg_budget_opt >= 0 ? (size_t)c->knobs.cg_budget_opt : kCgBudgetBytes;
  if (total > limit || total > (free_b + held) / 2) return RT_OK;
  if (!grow_soft(c, c->cg.count, b_count) || !grow_soft(c, c->cg.ent, b_ent) || !grow_soft(c, c->cg.npairs, b_np) ||
      !grow_soft(c, c->cg.disks, b_disks) || !grow_soft(c, c->cg.pairs, b_pairs))
    return RT_OK;  // no memory for the grid: this launch sweeps
  p.use = p.build = true;
  p.N = N;
  p.ngrid = ngrid;
  p.maxp = maxp;
  p.nblocks = nblocks;
  p.pos = std::move(pos);
  p.tab = tab;
  return RT_OK;
}

int cam_grid_enqueue(rt_ctx *c, const CgPlan &p, CgArgs &out) {
  out = CgArgs{};
  if (!p.use) return RT_OK;
  const size_t cells = 6 * (size_t)p.N * p.N;
  if (p.build) {
    const auto t0 = std::chrono::steady_clock::now();
    const int ngrid = p.ngrid;
    CgBuild b{};
    b.j = GridJob{c->scene.geo.get(), c->scene.rad.get(), p.tab->view, c->cg.disks.get(), c->cg.pairs.get(),
                  c->cg.npairs.get(), c->scene.nsph, ngrid, p.maxp};
    b.count = c->cg.count.get(), b.ent = c->cg.ent.get(), b.K = kCgSlots;
    for (int g = 0; g < ngrid; g++) {
      b.px[g] = p.pos[3 * g];
      b.py[g] = p.pos[3 * g + 1];
      b.pz[g] = p.pos[3 * g + 2];
      b.diam[g] = extent_with(c->scene, &p.pos[3 * (size_t)g]);  // (the grown radius' margin)
    }
    RT_TRY(c, hipMemsetAsync(b.count, 0, ngrid * cells * sizeof(int32_t), c->stream));
    RT_TRY(c, hipMemsetAsync(b.j.npairs, 0, ngrid * kCgCntStride * sizeof(unsigned), c->stream));
    const int nthr = b.j.n * ngrid;
    hipLaunchKernelGGL(cg_disk_kernel, dim3((unsigned)((nthr + 3) / 4)), dim3(256), 0, c->stream, b);
    hipLaunchKernelGGL(cg_bin_kernel, dim3((unsigned)std::min<long long>(8192, 8LL * nthr * p.nblocks)), dim3(64), 0,
                       c->stream, b);
    hipLaunchKernelGGL(cg_sort_kernel, dim3((unsigned)((ngrid * cells + 255) / 256)), dim3(256), 0, c->stream, b);
    RT_TRY(c, hipGetLastError());
    // the grids are valid for later launches only once their passes are on the stream
    c->cg.gen = c->scene_gen;
    c->cg.n = p.N;
    c->cg.ngrid = ngrid;
    c->cg.pos = p.pos;
    c->info.cg_builds++;
    c->info.cg_build_ms += ms_since(t0);
  }
  out = CgArgs{c->cg.count.get(), c->cg.ent.get(), p.N, 1, p.ngrid > 1 ? 1 : 0, p.ngrid};
  return RT_OK;
}

// The ray table of this launch (rt_sched.h ray_table_policy; plan.use = false: the launch forms its rays
// inline as before).  Like the camera grids: the host part -- policy and buffer, which may wait for the
// stream -- runs before the launch's start event, ray_table_enqueue puts the build pass on the stream ahead
// of the render kernel.  The table takes at most kRayBudgetBytes and half the device's free memory; past
// that, or when the allocation fails, the launch runs inline (RT_OK).
constexpr size_t kRayBudgetBytes = size_t(1) << 30;
struct RayPlan {
  bool use = false, build = false;
  RayKey key{};
  int ntx = 0;
  long long ntiles = 0;
};
Cam to_cam(const rt_camera &cm);
RayKey ray_key(const rt_camera &cm, const LaunchReq &q) {
  RayKey k{};
  std::memcpy(k.orient, cm.forward, 3 * sizeof(double));
  std::memcpy(k.orient + 3, cm.right, 3 * sizeof(double));
  std::memcpy(k.orient + 6, cm.up, 3 * sizeof(double));
  k.orient[9] = cm.scale;
  k.W = q.W, k.H = q.H;
  k.band = q.rows.band, k.first = q.rows.first, k.stride = q.rows.stride, k.count = q.rows.count;
  return k;
}
void ray_table_prepare(rt_ctx *c, const LaunchReq &q, int ntx, long long ntiles, RayPlan &p) {
  p = RayPlan{};
  RayTable &t = c->rays;
  const RayKey key = ray_key(q.cams[0], q);
  bool uniform = true;
  for (int f = 1; f < q.nframes; f++) uniform = uniform && ray_key_equal(ray_key(q.cams[f], q), key);
  const RayUse use = ray_table_policy(t.mode, uniform, q.nframes, key, t.valid ? &t.key : nullptr,
                                      t.seen_valid ? &t.seen : nullptr);
  t.seen = key;
  t.seen_valid = uniform;
  if (use == kRayInline) return;
  p.key = key, p.ntx = ntx, p.ntiles = ntiles;
  if (use == kRayReuse) {
    p.use = true;
    return;
  }
  const size_t total = (size_t)ntiles * kRayTileBytes;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void)hipGetLastError();
    free_b = 0;
  }
  const size_t limit = t.budget >= 0 ? (size_t)t.budget : kRayBudgetBytes;
  // what the table holds now counts as available: growing frees it first
  if (total > limit || total > (free_b + t.bytes()) / 2) return;
  t.valid = false;  // from here the buffer changes: the kept table is gone whatever happens
  if (!grow_soft(c, t.buf, total)) return;  // no memory for the table: this launch forms its rays inline
  p.use = p.build = true;
}

int ray_table_enqueue(rt_ctx *c, const LaunchReq &q, const RayPlan &p, RenderArgs &ra) {
  ra.dirs = nullptr;
  if (!p.use) return RT_OK;
  RayTable &t = c->rays;
  if (p.build) {
    const auto t0 = std::chrono::steady_clock::now();
    const RayBuild b{to_cam(q.cams[0]), q.W, q.H, q.rows, p.ntx, (int)p.ntiles, t.buf.get()};
    hipLaunchKernelGGL(ray_table_kernel, dim3((unsigned)((p.ntiles + 3) / 4)), dim3(256), 0, c->stream, b);
    RT_TRY(c, hipGetLastError());
    // valid for later launches only once its pass is on the stream
    t.key = p.key;
    t.valid = true;
    c->info.rays_builds++;
    c->info.rays_build_ms += ms_since(t0);
  }
  ra.dirs = t.buf.get();
  return RT_OK;
}

// sphere grid cells per cube-map face edge: 32 up to kSgFineSpheres spheres,
// else 16 (r3s: synth200 0.2031 / 0.2014 / 0.2003 ms per frame at 16 / 24 / 32,
// a 61 / 138 ms build at 16 / 32)
constexpr int kSgN = 16, kSgNFine = 32, kSgFineSpheres = 512;
constexpr int kSgMaxSpheres = 2048;     // RT_HIP_SPHERE_GRID=-1: larger scenes keep the BVH walks
constexpr int kSgMaxGlobal = 32;        // spheres overlapping an origin ball (on every list of its grid)
constexpr size_t kSgMaxEntries = size_t(256) << 20;  // 2 GiB of lists (built on the device)

// device scratch of one upload-time build, freed on every exit path
struct DevScratch {
  std::vector<DevBuf<unsigned char>> bufs;
  template <class T>
  hipError_t alloc(T *&out, size_t bytes) {
    bufs.emplace_back();
    const hipError_t e = bufs.back().alloc(bytes);
    out = reinterpret_cast<T *>(bufs.back().get());
    return e;
  }
};

// The exclusive prefix sum of x[0 .. n) into y[0 .. n] (y[n] = the total) on
// the stream; `total` the sum in 64 bits (y holds it only when below 2^31).
int device_scan(rt_ctx *c, const int *x, long long n, int *y, long long &total) {
  const long long nb = std::max(1LL, (n + kScanChunk - 1) / kScanChunk);
  DevScratch sc;
  long long *bsum = nullptr;
  RT_TRY(c, sc.alloc(bsum, sizeof(long long) * (size_t)(nb + 1)));
  hipLaunchKernelGGL(scan_chunk_sums, dim3((unsigned)nb), dim3(256), 0, c->stream, x, n, bsum);
  hipLaunchKernelGGL(scan_sums, dim3(1), dim3(64), 0, c->stream, bsum, (int)nb);
  hipLaunchKernelGGL(scan_apply, dim3((unsigned)nb), dim3(256), 0, c->stream, x, n, bsum, y);
  RT_TRY(c, hipGetLastError());
  RT_TRY(c, hipMemcpyAsync(&total, bsum + nb, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  RT_TRY(c, hipStreamSynchronize(c->stream));  // bsum is freed on return
  return RT_OK;
}

// Point grids on the device (pg_*_kernel passes) over the n spheres of
// scene.geo / scene.rad (uploaded; scene.nsph is set later) for the grids `pts`, each
// with N cells per cube-map face edge: per grid ok (sphere grids: refused past
// max_global global spheres or dropped pairs; light grids: never), the CSR
// offsets of the ng x row lists (device, ng * row + 1 ints, held by `keep`)
// and the entries (`out`: int2 (sphere, tlo) or, for light grids, int ids;
// empty when the lists would exceed max_entries).
struct PgMode {
  int sides, globlist, max_global;
  size_t max_entries;
  // light grids: lists by distance from the point (ids_sort_kernel; synth10k
  // 2.439 -> 2.386 ms per frame against sphere-index order, synth200 and
  // complex within +-0.3 %, profiles/r5x/ab_lg_order.log)
  int near = 0;
};
template <class E>  // the entries: int2 for sphere grids, int32_t for light grids (md.globlist)
int point_grids(rt_ctx *c, int n, const std::vector<GridPt> &pts, const std::vector<unsigned char> &allglob,
                double diam, int N, const PgMode &md, DevScratch &keep, int *&d_off, std::vector<unsigned char> &ok,
                long long &total, DevBuf<E> &out) {
  const int ng = (int)pts.size();
  const long long cells = 6LL * N * N, row = cells + (md.globlist ? 1 : 0);
  out.reset();
  total = 0;
  ok.assign((size_t)ng, 0);
  CgTables tab;
  int rc = upload_tables(c, N, tab);
  if (rc != RT_OK) return rc;
  const long long nblocks = 6LL * tab.view.NB * tab.view.NB;
  // pairs kept per grid (past it a sphere grid is refused, as one past the
  // host builder's entry cap; a light grid keeps every pair); grids in batches
  // whose disks and pairs fit kPgScratch
  constexpr size_t kPgScratch = size_t(128) << 20;
  const long long worst = (long long)md.sides * n * nblocks;
  const long long maxp = std::max(1LL, md.globlist ? worst : std::min<long long>(worst, 1 << 22));
  const size_t per_grid = 2 * (size_t)n * sizeof(CgDisk) + (size_t)maxp * sizeof(int2);
  const int batch = (int)std::max<long long>(
      1, std::min<long long>({(long long)ng, (long long)(kPgScratch / per_grid),
                              (long long)(((1ull << 32) - 1) / (4ull * (unsigned long long)maxp))}));
  if (4ull * (unsigned long long)maxp >= (1ull << 32)) return RT_OK;  // a grid's work items past 32 bits: none
  DevScratch sc;
  GridPt *d_pts = nullptr;
  unsigned char *d_ag = nullptr;
  int *d_cnt = nullptr;
  CgDisk *d_disks = nullptr;
  int2 *d_pairs = nullptr;
  unsigned *d_np = nullptr, *d_woff = nullptr;
  RT_TRY(c, sc.alloc(d_pts, sizeof(GridPt) * (size_t)ng));
  RT_TRY(c, sc.alloc(d_ag, (size_t)ng));
  RT_TRY(c, sc.alloc(d_cnt, sizeof(int) * (size_t)(ng * row)));
  RT_TRY(c, keep.alloc(d_off, sizeof(int) * (size_t)(ng * row + 1)));
  RT_TRY(c, sc.alloc(d_disks, 2 * (size_t)std::max(n, 1) * batch * sizeof(CgDisk)));
  RT_TRY(c, sc.alloc(d_pairs, (size_t)maxp * batch * sizeof(int2)));
  RT_TRY(c, sc.alloc(d_np, 2 * sizeof(unsigned) * kSgCntStride * (size_t)batch));
  RT_TRY(c, sc.alloc(d_woff, sizeof(unsigned) * (size_t)(batch + 1)));
  RT_TRY(c, hipMemcpy(d_pts, pts.data(), sizeof(GridPt) * (size_t)ng, hipMemcpyHostToDevice));
  RT_TRY(c, hipMemcpy(d_ag, allglob.data(), (size_t)ng, hipMemcpyHostToDevice));
  RT_TRY(c, hipMemsetAsync(d_cnt, 0, sizeof(int) * (size_t)(ng * row), c->stream));
  SgBuild b{};
  b.j = GridJob{c->scene.geo.get(), c->scene.rad.get(), tab.view, d_disks, d_pairs, d_np, n, 0, (int)maxp};
  b.nglob = d_np + kSgCntStride * (size_t)batch;
  b.woff = d_woff, b.off = d_off, b.row = (int)row;
  b.sides = md.sides, b.globlist = md.globlist, b.diam = diam;
  std::vector<std::vector<unsigned>> woffs;
  // one batch of grids: disks and pairs (pass 1) -- and, counting, the
  // grids' refusals and work offsets -- then the bin pass
  auto run_batch = [&](int g0, bool fill) -> int {
    const int nbg = std::min(batch, ng - g0);
    b.pts = d_pts + g0;
    b.allglob = d_ag + g0;
    b.j.ng = nbg;
    b.g0 = g0;
    b.cnt = d_cnt + (size_t)g0 * row;
    b.fill = fill ? 1 : 0;
    RT_TRY(c, hipMemsetAsync(d_np, 0, 2 * sizeof(unsigned) * kSgCntStride * (size_t)batch, c->stream));
    const long long waves = (long long)n * nbg;
    if (waves > 0) hipLaunchKernelGGL(pg_disk_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, c->stream, b);
    RT_TRY(c, hipGetLastError());
    if (!fill) {
      std::vector<unsigned> hn(2 * kSgCntStride * (size_t)batch);
      RT_TRY(c, hipMemcpyAsync(hn.data(), d_np, sizeof(unsigned) * hn.size(), hipMemcpyDeviceToHost, c->stream));
      RT_TRY(c, hipStreamSynchronize(c->stream));
      std::vector<unsigned> wo((size_t)nbg + 1, 0);
      for (int j = 0; j < nbg; j++) {
        const unsigned np = hn[(size_t)j * kSgCntStride], nglob = hn[((size_t)batch + j) * kSgCntStride];
        const bool g_ok = nglob <= (unsigned)md.max_global && np <= (unsigned)maxp;
        ok[(size_t)(g0 + j)] = g_ok ? 1 : 0;
        wo[(size_t)j + 1] = wo[(size_t)j] + (g_ok ? 4u * np : 0u);
      }
      woffs.push_back(wo);
    }
    const std::vector<unsigned> &wo = woffs[(size_t)(g0 / batch)];
    RT_TRY(c, hipMemcpyAsync(d_woff, wo.data(), sizeof(unsigned) * wo.size(), hipMemcpyHostToDevice, c->stream));
    const unsigned items = wo.back();
    if (items) {
      hipLaunchKernelGGL(pg_bin_kernel, dim3((unsigned)std::min<unsigned>(items, 16384u)), dim3(64), 0, c->stream, b);
      RT_TRY(c, hipGetLastError());
    }
    // the host copy of the work offsets is read by the stream: wait before the next batch rewrites them
    RT_TRY(c, hipStreamSynchronize(c->stream));
    return RT_OK;
  };
  for (int g0 = 0; g0 < ng; g0 += batch)
    if ((rc = run_batch(g0, false)) != RT_OK) return rc;
  if (md.globlist)  // a refused light grid's global list holds spheres too: keep it out of the counts
    for (int j = 0; j < ng; j++)
      if (!ok[(size_t)j]) return RT_OK;
  if ((rc = device_scan(c, d_cnt, (long long)ng * row, d_off, total)) != RT_OK) return rc;
  if ((size_t)total > md.max_entries || total > INT32_MAX) return RT_OK;
  RT_TRY(c, out.alloc(sizeof(E) * ((size_t)total + 1)));
  if constexpr (std::is_same<E, int2>::value)
    b.ent = out.get();
  else
    b.ids = out.get();
  b.nent = total;
  RT_TRY(c, hipMemsetAsync(d_cnt, 0, sizeof(int) * (size_t)(ng * row), c->stream));
  for (int g0 = 0; g0 < ng; g0 += batch)
    if ((rc = run_batch(g0, true)) != RT_OK) return rc;
  const long long nlists = (long long)ng * row;
  if (md.globlist)
    hipLaunchKernelGGL(ids_sort_kernel, dim3((unsigned)((nlists + 255) / 256)), dim3(256), 0, c->stream, d_off, nlists,
                       b.ids, b.j.geo, d_pts, row, md.near);
  else
    hipLaunchKernelGGL(sg_sort_kernel, dim3((unsigned)((nlists + 255) / 256)), dim3(256), 0, c->stream, d_off, nlists,
                       b.ent);
  RT_TRY(c, hipGetLastError());
  RT_TRY(c, hipStreamSynchronize(c->stream));  // the scratch is freed on return
  return RT_OK;
}

// Sphere grids for the reflective spheres of the scene being uploaded (the
// origins of reflection rays, main.cpp:46, lie within |r| + 0.001 of their
// sphere's centre up to the rounding of the hit point; the ball is grown by a
// relative 1e-6 and the device checks every ray against it), built on the
// device (point_grids; the geometry is on the device already).  No grids (and
// RT_OK) when disabled, too large, or refused.
int sphere_grids(rt_ctx *c) {
  Scene &scn = c->scene;
  std::vector<rt_sphere> src;  // the scene's copy of the spheres ends with this build
  src.swap(scn.sg_src);
  const int n = (int)src.size();
  const double diam = scn.sg_diam;
  scn.sg_pending = false;
  if (c->knobs.sg_mode == 0 || (c->knobs.sg_mode < 0 && n > kSgMaxSpheres) || n == 0 || !std::isfinite(diam)) return RT_OK;
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<double> rho((size_t)n, -1.0);
  std::vector<int> gidx((size_t)n, -1);
  std::vector<GridPt> pts;
  for (int i = 0; i < n; i++) {
    const rt_sphere &sp = src[(size_t)i];
    const double r = std::fabs(sp.radius);
    const double mag = std::fabs(sp.center[0]) + std::fabs(sp.center[1]) + std::fabs(sp.center[2]);
    if (sp.reflectivity > 0.0 && std::isfinite(r) && std::isfinite(mag))  // main.cpp:43
      rho[(size_t)i] = (r + kEps) * (1.0 + 1e-6) + 1e-12 * mag + 1e-9 * diam;
    if (rho[(size_t)i] >= 0.0 && std::isfinite(rho[(size_t)i])) {  // (build_sphere_grids: a finite ball)
      gidx[(size_t)i] = (int)pts.size();
      pts.push_back(GridPt{sp.center[0], sp.center[1], sp.center[2], rho[(size_t)i]});
    }
  }
  const int N = c->knobs.sg_n_opt ? c->knobs.sg_n_opt : (n <= kSgFineSpheres ? kSgNFine : kSgN);
  // the device indexes grid key's starts at key * (6 N^2 + 1) in 32 bits, and
  // every sphere has its row of starts: refuse grids that would overflow it
  // or hold more than 1 GiB of starts
  const long long cells = 6LL * N * N;
  const size_t nstart = (size_t)n * (size_t)(cells + 1);
  if (nstart > (size_t)INT32_MAX || nstart * sizeof(int32_t) > ((size_t)1 << 30)) return RT_OK;
  const int ng = (int)pts.size();
  scn.sg_grids = 0;
  scn.sg_entries = 0;
  if (ng == 0 || (long long)ng * cells >= INT32_MAX) {  // (32-bit CSR offsets)
    c->info.sg_build_ms = ms_since(t0);
    return RT_OK;
  }
  // built in buffers of this call, handed to the scene when complete: a
  // build that fails on the way leaves nothing behind
  DevScratch keep;
  int *d_off = nullptr;
  std::vector<unsigned char> ok;
  long long total = 0;
  DevBuf<int2> ent;
  DevBuf<int32_t> start;
  DevBuf<double> d_rho2;
  int rc = point_grids(c, n, pts, std::vector<unsigned char>((size_t)ng, 0), diam, N,
                       PgMode{2, 0, kSgMaxGlobal, kSgMaxEntries}, keep, d_off, ok, total, ent);
  if (rc != RT_OK) return rc;
  int grids = 0;
  for (int j = 0; j < ng; j++) grids += ok[(size_t)j];
  if (!ent.get() || grids == 0) {  // as build_sphere_grids past max_entries: no grids
    c->info.sg_build_ms = ms_since(t0);
    return RT_OK;
  }
  DevScratch sc;
  int *d_gidx = nullptr;
  unsigned char *d_ok = nullptr;
  RT_TRY(c, sc.alloc(d_gidx, sizeof(int) * (size_t)n));
  RT_TRY(c, sc.alloc(d_ok, (size_t)ng));
  RT_TRY(c, hipMemcpy(d_gidx, gidx.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
  RT_TRY(c, hipMemcpy(d_ok, ok.data(), (size_t)ng, hipMemcpyHostToDevice));
  RT_TRY(c, start.alloc(sizeof(int32_t) * nstart));
  hipLaunchKernelGGL(sg_start_kernel, dim3((unsigned)((nstart + 255) / 256)), dim3(256), 0, c->stream, d_gidx, d_ok,
                     d_off, n, cells, start.get());
  RT_TRY(c, hipGetLastError());
  std::vector<double> rho2((size_t)n);
  for (int i = 0; i < n; i++) {
    const int j = gidx[(size_t)i];
    rho2[(size_t)i] = (j >= 0 && ok[(size_t)j]) ? rho[(size_t)i] * rho[(size_t)i] : -1.0;
  }
  RT_TRY(c, d_rho2.upload(rho2));
  RT_TRY(c, hipStreamSynchronize(c->stream));  // the scratch is freed on return
  scn.sg_start = std::move(start);
  scn.sg_ent = std::move(ent);
  scn.sg_rho2 = std::move(d_rho2);
  scn.sg_n = N;
  scn.sg_nstart = (long long)nstart;
  scn.sg_nent = total;
  scn.sg_ok = true;
  scn.sg_grids = grids;
  scn.sg_entries = (size_t)total;
  c->info.sg_build_ms = ms_since(t0);
  return RT_OK;
}

// The host half of rt_upload_scene: what the scene's device arrays are copied
// from, built from the caller's scene without touching the device.
struct StagedScene {
  std::vector<SphGeo> geo;
  std::vector<double> rad;
  std::vector<SphMat> mat;
  std::vector<LightD> lights;
  // bounds of spheres and lights, their centre, the largest radius, the diameter
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, c0[3] = {0, 0, 0};
  double rmax = 0.0, diam = 0.0;
  std::vector<double> sx, sy, sz;      // sphere centres
  std::vector<double> bx, by, bz, br;  // ... relative to c0 (the BVH's frame), and the radii
  std::vector<BvhNode> nodes;
  std::vector<int32_t> prims;
  std::vector<float4> pf;  // prefilter records in leaf order (centre - c0 in fp32, |radius| rounded up)
  std::vector<BvhNode2> nodes2;
  std::vector<BvhNode4> nodes4;
  int32_t root2 = -1, root4 = -1;
  int depth2 = 0, stack4 = 0;
  bool ug_built = false;  // the behind grid, when asked for and within kUgMaxEntries
  UgridHost ug;
  std::vector<SchedSphere> refl;   // reflective spheres (rt_sched.h)
  double bvh_ms = 0.0, ug_ms = 0.0;  // the host time of the two builds
};

void stage_scene(const rt_scene *s, int bvh_leaf, bool want_ug, double ug_cells, StagedScene &st) {
  const int n = s->num_spheres, nl = s->num_lights;
  st.geo.resize(n), st.rad.resize(n), st.mat.resize(n), st.lights.resize(nl);
  for (int i = 0; i < n; i++) {
    const rt_sphere &sp = s->spheres[i];
    st.geo[i] = SphGeo{sp.center[0], sp.center[1], sp.center[2], sp.radius * sp.radius};
    st.rad[i] = sp.radius < 0 ? -sp.radius : sp.radius;
    st.mat[i] = SphMat{sp.color[0], sp.color[1], sp.color[2], sp.reflectivity, sp.shininess, 0.0};
    if (sp.reflectivity > 0.0)  // main.cpp:43
      st.refl.push_back(SchedSphere{sp.center[0], sp.center[1], sp.center[2], sp.radius});
  }
  for (int i = 0; i < nl; i++) {
    const rt_light &L = s->lights[i];
    st.lights[i] = LightD{L.position[0], L.position[1], L.position[2], L.color[0], L.color[1], L.color[2]};
  }
  auto extend = [&](const double *p, double r) {
    for (int k = 0; k < 3; k++) {
      st.lo[k] = std::min(st.lo[k], p[k] - r);
      st.hi[k] = std::max(st.hi[k], p[k] + r);
    }
  };
  for (int i = 0; i < n; i++) {
    const double r = std::fabs(s->spheres[i].radius);
    extend(s->spheres[i].center, r);
    if (r > st.rmax || r != r) st.rmax = r != r ? INFINITY : r;
  }
  for (int i = 0; i < nl; i++) extend(s->lights[i].position, 0.0);
  double d2 = 0.0;
  for (int k = 0; k < 3; k++) {
    if (n + nl > 0) st.c0[k] = std::isfinite(st.lo[k] + st.hi[k]) ? 0.5 * (st.lo[k] + st.hi[k]) : 0.0;
    d2 += (st.hi[k] - st.lo[k]) * (st.hi[k] - st.lo[k]);
  }
  st.diam = n + nl > 0 ? std::sqrt(d2) : 0.0;
  st.sx.resize(n), st.sy.resize(n), st.sz.resize(n);
  st.bx.resize(n), st.by.resize(n), st.bz.resize(n), st.br.resize(n);
  for (int i = 0; i < n; i++) {
    st.sx[i] = s->spheres[i].center[0];
    st.sy[i] = s->spheres[i].center[1];
    st.sz[i] = s->spheres[i].center[2];
    st.bx[i] = st.sx[i] - st.c0[0];
    st.by[i] = st.sy[i] - st.c0[1];
    st.bz[i] = st.sz[i] - st.c0[2];
    st.br[i] = s->spheres[i].radius;
  }
  const auto t_bvh = std::chrono::steady_clock::now();
  build_bvh(st.bx.data(), st.by.data(), st.bz.data(), st.br.data(), n, bvh_leaf, st.nodes, st.prims);
  st.pf.resize(st.prims.size());
  for (size_t k = 0; k < st.prims.size(); k++) {
    const int id = st.prims[k];
    float rr = (float)std::fabs(st.br[id]);
    if ((double)rr < std::fabs(st.br[id])) rr = std::nextafter(rr, INFINITY);
    st.pf[k] = make_float4((float)st.bx[id], (float)st.by[id], (float)st.bz[id], rr);
  }
  st.root2 = build_bvh2(st.nodes, st.nodes2, st.depth2);
  st.root4 = build_bvh4(st.nodes, st.nodes4, st.stack4);
  st.bvh_ms = ms_since(t_bvh);
  if (want_ug) {
    const auto t_ug = std::chrono::steady_clock::now();
    st.ug_built = build_ugrid(st.bx.data(), st.by.data(), st.bz.data(), st.br.data(), n, kUgMaxEntries, st.ug, ug_cells);
    st.ug_ms = ms_since(t_ug);
  }
}

// The per-light direction grids for shadow rays (rt_lightgrid.h
// build_light_grid's lists and layout), built on the device (point_grids,
// one side, global lists); the host builder when the device lists would not
// fit 32-bit offsets.
int light_grids(rt_ctx *c, const rt_scene *s, const StagedScene &st) {
  const auto t0 = std::chrono::steady_clock::now();
  const int n = s->num_spheres, nl = s->num_lights, N = c->scene.lg_n;
  const double diam = st.diam;
  Scene &scn = c->scene;
  const long long cells = 6LL * N * N;
  c->scene.lg_max_off = std::isfinite(diam) ? 1e-7 * diam : 0.0;
  {
    // every hit point lies on a finite sphere, inside the scene box up to
    // rounding, and every light inside it: with B the box's largest |coordinate|
    // the shadow lines' computed distance from their light stays below
    // 2^-41 (1.01 B + 0.01) (shadow_cells), so the per-ray check can go
    double B = 0.0;
    for (int k = 0; k < 3; k++) B = std::max(B, std::max(std::fabs(st.lo[k]), std::fabs(st.hi[k])));
    c->scene.lg_off_free = std::isfinite(B) && c->scene.lg_max_off > 0.0 && 0x1p-41 * (1.01 * B + 0.01) <= c->scene.lg_max_off;
  }
  const double dm = std::isfinite(diam) ? diam : 0.0;
  std::vector<GridPt> pts((size_t)nl);
  std::vector<unsigned char> allglob((size_t)nl);
  for (int l = 0; l < nl; l++) {
    const rt_light &L = s->lights[l];
    pts[(size_t)l] = GridPt{L.position[0], L.position[1], L.position[2], 0.0};
    allglob[(size_t)l] = !(std::isfinite(L.position[0]) && std::isfinite(L.position[1]) && std::isfinite(L.position[2]));
  }
  long long total = 0;
  bool dev = nl > 0 && (long long)nl * (cells + 2) < INT32_MAX;
  if (dev) {
    DevScratch keep;
    int *d_off = nullptr;
    std::vector<unsigned char> ok;
    int rc = point_grids(c, n, pts, allglob, dm, N, PgMode{1, 1, INT32_MAX, (size_t)INT32_MAX, 1}, keep, d_off, ok,
                         total, scn.lg_ids);
    if (rc != RT_OK) return rc;
    if (scn.lg_ids.get()) {
      const long long nstart = (long long)nl * (cells + 2);
      RT_TRY(c, scn.lg_start.alloc(sizeof(int32_t) * (size_t)(nstart + 1)));
      hipLaunchKernelGGL(lg_start_kernel, dim3((unsigned)((nstart + 255) / 256)), dim3(256), 0, c->stream, d_off, nl,
                         cells, scn.lg_start.get());
      RT_TRY(c, hipGetLastError());
      RT_TRY(c, hipStreamSynchronize(c->stream));  // d_off is freed on return
      scn.lg_nstart = nstart;
      scn.lg_nids = total;
    } else {
      dev = false;
    }
  }
  if (!dev) {  // no lights, or lists past 32 bits: the host builder
    std::vector<double> lx((size_t)nl), ly((size_t)nl), lz((size_t)nl);
    for (int l = 0; l < nl; l++) {
      lx[(size_t)l] = s->lights[l].position[0];
      ly[(size_t)l] = s->lights[l].position[1];
      lz[(size_t)l] = s->lights[l].position[2];
    }
    std::vector<int32_t> lg_start, lg_ids;
    build_light_grid(st.sx.data(), st.sy.data(), st.sz.data(), st.br.data(), n, lx.data(), ly.data(), lz.data(), nl,
                     diam, N, lg_start, lg_ids);
    scn.lg_nstart = (long long)lg_start.size();
    scn.lg_nids = (long long)lg_ids.size();
    RT_TRY(c, scn.lg_start.upload(lg_start, 1));
    RT_TRY(c, scn.lg_ids.upload(lg_ids, 1));
  }
  c->info.lg_build_ms = ms_since(t0);
  return RT_OK;
}

Cam to_cam(const rt_camera &cm) {
  return Cam{cm.position[0], cm.position[1], cm.position[2], cm.forward[0], cm.forward[1], cm.forward[2],
             cm.right[0],    cm.right[1],    cm.right[2],    cm.up[0],      cm.up[1],      cm.up[2],
             cm.scale};
}

// The tile launch order for this view (rt_sched.h), on the device; rebuilt
// only when the camera, the image/shard geometry, the tile size or the scene
// changed since the last build.
int tile_perm(rt_ctx *c, const LaunchReq &q, const Cam &cam, int tw, int th, long long ntiles, const int *&out) {
  const Rows &rows = q.rows;
  const OutDesc &od = q.od;
  SchedView v{};
  v.px = cam.px, v.py = cam.py, v.pz = cam.pz, v.fx = cam.fx, v.fy = cam.fy, v.fz = cam.fz;
  v.rx = cam.rx, v.ry = cam.ry, v.rz = cam.rz, v.ux = cam.ux, v.uy = cam.uy, v.uz = cam.uz, v.scale = cam.scale;
  v.W = q.W, v.H = q.H, v.band = rows.band, v.first = rows.first, v.stride = rows.stride, v.count = rows.count;
  v.x0 = od.x0, v.xw = od.xw, v.tw = tw, v.th = th;
  if (c->order.gen == c->scene_gen && std::memcmp(&v, &c->order.view, sizeof v) == 0 && c->order.perm.get()) {
    out = c->order.perm.get();
    return RT_OK;
  }
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<int> perm;
  long long cls[kSchedClasses] = {};
  tile_order(v, c->scene.refl, perm, cls);
  if ((long long)perm.size() != ntiles) return RT_ERR_INVALID_ARG;
  const size_t bytes = perm.size() * sizeof(int);
  RT_TRY(c, hipStreamSynchronize(c->stream));  // the previous order may still be in flight from h_perm
  if (c->order.perm.bytes() < bytes || c->order.h_perm.bytes() < bytes) {  // grow-only, the pair together
    c->order.gen = ~0ull;
    RT_TRY(c, c->order.perm.alloc(bytes));
    RT_TRY(c, c->order.h_perm.alloc(bytes));
  }
  std::memcpy(c->order.h_perm.get(), perm.data(), bytes);
  RT_TRY(c, hipMemcpyAsync(c->order.perm.get(), c->order.h_perm.get(), bytes, hipMemcpyHostToDevice, c->stream));
  c->order.view = v;
  c->order.gen = c->scene_gen;
  for (int k = 0; k < kSchedClasses; k++) c->order.cls[k] = cls[k];
  out = c->order.perm.get();
  c->info.perm_builds++;
  c->info.perm_build_ms += ms_since(t0);
  return RT_OK;
}

// (Re-)records the launch's start event just before its first kernel: the
// host-side builds a launch may make first (tile order, camera grid) are not
// kernel time.  enqueue() has recorded it already for launches with no kernel.
hipError_t mark_start(rt_ctx *c) { return hipEventRecord(c->timing.ev0[c->timing.slot()], c->stream); }

// Which render kernel a launch runs: the scene staged in LDS or read through
// L2, the cull sweeps, 1 or 4 samples, kStackGlobal or kStackMerge; fast /
// wide (kStackMerge only) are launch_tiles' to set.
struct KernelSel {
  bool lds, cull;
  int samples, stack;
  bool fast = false, wide = false;
  int merge_q = 64;  // kStackMerge: the LDS ray-queue entries per wave launch_render picked (no other kernel reads it)
};

// The two tables of kernel instantiations: every render and deferred kernel
// of the build is named here and nowhere else.
const void *render_kernel_fn(const KernelSel &s) {
#define RT_RK(...) reinterpret_cast<const void *>(&render_kernel<__VA_ARGS__>)
  if (s.stack == kStackMerge) {  // the scene through L2, one sample
    if (s.cull)
      return s.wide   ? RT_RK(false, true, 1, kStackMerge, true, true)
             : s.fast ? RT_RK(false, true, 1, kStackMerge, true)
                      : RT_RK(false, true, 1, kStackMerge);
    return s.wide   ? RT_RK(false, false, 1, kStackMerge, true, true)
           : s.fast ? RT_RK(false, false, 1, kStackMerge, true)
                    : RT_RK(false, false, 1, kStackMerge);
  }
  static const void *const kGlobal[2][2][2] = {  // [lds][cull][samples == 4]
      {{RT_RK(false, false, 1, kStackGlobal), RT_RK(false, false, 4, kStackGlobal)},
       {RT_RK(false, true, 1, kStackGlobal), RT_RK(false, true, 4, kStackGlobal)}},
      {{RT_RK(true, false, 1, kStackGlobal), RT_RK(true, false, 4, kStackGlobal)},
       {RT_RK(true, true, 1, kStackGlobal), RT_RK(true, true, 4, kStackGlobal)}}};
  return kGlobal[s.lds][s.cull][s.samples == 4];
#undef RT_RK
}

// walk: render_deferred_walk; else render_deferred, with the light loop
// spread over the lanes (wide) or the fast paths only (s.fast)
const void *deferred_kernel_fn(const KernelSel &s, bool walk, bool wide) {
#define RT_RD(...) reinterpret_cast<const void *>(&render_deferred<__VA_ARGS__>)
  if (walk) return reinterpret_cast<const void *>(&render_deferred_walk);
  if (s.cull) return wide ? RT_RD(true, true, true) : s.fast ? RT_RD(true, true) : RT_RD(true);
  return wide ? RT_RD(false, true, true) : s.fast ? RT_RD(false, true) : RT_RD(false);
#undef RT_RD
}

int wg_waves_of(bool lds_geo) { return lds_geo ? wg_waves<true>() : wg_waves<false>(); }

// The dynamic LDS of a render launch as render_kernel lays it out from the
// same arguments: the staged scene (lds_layout), the ordered walk's stacks at
// ostk_off, then at pix_off the parked colours (trace_wave) or, for merged
// levels, the wave's ray queue of merge_q entries and finished pixels
// (merge_tiles).
struct LdsPlan {
  size_t scene_end, ostk_off, pix_off, total;
};
LdsPlan lds_plan(const Scene &scn, const BvhArgs &bv, bool lds_geo, bool merge, int merge_q) {
  const size_t wg = (size_t)wg_waves_of(lds_geo);
  LdsPlan p;
  p.scene_end = lds_layout(lds_geo, scn.nsph, scn.nlight, bv.nnodes).end;
  p.ostk_off = (p.scene_end + 31) & ~(size_t)31;
  p.pix_off = p.ostk_off + (bv.ordered ? wg * bv.odepth * 64 * sizeof(int2) : 0);
  p.total = p.pix_off;
  if (!lds_geo && !merge) p.total += wg * 64 * sizeof(D3);
  if (merge) p.total += (size_t)merge_q * sizeof(QRay) + kPixbufBytes;
  return p;
}

// rt_render_tiles: the blocks (launch tiles of bw x bh pixels, ntx per row)
// that overlap a requested tile, in scanline order of the blocks, copied to
// the device (`out`); n of them, 0: nothing to launch.
int block_list(rt_ctx *c, const LaunchReq &q, int bw, int bh, int ntx, long long ntiles, const int *&out,
               long long &n) {
  std::vector<unsigned char> mark((size_t)ntiles, 0);
  for (int i = 0; i < q.ntiles; i++) {
    const rt_tile &t = q.tiles[i];
    // in 64 bits: a caller's x + width near INT_MAX must still clip to the image
    const int x1 = (int)std::min<long long>(q.W, (long long)t.x + t.width);
    const int j1 = (int)std::min<long long>(q.H, (long long)t.y + t.height);
    if (t.x >= x1 || t.y >= j1) continue;
    // framebuffer rows j (0 = bottom) are PPM rows H-1-j
    const int y0 = q.H - j1, y1 = q.H - 1 - t.y;
    for (int by = y0 / bh; by <= y1 / bh; by++)
      for (int bx = t.x / bw; bx <= (x1 - 1) / bw; bx++) mark[(size_t)by * ntx + bx] = 1;
  }
  std::vector<int> list;
  for (long long b = 0; b < ntiles; b++)
    if (mark[(size_t)b]) list.push_back((int)b);
  n = (long long)list.size();
  if (n == 0) return RT_OK;
  const size_t bytes = list.size() * sizeof(int);
  RT_TRY(c, hipStreamSynchronize(c->stream));  // the previous list may still be in flight from h_bperm
  if (c->bperm.bytes() < bytes || c->h_bperm.bytes() < bytes) {  // grow-only, the pair together
    RT_TRY(c, c->bperm.alloc(bytes));
    RT_TRY(c, c->h_bperm.alloc(bytes));
  }
  std::memcpy(c->h_bperm.get(), list.data(), bytes);
  RT_TRY(c, hipMemcpyAsync(c->bperm.get(), c->h_bperm.get(), bytes, hipMemcpyHostToDevice, c->stream));
  out = c->bperm.get();
  return RT_OK;
}

// How a launch's tiles go to wave slots: `perm` their order (nullptr:
// scanline), the first nsingle a wave each, the last `tail` too, the rest
// kMergeTiles per wave; nslots wave slots per frame.
struct SlotPlan {
  const int *perm = nullptr;
  int nsingle = 0;
  long long tail = 0, nslots = 0;
};

// kStackMerge with a tile order of `cls` tiles per class, the heaviest classes
// leading it: one wave per tile for them.
SlotPlan slot_plan(const long long *cls, long long ntiles, int nf, const Knobs &k, int n_cu) {
  SlotPlan s;
  // one-frame launches: the tiles under reflective spheres (class >= 1) a
  // wave each, the rest four per wave, the last ones (tail) single again
  // (synth200 0.314 -> 0.298 ms, complex 0.293 -> 0.286 against every tile
  // single, profiles/r5g/); multi-frame launches merge every class
  const int sc = k.single_class >= 0 ? k.single_class : (nf == 1 ? 1 : kSchedClasses);
  long long heavy = 0;
  for (int i = sc; i < kSchedClasses; i++) heavy += cls[i];
  s.nsingle = (int)std::min<long long>(heavy, ntiles);
  // multi-frame launches end on their lightest tiles one per wave: about
  // as many as the chip holds waves (12 per CU), over the launch's frames
  if (k.tail) s.tail = std::min<long long>(ntiles - s.nsingle, ((long long)n_cu * k.tail_waves + nf - 1) / nf);
  s.nslots = s.nsingle + (ntiles - s.nsingle - s.tail + kMergeTiles - 1) / kMergeTiles + s.tail;
  return s;
}

// kStackMerge: the deferred queue of a launch that defers (ra.dq, dq_cap,
// dstack; none otherwise).
void defer_room(rt_ctx *c, const LaunchReq &q, RenderArgs &ra) {
  const int nf = q.nframes, depth = q.depth;
  if (!(c->knobs.defer > 0 || (c->knobs.defer < 0 && nf > 1)) || depth <= c->knobs.defer_level) return;
  // room for 1/8 of the launch's pixels (deferred rays are ~2 % on synth200); a ray
  // that finds its shard segment full simply continues in its merge_tiles lane.
  // Each queue slot has its chain's stack after the queue: [depth-1][kShards * cap]
  const size_t npx = (size_t)q.rows.count * q.od.xw * nf;
  const size_t cap = std::max<size_t>(64, ((npx / kShards / (size_t)c->knobs.defer_div) + 63) & ~(size_t)63);
  const size_t need = cap * kShards * (sizeof(QRay) + (size_t)(depth - 1) * sizeof(StackEnt));
  // the queue is a speed-up: past the 32-bit slot-stack index, or when the
  // memory is not there (grow_soft), the launch runs without deferral
  if (cap < (size_t)1 << 30 && (unsigned long long)cap * kShards * (unsigned)(depth - 1) < (1ull << 32) &&
      grow_soft(c, c->dq, need)) {
    ra.dq = c->dq.get();
    ra.dq_cap = (int)cap;
    ra.dstack = reinterpret_cast<StackEnt *>(c->dq.get() + cap * kShards);
  }
}

// kStackMerge: the stack homes (ra.homes, home_bits, home_words), 2 x the
// resident waves of render kernel kf with `lds` bytes of LDS per workgroup of wg waves.
int stack_homes(rt_ctx *c, const void *kf, int wg, size_t lds, int depth, RenderArgs &ra) {
  if (kf != c->occ.kernel || lds != c->occ.lds) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kf, 64 * wg, lds) != hipSuccess || nb < 1) {
      (void)hipGetLastError();
      nb = 32;  // the most waves a CU holds
    }
    c->occ = OccCache{kf, lds, nb};
  }
  const size_t words = (size_t)(((long long)2 * c->occ.blocks * wg * c->n_cu + 63) / 64);
  const size_t hb = words * 64 * (size_t)(depth - 1) * kHomePx * sizeof(StackEnt);
  const size_t wb = words * sizeof(unsigned long long);
  if (c->homes.bytes() < hb || c->home_bits.bytes() < wb) {
    RT_TRY(c, hipStreamSynchronize(c->stream));  // launches in flight hold homes
    c->homes.reset(), c->home_bits.reset();      // both go, whichever was too small
    RT_TRY(c, c->homes.alloc(hb));
    RT_TRY(c, c->home_bits.alloc(wb));
    // zero once: every wave returns the home it took, so a drained launch leaves the bitmap zero
    RT_TRY(c, hipMemset(c->home_bits.get(), 0, wb));
  }
  ra.homes = c->homes.get();
  ra.home_bits = c->home_bits.get();
  ra.home_words = (int)(c->home_bits.bytes() / sizeof(unsigned long long));
  return RT_OK;
}

// The kernels' argument block of a launch, but for what launch_tiles adds
// when it has it: the deferred queue, the stack homes, the camera and sphere grids.
RenderArgs render_args(const rt_ctx *c, const LaunchReq &q, const Cam &cam, const KernelSel &sel, const BvhArgs &bv,
                       const LdsPlan &lp, int ntx, long long ntiles, const SlotPlan &sp, StackEnt *gstack) {
  const Scene &scn = c->scene;
  const int nf = q.nframes;
  RenderArgs ra{};
  ra.geo = scn.geo.get(), ra.radius = scn.rad.get(), ra.mat = scn.mat.get(), ra.lights = scn.lights.get();
  ra.n = scn.nsph, ra.nl = scn.nlight;
  ra.amb = D3{scn.amb[0], scn.amb[1], scn.amb[2]};
  ra.cam[0] = cam;
  for (int f = 1; f < nf; f++) ra.cam[f] = to_cam(q.cams[f]);
  ra.frames = nf;
  ra.W = q.W, ra.H = q.H, ra.depth = q.depth, ra.rows = q.rows, ra.od = q.od;
  ra.bv = bv;
  ra.lg = lg_args(c);
  ra.gstack = gstack;
  ra.counters = c->ctr.cur;
  ra.ntx = ntx, ra.ntiles = (int)ntiles, ra.nslots = (int)sp.nslots, ra.perm = sp.perm;
  // zero the other counter half for the next launch (enqueue's alternation)
  const int next = (int)((c->timing.launches + 1) & 1);
  ra.zero_next = c->ctr.base.get() + (size_t)next * kShards * kShardStride;
  ra.merge_q = sel.merge_q, ra.nsingle = sp.nsingle, ra.merge_end = (int)(ntiles - sp.tail);
  // merge_tiles' pixel bytes: after the scene and the walk stacks, where render_kernel's park/queue region starts
  ra.pix_off = (int)lp.pix_off;
  // row k of frame f starts at ptr + f fstride + 3 (k W + x): dword aligned for every k, f and x = 8i
  ra.rows_dword =
      ((reinterpret_cast<uintptr_t>(q.od.ptr) | (uintptr_t)(3 * (size_t)q.W) | (uintptr_t)q.od.fstride) & 3) == 0;
  ra.defer_level = c->knobs.defer_level;
  ra.xcd_frames = (nf > 1 && (c->knobs.xcd_frames > 0 || (c->knobs.xcd_frames < 0 && bv.ug.on))) ? 1 : 0;
  return ra;
}

// What a launch put on the stream, for enqueue's bookkeeping: a render kernel (it zeroes
// the other counter half), whether it used camera grids (of cg_n cells) / the behind grid.
struct Launched {
  bool kernel = false, cg = false, ug = false, rays = false;
  int cg_n = 0;
};

int launch_tiles(rt_ctx *c, const LaunchReq &q, KernelSel sel, const Cam &cam, BvhArgs bv, Launched &did) {
  Scene &scn = c->scene;
  const int nf = q.nframes, depth = q.depth;
  const bool merge = sel.stack == kStackMerge;
  const int kWg = wg_waves_of(sel.lds), kWx = kWg == 4 ? 2 : 1, kWy = kWg / kWx;
  const LdsPlan lp = lds_plan(scn, bv, sel.lds, merge, sel.merge_q);
  // the ordered walk's stacks follow the scene in LDS (render_kernel)
  if (bv.ordered) bv.ostk_off = (int)lp.ostk_off;
  const int ntx = (q.od.xw + 8 * kWx - 1) / (8 * kWx), nty = (q.rows.count + 8 * kWy - 1) / (8 * kWy);
  const long long ntiles = (long long)ntx * nty;
  if (ntiles * nf > (1LL << 30)) return RT_ERR_INVALID_ARG;
  int rc = RT_OK;
  SlotPlan sp;
  // kStackMerge: one wave per kMergeTiles consecutive tile slots
  sp.nslots = merge ? (ntiles + kMergeTiles - 1) / kMergeTiles : ntiles;
  if (!merge && q.tiles)
    if ((rc = block_list(c, q, 8 * kWx, 8 * kWy, ntx, ntiles, sp.perm, sp.nslots)) != RT_OK || sp.nslots == 0) return rc;
  StackEnt *gstack = nullptr;
  if (depth > 1 && !merge) {
    // the kernel indexes the stack with 32 bits: entry + level * npx < 2^32
    if ((unsigned long long)(depth - 1) * q.rows.count * q.od.xw * nf >= (1ull << 32)) return RT_ERR_INVALID_ARG;
    // grow-only: sized for this launch's frames; a later launch of as many
    // frames or fewer (a last partial batch) reuses it
    if ((rc = grow(c, c->gstack, (size_t)(depth - 1) * q.rows.count * q.od.xw * nf * sizeof(StackEnt))) != RT_OK) return rc;
    gstack = c->gstack.get();
  }
  // The heavy-first order pays off when a launch has many more tiles than the
  // chip has wave slots; a small launch (a hybrid driver's 64x64 tile) keeps
  // scanline order and skips building and uploading one (which waits for the
  // stream whenever the tile shape changes).
  if (!sp.perm && c->knobs.sched && ntiles >= kSchedMinTiles) {
    const int *perm = nullptr;
    if ((rc = tile_perm(c, q, cam, 8 * kWx, 8 * kWy, ntiles, perm)) != RT_OK) return rc;
    if (merge) sp = slot_plan(c->order.cls, ntiles, nf, c->knobs, c->n_cu);
    sp.perm = perm;
  }
  RenderArgs ra = render_args(c, q, cam, sel, bv, lp, ntx, ntiles, sp, gstack);
  const dim3 grid((unsigned)((ra.xcd_frames ? (sp.nslots + 7) / 8 * 8 : sp.nslots) * nf));
  if (merge) defer_room(c, q, ra);
  // the default configuration (ordered 4-wide BVH walk, light grids) has kernels
  // compiled with only those paths (kFast): no registers held for the others
  sel.fast = merge && bv.ordered && bv.wide && ra.lg.on;
  // the light loop of sparse waves spread over the lanes (shade_hit kWide, the default)
  sel.wide = sel.fast && (c->knobs.wide_mode >= 2 || (nf == 1 && c->knobs.wide_mode == 1));
  const void *const kf = render_kernel_fn(sel);
  const size_t lds = lp.total;
  if (merge && depth > 1 && (rc = stack_homes(c, kf, kWg, lds, depth, ra)) != RT_OK) return rc;
  // the sphere grids, lazily (sg_pending): the scene's first multi-frame
  // launch or its second launch builds them, before the launch's timing
  // (a speed-up: if its build fails the launch runs without the grids)
  if (sel.fast && sel.cull && scn.sg_pending && (nf > 1 || scn.launches > 0)) {
    // an error of the launches in flight is theirs, not a failed build
    RT_TRY(c, hipStreamSynchronize(c->stream));
    if (sphere_grids(c) != RT_OK) {
      (void)hipGetLastError();
      c->err.clear();
      scn.sg_ok = false;  // (nothing half-built to release: sphere_grids hands its buffers over only when complete)
    }
  }
  // the camera grids' host part (policy, tables, buffers) first; the
  // launch's timing starts after it: the grids' device passes ahead of the
  // render kernel are part of the launch
  CgPlan plan;
  if (sel.fast && sel.cull && (rc = cam_grid_prepare(c, q, plan)) != RT_OK) return rc;
  // the ray table's host part likewise (merged launches of whole images; rt_render_tiles keeps its inline rays)
  RayPlan rays;
  if (merge && !q.tiles) ray_table_prepare(c, q, ntx, ntiles, rays);
  RT_TRY(c, mark_start(c));
  if ((rc = cam_grid_enqueue(c, plan, ra.cg)) != RT_OK) return rc;
  if ((rc = ray_table_enqueue(c, q, rays, ra)) != RT_OK) return rc;
  if (sel.fast && sel.cull && scn.sg_ok)
    ra.sg = SgArgs{scn.sg_start.get(), scn.sg_ent.get(), scn.sg_rho2.get(), scn.sg_n, 1,
                   scn.sg_nstart,      scn.sg_nent, scn.nsph};
  void *args[] = {&ra};
  RT_TRY(c, hipLaunchKernel(kf, grid, dim3(64 * kWg), args, lds, c->stream));
  did = Launched{true, ra.cg.on != 0, bv.ug.on != 0, ra.dirs != nullptr, ra.cg.on ? ra.cg.N : 0};
  if (ra.dq_cap > 0) {  // 48 one-wave workgroups per shard segment
    // the walk kernel where every closest hit walks the BVH anyway (large
    // scenes: synth10k 12.2 -> 11.0 ms per 8-frame launch); small scenes keep
    // the cull sweeps (synth200 1 % slower on the walk kernel); else the
    // deferred waves' tails spread their light loops too (wide_mode 3)
    const bool walk = sel.cull && sel.fast && c->knobs.defer_walk && bv.nnodes > 0 && bv.always &&
                      !(bv.ug.on && bv.ug.closest);
    RT_TRY(c, hipLaunchKernel(deferred_kernel_fn(sel, walk, sel.fast && c->knobs.wide_mode == 3),
                              dim3(RT_DEFER_WGS * kShards), dim3(64), args, lds, c->stream));
  }
  return RT_OK;
}

int launch_render(rt_ctx *c, const LaunchReq &q, Launched &did) {
  const Cam cam = to_cam(q.cams[0]);
  const BvhArgs bv = bvh_args(c, cam);
  const OutDesc &od = q.od;
  // RT_HIP_LDS_SCENE: the scene and its BVH are staged in LDS when they fit (lds_layout)
  const bool lds_geo =
      c->knobs.lds_scene && lds_layout(true, c->scene.nsph, c->scene.nlight, bv.nnodes).end <= kLdsBudget;
  KernelSel sel{lds_geo, c->cull, c->samples == 4 ? 4 : 1, kStackGlobal};
  // merged reflection levels: RGB8 row-compact output, one sample, scene through L2,
  // and only while the wave's LDS (BVH stacks + ray queue) still allows the
  // 12 waves per CU its registers allow (synth10k's 22-entry stacks do not:
  // 10 waves, 12 % slower); otherwise the per-pixel global stack
  if (c->knobs.stack_mode == kStackMerge && !sel.lds && sel.samples == 1 && od.fmt == RT_FB_RGB8 && !od.full &&
      od.x0 == 0 && od.xw == q.W)
    for (int mq = c->knobs.merge_q_max; mq >= 8; mq /= 2)  // the longest queue that keeps 12 waves per CU
      if (12 * lds_plan(c->scene, bv, false, true, mq).total <= 160 * 1024) {
        sel.merge_q = mq;
        sel.stack = kStackMerge;
        break;
      }
  return launch_tiles(c, q, sel, cam, bv, did);
}

// The checks of every render entry point, in this order: arguments (`tiles`: the caller's
// tiles, whose signs are checked), the scene, the depth, then the request's rows and frames.
int validate(const rt_ctx *c, const LaunchReq &q, const rt_tile *tiles = nullptr, int ntiles = 0) {
  if (!c || !q.cams || !q.od.ptr || q.W <= 0 || q.H <= 0 || ntiles < 0 || (ntiles > 0 && !tiles))
    return RT_ERR_INVALID_ARG;
  if (q.od.fmt != RT_FB_RGB8 && q.od.fmt != RT_FB_F32X3 && q.od.fmt != RT_FB_F64X3) return RT_ERR_INVALID_ARG;
  for (int i = 0; i < ntiles; i++)
    if (tiles[i].x < 0 || tiles[i].y < 0 || tiles[i].width < 0 || tiles[i].height < 0) return RT_ERR_INVALID_ARG;
  if (!c->scene.has_scene) return RT_ERR_NO_SCENE;
  if (q.depth > RT_MAX_DEPTH) return RT_ERR_DEPTH;
  const Rows &r = q.rows;
  if (r.band < 1 || r.stride < 1 || r.first < 0 || r.count < 0) return RT_ERR_INVALID_ARG;
  if (!q.od.full && (long long)q.W * 3 * (long long)r.count > (1LL << 40)) return RT_ERR_INVALID_ARG;
  if (q.nframes < 1 || q.nframes > RT_MAX_FRAMES) return RT_ERR_INVALID_ARG;
  const size_t fstride = (size_t)q.od.fstride;  // (as rt_render_frames_async was given it)
  if (q.nframes > 1 && (fstride < (size_t)r.count * q.W * 3 || fstride > (size_t)1 << 62)) return RT_ERR_INVALID_ARG;
  return RT_OK;
}

Rows to_rows(const rt_rows *rows, int H) {  // nullptr: every row of the image
  return rows ? Rows{rows->band, rows->first, rows->stride, rows->count} : Rows{1, 0, 1, H};
}

int enqueue(rt_ctx *c, const LaunchReq &q) {
  RT_TRY(c, hipSetDevice(c->device));
  const int half = (int)(c->timing.launches & 1);
  c->ctr.cur = c->ctr.base.get() + (size_t)half * kShards * kShardStride;
  if (!c->ctr.clean[half])
    RT_TRY(c, hipMemsetAsync(c->ctr.cur, 0, kShards * kShardStride * sizeof(unsigned long long), c->stream));
  c->ctr.clean[half] = false;
  const int slot = c->timing.slot();
  RT_TRY(c, hipEventRecord(c->timing.ev0[slot], c->stream));
  Launched did;
  if (q.rows.count > 0) {
    const int rc = launch_render(c, q, did);
    if (rc != RT_OK) return rc;
    RT_TRY(c, hipGetLastError());
  }
  RT_TRY(c, hipEventRecord(c->timing.ev1[slot], c->stream));
  // the launch is on the stream: what it leaves for the next one and for rt_get_info
  if (did.kernel) {
    c->ctr.clean[(c->timing.launches + 1) & 1] = true;
    c->info.ug_last = did.ug;
  }
  c->info.cg_last = did.cg;
  c->info.cg_last_n = did.cg_n;
  c->info.rays_last = did.rays;
  c->timing.launches++;
  c->scene.launches++;
  return RT_OK;  // the counters are read back by rt_render_stats, after the stream drains
}

// ---- the caller-ray queries' host layer --------------------------------------
// What the ray, path and radiance entry points below share: the checks, a
// family's launch state, a launch's size, scene arguments and bracket, the
// counter read, and the staging of the synchronous calls.

// The checks, before any HIP call; an entry point lists them in the order it reports them.
bool bad_batch(const rt_ctx *c, size_t n, size_t max_n, const void *in, const void *out) {
  return !c || n > max_n || (n > 0 && (!in || !out));
}
int depth_status(int depth) {
  return depth < 1 ? RT_ERR_INVALID_ARG : depth > RT_MAX_DEPTH ? RT_ERR_DEPTH : RT_OK;
}
bool misaligned(const void *a, const void *b, const void *d = nullptr) {  // device arrays: 16 bytes
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(d)) & 15u) != 0;
}

// A family's events, counters and pinned read-back buffer, once per context.
int trace_state(rt_ctx *c, TraceState &q) {
  if (!q.ev0) RT_TRY(c, hipEventCreate(&q.ev0));
  if (!q.ev1) RT_TRY(c, hipEventCreate(&q.ev1));
  const size_t bytes = kShards * kShardStride * sizeof(unsigned long long);
  if (!q.ctr.get()) RT_TRY(c, q.ctr.alloc(bytes));
  if (!q.host.get()) {
    RT_TRY(c, q.host.alloc(bytes));
    std::memset(q.host.get(), 0, bytes);
  }
  return RT_OK;
}

// Dynamic LDS of the ordered walks' stacks: one wave per workgroup, [entry][lane]
// at the base of dynamic LDS.  Deeper than kOrderedStack (12 KiB; bvh_args never
// allows it) the launch takes the stackless walk and no LDS.
size_t walk_lds(BvhArgs &bv) {
  if (!bv.ordered) return 0;
  const size_t lds = (size_t)bv.odepth * 64 * 8;
  if (lds <= 12 * 1024) {
    bv.ostk_off = 0;
    return lds;
  }
  bv.ordered = bv.wide = 0;
  return 0;
}

// One-wave workgroups for n lanes, grid-stride: at most 64 waves per CU.
long long trace_grid(const rt_ctx *c, size_t n) {
  return std::min<long long>(((long long)n + 63) / 64, (long long)c->n_cu * 64);
}

// The scene half of a launch's arguments (QueryArgs, PathArgs), counting into q.
template <class A>
void scene_args(const rt_ctx *c, const TraceState &q, A &a) {
  const Scene &sc = c->scene;
  a.geo = sc.geo.get(), a.rad = sc.rad.get(), a.n = sc.nsph;
  a.accel = c->cull ? 1 : 0;
  for (int k = 0; k < 3; k++) a.rlo[k] = sc.q_lo[k], a.rhi[k] = sc.q_hi[k];
  a.bv = query_bvh_args(c);
  a.counters = q.ctr.get();
}
void path_scene_args(const rt_ctx *c, const TraceState &q, PathArgs &a) {
  scene_args(c, q, a);
  a.mat = c->scene.mat.get(), a.lights = c->scene.lights.get(), a.nl = c->scene.nlight;
}

// The bracket of a launch on the context's stream: q's counters zeroed and its
// events around `launch` (which enqueues the kernel), making it q's most recent.
template <class Launch>
int trace_launch(rt_ctx *c, TraceState &q, Launch launch) {
  RT_TRY(c, hipMemsetAsync(q.ctr.get(), 0, q.ctr.bytes(), c->stream));
  RT_TRY(c, hipEventRecord(q.ev0, c->stream));
  launch();
  RT_TRY(c, hipGetLastError());
  RT_TRY(c, hipEventRecord(q.ev1, c->stream));
  q.launched = true;
  return RT_OK;
}

// The shared part of the stats getters: waits for the stream; q's most recent
// launch as its counters summed over the shards and its event time, zeros
// before the first.
static_assert(kQueryCounters <= kRadianceCounters && kPathCounters <= kRadianceCounters, "sum[] holds every family's");
struct TraceCounts {
  unsigned long long sum[kRadianceCounters];
  double ms;
};
int trace_counts(rt_ctx *c, TraceState &q, TraceCounts &t) {
  t = TraceCounts{};
  RT_TRY(c, hipSetDevice(c->device));
  RT_TRY(c, hipStreamSynchronize(c->stream));
  if (!q.launched) return RT_OK;
  float ms = 0.f;
  RT_TRY(c, hipEventElapsedTime(&ms, q.ev0, q.ev1));
  t.ms = ms;
  unsigned long long *hc = q.host.get();
  RT_TRY(c, hipMemcpy(hc, q.ctr.get(), q.host.bytes(), hipMemcpyDeviceToHost));
  for (int sh = 0; sh < kShards; sh++)
    for (int k = 0; k < kRadianceCounters; k++) t.sum[k] += hc[sh * kShardStride + k];
  return RT_OK;
}
template <class S>  // rt_path_stats, and rt_radiance_stats' same fields
void path_stats_of(const TraceCounts &t, S *st) {
  st->rays = t.sum[kPcRays];
  st->segments = t.sum[kPcSegments];
  st->hits = t.sum[kPcHits];
  st->shadow_rays = t.sum[kPcShadow];
  st->tests_exact = t.sum[kPcExact];
  st->tests_cull = t.sum[kPcCull];
  st->unaccelerated = t.sum[kPcUnaccel];
  st->kernel_ms = t.ms;
}
void radiance_stats_of(const TraceCounts &t, rt_radiance_stats *st) {
  path_stats_of(t, st);
  st->negative_clamped = t.sum[kRcNegative];
}

// One array of a synchronous call: the caller's, and where the launch finds it.
enum { kStageIn = 1, kStageOut = 2 };
struct Staged {
  const void *p;         // the caller's pointer; nullptr: the array is not passed
  DevBuf<uint8_t> *buf;  // its grow-only place on the device when p is host memory
  size_t bytes;
  int dir;               // kStageIn: copied to the device ahead of the launch; kStageOut: copied back after it
  void *dev = nullptr;
  template <class T>
  T *as() const { return static_cast<T *>(dev); }
};

// The body of a synchronous entry point, after its checks: no rays is zero
// stats; the arrays are used where they are (on_device) or staged around
// `launch`, the family's _async form reading io[k].dev; then the family's stats.
template <class Stats, size_t K, class Launch>
int staged_call(rt_ctx *c, size_t n, Staged (&io)[K], bool on_device, int (*get)(rt_ctx *, Stats *), Stats *st,
                Launch launch) {
  if (n == 0) {
    if (st) *st = Stats{};
    return RT_OK;
  }
  RT_TRY(c, hipSetDevice(c->device));
  int rc;
  for (Staged &s : io) s.dev = const_cast<void *>(s.p);
  if (!on_device) {
    for (Staged &s : io) {
      if (!s.p) continue;
      if ((rc = grow(c, *s.buf, s.bytes)) != RT_OK) return rc;
      s.dev = s.buf->get();
    }
    for (Staged &s : io)
      if (s.p && (s.dir & kStageIn)) RT_TRY(c, hipMemcpyAsync(s.dev, s.p, s.bytes, hipMemcpyHostToDevice, c->stream));
  }
  if ((rc = launch()) != RT_OK) return rc;
  if (!on_device)
    for (Staged &s : io)
      if (s.p && (s.dir & kStageOut))
        RT_TRY(c, hipMemcpyAsync(const_cast<void *>(s.p), s.dev, s.bytes, hipMemcpyDeviceToHost, c->stream));
  Stats tmp;
  return get(c, st ? st : &tmp);
}

}  // namespace

extern "C" {

int rt_device_count(int *count) {
  if (!count) return RT_ERR_INVALID_ARG;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  *count = e == hipSuccess ? n : 0;
  return e == hipSuccess ? RT_OK : RT_ERR_NO_DEVICE;
}

int rt_create(int device, rt_ctx **out) {
  if (!out) return RT_ERR_INVALID_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return RT_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return RT_ERR_INVALID_ARG;
  rt_ctx *c = new rt_ctx(device, read_knobs());
  auto bail = [&](int rc) {
    rt_destroy(c);
    return rc;
  };
  if (hipSetDevice(device) != hipSuccess) return bail(RT_ERR_HIP);
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
      c->n_cu = prop.multiProcessorCount;
  }
  // A blocking stream: it is ordered with the legacy NULL stream (torch's
  // default stream), so buffers a caller fills there are ready before a
  // render on the context's own stream reads or overwrites them, and the
  // caller's later NULL-stream work sees the render's output.
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamDefault) != hipSuccess) return bail(RT_ERR_HIP);
  if (hipEventCreateWithFlags(&c->switch_ev, hipEventDisableTiming) != hipSuccess) return bail(RT_ERR_HIP);
  c->stream = c->own_stream;
  if (c->ctr.base.alloc(2 * kShards * kShardStride * sizeof(unsigned long long)) != hipSuccess)
    return bail(RT_ERR_OUT_OF_MEMORY);
  if (hipMemset(c->ctr.base.get(), 0, c->ctr.base.bytes()) != hipSuccess) return bail(RT_ERR_HIP);
  c->ctr.cur = c->ctr.base.get();
  if (c->ctr.host.alloc(kShards * kShardStride * sizeof(unsigned long long)) != hipSuccess)
    return bail(RT_ERR_OUT_OF_MEMORY);
  std::memset(c->ctr.host.get(), 0, c->ctr.host.bytes());
  for (int i = 0; i < LaunchTiming::kRing; i++)
    if (hipEventCreate(&c->timing.ev0[i]) != hipSuccess || hipEventCreate(&c->timing.ev1[i]) != hipSuccess) return bail(RT_ERR_HIP);
  // The HIP runtime's one-time work in a process, done here rather than
  // inside the first render: the kernels' code object loads at the first
  // launch, and the first blocking host-to-device copy, the first large
  // asynchronous copy (the staging path) each cost ~8 ms on the box
  // (scripts/copy_warm_probe.cpp).  So a drop-in's first render -- the time
  // ray_serial prints, main.cpp:139-163 -- is the render alone.  Once per
  // process and device.
  {
    static std::mutex warm_mu;
    static std::vector<int> warmed;
    std::lock_guard<std::mutex> lk(warm_mu);
    if (std::find(warmed.begin(), warmed.end(), device) == warmed.end()) {
      hipFuncAttributes fa;
      (void)hipFuncGetAttributes(&fa, render_kernel_fn(KernelSel{false, true, 1, kStackMerge, true, true}));  // the default
      std::vector<unsigned char> h((size_t)1 << 20);
      void *d = nullptr;
      if (hipMalloc(&d, h.size()) == hipSuccess) {
        (void)hipMemcpy(d, h.data(), 8, hipMemcpyHostToDevice);
        (void)hipMemcpyAsync(d, h.data(), h.size(), hipMemcpyHostToDevice, c->stream);
        (void)hipMemcpyAsync(h.data(), d, h.size(), hipMemcpyDeviceToHost, c->stream);
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(d);
      }
      (void)hipGetLastError();
      warmed.push_back(device);
    }
  }
  *out = c;
  return RT_OK;
}

void rt_destroy(rt_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
  if (c->stream && c->stream != c->own_stream) (void)hipStreamSynchronize(c->stream);
  for (int i = 0; i < LaunchTiming::kRing; i++) {
    if (c->timing.ev0[i]) (void)hipEventDestroy(c->timing.ev0[i]);
    if (c->timing.ev1[i]) (void)hipEventDestroy(c->timing.ev1[i]);
  }
  for (TraceState *q : {&c->query, &c->paths, &c->radiance}) {
    if (q->ev0) (void)hipEventDestroy(q->ev0);
    if (q->ev1) (void)hipEventDestroy(q->ev1);
  }
  if (c->switch_ev) (void)hipEventDestroy(c->switch_ev);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;  // the buffers free themselves
}

const char *rt_last_error(const rt_ctx *c) { return c ? c->err.c_str() : "null context"; }

int rt_set_stream(rt_ctx *c, void *s) {
  if (!c) return RT_ERR_INVALID_ARG;
  hipStream_t next = s ? (hipStream_t)s : c->own_stream;
  if (next != c->stream) {
    // The context's scratch (reflection stack, deferred queue, counters, tile
    // order) is shared by every launch: work enqueued on the new stream waits
    // for everything already enqueued on the old one.
    RT_TRY(c, hipSetDevice(c->device));
    RT_TRY(c, hipEventRecord(c->switch_ev, c->stream));
    RT_TRY(c, hipStreamWaitEvent(next, c->switch_ev, 0));
    c->stream = next;
  }
  return RT_OK;
}

int rt_set_culling(rt_ctx *c, int enable) {
  if (!c) return RT_ERR_INVALID_ARG;
  c->cull = enable != 0;
  return RT_OK;
}

// The device half of rt_upload_scene: the staged arrays to the device, then
// the grids that are built there.  The caller frees the scene on an error.
static int upload_staged(rt_ctx *c, const rt_scene *s, StagedScene &st, bool want_ug) {
  Scene &scn = c->scene;
  const int n = s->num_spheres;
  const auto t_bvh = std::chrono::steady_clock::now();
  RT_TRY(c, scn.bvh2.upload(st.nodes2, 1));
  RT_TRY(c, scn.bvh4.upload(st.nodes4, 1));
  RT_TRY(c, scn.pf.upload(st.pf, 1));
  RT_TRY(c, scn.bvh.upload(st.nodes, 1));
  RT_TRY(c, scn.prims.upload(st.prims, 1));
  c->info.bvh_build_ms = st.bvh_ms + ms_since(t_bvh);
  if (want_ug) {
    const auto t_ug = std::chrono::steady_clock::now();
    if (st.ug_built) {
      const UgridHost &ug = st.ug;
      RT_TRY(c, scn.ug_rec.upload(ug.rec));
      RT_TRY(c, scn.ug_rid.upload(ug.rid));
      RT_TRY(c, scn.ug_q.upload(ug.q));
      RT_TRY(c, scn.ug_ids.upload(ug.ids, 1));
      RT_TRY(c, scn.ug_glob.upload(ug.glob, 1));
      scn.ug = UgArgs{reinterpret_cast<const float4 *>(scn.ug_rec.get()), scn.ug_rid.get(),
                      reinterpret_cast<const float4 *>(scn.ug_q.get()), scn.ug_ids.get(), scn.ug_glob.get(),
                      (int)ug.glob.size(), ug.nx, ug.ny, ug.nz, ug.gx, ug.gy, ug.gz, ug.cs, 0, 0,
                      (float)(1e-4 * (double)ug.extent), (int)ug.q.size()};
      scn.ug_reg_margin = ug.reg_margin;
      scn.ug_extent = ug.extent;
      scn.ug_entries = ug.ids.size();
      scn.ug_ok = true;
    }
    c->info.ug_build_ms = st.ug_ms + ms_since(t_ug);
  }
  scn.bvh_nodes = (int)st.nodes.size(), scn.bvh2_nodes = (int)st.nodes2.size(), scn.bvh4_nodes = (int)st.nodes4.size();
  scn.bvh_prims = (int)st.prims.size();
  scn.bvh2_root = st.root2, scn.bvh_depth = st.depth2, scn.bvh4_root = st.root4, scn.bvh4_stack = st.stack4;
  for (int k = 0; k < 3; k++) {
    scn.c0[k] = st.c0[k];
    scn.lo[k] = st.lo[k];
    scn.hi[k] = st.hi[k];
  }
  scn.rmax = st.rmax;
  {  // the query region: the bounds grown on every side by their own diagonal (non-finite bounds: no region)
    double d2 = 0.0, r2 = 0.0;
    for (int k = 0; k < 3; k++) d2 += (scn.hi[k] - scn.lo[k]) * (scn.hi[k] - scn.lo[k]);
    const double diag = std::sqrt(d2);
    for (int k = 0; k < 3; k++) {
      scn.q_lo[k] = scn.lo[k] - diag;
      scn.q_hi[k] = scn.hi[k] + diag;
      r2 += (scn.q_hi[k] - scn.q_lo[k]) * (scn.q_hi[k] - scn.q_lo[k]);
    }
    scn.q_diam = std::sqrt(r2);
  }
  RT_TRY(c, scn.geo.upload(st.geo, 1));
  RT_TRY(c, scn.rad.upload(st.rad, 1));
  RT_TRY(c, scn.mat.upload(st.mat, 1));
  RT_TRY(c, scn.lights.upload(st.lights, 1));
  scn.lights_host = st.lights;
  // built on the device from geo / rad
  int rc = light_grids(c, s, st);
  if (rc != RT_OK) return rc;
  // the spheres' copy only where a grid may be built from it, until it has been
  const bool sg_auto = c->knobs.sg_mode < 0 && n <= kSgMaxSpheres;
  if (c->knobs.sg_mode > 0 || sg_auto) scn.sg_src.assign(s->spheres, s->spheres + n);
  scn.sg_diam = st.diam;
  scn.launches = 0;
  scn.sg_pending = sg_auto;
  if (c->knobs.sg_mode > 0 && (rc = sphere_grids(c)) != RT_OK) return rc;
  scn.nsph = n;
  scn.nlight = s->num_lights;
  scn.refl = std::move(st.refl);
  for (int q = 0; q < 3; q++) scn.amb[q] = s->ambient[q];
  return RT_OK;
}

int rt_upload_scene(rt_ctx *c, const rt_scene *s) {
  if (!c || !s || s->num_spheres < 0 || s->num_lights < 0) return RT_ERR_INVALID_ARG;
  if ((s->num_spheres > 0 && !s->spheres) || (s->num_lights > 0 && !s->lights)) return RT_ERR_INVALID_ARG;
  const auto t_upload = std::chrono::steady_clock::now();
  RT_TRY(c, hipSetDevice(c->device));
  RT_TRY(c, hipStreamSynchronize(c->stream));
  free_scene(c);
  c->radiance.area.reset();  // the light table goes with the scene: the light count may change
  c->radiance.area_samples = 0;
  c->radiance.gloss.reset();  // and the gloss table: the sphere count may change
  c->radiance.rough.reset();
  c->radiance.gloss_samples = c->radiance.gloss_bounces = 0;
  const bool big = s->num_spheres > kBvhAlwaysAbove;
  // leaves of 2 spheres (+0.6..0.9 % over 4 on synth200 with the merged levels);
  // 1 above kBvhAlwaysAbove, where every closest hit walks (synth10k 4.37 -> 4.16 ms)
  c->scene.bvh_leaf = c->knobs.bvh_leaf_opt ? c->knobs.bvh_leaf_opt : (big ? 1 : 2);
  c->scene.lg_n = c->knobs.lg_n_opt ? c->knobs.lg_n_opt : (big ? 768 : 128);
  const bool want_ug = c->knobs.ug_mode > 0 || (c->knobs.ug_mode < 0 && big);
  StagedScene st;
  stage_scene(s, c->scene.bvh_leaf, want_ug, c->knobs.ug_cells, st);
  const int rc = upload_staged(c, s, st, want_ug);
  if (rc != RT_OK) {
    free_scene(c);
    return rc;
  }
  c->scene_gen++;
  c->scene.has_scene = true;
  c->info.upload_ms = ms_since(t_upload);
  return RT_OK;
}

int rt_render_async(rt_ctx *c, const rt_camera *cam, int W, int H, int depth, const rt_rows *rows, uint8_t *out) {
  return rt_render_frames_async(c, cam, 1, W, H, depth, rows, out, 0);
}

int rt_render_frames_async(rt_ctx *c, const rt_camera *cams, int nframes, int W, int H, int depth,
                           const rt_rows *rows, uint8_t *out, size_t frame_stride) {
  const LaunchReq q{cams, nframes, W, H, depth, to_rows(rows, H),
                    OutDesc{out, RT_FB_RGB8, 0, 0, W, (long long)frame_stride}};
  const int rc = validate(c, q);
  return rc != RT_OK ? rc : enqueue(c, q);
}

int rt_render_stats(rt_ctx *c, rt_stats *st) {
  if (!c || !st) return RT_ERR_INVALID_ARG;
  RT_TRY(c, hipSetDevice(c->device));
  RT_TRY(c, hipStreamSynchronize(c->stream));
  float ms = 0.f;
  if (c->timing.launches > 0) {
    const int slot = (int)((c->timing.launches - 1) % LaunchTiming::kRing);
    RT_TRY(c, hipEventElapsedTime(&ms, c->timing.ev0[slot], c->timing.ev1[slot]));
  }
  const unsigned long long *hc = c->ctr.host.get();
  RT_TRY(c, hipMemcpy(c->ctr.host.get(), c->ctr.cur, c->ctr.host.bytes(), hipMemcpyDeviceToHost));
  unsigned long long sum[kCounters] = {};
  for (int sh = 0; sh < kShards; sh++)
    for (int q = 0; q < kCounters; q++) sum[q] += hc[sh * kShardStride + q];
  st->rays_primary = sum[0];
  st->rays_shadow = sum[1];
  st->rays_reflect = sum[2];
  st->negative_clamped = sum[3];
  st->tests_exact = sum[4];
  st->tests_cull = sum[5];
#ifdef RT_CHECK
  {
    // the first out-of-range device index of the launches since the last
    // read (rt_device.h RT_CK), then cleared for the next ones
    static const char *const kSiteNames[kCkSites] = {
        "?", "sphere index", "light-grid start", "light-grid list slot", "camera-grid start",
        "camera/sphere-grid list slot", "sphere-grid start", "sphere-grid key", "uniform-grid cell",
        "uniform-grid overflow slot", "BVH node reference", "BVH leaf slot", "tile order slot / tile id",
        "deferred-queue slot", "reflection-stack slot", "LDS ray-queue slot", "LDS pixel slot",
        "framebuffer offset", "camera-grid build slot", "stack-home pool exhausted"};
    CheckRec rec{};
    RT_TRY(c, hipMemcpyFromSymbol(&rec, HIP_SYMBOL(g_check), sizeof rec));
    if (rec.count) {
      const CheckRec zero{};
      RT_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(g_check), &zero, sizeof zero));
      c->err = std::string("RT_CHECK: ") + (rec.site < (unsigned long long)kCkSites ? kSiteNames[rec.site] : "?") +
               " index " + std::to_string((long long)rec.idx) + " outside [0, " + std::to_string(rec.bound) +
               ") (" + std::to_string(rec.count) + " violations)";
      return RT_ERR_CHECK;
    }
  }
#endif
#ifdef RT_STAMPS
  if (const char *tf = std::getenv("RT_HIP_STAMPS_FILE")) {
    static unsigned long long host_tl[kTimelineWaves * kTl];
    if (hipMemcpyFromSymbol(host_tl, HIP_SYMBOL(g_timeline), sizeof(host_tl)) == hipSuccess) {
      if (FILE *f = std::fopen(tf, "wb")) {
        std::fwrite(host_tl, sizeof(host_tl), 1, f);
        std::fclose(f);
      }
    }
  }
  if (std::getenv("RT_HIP_STAMPS")) {  // diagnostic builds (-DRT_STAMPS) fill slots 8..14
    unsigned long long d[12] = {};
    for (int sh = 0; sh < kShards; sh++)
      for (int q = 0; q < 12; q++) d[q] += hc[sh * kShardStride + 8 + q];
    const double nw = (double)(d[6] ? d[6] : 1);
    unsigned long long bvh = 0;
    for (int sh = 0; sh < kShards; sh++) bvh += hc[sh * kShardStride + 20];
    std::fprintf(stderr,
                 "RT_STAMPS per wave: candidate iterations %.1f (closest %.1f, of which primary %.1f), sweeps %.2f "
                 "(closest %.2f), bvh cycles %.0f\n",
                 d[7] / nw, d[9] / nw, d[11] / nw, d[8] / nw, d[10] / nw, bvh / nw);
    unsigned long long cl = 0, sh = 0;
    for (int s2 = 0; s2 < kShards; s2++) {
      cl += hc[s2 * kShardStride + 21];
      sh += hc[s2 * kShardStride + 22];
    }
    std::fprintf(stderr, "RT_STAMPS cycles/wave: closest hits %.0f, shadow queries %.0f\n", cl / nw, sh / nw);
    unsigned long long trips[3] = {};
    for (int s2 = 0; s2 < kShards; s2++)
      for (int q = 0; q < 3; q++) trips[q] += hc[s2 * kShardStride + 25 + q];
    std::fprintf(stderr, "RT_STAMPS wave-trips of the exact test: shadow lists %llu, grid scans %llu, sweeps and walks %llu\n",
                 trips[0], trips[1], trips[2]);
    std::fprintf(stderr, "RT_STAMPS waves=%llu cycles/wave: bound %.0f cull %.0f cand %.0f setup %.0f shade %.0f total %.0f\n",
                 d[6], (double)d[0] / (d[6] ? d[6] : 1), (double)d[1] / (d[6] ? d[6] : 1),
                 (double)d[2] / (d[6] ? d[6] : 1), (double)d[3] / (d[6] ? d[6] : 1),
                 (double)d[4] / (d[6] ? d[6] : 1), (double)d[5] / (d[6] ? d[6] : 1));
  }
#endif
  st->kernel_ms = ms;
  return RT_OK;
}

int rt_render(rt_ctx *c, const rt_camera *cam, int W, int H, int depth, const rt_rows *rows, uint8_t *out,
              int out_on_device, rt_stats *st) {
  LaunchReq q{cam, 1, W, H, depth, to_rows(rows, H), OutDesc{out, RT_FB_RGB8, 0, 0, W}};
  int rc = validate(c, q);
  if (rc != RT_OK) return rc;
  RT_TRY(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)q.rows.count * W * 3;
  if (!out_on_device) {
    rc = grow(c, c->tmp, bytes);
    if (rc != RT_OK) return rc;
    q.od.ptr = c->tmp.get();
  }
  rc = enqueue(c, q);
  if (rc != RT_OK) return rc;
  if (!out_on_device && bytes) RT_TRY(c, hipMemcpyAsync(out, q.od.ptr, bytes, hipMemcpyDeviceToHost, c->stream));
  rt_stats tmp;
  return rt_render_stats(c, st ? st : &tmp);
}

int rt_set_antialias(rt_ctx *c, int samples) {
  if (!c || (samples != 1 && samples != 4)) return RT_ERR_INVALID_ARG;
  c->samples = samples;
  return RT_OK;
}

int rt_render_tile(rt_ctx *c, const rt_camera *cam, int W, int H, int depth, int tile_x, int tile_y, int tile_w,
                   int tile_h, int fb_format, void *fb_device) {
  const rt_tile t{tile_x, tile_y, tile_w, tile_h};
  // the reference kernel clips the tile to the image (kernel.cu:103); in 64 bits: no overflow near INT_MAX
  const long long xe = std::min<long long>(W, (long long)tile_x + tile_w), ye = std::min<long long>(H, (long long)tile_y + tile_h);
  const int xw = (int)std::max(0LL, xe - tile_x), th = (int)std::max(0LL, ye - tile_y);
  // framebuffer rows j = tile_y .. ye-1 (j = 0 the bottom row) are PPM rows H-ye .. H-1-tile_y
  const Rows r{1, (int)(H - ye), 1, xw > 0 ? th : 0};
  const LaunchReq q{cam, 1, W, H, depth, r, OutDesc{fb_device, fb_format, 1, tile_x, xw}};
  const int rc = validate(c, q, &t, 1);
  return rc != RT_OK ? rc : enqueue(c, q);
}

int rt_render_tiles(rt_ctx *c, const rt_camera *cam, int W, int H, int depth, const rt_tile *tiles, int ntiles,
                    int fb_format, void *fb_device) {
  const LaunchReq q{cam, 1, W, H, depth, Rows{1, 0, 1, H}, OutDesc{fb_device, fb_format, 1, 0, W}, tiles, ntiles};
  const int rc = validate(c, q, tiles, ntiles);
  return rc != RT_OK ? rc : enqueue(c, q);
}

// ---- ray queries (rt_query.h) ----------------------------------------------
static int query_validate(const rt_ctx *c, int mode, const void *rays, size_t n, const void *hits) {
  if (bad_batch(c, n, INT32_MAX, rays, hits)) return RT_ERR_INVALID_ARG;
  if (mode != RT_QUERY_CLOSEST && mode != RT_QUERY_OCCLUDED) return RT_ERR_INVALID_ARG;
  return RT_OK;
}

int rt_trace_rays_async(rt_ctx *c, int mode, const rt_ray *rays, size_t n, rt_hit *hits) {
  int rc = query_validate(c, mode, rays, n, hits);
  if (rc != RT_OK) return rc;
  if (n == 0) return RT_OK;
  if (misaligned(rays, hits)) return RT_ERR_INVALID_ARG;  // ahead of the scene, unlike the paths and the radiance
  if (!c->scene.has_scene) return RT_ERR_NO_SCENE;
  RT_TRY(c, hipSetDevice(c->device));
  if ((rc = trace_state(c, c->query)) != RT_OK) return rc;
  QueryArgs a{};
  scene_args(c, c->query, a);
  a.nrays = (int)n, a.rays = rays, a.hits = hits;
  const size_t lds = walk_lds(a.bv);
  const dim3 grid((unsigned)trace_grid(c, n));
  return trace_launch(c, c->query, [&] {
    if (mode == RT_QUERY_CLOSEST)
      hipLaunchKernelGGL(query_kernel<RT_QUERY_CLOSEST>, grid, dim3(64), lds, c->stream, a);
    else
      hipLaunchKernelGGL(query_kernel<RT_QUERY_OCCLUDED>, grid, dim3(64), lds, c->stream, a);
  });
}

int rt_trace_stats(rt_ctx *c, rt_query_stats *st) {
  if (!c || !st) return RT_ERR_INVALID_ARG;
  *st = rt_query_stats{};
  TraceCounts t;
  const int rc = trace_counts(c, c->query, t);
  if (rc != RT_OK) return rc;
  st->rays = t.sum[kQcRays];
  st->hits = t.sum[kQcHits];
  st->tests_exact = t.sum[kQcExact];
  st->tests_cull = t.sum[kQcCull];
  st->rays_unaccelerated = t.sum[kQcUnaccel];
  st->kernel_ms = t.ms;
  return RT_OK;
}

int rt_trace_rays(rt_ctx *c, int mode, const rt_ray *rays, size_t n, rt_hit *hits, int on_device,
                  rt_query_stats *st) {
  const int rc = query_validate(c, mode, rays, n, hits);
  if (rc != RT_OK) return rc;
  if (n > 0 && !c->scene.has_scene) return RT_ERR_NO_SCENE;  // ahead of the _async form's alignment check
  Staged io[] = {{rays, &c->query.rays, n * sizeof(rt_ray), kStageIn},
                 {hits, &c->query.out[0], n * sizeof(rt_hit), kStageOut}};
  return staged_call(c, n, io, on_device, rt_trace_stats, st, [&] {
    return rt_trace_rays_async(c, mode, io[0].as<const rt_ray>(), n, io[1].as<rt_hit>());
  });
}

int rt_camera_rays(rt_ctx *c, const rt_camera *cam, int W, int H, const rt_rows *rows, rt_ray *rays) {
  if (!c || !cam || !rays || W <= 0 || H <= 0) return RT_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(rays) & 15u) return RT_ERR_INVALID_ARG;
  const Rows r = to_rows(rows, H);
  if (r.band < 1 || r.stride < 1 || r.first < 0 || r.count < 0) return RT_ERR_INVALID_ARG;
  const long long total = (long long)r.count * W;
  if (total > (long long)INT32_MAX) return RT_ERR_INVALID_ARG;
  if (total == 0) return RT_OK;
  RT_TRY(c, hipSetDevice(c->device));
  const unsigned grid = (unsigned)((total + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(camera_rays_kernel, dim3(grid), dim3(kBlock), 0, c->stream, to_cam(*cam), W, H, r, rays);
  RT_TRY(c, hipGetLastError());
  return RT_OK;
}

// ---- path queries (rt_paths.h) ---------------------------------------------
static int path_validate(const rt_ctx *c, const void *rays, size_t n, int depth, const void *verts) {
  if (bad_batch(c, n, INT32_MAX, rays, verts)) return RT_ERR_INVALID_ARG;
  if (const int rc = depth_status(depth)) return rc;
  if (n == 0) return RT_OK;
  if (!c->scene.has_scene) return RT_ERR_NO_SCENE;
  if (c->scene.nlight > RT_PATH_MAX_LIGHTS) return RT_ERR_INVALID_ARG;
  return RT_OK;
}

int rt_trace_paths_async(rt_ctx *c, const rt_ray *rays, size_t n, int depth, rt_vertex *verts, rt_surface *surf) {
  int rc = path_validate(c, rays, n, depth, verts);
  if (rc != RT_OK) return rc;
  if (n == 0) return RT_OK;
  if (misaligned(rays, verts, surf)) return RT_ERR_INVALID_ARG;
  RT_TRY(c, hipSetDevice(c->device));
  if ((rc = trace_state(c, c->paths)) != RT_OK) return rc;
  PathArgs a{};
  path_scene_args(c, c->paths, a);
  a.nrays = (int)n, a.depth = depth;
  a.rays = rays, a.verts = verts, a.surf = surf;
  const size_t lds = walk_lds(a.bv);
  const dim3 grid((unsigned)trace_grid(c, n));
  return trace_launch(c, c->paths, [&] {
    if (surf)
      hipLaunchKernelGGL(path_kernel<true>, grid, dim3(64), lds, c->stream, a);
    else
      hipLaunchKernelGGL(path_kernel<false>, grid, dim3(64), lds, c->stream, a);
  });
}

int rt_path_stats_get(rt_ctx *c, rt_path_stats *st) {
  if (!c || !st) return RT_ERR_INVALID_ARG;
  *st = rt_path_stats{};
  TraceCounts t;
  const int rc = trace_counts(c, c->paths, t);
  if (rc == RT_OK) path_stats_of(t, st);
  return rc;
}

int rt_trace_paths(rt_ctx *c, const rt_ray *rays, size_t n, int depth, rt_vertex *verts, rt_surface *surf,
                   int on_device, rt_path_stats *st) {
  const int rc = path_validate(c, rays, n, depth, verts);
  if (rc != RT_OK) return rc;
  const size_t nrec = n * (size_t)depth;
  // surfaces of untraced levels are not touched: the caller's bytes travel there and back
  Staged io[] = {{rays, &c->paths.rays, n * sizeof(rt_ray), kStageIn},
                 {verts, &c->paths.out[0], nrec * sizeof(rt_vertex), kStageOut},
                 {surf, &c->paths.out[1], nrec * sizeof(rt_surface), kStageIn | kStageOut}};
  return staged_call(c, n, io, on_device, rt_path_stats_get, st, [&] {
    return rt_trace_paths_async(c, io[0].as<const rt_ray>(), n, depth, io[1].as<rt_vertex>(), io[2].as<rt_surface>());
  });
}

// ---- radiance queries (rt_radiance.h) --------------------------------------
// Bytes of one output record; 0 for an unknown format.
static size_t radiance_record(int fmt) {
  return fmt == RT_FB_RGB8 ? 3 : fmt == RT_FB_F32X3 ? 3 * sizeof(float) : fmt == RT_FB_F64X3 ? 3 * sizeof(double) : 0;
}

// n records of `samples` rays each: 1 for rt_trace_radiance.
static int radiance_validate(const rt_ctx *c, const void *rays, size_t n, int samples, int depth, int fmt,
                             const void *out) {
  if (samples < 1 || samples > RT_MAX_SAMPLES) return RT_ERR_INVALID_ARG;
  if (bad_batch(c, n, (size_t)INT32_MAX / (size_t)samples, rays, out)) return RT_ERR_INVALID_ARG;
  if (radiance_record(fmt) == 0) return RT_ERR_INVALID_ARG;
  if (const int rc = depth_status(depth)) return rc;
  if (n == 0) return RT_OK;
  if (!c->scene.has_scene) return RT_ERR_NO_SCENE;
  return RT_OK;
}

// The light table of the resolving launches: record s * nl + l is the uploaded light l with its position
// moved by the caller's offset, one fp64 add per component, formed here so that the kernel only reads.
int rt_set_light_samples(rt_ctx *c, const double *xyz, int samples) {
  if (!c) return RT_ERR_INVALID_ARG;
  if (xyz && (samples < 1 || samples > RT_MAX_SAMPLES)) return RT_ERR_INVALID_ARG;
  if (!c->scene.has_scene) return RT_ERR_NO_SCENE;
  RT_TRY(c, hipSetDevice(c->device));
  RT_TRY(c, hipStreamSynchronize(c->stream));  // work in flight may read the table being replaced
  TraceState &rs = c->radiance;
  if (!xyz) {
    rs.area.reset();
    rs.area_samples = 0;
    return RT_OK;
  }
  const std::vector<LightD> &src = c->scene.lights_host;
  const size_t nl = src.size();
  std::vector<LightD> rec((size_t)samples * nl);
  for (size_t s = 0; s < (size_t)samples; s++)
    for (size_t l = 0; l < nl; l++) {
      const double *o = xyz + (s * nl + l) * 3;
      LightD L = src[l];
      L.px = L.px + o[0], L.py = L.py + o[1], L.pz = L.pz + o[2];
      rec[s * nl + l] = L;
    }
  DevBuf<LightD> next;  // the previous table stays in force if this fails
  RT_TRY(c, next.upload(rec, 1));
  rs.area = std::move(next);
  rs.area_samples = samples;
  return RT_OK;
}

// `samples` of a resolving call against the light table's, where a table is set: they agree.
static bool light_table_mismatch(const rt_ctx *c, int samples) {
  return c->radiance.area_samples != 0 && c->radiance.area_samples != samples;
}

// The gloss table of the resolving launches: the caller's points and the spheres' roughness, uploaded as
// they are; the kernel forms rd + g * roughness itself (radiance_kernel, kGloss).
int rt_set_gloss_samples(rt_ctx *c, const double *roughness, const double *xyz, int samples, int bounces) {
  if (!c) return RT_ERR_INVALID_ARG;
  if (xyz && (!roughness || samples < 1 || samples > RT_MAX_SAMPLES || bounces < 1 || bounces > RT_MAX_GLOSS_BOUNCES))
    return RT_ERR_INVALID_ARG;
  if (!c->scene.has_scene) return RT_ERR_NO_SCENE;
  RT_TRY(c, hipSetDevice(c->device));
  RT_TRY(c, hipStreamSynchronize(c->stream));  // work in flight may read the table being replaced
  TraceState &rs = c->radiance;
  if (!xyz) {
    rs.gloss.reset();
    rs.rough.reset();
    rs.gloss_samples = rs.gloss_bounces = 0;
    return RT_OK;
  }
  const size_t np = (size_t)samples * (size_t)bounces;
  std::vector<D3> pts(np);
  for (size_t i = 0; i < np; i++) pts[i] = D3{xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]};
  const std::vector<double> rough(roughness, roughness + c->scene.nsph);
  DevBuf<D3> next;  // the previous table stays in force if this fails
  DevBuf<double> next_rough;
  RT_TRY(c, next.upload(pts, 1));
  RT_TRY(c, next_rough.upload(rough, 1));
  rs.gloss = std::move(next);
  rs.rough = std::move(next_rough);
  rs.gloss_samples = samples, rs.gloss_bounces = bounces;
  return RT_OK;
}

// `samples` of a resolving call against the gloss table's, where a table is set: they agree.
static bool gloss_table_mismatch(const rt_ctx *c, int samples) {
  return c->radiance.gloss_samples != 0 && c->radiance.gloss_samples != samples;
}

// The most reflection-stack scratch a radiance launch takes.  A launch of
// `grid` one-wave workgroups at `depth` needs grid * 64 * (depth - 1) entries
// of 32 bytes: 32 MiB per level below the first for the full grid of 64 waves
// per CU on 256 CUs.  Depths up to 9 fit; a deeper launch gets a smaller grid
// (at depth 64 still 2080 waves, two per SIMD of such a device), never a
// larger budget ("Radiance").
constexpr size_t kRadianceStackBudget = 256u << 20;

// What a resolving launch adds to a radiance launch (rt_trace_radiance_resolve).
struct ResolveSpec {
  int samples;
  const double *weights;  // host, samples of them; nullptr: the box filter
};

// What the fused launch adds to a resolving launch (rt_render_samples_async): the view its lanes form
// their rays from.  `rows` holds the real output rows only.
struct GenSpec {
  const rt_camera *cam;
  int W, H;
  Rows rows;
  const double *offsets;  // host, 2 * samples of them
  const double *lens;     // host, 2 * samples lens points: radiance_kernel<true, true, true>; nullptr: the pinhole
  double focus;           // with `lens`: the distance of the plane that stays sharp
};

// Bytes of reflection stack per one-wave workgroup of a launch at `depth` (> 1).
static size_t radiance_stack_per_wave(int depth) { return (size_t)64 * (size_t)(depth - 1) * sizeof(StackEnt); }

// The one-wave workgroups of a radiance launch of n lanes' worth of records: the reflection stack belongs
// to the launch's lane slots, so the grid bounds it, not n; depth 1 spawns nothing and takes none.
static long long radiance_grid(const rt_ctx *c, size_t n, int depth) {
  long long grid = trace_grid(c, n);
  if (depth > 1)
    grid = std::min<long long>(
        grid, std::max<long long>(1, (long long)(kRadianceStackBudget / radiance_stack_per_wave(depth))));
  return grid;
}

// The tables of a context that a resolving launch reads: each nullptr where none is set (or the scene has
// nothing for it to act on: no lights, no spheres).
struct ResolveTables {
  const LightD *area;
  const D3 *gloss;
  const double *rough;
  int bounces;
};

// A resolving launch of the form <kGen, kLens> on its own argument block: the instantiation the tables
// choose (kArea, kGloss), the block followed by their addresses.
extern "C++" {
template <bool kGen, bool kLens, class Base>
static void resolve_go(const Base &b, const ResolveTables &t, unsigned grid, size_t lds, hipStream_t stream) {
  auto go = [&](auto kernel, const auto &args) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, stream, args);
  };
  auto with_gloss = [&](auto &x) { x.gloss = t.gloss, x.rough = t.rough, x.bounces = t.bounces; };
  if (!t.area && !t.gloss) {
    go(radiance_kernel<true, kGen, kLens>, b);
  } else if (!t.gloss) {
    AreaArgs<Base> x{};
    static_cast<Base &>(x) = b;
    x.area = t.area;
    go(radiance_kernel<true, kGen, kLens, true>, x);
  } else if (!t.area) {
    GlossArgs<Base> x{};
    static_cast<Base &>(x) = b;
    with_gloss(x);
    go(radiance_kernel<true, kGen, kLens, false, true>, x);
  } else {
    GlossArgs<AreaArgs<Base>> x{};
    static_cast<Base &>(x) = b;
    x.area = t.area;
    with_gloss(x);
    go(radiance_kernel<true, kGen, kLens, true, true>, x);
  }
}
}  // extern "C++"

// One radiance launch, validated by its entry point: n records from n rays (rv == nullptr,
// radiance_kernel<false>), from n * rv->samples rays (radiance_kernel<true>) or, with `gen`, from
// n * rv->samples rays the lanes form themselves (radiance_kernel<true, true>, or with gen->lens
// radiance_kernel<true, true, true>; rays == nullptr).  A resolving launch of a context with a light table
// (and lights) is the same form's kArea instantiation, its argument block followed by the table's address;
// of one with a gloss table (and spheres) the kGloss instantiation, likewise (resolve_go).
static int radiance_launch(rt_ctx *c, const rt_ray *rays, size_t n, int depth, int fmt, void *out,
                           const ResolveSpec *rv, const GenSpec *gen = nullptr) {
  int rc;
  RT_TRY(c, hipSetDevice(c->device));
  TraceState &rs = c->radiance;
  if ((rc = trace_state(c, rs)) != RT_OK) return rc;
  RadianceArgs a{};
  path_scene_args(c, rs, a.q);
  a.q.nrays = (int)n, a.q.depth = depth, a.q.rays = rays;
  a.amb = D3{c->scene.amb[0], c->scene.amb[1], c->scene.amb[2]};
  a.fmt = fmt, a.out = out;
  size_t lds = walk_lds(a.q.bv);
  a.park_off = (int)lds;  // the wave's parked colours behind the walks' stacks
  lds += 64 * sizeof(D3);
  const long long grid = radiance_grid(c, n, depth);
  if (depth > 1) {
    if ((rc = grow(c, rs.stack, (size_t)grid * radiance_stack_per_wave(depth))) != RT_OK) return rc;
    a.stack = rs.stack.get();
  }
  a.sstride = (unsigned)grid * 64u;
  return trace_launch(c, rs, [&] {
    if (!rv) {
      hipLaunchKernelGGL(radiance_kernel<false>, dim3((unsigned)grid), dim3(64), lds, c->stream, a);
      return;
    }
    auto resolve_args = [&](ResolveArgs &ra) {
      ra.r = a;
      ra.samples = rv->samples;
      ra.mode = rv->weights ? kResolveWeighted : rv->samples == 1 ? kResolveSingle : kResolveBox;
      ra.inv = 1.0 / (double)rv->samples;
      for (int s = 0; s < rv->samples; s++) ra.w[s] = rv->weights ? rv->weights[s] : 1.0;
    };
    lds += 64 * sizeof(D3);  // the wave's accumulators, right behind its parked colours
    const ResolveTables tab{rs.area_samples != 0 && c->scene.nlight > 0 ? rs.area.get() : nullptr,
                            rs.gloss_samples != 0 && c->scene.nsph > 0 ? rs.gloss.get() : nullptr, rs.rough.get(),
                            rs.gloss_bounces};
    if (!gen) {
      ResolveArgs ra{};
      resolve_args(ra);
      resolve_go<false, false>(ra, tab, (unsigned)grid, lds, c->stream);
      return;
    }
    auto gen_args = [&](GenArgs &ga) {
      resolve_args(ga);
      ga.cam = to_cam(*gen->cam);
      ga.W = gen->W, ga.H = gen->H, ga.rows = gen->rows;
      std::memcpy(ga.xy, gen->offsets, (size_t)rv->samples * 2 * sizeof(double));  // by value: free on return
    };
    if (!gen->lens) {
      GenArgs ga{};
      gen_args(ga);
      resolve_go<true, false>(ga, tab, (unsigned)grid, lds, c->stream);
      return;
    }
    LensArgs la{};
    gen_args(la);
    la.focus = gen->focus;
    std::memcpy(la.lens, gen->lens, (size_t)rv->samples * 2 * sizeof(double));
    resolve_go<true, true>(la, tab, (unsigned)grid, lds, c->stream);
  });
}

int rt_trace_radiance_async(rt_ctx *c, const rt_ray *rays, size_t n, int depth, int fmt, void *out) {
  const int rc = radiance_validate(c, rays, n, 1, depth, fmt, out);
  if (rc != RT_OK) return rc;
  if (n == 0) return RT_OK;
  if (misaligned(rays, out)) return RT_ERR_INVALID_ARG;
  return radiance_launch(c, rays, n, depth, fmt, out, nullptr);
}

int rt_radiance_stats_get(rt_ctx *c, rt_radiance_stats *st) {
  if (!c || !st) return RT_ERR_INVALID_ARG;
  *st = rt_radiance_stats{};
  TraceCounts t;
  const int rc = trace_counts(c, c->radiance, t);
  if (rc == RT_OK) radiance_stats_of(t, st);
  return rc;
}

int rt_trace_radiance(rt_ctx *c, const rt_ray *rays, size_t n, int depth, int fmt, void *out, int on_device,
                      rt_radiance_stats *st) {
  const int rc = radiance_validate(c, rays, n, 1, depth, fmt, out);
  if (rc != RT_OK) return rc;
  Staged io[] = {{rays, &c->radiance.rays, n * sizeof(rt_ray), kStageIn},
                 {out, &c->radiance.out[0], n * radiance_record(fmt), kStageOut}};
  return staged_call(c, n, io, on_device, rt_radiance_stats_get, st, [&] {
    return rt_trace_radiance_async(c, io[0].as<const rt_ray>(), n, depth, fmt, io[1].dev);
  });
}

// ---- multi-sample pixels (rt_radiance.h, kResolve) --------------------------
// The checks rt_camera_sample_rays and rt_render_samples share, before any HIP call.
static int sample_rays_validate(const rt_ctx *c, const rt_camera *cam, int W, int H, const Rows &r,
                                const double *offsets, int samples) {
  if (!c || !cam || !offsets || W <= 0 || H <= 0) return RT_ERR_INVALID_ARG;
  if (samples < 1 || samples > RT_MAX_SAMPLES) return RT_ERR_INVALID_ARG;
  if (r.band < 1 || r.stride < 1 || r.first < 0 || r.count < 0) return RT_ERR_INVALID_ARG;
  return RT_OK;
}

// The rays of output rows k_first .. k_first + nrows - 1 of `r`, nrows * W * samples <= 2^31-1 of them.
static int sample_rays_launch(rt_ctx *c, const rt_camera *cam, int W, int H, const Rows &r, int k_first, int nrows,
                              const double *offsets, int samples, rt_ray *rays) {
  SampleOffsets off{};
  std::memcpy(off.xy, offsets, (size_t)samples * 2 * sizeof(double));  // by value: the caller's array is free on return
  const long long total = (long long)nrows * W * samples;
  const unsigned grid = (unsigned)((total + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(camera_sample_rays_kernel, dim3(grid), dim3(kBlock), 0, c->stream, to_cam(*cam), W, H, r, k_first,
                     nrows, samples, off, rays);
  RT_TRY(c, hipGetLastError());
  return RT_OK;
}

int rt_camera_sample_rays(rt_ctx *c, const rt_camera *cam, int W, int H, const rt_rows *rows, const double *offsets,
                          int samples, rt_ray *rays) {
  if (!rays || (reinterpret_cast<uintptr_t>(rays) & 15u)) return RT_ERR_INVALID_ARG;
  const Rows r = to_rows(rows, H);
  const int rc = sample_rays_validate(c, cam, W, H, r, offsets, samples);
  if (rc != RT_OK) return rc;
  const long long total = (long long)r.count * W * samples;  // < 2^31 * 2^31 * 2^6
  if (total > (long long)INT32_MAX) return RT_ERR_INVALID_ARG;
  if (total == 0) return RT_OK;
  RT_TRY(c, hipSetDevice(c->device));
  return sample_rays_launch(c, cam, W, H, r, 0, r.count, offsets, samples, rays);
}

int rt_camera_lens_rays(rt_ctx *c, const rt_camera *cam, int W, int H, const rt_rows *rows, const double *offsets,
                        const double *lens, double focus, int samples, rt_ray *rays) {
  if (!rays || !lens || (reinterpret_cast<uintptr_t>(rays) & 15u)) return RT_ERR_INVALID_ARG;
  const Rows r = to_rows(rows, H);
  const int rc = sample_rays_validate(c, cam, W, H, r, offsets, samples);
  if (rc != RT_OK) return rc;
  const long long total = (long long)r.count * W * samples;  // < 2^31 * 2^31 * 2^6
  if (total > (long long)INT32_MAX) return RT_ERR_INVALID_ARG;
  if (total == 0) return RT_OK;
  RT_TRY(c, hipSetDevice(c->device));
  SampleOffsets off{};
  SampleLens ln{};
  std::memcpy(off.xy, offsets, (size_t)samples * 2 * sizeof(double));  // by value: the caller's arrays are free on return
  std::memcpy(ln.xy, lens, (size_t)samples * 2 * sizeof(double));
  ln.focus = focus;
  const unsigned grid = (unsigned)((total + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(camera_lens_rays_kernel, dim3(grid), dim3(kBlock), 0, c->stream, to_cam(*cam), W, H, r, samples,
                     off, ln, rays);
  RT_TRY(c, hipGetLastError());
  return RT_OK;
}

int rt_trace_radiance_resolve_async(rt_ctx *c, const rt_ray *rays, size_t n, int samples, const double *weights,
                                    int depth, int fmt, void *out) {
  const int rc = radiance_validate(c, rays, n, samples, depth, fmt, out);
  if (rc != RT_OK) return rc;
  if (light_table_mismatch(c, samples) || gloss_table_mismatch(c, samples)) return RT_ERR_INVALID_ARG;
  if (n == 0) return RT_OK;
  if (misaligned(rays, out)) return RT_ERR_INVALID_ARG;
  const ResolveSpec rv{samples, weights};
  return radiance_launch(c, rays, n, depth, fmt, out, &rv);
}

int rt_trace_radiance_resolve(rt_ctx *c, const rt_ray *rays, size_t n, int samples, const double *weights, int depth,
                              int fmt, void *out, int on_device, rt_radiance_stats *st) {
  const int rc = radiance_validate(c, rays, n, samples, depth, fmt, out);
  if (rc != RT_OK) return rc;
  if (light_table_mismatch(c, samples) || gloss_table_mismatch(c, samples)) return RT_ERR_INVALID_ARG;
  Staged io[] = {{rays, &c->radiance.rays, n * (size_t)samples * sizeof(rt_ray), kStageIn},
                 {out, &c->radiance.out[0], n * radiance_record(fmt), kStageOut}};
  return staged_call(c, n, io, on_device, rt_radiance_stats_get, st, [&] {
    return rt_trace_radiance_resolve_async(c, io[0].as<const rt_ray>(), n, samples, weights, depth, fmt, io[1].dev);
  });
}

// The rows of the image among the output rows of `r`: a prefix (y grows with k), the padding rows
// their suffix.  The first k with row_y(k) >= H.
static int real_rows(const Rows &r, int H) {
  auto row_y = [&](int k) {
    return (long long)(k / r.band) * r.band * r.stride + (long long)r.first * r.band + (k % r.band);
  };
  int lo = 0, hi = r.count;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (row_y(mid) < H) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The ray buffer of rt_render_samples when the caller names no bound: a choice, 4 Mi rays
// ("Samples", has the sweep).
constexpr size_t kSampleRayBytes = 256u << 20;

int rt_render_samples(rt_ctx *c, const rt_camera *cam, int W, int H, int depth, const rt_rows *rows,
                      const double *offsets, int samples, const double *weights, int fmt, void *out, int on_device,
                      size_t max_ray_bytes, rt_radiance_stats *st) {
  const Rows r = to_rows(rows, H);
  int rc = sample_rays_validate(c, cam, W, H, r, offsets, samples);
  if (rc != RT_OK) return rc;
  if (light_table_mismatch(c, samples) || gloss_table_mismatch(c, samples)) return RT_ERR_INVALID_ARG;
  const long long row_rays = (long long)W * samples;  // one output row: the smallest chunk
  if (row_rays > (long long)INT32_MAX) return RT_ERR_INVALID_ARG;
  const size_t rec = radiance_record(fmt);
  if (rec == 0) return RT_ERR_INVALID_ARG;
  if ((rc = depth_status(depth)) != RT_OK) return rc;
  if (r.count == 0) {
    if (st) *st = rt_radiance_stats{};
    return RT_OK;
  }
  if (!out || (on_device && (reinterpret_cast<uintptr_t>(out) & 15u))) return RT_ERR_INVALID_ARG;
  if (!c->scene.has_scene) return RT_ERR_NO_SCENE;
  RT_TRY(c, hipSetDevice(c->device));
  const int real = real_rows(r, H);
  const size_t cap = max_ray_bytes ? max_ray_bytes : kSampleRayBytes;
  long long chunk = std::max<long long>(1, (long long)(cap / ((size_t)row_rays * sizeof(rt_ray))));
  chunk = std::min<long long>(chunk, (long long)INT32_MAX / row_rays);
  TraceState &rs = c->radiance;  // the chunks' rays and, for host memory, their records: the family's staging
  uint8_t *dst = static_cast<uint8_t *>(out);
  const ResolveSpec rv{samples, weights};
  TraceCounts sum{}, one;
  for (int k0 = 0; k0 < real; k0 += (int)chunk) {
    const int nr = (int)std::min<long long>(chunk, real - k0);
    const size_t npx = (size_t)nr * W, off = (size_t)k0 * W * rec;
    if ((rc = grow(c, rs.rays, npx * samples * sizeof(rt_ray))) != RT_OK) return rc;
    if (!on_device && (rc = grow(c, rs.out[0], npx * rec)) != RT_OK) return rc;
    rt_ray *rays = reinterpret_cast<rt_ray *>(rs.rays.get());
    if ((rc = sample_rays_launch(c, cam, W, H, r, k0, nr, offsets, samples, rays)) != RT_OK) return rc;
    // a chunk's records begin where the previous chunk's end: aligned as the format, not to 16 bytes (the
    // kernel's packed RGB8 store tests the alignment it needs)
    void *d_out = on_device ? static_cast<void *>(dst + off) : static_cast<void *>(rs.out[0].get());
    if ((rc = radiance_launch(c, rays, npx, depth, fmt, d_out, &rv)) != RT_OK) return rc;
    if (!on_device) RT_TRY(c, hipMemcpyAsync(dst + off, d_out, npx * rec, hipMemcpyDeviceToHost, c->stream));
    if ((rc = trace_counts(c, rs, one)) != RT_OK) return rc;
    for (int k = 0; k < kRadianceCounters; k++) sum.sum[k] += one.sum[k];
    sum.ms += one.ms;
  }
  // padding rows: not traced, not counted, zero bytes
  const size_t pad_off = (size_t)real * W * rec, pad = (size_t)(r.count - real) * W * rec;
  if (pad) {
    if (on_device) {
      RT_TRY(c, hipMemsetAsync(dst + pad_off, 0, pad, c->stream));
      RT_TRY(c, hipStreamSynchronize(c->stream));
    } else {
      std::memset(dst + pad_off, 0, pad);
    }
  }
  if (st) {
    *st = rt_radiance_stats{};
    radiance_stats_of(sum, st);
  }
  return RT_OK;
}

// What the fused calls check before any HIP call, in rt_render_samples' order; `align`: out is device
// memory.  real: the real rows of r.  r.count == 0 returns RT_OK with nothing else checked.
static int fused_validate(const rt_ctx *c, const rt_camera *cam, int W, int H, int depth, const Rows &r,
                          const double *offsets, int samples, int fmt, const void *out, bool align, int &real) {
  real = 0;
  int rc = sample_rays_validate(c, cam, W, H, r, offsets, samples);
  if (rc != RT_OK) return rc;
  if (light_table_mismatch(c, samples) || gloss_table_mismatch(c, samples)) return RT_ERR_INVALID_ARG;
  if ((long long)W * samples > (long long)INT32_MAX) return RT_ERR_INVALID_ARG;  // rt_render_samples' row limit
  if ((long long)r.count * W > (long long)INT32_MAX) return RT_ERR_INVALID_ARG;  // one launch: its pixels
  if (radiance_record(fmt) == 0) return RT_ERR_INVALID_ARG;
  if ((rc = depth_status(depth)) != RT_OK) return rc;
  if (r.count == 0) return RT_OK;
  if (!out || (align && (reinterpret_cast<uintptr_t>(out) & 15u))) return RT_ERR_INVALID_ARG;
  if (!c->scene.has_scene) return RT_ERR_NO_SCENE;
  real = real_rows(r, H);
  const size_t npx = (size_t)real * W;
  if (npx) {
    // The kernel counts per lane in 32 bits and adds up per wave in 64.  A lane makes `trips` grid-stride
    // trips of `samples` chains of at most `depth` segments, each with at most one shadow ray per light;
    // its largest counter (the unaccelerated segments and shadow rays) stays below this product.
    const long long lanes = radiance_grid(c, npx, depth) * 64;
    const long long trips = ((long long)npx + lanes - 1) / lanes;  // <= 2^25
    const long long per_trip = (long long)samples * depth * (1 + (long long)c->scene.nlight);  // < 2^12 * 2^32
    if (per_trip > (long long)UINT32_MAX / trips) return RT_ERR_INVALID_ARG;
  }
  return RT_OK;
}

// A validated fused call, r.count > 0: the real rows are one launch whose lanes form their pixels' sample
// rays (through the lens when `lens` is given), the padding rows one memset behind it.  Only enqueues.
static int fused_enqueue(rt_ctx *c, const rt_camera *cam, int W, int H, int depth, const Rows &r, int real,
                         const double *offsets, const double *lens, double focus, int samples,
                         const double *weights, int fmt, void *out) {
  int rc;
  const size_t rec = radiance_record(fmt), npx = (size_t)real * W;
  uint8_t *dst = static_cast<uint8_t *>(out);
  if (npx) {
    const ResolveSpec rv{samples, weights};
    const GenSpec gen{cam, W, H, Rows{r.band, r.first, r.stride, real}, offsets, lens, focus};
    if ((rc = radiance_launch(c, nullptr, npx, depth, fmt, dst, &rv, &gen)) != RT_OK) return rc;
  } else {
    RT_TRY(c, hipSetDevice(c->device));
  }
  // padding rows: not traced, not counted, zero bytes
  const size_t pad = (size_t)(r.count - real) * W * rec;
  if (pad) RT_TRY(c, hipMemsetAsync(dst + npx * rec, 0, pad, c->stream));
  return RT_OK;
}

// rt_render_samples without its ray buffer, and so without its chunks and host waits: the real rows are
// one radiance_kernel<true, true> launch whose lanes form their pixels' sample rays, the padding rows one
// memset behind it.
int rt_render_samples_async(rt_ctx *c, const rt_camera *cam, int W, int H, int depth, const rt_rows *rows,
                            const double *offsets, int samples, const double *weights, int fmt, void *out) {
  const Rows r = to_rows(rows, H);
  int real;
  const int rc = fused_validate(c, cam, W, H, depth, r, offsets, samples, fmt, out, true, real);
  if (rc != RT_OK || r.count == 0) return rc;
  return fused_enqueue(c, cam, W, H, depth, r, real, offsets, nullptr, 0.0, samples, weights, fmt, out);
}

// rt_render_samples_async through a thin lens: radiance_kernel<true, true, true>.
int rt_render_lens_samples_async(rt_ctx *c, const rt_camera *cam, int W, int H, int depth, const rt_rows *rows,
                                 const double *offsets, const double *lens, double focus, int samples,
                                 const double *weights, int fmt, void *out) {
  if (!lens) return RT_ERR_INVALID_ARG;
  const Rows r = to_rows(rows, H);
  int real;
  const int rc = fused_validate(c, cam, W, H, depth, r, offsets, samples, fmt, out, true, real);
  if (rc != RT_OK || r.count == 0) return rc;
  return fused_enqueue(c, cam, W, H, depth, r, real, offsets, lens, focus, samples, weights, fmt, out);
}

// The synchronous form: the fused launch where `out` is (device memory) or into the family's grow-only
// `out` staging with one copy back behind it (host memory), then one wait.
int rt_render_lens_samples(rt_ctx *c, const rt_camera *cam, int W, int H, int depth, const rt_rows *rows,
                           const double *offsets, const double *lens, double focus, int samples,
                           const double *weights, int fmt, void *out, int on_device, rt_radiance_stats *st) {
  if (!lens) return RT_ERR_INVALID_ARG;
  const Rows r = to_rows(rows, H);
  int real, rc = fused_validate(c, cam, W, H, depth, r, offsets, samples, fmt, out, on_device != 0, real);
  if (rc != RT_OK) return rc;
  if (st) *st = rt_radiance_stats{};
  if (r.count == 0) return RT_OK;
  RT_TRY(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)r.count * W * radiance_record(fmt);
  void *dev = out;
  if (!on_device) {
    if ((rc = grow(c, c->radiance.out[0], bytes)) != RT_OK) return rc;
    dev = c->radiance.out[0].get();
  }
  if ((rc = fused_enqueue(c, cam, W, H, depth, r, real, offsets, lens, focus, samples, weights, fmt, dev)) != RT_OK)
    return rc;
  if (!on_device) RT_TRY(c, hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  if (real == 0) {  // nothing launched: the family's report is an earlier call's
    RT_TRY(c, hipStreamSynchronize(c->stream));
    return RT_OK;
  }
  rt_radiance_stats tmp;
  return rt_radiance_stats_get(c, st ? st : &tmp);
}

int rt_kernel_times(rt_ctx *c, double *ms_out, int max_n, int *n_out) {
  if (!c || !n_out || max_n < 0 || (max_n > 0 && !ms_out)) return RT_ERR_INVALID_ARG;
  RT_TRY(c, hipSetDevice(c->device));
  RT_TRY(c, hipStreamSynchronize(c->stream));
  long long avail = c->timing.launches - c->timing.hist_begin;
  if (avail > LaunchTiming::kRing) avail = LaunchTiming::kRing;
  if (avail > max_n) avail = max_n;
  for (long long i = 0; i < avail; i++) {
    const int slot = (int)((c->timing.launches - avail + i) % LaunchTiming::kRing);
    float ms = 0.f;
    RT_TRY(c, hipEventElapsedTime(&ms, c->timing.ev0[slot], c->timing.ev1[slot]));
    ms_out[i] = ms;
  }
  *n_out = (int)avail;
  c->timing.hist_begin = c->timing.launches;
  return RT_OK;
}

int rt_get_info(rt_ctx *c, rt_info *out) {
  if (!c || !out) return RT_ERR_INVALID_ARG;
  *out = rt_info{};
  out->cam_grid_last = c->info.cg_last ? 1 : 0;
  out->cam_grid_n = c->info.cg_last_n;
  out->cam_grid_builds = c->info.cg_builds;
  out->cam_grid_build_ms = c->info.cg_build_ms;
  out->tile_order_builds = c->info.perm_builds;
  out->tile_order_build_ms = c->info.perm_build_ms;
  out->upload_ms = c->info.upload_ms;
  out->launches = (uint64_t)c->timing.launches;
  const Scene &scn = c->scene;
  out->sphere_grids = scn.sg_ok ? scn.sg_grids : 0;
  out->sphere_grid_n = scn.sg_ok ? scn.sg_n : 0;
  out->sphere_grid_entries = scn.sg_ok ? (uint64_t)scn.sg_entries : 0;
  out->sphere_grid_build_ms = c->info.sg_build_ms;
  out->behind_grid = scn.ug_ok ? 1 : 0;
  out->behind_grid_last = c->info.ug_last ? 1 : 0;
  out->behind_grid_cells = scn.ug_ok ? (uint64_t)scn.ug.nx * (uint64_t)scn.ug.ny * (uint64_t)scn.ug.nz : 0;
  out->behind_grid_entries = scn.ug_ok ? (uint64_t)scn.ug_entries : 0;
  out->behind_grid_build_ms = c->info.ug_build_ms;
  out->bvh_build_ms = c->info.bvh_build_ms;
  out->light_grid_build_ms = c->info.lg_build_ms;
  out->scratch_bytes = (uint64_t)(c->gstack.bytes() + c->dq.bytes() + c->homes.bytes() + c->home_bits.bytes() +
                                  c->cg.bytes() + c->order.perm.bytes() + c->rays.bytes());
  out->shadow_line_bounded = c->scene.lg_off_free ? 1 : 0;
  out->reserved0 = 0;
  return RT_OK;
}

int rt_set_ray_table(rt_ctx *c, int mode, int64_t budget_bytes) {
  if (!c || mode < 0 || mode > 2) return RT_ERR_INVALID_ARG;
  c->rays.mode = mode;
  c->rays.budget = budget_bytes < 0 ? -1 : budget_bytes;
  return RT_OK;
}

int rt_get_ray_table_info(rt_ctx *c, rt_ray_table_info *out) {
  if (!c || !out) return RT_ERR_INVALID_ARG;
  *out = rt_ray_table_info{};
  out->builds = c->info.rays_builds;
  out->used_last = c->info.rays_last ? 1 : 0;
  out->bytes = (uint64_t)c->rays.bytes();
  out->build_ms = c->info.rays_build_ms;
  return RT_OK;
}

int rt_unpermute_rows(rt_ctx *c, const uint8_t *gathered, uint8_t *image, int W, int H, int band, int G, int R) {
  if (!c || !gathered || !image || W <= 0 || H <= 0 || band < 1 || G < 1 || R < 0) return RT_ERR_INVALID_ARG;
  const long long bands = (H + band - 1) / band;
  if ((long long)((bands + G - 1) / G) * band > R) return RT_ERR_INVALID_ARG;
  RT_TRY(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(unpermute_kernel, dim3(H), dim3(kBlock), 0, c->stream, gathered, image, W, H, band, G, R);
  RT_TRY(c, hipGetLastError());
  return RT_OK;
}

}  // extern "C"

// ---- rt_internal.h: the device group's view of a member's launches ---------
namespace {
// acc[q] += counter q of one launch, summed over its shards.  One wave; only
// the calling stream writes acc, so no atomics.
__global__ __launch_bounds__(64) void add_counts_kernel(const unsigned long long *__restrict__ counters,
                                                        unsigned long long *__restrict__ acc) {
  const int q = threadIdx.x;
  if (q >= kRtCountSlots) return;
  unsigned long long s = 0ull;
  for (int sh = 0; sh < kShards; sh++) s += counters[(size_t)sh * kShardStride + q];
  acc[q] += s;
}
}  // namespace

int rt_light_samples(const rt_ctx *c) { return c ? c->radiance.area_samples : 0; }
int rt_gloss_samples(const rt_ctx *c) { return c ? c->radiance.gloss_samples : 0; }

int rt_add_counts(rt_ctx *c, unsigned long long *acc) {
  static_assert(kRtCountSlots == kCounters, "rt_stats' counters");
  if (!c || !acc) return RT_ERR_INVALID_ARG;
  RT_TRY(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(add_counts_kernel, dim3(1), dim3(64), 0, c->stream, c->ctr.cur, acc);
  RT_TRY(c, hipGetLastError());
  return RT_OK;
}

int rt_launch_ms(rt_ctx *c, long long index, double *ms_out) {
  if (!c || !ms_out || index < 0 || index >= c->timing.launches ||
      c->timing.launches - index > LaunchTiming::kRing)
    return RT_ERR_INVALID_ARG;
  const int slot = (int)(index % LaunchTiming::kRing);
  RT_TRY(c, hipSetDevice(c->device));
  RT_TRY(c, hipEventSynchronize(c->timing.ev1[slot]));
  float ms = 0.f;
  RT_TRY(c, hipEventElapsedTime(&ms, c->timing.ev0[slot], c->timing.ev1[slot]));
  *ms_out = ms;
  return RT_OK;
}
