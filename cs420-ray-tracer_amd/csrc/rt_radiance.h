// Radiance queries (rt_trace_radiance): trace_ray (src/main.cpp:16-58) for rays
// the caller supplies -- path_kernel's levels (rt_paths.h: the closest hit, the
// whole of Scene::in_shadow per light, the reflection decision and its ray) with
// Scene::shade (scene.h:89-121) formed at every hit and the levels composited
// innermost first, as trace_wave unwinds them (rt_kernel.hip).  The Phong
// arithmetic is shade_hit's, operand for operand, so a camera ray's radiance is
// the render's RT_FB_F64X3 value of its pixel.  Included only by rt_kernel.hip,
// after rt_paths.h.
#pragma once

#include "rt_paths.h"

namespace rtk {

// The radiance query's own counter block: the path counters, then the channels
// RT_FB_RGB8 stored as 0 because they were negative.
enum { kRcNegative = kPathCounters, kRadianceCounters };
static_assert(kRadianceCounters <= kShardStride, "a shard holds the radiance counters");

struct RadianceArgs {
  PathArgs q;       // scene, rays, depth, region, walks and counters as a path launch's; verts / surf unused
  D3 amb;           // scene.h:91
  int fmt;          // RT_FB_*: the record written per ray
  void *out;        // [nrays] records, ray i at record i
  StackEnt *stack;  // [depth - 1][sstride]: the reflection stack of the launch's lane slots
  unsigned sstride; // lane slots of the launch: gridDim.x * 64
  int park_off;     // byte offset in dynamic LDS of the wave's parked colours, D3[64]
};

// The resolving launch (rt_trace_radiance_resolve): q.nrays counts PIXELS, pixel p's samples are
// the rays p*samples .. p*samples + samples - 1, and record p is the pixel's.  Everything here is
// wave-uniform and read from the kernel arguments.
enum { kResolveSingle = 0, kResolveBox, kResolveWeighted };
struct ResolveArgs {
  RadianceArgs r;
  int samples;  // 1..RT_MAX_SAMPLES
  int mode;     // kResolveSingle: the colour itself; kResolveBox: (0 + c_0 + ...) * inv; kResolveWeighted: 0 + c_0*w_0 + ...
  double inv;   // 1.0 / samples, formed once on the host
  double w[RT_MAX_SAMPLES];
};
static_assert(offsetof(ResolveArgs, r) == 0, "radiance_kernel reads a ResolveArgs' launch through its first member");

// The fused launch (rt_render_samples_async): a resolving launch whose lanes form their sample rays
// themselves, camera_sample_rays_kernel's arithmetic (rt_query.h) in place of its records.  r.q.nrays
// counts the pixels of the REAL output rows of `rows` (the padding rows are a suffix, which the host
// zeroes), r.q.rays is unused.  All of it is wave-uniform and read from the kernel arguments.  A
// ResolveArgs by inheritance: the kernel's `ka.samples`, `ka.mode`, `ka.w` and its cast to RadianceArgs
// are the same text for both resolving forms.
struct GenArgs : ResolveArgs {
  Cam cam;
  int W, H;
  Rows rows;
  double xy[2 * RT_MAX_SAMPLES];  // (ox_s, oy_s)
};
static_assert(sizeof(GenArgs) <= 4096, "the kernel argument segment of a launch");

// The fused launch through a thin lens (rt_render_lens_samples_async): GenArgs and, per sample, the
// point of the lens its ray leaves from, in scene units along the camera's right and up, and per launch
// the distance along forward of the plane that stays sharp.  Wave-uniform, read from the kernel arguments.
struct LensArgs : GenArgs {
  double focus;
  double lens[2 * RT_MAX_SAMPLES];  // (lx_s, ly_s)
};
static_assert(sizeof(LensArgs) <= 4096, "the kernel argument segment of a launch");

// A resolving launch under area lights (rt_set_light_samples): any of the three argument blocks above
// and, behind it, the context's table of shifted light records, [samples][q.nl] of them: record
// s * q.nl + l is light l as sample s sees it.  The table lives in device memory -- 64 samples of 64
// lights are 192 KiB, and even one [64][3] block more would push LensArgs past the argument segment --
// and only its address travels here.  Appended, not a member of ResolveArgs: the blocks of the launches
// without a table keep their layout, and so their kernels every operand offset.
template <class Base>
struct AreaArgs : Base {
  const LightD *area;
};
static_assert(sizeof(AreaArgs<LensArgs>) <= 4096, "the kernel argument segment of a launch");

// A resolving launch with glossy reflections (rt_set_gloss_samples): any of the blocks above, AreaArgs among
// them, and behind it the context's gloss table, [samples][bounces] points g, and the spheres' roughness:
// sample s's reflection ray off sphere i at level k < bounces leaves along rd + g[s * bounces + k] *
// rough[i] where that stays on rd's side of the surface.  Both live in device memory (64 samples of 63
// bounces are 94.5 KiB) and only their addresses travel here, appended for AreaArgs' reason: the blocks of
// the launches without a table keep their layout.
template <class Base>
struct GlossArgs : Base {
  const D3 *gloss;
  const double *rough;
  int bounces;
};
static_assert(sizeof(GlossArgs<AreaArgs<LensArgs>>) <= 4096, "the kernel argument segment of a launch");

template <bool kResolve, bool kGen, bool kLens>
struct RadianceLaunch {
  using Args = RadianceArgs;
};
template <>
struct RadianceLaunch<true, false, false> {
  using Args = ResolveArgs;
};
template <>
struct RadianceLaunch<true, true, false> {
  using Args = GenArgs;
};
template <>
struct RadianceLaunch<true, true, true> {
  using Args = LensArgs;
};
template <class Args, bool kArea>
struct AreaLaunch {
  using type = Args;
};
template <class Args>
struct AreaLaunch<Args, true> {
  using type = AreaArgs<Args>;
};
template <class Args, bool kGloss>
struct GlossLaunch {
  using type = Args;
};
template <class Args>
struct GlossLaunch<Args, true> {
  using type = GlossArgs<Args>;
};

// path_kernel's shape: one wave per workgroup, one ray per lane, grid-stride
// over the batch, a wave-uniform level loop in which an ended lane (or one past
// the end of the batch) stays in every sweep with act = false, and the same
// fast / slow split per segment and per shadow ray.  What it adds:
//  * col, Scene::shade's accumulator: per unshadowed light the Phong terms of
//    shade_hit's light loop.  The wide form (hit lanes at most half the wave)
//    has the helper lane compute the term of its (hit lane, light) pair from the
//    owner's hit point, normal, view direction and sphere, and the owner add
//    its lights' terms in file order: the same bits as the lane-per-ray loop.
//  * the reflection stack.  A level that spawns stores {shade*(1-refl), refl}
//    at stack[slot + level * sstride], slot = blockIdx.x * 64 + lane: a slot
//    belongs to a lane of the launch, not to a ray, and is reused on every
//    grid-stride trip (a lane reads only what it wrote on this trip).
//  * the parked colour.  The colour of the level at which a lane's chain ends
//    (sky, shade, or shade*(1-refl) with no depth left) waits in LDS, 24 bytes
//    per lane behind the walks' stacks, while the wave's other lanes go on, as
//    trace_wave's kPark does: held in registers it cost 44 spilled VGPRs, not 28.
//  * the store: one record per lane, consecutive lanes to consecutive records.
// The format is switched at the store, after the level loop: it holds no
// register where the pressure is, and one instantiation serves the three.
// amdgpu_waves_per_eu(3), as path_kernel: left alone the allocator takes 201
// VGPRs and no scratch, two waves per SIMD; held to the 168 of three waves it
// spills 28 VGPRs (112 bytes of scratch per lane) and takes 14-20 % less time
// ("Radiance").
//
// kResolve (rt_trace_radiance_resolve, DESIGN.md section 5b, "Samples"): one lane per PIXEL, and a
// wave-uniform loop over the pixel's samples around the level loop, as trace_tile loops its samples
// around trace_wave: the wave traces sample s of 64 consecutive pixels together, a sample's chain
// unwinds before the next begins (the lane's stack slots are reused), and the samples are added in
// order by construction.  The accumulator waits in LDS right behind the parked colours (park[64 +
// lane]: the same address register, another offset), for the same reason; it is read and written
// once per sample.  With kResolve false the do-while's condition is a constant and every `if
// constexpr` is gone: rt_trace_radiance's instantiation compiles to the instructions it had before
// the template.  Two details keep it so (each was tried the other way and moved the code): the
// launch is read through a cast, not a helper returning a reference; a chain's colour `res` keeps
// its scope and is copied to `pix` for the store.
//
// kGen (rt_render_samples_async, DESIGN.md section 5b, "Samples, fused and on a group"): the resolving
// form with sample s's ray formed in the lane from its pixel, the camera and the sample's offsets, all
// read wave-uniformly from the kernel arguments, instead of loaded -- camera_sample_rays_kernel's
// direction, normalised once there and once more here as the loaded one is.  Pixel p is column p % W of
// output row p / W of the launch's rt_rows; the division is written once per trip and (x, j) held across
// the samples as two ints (written inside the sample loop it compiles to the same instructions and the
// same resource summary: 53 spilled VGPRs either way).  Everything after the ray is kResolve's.  With
// kGen false nothing of it is emitted: the two loading forms' assembly is the parent's, line for line.
//
// kLens (rt_render_lens_samples_async, DESIGN.md section 5b, "Samples through a lens"): kGen with sample
// s's ray leaving the lens point P + right*lx_s + up*ly_s towards the point of the focal plane the
// pinhole ray meets, camera_lens_rays_kernel's arithmetic (rt_query.h).  The origin becomes a per-lane
// value; the lens points and the focus distance are read wave-uniformly as the offsets are.  Only the ray
// formation differs, and with kLens false none of it is emitted.
//
// kArea (rt_set_light_samples, DESIGN.md section 5b, "Samples under area lights"): any resolving form
// with sample s's light records read from row s of the context's table, ka.area + s * q.nl, instead of
// q.lights.  The row is chosen once per sample, outside the level loop, so the whole chain of the sample
// -- every level's to_light, dist, ldir, shadow ray and Phong terms -- sees one position per light.  s and
// q.nl are wave-uniform, so the base is: the lane-per-ray loop's L stays a scalar load, the wide form's
// helper lanes load lights[lh] per lane as before.  The records were formed on the host; the kernel adds
// nothing.  The sweeps take a light anywhere: make_bound's margins are relative to its own P and the
// lanes' distance from it, the walks' to the origin (in R, path_in_region) and to dist, and none to the
// scene bound, so a row whose lights lie outside the uploaded bound changes no result and no counter
// rule.  With kArea false none of it is emitted and the argument block is the form's own.
//
// kGloss (rt_set_gloss_samples, DESIGN.md section 5b, "Samples with glossy reflections"): any resolving
// form, with or without kArea, whose reflection ray off sphere hi at level k < ka.bounces is bent: the
// mirror direction rd plus sample s's point of the table for that level, scaled by the sphere's roughness,
// where the sum stays on rd's side of the surface (the signs of the two dot products with the normal agree
// and neither is zero or a NaN); otherwise, and for roughness 0 and every level from ka.bounces on, rd as
// before.  s, k and ka.bounces are wave-uniform: the level test is a scalar branch and the point a scalar
// load; the roughness is loaded per lane by the lanes that spawn (hi is a sphere only for a hit, and the
// array is empty for a scene without spheres).  The spawn decision, the origin, the stack and every
// counter are untouched.  With kGloss false none of it is emitted and the argument block is the form's own.
template <bool kResolve, bool kGen = false, bool kLens = false, bool kArea = false, bool kGloss = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) void radiance_kernel(
    const typename GlossLaunch<
        typename AreaLaunch<typename RadianceLaunch<kResolve, kGen, kLens>::Args, kArea>::type, kGloss>::type ka) {
  static_assert(kResolve || !kGen, "the generating form resolves");
  static_assert(kGen || !kLens, "the lens form generates");
  static_assert(kResolve || !kArea, "the light table is indexed by the sample");
  static_assert(kResolve || !kGloss, "the gloss table is indexed by the sample");
  const RadianceArgs &a = reinterpret_cast<const RadianceArgs &>(ka);  // ResolveArgs::r, at offset 0
  const PathArgs &q = a.q;
  const int lane = (int)(threadIdx.x & 63);
  const long long n = q.nrays, step = (long long)gridDim.x * 64;
  const unsigned slot = blockIdx.x * 64u + (unsigned)lane;
  D3 *park = reinterpret_cast<D3 *>(rt_dyn_lds + a.park_off);
  Work work;
  unsigned c_rays = 0, c_seg = 0, c_hits = 0, c_shadow = 0, c_slow = 0, c_neg = 0;
  const double2 *__restrict__ src = reinterpret_cast<const double2 *>(q.rays);
  for (long long base = (long long)blockIdx.x * 64; base < n; base += step) {
    const long long i = base + lane;
    const bool act = i < n;
    const long long ld = act ? i : n - 1;
    int nsamp = 1;
    if constexpr (kResolve) {
      nsamp = ka.samples;
      if (ka.mode != kResolveSingle) park[64 + lane] = mk(0.0, 0.0, 0.0);
    }
    [[maybe_unused]] int gx = 0, gj = 0;  // kGen: the pixel's column and reference row (main.cpp:74)
    if constexpr (kGen) {
      const int p = (int)ld, k = p / ka.W;  // ld < nrays <= 2^31-1
      const Rows &rw = ka.rows;
      const long long y =
          (long long)(k / rw.band) * rw.band * rw.stride + (long long)rw.first * rw.band + (k % rw.band);
      gx = p - k * ka.W;
      gj = ka.H - 1 - (int)y;  // a real row: y < H
    }
    D3 pix;
    int s = 0;
    do {  // the pixel's samples; the body keeps the level loop's indentation
    D3 o, d;
    if constexpr (kLens) {
      const D3 dir0 = camera_dir(ka.cam, (double)gx + ka.xy[2 * s], (double)gj + ka.xy[2 * s + 1], ka.W, ka.H);
      const D3 dir = lens_ray(ka.cam, dir0, ka.lens[2 * s], ka.lens[2 * s + 1], ka.focus, o);  // the record's
      d = normalized(dir);  // Ray(o, d) on the record's direction: once more
    } else if constexpr (kGen) {
      const D3 dir = normalized(
          camera_dir(ka.cam, (double)gx + ka.xy[2 * s], (double)gj + ka.xy[2 * s + 1], ka.W, ka.H));  // the record's
      o = mk(ka.cam.px, ka.cam.py, ka.cam.pz);
      d = normalized(dir);  // Ray(o, d) on the record's direction: once more
    } else {
      const long long ri = kResolve ? ld * nsamp + s : ld;
      const double2 r0 = src[ri * 4 + 0], r1 = src[ri * 4 + 1], r2 = src[ri * 4 + 2];
      o = mk(r0.x, r0.y, r1.x);
      d = normalized(mk(r1.y, r2.x, r2.y));  // Ray(o, d), ray.h:12: once
    }
    const LightD *lights = q.lights;  // kArea: the sample's row of the table, for the whole of its chain
    if constexpr (kArea) lights = ka.area + (size_t)s * (size_t)q.nl;
    bool alive = act;
    int key = -1;  // the sphere the ray leaves: groups the sweeps' lanes, changes no result
    int lev = 0;   // stack entries this lane holds
    for (int k = 0; k < q.depth && __ballot(alive) != 0; ++k) {
      // ---- the closest hit of this level's ray (scene.h:41-61), as path_kernel
      const bool fast = alive && q.accel != 0 && path_in_region(q, o, d);
      const bool slow = alive && !fast;
      double t_fast = kInf, t_slow = kInf;
      int s_fast = -1, s_slow = -1;
      if (__ballot(fast) != 0) s_fast = sweep_closest<true, false>(q.geo, q.rad, q.n, fast, o, d, key, q.bv, t_fast, work);
      if (__ballot(slow) != 0) s_slow = sweep_closest<false>(q.geo, q.rad, q.n, slow, o, d, key, q.bv, t_slow, work);
      const int sphere = alive ? (fast ? s_fast : s_slow) : -1;
      const double t = alive ? (fast ? t_fast : t_slow) : kInf;
      const bool hit = alive && sphere >= 0;
      c_seg += alive ? 1u : 0u;
      c_slow += slow ? 1u : 0u;
      c_hits += hit ? 1u : 0u;
      if (alive && !hit) {  // sky, main.cpp:26-30 (shade_hit)
        const double st = 0.5 * (d.y + 1.0);
        park[lane] = add(scale(mk(1.0, 1.0, 1.0), 1.0 - st), scale(mk(0.5, 0.7, 1.0), st));
      }
      const int hi = RT_CK(kCkSphere, hit ? sphere : 0, q.n > 0 ? q.n : 1);
      const D3 hp = add(o, scale(d, t));  // main.cpp:32
      D3 col;
      {
        const SphMat m0 = q.mat[hi];
        col = mul(a.amb, mk(m0.cr, m0.cg, m0.cb));  // scene.h:91
      }
      D3 nrm = mk(0.0, 0.0, 0.0), view = nrm;
      if (hit) {
        const SphGeo sg = q.geo[hi];
        nrm = normalized(sub(hp, mk(sg.cx, sg.cy, sg.cz)));  // sphere.h:62-64
        view = normalized(sub(o, hp));                       // main.cpp:38
      }
      // ---- Scene::shade's light loop (scene.h:94-120): per light in file order the whole of
      // in_shadow (path_kernel's query), then, if lit, the Phong terms with the same ldir
      auto in_shadow = [&](bool need, D3 hq, D3 lp, D3 ldir, double dist, int gkey, bool one_light) {
        const D3 so = add(hq, scale(ldir, kEps));
        const D3 sd = renormalized(ldir);  // Ray() normalises the unit direction again
        const bool sfast = need && q.accel != 0 && path_in_region(q, so, sd);
        const bool sslow = need && !sfast;  // a light at the hit point among them: a NaN direction, never shadowed
        bool occ = false;
        const unsigned long long fm = __ballot(sfast);
        if (fm != 0) {
          const int f0 = __builtin_ctzll(fm);
          const D3 P = one_light ? lp : mk(lane_bcast(so.x, f0), lane_bcast(so.y, f0), lane_bcast(so.z, f0));
          occ = sweep_shadow<true>(q.geo, q.rad, q.n, sfast, so, sd, P, gkey, dist, q.bv, work);
        }
        if (__ballot(sslow) != 0) {
          const bool os = sweep_shadow<false>(q.geo, q.rad, q.n, sslow, so, sd, so, gkey, dist, q.bv, work);
          occ = sfast ? occ : os;
        }
        c_slow += sslow ? 1u : 0u;
        return need && occ;
      };
      // one light's specular + diffuse for a lit point: shade_hit's terms, same operands and order
      auto phong = [&](const SphMat &m, const LightD &L, D3 nq, D3 vq, D3 ldir) {
        const double ndl = max0(dot(nq, ldir));
        const D3 diffuse = scale(scale(mk(m.cr, m.cg, m.cb), 1.0 - m.refl), ndl);
        const D3 nl2 = scale(ldir, -1.0);
        const D3 rdir = sub(nl2, scale(scale(nq, 2.0), dot(nl2, nq)));  // reflect(), vec3.h:31-33
        const double rdv = max0(dot(rdir, vq));
        double spec = 0.0;  // pow(+0, y > 0) is +0 exactly (C99 F.10.4.4)
        int ipow = 0;
        if (!(rdv == 0.0 && m.shin > 0.0))
          spec = int_pow_ok(rdv, m.shin, ipow) ? int_pow(rdv, ipow) : pow_call(rdv, m.shin);
        const D3 specular = scale(scale(mk(L.cr, L.cg, L.cb), kSpec), spec);
        return add(specular, diffuse);
      };
      const unsigned long long hm = __ballot(hit);
      const int nh = __popcll(hm);
      const int lpp = nh ? (64 / nh < q.nl ? 64 / nh : q.nl) : 0;  // lights per pass
      if (q.nl >= 2 && lpp >= 2) {  // wave-uniform: the wide form, as shade_hit's kWide branch
        const int rank = (int)__popcll(hm & ((1ull << lane) - 1ull));
        for (int l0 = 0; l0 < q.nl; l0 += lpp) {  // lights l0 .. l0 + cnt - 1 in this pass
          const int cnt = q.nl - l0 < lpp ? q.nl - l0 : lpp;
          const bool helper = lane < nh * cnt;
          const int r = helper ? lane / cnt : 0, lh = l0 + (helper ? lane - r * cnt : 0);
          const int own = nth_set_bit(hm, r);  // the owner: the r-th hit lane
          const D3 hq = mk(__shfl(hp.x, own, 64), __shfl(hp.y, own, 64), __shfl(hp.z, own, 64));
          const int hq_i = RT_CK(kCkSphere, __shfl(hi, own, 64), q.n > 0 ? q.n : 1);
          const LightD L = lights[lh];
          const D3 lp = mk(L.px, L.py, L.pz);
          const D3 to_light = sub(lp, hq);
          const double dist = length(to_light);
          const D3 ldir = normalized(to_light);
          const bool occ = in_shadow(helper, hq, lp, ldir, dist, lh, false);  // lanes of one light sweep together
          // the owner's normal and view direction, passed over after the sweeps (by every lane: a
          // shuffle reads nothing from a lane that is switched off)
          const D3 nq = mk(__shfl(nrm.x, own, 64), __shfl(nrm.y, own, 64), __shfl(nrm.z, own, 64));
          const D3 vq = mk(__shfl(view.x, own, 64), __shfl(view.y, own, 64), __shfl(view.z, own, 64));
          D3 term = mk(0.0, 0.0, 0.0);
          const bool lit = helper && !occ;
          if (lit) term = phong(q.mat[hq_i], L, nq, vq, ldir);
          // each hit lane adds this pass's lights' terms in file order (scene.h:117)
          const unsigned long long litm = __ballot(lit);
          for (int l = 0; l < cnt; ++l) {
            const int sl = hit ? rank * cnt + l : 0;
            const D3 tl = mk(__shfl(term.x, sl, 64), __shfl(term.y, sl, 64), __shfl(term.z, sl, 64));
            if (hit && ((litm >> sl) & 1ull)) col = add(tl, col);
          }
        }
      } else if (hm != 0) {
        for (int l = 0; l < q.nl; ++l) {
          const LightD L = lights[l];
          const D3 lp = mk(L.px, L.py, L.pz);
          const D3 to_light = sub(lp, hp);
          const double dist = length(to_light);
          const D3 ldir = normalized(to_light);
          const bool occ = in_shadow(hit, hp, lp, ldir, dist, hi, true);
          if (hit && !occ) col = add(phong(q.mat[hi], L, nrm, view, ldir), col);  // scene.h:117
        }
      }
      c_shadow += hit ? (unsigned)q.nl : 0u;
      // ---- the reflection decision (main.cpp:43-55, shade_hit) and this level's stack entry; the
      // material is read again here rather than held across the light loop
      bool spawn = false;
      if (hit) {
        const double refl = q.mat[hi].refl;
        if (refl > 0.0) {
          const double w = 1.0 - refl;
          const D3 A = mk(col.x * w, col.y * w, col.z * w);
          spawn = q.depth - (k + 1) >= 1;
          if (spawn) {
            a.stack[RT_CK(kCkStack, slot + (unsigned)lev * a.sstride, (long long)(q.depth - 1) * a.sstride)] =
                StackEnt{A.x, A.y, A.z, refl};
            ++lev;
          } else {
            park[lane] = A;  // with no depth left trace_ray(depth 0) is black: A + (0,0,0)*refl == A
          }
        } else {
          park[lane] = col;
        }
      }
      // the reflection ray (main.cpp:45-48), shade_hit's operand order; formed by every lane, used
      // by the lanes that spawn one (the others' chains have ended)
      const D3 rd = sub(d, scale(scale(nrm, 2.0), dot(d, nrm)));
      o = add(hp, scale(nrm, kEps));
      if constexpr (kGloss) {
        D3 chosen = rd;
        if (k < ka.bounces) {  // wave-uniform; beyond the table every bounce is a mirror
          // read through the constant address space: the table is read-only for the whole launch and the
          // address is wave-uniform, which makes the point two scalar loads (a plain load stays a vector one,
          // the stack's stores ahead of it in the loop keep the compiler from proving the table invariant)
          typedef const __attribute__((address_space(4))) double *ConstDoubles;
          const ConstDoubles gp = (ConstDoubles)(ka.gloss + ((size_t)s * (size_t)ka.bounces + (size_t)k));
          const D3 g = mk(gp[0], gp[1], gp[2]);
          const double rough = spawn ? ka.rough[hi] : 0.0;
          const D3 rp = add(rd, scale(g, rough));  // the product rounded, then the sum
          // refused on the wrong side of the surface, in the tangent plane, and for a NaN
          if (rough != 0.0 && dot(rp, nrm) * dot(rd, nrm) > 0.0) chosen = rp;
        }
        d = renormalized(chosen);
      } else {
        d = renormalized(rd);
      }
      key = spawn ? hi : key;
      alive = spawn;
    }
    D3 res = mk(0.0, 0.0, 0.0);
    if (act) res = park[lane];
    while (lev > 0) {  // unwind: shade*(1-refl) + reflected*refl, innermost first (trace_wave)
      --lev;
      const StackEnt e = a.stack[RT_CK(kCkStack, slot + (unsigned)lev * a.sstride, (long long)(q.depth - 1) * a.sstride)];
      res = mk(e.ax + res.x * e.refl, e.ay + res.y * e.refl, e.az + res.z * e.refl);
    }
    c_rays += act ? 1u : 0u;
    if constexpr (kResolve) {
      if (ka.mode != kResolveSingle) {  // acc = acc + c_s, or acc + c_s * w_s: the product rounded, then the sum
        D3 *accp = park + 64 + lane;
        const D3 v = ka.mode == kResolveWeighted ? scale(res, ka.w[s]) : res;
        *accp = add(*accp, v);
      }
    }
    pix = res;
    } while (kResolve && ++s < nsamp);  // constant false without kResolve: no loop is emitted
    if constexpr (kResolve) {
      if (ka.mode != kResolveSingle) {
        pix = park[64 + lane];
        if (ka.mode == kResolveBox) pix = scale(pix, ka.inv);  // trace_tile's scale(acc, 0.25) for four samples
      }
    }
    // ---- the record of ray i (kResolve: of pixel i)
    if (a.fmt == RT_FB_RGB8) {
      // quantised as write_ppm (main.cpp:85-87): a negative channel is stored as 0 and counted; a NaN
      // is 1.0 to std::min(1.0, c), so 255 and not counted.  A whole wave's 64 records are 192 contiguous bytes from a dword boundary
      // (base is a multiple of 64): lanes 0-47 store them as dwords assembled with two shuffles, as
      // trace_tile's rows are; the batch's last, partial wave stores bytes.
      unsigned v = 0;  // r | g << 8 | b << 16
      if (act) {
        const int q0 = quantize(pix.x), q1 = quantize(pix.y), q2 = quantize(pix.z);
        c_neg += (unsigned)((q0 < 0) + (q1 < 0) + (q2 < 0));
        v = (unsigned)(q0 < 0 ? 0 : q0) | (unsigned)(q1 < 0 ? 0 : q1) << 8 | (unsigned)(q2 < 0 ? 0 : q2) << 16;
      }
      uint8_t *rec = static_cast<uint8_t *>(a.out) + (size_t)base * 3;
      const bool packed = __ballot(act) == ~0ull && (reinterpret_cast<uintptr_t>(rec) & 3u) == 0;
      const int p0 = (4 * lane) / 3;  // dword `lane` holds bytes 4 lane .. 4 lane + 3: records p0, p0 + 1
      const unsigned v0 = __shfl(v, p0 < 63 ? p0 : 63, 64), v1 = __shfl(v, p0 + 1 < 63 ? p0 + 1 : 63, 64);
      if (packed) {
        if (lane < 48) {
          const unsigned long long both = (unsigned long long)v0 | (unsigned long long)v1 << 24;
          reinterpret_cast<unsigned *>(rec)[lane] = (unsigned)(both >> (8 * (4 * lane - 3 * p0)));
        }
      } else if (act) {
        uint8_t *px = rec + lane * 3;
        px[0] = (uint8_t)v;
        px[1] = (uint8_t)(v >> 8);
        px[2] = (uint8_t)(v >> 16);
      }
    } else if (act) {
      if (a.fmt == RT_FB_F64X3) {
        double *f = static_cast<double *>(a.out) + (size_t)i * 3;
        f[0] = pix.x;
        f[1] = pix.y;
        f[2] = pix.z;
      } else {  // RT_FB_F32X3, converted as trace_tile's store converts
        float *f = static_cast<float *>(a.out) + (size_t)i * 3;
        f[0] = (float)pix.x;
        f[1] = (float)pix.y;
        f[2] = (float)pix.z;
      }
    }
  }
  const unsigned long long s_rays = wave_sum(c_rays), s_seg = wave_sum(c_seg), s_hits = wave_sum(c_hits);
  const unsigned long long s_shadow = wave_sum(c_shadow), s_slow = wave_sum(c_slow), s_neg = wave_sum(c_neg);
  const unsigned long long s_exact = wave_sum64(work.exact), s_cull = wave_sum64(work.cull);
  if (lane == 0) {
    unsigned long long *cs = counter_shard(q.counters);
    atomicAdd(cs + kPcRays, s_rays);
    atomicAdd(cs + kPcSegments, s_seg);
    atomicAdd(cs + kPcHits, s_hits);
    atomicAdd(cs + kPcShadow, s_shadow);
    atomicAdd(cs + kPcExact, s_exact);
    atomicAdd(cs + kPcCull, s_cull);
    atomicAdd(cs + kPcUnaccel, s_slow);
    atomicAdd(cs + kRcNegative, s_neg);
  }
}

}  // namespace rtk
