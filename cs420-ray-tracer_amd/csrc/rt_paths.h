// Path queries (rt_trace_paths): the geometric skeleton of trace_ray
// (src/main.cpp:16-58) for rays the caller supplies -- per reflection level the
// closest hit (scene.h:41-61), per light the whole of Scene::in_shadow
// (scene.h:65-86) as one bit, and the reflection decision with its ray
// (main.cpp:43-48) -- one ray per lane, through the render kernels' own sweeps
// and walks (rt_device.h sweep_closest / sweep_shadow) and their normalisation
// helpers, so every bit is the render's.  No colour is formed.  Included only
// by rt_kernel.hip, after rt_query.h.
#pragma once

#include "rt_device.h"

namespace rtk {

static_assert(sizeof(rt_vertex) == 32 && sizeof(rt_surface) == 96, "rt_vertex / rt_surface layout (rt_hip.h)");
static_assert(RT_PATH_MAX_LIGHTS == 64, "rt_vertex.shadowed has one bit per light");

// The path query's own counter block, sharded like the render counters.
enum { kPcRays = 0, kPcSegments, kPcHits, kPcShadow, kPcExact, kPcCull, kPcUnaccel, kPathCounters };
static_assert(kPathCounters <= kShardStride, "a shard holds the path counters");

struct PathArgs {
  const SphGeo *geo;
  const double *rad;
  const SphMat *mat;
  const LightD *lights;
  int n, nl;    // spheres, lights (nl <= RT_PATH_MAX_LIGHTS)
  int nrays;    // >= 1
  int depth;    // 1..RT_MAX_DEPTH
  int accel;    // 0: every query tests every sphere (rt_set_culling(ctx, 0))
  const rt_ray *rays;
  rt_vertex *verts;    // [depth][nrays]
  rt_surface *surf;    // [depth][nrays]; unused by path_kernel<false>
  double rlo[3], rhi[3];  // the query region R (QueryArgs)
  BvhArgs bv;
  unsigned long long *counters;
};

// rt_vertex as two 16-byte words: (t, sphere | flags << 32) and (shadowed, reserved = 0).
__device__ __forceinline__ double2 vertex_head(double t, int sphere, int flags) {
  const unsigned long long w = (unsigned long long)(unsigned)sphere | (unsigned long long)(unsigned)flags << 32;
  return make_double2(t, __longlong_as_double((long long)w));
}
__device__ __forceinline__ double2 vertex_tail(unsigned long long shadowed) {
  return make_double2(__longlong_as_double((long long)shadowed), 0.0);
}

// Position of the k-th set bit of m (rt_kernel.hip, beside shade_hit's wide loop).
__device__ __forceinline__ int nth_set_bit(unsigned long long m, int k);

// The lanes whose query may take the culled sweep and the walks: origin in R
// (false for a NaN component) and a finite normalised direction (query_kernel).
__device__ __forceinline__ bool path_in_region(const PathArgs &a, D3 o, D3 d) {
  const bool in_r = o.x >= a.rlo[0] && o.x <= a.rhi[0] && o.y >= a.rlo[1] && o.y <= a.rhi[1] && o.z >= a.rlo[2] &&
                    o.z <= a.rhi[2];
  const bool finite_d = __builtin_fabs(d.x) <= 2.0 && __builtin_fabs(d.y) <= 2.0 && __builtin_fabs(d.z) <= 2.0;
  return in_r && finite_d;
}

// One wave per workgroup, one ray per lane, grid-stride over the batch, as
// query_kernel.  The level loop is wave-uniform: it runs while any lane's path
// is alive, and a lane whose path has ended (or that lies past the end of the
// batch) stays in every sweep with act = false -- the sweeps' wave reductions
// need all 64 lanes.  Per level and per light the lanes split into those that
// take the culled sweep and the walks and those that take the every-sphere
// sweep: a reflection origin or a shadow origin may leave R although the
// level-0 origin was inside.  Level-major output: lane i writes record
// k * nrays + i, so consecutive lanes write consecutive records.
// amdgpu_waves_per_eu(3): without it the allocator stops at 169 VGPRs, one over
// what three waves per SIMD allow; with it 168 and still no scratch, and the
// latency-bound walks run 12-25 % faster ("Paths").
template <bool kSurf>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) void path_kernel(const PathArgs a) {
  const int lane = (int)(threadIdx.x & 63);
  const long long n = a.nrays, step = (long long)gridDim.x * 64;
  Work work;
  unsigned c_rays = 0, c_seg = 0, c_hits = 0, c_shadow = 0, c_slow = 0;
  const double2 *__restrict__ src = reinterpret_cast<const double2 *>(a.rays);
  double2 *__restrict__ vdst = reinterpret_cast<double2 *>(a.verts);
  double2 *__restrict__ sdst = reinterpret_cast<double2 *>(a.surf);
  for (long long base = (long long)blockIdx.x * 64; base < n; base += step) {
    const long long i = base + lane;
    const bool act = i < n;
    const long long ld = act ? i : n - 1;
    const double2 r0 = src[ld * 4 + 0], r1 = src[ld * 4 + 1], r2 = src[ld * 4 + 2];
    D3 o = mk(r0.x, r0.y, r1.x);
    D3 d = normalized(mk(r1.y, r2.x, r2.y));  // Ray(o, d), ray.h:12: once
    bool alive = act;
    int key = -1;  // the sphere the ray leaves: groups the sweeps' lanes, changes no result
    int k = 0;
    for (; k < a.depth && __ballot(alive) != 0; ++k) {
      // ---- the closest hit of this level's ray (scene.h:41-61), as query_kernel's closest mode
      const bool fast = alive && a.accel != 0 && path_in_region(a, o, d);
      const bool slow = alive && !fast;
      double t_fast = kInf, t_slow = kInf;
      int s_fast = -1, s_slow = -1;
      if (__ballot(fast) != 0) s_fast = sweep_closest<true, false>(a.geo, a.rad, a.n, fast, o, d, key, a.bv, t_fast, work);
      if (__ballot(slow) != 0) s_slow = sweep_closest<false>(a.geo, a.rad, a.n, slow, o, d, key, a.bv, t_slow, work);
      const int sphere = alive ? (fast ? s_fast : s_slow) : -1;
      const double t = alive ? (fast ? t_fast : t_slow) : kInf;
      const bool hit = alive && sphere >= 0;
      c_seg += alive ? 1u : 0u;
      c_slow += slow ? 1u : 0u;
      c_hits += hit ? 1u : 0u;
      const int hi = RT_CK(kCkSphere, hit ? sphere : 0, a.n > 0 ? a.n : 1);
      const D3 hp = add(o, scale(d, t));  // main.cpp:32
      D3 nrm = mk(0.0, 0.0, 0.0);
      if (hit) {
        const SphGeo sg = a.geo[hi];
        nrm = normalized(sub(hp, mk(sg.cx, sg.cy, sg.cz)));  // sphere.h:62-64
      }
      // the reflection decision (main.cpp:43, :17) and the record's first half are settled here, so
      // that t and the flags need no register across the light loop
      const bool spawn = hit && a.depth - (k + 1) >= 1 && a.mat[hi].refl > 0.0;
      const long long rec = (long long)k * n + i;
      if (act)
        vdst[rec * 2] = vertex_head(t, sphere, alive ? (RT_VERTEX_TRACED | (spawn ? RT_VERTEX_REFLECTS : 0)) : 0);
      if constexpr (kSurf) {
        // the surface record of a traced level; a miss is its direction and zeros
        if (alive) {
          const D3 z = mk(0.0, 0.0, 0.0);
          const D3 hq = hit ? hp : z;
          const D3 view = hit ? normalized(sub(o, hp)) : z;  // main.cpp:38
          double2 *s = sdst + rec * 6;
          s[0] = make_double2(d.x, d.y);
          s[1] = make_double2(d.z, hq.x);
          s[2] = make_double2(hq.y, hq.z);
          s[3] = make_double2(nrm.x, nrm.y);
          s[4] = make_double2(nrm.z, view.x);
          s[5] = make_double2(view.y, view.z);
        }
      }
      // ---- Scene::in_shadow per light in file order (scene.h:65-86): bit l of the mask.
      // A wave whose hit lanes are at most half of it spreads the lights over the lanes, as shade_hit's
      // wide loop does: in passes of lpp = 64 / hits lights, lane j asks light l0 + j % cnt for the
      // (j / cnt)-th hit lane, with that lane's hit point and the operations of the loop below, and each
      // hit lane then collects its lights' bits.  The same bits in ceil(lights / lpp) sweeps instead of
      // one per light: the deep levels, where few paths of a wave are still alive, are mostly these waves.
      unsigned long long shadowed = 0ull;
      const unsigned long long hm = __ballot(hit);
      const int nh = __popcll(hm);
      const int lpp = nh ? (64 / nh < a.nl ? 64 / nh : a.nl) : 0;  // lights per pass
      auto in_shadow = [&](bool need, D3 hq, int lh, int gkey, bool one_light) {
        const LightD L = a.lights[lh];
        const D3 lp = mk(L.px, L.py, L.pz);
        const D3 to_light = sub(lp, hq);
        const double dist = length(to_light);
        const D3 ldir = normalized(to_light);
        const D3 so = add(hq, scale(ldir, kEps));
        const D3 sd = renormalized(ldir);  // Ray() normalises the unit direction again
        const bool sfast = need && a.accel != 0 && path_in_region(a, so, sd);
        const bool sslow = need && !sfast;  // a light at the hit point among them: a NaN direction, never shadowed
        bool occ = false;
        const unsigned long long fm = __ballot(sfast);
        if (fm != 0) {
          // the bound's reference point (wave-uniform; any point keeps the cull conservative): the
          // light when every lane asks the same one, as the render does, else the first lane's origin
          const int f0 = __builtin_ctzll(fm);
          const D3 P = one_light ? lp : mk(lane_bcast(so.x, f0), lane_bcast(so.y, f0), lane_bcast(so.z, f0));
          occ = sweep_shadow<true>(a.geo, a.rad, a.n, sfast, so, sd, P, gkey, dist, a.bv, work);
        }
        if (__ballot(sslow) != 0) {
          const bool os = sweep_shadow<false>(a.geo, a.rad, a.n, sslow, so, sd, so, gkey, dist, a.bv, work);
          occ = sfast ? occ : os;
        }
        c_slow += sslow ? 1u : 0u;
        return need && occ;
      };
      if (a.nl >= 2 && lpp >= 2) {  // wave-uniform
        const int rank = (int)__popcll(hm & ((1ull << lane) - 1ull));
        for (int l0 = 0; l0 < a.nl; l0 += lpp) {  // lights l0 .. l0 + cnt - 1 in this pass
          const int cnt = a.nl - l0 < lpp ? a.nl - l0 : lpp;
          const bool helper = lane < nh * cnt;
          const int r = helper ? lane / cnt : 0, lh = l0 + (helper ? lane - r * cnt : 0);
          const int src = nth_set_bit(hm, r);  // the owner: the r-th hit lane
          const D3 hq = mk(__shfl(hp.x, src, 64), __shfl(hp.y, src, 64), __shfl(hp.z, src, 64));
          const bool occ = in_shadow(helper, hq, lh, lh, false);  // lanes of one light sweep together
          const unsigned long long om = __ballot(occ);
          const unsigned long long bits = (om >> (hit ? rank * cnt : 0)) & (cnt >= 64 ? ~0ull : (1ull << cnt) - 1ull);
          shadowed |= hit ? bits << l0 : 0ull;  // 64-bit shifts: light 63 is bit 63
        }
      } else if (hm != 0) {
        for (int l = 0; l < a.nl; ++l)
          shadowed |= (unsigned long long)(in_shadow(hit, hp, l, hi, true) ? 1u : 0u) << l;  // 64-bit shift
      }
      c_shadow += hit ? (unsigned)a.nl : 0u;
      if (act) vdst[rec * 2 + 1] = vertex_tail(shadowed);
      // ---- the reflection ray (main.cpp:45-48), shade_hit's operand order; formed by every lane, used
      // by the lanes that spawn one (the others' paths have ended)
      const D3 rd = sub(d, scale(scale(nrm, 2.0), dot(d, nrm)));
      o = add(hp, scale(nrm, kEps));
      d = renormalized(rd);
      key = spawn ? hi : key;
      alive = spawn;
    }
    // the levels the loop never reached: every vertex record is written
    for (; k < a.depth; ++k) {
      if (act) {
        const long long rec = (long long)k * n + i;
        vdst[rec * 2] = vertex_head(kInf, -1, 0);
        vdst[rec * 2 + 1] = vertex_tail(0ull);
      }
    }
    c_rays += act ? 1u : 0u;
  }
  const unsigned long long s_rays = wave_sum(c_rays), s_seg = wave_sum(c_seg), s_hits = wave_sum(c_hits);
  const unsigned long long s_shadow = wave_sum(c_shadow), s_slow = wave_sum(c_slow);
  const unsigned long long s_exact = wave_sum64(work.exact), s_cull = wave_sum64(work.cull);
  if (lane == 0) {
    unsigned long long *cs = counter_shard(a.counters);
    atomicAdd(cs + kPcRays, s_rays);
    atomicAdd(cs + kPcSegments, s_seg);
    atomicAdd(cs + kPcHits, s_hits);
    atomicAdd(cs + kPcShadow, s_shadow);
    atomicAdd(cs + kPcExact, s_exact);
    atomicAdd(cs + kPcCull, s_cull);
    atomicAdd(cs + kPcUnaccel, s_slow);
  }
}

}  // namespace rtk
