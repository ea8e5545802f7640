// Ray queries (rt_trace_rays, rt_camera_rays): the closest hit
// (Scene::find_intersection, scene.h:41-61) and the occlusion test (the
// any-hit half of Scene::in_shadow, scene.h:65-86) for rays the caller
// supplies, one ray per lane, through the render kernels' own sweeps and walks
// (rt_device.h sweep_closest / sweep_shadow, used as they are).  Included only
// by rt_kernel.hip, after rt_hip.h and rt_device.h.
#pragma once

#include "rt_device.h"

namespace rtk {

static_assert(sizeof(rt_ray) == 64 && sizeof(rt_hit) == 16, "rt_ray / rt_hit layout (rt_hip.h)");

// The query path's own counter block, sharded like the render counters.
enum { kQcRays = 0, kQcHits, kQcExact, kQcCull, kQcUnaccel, kQueryCounters };

struct QueryArgs {
  const SphGeo *geo;
  const double *rad;
  int n;        // spheres
  int nrays;    // >= 1
  int accel;    // 0: every ray tests every sphere (rt_set_culling(ctx, 0))
  const rt_ray *rays;
  rt_hit *hits;
  // The query region R: BvhArgs' margins are sized for origins inside it.
  double rlo[3], rhi[3];
  BvhArgs bv;
  unsigned long long *counters;
};

// rt_hit as one 16-byte word: t, then sphere (low half) and occluded.
__device__ __forceinline__ double2 pack_hit(double t, int sphere, int occluded) {
  const unsigned long long w = (unsigned long long)(unsigned)sphere | (unsigned long long)(unsigned)occluded << 32;
  return make_double2(t, __longlong_as_double((long long)w));
}

// One wave per workgroup, one ray per lane, grid-stride over the batch.  Every
// lane stays in every sweep (the sweeps' wave reductions need all 64): the
// lanes past the end of the batch re-read its last ray with act = false, and
// only the store is guarded.  Lanes whose origin lies in R (and whose
// normalised direction is finite, so that one NaN ray does not loosen its
// wave's cull bound) take the culled sweep and the BVH walks; the others the
// every-sphere sweep, which is the reference's own scan for any input.
template <int kMode>
__global__ __launch_bounds__(64) void query_kernel(const QueryArgs a) {
  const int lane = (int)(threadIdx.x & 63);
  const long long n = a.nrays, step = (long long)gridDim.x * 64;
  Work work;
  unsigned c_rays = 0, c_hits = 0, c_slow = 0;
  const double2 *__restrict__ src = reinterpret_cast<const double2 *>(a.rays);
  double2 *__restrict__ dst = reinterpret_cast<double2 *>(a.hits);
  for (long long base = (long long)blockIdx.x * 64; base < n; base += step) {
    const long long i = base + lane;
    const bool act = i < n;
    const long long ld = act ? i : n - 1;
    const double2 r0 = src[ld * 4 + 0], r1 = src[ld * 4 + 1], r2 = src[ld * 4 + 2], r3 = src[ld * 4 + 3];
    const D3 o = mk(r0.x, r0.y, r1.x);
    const D3 d = normalized(mk(r1.y, r2.x, r2.y));  // Ray(o, d), ray.h:12: once
    const double tmax = r3.x;
    const bool in_r = o.x >= a.rlo[0] && o.x <= a.rhi[0] && o.y >= a.rlo[1] && o.y <= a.rhi[1] && o.z >= a.rlo[2] &&
                      o.z <= a.rhi[2];  // false for a NaN component
    const bool finite_d = __builtin_fabs(d.x) <= 2.0 && __builtin_fabs(d.y) <= 2.0 && __builtin_fabs(d.z) <= 2.0;
    const bool fast = act && a.accel != 0 && in_r && finite_d;
    const bool slow = act && !fast;
    double t = kInf;
    int sphere = -1, occ = 0;
    if (kMode == RT_QUERY_CLOSEST) {
      double t_fast = kInf, t_slow = kInf;
      int s_fast = -1, s_slow = -1;
      if (__ballot(fast) != 0) s_fast = sweep_closest<true, false>(a.geo, a.rad, a.n, fast, o, d, -1, a.bv, t_fast, work);
      if (__ballot(slow) != 0) s_slow = sweep_closest<false>(a.geo, a.rad, a.n, slow, o, d, -1, a.bv, t_slow, work);
      sphere = fast ? s_fast : s_slow;
      t = fast ? t_fast : t_slow;
      // in_shadow's test on the closest root: some sphere reports t < 1e20 and
      // t < tmax exactly when the smallest recorded t is below tmax
      occ = (sphere >= 0 && t < tmax) ? 1 : 0;
      c_hits += (act && sphere >= 0) ? 1u : 0u;
    } else {
      const unsigned long long fm = __ballot(fast);
      const int l0 = fm ? __builtin_ctzll(fm) : 0;
      const D3 P = mk(lane_bcast(o.x, l0), lane_bcast(o.y, l0), lane_bcast(o.z, l0));
      bool oc = false;
      if (fm != 0) oc = sweep_shadow<true>(a.geo, a.rad, a.n, fast, o, d, P, -1, tmax, a.bv, work);
      if (__ballot(slow) != 0) {
        const bool os = sweep_shadow<false>(a.geo, a.rad, a.n, slow, o, d, o, -1, tmax, a.bv, work);
        oc = fast ? oc : os;
      }
      occ = (act && oc) ? 1 : 0;
      c_hits += (unsigned)occ;
    }
    c_rays += act ? 1u : 0u;
    c_slow += slow ? 1u : 0u;
    if (act) dst[i] = pack_hit(t, sphere, occ);
  }
  const unsigned long long s_rays = wave_sum(c_rays), s_hits = wave_sum(c_hits), s_slow = wave_sum(c_slow);
  const unsigned long long s_exact = wave_sum64(work.exact), s_cull = wave_sum64(work.cull);
  if (lane == 0) {
    unsigned long long *cs = counter_shard(a.counters);
    atomicAdd(cs + kQcRays, s_rays);
    atomicAdd(cs + kQcHits, s_hits);
    atomicAdd(cs + kQcExact, s_exact);
    atomicAdd(cs + kQcCull, s_cull);
    atomicAdd(cs + kQcUnaccel, s_slow);
  }
}

// rt_camera_rays: the ray of output row k, column x, as get_ray hands it to
// Ray() -- the camera position and the once-normalised direction -- or zeros
// for a padding row.  One thread per ray, 64 bytes as four 16-byte stores.
__global__ __launch_bounds__(kBlock) void camera_rays_kernel(const Cam cam, int W, int H, const Rows rows,
                                                              rt_ray *__restrict__ out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (long long)rows.count * W) return;
  const int k = (int)(i / W), x = (int)(i % W);
  const long long y = (long long)(k / rows.band) * rows.band * rows.stride + (long long)rows.first * rows.band +
                      (k % rows.band);
  double2 *dst = reinterpret_cast<double2 *>(out) + i * 4;
  if (y >= H) {  // padding rows of a shard
    dst[0] = dst[1] = dst[2] = dst[3] = make_double2(0.0, 0.0);
    return;
  }
  const int j = H - 1 - (int)y;  // reference row (main.cpp:74)
  const D3 d = normalized(camera_dir(cam, (double)x, (double)j, W, H));
  dst[0] = make_double2(cam.px, cam.py);
  dst[1] = make_double2(cam.pz, d.x);
  dst[2] = make_double2(d.y, d.z);
  dst[3] = make_double2(__builtin_inf(), 0.0);
}

// rt_camera_sample_rays: camera_rays_kernel for a caller's sample pattern.  The
// ray of output row k_first + k, column x, sample s is out[(k*W + x)*S + s]: the
// camera position and normalized(camera_dir(x + ox_s, j + oy_s)), trace_tile's
// antialias arithmetic (the offset is added before the division by W-1 / H-1;
// x + 0.0 == x, so one (0,0) sample gives camera_rays_kernel's records).  The
// offsets travel in the kernel arguments: a lane reads its sample's pair from
// the kernarg segment.  k_first / nrows select a run of the output rows of
// `rows` (rt_render_samples traces them in chunks).  One thread per ray.
struct SampleOffsets {
  double xy[2 * RT_MAX_SAMPLES];
};
__global__ __launch_bounds__(kBlock) void camera_sample_rays_kernel(const Cam cam, int W, int H, const Rows rows,
                                                                     int k_first, int nrows, int S,
                                                                     const SampleOffsets off,
                                                                     rt_ray *__restrict__ out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (long long)nrows * W * S) return;
  const int s = (int)(i % S);
  const long long p = i / S;
  const int k = k_first + (int)(p / W), x = (int)(p % W);
  const long long y = (long long)(k / rows.band) * rows.band * rows.stride + (long long)rows.first * rows.band +
                      (k % rows.band);
  double2 *dst = reinterpret_cast<double2 *>(out) + i * 4;
  if (y >= H) {  // padding rows of a shard
    dst[0] = dst[1] = dst[2] = dst[3] = make_double2(0.0, 0.0);
    return;
  }
  const int j = H - 1 - (int)y;  // reference row (main.cpp:74)
  const D3 d = normalized(camera_dir(cam, (double)x + off.xy[2 * s], (double)j + off.xy[2 * s + 1], W, H));
  dst[0] = make_double2(cam.px, cam.py);
  dst[1] = make_double2(cam.pz, d.x);
  dst[2] = make_double2(d.y, d.z);
  dst[3] = make_double2(__builtin_inf(), 0.0);
}

// A thin lens in front of camera_dir: the ray of one sample leaves the lens point P + right*lx + up*ly
// and passes through the point P + dir0*focus of the focal plane, where dir0 (camera_dir's unnormalised
// direction, forward component 1) is the pinhole ray of the sample.  Returns the record's direction,
// normalised once, and the record's origin in `o`.  (lx, ly) = (0, 0) and focus = 1.0 give the pinhole
// record as values: o = P + 0, dir = normalized(dir0*1 - 0).  Any double is allowed: a non-finite lens
// point or focus gives NaN rays, which the queries treat as misses.  rt_camera_lens_rays and
// radiance_kernel's kLens form share it.
__device__ __forceinline__ D3 lens_ray(const Cam &cam, D3 dir0, double lx, double ly, double focus, D3 &o) {
  const D3 lv = add(scale(mk(cam.rx, cam.ry, cam.rz), lx), scale(mk(cam.ux, cam.uy, cam.uz), ly));
  o = add(mk(cam.px, cam.py, cam.pz), lv);
  return normalized(sub(scale(dir0, focus), lv));
}

// rt_camera_lens_rays: camera_sample_rays_kernel with the lens.  The same layout and padding rows; the
// lens points travel in the kernel arguments beside the offsets, sample s pairing offset s with lens
// point s.  One thread per ray.
struct SampleLens {
  double focus;
  double xy[2 * RT_MAX_SAMPLES];  // (lx_s, ly_s)
};
__global__ __launch_bounds__(kBlock) void camera_lens_rays_kernel(const Cam cam, int W, int H, const Rows rows, int S,
                                                                   const SampleOffsets off, const SampleLens lens,
                                                                   rt_ray *__restrict__ out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (long long)rows.count * W * S) return;
  const int s = (int)(i % S);
  const long long p = i / S;
  const int k = (int)(p / W), x = (int)(p % W);
  const long long y = (long long)(k / rows.band) * rows.band * rows.stride + (long long)rows.first * rows.band +
                      (k % rows.band);
  double2 *dst = reinterpret_cast<double2 *>(out) + i * 4;
  if (y >= H) {  // padding rows of a shard
    dst[0] = dst[1] = dst[2] = dst[3] = make_double2(0.0, 0.0);
    return;
  }
  const int j = H - 1 - (int)y;  // reference row (main.cpp:74)
  const D3 dir0 = camera_dir(cam, (double)x + off.xy[2 * s], (double)j + off.xy[2 * s + 1], W, H);
  D3 o;
  const D3 d = lens_ray(cam, dir0, lens.xy[2 * s], lens.xy[2 * s + 1], lens.focus, o);
  dst[0] = make_double2(o.x, o.y);
  dst[1] = make_double2(o.z, d.x);
  dst[2] = make_double2(d.y, d.z);
  dst[3] = make_double2(__builtin_inf(), 0.0);
}

}  // namespace rtk
