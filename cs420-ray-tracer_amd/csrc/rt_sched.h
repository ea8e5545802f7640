// rt_sched.h -- host-side launch order of the render kernel's tiles.
//
// A wave's cost is set mostly by the reflection chains its pixels start: a
// tile whose camera rays land on reflective spheres traces up to depth-1
// more levels of incoherent rays (3-10x a ground or sky tile on synth200).
// Workgroups are dispatched in blockIdx order, so with tiles in scanline
// order the expensive band of the image starts mid-kernel and its slowest
// waves end long after the rest (the tail).  tile_order() predicts each
// tile's class from the projections of the reflective spheres onto the image
// (the reference's camera model, camera.h:17-25 / main.cpp:151-154) and
// returns the tiles heaviest class first, scanline order within a class
// (longest-processing-time-first list scheduling).  Only the order of the
// launch changes; every pixel is traced exactly as before.
#pragma once
#include <cstring>
#include <vector>

namespace rtk {

struct SchedSphere {
  double cx, cy, cz, r;
};

struct SchedView {
  double px, py, pz, fx, fy, fz, rx, ry, rz, ux, uy, uz, scale;  // Cam
  int W, H;
  int band, first, stride, count;  // Rows: launch row k -> image row y
  int x0, xw;                      // pixel columns [x0, x0 + xw)
  int tw, th;                      // tile size in pixels
};

// perm[b] = tile index (ty * ntx + tx) dispatched b-th; ntx = ceil(xw / tw),
// nty = ceil(count / th).  `refl` holds the reflective spheres only.
// class_count (optional, kSchedClasses entries): tiles per class; perm lists
// class kSchedClasses-1 first, then the lower classes in turn.
constexpr int kSchedClasses = 4;  // 0 .. 3 reflective spheres over a tile (capped)
void tile_order(const SchedView &v, const std::vector<SchedSphere> &refl, std::vector<int> &perm,
                long long *class_count = nullptr);

// The ray table of a launch (rt_kernel.hip ray_table_prepare): the camera
// rays' directions depend only on the camera's
// orientation, the image and the launch's rows -- not on the scene, the
// camera's position or the frame -- so a launch whose frames share them forms
// them once, in a pass ahead of the render kernel, and keeps them for the
// launches that follow.  This is what a table was formed for, compared by
// memcmp as the camera grid compares positions.
struct RayKey {
  double orient[10];               // forward, right, up, scale (Cam's)
  int W, H;
  int band, first, stride, count;  // Rows
  int pad[2];                      // 0 (no padding bytes: the struct is compared whole)
};
static_assert(sizeof(RayKey) == 10 * sizeof(double) + 8 * sizeof(int), "RayKey has padding");
inline bool ray_key_equal(const RayKey &a, const RayKey &b) { return std::memcmp(&a, &b, sizeof(RayKey)) == 0; }

// What a launch does about the table.  mode: rt_set_ray_table's (0 never, 1 the
// policy below, 2 every launch with one key).  uniform: every frame of the
// launch has `key`.  kept: the key of the table the context holds, prev: the
// key of the previous launch (nullptr: none, or its frames had several).
//  - frames of differing keys, or mode 0: the rays are formed inline;
//  - the kept table has this key: it is used as it is;
//  - else a launch of two frames or more builds one, and so does a one-frame
//    launch whose key the previous launch had too (the camera grid's
//    second-sighting rule: the build pass costs a first frame more than
//    forming its rays inline), or any launch with mode 2.
enum RayUse { kRayInline = 0, kRayReuse = 1, kRayBuild = 2 };
inline RayUse ray_table_policy(int mode, bool uniform, int nframes, const RayKey &key, const RayKey *kept,
                               const RayKey *prev) {
  if (mode <= 0 || !uniform || nframes < 1) return kRayInline;
  if (kept && ray_key_equal(key, *kept)) return kRayReuse;
  if (mode >= 2 || nframes >= 2 || (prev && ray_key_equal(key, *prev))) return kRayBuild;
  return kRayInline;
}

}  // namespace rtk
