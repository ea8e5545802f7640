// ray_hip.cpp -- C++ host driver over librt_hip.so; the drop-in CLI.
//
// Invoked as `ray_serial` / `ray_openmp` (symlinks) it keeps the reference's
// argv grammar, output file names and stdout lines (src/main.cpp:93-209):
//   ray_serial [scene]            -> output_serial.ppm, "Serial time: X seconds"
//   ray_openmp [--openmp] [scene] -> without --openmp: serial pass then OpenMP
//                                    pass (output_serial.ppm + output_openmp.ppm),
//                                    with --openmp: only output_openmp.ppm
// Both passes run on the GPU through the C-ABI: the names keep scripts such as
// the reference's makefile:48-96 and scripts/test.sh working unchanged.
// Invoked as `ray_hip` it behaves like the reference's ray_cuda driver
// (src/main_gpu.cu:357-540): output_gpu.ppm and "GPU rendering time: X seconds".
//
// Extra options (defaults equal the reference's hard-coded values,
// main.cpp:95-97): --width W --height H --depth D, --gpus G (rows sharded over
// G devices in cyclic 8-row bands, gathered to device 0 with ncclGather over
// xGMI), --device N, --out FILE, --p6 (binary PPM), --repeat N, --json, and
// -a (4-sample antialias, the ray_cuda flag of src/main_gpu.cu:363-370).
// --devices LIST (e.g. 0,1,2 or 0,0,0): the same row shards, one per listed
// device, through the library's device group (rt_group_*, no RCCL); a device
// may repeat, so one GPU can rehearse the multi-device path.
// --frames N [--batch B] (only with --devices): every pass renders a sequence
// of N frames of the scene's view with rt_group_render_frames, the members in
// launches of at most B frames (default: the library's largest), into memory of
// the first device; the time line is the whole sequence's, one more line gives
// the frames and the time per frame, and the LAST frame is the output image.
// --supersample N (1..8, one device only: not with --gpus, --devices or -a):
// N x N samples per pixel at the offsets (a/N, b/N), box-filtered, through
// rt_render_samples; --supersample 2 writes the bytes of -a.
// --sample-devices LIST (only with --supersample; not with --gpus, --devices or
// -a): the supersampled frame as row shards, one per listed device, through the
// device group (rt_group_render_samples); the same lines, file and --json fields.
// --aperture R [--focus F] (only with --supersample N; R >= 0): depth of field.
// Sample s leaves the thin-lens point lens_pattern(N, R)[s] of rt_hip.py (a disk
// of radius R) towards the plane F along forward, which stays sharp (default: the
// distance from the scene's camera position to its look-at point), through
// rt_render_lens_samples, or with --sample-devices rt_group_render_lens_samples.
// --focus without --aperture is a usage error; without --aperture nothing changes.
// --light-radius R (only with --supersample N; R >= 0; with or without --aperture and
// --sample-devices): area lights, soft shadows.  Sample s sees light l moved by
// light_pattern(N, R, num_lights)[s][l] of rt_hip.py (a horizontal disk of radius
// R), set once through rt_set_light_samples, or rt_group_set_light_samples, ahead
// of the render.  Without --light-radius nothing changes.
// --gloss SCALE [--gloss-bounces B] (only with --supersample N; B in 1..RT_MAX_GLOSS_BOUNCES, default 1;
// with or without --aperture, --light-radius and --sample-devices): glossy reflections.  The scene
// file's roughness column times SCALE, and gloss_pattern(N, B) of rt_hip.py, set once through
// rt_set_gloss_samples, or rt_group_set_gloss_samples, ahead of the render.  Without --gloss nothing changes.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include <sys/mman.h>
#include <string>
#include <vector>

#include "rt_hip.h"

namespace {

struct Opts {
  std::string mode = "hip";  // hip | serial | openmp
  std::string scene = "scenes/simple.txt";
  bool openmp_only = false;
  int width = 1280, height = 720, depth = 10;
  int gpus = 1, device = 0, repeat = 1;
  std::string out;
  bool p6 = false, json = false;
  bool force_gather = false;  // --force-gather: the G-device gather path even for G = 1 (rehearsal)
  int samples = 1;
  std::vector<int> devices;  // --devices LIST: the pass renders through rt_group_*
  int frames = -1, batch = -1;  // --frames N [--batch B]: a sequence per pass (rt_group_render_frames); -1: not given
  int supersample = 0;  // --supersample N: N x N samples per pixel through rt_render_samples; 0: not given
  std::vector<int> sample_devices;  // --sample-devices LIST: --supersample through rt_group_render_samples
  bool lens = false, focus_given = false;  // --aperture R [--focus F]: --supersample through rt_render_lens_samples
  double aperture = 0.0, focus = 0.0;
  bool area = false;  // --light-radius R: --supersample under rt_set_light_samples
  double light_radius = 0.0;
  bool gloss = false;  // --gloss SCALE [--gloss-bounces B]: --supersample under rt_set_gloss_samples
  bool gloss_bounces_given = false;
  double gloss_scale = 0.0;
  int gloss_bounces = 1;
};

int usage(const char *argv0) {
  std::fprintf(stderr,
               "usage: %s [--openmp] [-a | --supersample N] [--width W] [--height H] [--depth D] [--gpus G] [--device N]\n"
               "          [--devices D0,D1,... [--frames N [--batch B]]] [--out FILE] [--p6] [--repeat N]\n"
               "          [--sample-devices D0,D1,...] [--aperture R [--focus F]] [--light-radius R]\n"
               "          [--gloss SCALE [--gloss-bounces B]] [--json] [scene.txt]\n"
               "  --devices LIST  one row shard per listed device through the library's device group\n"
               "                  (a device may repeat: 0,0,0); not with --gpus > 1 or --force-gather\n"
               "  --frames N      with --devices: each pass renders N >= 1 frames of the view as one pipelined\n"
               "                  sequence and writes the last; --batch B (0..%d, 0 = %d): frames per launch\n"
               "  --supersample N N x N box-filtered samples per pixel (1..8); one device: not with --gpus,\n"
               "                  --devices or -a\n"
               "  --sample-devices LIST  with --supersample: the frame's row shards, one per listed device,\n"
               "                  through the device group; not with --gpus, --devices or -a\n"
               "  --aperture R    with --supersample: depth of field, a thin lens of radius R >= 0 (scene units);\n"
               "                  --focus F: the distance of the sharp plane (default: camera to look-at point)\n"
               "  --light-radius R  with --supersample: area lights, each light a horizontal disk of radius R >= 0\n"
               "                  (scene units) sampled once per pixel sample: soft shadows\n"
               "  --gloss SCALE   with --supersample: glossy reflections, the scene file's roughness column times\n"
               "                  SCALE bending each sample's reflection rays; --gloss-bounces B: the reflection\n"
               "                  levels bent, 1..%d (default 1), the later ones stay mirrors\n",
               argv0, RT_MAX_FRAMES, RT_MAX_FRAMES, RT_MAX_GLOSS_BOUNCES);
  return 2;
}

#define CK(call)                                                                          \
  do {                                                                                    \
    int rc_ = (call);                                                                     \
    if (rc_ != RT_OK) {                                                                   \
      std::fprintf(stderr, "%s failed: %s\n", #call, rt_error_string(rc_));                \
      return 1;                                                                           \
    }                                                                                     \
  } while (0)
#define HK(call)                                                                          \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) {                                                               \
      std::fprintf(stderr, "%s failed: %s\n", #call, hipGetErrorString(e_));               \
      return 1;                                                                           \
    }                                                                                     \
  } while (0)
#define NK(call)                                                                          \
  do {                                                                                    \
    ncclResult_t r_ = (call);                                                             \
    if (r_ != ncclSuccess) {                                                              \
      std::fprintf(stderr, "%s failed: %s\n", #call, ncclGetErrorString(r_));              \
      return 1;                                                                           \
    }                                                                                     \
  } while (0)

struct Result {
  double wall_s = 0;       // host wall time of the last frame (render + gather)
  double kernel_ms = 0;    // max over devices of the render kernel time
  uint64_t primary = 0, shadow = 0, reflect = 0, negative = 0;
  int frames = 0;          // --frames: wall_s, kernel_ms and the counts are the sequence's
};

// Single device: render the full frame.
int render_single(const Opts &o, const rt_scene &sc, const rt_camera &cam, uint8_t *img, Result &res) {
  rt_ctx *ctx = nullptr;
  CK(rt_create(o.device, &ctx));
  CK(rt_upload_scene(ctx, &sc));
  CK(rt_set_antialias(ctx, o.samples));
  rt_stats st{};
  for (int it = 0; it < o.repeat; it++) {
    auto t0 = std::chrono::high_resolution_clock::now();
    CK(rt_render(ctx, &cam, o.width, o.height, o.depth, nullptr, img, 0, &st));
    auto t1 = std::chrono::high_resolution_clock::now();
    res.wall_s = std::chrono::duration<double>(t1 - t0).count();
  }
  res.kernel_ms = st.kernel_ms;
  res.primary = st.rays_primary;
  res.shadow = st.rays_shadow;
  res.reflect = st.rays_reflect;
  res.negative = st.negative_clamped;
  rt_destroy(ctx);
  return 0;
}

// --supersample N: the full frame through rt_render_samples, N x N samples per pixel at (a/N, b/N), a fastest;
// with --sample-devices through rt_group_render_samples on a group of band 8.  With --aperture R the
// lens forms of the two calls, sample s at the lens point of grid cell N*N-1-s (rt_hip.py lens_pattern:
// the same doubles in the same order).  With --light-radius R the light table of rt_hip.py
// light_pattern(N, R, num_lights), restated the same way, is set ahead of the render; with --gloss SCALE
// the gloss table of gloss_pattern(N, B) and the scene file's roughness column times SCALE.
int render_supersampled(const Opts &o, const rt_scene &sc, const rt_camera &cam, uint8_t *img, Result &res) {
  const int N = o.supersample;
  std::vector<double> offsets;
  for (int b = 0; b < N; b++)
    for (int a = 0; a < N; a++) {
      offsets.push_back((double)a / N);
      offsets.push_back((double)b / N);
    }
  // point s of lens_pattern(N, radius): the centre of grid cell N*N-1-s on the disk of that radius
  auto disk_point = [N](int s, double radius, double &x, double &y) {
    const int c = N * N - 1 - s, a = c % N, b = c / N;
    const double u = (a + 0.5) / N * 2.0 - 1.0, v = (b + 0.5) / N * 2.0 - 1.0;
    x = u * std::sqrt(1.0 - v * v / 2.0) * radius;
    y = v * std::sqrt(1.0 - u * u / 2.0) * radius;
  };
  std::vector<double> lens;
  if (o.lens)
    for (int s = 0; s < N * N; s++) {
      double x, y;
      disk_point(s, o.aperture, x, y);
      lens.push_back(x);
      lens.push_back(y);
    }
  std::vector<double> light_xyz;  // [s][l]: point (s + 17 l) % (N*N) of the disk, as (x, 0, z)
  if (o.area) {
    for (int s = 0; s < N * N; s++)
      for (int l = 0; l < sc.num_lights; l++) {
        double x, z;
        disk_point((s + 17 * l) % (N * N), o.light_radius, x, z);
        light_xyz.push_back(x);
        light_xyz.push_back(0.0);
        light_xyz.push_back(z);
      }
    if (light_xyz.empty()) light_xyz.push_back(0.0);  // a scene without lights: a non-NULL, empty table
  }
  std::vector<double> gloss_xyz, rough;  // [s][b]: disk point i = (s + 17 (b+1)) % (N*N) lifted into the unit ball
  if (o.gloss) {
    const int nn = N * N;
    for (int s = 0; s < nn; s++)
      for (int b = 0; b < o.gloss_bounces; b++) {
        const int i = (s + 17 * (b + 1)) % nn;
        double x, y;
        disk_point(i, 1.0, x, y);
        const double h = (double)(2 * ((7 * i + 3) % nn) + 1) / nn - 1.0;
        gloss_xyz.push_back(x);
        gloss_xyz.push_back(y);
        gloss_xyz.push_back(h * std::sqrt(std::max(0.0, 1.0 - x * x - y * y)));
      }
    int n = 0;
    rough.resize((size_t)sc.num_spheres + 1);
    CK(rt_scene_load_roughness(o.scene.c_str(), rough.data(), sc.num_spheres, &n));
    if (n != sc.num_spheres) {
      std::fprintf(stderr, "%s changed while it was read\n", o.scene.c_str());
      return 1;
    }
    for (double &r : rough) r = r * o.gloss_scale;
  }
  double focus = o.focus;
  if (o.lens && !o.focus_given) {
    const double dx = sc.cam_look_at[0] - sc.cam_position[0], dy = sc.cam_look_at[1] - sc.cam_position[1],
                 dz = sc.cam_look_at[2] - sc.cam_position[2];
    focus = std::sqrt(dx * dx + dy * dy + dz * dz);
  }
  rt_radiance_stats st{};
  auto report = [&] {
    res.kernel_ms = st.kernel_ms;
    res.primary = st.rays;
    res.shadow = st.shadow_rays;
    res.reflect = st.segments - st.rays;
    res.negative = st.negative_clamped;
  };
  if (!o.sample_devices.empty()) {
    rt_group *grp = nullptr;
    CK(rt_group_create(o.sample_devices.data(), (int)o.sample_devices.size(), 8, &grp));
    int rc = rt_group_upload_scene(grp, &sc);
    if (rc == RT_OK && o.area) rc = rt_group_set_light_samples(grp, light_xyz.data(), N * N);
    if (rc == RT_OK && o.gloss)
      rc = rt_group_set_gloss_samples(grp, rough.data(), gloss_xyz.data(), N * N, o.gloss_bounces);
    for (int it = 0; it < o.repeat && rc == RT_OK; it++) {
      auto t0 = std::chrono::high_resolution_clock::now();
      rc = o.lens ? rt_group_render_lens_samples(grp, &cam, o.width, o.height, o.depth, offsets.data(), lens.data(),
                                                 focus, N * N, nullptr, RT_FB_RGB8, img, 0, &st)
                  : rt_group_render_samples(grp, &cam, o.width, o.height, o.depth, offsets.data(), N * N, nullptr,
                                            RT_FB_RGB8, img, 0, &st);
      auto t1 = std::chrono::high_resolution_clock::now();
      res.wall_s = std::chrono::duration<double>(t1 - t0).count();
    }
    if (rc != RT_OK)
      std::fprintf(stderr, "device group failed: %s (%s)\n", rt_error_string(rc), rt_group_last_error(grp));
    rt_group_destroy(grp);
    report();
    return rc != RT_OK ? 1 : 0;
  }
  rt_ctx *ctx = nullptr;
  CK(rt_create(o.device, &ctx));
  CK(rt_upload_scene(ctx, &sc));
  if (o.area) CK(rt_set_light_samples(ctx, light_xyz.data(), N * N));
  if (o.gloss) CK(rt_set_gloss_samples(ctx, rough.data(), gloss_xyz.data(), N * N, o.gloss_bounces));
  for (int it = 0; it < o.repeat; it++) {
    auto t0 = std::chrono::high_resolution_clock::now();
    if (o.lens)
      CK(rt_render_lens_samples(ctx, &cam, o.width, o.height, o.depth, nullptr, offsets.data(), lens.data(), focus,
                                N * N, nullptr, RT_FB_RGB8, img, 0, &st));
    else
      CK(rt_render_samples(ctx, &cam, o.width, o.height, o.depth, nullptr, offsets.data(), N * N, nullptr, RT_FB_RGB8,
                           img, 0, 0, &st));
    auto t1 = std::chrono::high_resolution_clock::now();
    res.wall_s = std::chrono::duration<double>(t1 - t0).count();
  }
  report();
  rt_destroy(ctx);
  return 0;
}

// G devices in one process: cyclic 8-row bands, ncclGather to device 0, unpermute.
int render_multi(const Opts &o, const rt_scene &sc, const rt_camera &cam, uint8_t *img, Result &res) {
  const int G = o.gpus, W = o.width, H = o.height, band = 8;
  rt_rows layout;
  CK(rt_rows_for_shard(H, band, 0, G, &layout));  // the layout bench.py's ranks use
  const int R = layout.count;
  const size_t shard_bytes = (size_t)R * W * 3;
  std::vector<rt_ctx *> ctx(G, nullptr);
  std::vector<hipStream_t> streams(G);
  std::vector<uint8_t *> shard(G, nullptr);
  std::vector<int> devs(G);
  uint8_t *gathered = nullptr, *image = nullptr;
  for (int g = 0; g < G; g++) {
    devs[g] = g;
    CK(rt_create(g, &ctx[g]));
    CK(rt_upload_scene(ctx[g], &sc));
    CK(rt_set_antialias(ctx[g], o.samples));
    HK(hipSetDevice(g));
    HK(hipStreamCreateWithFlags(&streams[g], hipStreamNonBlocking));
    CK(rt_set_stream(ctx[g], streams[g]));
    HK(hipMalloc(&shard[g], shard_bytes));
  }
  HK(hipSetDevice(0));
  HK(hipMalloc(&gathered, shard_bytes * G));
  HK(hipMalloc(&image, (size_t)H * W * 3));
  std::vector<ncclComm_t> comms(G);
  NK(ncclCommInitAll(comms.data(), G, devs.data()));
  for (int it = 0; it < o.repeat; it++) {
    for (int g = 0; g < G; g++) {
      HK(hipSetDevice(g));
      HK(hipDeviceSynchronize());
    }
    auto t0 = std::chrono::high_resolution_clock::now();
    for (int g = 0; g < G; g++) {
      rt_rows rows;
      CK(rt_rows_for_shard(H, band, g, G, &rows));
      CK(rt_render_async(ctx[g], &cam, W, H, o.depth, &rows, shard[g]));
    }
    NK(ncclGroupStart());
    for (int g = 0; g < G; g++) {
      HK(hipSetDevice(g));
      NK(ncclGather(shard[g], g == 0 ? gathered : nullptr, shard_bytes, ncclUint8, 0, comms[g], streams[g]));
    }
    NK(ncclGroupEnd());
    CK(rt_unpermute_rows(ctx[0], gathered, image, W, H, band, G, R));
    HK(hipSetDevice(0));
    HK(hipStreamSynchronize(streams[0]));
    auto t1 = std::chrono::high_resolution_clock::now();
    res.wall_s = std::chrono::duration<double>(t1 - t0).count();
  }
  HK(hipSetDevice(0));
  HK(hipMemcpy(img, image, (size_t)H * W * 3, hipMemcpyDeviceToHost));
  res.kernel_ms = 0;
  for (int g = 0; g < G; g++) {
    rt_stats st{};
    CK(rt_render_stats(ctx[g], &st));
    res.kernel_ms = std::max(res.kernel_ms, st.kernel_ms);
    res.primary += st.rays_primary;
    res.shadow += st.rays_shadow;
    res.reflect += st.rays_reflect;
    res.negative += st.negative_clamped;
  }
  for (int g = 0; g < G; g++) {
    ncclCommDestroy(comms[g]);
    HK(hipSetDevice(g));
    HK(hipFree(shard[g]));
    rt_destroy(ctx[g]);
    HK(hipStreamDestroy(streams[g]));
  }
  HK(hipSetDevice(0));
  HK(hipFree(gathered));
  HK(hipFree(image));
  return 0;
}

// --devices: one shard per listed device through the library's device group.
int render_group(const Opts &o, const rt_scene &sc, const rt_camera &cam, uint8_t *img, Result &res) {
  rt_group *grp = nullptr;
  uint8_t *seq = nullptr;
  CK(rt_group_create(o.devices.data(), (int)o.devices.size(), 8, &grp));
  auto run = [&]() -> int {
    int rc = rt_group_upload_scene(grp, &sc);
    if (rc == RT_OK) rc = rt_group_set_antialias(grp, o.samples);
    rt_stats st{};
    // --frames: the sequence stays in memory of the first device, the last frame is copied out
    const size_t image_bytes = (size_t)o.width * o.height * 3;
    const std::vector<rt_camera> cams(o.frames > 0 ? (size_t)o.frames : 0, cam);
    hipError_t he = hipSuccess;
    if (o.frames > 0 && rc == RT_OK) {
      he = hipSetDevice(o.devices[0]);
      if (he == hipSuccess) he = hipMalloc(&seq, image_bytes * cams.size());
    }
    for (int it = 0; it < o.repeat && rc == RT_OK && he == hipSuccess; it++) {
      auto t0 = std::chrono::high_resolution_clock::now();
      rc = o.frames > 0 ? rt_group_render_frames(grp, cams.data(), o.frames, o.width, o.height, o.depth,
                                                 o.batch < 0 ? 0 : o.batch, seq, 1, image_bytes, &st)
                        : rt_group_render(grp, &cam, o.width, o.height, o.depth, img, 0, &st);
      auto t1 = std::chrono::high_resolution_clock::now();
      res.wall_s = std::chrono::duration<double>(t1 - t0).count();
    }
    if (o.frames > 0 && rc == RT_OK && he == hipSuccess) {
      he = hipSetDevice(o.devices[0]);
      if (he == hipSuccess)
        he = hipMemcpy(img, seq + image_bytes * (cams.size() - 1), image_bytes, hipMemcpyDeviceToHost);
      res.frames = o.frames;
    }
    if (he != hipSuccess) {
      std::fprintf(stderr, "the sequence's buffer on device %d: %s\n", o.devices[0], hipGetErrorString(he));
      return RT_ERR_HIP;
    }
    res.kernel_ms = st.kernel_ms;
    res.primary = st.rays_primary;
    res.shadow = st.rays_shadow;
    res.reflect = st.rays_reflect;
    res.negative = st.negative_clamped;
    return rc;
  };
  const int rc = run();
  if (rc != RT_OK)
    std::fprintf(stderr, "device group failed: %s (%s)\n", rt_error_string(rc), rt_group_last_error(grp));
  if (seq) (void)hipFree(seq);
  rt_group_destroy(grp);
  return rc != RT_OK ? 1 : 0;
}

// "0,1,2" -> {0, 1, 2}; false unless every item is a non-negative decimal number.
bool parse_devices(const char *list, std::vector<int> &out) {
  out.clear();
  for (const char *p = list;; p++) {
    if (*p < '0' || *p > '9') return false;
    long v = 0;
    for (; *p >= '0' && *p <= '9'; p++)
      if ((v = v * 10 + (*p - '0')) > 1 << 20) return false;
    out.push_back((int)v);
    if (*p == '\0') return true;
    if (*p != ',') return false;
  }
}

int render_pass(const Opts &o, const rt_scene &sc, const rt_camera &cam, const char *label, const char *file) {
  // the image: 2 MB-aligned and advised for huge pages (3 page faults at
  // 1080p instead of ~1,500), zeroed here as the reference value-initialises
  // its framebuffer (main.cpp:136) -- so the faults are taken before the timed
  // render, whose device-to-host copy would otherwise pay them (~7 ms)
  const size_t img_bytes = (size_t)o.width * o.height * 3;
  const size_t img_cap = (img_bytes + 1 + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
  std::unique_ptr<uint8_t[], void (*)(uint8_t *)> img(static_cast<uint8_t *>(std::aligned_alloc((size_t)2 << 20, img_cap)),
                                                      [](uint8_t *p) { std::free(p); });
  if (!img) {
    std::fprintf(stderr, "out of memory for a %dx%d image\n", o.width, o.height);
    return 1;
  }
  (void)madvise(img.get(), img_cap, MADV_HUGEPAGE);
  std::memset(img.get(), 0, img_cap);
  Result res;
  int rc = o.supersample                    ? render_supersampled(o, sc, cam, img.get(), res)
           : !o.devices.empty()             ? render_group(o, sc, cam, img.get(), res)
           : (o.gpus > 1 || o.force_gather) ? render_multi(o, sc, cam, img.get(), res)
                                            : render_single(o, sc, cam, img.get(), res);
  if (rc) return rc;
  if (o.mode == "hip")
    std::printf("GPU rendering time: %g seconds\n", res.wall_s);  // main_gpu.cu:519
  else
    std::printf("%s time: %g seconds\n", label, res.wall_s);      // main.cpp:161 / :203
  if (res.frames)
    std::printf("Frames: %d, %g ms per frame\n", res.frames, res.wall_s * 1e3 / res.frames);
  if (res.negative)
    std::fprintf(stderr, "warning: %llu channels quantised below 0 were stored as 0\n",
                 (unsigned long long)res.negative);
  if (o.json) {
    uint64_t rays = res.primary + res.shadow + res.reflect;
    const std::string frames = res.frames ? "\"frames\": " + std::to_string(res.frames) + ", " : "";
    std::printf(
        "{\"scene\": \"%s\", \"width\": %d, \"height\": %d, \"depth\": %d, \"gpus\": %d, %s\"rays\": %llu, "
        "\"primary\": %llu, \"shadow\": %llu, \"reflect\": %llu, \"kernel_ms\": %.4f, \"wall_ms\": %.4f, "
        "\"mrays_per_s\": %.2f}\n",
        o.scene.c_str(), o.width, o.height, o.depth,
        !o.sample_devices.empty() ? (int)o.sample_devices.size() : o.devices.empty() ? o.gpus : (int)o.devices.size(),
        frames.c_str(), (unsigned long long)rays,
        (unsigned long long)res.primary, (unsigned long long)res.shadow, (unsigned long long)res.reflect,
        res.kernel_ms, res.wall_s * 1e3, rays / (res.kernel_ms * 1e-3) / 1e6);
  }
  std::fflush(stdout);
  int wrc = rt_write_ppm(file, img.get(), o.width, o.height, o.p6 ? 1 : 0);
  if (wrc != RT_OK) {
    std::fprintf(stderr, "could not write %s: %s\n", file, rt_error_string(wrc));
    return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  Opts o;
  bool gpus_given = false;
  std::string base = argv[0];
  size_t slash = base.find_last_of('/');
  if (slash != std::string::npos) base = base.substr(slash + 1);
  if (base == "ray_serial") o.mode = "serial";
  else if (base == "ray_openmp") o.mode = "openmp";
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto next = [&](int &dst) {
      if (i + 1 >= argc) return false;
      dst = std::atoi(argv[++i]);
      return true;
    };
    auto next_double = [&](double &dst) {  // the whole argument, or nothing
      if (i + 1 >= argc) return false;
      char *end = nullptr;
      dst = std::strtod(argv[++i], &end);
      return end != argv[i] && *end == '\0';
    };
    if (a == "--openmp") o.openmp_only = true;
    else if (a == "--width") { if (!next(o.width)) return usage(argv[0]); }
    else if (a == "--height") { if (!next(o.height)) return usage(argv[0]); }
    else if (a == "--depth") { if (!next(o.depth)) return usage(argv[0]); }
    else if (a == "--gpus") { if (!next(o.gpus)) return usage(argv[0]); gpus_given = true; }
    else if (a == "--device") { if (!next(o.device)) return usage(argv[0]); }
    else if (a == "--devices") { if (i + 1 >= argc || !parse_devices(argv[++i], o.devices)) return usage(argv[0]); }
    else if (a == "--frames") { if (!next(o.frames) || o.frames < 1) return usage(argv[0]); }
    else if (a == "--batch") { if (!next(o.batch) || o.batch < 0 || o.batch > RT_MAX_FRAMES) return usage(argv[0]); }
    else if (a == "--repeat") { if (!next(o.repeat)) return usage(argv[0]); }
    else if (a == "--out") { if (i + 1 >= argc) return usage(argv[0]); o.out = argv[++i]; }
    else if (a == "--p6") o.p6 = true;
    else if (a == "--force-gather") o.force_gather = true;
    else if (a == "-a") o.samples = 4;
    else if (a == "--supersample") { if (!next(o.supersample) || o.supersample < 1 || o.supersample > 8) return usage(argv[0]); }
    else if (a == "--sample-devices") { if (i + 1 >= argc || !parse_devices(argv[++i], o.sample_devices)) return usage(argv[0]); }
    else if (a == "--aperture") { if (!next_double(o.aperture) || !(o.aperture >= 0.0)) return usage(argv[0]); o.lens = true; }
    else if (a == "--light-radius") { if (!next_double(o.light_radius) || !(o.light_radius >= 0.0)) return usage(argv[0]); o.area = true; }
    else if (a == "--gloss") { if (!next_double(o.gloss_scale)) return usage(argv[0]); o.gloss = true; }
    else if (a == "--gloss-bounces") { if (!next(o.gloss_bounces) || o.gloss_bounces < 1 || o.gloss_bounces > RT_MAX_GLOSS_BOUNCES) return usage(argv[0]); o.gloss_bounces_given = true; }
    else if (a == "--focus") { if (!next_double(o.focus)) return usage(argv[0]); o.focus_given = true; }
    else if (a == "--json") o.json = true;
    else if (a == "-h" || a == "--help") return usage(argv[0]);
    else o.scene = a;  // any other argument is the scene path, as main.cpp:103-110
  }
  if (o.width <= 0 || o.height <= 0 || o.gpus < 1 || o.repeat < 1) return usage(argv[0]);
  if (!o.devices.empty() && (o.gpus > 1 || o.force_gather)) return usage(argv[0]);
  if (o.supersample && (gpus_given || !o.devices.empty() || o.force_gather || o.samples != 1)) return usage(argv[0]);
  if (!o.sample_devices.empty() && !o.supersample) return usage(argv[0]);  // with --supersample: the line above
  if ((o.lens && !o.supersample) || (o.focus_given && !o.lens)) return usage(argv[0]);
  if (o.area && !o.supersample) return usage(argv[0]);
  if ((o.gloss && !o.supersample) || (o.gloss_bounces_given && !o.gloss)) return usage(argv[0]);
  if ((o.frames > 0 && o.devices.empty()) || (o.batch >= 0 && o.frames < 0)) return usage(argv[0]);

  std::printf("Testing scene loader with: %s\n\n", o.scene.c_str());  // main.cpp:116
  rt_scene sc;
  int rc = rt_scene_load(o.scene.c_str(), &sc, 1);
  if (rc != RT_OK) {
    std::fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                         "  what():  Could not open scene file: %s\n", o.scene.c_str());
    return 134 - 128;  // the reference aborts on the uncaught exception
  }
  rt_camera cam;
  rt_camera_from_scene(&sc, &cam);

  int status = 0;
  if (o.mode == "hip") {
    status = render_pass(o, sc, cam, "GPU", o.out.empty() ? "output_gpu.ppm" : o.out.c_str());
  } else {
    if (!o.openmp_only) {  // main.cpp:142-164
      std::printf("Rendering (Serial)...\n");
      status = render_pass(o, sc, cam, "Serial", o.out.empty() ? "output_serial.ppm" : o.out.c_str());
    }
    if (!status && o.mode == "openmp") {  // main.cpp:168-206
      std::printf("\nRendering (OpenMP)...\n");
      status = render_pass(o, sc, cam, "OpenMP", "output_openmp.ppm");
    }
  }
  rt_scene_free(&sc);
  return status;
}
