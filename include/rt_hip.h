/*
 * rt_hip.h -- C-ABI of the MI355X (gfx950) render-loop library, librt_hip.so.
 *
 * Drop-in boundary for the per-pixel render loop of shininglegend/cs420-ray-tracer.
 * Plain C, POD structs, plain pointers and sizes; no HIP/torch types appear in
 * any signature (streams are passed as `void *` = hipStream_t).
 *
 * What each entry point replaces in the reference (file:line):
 *   rt_scene_load / rt_scene_parse  <- load_scene()           include/scene_loader.h:27-135
 *   rt_scene_free                   <- Scene destructor       include/scene.h:28-33
 *   rt_camera_from_scene            <- Camera::Camera()       include/camera.h:10-15 (+ scale of get_ray, :18-19)
 *   rt_create / rt_destroy          <- GPUResources ctor/dtor src/main_hybrid.cpp:182-195, 300-316
 *   rt_upload_scene                 <- GPUResources::upload_scene + upload_lights_and_ambience
 *                                      src/main_hybrid.cpp:198-279, src/kernel.cu:202-207
 *   rt_render                       <- the serial pixel loop  src/main.cpp:146-157 (trace_ray :16-58),
 *                                      the OpenMP loop :185-199, and launch_gpu_kernel src/kernel.cu:185-200
 *   rt_render_async                 <- launch_gpu_kernel(..., cudaStream_t) src/kernel.cu:185-200
 *   rt_render_frames_async          <- (new) the pixel loop over a sequence of frames in one launch
 *                                      (frame f = rt_render_async with cams[f])
 *   rt_write_ppm                    <- write_ppm()            src/main.cpp:69-91
 *   rt_kernel_times                 <- cudaEventElapsedTime around the kernel, src/main_gpu.cu:496-519
 *   rt_unpermute_rows               <- (new) reassembly of the multi-GPU row shards
 *   rt_group_create / _destroy / _size / _member / _last_error / _upload_scene / _set_antialias / _render
 *                                   <- (new) render_multi in csrc/ray_hip.cpp: the contexts, streams
 *                                      and shard buffers of G devices, the gather to device 0 and the reassembly,
 *                                      as one library call without RCCL
 *   rt_group_render_frames          <- (new) rt_frames.run_frames plus the RCCL gather of cs420-ray-tracer_amd/rt_frames.py:
 *                                      a frame sequence on the group, batch b travelling to device 0 and being
 *                                      reassembled while the members render batch b+1
 *   rt_render_tiles                 <- the same for a list of tiles in one launch (the hybrid driver's GPU share)
 *   rt_render_tile                  <- launch_gpu_kernel's tile semantics  src/kernel.cu:185-200 (x = tile_x + ...,
 *                                      y = tile_y + ..., fb[y*W + x], kernel.cu:99-112), as main_hybrid.cpp:457-470
 *                                      calls it; float3 / Vec3 / RGB8 framebuffers
 *   rt_set_antialias                <- the `-a` flag of ray_gpu, src/main_gpu.cu:249-333, 363-370
 *   rt_get_info                     <- (new) the host-side builds the render calls made (camera grid,
 *                                      tile launch order) and their cost
 *   rt_get_ray_table_info / rt_set_ray_table
 *                                   <- (new) the ray table of the render launches: Camera::get_ray
 *                                      include/camera.h:17-25 formed once per orientation, not once per frame
 *   rt_trace_rays / rt_trace_rays_async / rt_trace_stats
 *                                   <- Scene::find_intersection include/scene.h:41-61 (closest hit) and the any-hit
 *                                      half of Scene::in_shadow include/scene.h:65-86 (occlusion), for rays the
 *                                      caller supplies; ray i is Ray(origin, direction), include/ray.h:12
 *   rt_camera_rays                  <- Camera::get_ray        include/camera.h:17-25, per pixel as
 *                                      src/main.cpp:150-153 calls it: the rays of a view, as rt_ray records
 *   rt_trace_paths / rt_trace_paths_async / rt_path_stats_get
 *                                   <- trace_ray without its colour arithmetic, src/main.cpp:16-58: per level
 *                                      the closest hit, Scene::in_shadow include/scene.h:65-86 per light as a
 *                                      bit mask, Sphere::normal_at include/sphere.h:62-64 and the reflection
 *                                      ray main.cpp:43-48, for rays the caller supplies
 *   rt_trace_radiance / rt_trace_radiance_async / rt_radiance_stats_get
 *                                   <- trace_ray, src/main.cpp:16-58, for rays the caller supplies
 *   rt_camera_sample_rays / rt_trace_radiance_resolve / rt_trace_radiance_resolve_async / rt_render_samples
 *                                   <- the four-sample loop of ray_gpu's `-a`, src/main_gpu.cu:249-333, for a
 *                                      sample pattern and weights the caller supplies
 *   rt_render_samples_async         <- (new) rt_render_samples' chunk loop, as one launch that forms its own rays
 *                                      and only enqueues
 *   rt_group_render_samples         <- (new) rt_render_samples of a frame, row-sharded over a device group as
 *                                      rt_group_render shards rt_render
 *   rt_camera_lens_rays / rt_render_lens_samples_async / rt_render_lens_samples / rt_group_render_lens_samples
 *                                   <- (new) a caller's own camera kernel for depth of field (the reference has
 *                                      a pinhole only, include/camera.h:17-25): rt_camera_sample_rays,
 *                                      rt_render_samples_async, rt_render_samples and rt_group_render_samples
 *                                      with each sample's ray leaving a point of a thin lens
 *   rt_set_light_samples / rt_group_set_light_samples
 *                                   <- (new) one rt_upload_scene with moved lights, one radiance call and a
 *                                      reduction of the caller's per sample (the reference has point lights only,
 *                                      include/scene.h:94-120): per-sample light positions for the multi-sample
 *                                      entries, i.e. area lights with soft shadows
 *   rt_set_gloss_samples / rt_group_set_gloss_samples, rt_scene_parse_roughness / rt_scene_load_roughness
 *                                   <- (new) per reflection level one rt_trace_paths, one rt_trace_radiance and a
 *                                      host pass that bends the reflection rays (the reference reflects as a
 *                                      perfect mirror, src/main.cpp:45-48, and drops the scene files' roughness
 *                                      column, include/scene_loader.h:66-70): glossy reflections for the
 *                                      multi-sample entries
 *   launch_gpu_kernel, upload_lights_and_ambience (include/rt_hip_compat.h)
 *                                   <- the same symbols of src/kernel.cu:185-207, link-compatible
 *
 * Errors: every call returns an rt_status (0 = ok); the library never exits
 * (the reference's CUDA_CHECK -> exit(1), src/main_gpu.cu:27-35, is not kept).
 * Threading: one rt_ctx per device per host thread; distinct contexts are
 * independent and may be used concurrently.
 * Streams: all device work of a context (renders, ray, path and radiance queries, rt_unpermute_rows) is
 * enqueued on ONE stream, the context's current stream, and is ordered only
 * on it.  The context's own stream (the default) is a BLOCKING stream: it is
 * ordered with the legacy NULL stream, so device buffers a caller fills or
 * reads on the NULL stream are ordered with the context's work.  A caller
 * that uses another stream of its own either passes it to rt_set_stream or
 * orders it against the context's stream itself.
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_HIP_ABI_VERSION 12 /* 4: the reference hybrid interface (rt_hip_compat.h); 5: rt_rows_for_shard;
                                   6: rt_render_tiles; 7: rt_get_info; 8: rt_info sphere-grid fields;
                                   9: rt_info behind-grid fields; 10: RT_ERR_CHECK;
                                   11: rt_info BVH / light-grid build times, scratch bytes;
                                   12: rt_info shadow_line_bounded; the rt_group_* entry points were added
                                   under 12 as well (new symbols only: nothing existing changed),
                                   and so were rt_group_render_frames, the ray queries (rt_trace_rays,
                                   rt_trace_rays_async, rt_trace_stats, rt_camera_rays) and the path queries
                                   (rt_trace_paths, rt_trace_paths_async, rt_path_stats_get) and the radiance
                                   queries (rt_trace_radiance, rt_trace_radiance_async, rt_radiance_stats_get) and the
                                   multi-sample entries (rt_camera_sample_rays, rt_trace_radiance_resolve,
                                   rt_trace_radiance_resolve_async, rt_render_samples) and their fused and
                                   group forms (rt_render_samples_async, rt_group_render_samples) and the
                                   thin-lens forms (rt_camera_lens_rays, rt_render_lens_samples_async,
                                   rt_render_lens_samples, rt_group_render_lens_samples) and the light table
                                   of the multi-sample entries (rt_set_light_samples,
                                   rt_group_set_light_samples) and their gloss table (rt_set_gloss_samples,
                                   rt_group_set_gloss_samples, rt_scene_parse_roughness,
                                   rt_scene_load_roughness) and rt_get_ray_table_info, rt_set_ray_table */
/* Longest reflection chain the GPU path keeps per pixel (depth <= RT_MAX_DEPTH). */
#define RT_MAX_DEPTH 64

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARG = 1,
    RT_ERR_NO_DEVICE = 2,
    RT_ERR_HIP = 3,          /* a HIP runtime call failed; see rt_last_error() */
    RT_ERR_OUT_OF_MEMORY = 4,
    RT_ERR_NO_SCENE = 5,     /* rt_render before rt_upload_scene */
    RT_ERR_IO = 6,           /* scene file could not be opened / image not written */
    RT_ERR_DEPTH = 7,        /* depth > RT_MAX_DEPTH */
    RT_ERR_CHECK = 8,        /* bounds-checked build (-DRT_CHECK) only: a device index into a host-built
                                structure was out of range; rt_last_error() names the site (rt_render_stats) */
} rt_status;

/* Sphere + Material, include/sphere.h:8-21.  reflectivity = the file's
 * "metallic" column (scene_loader.h:288); roughness is dropped as upstream. */
typedef struct rt_sphere {
    double center[3];
    double radius;
    double color[3];
    double reflectivity;
    double shininess;
} rt_sphere;

/* Light, include/scene.h:10-14 (intensity is parsed but unused, scene.h:117). */
typedef struct rt_light {
    double position[3];
    double color[3];
    double intensity;
} rt_light;

/* Scene + CameraConfig, include/scene.h:17-38. */
typedef struct rt_scene {
    int32_t num_spheres;
    int32_t num_lights;
    rt_sphere *spheres;
    rt_light *lights;
    double ambient[3];        /* default (0,0,0) */
    double cam_position[3];   /* default (0,0,0)   scene.h:22 */
    double cam_look_at[3];    /* default (0,0,-1)  scene.h:22 */
    double cam_fov;           /* default 60        scene.h:22 */
    int32_t has_camera;
    int32_t warnings;         /* records skipped by the parser */
} rt_scene;

/* Camera basis computed on the host (camera.h:10-15); scale = tan(fov*0.5*M_PI/180). */
typedef struct rt_camera {
    double position[3];
    double forward[3];
    double right[3];
    double up[3];
    double scale;
} rt_camera;

/* Which image rows a call renders.  Output row k (0 <= k < count) is image row
 *   y = (k / band) * band * stride + first * band + (k % band)
 * in PPM order (y = 0 is the TOP row, i.e. reference row j = H-1-y,
 * src/main.cpp:74).  Rows with y >= H are padding: they are written as zeros.
 * Full frame: {band=1, first=0, stride=1, count=H}.  Rank r of G GPUs with
 * cyclic bands of B rows: {B, r, G, ceil(ceil(H/B)/G)*B}. */
typedef struct rt_rows {
    int32_t band;
    int32_t first;
    int32_t stride;
    int32_t count;
} rt_rows;

/* The multi-GPU row layout every driver uses -- ray_hip --gpus G,
 * bench.py's torch.distributed ranks, rt_unpermute_rows: rank `rank` of
 * `num_shards` renders the cyclic bands of `band` rows rank, rank + G, ...;
 * every rank gets the same row count ceil(ceil(H / band) / G) * band (rows past
 * the image are padding).  Fails for band < 1, G < 1, rank outside [0, G). */
int rt_rows_for_shard(int height, int band, int rank, int num_shards, rt_rows *out);

/* Ray counts: primary = pixels traced; shadow = lights x shaded
 * hits (counted even when the GPU exits early); reflect = reflection rays
 * traced (reflective hit with depth-1 >= 1).  kernel_ms = HIP-event time of the
 * render kernel(s) on the context's stream. */
typedef struct rt_stats {
    uint64_t rays_primary;
    uint64_t rays_shadow;
    uint64_t rays_reflect;
    uint64_t negative_clamped; /* channels whose int(255.99*min(1,c)) < 0, stored as 0: RT_FB_RGB8 output only
                                  (RT_FB_F32X3 / RT_FB_F64X3 are unquantised and count 0).  A NaN channel is
                                  outside the contract ((int)NaN is undefined in the reference): the device
                                  stores 0 for it without counting it, an x86 host converts it to INT_MIN
                                  and counts it. */
    double kernel_ms;
    uint64_t tests_exact;      /* exact ray-sphere tests executed (sphere.h:26-59), live lanes only */
    uint64_t tests_cull;       /* sphere-vs-wave-bound tests (one per sphere per wave sweep) */
} rt_stats;

typedef struct rt_ctx rt_ctx;

/* ---- host-side scene / camera / image I/O (no GPU needed) ---------------- */
int rt_scene_load(const char *path, rt_scene *out, int verbose);
int rt_scene_parse(const char *text, rt_scene *out, int verbose);
void rt_scene_free(rt_scene *scene);
/* Column 9 ("roughness") of every `sphere` record that rt_scene_parse / rt_scene_load accept, in file order:
   the same reader, so out[i] belongs to scene.spheres[i] (rt_sphere has no field for it, as upstream's
   loader drops it).  *n_out: the number of accepted records; at most `capacity` values are written, and out
   may be NULL with capacity 0 (the sizing call).  Silent: the warnings are rt_scene_parse's to print.
   Errors: a NULL text / path / n_out, a negative capacity or a NULL out with capacity > 0
   RT_ERR_INVALID_ARG; a file that cannot be opened RT_ERR_IO.  What reads it: rt_set_gloss_samples. */
int rt_scene_parse_roughness(const char *text, double *out, int capacity, int *n_out);
int rt_scene_load_roughness(const char *path, double *out, int capacity, int *n_out);
int rt_camera_from_scene(const rt_scene *scene, rt_camera *out);
/* binary=0: P3 text byte-identical to write_ppm (src/main.cpp:69-91); binary=1: P6. */
int rt_write_ppm(const char *path, const uint8_t *rgb, int width, int height, int binary);
const char *rt_error_string(int status);
int rt_abi_version(void);

/* ---- device ------------------------------------------------------------- */
int rt_device_count(int *count);
int rt_create(int device, rt_ctx **out);
void rt_destroy(rt_ctx *ctx);
const char *rt_last_error(const rt_ctx *ctx);
/* Use an external stream (hipStream_t) for all later work of this context;
 * NULL restores the context's own (blocking) stream.  The switch is ordered:
 * work enqueued after it on the new stream waits for all work already
 * enqueued on the previous stream (the context's scratch buffers are shared
 * by every launch). */
int rt_set_stream(rt_ctx *ctx, void *hip_stream);
/* Per-wave conservative sphere culling (default on).  Off = every ray tests
 * every sphere (the reference's brute-force sweep, scene.h:47-58).  Output
 * bytes are identical either way; only the work differs. */
int rt_set_culling(rt_ctx *ctx, int enable);
/* Copies the scene into device memory owned by the context (replaces any
 * previous scene).  The host arrays may be freed afterwards. */
int rt_upload_scene(rt_ctx *ctx, const rt_scene *scene);

/* Synchronous render.  rgb_out: rows->count * width * 3 bytes, PPM row order
 * (see rt_rows).  out_on_device = 1 if rgb_out is device memory of this
 * context's device, 0 for host memory.  rows = NULL means the full frame.
 * stats may be NULL. */
int rt_render(rt_ctx *ctx, const rt_camera *cam, int width, int height, int depth, const rt_rows *rows,
              uint8_t *rgb_out, int out_on_device, rt_stats *stats);
/* Asynchronous render into DEVICE memory on the context's stream.  The kernels
 * are only enqueued, but host-side work can happen inside the call and then
 * wait for the context's stream first (work in flight may still read the
 * buffer being replaced):
 *   - the tile launch order (rt_sched), rebuilt when the view, the image or
 *     shard geometry or the scene changed since the previous launch (~0.1 ms);
 *   - the camera grid's cube-map tables and buffers, the first time a grid
 *     size is used.  The camera grids themselves (closest hits of camera rays)
 *     are built on the device ahead of the render kernel, per camera position,
 *     for a multi-frame launch (one grid per distinct position) or a one-frame
 *     launch at the previous launch's position (~0.05 ms, cached);
 *   - the sphere grids (closest hits of reflection rays; scenes of up to 2048
 *     spheres), built once per uploaded scene by its first multi-frame launch
 *     or its second launch: the call drains the stream, then builds them on
 *     the device and waits (~2 ms).
 * rt_get_info() reports all three.  rt_render_stats() waits for the stream and
 * returns the stats of the most recent rt_render_async. */
int rt_render_async(rt_ctx *ctx, const rt_camera *cam, int width, int height, int depth, const rt_rows *rows,
                    uint8_t *rgb_out_device);
int rt_render_stats(rt_ctx *ctx, rt_stats *stats);

/* Most frames one rt_render_frames_async launch renders. */
#define RT_MAX_FRAMES 32
/* Asynchronous render of `nframes` frames (1..RT_MAX_FRAMES) of the uploaded
 * scene in ONE kernel launch, frame f seen through cams[f]: a frame sequence
 * of the per-frame pixel loop src/main.cpp:146-157, each frame exactly what
 * rt_render_async(ctx, &cams[f], ...) writes, into DEVICE memory at
 * rgb_out_device + f * frame_stride (frame_stride >= rows' count * width * 3
 * bytes).  The tiles of all frames share one launch, so the long reflection
 * chains of one frame overlap the others' work instead of each frame ending
 * on its slowest tiles.  Counts as ONE launch for rt_kernel_times; the stats
 * of rt_render_stats are the sums over its frames.  The context's scratch
 * (reflection stack, deferred-ray queue) grows to the largest launch seen, so
 * launches of as many frames or fewer do not re-allocate: render the largest
 * batch once before timing a sequence. */
int rt_render_frames_async(rt_ctx *ctx, const rt_camera *cams, int nframes, int width, int height, int depth,
                           const rt_rows *rows, uint8_t *rgb_out_device, size_t frame_stride);

/* Durations (ms, HIP events recorded in-stream around each render kernel) of
 * the render launches issued since the previous call, oldest first, at most
 * max_n (and at most the 256 most recent).  Waits for the context stream. */
int rt_kernel_times(rt_ctx *ctx, double *ms_out, int max_n, int *n_out);

/* Framebuffer formats of rt_render_tile. */
#define RT_FB_RGB8 0  /* uint8 RGB, width*height*3, PPM row order (top row first), quantised as write_ppm */
#define RT_FB_F32X3 1 /* float RGB per pixel at index y*width + x, y = 0 the BOTTOM row: the reference's
                         d_framebuffer of launch_gpu_kernel (kernel.cu:112), unquantised */
#define RT_FB_F64X3 2 /* double RGB (Vec3) per pixel, same indexing: the serial framebuffer, main.cpp:156.
                         Numerically the reference's; a zero channel may differ in sign: a hit of
                         reflectivity > 1 with no depth left stores col*(1-refl) = -0.0 where the
                         reference adds (0,0,0)*refl and has +0.0 */

/* launch_gpu_kernel (src/kernel.cu:185-200) with its tile semantics: renders
 * pixels x in [tile_x, tile_x + tile_w), y in [tile_y, tile_y + tile_h)
 * (clipped to the image; y counts from the bottom row, v = y/(H-1)) into a
 * full-image DEVICE framebuffer of the given format; other pixels are not
 * touched.  Asynchronous on the context stream, like the reference; the
 * caller synchronises (rt_render_stats waits and returns this tile's counts).
 * The colours are the serial path's (fp64, A1-A13), not the reference CUDA
 * kernel's fp32 approximation. */
int rt_render_tile(rt_ctx *ctx, const rt_camera *cam, int image_width, int image_height, int depth, int tile_x,
                   int tile_y, int tile_width, int tile_height, int fb_format, void *fb_device);

/* One launch_gpu_kernel tile (kernel.cu:185-200): pixels x in [x, x + width),
 * framebuffer rows j in [y, y + height) (j = 0 the bottom row). */
typedef struct rt_tile {
    int32_t x, y, width, height;
} rt_tile;

/* Many tiles in ONE launch (a hybrid driver's GPU share of a frame,
 * main_hybrid.cpp:457-470 / 535-548, without a launch and a sync per tile):
 * every 8x8-pixel block of the image that overlaps a tile is rendered into the
 * full-image DEVICE framebuffer exactly as rt_render_tile renders it, so the
 * tiles' pixels are rt_render_tile's; the other pixels of those blocks are
 * written too (with their own colours), all others are not touched.
 * Asynchronous on the context stream; waits for the stream first when the
 * context's block list is still in use. */
int rt_render_tiles(rt_ctx *ctx, const rt_camera *cam, int image_width, int image_height, int depth,
                    const rt_tile *tiles, int num_tiles, int fb_format, void *fb_device);

/* Samples per pixel for later renders: 1 (default, the serial path) or 4 (the
 * reference GPU's `-a` antialias mode, main_gpu.cu:249-333: offsets
 * (0,0) (0.5,0) (0,0.5) (0.5,0.5) added to (x, y) before u = x/(W-1),
 * v = y/(H-1); the 4 colours summed in that order and scaled by 1/4, all in
 * the serial fp64 semantics).  Ray counts include every sample. */
int rt_set_antialias(rt_ctx *ctx, int samples);

/* Host-side work of the render calls since rt_create (see rt_render_async). */
typedef struct rt_info {
    int32_t cam_grid_last;       /* 1: the most recent launch traced its camera rays on a camera grid */
    int32_t cam_grid_n;          /* its cells per cube-map face edge (0: none) */
    uint64_t cam_grid_builds;    /* camera grids built */
    double cam_grid_build_ms;    /* host wall time of those builds (incl. the stream wait and the upload) */
    uint64_t tile_order_builds;  /* tile launch orders built */
    double tile_order_build_ms;  /* host wall time of those builds */
    double upload_ms;            /* host wall time of the most recent rt_upload_scene (BVH, light grids, copies) */
    uint64_t launches;           /* render launches enqueued */
    int32_t sphere_grids;        /* spheres with a sphere grid (reflection rays' closest hit; 0: none) */
    int32_t sphere_grid_n;       /* their cells per cube-map face edge */
    uint64_t sphere_grid_entries;  /* list entries of all sphere grids (8 bytes each) */
    double sphere_grid_build_ms; /* host wall time of their build (by the scene's first multi-frame or second launch) */
    int32_t behind_grid;         /* 1: the scene has a behind grid (closest-hit lines' part behind their origin) */
    int32_t behind_grid_last;    /* 1: the most recent launch's BVH walks used it */
    uint64_t behind_grid_cells;  /* its cells */
    uint64_t behind_grid_entries;  /* its list entries (20 bytes each) */
    double behind_grid_build_ms; /* host wall time of its build, part of upload_ms */
    double bvh_build_ms;         /* host wall time of the BVH build and upload, part of upload_ms */
    double light_grid_build_ms;  /* host wall time of the light grids' build and upload, part of upload_ms */
    uint64_t scratch_bytes;      /* device scratch the context holds for its launches: reflection stacks (stack
                                    homes / per-pixel stack), the deferred queue, the camera grids, the tile order,
                                    the ray table */
    int32_t shadow_line_bounded; /* 1: the scene's bound keeps every shadow line within its light grid's margin, so
                                    the per-ray check is skipped (rt_device.h shadow_cells off_free); 0: checked */
    int32_t reserved0;
} rt_info;
int rt_get_info(rt_ctx *ctx, rt_info *out);

/* The ray table of the whole-image render launches (rt_render, rt_render_async, rt_render_frames_async and
 * the rt_group renders; not rt_render_tile(s), the antialias mode or the query and sample families).  A
 * camera ray's direction depends only on the camera's orientation (forward, right, up, scale), the image
 * size and the launch's rows -- not on the scene, the camera's position or the frame -- so a launch whose
 * frames share them forms the directions once, in a device pass ahead of
 * the render kernel and inside the launch's timing, 24 bytes per launch pixel, and the context keeps the
 * table until a launch with another orientation, size or rows replaces it.  A table is
 * built by a launch of two frames or more and by a one-frame launch that repeats the previous launch's
 * orientation, size and rows; any other launch forms its rays in the render kernel, as does one whose
 * table would take more than 1 GiB or half the free device memory.  The pixels are the same bytes either
 * way.  rt_set_ray_table(ctx, mode, budget_bytes) sets the rule for the context's later launches: mode 0
 * never uses a table, 1 is the rule above (default), 2 builds one for a first one-frame launch too;
 * budget_bytes is the most a table may take (negative: the default of 1 GiB; 0: every launch forms its rays
 * in the kernel).  It is a call, not an environment variable: the library reads RT_HIP_LDS_SCENE and
 * RT_HIP_CAM_GRID from the environment and nothing else.  rt_info.scratch_bytes counts the table. */
typedef struct rt_ray_table_info {
    uint64_t builds;    /* tables built since rt_create */
    int32_t used_last;  /* 1: the most recent launch read its camera rays from a table */
    int32_t reserved0;
    uint64_t bytes;     /* device memory the context holds for the table */
    double build_ms;    /* host wall time of enqueueing those builds */
} rt_ray_table_info;
int rt_get_ray_table_info(rt_ctx *ctx, rt_ray_table_info *out);
int rt_set_ray_table(rt_ctx *ctx, int mode, int64_t budget_bytes); /* RT_ERR_INVALID_ARG: no context, mode not 0..2 */

/* Reassemble G shards gathered rank-major ([G][rows_per_rank][W][3], rank r
 * rendered with rt_rows{band, r, G, rows_per_rank}) into a PPM-ordered
 * [H][W][3] image.  Both pointers are device memory; runs on the ctx stream. */
int rt_unpermute_rows(rt_ctx *ctx, const uint8_t *gathered_device, uint8_t *image_device, int width, int height,
                      int band, int num_shards, int rows_per_shard);

/* ---- ray queries: closest hit and occlusion for the caller's rays ----------
 * The questions the render loop asks the scene, asked directly: "which sphere
 * does this ray hit, and where" (Scene::find_intersection, scene.h:41-61) and
 * "is anything between these two points" (the any-hit half of Scene::in_shadow,
 * scene.h:65-86), in the reference's fp64 semantics, bit for bit.  The path
 * queries below return a ray's whole reflection path, the radiance queries
 * after them its colour.
 * Queries are launches of their own: they have their own events and counters,
 * are not listed by rt_kernel_times, do not change what rt_render_stats or
 * rt_get_info report, and use none of the render scratch. */
typedef struct rt_ray {          /* 64 bytes */
    double origin[3];
    double direction[3];         /* any length; normalised once by the library, as Ray(o, d) does (ray.h:12, vec3.h:19-20) */
    double tmax;                 /* occlusion limit along the normalised direction; +inf = none */
    double reserved;             /* ignored */
} rt_ray;
typedef struct rt_hit {          /* 16 bytes */
    double  t;                   /* closest mode: find_intersection's t; 1e20 on a miss (scene.h:42) */
    int32_t sphere;              /* closest mode: its sphere index in file order; -1 on a miss */
    int32_t occluded;            /* 1: some sphere reports a hit with t < 1e20 and t < tmax, else 0 */
} rt_hit;
#define RT_QUERY_CLOSEST  0      /* t, sphere and occluded */
#define RT_QUERY_OCCLUDED 1      /* occluded only (may stop at the first occluder); t = 1e20, sphere = -1 */
typedef struct rt_query_stats {
    uint64_t rays, hits;         /* hits: sphere >= 0 (closest) / occluded == 1 (occluded mode) */
    uint64_t tests_exact, tests_cull;   /* as rt_stats */
    uint64_t rays_unaccelerated; /* rays answered by the every-sphere sweep: origin outside the query region (or
                                    not finite), direction not finite once normalised, or culling switched off */
    double   kernel_ms;          /* HIP-event time of the query kernel */
} rt_query_stats;
/* Ray i is the reference's Ray(origin, direction): d = direction.normalized(), once.  Closest mode scans
   in file order with strict < from 1e20 (ties keep the lowest index); the disc == 0 tangent root is kept
   even when negative (sphere.h:42-47); a NaN t is never recorded.  `occluded` is in_shadow's test with tmax
   in place of the light distance (a NaN tmax gives 0; a negative tmax can still be beaten by a negative
   tangent root).  A zero, NaN or infinite ray is a miss in both modes, never an error.
   The walks' margins are sized for the query region: the scene's bounding box grown on every side by its
   own diagonal.  Rays starting outside it test every sphere instead (rays_unaccelerated): the results are
   exact everywhere, only the speed depends on the region.  rt_set_culling(ctx, 0) makes every ray do so.
   rays_device / hits_device: device memory of the context's device, 16-byte aligned, n records each.
   n == 0 is a no-op (RT_OK); n > 2^31-1, a NULL pointer with n > 0 or an unknown mode is
   RT_ERR_INVALID_ARG (before any HIP call); no uploaded scene is RT_ERR_NO_SCENE.
   Asynchronous on the context's current stream, ordered as every other launch of the context. */
int rt_trace_rays_async(rt_ctx *ctx, int mode, const rt_ray *rays_device, size_t n, rt_hit *hits_device);
/* Synchronous; rays / hits in host memory, or (on_device = 1) device memory as above; stats may be NULL. */
int rt_trace_rays(rt_ctx *ctx, int mode, const rt_ray *rays, size_t n, rt_hit *hits, int on_device,
                  rt_query_stats *stats);
/* Waits for the stream; the counts and time of the most recent query launch (zeros before the first). */
int rt_trace_stats(rt_ctx *ctx, rt_query_stats *stats);
/* The camera rays of a view as rt_ray records in DEVICE memory (16-byte aligned, rows->count * width of
   them; rows = NULL means the full frame): for output row k of `rows` and column x, rays[k*width + x] is the
   ray get_ray hands to Ray() -- origin = cam->position, direction = the once-normalised
   forward + right*((u-0.5)*scale) + up*((v-0.5)*scale), u = x/(W-1), v = j/(H-1), j = H-1-y (camera.h:17-25,
   main.cpp:150-153), tmax = +inf, reserved = 0 -- by the arithmetic of the render kernels' own primary
   rays.  rt_trace_rays normalises the direction a second time, as Ray() does.  Padding rows (y >= H) get
   all-zero rays.  Needs no scene.  Asynchronous on the context's stream. */
int rt_camera_rays(rt_ctx *ctx, const rt_camera *cam, int width, int height, const rt_rows *rows,
                   rt_ray *rays_device);

/* ---- path queries: reflection paths and shadow masks for the caller's rays --
 * Everything trace_ray (src/main.cpp:16-58) does for a ray except the colour arithmetic: per reflection
 * level the closest hit, per light whether Scene::in_shadow says shadowed, and the reflection decision --
 * the geometric skeleton of the ray's path, in the reference's fp64 semantics, bit for bit.  No colour is
 * formed here: a caller shades from these records with a model of its own, or asks
 * rt_trace_radiance below for the reference's. */
#define RT_PATH_MAX_LIGHTS 64            /* bits of rt_vertex.shadowed */
#define RT_VERTEX_TRACED   1             /* this level's ray was traced */
#define RT_VERTEX_REFLECTS 2             /* a reflection ray was spawned: the next level is traced */
typedef struct rt_vertex {               /* 32 bytes */
    double   t;          /* find_intersection's t of this level's ray; 1e20 on a miss or an untraced level */
    int32_t  sphere;     /* file-order index; -1 on a miss or an untraced level */
    int32_t  flags;      /* RT_VERTEX_*; 0 for an untraced level */
    uint64_t shadowed;   /* bit l: Scene::in_shadow(hit, lights[l]) is true; 0 on a miss / untraced level */
    uint64_t reserved;   /* written as 0 */
} rt_vertex;
typedef struct rt_surface {              /* 96 bytes; optional output */
    double dir[3];       /* the direction stored in this level's Ray (after Ray()'s normalisation) */
    double hit[3];       /* ray.origin + ray.direction * t        main.cpp:32 */
    double normal[3];    /* spheres[sphere].normal_at(hit)        sphere.h:62-64 */
    double view[3];      /* (ray.origin - hit).normalized()       main.cpp:38 */
} rt_surface;
typedef struct rt_path_stats {
    uint64_t rays;           /* input rays */
    uint64_t segments;       /* levels traced, over all rays (level 0 included) */
    uint64_t hits;           /* traced levels that hit a sphere */
    uint64_t shadow_rays;    /* in_shadow calls: hits x lights */
    uint64_t tests_exact, tests_cull;   /* as rt_stats */
    uint64_t unaccelerated;  /* closest-hit and shadow queries answered by the every-sphere sweep */
    double   kernel_ms;      /* HIP-event time of the path kernel */
} rt_path_stats;
/* depth is trace_ray's: 1..RT_MAX_DEPTH levels.  Level 0 is Ray(origin, direction) of rays[i], the direction
   normalised once as rt_trace_rays does; rt_ray.tmax and reserved are ignored.
   A traced level k: the closest hit exactly as RT_QUERY_CLOSEST, and on a hit, for every light l in file
   order, bit l of `shadowed` is the whole of in_shadow (scene.h:65-86): to_light = L - hit, dist its length,
   ldir = to_light.normalized(), Ray(hit + ldir*EPSILON, ldir) with the direction normalised again by Ray(),
   shadowed when find_intersection finds a sphere and t < dist.  A light at the hit point gives a NaN
   direction and is not shadowed.
   Level k+1 is traced iff level k hit a sphere with reflectivity > 0 and depth - (k+1) >= 1; its ray is
   Ray(hit + normal*EPSILON, d - normal*2.0*dot(d, normal)) (main.cpp:45-48) and level k carries
   RT_VERTEX_REFLECTS.  A zero, NaN or infinite ray is a traced miss at level 0, never an error.
   Layout, level-major: verts[k*n + i] and surf[k*n + i], depth*n records each, 16-byte aligned device
   memory.  Every rt_vertex of every level is written; untraced levels get {1e20, -1, 0, 0, 0}.  An
   rt_surface is written only for traced levels (on a traced miss: dir, then zeros); surfaces of untraced
   levels are not touched.  surf == NULL: no surface is computed or written.
   Errors, before any HIP call: n == 0 is RT_OK and a no-op; n > 2^31-1, a NULL rays / verts with n > 0 or
   depth < 1 is RT_ERR_INVALID_ARG; depth > RT_MAX_DEPTH is RT_ERR_DEPTH; no uploaded scene is
   RT_ERR_NO_SCENE; an uploaded scene of more than RT_PATH_MAX_LIGHTS lights is RT_ERR_INVALID_ARG.
   Per traced segment and per shadow ray the acceleration rule of rt_trace_rays holds: the culled sweep and
   the walks when the origin lies in the query region, the normalised direction is finite and culling is on,
   else the every-sphere sweep (`unaccelerated`); results are exact everywhere.  Shadow queries do not use
   the light grids (their margins belong to renders), nor does anything here use camera or sphere grids.
   Path launches have their own events and counters: they are not listed by rt_kernel_times and change
   nothing that rt_render_stats, rt_get_info or rt_trace_stats report.
   Asynchronous on the context's current stream, ordered as every other launch of the context. */
int rt_trace_paths_async(rt_ctx *ctx, const rt_ray *rays_device, size_t n, int depth, rt_vertex *verts_device,
                         rt_surface *surf_device /* nullable */);
/* Synchronous; rays / verts / surf in host memory, or (on_device = 1) device memory as above; stats may be NULL. */
int rt_trace_paths(rt_ctx *ctx, const rt_ray *rays, size_t n, int depth, rt_vertex *verts,
                   rt_surface *surf /* nullable */, int on_device, rt_path_stats *stats /* nullable */);
/* Waits for the stream; the counts and time of the most recent path launch (zeros before the first). */
int rt_path_stats_get(rt_ctx *ctx, rt_path_stats *stats);

/* ---- radiance queries: trace_ray's colour for the caller's rays -------------
 * The last thing trace_ray (src/main.cpp:16-58) does with a ray: the path above, shaded at every hit by
 * Scene::shade (include/scene.h:89-121) and composited -- a renderer for ray sets of the caller's own
 * (fisheye or panoramic cameras, depth of field, supersampling patterns, light probes). */
typedef struct rt_radiance_stats {       /* 72 bytes */
    uint64_t rays, segments, hits, shadow_rays;   /* as rt_path_stats */
    uint64_t tests_exact, tests_cull, unaccelerated;
    uint64_t negative_clamped;           /* RT_FB_RGB8 only, as rt_stats.negative_clamped */
    double   kernel_ms;                  /* HIP-event time of the radiance kernel */
} rt_radiance_stats;
/* out[i] = trace_ray(Ray(origin_i, direction_i), scene, depth): the direction normalised once as
   rt_trace_rays does; rt_ray.tmax and reserved are ignored; depth is trace_ray's, 1..RT_MAX_DEPTH.
   Per level: the closest hit exactly as RT_QUERY_CLOSEST; a miss gets the sky (main.cpp:28-29); a hit gets
   Scene::shade over ALL lights in file order, each with the whole of in_shadow as rt_trace_paths describes
   it -- there is no RT_PATH_MAX_LIGHTS limit, because there is no mask.  The reflection decision and the
   reflection ray are rt_trace_paths'; the levels are composited innermost first,
   shade*(1-refl) + below*refl (main.cpp:54).
   The arithmetic is the render kernels' own -- the Phong terms and specular + diffuse + colour in their
   operand order, pow(+0, shininess > 0) skipped, the specular power by the render's routines, no
   contraction -- so the radiance of a camera ray is the RT_FB_F64X3 value rt_render_tile stores for its
   pixel.  The note on RT_FB_F64X3 applies: numerically the reference's, but a zero channel may differ in
   sign (a hit of reflectivity > 1 with no depth left stores col*(1-refl) = -0.0).
   A zero, NaN or infinite ray is a traced miss at level 0: its sky colour comes from the NaN direction.
   It is never an error.
   fb_format selects the packed record, ray i at record i: RT_FB_F64X3 3 doubles; RT_FB_F32X3 3 floats,
   converted as the render's F32X3 store converts; RT_FB_RGB8 3 bytes through write_ppm's quantiser
   (main.cpp:85-87), a negative value stored as 0 and counted in negative_clamped as rt_stats documents; a
   NaN channel passes std::min(1.0, c) as 1.0, so it is stored as 255, the reference's own byte, and not
   counted.  There is no row flip in any format: rt_camera_rays emits PPM order,
   so rt_camera_rays + rt_trace_radiance(RT_FB_RGB8) writes rt_render's bytes.
   rt_set_antialias does not apply (the samples are the caller's rays).  The acceleration rule per segment
   and per shadow ray is rt_trace_paths' (`unaccelerated`); rt_set_culling(ctx, 0) sends every query
   through the every-sphere sweep.  Light, camera and sphere grids are not used.
   rays_device / out_device: memory of the context's device, 16-byte aligned, n records each.
   Errors, before any HIP call: n == 0 is RT_OK and a no-op; n > 2^31-1, a NULL rays / out with n > 0,
   depth < 1, an unknown fb_format or a misaligned device pointer is RT_ERR_INVALID_ARG;
   depth > RT_MAX_DEPTH is RT_ERR_DEPTH; no uploaded scene is RT_ERR_NO_SCENE.
   Radiance launches have their own events, counters and scratch (a reflection stack bounded by the
   launch's grid, not by n): they are not listed by rt_kernel_times, change nothing that rt_render_stats,
   rt_get_info, rt_trace_stats or rt_path_stats_get report, and use none of the render scratch.
   Asynchronous on the context's current stream, ordered as every other launch of the context. */
int rt_trace_radiance_async(rt_ctx *ctx, const rt_ray *rays_device, size_t n, int depth, int fb_format,
                            void *out_device);
/* Synchronous; rays / out in host memory (staged through grow-only buffers of the context), or
   (on_device = 1) device memory as above; stats may be NULL. */
int rt_trace_radiance(rt_ctx *ctx, const rt_ray *rays, size_t n, int depth, int fb_format, void *out,
                      int on_device, rt_radiance_stats *stats /* nullable */);
/* Waits for the stream; the counts and time of the most recent radiance launch (zeros before the first). */
int rt_radiance_stats_get(rt_ctx *ctx, rt_radiance_stats *stats);

/* ---- multi-sample pixels: a caller's sample pattern, resolved on the device --
 * The `-a` mode of ray_gpu (src/main_gpu.cu:249-333: four samples per pixel, summed in order and scaled
 * by 0.25) for any pattern of up to RT_MAX_SAMPLES samples and any weights, on the query side: nothing
 * here touches a render kernel or rt_set_antialias. */
#define RT_MAX_SAMPLES 64
/* Replaces a host restatement of camera_dir for sub-pixel samples (rt_camera_rays emits one ray per pixel,
   at its corner).  samples rays per pixel as rt_ray records in DEVICE memory (16-byte aligned,
   rows->count * width * samples of them; rows = NULL means the full frame), pixel-major with a pixel's
   samples consecutive: the ray of output row k, column x, sample s is rays[(k*width + x)*samples + s].
   origin = cam->position; direction = normalized(camera_dir(cam, (double)x + ox_s, (double)j + oy_s, W, H)),
   j = H-1-y and (ox_s, oy_s) = offsets_xy[2s], offsets_xy[2s+1]: the antialias arithmetic of the render
   kernels (main_gpu.cu:253-256), the offset added to (x, j) BEFORE the division by W-1 and H-1;
   tmax = +inf, reserved = 0.  Padding rows (y >= H) get all-zero rays.  With samples = 1 and the offset
   (0, 0) the records are bit-identical to rt_camera_rays' (x + 0.0 == x).
   offsets_xy is HOST memory, 2*samples doubles, read during the call and passed to the kernel by value: it
   may be freed on return.  Any double is allowed: a non-finite offset gives a NaN ray, which the queries
   treat as a miss; it is never an error.  Needs no scene.  Asynchronous on the context's stream.
   Errors, before any HIP call, all RT_ERR_INVALID_ARG: samples outside 1..RT_MAX_SAMPLES; a NULL
   offsets_xy, cam or rays_device; a misaligned rays_device; rows->count * width * samples > 2^31-1. */
int rt_camera_sample_rays(rt_ctx *ctx, const rt_camera *cam, int width, int height, const rt_rows *rows,
                          const double *offsets_xy /* host, 2*samples doubles */, int samples,
                          rt_ray *rays_device);
/* Replaces rt_trace_radiance(RT_FB_F64X3) of n_pixels*samples rays followed by a reduction and a quantiser
   of the caller's own (24 B per sample through memory and back).  Input: n_pixels * samples rays, pixel
   p's samples at rays[p*samples .. p*samples + samples - 1].  c_s is exactly what rt_trace_radiance
   computes for that ray: the once-normalised direction, depth, acceleration rule, culling switch and
   arithmetic are the same.  Pixel p's value, S = samples:
     weights == NULL, S == 1: c_0 itself, bit for bit -- the call equals rt_trace_radiance (trace_tile's
                              one-sample rule; a -0.0 channel stays -0.0);
     weights == NULL, S > 1:  acc = (0,0,0); acc = acc + c_s for s = 0..S-1 in that order; the value is
                              acc * inv, inv = 1.0 / S formed once in fp64 on the host (for S = 4 the
                              render's scale(acc, 0.25));
     weights != NULL, S >= 1: acc = (0,0,0); acc = acc + c_s * w_s in order, the product rounded, then the
                              sum rounded, no contraction and no final scale: the caller normalises the
                              weights (HOST memory, S doubles, read during the call).
   Record p is written in fb_format exactly as rt_trace_radiance writes a record: RT_FB_F64X3 / RT_FB_F32X3
   convert as the render's store does; RT_FB_RGB8 goes through write_ppm's quantiser, a negative channel
   stored as 0 and counted in negative_clamped, a NaN stored as 255 and not counted.  No row flip.
   A zero, NaN or infinite ray is a traced miss whose colour comes from the NaN direction: it makes its
   pixel NaN and touches no other pixel.
   These are radiance launches: they use the context's radiance events, counters, reflection stack and
   staging buffers, and rt_radiance_stats_get reports the most recent launch of either kind, with
   rays = n_pixels*S and segments, hits, shadow_rays and unaccelerated counting every sample.  They change
   nothing that rt_render_stats, rt_kernel_times, rt_get_info, rt_trace_stats or rt_path_stats_get report.
   Errors: those of rt_trace_radiance (with n = n_pixels), and as RT_ERR_INVALID_ARG samples outside
   1..RT_MAX_SAMPLES and n_pixels * samples > 2^31-1.  n_pixels == 0 is a no-op.
   rays_device / out_device: device memory, 16-byte aligned; asynchronous on the context's stream. */
int rt_trace_radiance_resolve_async(rt_ctx *ctx, const rt_ray *rays_device, size_t n_pixels, int samples,
                                    const double *weights /* host, samples doubles; NULL = box */,
                                    int depth, int fb_format, void *out_device);
/* Synchronous; rays / out in host memory (staged through the radiance queries' grow-only buffers), or
   (on_device = 1) device memory as above; stats may be NULL. */
int rt_trace_radiance_resolve(rt_ctx *ctx, const rt_ray *rays, size_t n_pixels, int samples,
                              const double *weights, int depth, int fb_format, void *out, int on_device,
                              rt_radiance_stats *stats /* nullable */);
/* Replaces rt_set_antialias(4) + rt_render for a pattern of the caller's: rt_camera_sample_rays followed by
   rt_trace_radiance_resolve, in chunks of whole output rows.  Synchronous.  Writes the pixels of `rows`
   (NULL = the full frame) in PPM row order in every format, record k*width + x, to host memory or
   (out_on_device = 1) device memory, 16-byte aligned.  The context's grow-only ray buffer never exceeds
   max_ray_bytes (one output row is the minimum); 0 means the default of 256 MiB.
   Padding rows (a suffix of the output rows of an rt_rows) are not traced or counted; their records are
   written as zero bytes.  So with the offsets (0,0) (.5,0) (0,.5) (.5,.5), box weights and RT_FB_RGB8,
   every shard of an image is byte for byte rt_render's under rt_set_antialias(4).
   stats: the counts summed over the call's chunk launches; kernel_ms the sum of the chunks' resolve-kernel
   event times (ray generation is not in it).  rt_set_antialias does not apply to this call.
   Errors: as rt_camera_sample_rays and rt_trace_radiance_resolve, except that the ray limit is tested
   against width * samples (one output row, the smallest chunk), not rows->count * width * samples:
   max_ray_bytes is what bounds the ray buffer. */
int rt_render_samples(rt_ctx *ctx, const rt_camera *cam, int width, int height, int depth,
                      const rt_rows *rows /* NULL = full frame */, const double *offsets_xy, int samples,
                      const double *weights /* nullable */, int fb_format, void *out, int out_on_device,
                      size_t max_ray_bytes /* 0 = default */, rt_radiance_stats *stats /* nullable */);
/* Replaces rt_render_samples' host loop (a ray-generator launch, a resolving launch and a host wait per
   chunk of rows) with ONE launch that only enqueues: every lane forms its pixel's sample rays itself, so
   there is no ray buffer, no chunk and no max_ray_bytes.  Writes to out_device (device memory, 16-byte
   aligned) exactly the records rt_render_samples(..., out_on_device = 1, ...) writes for the same
   arguments, bit for bit, in the three formats: the ray arithmetic (rt_camera_sample_rays' direction,
   normalised once more), the resolve rule, the quantiser, the NaN -> 255 rule and the -0.0 rule of one
   unweighted sample are the same.
   The real rows of `rows` (NULL = the full frame) are one radiance launch on the context's current
   stream; the padding rows, a suffix of the output rows, are not traced or counted and are zeroed by a
   hipMemsetAsync on the same stream.  The call never waits.  offsets_xy and weights are HOST memory, read
   during the call and free on return.
   It uses the radiance queries' events, counters and reflection stack, but not their ray staging, which
   it neither touches nor grows.  rt_radiance_stats_get afterwards reports this launch for the whole call:
   rays = real pixels * samples, kernel_ms this one kernel.  A call without a real row launches nothing
   and leaves that report as it was.  As every radiance launch it changes nothing that rt_render_stats,
   rt_kernel_times, rt_get_info, rt_trace_stats or rt_path_stats_get report; rt_set_antialias does not
   apply.
   Errors, before any HIP call: rt_render_samples' (arguments, width * samples > 2^31-1, the format, the
   depth, then the scene), and as RT_ERR_INVALID_ARG a NULL or misaligned out_device and
   rows->count * width > 2^31-1 (the limit is on the pixels of the one launch; the rays may pass 2^31).
   The kernel counts per lane in 32 bits: a launch in which one lane could pass 2^32-1 --
   trips * samples * depth * (1 + lights), trips the lane's pixels at the launch's grid (at most 64 waves
   per CU; 2080 waves at depth 64) -- is RT_ERR_INVALID_ARG as well: on a 256-CU device 2^31-1 pixels of
   64 samples at depth 64 pass it with up to 63 lights, a 4K frame of them with more than 16,000.
   rows->count == 0 is RT_OK and a no-op. */
int rt_render_samples_async(rt_ctx *ctx, const rt_camera *cam, int width, int height, int depth,
                            const rt_rows *rows /* NULL = full frame */, const double *offsets_xy, int samples,
                            const double *weights /* nullable */, int fb_format, void *out_device);

/* ---- samples through a thin lens (depth of field) ---------------------------
   One definition for the four entries below.  Per sample s the caller gives the pixel offset (ox_s, oy_s)
   as above and a LENS POINT (lx_s, ly_s) = lens_xy[2s], lens_xy[2s+1], in scene units along cam->right and
   cam->up; per call one FOCUS distance, along cam->forward from cam->position to the plane that stays
   sharp.  With P = cam->position, R = cam->right, U = cam->up and no contraction:
     dir0 = camera_dir(cam, (double)x + ox_s, (double)j + oy_s, W, H)    unnormalised, forward component 1
     lv   = R*lx_s + U*ly_s
     o    = P + lv                                                       the record's origin
     dir  = normalized(dir0*focus - lv)                                  the record's direction
   and the record is {o, dir, tmax = +inf, reserved = 0}; a query normalises dir once more, as Ray() does.
   Rays of one pixel and offset from different lens points meet at P + dir0*focus.  Sample s pairs offset s
   with lens point s: decorrelating the two is the caller's job.  Any double is allowed: a non-finite lens
   point or focus gives NaN rays, which the queries treat as misses; it is never an error.  With every lens
   point (0, 0) and focus = 1.0 the rays are rt_camera_sample_rays' as values (a zero component may differ
   in sign).  lens_xy is HOST memory, 2*samples doubles, read during the call and free on return. */

/* Replaces a caller's own lens-camera kernel (or host loop) in front of the radiance queries:
   rt_camera_sample_rays with the lens.  The same layout (rays[(k*width + x)*samples + s]), the same
   all-zero rays for padding rows, asynchronous on the context's stream, needs no scene.
   Errors: rt_camera_sample_rays'; a NULL lens_xy is RT_ERR_INVALID_ARG as well. */
int rt_camera_lens_rays(rt_ctx *ctx, const rt_camera *cam, int width, int height, const rt_rows *rows,
                        const double *offsets_xy /* host, 2*samples doubles */,
                        const double *lens_xy /* host, 2*samples doubles */, double focus, int samples,
                        rt_ray *rays_device);
/* Replaces rt_camera_lens_rays into a ray buffer of the caller's (64 bytes per sample, chunked by the
   caller) followed by rt_trace_radiance_resolve_async: rt_render_samples_async with the lens.  ONE launch,
   no ray buffer, never waits.  Writes to out_device exactly the records that pair of calls writes, bit for
   bit, in the three formats.  Everything else is rt_render_samples_async's: the padding rows zeroed by a
   hipMemsetAsync, the radiance family's events, counters and reflection stack and none of its staging, the
   report of rt_radiance_stats_get, the order of the errors and the 32-bit per-lane counter check (the lens
   changes no trip, sample, depth or light count).  A NULL lens_xy is RT_ERR_INVALID_ARG as well. */
int rt_render_lens_samples_async(rt_ctx *ctx, const rt_camera *cam, int width, int height, int depth,
                                 const rt_rows *rows /* NULL = full frame */, const double *offsets_xy,
                                 const double *lens_xy, double focus, int samples,
                                 const double *weights /* nullable */, int fb_format, void *out_device);
/* Replaces rt_render_lens_samples_async, a device-to-host copy and a wait written by the caller: the
   synchronous form.  out is host memory or (out_on_device = 1) device memory, 16-byte aligned.  The fused
   launch, for host memory into the radiance family's grow-only `out` staging with one hipMemcpyAsync back,
   and ONE wait.  There is no max_ray_bytes: there is no ray buffer.  stats (nullable) are that launch's
   (rt_radiance_stats_get's); zeros when no row of `rows` is real or rows->count == 0.
   Errors: rt_render_lens_samples_async's, the alignment of out only for device memory. */
int rt_render_lens_samples(rt_ctx *ctx, const rt_camera *cam, int width, int height, int depth,
                           const rt_rows *rows /* NULL = full frame */, const double *offsets_xy,
                           const double *lens_xy, double focus, int samples, const double *weights /* nullable */,
                           int fb_format, void *out, int out_on_device, rt_radiance_stats *stats /* nullable */);

/* ---- samples under area lights (soft shadows) -------------------------------
   Replaces, per sample, one rt_upload_scene of the scene with its lights moved (a BVH and light-grid build
   each), one rt_trace_radiance of that sample's rays with fp64 colours through memory, and the caller's own
   reduction: a LIGHT TABLE, context state set once, which gives every sample of the multi-sample entries its
   own light positions.
   light_xyz: HOST memory, samples * num_lights * 3 doubles, num_lights the uploaded scene's; the offset of
   light l for sample s is light_xyz[(s*num_lights + l)*3 .. +2], in scene units, ADDED to the uploaded
   position.  NULL clears the table (samples is then ignored).  With a table, `samples` is its sample count.
   Which launches read it: while a table is set, every RESOLVING radiance launch --
   rt_trace_radiance_resolve[_async], rt_render_samples (through its resolve launches),
   rt_render_samples_async, rt_render_lens_samples[_async], rt_group_render_samples and
   rt_group_render_lens_samples.  For sample s (ray p*samples + s of pixel p) light l has the position
     (fl(Lx + ox), fl(Ly + oy), fl(Lz + oz))       one fp64 add per component, no contraction
   and its uploaded colour, for the WHOLE of that sample's chain: every reflection level, the shadow ray
   (to_light, dist, ldir) and the Phong terms alike.  The records written are, bit for bit, what the same
   call writes on a context whose scene was uploaded with those positions, sample by sample, resolved as the
   call resolves.
   What never reads it: rt_trace_radiance[_async] and the ray and path queries (no sample index), and every
   render (rt_render*, the tile renders, rt_set_antialias, rt_group_render, rt_group_render_frames).  Without a
   table every call writes exactly what it wrote before this entry existed.
   Sample-count mismatch: a resolving call whose `samples` differs from the table's is RT_ERR_INVALID_ARG,
   tested right behind the call's own samples range check, before any HIP call (also for n == 0 or no rows);
   on a group rt_group_last_error names the two counts.
   Any double is allowed: a non-finite offset gives that light a non-finite position and so a NaN direction
   for that sample, handled as a light at the hit point is (rt_trace_paths above: not shadowed; its Phong
   terms are what Scene::shade's arithmetic makes of a NaN, whose std::max(0.0, x) gives 0.0); it is never
   an error.  A light moved outside the uploaded scene's bound costs speed at most: the sweeps' and walks'
   margins are relative to the shadow ray's origin, the light and their distance, never to the bound.
   rays_unaccelerated follows the uploaded scene's own query region (lights included), as before: it is the
   one figure that may differ from a context whose scene was uploaded with the moved lights, whose region
   follows them.
   Synchronous: waits for the context's stream (work in flight may read the table being replaced, as
   rt_upload_scene waits for the scene's), uploads samples * num_lights records of 48 bytes, and returns;
   light_xyz is free on return.  The _async entries gain no launch, buffer or wait: they pass one pointer.
   Lifetime: rt_upload_scene clears the table (the light count may change), rt_destroy frees it.  A scene
   without lights accepts the call and stores an empty table: the launches write what they write without
   one, and the sample-count check still holds.
   Stats: unchanged rules -- rays_shadow = hits * lights per sample, the same counters and events, the
   same 32-bit per-lane counter check of the fused launches.
   Errors: NULL ctx, or a non-NULL light_xyz with samples outside 1..RT_MAX_SAMPLES, RT_ERR_INVALID_ARG
   before any HIP call; no uploaded scene RT_ERR_NO_SCENE; an error leaves the previous table in force. */
int rt_set_light_samples(rt_ctx *ctx, const double *light_xyz /* host, nullable */, int samples);

/* ---- samples with glossy reflections ----------------------------------------
   Replaces, per sample and reflection level, one rt_trace_paths with surfaces, one rt_trace_radiance with
   fp64 colours through memory and a host pass that bends the reflection rays: a GLOSS TABLE, context state
   set once, which gives every sample of the multi-sample entries its own perturbation of each reflection ray,
   scaled by the roughness of the sphere it leaves.
   roughness: HOST memory, num_spheres doubles, num_spheres the uploaded scene's (rt_scene_parse_roughness
   gives a scene file's column).  gloss_xyz: HOST memory, samples * bounces * 3 doubles; the point of sample s
   for bounce b is gloss_xyz[(s*bounces + b)*3 .. +2].  NULL clears the table (the other arguments are then
   ignored).  With a table, `samples` is its sample count.
   Which launches read it: while a table is set, every RESOLVING radiance launch --
   rt_trace_radiance_resolve[_async], rt_render_samples (through its resolve launches),
   rt_render_samples_async, rt_render_lens_samples[_async], rt_group_render_samples and
   rt_group_render_lens_samples.  For sample s (ray p*samples + s of pixel p), at a level k (the camera ray's
   hit is level 0) whose hit on sphere i spawns a reflection ray -- the decision itself is unchanged --, with
   d the incoming direction and nrm the normal, all in fp64 without contraction:
     rd  = d - (nrm*2.0)*dot(d, nrm)                   the mirror direction, unnormalised, as before
     g   = gloss_xyz[(s*bounces + k)*3 .. +2]          bounce index == level index
     rp  = rd + g*roughness[i]                         the product rounded, then the sum
     use = k < bounces && roughness[i] != 0.0 && dot(rp, nrm) * dot(rd, nrm) > 0.0
     d'  = normalized(use ? rp : rd)                   from hp + nrm*EPSILON as before
   Roughness 0 is always a mirror, and so is every bounce k >= bounces; the table is not read for either.  A
   perturbed direction on the wrong side of the surface or in its tangent plane, and every NaN (in g, in the
   roughness, or made of an infinity: 0 * inf, inf - inf), fail the comparison and fall back to the mirror
   direction.  Any double is allowed and nothing is an error: an infinite g or roughness that passes the
   comparison as written gives a direction that is not finite, which hits nothing, as a caller's own ray of
   that kind does.
   The closest hit, the shadow rays, the Phong terms, the stack, the composite, the resolve rule, the
   quantiser and the formats are untouched, and so are the acceleration rule per segment and the counters:
   segments, hits and shadow_rays count what is traced.  A light table (rt_set_light_samples) composes: one
   sample sees moved lights and bent reflections.
   What never reads it: rt_trace_radiance[_async] and the ray and path queries (no sample index), and every
   render (rt_render*, the tile renders, rt_set_antialias, rt_group_render, rt_group_render_frames).  Without a
   table every call writes exactly what it wrote before this entry existed.
   Sample-count mismatch: the light table's rule.  A resolving call whose `samples` differs from the gloss
   table's is RT_ERR_INVALID_ARG, tested next to the light table's check, before any HIP call (also for
   n == 0 or no rows); on a group rt_group_last_error names the two counts.  With both tables set each must
   match.
   Synchronous: waits for the context's stream (work in flight may read the table being replaced), uploads
   samples * bounces points of 24 bytes and num_spheres doubles, and returns; both host arrays are free on
   return.  The _async entries gain no launch, buffer or wait: they pass two pointers and an int.
   Lifetime: rt_upload_scene clears the table (the sphere count may change), rt_destroy frees it.  A scene
   without spheres accepts the call and stores an empty roughness array: the launches write what they write
   without a table, and the sample-count check still holds.
   Stats: unchanged rules, the same counters and events, the same 32-bit per-lane counter check of the
   fused launches (no trip, sample, depth or light count changes).
   Errors: NULL ctx, or a non-NULL gloss_xyz with a NULL roughness, samples outside 1..RT_MAX_SAMPLES or
   bounces outside 1..RT_MAX_GLOSS_BOUNCES, RT_ERR_INVALID_ARG before any HIP call; no uploaded scene
   RT_ERR_NO_SCENE; an error leaves the previous table in force. */
#define RT_MAX_GLOSS_BOUNCES (RT_MAX_DEPTH - 1)
int rt_set_gloss_samples(rt_ctx *ctx, const double *roughness /* host, num_spheres doubles */,
                         const double *gloss_xyz /* host, samples*bounces*3 doubles; NULL clears */, int samples,
                         int bounces);

/* ---- device group: one image row-sharded over several contexts ------------
 * Replaces render_multi in csrc/ray_hip.cpp -- G contexts, their
 * streams and shard buffers, ncclGather to device 0, rt_unpermute_rows -- with
 * one call that needs no RCCL: shards travel with hipMemcpyPeerAsync and are
 * placed into the image as they arrive.  Every rt_group_* call returns an
 * rt_status; argument errors return before any HIP call. */
typedef struct rt_group rt_group;
/* n >= 1 members; devices[i] may repeat (several shards on one device). band >= 1 is the cyclic band height
   (the CLI uses 8). Member i renders rt_rows_for_shard(H, band, i, n). The image is assembled on devices[0].
   Replaces render_multi's set-up (ray_hip.cpp): rt_create per device, streams, ncclCommInitAll.  On failure
   every member already created is destroyed and *out stays NULL. */
int  rt_group_create(const int *devices, int n, int band, rt_group **out);
/* Replaces render_multi's tear-down.  NULL is allowed. */
void rt_group_destroy(rt_group *grp);
int  rt_group_size(const rt_group *grp);               /* members (0 for NULL) */
rt_ctx *rt_group_member(rt_group *grp, int index);     /* borrowed; for rt_get_info / rt_render_stats / rt_kernel_times;
                                                          NULL outside [0, size).  Its stream is the group's. */
const char *rt_group_last_error(const rt_group *grp);
/* rt_upload_scene / rt_set_antialias on every member (render_multi's per-device loop). */
int  rt_group_upload_scene(rt_group *grp, const rt_scene *scene);
int  rt_group_set_antialias(rt_group *grp, int samples);
/* Synchronous. rgb_out: H*W*3 bytes in PPM row order, host memory or (out_on_device=1) memory of devices[0].
   stats (nullable): ray counts summed over members, kernel_ms = max over members.
   Replaces render_multi's frame: rt_render_async per shard, ncclGather, rt_unpermute_rows.  The image is
   assembled on a blocking stream of devices[0] (ordered with the legacy NULL stream, as a context's own). */
int  rt_group_render(rt_group *grp, const rt_camera *cam, int width, int height, int depth,
                     uint8_t *rgb_out, int out_on_device, rt_stats *stats);
/* `nframes` (>= 1, not limited to RT_MAX_FRAMES) frames of the uploaded scene, frame f seen through
   cams[f], each row-sharded over the members exactly as rt_group_render shards one frame, written to
   rgb_out + f * frame_stride (H*W*3 bytes each, PPM row order; host memory, or memory of devices[0]
   with out_on_device = 1): frame f is byte for byte what rt_group_render(grp, &cams[f], ...) writes, and
   no byte between the frames (frame_stride > H*W*3) or outside them is written.  Members render in
   launches of at most `batch` frames (1..RT_MAX_FRAMES; 0 = RT_MAX_FRAMES), split as
   rt_frames.batch_sizes splits them (near-equal launches, larger first); a batch travels to devices[0]
   and is assembled there while the members render the next one, and the host does not wait in between.
   Synchronous: returns when every frame is in rgb_out.  RT_ERR_INVALID_ARG also for nframes > 1 with
   frame_stride < H*W*3 (one frame ignores the stride, as rt_render_frames_async does).
   stats (nullable): ray counts and negative_clamped summed over all frames and members;
   kernel_ms = max over members of the sum of that member's launches.
   Afterwards rt_render_stats on a borrowed member reports that member's LAST launch of the call (its
   shard of the last batch), and rt_kernel_times every launch of the call, one per batch (the call itself
   does not consume that history).
   Replaces the frame loop of rt_frames.run_frames and its RCCL gather. */
int  rt_group_render_frames(rt_group *grp, const rt_camera *cams, int nframes, int width, int height,
                            int depth, int batch, uint8_t *rgb_out, int out_on_device,
                            size_t frame_stride, rt_stats *stats);
/* rt_render_samples of the full frame, row-sharded over the members as rt_group_render shards a frame.
   Synchronous.  out: H*W records in PPM row order, record y*width + x, in host memory or (out_on_device = 1)
   memory of devices[0], 16-byte aligned: byte for byte what rt_render_samples writes on one context, in
   the three formats.  rt_group_render's flow: member i enqueues rt_render_samples_async of
   rt_rows_for_shard(H, band, i, n) into its shard buffer, one hipMemcpyPeerAsync to devices[0], and the
   assembly stream places the shard's real rows (width * 3, 12 or 24 bytes each) as it arrives; the buffers
   and events are those of the other two render calls, any of which may follow any other.
   stats (nullable): counts summed over the members that had a real row, kernel_ms their maximum (a member
   whose shard is all padding launches nothing).  rt_group_set_antialias does not apply.
   Errors: a NULL grp, cam, offsets_xy or out and width / height <= 0 are RT_ERR_INVALID_ARG before any
   HIP call; so are an unknown fb_format, samples outside 1..RT_MAX_SAMPLES and a misaligned device out,
   with rt_group_last_error set; no uploaded scene is RT_ERR_NO_SCENE; the rest are
   rt_render_samples_async's, with the member named in rt_group_last_error.  The group stays usable. */
int  rt_group_render_samples(rt_group *grp, const rt_camera *cam, int width, int height, int depth,
                             const double *offsets_xy, int samples, const double *weights /* nullable */,
                             int fb_format, void *out, int out_on_device, rt_radiance_stats *stats /* nullable */);
/* Replaces a caller's own sharding of rt_render_lens_samples_async over devices: rt_group_render_samples
   with the lens (the section "samples through a thin lens" above).  Per member the fused lens call on its
   shard; the same buffers, events, placement kernel and stats rule, and byte for byte what
   rt_render_lens_samples writes on one context.  It may follow or precede the other three group render
   calls in any order.  Errors: rt_group_render_samples'; a NULL lens_xy is RT_ERR_INVALID_ARG before any
   HIP call as well. */
int  rt_group_render_lens_samples(rt_group *grp, const rt_camera *cam, int width, int height, int depth,
                                  const double *offsets_xy, const double *lens_xy, double focus, int samples,
                                  const double *weights /* nullable */, int fb_format, void *out,
                                  int out_on_device, rt_radiance_stats *stats /* nullable */);

/* rt_set_light_samples on every member ("samples under area lights" above): the two group sample renders
   then shade sample s under the moved lights, byte for byte what the single-context calls write.
   rt_group_upload_scene clears the table on every member.  Errors: rt_set_light_samples', with the cause
   in rt_group_last_error; RT_ERR_NO_SCENE without rt_group_upload_scene. */
int  rt_group_set_light_samples(rt_group *grp, const double *light_xyz /* host, nullable */, int samples);

/* rt_set_gloss_samples on every member ("samples with glossy reflections" above): the two group sample
   renders then bend sample s's reflection rays, byte for byte what the single-context calls write.
   rt_group_upload_scene clears the table on every member.  Errors: rt_set_gloss_samples', with the cause in
   rt_group_last_error; RT_ERR_NO_SCENE without rt_group_upload_scene. */
int  rt_group_set_gloss_samples(rt_group *grp, const double *roughness, const double *gloss_xyz /* nullable */,
                                int samples, int bounces);

#ifdef __cplusplus
}
#endif
#endif /* RT_HIP_H */
