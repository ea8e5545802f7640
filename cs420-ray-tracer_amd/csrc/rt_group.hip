// rt_group.hip -- the device group of the C-ABI (rt_group_*, include/rt_hip.h):
// one image rendered as n cyclic row shards, one shard per member, assembled on
// the first member's device.  What ray_hip's render_multi does with RCCL, as
// one library call and with plain HIP peer copies; a device may appear several
// times in the list, so a one-GPU machine runs the n > 1 path as it stands.
//
// One render (rt_group_render), the same code wherever a member lives:
//   member i, on its own non-blocking stream:
//     rt_render_async(shard i) -> hipMemcpyPeerAsync(stage + i * shard_bytes) -> event i
//   the assembly stream on devices[0]:
//     for every i: wait for event i, place_shard_kernel(shard i)   (early shards
//     are placed while later ones still render)
//     -> one device-to-host copy of the image, unless the caller's buffer is
//        device memory (the shards are then placed straight into it)
//
// A frame sequence (rt_group_render_frames): the frames go in batches of at
// most `batch` (rt_frames.batch_sizes), batch b through slot k = b & 1 of every
// buffer -- shard_i[k] on member i's device, stage[k] and (host output only)
// image[k] on devices[0], each [cap][rows][W][3] for the largest batch `cap`.
// The host only enqueues; it waits once, after the last batch:
//   member i, on its stream, for batch b of n_b frames:
//     rt_render_frames_async(n_b frames -> shard_i[k]) -> rt_add_counts
//     -> wait for consumed[k] of batch b-2 -> ONE hipMemcpyPeerAsync of the n_b
//        shards into stage[k] at member i's place -> event done_i[k]
//   the assembly stream:
//     for every i: wait for done_i[k], ONE place_frames_kernel(member i, batch b)
//     -> host output: the batch's frames device-to-host at frame_stride
//     -> event consumed[k]
// so batch b travels and is placed while the members render batch b+1.
// Hazards, and the edge that orders each:
//   (a) stage[k] is overwritten by batch b+2's copies while batch b is still
//       being placed out of it: every member's copy waits for consumed[k],
//       recorded on the assembly stream after batch b's last placement (and
//       host copy).  The wait sits before the copy, not before the render, so
//       it never holds back rendering.
//   (b) shard_i[k] is rendered into for batch b+2 before batch b's copy has
//       left it: both are on member i's stream, in that order.
//   (c) image[k] (host output) is placed into for batch b+2 before batch b's
//       device-to-host copy has read it: both are on the assembly stream.
//   (d) hipStreamWaitEvent on an event that has not been recorded yet is a
//       no-op, and the members and the assembly stream wait on each other:
//       every wait below names an event recorded EARLIER IN HOST ORDER --
//       done_i[k] in the member loop of the same batch, consumed[k] at the end
//       of batch b-2's iteration -- so no wait can be skipped, and with more
//       streams than hardware queues no barrier sits in front of the packet
//       it waits for.
//   (e) rt_group_render, rt_group_render_samples and rt_group_render_lens_samples
//       (rt_group_render's flow with rt_render_samples_async or
//       rt_render_lens_samples_async per shard, records of 3, 12 or 24 bytes and
//       place_rows_kernel) and rt_group_render_frames share the buffers and the
//       events (one frame uses slot 0): all are synchronous and return
//       with every stream of the group idle -- each member's last work is its
//       done event, which the assembly stream waits for before the host waits
//       for the assembly stream; a failed call drains every stream -- so
//       either may follow the other, and the buffers may be re-allocated.
// Ray counts: rt_add_counts (rt_internal.h) adds each launch's counters into a
// per-member accumulator on the member's stream, read once at the end; the
// context itself keeps one launch's counters and rt_render_stats waits for the
// whole stream, which would stall the pipeline once per batch.
// The only branch a one-GPU machine cannot execute is enable_peer below.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "rt_hip.h"
#include "rt_internal.h"

namespace {

constexpr int kPlaceBlock = 256;

// One row of nb bytes by the workgroup: 16-byte (else 4-byte) vector copies
// when source, destination and length all allow it, bytes otherwise; the
// condition is uniform per row.
__device__ __forceinline__ void copy_row(const uint8_t *__restrict__ s, uint8_t *__restrict__ d, int nb) {
  const uintptr_t bits = reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d) | (uintptr_t)nb;
  if ((bits & 15) == 0) {
    const uint4 *s4 = reinterpret_cast<const uint4 *>(s);
    uint4 *d4 = reinterpret_cast<uint4 *>(d);
    for (int i = threadIdx.x; i < nb / 16; i += kPlaceBlock) d4[i] = s4[i];
  } else if ((bits & 3) == 0) {
    const unsigned *s1 = reinterpret_cast<const unsigned *>(s);
    unsigned *d1 = reinterpret_cast<unsigned *>(d);
    for (int i = threadIdx.x; i < nb / 4; i += kPlaceBlock) d1[i] = s1[i];
  } else {
    for (int i = threadIdx.x; i < nb; i += kPlaceBlock) d[i] = s[i];
  }
}

// Shard r of G (rows k = 0 .. R-1, rendered with rt_rows{band, r, G, R}) into
// the PPM-ordered image: one workgroup per shard row, the inverse of rt_rows'
// row mapping (what unpermute_kernel computes from the image row).  Padding
// rows (y >= H) are skipped: nothing outside the image is written.
__global__ __launch_bounds__(kPlaceBlock) void place_shard_kernel(const uint8_t *__restrict__ src,
                                                                  uint8_t *__restrict__ dst, int W, int H, int band,
                                                                  int G, int r, int R) {
  const int k = blockIdx.x;
  if (k >= R) return;
  const long long y = (long long)(k / band) * band * G + (long long)r * band + (k % band);
  if (y >= H) return;
  const uint8_t *s = src + (size_t)k * (size_t)W * 3;
  uint8_t *d = dst + (size_t)y * (size_t)W * 3;
  copy_row(s, d, W * 3);
}

// The same for a batch of frames of one member (rt_group_render_frames): one
// workgroup per shard row per frame, grid (R, frames).  src is the member's
// [frames][R][W][3] part of the staging buffer, frame f of the destination
// starts at dst + f * dst_stride.  The copy width is chosen per row and per
// frame: an odd dst_stride moves every other frame off the wider paths.  All
// offsets are 64-bit (frames * dst_stride may pass 2^31).
__global__ __launch_bounds__(kPlaceBlock) void place_frames_kernel(const uint8_t *__restrict__ src,
                                                                   uint8_t *__restrict__ dst, size_t dst_stride,
                                                                   int W, int H, int band, int G, int r, int R) {
  const int k = blockIdx.x, f = blockIdx.y;
  if (k >= R) return;
  const long long y = (long long)(k / band) * band * G + (long long)r * band + (k % band);
  if (y >= H) return;
  const uint8_t *s = src + ((size_t)f * (size_t)R + (size_t)k) * (size_t)W * 3;
  uint8_t *d = dst + (size_t)f * dst_stride + (size_t)y * (size_t)W * 3;
  copy_row(s, d, W * 3);
}

// place_shard_kernel for rows of `row_bytes` bytes (rt_group_render_samples: W records of 3, 12 or 24
// bytes, which may pass 2^31 together): the same row mapping and the same choice of copy width per row.
__global__ __launch_bounds__(kPlaceBlock) void place_rows_kernel(const uint8_t *__restrict__ src,
                                                                 uint8_t *__restrict__ dst, size_t row_bytes, int H,
                                                                 int band, int G, int r, int R) {
  const int k = blockIdx.x;
  if (k >= R) return;
  const long long y = (long long)(k / band) * band * G + (long long)r * band + (k % band);
  if (y >= H) return;
  const uint8_t *__restrict__ s = src + (size_t)k * row_bytes;
  uint8_t *__restrict__ d = dst + (size_t)y * row_bytes;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d) | (uintptr_t)row_bytes;
  if ((bits & 15) == 0) {
    const uint4 *s4 = reinterpret_cast<const uint4 *>(s);
    uint4 *d4 = reinterpret_cast<uint4 *>(d);
    for (size_t i = threadIdx.x; i < row_bytes / 16; i += kPlaceBlock) d4[i] = s4[i];
  } else if ((bits & 3) == 0) {
    const unsigned *s1 = reinterpret_cast<const unsigned *>(s);
    unsigned *d1 = reinterpret_cast<unsigned *>(d);
    for (size_t i = threadIdx.x; i < row_bytes / 4; i += kPlaceBlock) d1[i] = s1[i];
  } else {
    for (size_t i = threadIdx.x; i < row_bytes; i += kPlaceBlock) d[i] = s[i];
  }
}

// Grow-only device memory on one device.
struct GroupBuf {
  uint8_t *p = nullptr;
  size_t cap = 0;
};

// Slot 0 of every pair serves rt_group_render; a frame sequence alternates.
struct Member {
  int device = 0;
  rt_ctx *ctx = nullptr;
  hipStream_t stream = nullptr;          // non-blocking, on `device`; the context's stream (rt_set_stream)
  hipEvent_t done[2] = {};               // slot k's shards have arrived in stage[k]
  GroupBuf shard[2];                     // on `device`
  unsigned long long *counts = nullptr;  // on `device`: the rt_add_counts accumulator of a frame sequence
  // of the frame sequence in flight: `ms` sums its launches below index `harvested` (harvest_ms)
  long long harvested = 0;
  double ms = 0.0;
};

}  // namespace

struct rt_group {
  int band = 8;
  std::vector<Member> m;
  // on m[0].device
  hipStream_t assembly = nullptr;
  GroupBuf stage[2], image[2];      // image: the assembled frame(s) of a render to host memory
  hipEvent_t consumed[2] = {};      // everything placed (and copied to the host) out of stage[k] / image[k]
  bool has_scene = false;
  std::string err;
};

namespace {

int fail(rt_group *g, hipError_t e, const char *what) {
  g->err = std::string(what) + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP;
}

#define GRP_TRY(grp, call)                              \
  do {                                                  \
    hipError_t e_ = (call);                             \
    if (e_ != hipSuccess) return fail(grp, e_, #call);  \
  } while (0)

// A member's own failure: its status, its message.
int member_fail(rt_group *g, int i, int rc, const char *what) {
  g->err = "member " + std::to_string(i) + " " + what + ": " + rt_last_error(g->m[i].ctx);
  return rc;
}

// The caller has made `device` current; nothing of the group is in flight.
int grow(rt_group *g, GroupBuf &b, size_t bytes) {
  if (bytes <= b.cap) return RT_OK;
  if (b.p) GRP_TRY(g, hipFree(b.p));
  b.p = nullptr, b.cap = 0;
  GRP_TRY(g, hipMalloc(reinterpret_cast<void **>(&b.p), bytes));
  b.cap = bytes;
  return RT_OK;
}

// Direct copies between `a` and `b` where the hardware has them (else
// hipMemcpyPeerAsync stages through the host).  Not reachable with one device.
int enable_peer(rt_group *g, int a, int b) {
  const int pair[2][2] = {{a, b}, {b, a}};
  for (const auto &p : pair) {
    int can = 0;
    GRP_TRY(g, hipDeviceCanAccessPeer(&can, p[0], p[1]));
    if (!can) continue;
    GRP_TRY(g, hipSetDevice(p[0]));
    const hipError_t e = hipDeviceEnablePeerAccess(p[1], 0);
    if (e == hipErrorPeerAccessAlreadyEnabled)
      (void)hipGetLastError();
    else if (e != hipSuccess)
      return fail(g, e, "hipDeviceEnablePeerAccess");
  }
  return RT_OK;
}

int add_member(rt_group *g, int device) {
  const int i = (int)g->m.size();
  g->m.emplace_back();
  Member &mb = g->m.back();
  mb.device = device;
  const int rc = rt_create(device, &mb.ctx);
  if (rc != RT_OK) {
    g->err = "member " + std::to_string(i) + " rt_create(" + std::to_string(device) + "): " + rt_error_string(rc);
    return rc;
  }
  GRP_TRY(g, hipSetDevice(device));
  GRP_TRY(g, hipStreamCreateWithFlags(&mb.stream, hipStreamNonBlocking));
  for (hipEvent_t &e : mb.done) GRP_TRY(g, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  GRP_TRY(g, hipMalloc(reinterpret_cast<void **>(&mb.counts), kRtCountSlots * sizeof(unsigned long long)));
  const int src = rt_set_stream(mb.ctx, mb.stream);
  if (src != RT_OK) return member_fail(g, i, src, "rt_set_stream");
  const int first = g->m[0].device;
  bool seen = device == first;
  for (int j = 0; j < i && !seen; j++) seen = g->m[j].device == device;
  return seen ? RT_OK : enable_peer(g, device, first);
}

// Waits for everything the group has enqueued (after a failed render: the
// call stays synchronous, and the buffers are idle for the next one).
void drain(rt_group *g) {
  for (Member &mb : g->m)
    if (mb.stream && hipSetDevice(mb.device) == hipSuccess) (void)hipStreamSynchronize(mb.stream);
  if (g->assembly && !g->m.empty() && hipSetDevice(g->m[0].device) == hipSuccess)
    (void)hipStreamSynchronize(g->assembly);
  (void)hipGetLastError();
}

int render(rt_group *g, const rt_camera *cam, int W, int H, int depth, uint8_t *out, int out_on_device,
           rt_stats *stats) {
  const int n = (int)g->m.size(), dev0 = g->m[0].device;
  rt_rows rows;
  int rc = rt_rows_for_shard(H, g->band, 0, n, &rows);
  if (rc != RT_OK) return rc;
  const int R = rows.count;
  const size_t shard_bytes = (size_t)R * (size_t)W * 3, image_bytes = (size_t)H * (size_t)W * 3;
  for (Member &mb : g->m) {
    GRP_TRY(g, hipSetDevice(mb.device));
    if ((rc = grow(g, mb.shard[0], shard_bytes)) != RT_OK) return rc;
  }
  GRP_TRY(g, hipSetDevice(dev0));
  if ((rc = grow(g, g->stage[0], shard_bytes * n)) != RT_OK) return rc;
  if (!out_on_device && (rc = grow(g, g->image[0], image_bytes)) != RT_OK) return rc;
  uint8_t *const image = out_on_device ? out : g->image[0].p;

  for (int i = 0; i < n; i++) {
    Member &mb = g->m[i];
    if ((rc = rt_rows_for_shard(H, g->band, i, n, &rows)) != RT_OK) return rc;
    if ((rc = rt_render_async(mb.ctx, cam, W, H, depth, &rows, mb.shard[0].p)) != RT_OK)
      return member_fail(g, i, rc, "rt_render_async");
    GRP_TRY(g, hipSetDevice(mb.device));
    GRP_TRY(g, hipMemcpyPeerAsync(g->stage[0].p + (size_t)i * shard_bytes, dev0, mb.shard[0].p, mb.device,
                                  shard_bytes, mb.stream));
    GRP_TRY(g, hipEventRecord(mb.done[0], mb.stream));
  }
  GRP_TRY(g, hipSetDevice(dev0));
  for (int i = 0; i < n; i++) {
    GRP_TRY(g, hipStreamWaitEvent(g->assembly, g->m[i].done[0], 0));
    hipLaunchKernelGGL(place_shard_kernel, dim3((unsigned)R), dim3(kPlaceBlock), 0, g->assembly,
                       g->stage[0].p + (size_t)i * shard_bytes, image, W, H, g->band, n, i, R);
    GRP_TRY(g, hipGetLastError());
  }
  if (!out_on_device) GRP_TRY(g, hipMemcpyAsync(out, image, image_bytes, hipMemcpyDeviceToHost, g->assembly));
  GRP_TRY(g, hipStreamSynchronize(g->assembly));

  rt_stats sum{};
  for (int i = 0; i < n; i++) {
    rt_stats st{};
    if ((rc = rt_render_stats(g->m[i].ctx, &st)) != RT_OK) return member_fail(g, i, rc, "rt_render_stats");
    sum.rays_primary += st.rays_primary;
    sum.rays_shadow += st.rays_shadow;
    sum.rays_reflect += st.rays_reflect;
    sum.negative_clamped += st.negative_clamped;
    sum.tests_exact += st.tests_exact;
    sum.tests_cull += st.tests_cull;
    sum.kernel_ms = std::max(sum.kernel_ms, st.kernel_ms);
  }
  if (stats) *stats = sum;
  return RT_OK;
}

// render()'s flow for a multi-sample frame: rt_render_samples_async per shard (with `lens`, the lens
// points of rt_group_render_lens_samples, rt_render_lens_samples_async), records of `rec` bytes.
// The same buffers and events (slot 0); the ordering edges are render()'s.
int render_samples(rt_group *g, const rt_camera *cam, int W, int H, int depth, const double *offsets,
                   const double *lens, double focus, int samples, const double *weights, int fmt, size_t rec,
                   uint8_t *out, int out_on_device, rt_radiance_stats *stats) {
  const int n = (int)g->m.size(), dev0 = g->m[0].device;
  rt_rows rows;
  int rc = rt_rows_for_shard(H, g->band, 0, n, &rows);
  if (rc != RT_OK) return rc;
  const int R = rows.count;
  const size_t row_bytes = (size_t)W * rec;
  const size_t shard_bytes = (size_t)R * row_bytes, image_bytes = (size_t)H * row_bytes;
  for (Member &mb : g->m) {
    GRP_TRY(g, hipSetDevice(mb.device));
    if ((rc = grow(g, mb.shard[0], shard_bytes)) != RT_OK) return rc;
  }
  GRP_TRY(g, hipSetDevice(dev0));
  if ((rc = grow(g, g->stage[0], shard_bytes * n)) != RT_OK) return rc;
  if (!out_on_device && (rc = grow(g, g->image[0], image_bytes)) != RT_OK) return rc;
  uint8_t *const image = out_on_device ? out : g->image[0].p;

  for (int i = 0; i < n; i++) {
    Member &mb = g->m[i];
    if ((rc = rt_rows_for_shard(H, g->band, i, n, &rows)) != RT_OK) return rc;
    rc = lens ? rt_render_lens_samples_async(mb.ctx, cam, W, H, depth, &rows, offsets, lens, focus, samples, weights,
                                             fmt, mb.shard[0].p)
              : rt_render_samples_async(mb.ctx, cam, W, H, depth, &rows, offsets, samples, weights, fmt,
                                        mb.shard[0].p);
    if (rc != RT_OK) return member_fail(g, i, rc, lens ? "rt_render_lens_samples_async" : "rt_render_samples_async");
    GRP_TRY(g, hipSetDevice(mb.device));
    GRP_TRY(g, hipMemcpyPeerAsync(g->stage[0].p + (size_t)i * shard_bytes, dev0, mb.shard[0].p, mb.device,
                                  shard_bytes, mb.stream));
    GRP_TRY(g, hipEventRecord(mb.done[0], mb.stream));
  }
  GRP_TRY(g, hipSetDevice(dev0));
  for (int i = 0; i < n; i++) {
    GRP_TRY(g, hipStreamWaitEvent(g->assembly, g->m[i].done[0], 0));
    hipLaunchKernelGGL(place_rows_kernel, dim3((unsigned)R), dim3(kPlaceBlock), 0, g->assembly,
                       g->stage[0].p + (size_t)i * shard_bytes, image, row_bytes, H, g->band, n, i, R);
    GRP_TRY(g, hipGetLastError());
  }
  if (!out_on_device) GRP_TRY(g, hipMemcpyAsync(out, image, image_bytes, hipMemcpyDeviceToHost, g->assembly));
  GRP_TRY(g, hipStreamSynchronize(g->assembly));

  rt_radiance_stats sum{};
  for (int i = 0; i < n; i++) {
    // Shard i's first row is image row i * band: without it the member launched nothing, and its
    // report is an earlier call's.
    if ((long long)i * g->band >= H) continue;
    rt_radiance_stats st{};
    if ((rc = rt_radiance_stats_get(g->m[i].ctx, &st)) != RT_OK) return member_fail(g, i, rc, "rt_radiance_stats_get");
    sum.rays += st.rays;
    sum.segments += st.segments;
    sum.hits += st.hits;
    sum.shadow_rays += st.shadow_rays;
    sum.tests_exact += st.tests_exact;
    sum.tests_cull += st.tests_cull;
    sum.unaccelerated += st.unaccelerated;
    sum.negative_clamped += st.negative_clamped;
    sum.kernel_ms = std::max(sum.kernel_ms, st.kernel_ms);
  }
  if (stats) *stats = sum;
  return RT_OK;
}

// Launches the context has enqueued since rt_create: the index of its next one.
long long launch_count(rt_ctx *ctx) {
  rt_info info;
  return rt_get_info(ctx, &info) == RT_OK ? (long long)info.launches : 0;
}

// Adds the kernel times of member i's launches [harvested, upto) to its sum.
// A launch's events live in a ring of 256 (rt_launch_ms): a long sequence
// collects them 128 launches behind the one being enqueued, so the wait inside
// is for work long finished.
int harvest_ms(rt_group *g, int i, long long upto) {
  Member &mb = g->m[i];
  for (; mb.harvested < upto; mb.harvested++) {
    double ms = 0.0;
    const int rc = rt_launch_ms(mb.ctx, mb.harvested, &ms);
    if (rc != RT_OK) return member_fail(g, i, rc, "rt_launch_ms");
    mb.ms += ms;
  }
  return RT_OK;
}

// The pipeline and its ordering edges: the head of this file.  fstride is the
// distance between frames in `out` (H*W*3 for one frame).
int render_frames(rt_group *g, const rt_camera *cams, int F, int W, int H, int depth, int batch, uint8_t *out,
                  int out_on_device, size_t fstride, rt_stats *stats) {
  const int n = (int)g->m.size(), dev0 = g->m[0].device;
  rt_rows rows;
  int rc = rt_rows_for_shard(H, g->band, 0, n, &rows);
  if (rc != RT_OK) return rc;
  const int R = rows.count;
  const size_t shard_bytes = (size_t)R * (size_t)W * 3, image_bytes = (size_t)H * (size_t)W * 3;
  // rt_frames.batch_sizes: near-equal launches, the larger ones first
  const int nbatch = (int)(((long long)F + batch - 1) / batch), q = F / nbatch, rem = F % nbatch;
  const size_t cap = (size_t)q + (rem ? 1 : 0);
  const int slots = nbatch > 1 ? 2 : 1;
  for (Member &mb : g->m) {
    GRP_TRY(g, hipSetDevice(mb.device));
    for (int k = 0; k < slots; k++)
      if ((rc = grow(g, mb.shard[k], cap * shard_bytes)) != RT_OK) return rc;
    GRP_TRY(g, hipMemsetAsync(mb.counts, 0, kRtCountSlots * sizeof(unsigned long long), mb.stream));
    mb.harvested = launch_count(mb.ctx);
    mb.ms = 0.0;
  }
  GRP_TRY(g, hipSetDevice(dev0));
  for (int k = 0; k < slots; k++) {
    if ((rc = grow(g, g->stage[k], cap * shard_bytes * n)) != RT_OK) return rc;
    if (!out_on_device && (rc = grow(g, g->image[k], cap * image_bytes)) != RT_OK) return rc;
  }

  int done = 0;
  for (int b = 0; b < nbatch; b++) {
    const int k = b & 1, nf = q + (b < rem ? 1 : 0);
    for (int i = 0; i < n; i++) {
      Member &mb = g->m[i];
      const long long next = launch_count(mb.ctx);
      if (next - mb.harvested >= 192 && (rc = harvest_ms(g, i, next - 128)) != RT_OK) return rc;
      if ((rc = rt_rows_for_shard(H, g->band, i, n, &rows)) != RT_OK) return rc;
      if ((rc = rt_render_frames_async(mb.ctx, cams + done, nf, W, H, depth, &rows, mb.shard[k].p, shard_bytes)) !=
          RT_OK)
        return member_fail(g, i, rc, "rt_render_frames_async");
      if ((rc = rt_add_counts(mb.ctx, mb.counts)) != RT_OK) return member_fail(g, i, rc, "rt_add_counts");
      GRP_TRY(g, hipSetDevice(mb.device));
      if (b >= 2) GRP_TRY(g, hipStreamWaitEvent(mb.stream, g->consumed[k], 0));  // (a); recorded by batch b-2 (d)
      GRP_TRY(g, hipMemcpyPeerAsync(g->stage[k].p + (size_t)i * cap * shard_bytes, dev0, mb.shard[k].p, mb.device,
                                    (size_t)nf * shard_bytes, mb.stream));
      GRP_TRY(g, hipEventRecord(mb.done[k], mb.stream));
    }
    GRP_TRY(g, hipSetDevice(dev0));
    uint8_t *const dst = out_on_device ? out + (size_t)done * fstride : g->image[k].p;
    const size_t dst_stride = out_on_device ? fstride : image_bytes;
    for (int i = 0; i < n; i++) {
      GRP_TRY(g, hipStreamWaitEvent(g->assembly, g->m[i].done[k], 0));  // recorded in the loop above (d)
      hipLaunchKernelGGL(place_frames_kernel, dim3((unsigned)R, (unsigned)nf), dim3(kPlaceBlock), 0, g->assembly,
                         g->stage[k].p + (size_t)i * cap * shard_bytes, dst, dst_stride, W, H, g->band, n, i, R);
      GRP_TRY(g, hipGetLastError());
    }
    if (!out_on_device) {
      if (fstride == image_bytes) {
        GRP_TRY(g, hipMemcpyAsync(out + (size_t)done * fstride, dst, (size_t)nf * image_bytes, hipMemcpyDeviceToHost,
                                  g->assembly));
      } else {
        for (int f = 0; f < nf; f++)  // nothing between the frames is written
          GRP_TRY(g, hipMemcpyAsync(out + (size_t)(done + f) * fstride, dst + (size_t)f * image_bytes, image_bytes,
                                    hipMemcpyDeviceToHost, g->assembly));
      }
    }
    if (b + 2 < nbatch) GRP_TRY(g, hipEventRecord(g->consumed[k], g->assembly));
    done += nf;
  }
  GRP_TRY(g, hipStreamSynchronize(g->assembly));  // every member's done events, so every member's stream too

  rt_stats sum{};
  for (int i = 0; i < n; i++) {
    Member &mb = g->m[i];
    rt_stats last{};  // the member's last launch; in the bounds-checked build, the sequence's RT_ERR_CHECK
    if ((rc = rt_render_stats(mb.ctx, &last)) != RT_OK) return member_fail(g, i, rc, "rt_render_stats");
    if ((rc = harvest_ms(g, i, launch_count(mb.ctx))) != RT_OK) return rc;
    unsigned long long c[kRtCountSlots];
    GRP_TRY(g, hipSetDevice(mb.device));
    GRP_TRY(g, hipMemcpy(c, mb.counts, sizeof c, hipMemcpyDeviceToHost));
    sum.rays_primary += c[0];
    sum.rays_shadow += c[1];
    sum.rays_reflect += c[2];
    sum.negative_clamped += c[3];
    sum.tests_exact += c[4];
    sum.tests_cull += c[5];
    sum.kernel_ms = std::max(sum.kernel_ms, mb.ms);
  }
  if (stats) *stats = sum;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_group_create(const int *devices, int n, int band, rt_group **out) {
  if (!out) return RT_ERR_INVALID_ARG;
  *out = nullptr;
  if (!devices || n < 1 || band < 1) return RT_ERR_INVALID_ARG;
  rt_group *g = new (std::nothrow) rt_group;
  if (!g) return RT_ERR_OUT_OF_MEMORY;
  g->band = band;
  g->m.reserve((size_t)n);
  int rc = RT_OK;
  for (int i = 0; i < n && rc == RT_OK; i++) rc = add_member(g, devices[i]);
  if (rc == RT_OK) {
    // A blocking stream, as a context's own: ordered with the legacy NULL
    // stream, so a device buffer the caller filled there (out_on_device) is
    // ready before the shards are placed into it.
    hipError_t e = hipSetDevice(g->m[0].device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&g->assembly, hipStreamDefault);
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipEventCreateWithFlags(&g->consumed[k], hipEventDisableTiming);
    if (e != hipSuccess) rc = fail(g, e, "the assembly stream and its events");
  }
  if (rc != RT_OK) {
    rt_group_destroy(g);  // every member created so far
    return rc;
  }
  *out = g;
  return RT_OK;
}

void rt_group_destroy(rt_group *g) {
  if (!g) return;
  drain(g);
  for (Member &mb : g->m) {
    if (!mb.ctx) continue;  // rt_create refused the device: nothing of this member exists, nor may the device
    rt_destroy(mb.ctx);     // before its stream: rt_destroy waits on it
    (void)hipSetDevice(mb.device);
    for (GroupBuf &b : mb.shard)
      if (b.p) (void)hipFree(b.p);
    if (mb.counts) (void)hipFree(mb.counts);
    for (hipEvent_t e : mb.done)
      if (e) (void)hipEventDestroy(e);
    if (mb.stream) (void)hipStreamDestroy(mb.stream);
  }
  if (g->assembly) {  // only a complete group has one, and only such a group has the two buffers
    (void)hipSetDevice(g->m[0].device);
    for (int k = 0; k < 2; k++) {
      if (g->stage[k].p) (void)hipFree(g->stage[k].p);
      if (g->image[k].p) (void)hipFree(g->image[k].p);
      if (g->consumed[k]) (void)hipEventDestroy(g->consumed[k]);
    }
    (void)hipStreamDestroy(g->assembly);
  }
  delete g;
}

int rt_group_size(const rt_group *g) { return g ? (int)g->m.size() : 0; }

rt_ctx *rt_group_member(rt_group *g, int index) {
  return g && index >= 0 && index < (int)g->m.size() ? g->m[index].ctx : nullptr;
}

const char *rt_group_last_error(const rt_group *g) { return g ? g->err.c_str() : "null group"; }

int rt_group_upload_scene(rt_group *g, const rt_scene *scene) {
  if (!g || !scene) return RT_ERR_INVALID_ARG;
  g->has_scene = false;
  for (int i = 0; i < (int)g->m.size(); i++) {
    const int rc = rt_upload_scene(g->m[i].ctx, scene);
    if (rc != RT_OK) return member_fail(g, i, rc, "rt_upload_scene");
  }
  g->has_scene = true;
  return RT_OK;
}

int rt_group_set_light_samples(rt_group *g, const double *light_xyz, int samples) {
  if (!g) return RT_ERR_INVALID_ARG;
  if (light_xyz && (samples < 1 || samples > RT_MAX_SAMPLES)) {
    g->err = "rt_group_set_light_samples: samples outside 1..RT_MAX_SAMPLES";
    return RT_ERR_INVALID_ARG;
  }
  if (!g->has_scene) {
    g->err = "rt_group_set_light_samples: no scene uploaded";
    return RT_ERR_NO_SCENE;
  }
  for (int i = 0; i < (int)g->m.size(); i++) {
    const int rc = rt_set_light_samples(g->m[i].ctx, light_xyz, samples);
    if (rc != RT_OK) return member_fail(g, i, rc, "rt_set_light_samples");
  }
  return RT_OK;
}

int rt_group_set_gloss_samples(rt_group *g, const double *roughness, const double *gloss_xyz, int samples,
                               int bounces) {
  if (!g) return RT_ERR_INVALID_ARG;
  if (gloss_xyz && !roughness) {
    g->err = "rt_group_set_gloss_samples: a table without the spheres' roughness";
    return RT_ERR_INVALID_ARG;
  }
  if (gloss_xyz && (samples < 1 || samples > RT_MAX_SAMPLES)) {
    g->err = "rt_group_set_gloss_samples: samples outside 1..RT_MAX_SAMPLES";
    return RT_ERR_INVALID_ARG;
  }
  if (gloss_xyz && (bounces < 1 || bounces > RT_MAX_GLOSS_BOUNCES)) {
    g->err = "rt_group_set_gloss_samples: bounces outside 1..RT_MAX_GLOSS_BOUNCES";
    return RT_ERR_INVALID_ARG;
  }
  if (!g->has_scene) {
    g->err = "rt_group_set_gloss_samples: no scene uploaded";
    return RT_ERR_NO_SCENE;
  }
  for (int i = 0; i < (int)g->m.size(); i++) {
    const int rc = rt_set_gloss_samples(g->m[i].ctx, roughness, gloss_xyz, samples, bounces);
    if (rc != RT_OK) return member_fail(g, i, rc, "rt_set_gloss_samples");
  }
  return RT_OK;
}

int rt_group_set_antialias(rt_group *g, int samples) {
  if (!g || (samples != 1 && samples != 4)) return RT_ERR_INVALID_ARG;
  for (int i = 0; i < (int)g->m.size(); i++) {
    const int rc = rt_set_antialias(g->m[i].ctx, samples);
    if (rc != RT_OK) return member_fail(g, i, rc, "rt_set_antialias");
  }
  return RT_OK;
}

int rt_group_render(rt_group *g, const rt_camera *cam, int W, int H, int depth, uint8_t *out, int out_on_device,
                    rt_stats *stats) {
  // the order of every render entry point: arguments, the scene, the depth
  if (!g || !cam || !out || W <= 0 || H <= 0) return RT_ERR_INVALID_ARG;
  if (!g->has_scene) return RT_ERR_NO_SCENE;
  if (depth > RT_MAX_DEPTH) return RT_ERR_DEPTH;
  const int rc = render(g, cam, W, H, depth, out, out_on_device, stats);
  if (rc != RT_OK) drain(g);
  return rc;
}

// rt_group_render_samples and, with `lens`, rt_group_render_lens_samples (`name` in the error texts).
static int group_render_samples(rt_group *g, const char *name, const rt_camera *cam, int W, int H, int depth,
                                const double *offsets, const double *lens, double focus, int samples,
                                const double *weights, int fmt, void *out, int out_on_device,
                                rt_radiance_stats *stats) {
  if (!g || !cam || !offsets || !out || W <= 0 || H <= 0) return RT_ERR_INVALID_ARG;
  // what sizes the group's buffers, checked here; the member calls check it again with everything else
  const size_t rec = fmt == RT_FB_RGB8 ? 3 : fmt == RT_FB_F32X3 ? 12 : fmt == RT_FB_F64X3 ? 24 : 0;
  if (rec == 0 || samples < 1 || samples > RT_MAX_SAMPLES ||
      (out_on_device && (reinterpret_cast<uintptr_t>(out) & 15u))) {
    g->err = std::string(name) + (rec == 0 ? ": unknown fb_format"
                                  : samples < 1 || samples > RT_MAX_SAMPLES ? ": samples outside 1..RT_MAX_SAMPLES"
                                                                            : ": device out is not 16-byte aligned");
    return RT_ERR_INVALID_ARG;
  }
  if (!g->has_scene) {
    g->err = std::string(name) + ": no scene uploaded";
    return RT_ERR_NO_SCENE;
  }
  // the members' light tables (rt_group_set_light_samples): the member calls would refuse too, without a text
  for (const Member &mb : g->m) {
    const int table = rt_light_samples(mb.ctx);
    if (table != 0 && table != samples) {
      g->err = std::string(name) + ": samples (" + std::to_string(samples) + ") differs from the light table's (" +
               std::to_string(table) + ", rt_group_set_light_samples)";
      return RT_ERR_INVALID_ARG;
    }
    const int gloss = rt_gloss_samples(mb.ctx);  // likewise (rt_group_set_gloss_samples)
    if (gloss != 0 && gloss != samples) {
      g->err = std::string(name) + ": samples (" + std::to_string(samples) + ") differs from the gloss table's (" +
               std::to_string(gloss) + ", rt_group_set_gloss_samples)";
      return RT_ERR_INVALID_ARG;
    }
  }
  const int rc = render_samples(g, cam, W, H, depth, offsets, lens, focus, samples, weights, fmt, rec,
                                static_cast<uint8_t *>(out), out_on_device, stats);
  if (rc != RT_OK) drain(g);
  return rc;
}

int rt_group_render_samples(rt_group *g, const rt_camera *cam, int W, int H, int depth, const double *offsets,
                            int samples, const double *weights, int fmt, void *out, int out_on_device,
                            rt_radiance_stats *stats) {
  return group_render_samples(g, "rt_group_render_samples", cam, W, H, depth, offsets, nullptr, 0.0, samples, weights,
                              fmt, out, out_on_device, stats);
}

int rt_group_render_lens_samples(rt_group *g, const rt_camera *cam, int W, int H, int depth, const double *offsets,
                                 const double *lens, double focus, int samples, const double *weights, int fmt,
                                 void *out, int out_on_device, rt_radiance_stats *stats) {
  if (!lens) return RT_ERR_INVALID_ARG;
  return group_render_samples(g, "rt_group_render_lens_samples", cam, W, H, depth, offsets, lens, focus, samples,
                              weights, fmt, out, out_on_device, stats);
}

int rt_group_render_frames(rt_group *g, const rt_camera *cams, int nframes, int W, int H, int depth, int batch,
                           uint8_t *out, int out_on_device, size_t frame_stride, rt_stats *stats) {
  if (!g || !cams || !out || W <= 0 || H <= 0 || nframes < 1 || batch < 0 || batch > RT_MAX_FRAMES)
    return RT_ERR_INVALID_ARG;
  const size_t image_bytes = (size_t)H * (size_t)W * 3;
  if (nframes > 1 && frame_stride < image_bytes) return RT_ERR_INVALID_ARG;
  if (!g->has_scene) return RT_ERR_NO_SCENE;
  if (depth > RT_MAX_DEPTH) return RT_ERR_DEPTH;
  const int rc = render_frames(g, cams, nframes, W, H, depth, batch ? batch : RT_MAX_FRAMES, out, out_on_device,
                               nframes > 1 ? frame_stride : image_bytes, stats);
  if (rc != RT_OK) drain(g);
  return rc;
}

}  // extern "C"
