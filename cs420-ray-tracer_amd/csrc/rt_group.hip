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
// The only branch a one-GPU machine cannot execute is enable_peer below.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "rt_hip.h"

namespace {

constexpr int kPlaceBlock = 256;

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
  const int nb = W * 3;
  // 16-byte (else 4-byte) vector copies when both rows allow it, bytes
  // otherwise; the condition is uniform per row
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

// Grow-only device memory on one device.
struct GroupBuf {
  uint8_t *p = nullptr;
  size_t cap = 0;
};

struct Member {
  int device = 0;
  rt_ctx *ctx = nullptr;
  hipStream_t stream = nullptr;  // non-blocking, on `device`; the context's stream (rt_set_stream)
  hipEvent_t done = nullptr;     // the shard has arrived in the staging buffer
  GroupBuf shard;                // on `device`
};

}  // namespace

struct rt_group {
  int band = 8;
  std::vector<Member> m;
  // on m[0].device
  hipStream_t assembly = nullptr;
  GroupBuf stage, image;
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
  GRP_TRY(g, hipEventCreateWithFlags(&mb.done, hipEventDisableTiming));
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
    if ((rc = grow(g, mb.shard, shard_bytes)) != RT_OK) return rc;
  }
  GRP_TRY(g, hipSetDevice(dev0));
  if ((rc = grow(g, g->stage, shard_bytes * n)) != RT_OK) return rc;
  if (!out_on_device && (rc = grow(g, g->image, image_bytes)) != RT_OK) return rc;
  uint8_t *const image = out_on_device ? out : g->image.p;

  for (int i = 0; i < n; i++) {
    Member &mb = g->m[i];
    if ((rc = rt_rows_for_shard(H, g->band, i, n, &rows)) != RT_OK) return rc;
    if ((rc = rt_render_async(mb.ctx, cam, W, H, depth, &rows, mb.shard.p)) != RT_OK)
      return member_fail(g, i, rc, "rt_render_async");
    GRP_TRY(g, hipSetDevice(mb.device));
    GRP_TRY(g, hipMemcpyPeerAsync(g->stage.p + (size_t)i * shard_bytes, dev0, mb.shard.p, mb.device, shard_bytes,
                                  mb.stream));
    GRP_TRY(g, hipEventRecord(mb.done, mb.stream));
  }
  GRP_TRY(g, hipSetDevice(dev0));
  for (int i = 0; i < n; i++) {
    GRP_TRY(g, hipStreamWaitEvent(g->assembly, g->m[i].done, 0));
    hipLaunchKernelGGL(place_shard_kernel, dim3((unsigned)R), dim3(kPlaceBlock), 0, g->assembly,
                       g->stage.p + (size_t)i * shard_bytes, image, W, H, g->band, n, i, R);
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
    if (e != hipSuccess) rc = fail(g, e, "hipStreamCreateWithFlags");
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
    if (mb.shard.p) (void)hipFree(mb.shard.p);
    if (mb.done) (void)hipEventDestroy(mb.done);
    if (mb.stream) (void)hipStreamDestroy(mb.stream);
  }
  if (g->assembly) {  // only a complete group has one, and only such a group has the two buffers
    (void)hipSetDevice(g->m[0].device);
    if (g->stage.p) (void)hipFree(g->stage.p);
    if (g->image.p) (void)hipFree(g->image.p);
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

}  // extern "C"
