"""What depth of field costs in the multi-sample renders: synth200 at 1920x1080 depth 4, RT_FB_RGB8 into
device memory (the workload of profiles/samples_fused/measure.py), grid_pattern(2) (4 samples) and
grid_pattern(8) (64 samples), lens_pattern of aperture 0 and of aperture 1.0 focused at 30 units (the
spheres lie 24 to 47 units from the camera: a blur of up to half a sphere's radius).

 (a) rt_render_samples_async: the pinhole fused launch;
 (b) rt_camera_lens_rays into a ray buffer, then rt_trace_radiance_resolve_async of it: both enqueued
     with no host wait between them, the whole frame in ONE ray buffer (531 MB at 4 samples, 8.5 GB at
     64: the route's best case, a caller with less memory chunks it);
 (c) rt_render_lens_samples_async: the fused lens launch.

One process, one device; every variant is warmed once and checked ((b) and (c) write the same bytes, at
aperture 0 and focus 1.0 also (a)'s); the variants alternate within each of the ROUNDS rounds; medians,
min-max and every run are recorded.  gpu_ms is the time between two events on the context's stream around
everything the variant enqueues (for (b) the generator and the resolving kernel), kernel_ms what
rt_radiance_stats_get reports (the resolving or fused kernel alone), wall_ms a host clock around the calls
and the wait.

    python profiles/lens_samples/measure.py [out.json]
"""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "cs420-ray-tracer_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import rt_hip  # noqa: E402

W, H, D, ROUNDS = 1920, 1080, 4, 7
FOCUS, APERTURE = 30.0, 1.0
F_RGB8 = rt_hip.RT_FB_RGB8


def main():
    scene = rt_hip.Scene.load(os.path.join(REPO, "cs420-ray-tracer_amd", "scenes", "synth200.txt"))
    cam = scene.camera()
    n = W * H
    r = rt_hip.Renderer(0)
    r.upload(scene)
    side = torch.cuda.Stream()
    r.set_stream(side.cuda_stream)
    rgb = torch.zeros((n * 3,), dtype=torch.uint8, device="cuda:0")
    rays = torch.zeros((n * 64 * 8,), dtype=torch.float64, device="cuda:0")  # 64 samples of 64 bytes per pixel
    torch.cuda.synchronize()
    pattern = {4: rt_hip.grid_pattern(2), 64: rt_hip.grid_pattern(8)}
    lens = {(4, 0): rt_hip.lens_pattern(2, 0.0), (64, 0): rt_hip.lens_pattern(8, 0.0),
            (4, 1): rt_hip.lens_pattern(2, APERTURE), (64, 1): rt_hip.lens_pattern(8, APERTURE)}

    def pinhole(S):
        r.render_samples_async(cam, W, H, D, pattern[S], rgb.data_ptr())

    def buffered(S, ap, focus=FOCUS):
        r.camera_lens_rays(cam, W, H, None, pattern[S], lens[S, ap], focus, rays.data_ptr())
        r.trace_radiance_resolve_device(rays.data_ptr(), n, S, D, F_RGB8, rgb.data_ptr())

    def fused(S, ap, focus=FOCUS):
        r.render_lens_samples_async(cam, W, H, D, pattern[S], lens[S, ap], focus, rgb.data_ptr())

    variants = {}
    for S in (4, 64):
        variants["a_pinhole_s%d" % S] = lambda S=S: pinhole(S)
        for ap in (0, 1):
            variants["b_rays_resolve_s%d_ap%d" % (S, ap)] = lambda S=S, ap=ap: buffered(S, ap)
            variants["c_fused_lens_s%d_ap%d" % (S, ap)] = lambda S=S, ap=ap: fused(S, ap)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(side)
        fn()
        e1.record(side)
        st = r.radiance_stats()  # waits for the stream
        wall = (time.perf_counter() - t0) * 1e3
        e1.synchronize()
        return e0.elapsed_time(e1), st.kernel_ms, wall, st

    def image(fn):
        rgb.zero_()
        torch.cuda.synchronize()
        fn()
        r.radiance_stats()
        return rgb.cpu().numpy().tobytes()

    checks = {}
    for S in (4, 64):  # the pinhole limit: a zero lens and focus 1.0 write (a)'s bytes by both routes
        ref = image(lambda: pinhole(S))
        assert image(lambda: buffered(S, 0, 1.0)) == ref and image(lambda: fused(S, 0, 1.0)) == ref, S
        for ap in (0, 1):  # warm-up of every shape, and the bytes
            b, c = image(lambda: buffered(S, ap)), image(lambda: fused(S, ap))
            assert b == c, (S, ap)
            differ = int((np.frombuffer(ref, np.uint8).reshape(n, 3) != np.frombuffer(c, np.uint8).reshape(n, 3))
                         .any(axis=1).sum())
            checks["s%d_ap%d_pixels_differing_from_pinhole" % (S, ap)] = differ
    gpu = {k: [] for k in variants}
    kernel = {k: [] for k in variants}
    wall = {k: [] for k in variants}
    stats = {}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            g, k, w, st = timed(fn)
            gpu[name].append(g)
            kernel[name].append(k)
            wall[name].append(w)
            stats[name] = {"rays": st.rays, "segments": st.segments, "shadow_rays": st.shadow_rays,
                           "tests_exact": st.tests_exact, "tests_cull": st.tests_cull}

    def summary(runs):
        return {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                    "runs": [round(x, 3) for x in v]} for k, v in runs.items()}

    ndev = torch.cuda.device_count()
    out = {"scene": "synth200", "width": W, "height": H, "depth": D, "rounds": ROUNDS, "focus": FOCUS,
           "aperture": {"ap0": 0.0, "ap1": APERTURE},
           "device": torch.cuda.get_device_name(0), "devices": ndev,
           "distinct_device_group_rows": "not measured" + (": one device" if ndev < 2 else ""),
           "ray_buffer_bytes": {"s4": n * 4 * 64, "s64": n * 64 * 64},
           "checks": checks, "counts": stats,
           "gpu_ms": summary(gpu), "kernel_ms": summary(kernel), "wall_ms": summary(wall)}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    r.set_stream(None)
    r.close()


if __name__ == "__main__":
    main()
