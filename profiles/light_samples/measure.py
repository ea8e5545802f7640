"""What the light table costs in the multi-sample renders: complex.txt (154 spheres, 5 lights) at 1920x1080
depth 4, 16 samples (grid_pattern(4)), RT_FB_RGB8 into device memory, through the two fused launches:

 (a) rt_render_samples_async, the pinhole launch;
 (b) rt_render_lens_samples_async, lens_pattern(4, 0.3) focused at 30 units;

each without a table (radiance_kernel<true, true[, true]>, the launch as it was), with a table of radius 0
(the kArea instantiation reading rows that all hold the uploaded positions: the mechanism alone) and with
light_pattern(4, 0.5, 5) (the mechanism and what soft shadows do to the rays: a wave's shadow rays of one
sample still meet in one point, but the point moves from sample to sample).

One process, one device; every variant is warmed once and checked (radius 0 writes the bytes of no table);
the variants alternate within each of the ROUNDS rounds, the table set by rt_set_light_samples outside the
timed region (it is context state: a frame sequence sets it once); medians, min-max and every run are
recorded.  gpu_ms is the time between two events on the context's stream around the launch, kernel_ms what
rt_radiance_stats_get reports, set_ms a host clock around one rt_set_light_samples (16 x 5 records).

    python profiles/light_samples/measure.py [out.json]
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

W, H, D, N, ROUNDS = 1920, 1080, 4, 4, 7
FOCUS, APERTURE, RADIUS = 30.0, 0.3, 0.5


def main():
    scene = rt_hip.Scene.load(os.path.join(REPO, "cs420-ray-tracer_amd", "scenes", "complex.txt"))
    cam = scene.camera()
    n = W * H
    r = rt_hip.Renderer(0)
    r.upload(scene)
    side = torch.cuda.Stream()
    r.set_stream(side.cuda_stream)
    rgb = torch.zeros((n * 3,), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    pattern, lens = rt_hip.grid_pattern(N), rt_hip.lens_pattern(N, APERTURE)
    tables = {"none": None, "r0": rt_hip.light_pattern(N, 0.0, scene.num_lights),
              "r05": rt_hip.light_pattern(N, RADIUS, scene.num_lights)}

    def pinhole():
        r.render_samples_async(cam, W, H, D, pattern, rgb.data_ptr())

    def through_lens():
        r.render_lens_samples_async(cam, W, H, D, pattern, lens, FOCUS, rgb.data_ptr())

    forms = {"a_pinhole": pinhole, "b_lens": through_lens}
    variants = [(f, t) for f in forms for t in tables]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        fn()
        e1.record(side)
        st = r.radiance_stats()  # waits for the stream
        e1.synchronize()
        return e0.elapsed_time(e1), st.kernel_ms, st

    def image(fn):
        rgb.zero_()
        torch.cuda.synchronize()
        fn()
        r.radiance_stats()
        return rgb.cpu().numpy().tobytes()

    checks, set_ms = {}, []
    for f, fn in forms.items():  # warm-up of every shape, and the bytes
        img = {}
        for t, table in tables.items():
            r.set_light_samples(table)
            img[t] = image(fn)
        assert img["r0"] == img["none"], f
        a, b = (np.frombuffer(img[t], np.uint8).reshape(n, 3) for t in ("none", "r05"))
        checks[f + "_pixels_differing_from_no_table"] = int((a != b).any(axis=1).sum())
    gpu = {"%s_%s" % v: [] for v in variants}
    kernel = {k: [] for k in gpu}
    stats = {}
    for _ in range(ROUNDS):
        for f, t in variants:
            t0 = time.perf_counter()
            r.set_light_samples(tables[t])
            if tables[t] is not None:
                set_ms.append((time.perf_counter() - t0) * 1e3)
            g, k, st = timed(forms[f])
            name = "%s_%s" % (f, t)
            gpu[name].append(g)
            kernel[name].append(k)
            stats[name] = {"rays": st.rays, "segments": st.segments, "hits": st.hits, "shadow_rays": st.shadow_rays,
                           "unaccelerated": st.unaccelerated, "tests_exact": st.tests_exact,
                           "tests_cull": st.tests_cull}
    r.set_light_samples(None)

    def summary(runs):
        return {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                    "runs": [round(x, 3) for x in v]} for k, v in runs.items()}

    out = {"scene": "complex", "width": W, "height": H, "depth": D, "samples": N * N, "rounds": ROUNDS,
           "focus": FOCUS, "aperture": APERTURE, "light_radius": {"r0": 0.0, "r05": RADIUS},
           "device": torch.cuda.get_device_name(0), "devices": torch.cuda.device_count(),
           "table_bytes": N * N * scene.num_lights * 48,
           "checks": checks, "counts": stats,
           "gpu_ms": summary(gpu), "kernel_ms": summary(kernel), "set_ms": summary({"rt_set_light_samples": set_ms})}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    r.set_stream(None)
    r.close()


if __name__ == "__main__":
    main()
