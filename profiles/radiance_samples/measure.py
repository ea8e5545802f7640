"""What four samples per pixel cost by each route, synth200 at 1920x1080 depth 4
with the antialias pattern (0,0) (.5,0) (0,.5) (.5,.5):

 (a) rt_render_samples, RT_FB_RGB8 into device memory: the sum of its resolve
     kernels' event times (rt_radiance_stats.kernel_ms) and the call's wall time
     (which adds the ray generation and the per-chunk synchronise), at
     max_ray_bytes of 64 MiB, 256 MiB (the default) and 1 GiB;
 (b) rt_trace_radiance RT_FB_F64X3 over the same 4*W*H rays, already on the
     device: what a caller paid before, ahead of a reduction of their own.  Its
     kernel event time and its wall time;
 (c) rt_render under rt_set_antialias(4) into device memory: the render kernel's
     event time and the call's wall time.

One process; every variant is warmed once and checked (a's bytes are c's); the
variants alternate within each of the ROUNDS rounds; medians and every run are
recorded, and (b)'s own spread is what (a) - (b) is judged against.  Wall times
are a host clock around calls that end in a device synchronise.

    python profiles/radiance_samples/measure.py [out.json]
"""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "cs420-ray-tracer_amd"))

import torch  # noqa: E402
import rt_hip  # noqa: E402

W, H, D, S, ROUNDS = 1920, 1080, 4, 4, 7
MIB = 1 << 20
CAPS = {"64MiB": 64 * MIB, "256MiB": 256 * MIB, "1GiB": 1024 * MIB}


def main():
    scene = rt_hip.Scene.load(os.path.join(REPO, "cs420-ray-tracer_amd", "scenes", "synth200.txt"))
    cam = scene.camera()
    pattern = rt_hip.grid_pattern(2)
    n = W * H
    r, aa = rt_hip.Renderer(0), rt_hip.Renderer(0)
    r.upload(scene)
    aa.upload(scene)
    aa.set_antialias(4)
    rgb = torch.zeros((n * 3,), dtype=torch.uint8, device="cuda:0")
    rays = torch.zeros((n * S, 8), dtype=torch.float64, device="cuda:0")
    f64 = torch.zeros((n * S, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    r.camera_sample_rays(cam, W, H, None, pattern, rays.data_ptr())
    r.radiance_stats()  # waits for the stream

    def samples(cap):
        _, st = r.render_samples(cam, W, H, D, pattern, out=rgb.data_ptr(), out_on_device=True, max_ray_bytes=cap)
        return st.kernel_ms

    def per_ray():
        r.trace_radiance_device(rays.data_ptr(), n * S, D, rt_hip.RT_FB_F64X3, f64.data_ptr())
        return r.radiance_stats().kernel_ms

    def render():
        _, st = aa.render(cam, W, H, D, out=rgb, out_on_device=True)
        return st.kernel_ms

    variants = {"a_render_samples_" + k: (lambda c=c: samples(c)) for k, c in CAPS.items()}
    variants["b_trace_radiance_f64"] = per_ray
    variants["c_render_antialias"] = render
    render()
    ref = rgb.cpu().numpy().tobytes()
    for name, fn in variants.items():  # warm-up of every shape; (a) writes (c)'s bytes
        rgb.zero_()
        torch.cuda.synchronize()
        fn()
        if name[0] != "b":
            assert rgb.cpu().numpy().tobytes() == ref, name
    kernel = {k: [] for k in variants}
    wall = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            ms = fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            kernel[name].append(ms)

    def summary(runs):
        return {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                    "runs": [round(x, 3) for x in v]} for k, v in runs.items()}

    out = {"scene": "synth200", "width": W, "height": H, "depth": D, "samples": S, "rounds": ROUNDS,
           "device": torch.cuda.get_device_name(0), "rays": n * S,
           "kernel_ms": summary(kernel), "wall_ms": summary(wall)}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    r.close()
    aa.close()


if __name__ == "__main__":
    main()
