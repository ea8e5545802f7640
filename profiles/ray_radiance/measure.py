"""Kernel time of the radiance queries (rt_trace_radiance_async) in each output
format, with two yardsticks measured in the same run beside each case:

  (a) rt_trace_paths_async with surfaces over the same rays: everything the
      radiance kernel does except the Phong terms and the compositing, plus 128
      bytes of records per level per ray that the radiance kernel does not write;
  (b) the context's one-frame render of the same view at the same depth (for
      the generator rays of synth10k: of the scene's own 1920x1080 view).

Workloads, as profiles/ray_paths/measure.py: the 1920x1080 camera rays
(rt_camera_rays) of synth200 and complex at depth 4, and 2 M rays of the tests'
generator (tests/ray_ref.py gen_rays, seed 1) in synth10k at depth 6.  Per
launch the in-stream HIP-event time of its kernel (rt_radiance_stats_get /
rt_path_stats_get / rt_render's stats), median of 5 after one warm-up.
Everything stays in device memory.  Nothing here is a pass/fail number.

    python profiles/ray_radiance/measure.py [out.json]     (default: ray_radiance.json beside this script)
"""
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = HERE
while not os.path.isdir(os.path.join(REPO, "cs420-ray-tracer_amd")):  # from any directory of the repository
    REPO = os.path.dirname(REPO)
sys.path.insert(0, os.path.join(REPO, "cs420-ray-tracer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import ray_ref  # noqa: E402
import rt_hip  # noqa: E402

W, H, ROUNDS, N_GEN = 1920, 1080, 5, 2_000_000
FORMATS = (("f64x3", rt_hip.RT_FB_F64X3, 24), ("f32x3", rt_hip.RT_FB_F32X3, 12), ("rgb8", rt_hip.RT_FB_RGB8, 3))


def median_ms(launch, stats):
    launch()
    stats()
    ms, st = [], None
    for _ in range(ROUNDS):
        launch()
        st = stats()
        ms.append(st.kernel_ms)
    return statistics.median(ms), [round(x, 4) for x in ms], st


def radiance(r, rays, n, depth, fmt, size):
    out = torch.zeros((n * size + 16,), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    med, runs, st = median_ms(lambda: r.trace_radiance_device(rays.data_ptr(), n, depth, fmt, out.data_ptr()),
                              r.radiance_stats)
    queries = st.segments + st.shadow_rays
    return {"kernel_ms": round(med, 4), "kernel_ms_runs": runs, "segments": st.segments, "hits": st.hits,
            "shadow_rays": st.shadow_rays, "mqueries_per_s": round(queries / med / 1e3, 1),
            "tests_exact": st.tests_exact, "tests_cull": st.tests_cull, "unaccelerated": st.unaccelerated,
            "negative_clamped": st.negative_clamped}


def paths_surfaces(r, rays, n, depth):
    """Yardstick (a)."""
    verts = torch.zeros((depth * n * 32,), dtype=torch.uint8, device="cuda:0")
    surf = torch.zeros((depth * n * 96,), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    med, runs, st = median_ms(
        lambda: r.trace_paths_device(rays.data_ptr(), n, depth, verts.data_ptr(), surf.data_ptr()), r.path_stats)
    return {"kernel_ms": round(med, 4), "kernel_ms_runs": runs, "segments": st.segments, "hits": st.hits,
            "shadow_rays": st.shadow_rays, "tests_exact": st.tests_exact, "tests_cull": st.tests_cull,
            "unaccelerated": st.unaccelerated}


def render(r, cam, depth):
    """Yardstick (b)."""
    img = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ms, st = [], None
    for _ in range(ROUNDS + 1):
        _, st = r.render(cam, W, H, depth, out=img, out_on_device=True)
        ms.append(st.kernel_ms)
    return {"kernel_ms": round(statistics.median(ms[1:]), 4), "kernel_ms_runs": [round(x, 4) for x in ms[1:]],
            "rays": {"primary": st.rays_primary, "reflect": st.rays_reflect, "shadow": st.rays_shadow}}


def main():
    out = {"device": torch.cuda.get_device_name(0), "width": W, "height": H, "rounds": ROUNDS, "cases": {}}
    r = rt_hip.Renderer(0)
    for name, depth in (("synth200", 4), ("complex", 4), ("synth10k", 6)):
        scene = rt_hip.Scene.load(os.path.join(REPO, "cs420-ray-tracer_amd", "scenes", name + ".txt"))
        cam = scene.camera()
        r.upload(scene)
        if name == "synth10k":
            c, rad = ray_ref.spheres_of(scene)
            o, d = ray_ref.gen_rays(1, N_GEN, c, rad, tuple(cam.position))
            n, kind = N_GEN, "generator rays (tests/ray_ref.py, seed 1)"
            rec = np.zeros((n, 8), np.float64)
            rec[:, 0:3], rec[:, 3:6], rec[:, 6] = o, d, np.inf
            rays = torch.from_numpy(rec).to("cuda:0")
        else:
            n, kind = W * H, "camera rays (rt_camera_rays)"
            rays = torch.zeros((n, 8), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            r.camera_rays(cam, W, H, None, rays.data_ptr())
        case = {"spheres": scene.num_spheres, "lights": scene.num_lights, "rays": n, "depth": depth, "kind": kind}
        case["radiance"] = {tag: radiance(r, rays, n, depth, fmt, size) for tag, fmt, size in FORMATS}
        case["paths_surfaces"] = paths_surfaces(r, rays, n, depth)
        case["render"] = render(r, cam, depth)
        f64 = case["radiance"]["f64x3"]
        case["same_work_as_paths"] = all(f64[k] == case["paths_surfaces"][k] for k in ("segments", "hits", "shadow_rays"))
        case["radiance_over_paths"] = round(f64["kernel_ms"] / case["paths_surfaces"]["kernel_ms"], 3)
        case["radiance_over_render"] = round(f64["kernel_ms"] / case["render"]["kernel_ms"], 3)
        out["cases"][name] = case
    r.close()
    text = json.dumps(out, indent=1)
    print(text)
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ray_radiance.json"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
