"""Throughput of the ray queries (rt_trace_rays_async), with the same
context's one-frame depth-1 render of the same view beside it as the yardstick.

For synth200 and complex: the 1920x1080 camera rays of the scene's view from
rt_camera_rays, both modes.  For synth10k: 2 M rays of the tests' generator
(tests/ray_ref.py gen_rays, seed 1), both modes, with the render of the scene's
own 1920x1080 view beside them.  Per case: the in-stream HIP-event time of the
query kernel (rt_trace_stats), median of 5 launches after one warm-up launch,
Mrays/s from it, tests_exact / (rays * spheres) and rays_unaccelerated.
Everything stays in device memory.  Nothing here is a pass/fail number.

    python profiles/ray_queries/measure.py [out.json]
"""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.abspath(__file__))
while not os.path.isdir(os.path.join(REPO, "cs420-ray-tracer_amd")):  # from any directory of the repository
    REPO = os.path.dirname(REPO)
sys.path.insert(0, os.path.join(REPO, "cs420-ray-tracer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import ray_ref  # noqa: E402
import rt_hip  # noqa: E402

W, H, ROUNDS, N_GEN = 1920, 1080, 5, 2_000_000
MODES = {"closest": rt_hip.RT_QUERY_CLOSEST, "occluded": rt_hip.RT_QUERY_OCCLUDED}


def query(r, rays, n, spheres):
    hits = torch.zeros((n, 2), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    out = {}
    for name, mode in MODES.items():
        r.trace_rays_device(rays.data_ptr(), n, hits.data_ptr(), mode)  # warm-up
        r.trace_stats()
        ms, st = [], None
        for _ in range(ROUNDS):
            r.trace_rays_device(rays.data_ptr(), n, hits.data_ptr(), mode)
            st = r.trace_stats()
            ms.append(st.kernel_ms)
        med = statistics.median(ms)
        out[name] = {"kernel_ms": round(med, 4), "kernel_ms_runs": [round(x, 4) for x in ms],
                     "mrays_per_s": round(n / med / 1e3, 1), "hits": st.hits,
                     "tests_exact_per_pair": round(st.tests_exact / (n * spheres), 6),
                     "tests_cull": st.tests_cull, "rays_unaccelerated": st.rays_unaccelerated}
    return out


def render_depth1(r, cam):
    img = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS + 1):
        _, st = r.render(cam, W, H, 1, out=img, out_on_device=True)
        ms.append(st.kernel_ms)
    return {"kernel_ms": round(statistics.median(ms[1:]), 4), "kernel_ms_runs": [round(x, 4) for x in ms[1:]],
            "mrays_per_s_primary": round(W * H / statistics.median(ms[1:]) / 1e3, 1)}


def main():
    out = {"device": torch.cuda.get_device_name(0), "width": W, "height": H, "rounds": ROUNDS, "cases": {}}
    r = rt_hip.Renderer(0)
    for name in ("synth200", "complex", "synth10k"):
        scene = rt_hip.Scene.load(os.path.join(REPO, "cs420-ray-tracer_amd", "scenes", name + ".txt"))
        cam = scene.camera()
        r.upload(scene)
        if name == "synth10k":
            c, rad = ray_ref.spheres_of(scene)
            o, d = ray_ref.gen_rays(1, N_GEN, c, rad, tuple(cam.position))
            host = np.zeros((N_GEN, 8), np.float64)
            host[:, 0:3], host[:, 3:6], host[:, 6] = o, d, np.inf
            rays, n, kind = torch.from_numpy(host).to("cuda:0"), N_GEN, "generator rays (tests/ray_ref.py, seed 1)"
        else:
            n, kind = W * H, "camera rays (rt_camera_rays)"
            rays = torch.zeros((n, 8), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            r.camera_rays(cam, W, H, None, rays.data_ptr())
        case = {"spheres": scene.num_spheres, "rays": n, "kind": kind}
        case.update(query(r, rays, n, scene.num_spheres))
        case["render_depth1"] = render_depth1(r, cam)
        out["cases"][name] = case
    r.close()
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
