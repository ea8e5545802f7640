"""Kernel time of the path queries (rt_trace_paths_async), with two yardsticks
measured in the same run beside each case:

  (a) the sum of the rt_trace_rays launches that answer the same questions from
      prepared device buffers: per level one closest launch over that level's
      rays and one occluded launch over its shadow rays (hits x lights, tmax =
      the light distance).  The buffers are built on the host from the path
      query's own output before anything is timed; building them (what a caller
      without rt_trace_paths would have to do between the launches) is not
      counted.
  (b) the context's one-frame render of the same view at the same depth (for
      the generator rays of synth10k: of the scene's own 1920x1080 view).

Workloads: the 1920x1080 camera rays (rt_camera_rays) of synth200 and complex
at depth 4, and 2 M rays of the tests' generator (tests/ray_ref.py gen_rays,
seed 1) in synth10k at depth 6, each with and without surfaces.  Per launch the
in-stream HIP-event time of its kernel (rt_path_stats_get / rt_trace_stats /
rt_render's stats), median of 5 after one warm-up.  Everything stays in device
memory.  Nothing here is a pass/fail number.

    python profiles/ray_paths/measure.py [out.json]
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
EPSILON = 0.001


def median_ms(launch, stats):
    launch()
    stats()
    ms, st = [], None
    for _ in range(ROUNDS):
        launch()
        st = stats()
        ms.append(st.kernel_ms)
    return statistics.median(ms), [round(x, 4) for x in ms], st


def paths(r, rays, n, depth, surfaces):
    verts = torch.zeros((depth * n * 32,), dtype=torch.uint8, device="cuda:0")
    surf = torch.zeros((depth * n * 96,), dtype=torch.uint8, device="cuda:0") if surfaces else None
    torch.cuda.synchronize()
    med, runs, st = median_ms(
        lambda: r.trace_paths_device(rays.data_ptr(), n, depth, verts.data_ptr(), surf.data_ptr() if surfaces else 0),
        r.path_stats)
    queries = st.segments + st.shadow_rays
    out = {"kernel_ms": round(med, 4), "kernel_ms_runs": runs, "segments": st.segments, "hits": st.hits,
           "shadow_rays": st.shadow_rays, "mqueries_per_s": round(queries / med / 1e3, 1),
           "tests_exact": st.tests_exact, "tests_cull": st.tests_cull, "unaccelerated": st.unaccelerated}
    return out, verts, surf


def ray_records(o, d, tmax):
    rec = np.zeros((o.shape[0], 8), np.float64)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6] = o, d, tmax
    return torch.from_numpy(rec).to("cuda:0")


def separate_launches(r, scene, host_rays, verts, surf, depth):
    """Yardstick (a): the per-level closest and occluded launches."""
    n = host_rays.shape[0]
    v = verts.cpu().numpy().view(rt_hip.VERTEX_DTYPE).reshape(depth, n)
    s = surf.cpu().numpy().view(rt_hip.SURFACE_DTYPE).reshape(depth, n)
    lights = np.array([scene.light(i)["position"] for i in range(scene.num_lights)], np.float64).reshape(-1, 3)
    levels, total = [], 0.0
    org = host_rays[:, 0:3]
    for k in range(depth):
        tr = (v[k]["flags"] & rt_hip.RT_VERTEX_TRACED) != 0
        if not tr.any():
            break
        hit = tr & (v[k]["sphere"] >= 0)
        hp = s[k]["hit"][hit]
        with np.errstate(all="ignore"):
            so, sd, dist = [], [], []
            for L in lights:
                to_light = L[None, :] - hp
                ln = np.sqrt((to_light[:, 0] ** 2 + to_light[:, 1] ** 2) + to_light[:, 2] ** 2)
                ldir = to_light / ln[:, None]
                so.append(hp + ldir * EPSILON)
                sd.append(ldir)
                dist.append(ln)
        lv = {"rays": int(tr.sum()), "shadow_rays": int(hit.sum()) * len(lights)}
        # level 0: the caller's own directions; deeper: the stored ones (normalising them again changes nothing measurable)
        buf = ray_records(org[tr], (host_rays[:, 3:6] if k == 0 else s[k]["dir"])[tr], np.inf)
        hits = torch.zeros((lv["rays"], 2), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        med, _, st = median_ms(lambda: r.trace_rays_device(buf.data_ptr(), lv["rays"], hits.data_ptr(),
                                                           rt_hip.RT_QUERY_CLOSEST), r.trace_stats)
        lv["closest_hits_equal"] = st.hits == int(hit.sum())
        lv["closest_ms"] = round(med, 4)
        total += med
        del buf, hits
        if lv["shadow_rays"]:
            buf = ray_records(np.concatenate(so), np.concatenate(sd), np.concatenate(dist))
            hits = torch.zeros((lv["shadow_rays"], 2), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            med, _, st = median_ms(lambda: r.trace_rays_device(buf.data_ptr(), lv["shadow_rays"], hits.data_ptr(),
                                                               rt_hip.RT_QUERY_OCCLUDED), r.trace_stats)
            shadowed = sum(int(((v[k]["shadowed"][hit] >> np.uint64(l)) & np.uint64(1)).sum())
                           for l in range(len(lights)))
            lv["occluded_equal"] = st.hits == shadowed  # the same answers
            lv["occluded_ms"] = round(med, 4)
            total += med
            del buf, hits
        levels.append(lv)
        org = s[k]["hit"] + s[k]["normal"] * EPSILON  # the next level's origins, where it is traced
    return {"kernel_ms_sum": round(total, 4), "launches": sum(1 + ("occluded_ms" in lv) for lv in levels),
            "levels": levels}


def render(r, cam, depth):
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
            rays = ray_records(o, d, np.inf)
        else:
            n, kind = W * H, "camera rays (rt_camera_rays)"
            rays = torch.zeros((n, 8), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            r.camera_rays(cam, W, H, None, rays.data_ptr())
        case = {"spheres": scene.num_spheres, "lights": scene.num_lights, "rays": n, "depth": depth, "kind": kind}
        case["paths"], _, _ = paths(r, rays, n, depth, False)
        case["paths_surfaces"], verts, surf = paths(r, rays, n, depth, True)
        case["separate_launches"] = separate_launches(r, scene, rays.cpu().numpy(), verts, surf, depth)
        del verts, surf
        case["render"] = render(r, cam, depth)
        a = case["separate_launches"]["kernel_ms_sum"]
        case["paths_over_separate"] = round(case["paths"]["kernel_ms"] / a, 3)
        case["paths_surfaces_over_separate"] = round(case["paths_surfaces"]["kernel_ms"] / a, 3)
        case["paths_over_render"] = round(case["paths"]["kernel_ms"] / case["render"]["kernel_ms"], 3)
        out["cases"][name] = case
    r.close()
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
