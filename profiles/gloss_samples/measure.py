"""What the gloss table costs in the fused multi-sample launch: synth200.txt (200 spheres, 143 of them
reflective, roughness 0.5) at 1920x1080 depth 4, 16 samples (grid_pattern(4)), RT_FB_RGB8 into device memory,
through rt_render_samples_async:

  none       no table: radiance_kernel<true, true>, the launch as it was;
  none_again the same variant a second time in every round: the spread of one and the same code;
  zero       an all-zero table with the file's roughness: the kGloss instantiation bending nothing (rd + 0 *
             roughness), the mechanism alone -- it writes the bytes of no table;
  gloss      gloss_pattern(4, 3) with the file's roughness: the mechanism and what bent reflection rays do to
             the chains (they lose their coherence within a wave);
  parent     with --parent LIB: `none` on a build of the parent commit, loaded into the same process.

One process, one device; every variant is warmed once and checked; the variants alternate within each of
the ROUNDS rounds, the table set by rt_set_gloss_samples outside the timed region (it is context state: a
frame sequence sets it once); medians, min-max and every run are recorded.  gpu_ms is the time between two
events on the context's stream around the launch, kernel_ms what rt_radiance_stats_get reports, set_ms a
host clock around one rt_set_gloss_samples (16 x 3 points, 200 roughness values).

    python profiles/gloss_samples/measure.py [--parent librt_hip_parent.so] [out.json]
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

W, H, D, N, B, ROUNDS = 1920, 1080, 4, 4, 3, 7


def parent_renderer(path):
    """A context of a build that predates the gloss entries: rt_hip binds what it has (RT_HIP_LIB's rule)."""
    os.environ["RT_HIP_LIB"] = path
    try:
        rt_hip.lib(path)
    finally:
        del os.environ["RT_HIP_LIB"]
    rt_hip.VARIANTS["parent"] = path
    return rt_hip.Renderer(0, variant="parent")


def main():
    args = sys.argv[1:]
    parent = None
    if args[:1] == ["--parent"]:
        parent, args = os.path.abspath(args[1]), args[2:]
    path = os.path.join(REPO, "cs420-ray-tracer_amd", "scenes", "synth200.txt")
    scene = rt_hip.Scene.load(path)
    rough = rt_hip.scene_roughness(path)
    cam = scene.camera()
    n = W * H
    side = torch.cuda.Stream()
    ctx = {"new": rt_hip.Renderer(0)}
    if parent:
        ctx["parent"] = parent_renderer(parent)
    for r in ctx.values():
        r.upload(scene)
        r.set_stream(side.cuda_stream)
    rgb = torch.zeros((n * 3,), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    pattern = rt_hip.grid_pattern(N)
    tables = {"none": None, "none_again": None, "zero": np.zeros((N * N, B, 3)), "gloss": rt_hip.gloss_pattern(N, B)}
    variants = [("new", t) for t in tables] + ([("parent", "none")] if parent else [])

    def name(v):
        return v[1] if v[0] == "new" else "parent"

    def prepare(v):
        if v[0] == "new":
            ctx["new"].set_gloss_samples(rough, tables[v[1]])

    def timed(r):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        r.render_samples_async(cam, W, H, D, pattern, rgb.data_ptr())
        e1.record(side)
        st = r.radiance_stats()  # waits for the stream
        e1.synchronize()
        return e0.elapsed_time(e1), st.kernel_ms, st

    def image(r):
        rgb.zero_()
        torch.cuda.synchronize()
        r.render_samples_async(cam, W, H, D, pattern, rgb.data_ptr())
        r.radiance_stats()
        return rgb.cpu().numpy().tobytes()

    img = {}
    for v in variants:  # warm-up of every variant, and the bytes
        prepare(v)
        img[name(v)] = image(ctx[v[0]])
    assert img["zero"] == img["none"] == img["none_again"]
    assert parent is None or img["parent"] == img["none"]
    a, b = (np.frombuffer(img[t], np.uint8).reshape(n, 3) for t in ("none", "gloss"))
    checks = {"gloss_pixels_differing_from_no_table": int((a != b).any(axis=1).sum())}
    gpu = {name(v): [] for v in variants}
    kernel = {k: [] for k in gpu}
    stats, set_ms = {}, []
    for _ in range(ROUNDS):
        for v in variants:
            t0 = time.perf_counter()
            prepare(v)
            if v[0] == "new" and tables[v[1]] is not None:
                set_ms.append((time.perf_counter() - t0) * 1e3)
            g, k, st = timed(ctx[v[0]])
            gpu[name(v)].append(g)
            kernel[name(v)].append(k)
            stats[name(v)] = {"rays": st.rays, "segments": st.segments, "hits": st.hits, "shadow_rays": st.shadow_rays,
                              "unaccelerated": st.unaccelerated, "tests_exact": st.tests_exact,
                              "tests_cull": st.tests_cull}
    ctx["new"].set_gloss_samples(None, None)

    def summary(runs):
        return {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                    "runs": [round(x, 3) for x in v]} for k, v in runs.items()}

    out = {"scene": "synth200", "width": W, "height": H, "depth": D, "samples": N * N, "bounces": B, "rounds": ROUNDS,
           "device": torch.cuda.get_device_name(0), "devices": torch.cuda.device_count(),
           "table_bytes": N * N * B * 24 + len(rough) * 8, "parent_build": bool(parent),
           "checks": checks, "counts": stats,
           "gpu_ms": summary(gpu), "kernel_ms": summary(kernel), "set_ms": summary({"rt_set_gloss_samples": set_ms})}
    text = json.dumps(out, indent=1)
    print(text)
    if args:
        with open(args[0], "w") as f:
            f.write(text + "\n")
    for r in ctx.values():
        r.set_stream(None)
        r.close()


if __name__ == "__main__":
    main()
