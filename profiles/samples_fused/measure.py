"""What the fused and the group forms of rt_render_samples cost, beside the call they come from:
synth200 at 1920x1080 depth 4, RT_FB_RGB8 into device memory (the workload of
profiles/radiance_samples/measure.py), with the antialias pattern (4 samples) and, for the new calls,
with grid_pattern(8) (64 samples).

 (a) rt_render_samples at max_ray_bytes of 256 MiB (the default: two chunks) and 1 GiB (one chunk):
     the sum of its resolve kernels' event times and the call's wall time;
 (f) rt_render_samples_async: its one kernel's event time, and the wall time of the call followed by
     rt_radiance_stats_get (a stream synchronise);
 (g) rt_group_render_samples with devices [0], [0, 0] and [0, 0, 0, 0] -- REPEATED devices: the shards
     share one GPU, so these rows show the group's overhead, not scaling -- and, where the machine has
     them, with 2, 4 and 8 distinct devices: kernel_ms is the largest member's, wall the whole call.

One process; every variant is warmed once and checked (the 4-sample variants write rt_render's bytes
under rt_set_antialias(4), the 64-sample ones rt_render_samples'); the variants alternate within each of
the ROUNDS rounds; medians, min-max and every run are recorded.  Wall times are a host clock around
calls that end in a device synchronise.

    python profiles/samples_fused/measure.py [out.json]
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

W, H, D, ROUNDS = 1920, 1080, 4, 7
MIB = 1 << 20
CAPS = {"256MiB": 256 * MIB, "1GiB": 1024 * MIB}
REPEATED = {"0": [0], "0,0": [0, 0], "0,0,0,0": [0, 0, 0, 0]}


def main():
    scene = rt_hip.Scene.load(os.path.join(REPO, "cs420-ray-tracer_amd", "scenes", "synth200.txt"))
    cam = scene.camera()
    p4, p64 = rt_hip.grid_pattern(2), rt_hip.grid_pattern(8)
    n = W * H
    r, aa = rt_hip.Renderer(0), rt_hip.Renderer(0)
    r.upload(scene)
    aa.upload(scene)
    aa.set_antialias(4)
    rgb = torch.zeros((n * 3,), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ndev = torch.cuda.device_count()
    lists = dict(REPEATED)
    for g in (2, 4, 8):
        if ndev >= g:
            lists["distinct%d" % g] = list(range(g))
    groups = {}
    for key, devs in lists.items():
        groups[key] = rt_hip.Group(devs, band=8)
        groups[key].upload(scene)

    def samples(cap, pattern=p4):
        _, st = r.render_samples(cam, W, H, D, pattern, out=rgb.data_ptr(), out_on_device=True, max_ray_bytes=cap)
        return st.kernel_ms

    def fused(pattern):
        r.render_samples_async(cam, W, H, D, pattern, rgb.data_ptr())
        return r.radiance_stats().kernel_ms  # waits for the stream

    def group(key, pattern):
        _, st = groups[key].render_samples(cam, W, H, D, pattern, out=rgb, out_on_device=True)
        return st.kernel_ms

    variants = {"a_render_samples_" + k: (lambda c=c: samples(c)) for k, c in CAPS.items()}
    variants["f_fused_s4"] = lambda: fused(p4)
    for key in lists:
        variants["g_group[%s]_s4" % key] = lambda key=key: group(key, p4)
    variants["f_fused_s64"] = lambda: fused(p64)
    for key in lists:
        variants["g_group[%s]_s64" % key] = lambda key=key: group(key, p64)

    aa.render(cam, W, H, D, out=rgb, out_on_device=True)
    ref = {"s4": rgb.cpu().numpy().tobytes()}
    samples(0, p64)
    ref["s64"] = rgb.cpu().numpy().tobytes()
    for name, fn in variants.items():  # warm-up of every shape, and the bytes
        rgb.zero_()
        torch.cuda.synchronize()
        fn()
        assert rgb.cpu().numpy().tobytes() == ref["s64" if name.endswith("_s64") else "s4"], name
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

    out = {"scene": "synth200", "width": W, "height": H, "depth": D, "rounds": ROUNDS,
           "device": torch.cuda.get_device_name(0), "devices": ndev,
           "distinct_device_rows": "measured" if ndev > 1 else "not measured: one device",
           "repeated_device_rows": "overhead on one GPU, not scaling",
           "rays": {"s4": n * 4, "s64": n * 64},
           "kernel_ms": summary(kernel), "wall_ms": summary(wall)}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    for g in groups.values():
        g.close()
    r.close()
    aa.close()


if __name__ == "__main__":
    main()
