"""Wall time per frame of a 64-frame sequence on the device group
(rt_group_render_frames) against the two things it is judged by: (i) 64
one-frame rt_group_render calls on the same group, the only route before the
sequence call existed, and (ii) two direct 32-frame rt_render_frames_async
launches on a plain context, which pay no staging and no placement.

synth200 at 1920x1080 depth 4, the static view, every image in device memory
(out_on_device).  One process; every shape is warmed once; the variants
alternate within each of the 5 rounds and the median per variant is reported.
A host clock around calls that end in a device synchronise (every group call
is synchronous; (ii) ends in rt_render_stats, which waits for the stream).
All members live on device 0: nothing here runs on more than one physical GPU.

    python profiles/group_frames/measure.py [out.json]
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

W, H, D, F, BATCH, ROUNDS = 1920, 1080, 4, 64, 32, 5
N = W * H * 3


def main():
    scene = rt_hip.Scene.load(os.path.join(REPO, "cs420-ray-tracer_amd", "scenes", "synth200.txt"))
    cam = scene.camera()
    cams, cams_batch = rt_hip.camera_array([cam] * F), rt_hip.camera_array([cam] * BATCH)
    buf = torch.zeros((F, N), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    groups = {1: rt_hip.Group([0]), 2: rt_hip.Group([0, 0])}
    for g in groups.values():
        g.upload(scene)
    plain = rt_hip.Renderer(0)
    plain.upload(scene)
    ref, _ = plain.render(cam, W, H, D)
    ref = bytes(ref)

    def sequence(G):
        groups[G].render_frames(cams, W, H, D, batch=BATCH, out=buf, out_on_device=True, frame_stride=N)

    def singles(G):
        for f in range(F):
            groups[G].render(cam, W, H, D, out=buf[f], out_on_device=True)

    def direct():
        for b in range(F // BATCH):
            plain.render_frames_async(cams_batch, W, H, D, None, buf[b * BATCH].data_ptr(), N)
        plain.stats()

    variants = {"group_frames_1": lambda: sequence(1), "group_frames_2": lambda: sequence(2),
                "group_render_x64_1": lambda: singles(1), "group_render_x64_2": lambda: singles(2),
                "direct_2x32": direct}
    times = {k: [] for k in variants}
    for name, fn in variants.items():  # warm-up of every shape, and the images are the plain render's
        buf.zero_()
        torch.cuda.synchronize()
        fn()
        host = buf.cpu().numpy()
        assert all(host[f].tobytes() == ref for f in (0, 1, BATCH - 1, BATCH, F - 1)), name
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3 / F)
    out = {"scene": "synth200", "width": W, "height": H, "depth": D, "frames": F, "batch": BATCH, "rounds": ROUNDS,
           "device": torch.cuda.get_device_name(0), "physical_devices_used": 1,
           "ms_per_frame_median": {k: round(statistics.median(v), 4) for k, v in times.items()},
           "ms_per_frame_runs": {k: [round(x, 4) for x in v] for k, v in times.items()}}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    for g in groups.values():
        g.close()
    plain.close()


if __name__ == "__main__":
    main()
