"""One context through the life of every buffer it owns: first allocation,
reuse, growth and a scene change, in one `Renderer` of the product library.

Every image is compared byte for byte, and every ray count, with the oracle
(orc.py), as tests/test_gpu_parity.py does.  The steps, in order:

 1. simple.txt, one frame 64x48 depth 3: no grids, no deferral.
 2. three frames from three camera positions: the lazy sphere grids, three
    camera grids at N = 128, the stack homes and the deferred queue.
 3. two frames from one position at 96x64 depth 6: homes and queue grow with
    the depth; the camera grid at N = 256 takes the second table slot.
 4. one frame at 256x256, then at 320x256: 1,024 and 1,280 tiles, the smallest
    launches at or above the tile-order threshold -- built, then grown.
 5. a synth scene of 1,100 spheres (the smallest count above the 1,024-sphere
    threshold, as the fuzz uses): the behind grid.
 6. simple.txt again: the behind grid is gone, step 1's bytes are back.
 7. render() to host memory at 32x32, then 128x96: the staging buffer.
 8. render_tiles into an RGB8 framebuffer with 2, then 5 unaligned tiles that
    cover more blocks: the block list and its growth (only the covering 8x8
    blocks are checked, and written).
 9. antialias 4, a 32x32 tile against orc_render_aa: the global stack.
10. info().scratch_bytes never decreases over steps 1-9.
11. step 2's launch enqueued again and the context closed at once; a new
    context then renders step 1's bytes.
"""
import numpy as np
import pytest

from conftest import diff_summary, scene_path

pytestmark = pytest.mark.gpu


def _moved(cam, k):
    """The scene camera moved sideways and zoomed a little, k steps (still a valid basis)."""
    import rt_hip

    c = rt_hip.rt_camera()
    for f in ("position", "forward", "right", "up"):
        getattr(c, f)[:] = list(getattr(cam, f))
    c.position[0] += 0.37 * k
    c.position[1] -= 0.11 * k
    c.scale = cam.scale * (1.0 + 0.05 * k)
    return c


class _Oracle:
    """The oracle's image and ray counts of (scene, camera, W, H, D), computed once each."""

    def __init__(self):
        self.scenes, self.done = {}, {}

    def add(self, key, **kw):
        import orc

        self.scenes[key] = orc.OracleScene(**kw)

    def render(self, key, cam, k, W, H, D):
        if (key, k, W, H, D) not in self.done:
            rgb, counts, _ = self.scenes[key].render(W, H, D, threads=4, camera=cam)
            self.done[(key, k, W, H, D)] = (rgb, counts)
        return self.done[(key, k, W, H, D)]


def _launch(r, orc_, key, cam, ks, W, H, D, wait=True):
    """One launch of len(ks) frames (camera moved ks[f] steps) into device memory,
    checked against the oracle; returns frame 0's bytes."""
    import torch

    cams = [_moved(cam, k) for k in ks]
    stride = H * W * 3
    buf = torch.full((len(ks) * stride,), 77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()  # the fill (torch's stream) lands before the render
    r.render_frames_async(cams, W, H, D, None, buf.data_ptr(), stride)
    if not wait:
        return buf
    st = r.stats()
    host = buf.cpu().numpy()
    total = {"primary": 0, "shadow": 0, "reflect": 0}
    for f, k in enumerate(ks):
        want, counts = orc_.render(key, cams[f], k, W, H, D)
        got = host[f * stride:(f + 1) * stride].tobytes()
        assert got == want, f"{key} {W}x{H} d{D} frame {f}: {diff_summary(got, want)}"
        for q in total:
            total[q] += counts[q]
    assert (st.rays_primary, st.rays_shadow, st.rays_reflect) == (total["primary"], total["shadow"], total["reflect"])
    return host[:stride].tobytes()


def _blocks(tiles, W, H):
    """The 8x8 blocks (PPM row order, as the RGB8 framebuffer) overlapping the tiles."""
    blocks = np.zeros((H, W), bool)
    for x, y, w, h in tiles:
        x1, j1 = min(W, x + w), min(H, y + h)
        p0, p1 = H - j1, H - 1 - y  # framebuffer rows j (0 = bottom) are PPM rows H-1-j
        for by in range(p0 // 8, p1 // 8 + 1):
            for bx in range(x // 8, (x1 - 1) // 8 + 1):
                blocks[by * 8:min(H, by * 8 + 8), bx * 8:min(W, bx * 8 + 8)] = True
    return blocks


def test_buffers_through_allocation_growth_and_scene_change():
    import orc  # noqa: F401  (the oracle library must be there before any GPU work)
    import rt_hip
    import synth
    import torch

    simple = rt_hip.Scene.load(scene_path("simple"))
    cloud_text = synth.generate("synth10k", n=1100)
    cloud = rt_hip.Scene.parse(cloud_text)
    o = _Oracle()
    o.add("simple", path=scene_path("simple"))
    o.add("cloud", text=cloud_text)
    cam = simple.camera()
    reflective = any(simple.sphere(i)["reflectivity"] > 0 for i in range(simple.num_spheres))

    r = rt_hip.Renderer(0)
    scratch = [0]

    def grown():
        scratch.append(r.info().scratch_bytes)
        assert scratch[-1] >= scratch[-2], scratch  # step 10

    try:
        # 1
        r.upload(simple)
        first = _launch(r, o, "simple", cam, [0], 64, 48, 3)
        assert r.info().sphere_grids == 0 and r.info().cam_grid_last == 0
        grown()
        # 2
        _launch(r, o, "simple", cam, [0, 1, 2], 64, 48, 3)
        inf = r.info()
        assert (inf.cam_grid_last, inf.cam_grid_n) == (1, 128)
        assert (inf.sphere_grids > 0) == reflective
        grown()
        # 3
        _launch(r, o, "simple", cam, [0, 0], 96, 64, 6)
        inf = r.info()
        assert (inf.cam_grid_last, inf.cam_grid_n) == (1, 256)
        grown()
        # 4
        builds = r.info().tile_order_builds
        _launch(r, o, "simple", cam, [0], 256, 256, 3)
        _launch(r, o, "simple", cam, [0], 320, 256, 3)
        assert r.info().tile_order_builds == builds + 2
        grown()
        # 5
        r.upload(cloud)
        _launch(r, o, "cloud", cloud.camera(), [0, 0], 64, 48, 3)
        assert r.info().behind_grid == 1
        grown()
        # 6
        r.upload(simple)
        assert r.info().behind_grid == 0
        assert _launch(r, o, "simple", cam, [0], 64, 48, 3) == first
        grown()
        # 7
        for W, H in ((32, 32), (128, 96)):
            rgb, st = r.render(cam, W, H, 3)
            want, counts = o.render("simple", cam, 0, W, H, 3)
            assert bytes(rgb) == want, diff_summary(bytes(rgb), want)
            assert (st.rays_primary, st.rays_shadow, st.rays_reflect) == (counts["primary"], counts["shadow"],
                                                                           counts["reflect"])
        grown()
        # 8
        W, H = 128, 96
        want, _ = o.render("simple", cam, 0, W, H, 3)
        want = np.frombuffer(want, np.uint8).reshape(H, W, 3)
        lists = ([(0, 0, 16, 16), (120, 90, 100, 100)],  # 4 + 1 blocks, the second overhanging
                 [(3, 5, 13, 7), (40, 13, 17, 9), (77, 2, 5, 30), (10, 60, 50, 3), (120, 90, 20, 20)])
        assert _blocks(lists[1], W, H).sum() > _blocks(lists[0], W, H).sum()  # the second list grows the buffers
        for tiles in lists:
            fb = torch.full((H * W * 3,), 7, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()  # the fill (torch's stream) lands before the launch
            r.render_tiles(cam, W, H, 3, tiles, rt_hip.RT_FB_RGB8, fb.data_ptr())
            st = r.stats()
            got = fb.cpu().numpy().reshape(H, W, 3)
            blocks = _blocks(tiles, W, H)
            assert (got[blocks] == want[blocks]).all()
            assert (got[~blocks] == 7).all()
            assert st.rays_primary == int(blocks.sum())
        grown()
        # 9
        r.set_antialias(4)
        try:
            fb = torch.zeros(32 * 32 * 3, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            r.render_tile(cam, 32, 32, 3, 0, 0, 32, 32, rt_hip.RT_FB_RGB8, fb.data_ptr())
            st = r.stats()
            want_aa, counts, _ = o.scenes["simple"].render_aa(32, 32, 3, samples=4, threads=4)
            got = fb.cpu().numpy().tobytes()
            assert got == want_aa, diff_summary(got, want_aa)
            assert (st.rays_primary, st.rays_shadow, st.rays_reflect) == (counts["primary"], counts["shadow"],
                                                                           counts["reflect"])
        finally:
            r.set_antialias(1)
        grown()
        # 11
        buf = _launch(r, o, "simple", cam, [0, 1, 2], 64, 48, 3, wait=False)
        r.close()
        del buf
        r = rt_hip.Renderer(0)
        r.upload(simple)
        assert _launch(r, o, "simple", cam, [0], 64, 48, 3) == first
    finally:
        r.close()
