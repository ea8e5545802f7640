"""No launch inherits anything from the call before it: one `Renderer` of the
product library goes through every render entry point in turn, with refused
calls in between, and every result is compared with the oracle (orc.py) as
tests/test_gpu_lifecycle.py does.  simple.txt at 64x48, depth 3.  In order:

 1. three frames from three camera positions in one launch.
 2. three refused render_frames_async calls: 33 cameras, two cameras with a
    stride one byte short, depth RT_MAX_DEPTH + 1.
 3. render_async of one frame into a buffer pre-filled with 77: the whole
    image, and one frame's ray counts.
 4. render_tiles with two unaligned tiles into a framebuffer pre-filled with
    7: the covering 8x8 blocks and nothing else.
 5. a refused render_tiles call (a tile at x = -1).
 6. render_async again: the whole image, not only step 4's blocks.
 7. render_tile of a 16x16 tile into an RT_FB_F64X3 framebuffer pre-filled
    with a sentinel: the tile within 64 ulp of the oracle's fp64 framebuffer
    (the bar of tests/test_gpu_tile_aa.py), the sentinel everywhere else.
 8. step 1's launch again: step 1's bytes and counts.
"""
import numpy as np
import pytest

from conftest import diff_summary, scene_path
from test_gpu_lifecycle import _blocks, _moved
from test_gpu_tile_aa import MAX_ULP, ulp_diff

pytestmark = pytest.mark.gpu

W, H, D = 64, 48, 3
STRIDE = H * W * 3
KEYS = ("primary", "shadow", "reflect")


def _counts(st):
    return st.rays_primary, st.rays_shadow, st.rays_reflect


def test_no_launch_inherits_from_the_call_before():
    import orc
    import rt_hip
    import torch

    simple = rt_hip.Scene.load(scene_path("simple"))
    oracle = orc.OracleScene(path=scene_path("simple"))
    cam = simple.camera()
    cams = [_moved(cam, k) for k in range(3)]
    want, want_counts = [], []
    for cm in cams:
        rgb, counts, _ = oracle.render(W, H, D, threads=4, camera=cm)
        want.append(rgb)
        want_counts.append(tuple(counts[q] for q in KEYS))
    summed = tuple(sum(c[i] for c in want_counts) for i in range(3))
    _, _, _, ref_fb = oracle.render(W, H, D, threads=4, want_fb=True, camera=cam)
    # oracle fb is in PPM row order; the tile framebuffer is indexed j*W + x with j = 0 the bottom row
    ref_fb = np.array(ref_fb, dtype=np.float64).reshape(H, W, 3)[::-1]
    want0 = np.frombuffer(want[0], np.uint8).reshape(H, W, 3)

    def filled(n, value, dtype=torch.uint8):
        buf = torch.full((n,), value, dtype=dtype, device="cuda:0")
        torch.cuda.synchronize()  # the fill (torch's stream) lands before the render
        return buf

    def three_frames():
        buf = filled(3 * STRIDE, 77)
        r.render_frames_async(cams, W, H, D, None, buf.data_ptr(), STRIDE)
        st = r.stats()
        host = buf.cpu().numpy()
        for f in range(3):
            got = host[f * STRIDE:(f + 1) * STRIDE].tobytes()
            assert got == want[f], f"frame {f}: {diff_summary(got, want[f])}"
        assert _counts(st) == summed
        return host.tobytes()

    def one_frame():
        buf = filled(STRIDE, 77)
        r.render_async(cam, W, H, D, None, buf.data_ptr())
        st = r.stats()
        got = buf.cpu().numpy().tobytes()
        assert got == want[0], diff_summary(got, want[0])
        assert _counts(st) == want_counts[0]

    r = rt_hip.Renderer(0)
    try:
        r.upload(simple)
        # 1
        first = three_frames()
        # 2
        buf = filled(33 * STRIDE, 77)
        with pytest.raises(rt_hip.RtError):
            r.render_frames_async([cam] * 33, W, H, D, None, buf.data_ptr(), STRIDE)
        with pytest.raises(rt_hip.RtError):
            r.render_frames_async(cams[:2], W, H, D, None, buf.data_ptr(), STRIDE - 1)
        with pytest.raises(rt_hip.RtError):
            r.render_frames_async(cams[:2], W, H, rt_hip.RT_MAX_DEPTH + 1, None, buf.data_ptr(), STRIDE)
        # 3
        one_frame()
        # 4
        tiles = [(3, 5, 13, 7), (41, 30, 17, 30)]  # unaligned; the second overhangs the top edge
        fb = filled(STRIDE, 7)
        r.render_tiles(cam, W, H, D, tiles, rt_hip.RT_FB_RGB8, fb.data_ptr())
        st = r.stats()
        got = fb.cpu().numpy().reshape(H, W, 3)
        blocks = _blocks(tiles, W, H)
        assert 0 < blocks.sum() < W * H
        assert (got[blocks] == want0[blocks]).all()
        assert (got[~blocks] == 7).all()
        assert st.rays_primary == int(blocks.sum())
        # 5
        with pytest.raises(rt_hip.RtError):
            r.render_tiles(cam, W, H, D, [(-1, 0, 8, 8)], rt_hip.RT_FB_RGB8, fb.data_ptr())
        # 6
        one_frame()
        # 7
        sentinel = -12345.0
        tx, ty, tw, th = 20, 10, 16, 16
        fb64 = filled(STRIDE, sentinel, torch.float64)
        r.render_tile(cam, W, H, D, tx, ty, tw, th, rt_hip.RT_FB_F64X3, fb64.data_ptr())
        r.stats()
        got = fb64.cpu().numpy().reshape(H, W, 3)
        inside = np.zeros((H, W), bool)
        inside[ty:ty + th, tx:tx + tw] = True
        d = ulp_diff(got[inside], ref_fb[inside])
        assert d.max() <= MAX_ULP, (int(d.max()), int((d > 0).sum()))
        assert (got[~inside] == sentinel).all()
        # 8
        assert three_frames() == first
    finally:
        r.close()
