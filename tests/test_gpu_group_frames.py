"""Frame sequences on the device group (rt_group_render_frames,
rt_hip.Group.render_frames, ray_hip --devices --frames) on one GPU: every member
lives on device 0, as in tests/test_gpu_group.py.  Bar: every frame of a
sequence is byte-identical to the golden / the CPU oracle / the group's own
one-frame render of its camera, the ray counts are the sums over the frames,
and no byte between or around the frames is written.

Shapes: 97x61 has 291-byte rows (the byte copies of the placement), 100x75
300-byte rows (4-byte copies), 64x48 192-byte rows (16-byte copies; an odd
frame stride or start moves frames off them).  Batches stay <= 4 frames: a
context's multi-frame scratch grows with the batch and up to 8 contexts share
the device."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, diff_summary, golden_rgb, manifest, scene_path

pytestmark = pytest.mark.gpu

SMALL = "complex_97x61_d4"
# (G, band, F, batch): batches 2,2,1 (both slots, slot 0 reused, a short tail); four members all
# padding; one member, one batch; batches 3,2,2; one frame at the default batch
GOLDEN_CASES = [(3, 8, 5, 2), (8, 16, 3, 1), (1, 8, 4, 4), (5, 1, 7, 3), (3, 8, 1, 0)]
ORACLE_CASES = [(64, 48, 3), (100, 75, 2)]  # complex at W x H, depth
STEPS = (0, 3, -2, 1, 5)  # the camera of frame f is _moved(cam, STEPS[f])


@functools.lru_cache(maxsize=None)
def _scene(name):
    import rt_hip

    return rt_hip.Scene.load(scene_path(name))


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


@functools.lru_cache(maxsize=None)
def _oracle(W, H, depth, k=0):
    """complex at W x H through the camera moved k steps, from the CPU oracle, once: (rgb, counts)."""
    import orc

    rgb, counts, _ = orc.OracleScene(scene_path("complex")).render(W, H, depth, threads=4,
                                                                   camera=_moved(_scene("complex").camera(), k))
    return rgb, {q: counts[q] for q in ("primary", "shadow", "reflect")}


def _group(G, band=8, scene=None, variant=None):
    import rt_hip

    g = rt_hip.Group([0] * G, band=band, variant=variant)
    assert g.size == G
    if scene is not None:
        g.upload(_scene(scene))
    return g


def _counts(st):
    return {"primary": st.rays_primary, "shadow": st.rays_shadow, "reflect": st.rays_reflect}


def _times(counts, F):
    return {q: F * v for q, v in counts.items()}


def _sequence_golden(g, name, F, batch):
    """F frames of the golden's static view: every frame the golden, F times its counts."""
    m = manifest()[name]
    n = m["width"] * m["height"] * 3
    cams = [_scene(m["scene"]).camera()] * F
    rgb, st = g.render_frames(cams, m["width"], m["height"], m["depth"], batch=batch)
    want = golden_rgb(name)
    assert len(rgb) == F * n
    for f in range(F):
        got = bytes(rgb[f * n:(f + 1) * n])
        assert got == want, f"{name} G={g.size} frame {f} of {F}, batch {batch}: {diff_summary(got, want)}"
    assert _counts(st) == _times(m["rays"], F)
    assert st.negative_clamped == 0
    assert st.kernel_ms > 0
    return st


def _single_golden(g, name):
    m = manifest()[name]
    rgb, st = g.render(_scene(m["scene"]).camera(), m["width"], m["height"], m["depth"])
    assert bytes(rgb) == golden_rgb(name), name
    assert _counts(st) == m["rays"]


@pytest.mark.parametrize("G,band,F,batch", GOLDEN_CASES, ids=[f"G{G}-b{b}-F{F}-batch{n}" for G, b, F, n in GOLDEN_CASES])
def test_sequence_matches_golden(G, band, F, batch):
    g = _group(G, band, "complex")
    try:
        _sequence_golden(g, SMALL, F, batch)
    finally:
        g.close()


@pytest.mark.parametrize("W,H,depth", ORACLE_CASES, ids=["64x48-16B", "100x75-4B"])
def test_distinct_cameras_match_oracle(W, H, depth):
    cam = _scene("complex").camera()
    n = W * H * 3
    g = _group(3, 8, "complex")
    try:
        rgb, st = g.render_frames([_moved(cam, k) for k in STEPS], W, H, depth, batch=2)
        total = {"primary": 0, "shadow": 0, "reflect": 0}
        for f, k in enumerate(STEPS):
            want, counts = _oracle(W, H, depth, k)
            got = bytes(rgb[f * n:(f + 1) * n])
            assert got == want, f"frame {f}: {diff_summary(got, want)}"
            for q in total:
                total[q] += counts[q]
        assert _counts(st) == total
        assert bytes(rgb[n:2 * n]) != bytes(rgb[:n])  # the frames are different views
    finally:
        g.close()


@pytest.mark.parametrize("samples,steps", [(1, STEPS), (4, STEPS[:2])], ids=["aa1", "aa4"])
def test_sequence_equals_single_renders(samples, steps):
    W, H, depth = 97, 61, 4
    n = W * H * 3
    cams = [_moved(_scene("complex").camera(), k) for k in steps]
    g = _group(3, 8, "complex")
    try:
        g.set_antialias(samples)
        singles = [g.render(c, W, H, depth) for c in cams]
        rgb, st = g.render_frames(cams, W, H, depth, batch=2)
        for f, (want, _) in enumerate(singles):
            got = bytes(rgb[f * n:(f + 1) * n])
            assert got == bytes(want), f"frame {f}: {diff_summary(got, bytes(want))}"
        for q in ("rays_primary", "rays_shadow", "rays_reflect"):
            assert getattr(st, q) == sum(getattr(s, q) for _, s in singles), q
        assert st.rays_primary == len(cams) * W * H * samples
    finally:
        g.close()


def _check_strided(buf, lead, stride, F, want):
    """buf (numpy uint8, 0xAA-filled before the call): frame f at lead + f * stride, nothing else written."""
    n = len(want)
    untouched = np.ones(buf.shape, bool)
    for f in range(F):
        a = lead + f * stride
        assert buf[a:a + n].tobytes() == want, f"frame {f}"
        untouched[a:a + n] = False
    assert int(untouched.sum()) == len(buf) - F * n
    assert (buf[untouched] == 0xAA).all(), "bytes between or around the frames were written"


@pytest.mark.parametrize("off", [0, 4, 1], ids=["dst16", "dst4", "dst1"])
def test_device_output_strided(off):
    """64x48 rows are 192 bytes and the stride is odd: the alignment of each frame's
    destination alone picks the 16-byte, 4-byte or byte copies, frame by frame."""
    import torch

    W, H, depth, F = 64, 48, 3, 3
    n = W * H * 3
    stride, lead = n + 13, 64 + off
    want, counts = _oracle(W, H, depth)
    g = _group(3, 8, "complex")
    try:
        buf = torch.full((lead + (F - 1) * stride + n + 64,), 0xAA, dtype=torch.uint8, device="cuda:0")
        assert buf.data_ptr() % 16 == 0
        torch.cuda.synchronize()  # the fill has landed before the group's streams start
        view = buf[lead:]
        out, st = g.render_frames([_scene("complex").camera()] * F, W, H, depth, batch=2, out=view,
                                  out_on_device=True, frame_stride=stride)
        assert out is view
        _check_strided(buf.cpu().numpy(), lead, stride, F, want)
        assert _counts(st) == _times(counts, F)
    finally:
        g.close()


def test_host_output_strided():
    W, H, depth, F = 64, 48, 3, 3
    n = W * H * 3
    stride = n + 5
    want, counts = _oracle(W, H, depth)
    g = _group(3, 8, "complex")
    try:
        out = bytearray(b"\xaa" * ((F - 1) * stride + n))
        got, st = g.render_frames([_scene("complex").camera()] * F, W, H, depth, batch=2, out=out, frame_stride=stride)
        assert got is out
        _check_strided(np.frombuffer(out, np.uint8), 0, stride, F, want)
        assert _counts(st) == _times(counts, F)
    finally:
        g.close()


def test_mixed_calls_and_regrow():
    """One group through single frames and sequences of growing and shrinking
    images: both calls share the group's buffers, which grow (97x61 -> 1080p)
    and are reused, and a new scene follows."""
    g = _group(3, 8, "complex")
    try:
        _single_golden(g, SMALL)
        _sequence_golden(g, SMALL, 5, 2)
        _sequence_golden(g, "complex_1920x1080_d4", 4, 2)
        _sequence_golden(g, SMALL, 5, 2)
        _single_golden(g, SMALL)
        g.upload(_scene("simple"))
        _sequence_golden(g, "simple_800x600_d10", 3, 2)
    finally:
        g.close()


def test_member_stats_after_a_sequence():
    """A borrowed member reports its launches of the call: rt_render_stats the last
    one (its shard of the last batch), rt_kernel_times one time per batch."""
    import ctypes as C

    m = manifest()[SMALL]
    W, H = m["width"], m["height"]
    g = _group(3, 8, "complex")
    try:
        L = g._L
        buf, n = (C.c_double * 16)(), C.c_int(0)
        for i in range(3):
            assert L.rt_kernel_times(g.member(i), buf, 16, C.byref(n)) == 0  # the history starts here
        st = _sequence_golden(g, SMALL, 5, 2)  # batches 2, 2, 1
        sums = []
        for i in range(3):
            rows = sum(1 for y in range(H) if (y // 8) % 3 == i)
            assert g.member_stats(i).rays_primary == 1 * W * rows  # the last batch has one frame
            assert L.rt_kernel_times(g.member(i), buf, 16, C.byref(n)) == 0
            assert n.value == 3
            sums.append(sum(buf[:3]))
        assert st.kernel_ms == pytest.approx(max(sums), rel=1e-6)  # float event times summed in double
    finally:
        g.close()


def test_long_sequence_of_one_frame_launches():
    """200 launches in one call: more than the 192 after which the call starts to
    collect its launches' times from the context's ring of 256 events while it
    still enqueues.  Every launch is counted once, in the counts and in kernel_ms."""
    import ctypes as C

    W, H, depth, F = 16, 16, 2, 200
    n = W * H * 3
    cam = _scene("complex").camera()
    g = _group(1, 8, "complex")
    try:
        want, one = g.render(cam, W, H, depth)
        buf, cnt = (C.c_double * 256)(), C.c_int(0)
        assert g._L.rt_kernel_times(g.member(0), buf, 256, C.byref(cnt)) == 0  # the history starts here
        rgb, st = g.render_frames([cam] * F, W, H, depth, batch=1)
        assert all(bytes(rgb[f * n:(f + 1) * n]) == bytes(want) for f in range(F))
        assert _counts(st) == _times(_counts(one), F)
        assert g._L.rt_kernel_times(g.member(0), buf, 256, C.byref(cnt)) == 0
        assert cnt.value == F
        assert st.kernel_ms == pytest.approx(sum(buf[:F]), rel=1e-6)  # the same float times, summed in double
    finally:
        g.close()


def test_errors_leave_the_group_usable():
    import rt_hip

    W, H = 16, 16
    n = W * H * 3
    cams = [_scene("complex").camera()] * 2
    g = _group(2, 8)
    try:
        with pytest.raises(rt_hip.RtError) as e:
            g.render_frames(cams, W, H, 2)
        assert e.value.status == 5  # RT_ERR_NO_SCENE
        g.upload(_scene("complex"))
        with pytest.raises(rt_hip.RtError) as e:
            g.render_frames(cams, W, H, rt_hip.RT_MAX_DEPTH + 1)
        assert e.value.status == 7  # RT_ERR_DEPTH
        out = bytearray(2 * n)
        with pytest.raises(rt_hip.RtError) as e:
            g.render_frames(cams, W, H, 2, out=out, frame_stride=n - 1)
        assert e.value.status == 1
        one, _ = g.render_frames(cams[:1], W, H, 2, out=bytearray(n), frame_stride=n - 1)  # one frame: no stride
        want, _ = g.render(cams[0], W, H, 2)
        assert bytes(one) == bytes(want)
        _sequence_golden(g, SMALL, 3, 2)
    finally:
        g.close()


def test_check_build():
    """The bounds-checked build: no device index of a sequence's launches is out of range."""
    g = _group(3, 8, "complex", variant="check")
    try:
        _sequence_golden(g, SMALL, 5, 2)
    finally:
        g.close()


def test_cli_frames(tmp_path):
    name = "complex_1920x1080_d4"
    r = subprocess.run([os.path.join(PKG, "ray_hip"), "--devices", "0,0,0", "--frames", "5", "--batch", "2",
                        "--width", "1920", "--height", "1080", "--depth", "4", "--p6", "--json",
                        scene_path("complex")], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    data = open(tmp_path / "output_gpu.ppm", "rb").read()
    head = b"P6\n1920 1080\n255\n"
    assert data.startswith(head) and data[len(head):] == golden_rgb(name)
    assert "GPU rendering time:" in r.stdout and "Frames: 5," in r.stdout
    rec = json.loads(next(line for line in r.stdout.splitlines() if line.startswith("{")))
    rays = manifest()[name]["rays"]
    assert rec["frames"] == 5 and rec["gpus"] == 3
    assert {q: rec[q] for q in ("primary", "shadow", "reflect")} == _times(rays, 5)
    assert rec["rays"] == 5 * sum(rays.values())
