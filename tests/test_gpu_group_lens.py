"""GPU: rt_group_render_lens_samples (include/rt_hip.h, rt_hip.Group.render_lens_samples, ray_hip
--aperture / --focus) on one GPU: every member lives on device 0, which runs the code a list of distinct
devices runs.  Bar: the assembled frame is byte for byte rt_render_lens_samples' on one context and the
summed counts are the full frame's.

Shapes as test_gpu_group_samples.py: 97x61 has odd row bytes in RGB8 and 16-byte multiples in F64X3;
37x21 has 4-byte-copy rows in F32X3; at 2x2 and G = 3 two members have no real row."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, golden_rgb, manifest, scene_path
from test_gpu_group_samples import AA, F32X3, F64X3, RECORD, RGB8, _aa_bytes, _group, _scene, _weights, counts
from test_gpu_samples import same_bits

pytestmark = pytest.mark.gpu

INVALID, NO_SCENE, DEPTH = 1, 5, 7  # rt_status
FOCUS, APERTURE = 7.25, 0.3


def _pattern(S):
    """(offsets, lens points): the first S of the 3 x 3 grid and of its lens pattern."""
    import rt_hip

    return rt_hip.grid_pattern(3)[:S], rt_hip.lens_pattern(3, APERTURE)[:S]


@functools.lru_cache(maxsize=None)
def _one_context(scene, W, H, D, S, weighted, fmt):
    """rt_render_lens_samples of the full frame on one context, once: (records, counts)."""
    import rt_hip

    r = rt_hip.Renderer(0)
    try:
        r.upload(_scene(scene))
        rec, st = r.render_lens_samples(_scene(scene).camera(), W, H, D, *_pattern(S), FOCUS,
                                        _weights(S) if weighted else None, None, fmt)
    finally:
        r.close()
    rec.setflags(write=False)
    return rec, counts(st)


def _same(got, want, fmt):
    return np.array_equal(got, want) if fmt == RGB8 else bool(same_bits(got, want).all())


def _check(g, scene, W, H, D, S, weighted, fmt):
    want, cnt = _one_context(scene, W, H, D, S, weighted, fmt)
    got, st = g.render_lens_samples(_scene(scene).camera(), W, H, D, *_pattern(S), FOCUS,
                                    _weights(S) if weighted else None, fmt)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert _same(got, want, fmt), (scene, W, H, g.size, fmt)
    assert counts(st) == cnt and st.rays == S * W * H and st.kernel_ms > 0
    return got


# ---- 1. the group is the one context ---------------------------------------------------------------------
@pytest.mark.parametrize("band", [1, 8])
@pytest.mark.parametrize("G", [1, 2, 3, 5])
def test_group_matches_one_context(G, band):
    import torch

    m = manifest()[AA]
    W, H, D = m["width"], m["height"], m["depth"]
    g = _group(G, band, m["scene"])
    try:
        for fmt in (RGB8, F32X3, F64X3):
            got = _check(g, m["scene"], W, H, D, 9, fmt == F32X3, fmt)
            nbytes, guard = W * H * RECORD[fmt][1], 4096
            dev = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
            assert dev.data_ptr() % 16 == 0
            torch.cuda.synchronize()  # the fill has landed before the group's streams start
            out, st = g.render_lens_samples(_scene(m["scene"]).camera(), W, H, D, *_pattern(9), FOCUS,
                                            _weights(9) if fmt == F32X3 else None, fmt, out=dev, out_on_device=True)
            assert out is dev and counts(st) == _one_context(m["scene"], W, H, D, 9, fmt == F32X3, fmt)[1]
            host = dev.cpu().numpy()
            assert host[:nbytes].tobytes() == got.tobytes()
            assert (host[nbytes:] == 0xA5).all(), "bytes behind the frame were written"
        _check(g, m["scene"], 37, 21, 4, 5, True, F32X3)  # 444-byte rows: the placement's 4-byte copies
    finally:
        g.close()


def test_members_without_rows():
    """H < band: members 1 and 2 of three launch nothing, and what they report is the larger render made
    first -- which must not be added."""
    g = _group(3, 8, "simple")
    try:
        _check(g, "simple", 40, 30, 3, 4, False, RGB8)
        _check(g, "simple", 2, 2, 10, 4, False, RGB8)
        _check(g, "simple", 2, 2, 10, 4, True, F64X3)
    finally:
        g.close()


# ---- 2. interleaving --------------------------------------------------------------------------------------
def test_the_four_group_calls_in_turn():
    """The four group render calls share the buffers and events of slot 0 (hazard (e) of rt_group.hip):
    each in turn, twice round, the lens call before and after each of the others."""
    import rt_hip

    m = manifest()[AA]
    W, H, D = m["width"], m["height"], m["depth"]
    cam = _scene("complex").camera()
    g = _group(3, 8, "complex")
    try:
        for _ in range(2):
            _check(g, "complex", W, H, D, 9, False, F64X3)
            rgb, _ = g.render(cam, W, H, D)
            assert bytes(rgb) == golden_rgb(AA)
            _check(g, "complex", W, H, D, 9, False, RGB8)
            aa, _ = g.render_samples(cam, W, H, D, rt_hip.grid_pattern(2))
            assert aa.tobytes() == _aa_bytes(AA)
            _check(g, "complex", W, H, D, 5, True, F32X3)
            frames, _ = g.render_frames([cam] * 3, W, H, D, batch=1)
            assert all(bytes(frames[f * W * H * 3:(f + 1) * W * H * 3]) == golden_rgb(AA) for f in range(3))
    finally:
        g.close()


# ---- 3. errors ---------------------------------------------------------------------------------------------
def test_errors_leave_the_group_usable():
    import ctypes as C

    import rt_hip
    import torch

    cam = _scene("complex").camera()
    g = _group(3)
    try:
        def status(offsets, lens, **kw):
            with pytest.raises(rt_hip.RtError) as e:
                g.render_lens_samples(cam, 16, 12, 3, offsets, lens, FOCUS, **kw)
            assert "rt_group_render_lens_samples" in g._L.rt_group_last_error(g._grp).decode()
            return e.value.status

        assert status(*_pattern(4)) == NO_SCENE
        g.upload(_scene("complex"))
        assert status([], []) == INVALID                                       # no samples
        assert status([(0.0, 0.0)] * 65, [(0.0, 0.0)] * 65) == INVALID         # too many
        assert status(*_pattern(4), fmt=3) == INVALID
        dev = torch.zeros((16 * 12 * 3 + 32,), dtype=torch.uint8, device="cuda:0")
        assert status(*_pattern(4), out=dev.data_ptr() + 8, out_on_device=True) == INVALID
        off = (C.c_double * 8)()
        st = rt_hip.rt_radiance_stats()
        assert g._L.rt_group_render_lens_samples(g._grp, C.byref(cam), 16, 12, 3, off, None, FOCUS, 4, None, RGB8,
                                                 C.c_void_p(dev.data_ptr()), 1, C.byref(st)) == INVALID  # NULL lens_xy
        with pytest.raises(rt_hip.RtError) as e:
            g.render_lens_samples(cam, 16, 12, rt_hip.RT_MAX_DEPTH + 1, *_pattern(4), FOCUS)
        assert e.value.status == DEPTH and "member 0" in str(e.value)  # a member call's error, through member_fail
        assert "rt_render_lens_samples_async" in str(e.value)
        with pytest.raises(rt_hip.RtError) as e:
            g.render_lens_samples(cam, 16, 12, 0, *_pattern(4), FOCUS)
        assert e.value.status == INVALID and "member 0" in str(e.value)
        m = manifest()[AA]
        _check(g, m["scene"], m["width"], m["height"], m["depth"], 9, False, RGB8)
    finally:
        g.close()


def test_checked_build():
    m = manifest()[AA]
    g = _group(3, 8, m["scene"], variant="check")
    try:
        _check(g, m["scene"], m["width"], m["height"], m["depth"], 9, False, RGB8)
        for i in range(3):
            g.member_stats(i)  # raises on RT_ERR_CHECK
    finally:
        g.close()


# ---- 4. the CLI --------------------------------------------------------------------------------------------
def _ray_hip(cwd, *args):
    return subprocess.run([os.path.join(PKG, "ray_hip"), *args], cwd=cwd, capture_output=True, text=True, timeout=300)


def test_cli_aperture_and_focus(tmp_path):
    import rt_hip

    W, H, D = 97, 61, 4
    size = ("--width", str(W), "--height", str(H), "--depth", str(D))
    scene = scene_path("complex")
    sc = _scene("complex")
    r = rt_hip.Renderer(0)
    try:
        r.upload(sc)
        lens, _ = r.render_lens_samples(sc.camera(), W, H, D, rt_hip.grid_pattern(3), rt_hip.lens_pattern(3, 0.2), FOCUS)
        pin, _ = r.render_samples(sc.camera(), W, H, D, rt_hip.grid_pattern(3))
    finally:
        r.close()
    rt_hip.write_ppm(str(tmp_path / "want.ppm"), lens, W, H)
    rt_hip.write_ppm(str(tmp_path / "pin.ppm"), pin, W, H)
    want = open(tmp_path / "want.ppm", "rb").read()
    assert want.startswith(b"P3\n") and lens.tobytes() != pin.tobytes()
    lens_flags = ("--supersample", "3", "--aperture", "0.2", "--focus", str(FOCUS))
    for flags, out in ((lens_flags, "one.ppm"), (lens_flags + ("--sample-devices", "0,0"), "grp.ppm"),
                       (("--supersample", "3"), "none.ppm"), (("--supersample", "3", "--aperture", "0.2"), "auto.ppm")):
        p = _ray_hip(tmp_path, *flags, *size, "--out", out, scene)
        assert p.returncode == 0 and "GPU rendering time:" in p.stdout, p.stdout + p.stderr
    assert open(tmp_path / "one.ppm", "rb").read() == want
    assert open(tmp_path / "grp.ppm", "rb").read() == want
    assert open(tmp_path / "none.ppm", "rb").read() == open(tmp_path / "pin.ppm", "rb").read()  # nothing changes
    auto = open(tmp_path / "auto.ppm", "rb").read()  # the focus: the camera's distance to its look-at point
    assert auto != open(tmp_path / "pin.ppm", "rb").read() and auto != want


def test_cli_usage_errors(tmp_path):
    scene = scene_path("simple")
    for flags in (("--aperture", "0.2"),                                     # only with --supersample
                  ("--focus", "5"),
                  ("--supersample", "2", "--focus", "5"),                    # --focus needs --aperture
                  ("--supersample", "2", "--aperture", "-0.1"),              # R >= 0
                  ("--supersample", "2", "--aperture", "nan"),
                  ("--supersample", "2", "--aperture", "x"),
                  ("--supersample", "2", "--aperture", "0.2", "--focus", "1x"),
                  ("--supersample", "2", "--aperture"),
                  ("-a", "--aperture", "0.2")):
        p = _ray_hip(tmp_path, *flags, "--width", "8", "--height", "8", scene)
        assert p.returncode == 2 and p.stderr.startswith("usage:"), flags
    assert not any(tmp_path.iterdir())  # nothing was rendered
