"""GPU: rt_group_render_samples (include/rt_hip.h, rt_hip.Group.render_samples, ray_hip
--sample-devices) on one GPU: every member lives on device 0, which runs the code a list of distinct
devices runs.  Bar: the assembled frame is byte for byte rt_render_samples' on one context -- for the
antialias pattern the committed antialias bytes of the oracle's render_aa -- and the summed counts are
the full frame's.

Shapes: 97x61 has odd row bytes in RGB8 (291: the placement's byte path) and 16-byte multiples in
F64X3; 37x21 has 111-byte RGB8 rows and 444-byte F32X3 rows (4-byte copies); 1x1 and 2x2 have
H < band, so at G = 3 two members have no real row."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, diff_summary, golden_rgb, manifest, scene_path
from test_gpu_samples import same_bits

pytestmark = pytest.mark.gpu

RGB8, F32X3, F64X3 = 0, 1, 2  # RT_FB_*
RECORD = {RGB8: (np.uint8, 3), F32X3: (np.float32, 12), F64X3: (np.float64, 24)}
INVALID, NO_SCENE, DEPTH = 1, 5, 7  # rt_status
COUNTS = ("rays", "segments", "hits", "shadow_rays", "unaccelerated", "negative_clamped")
AA = "complex_97x61_d4"


def counts(st):
    return {k: getattr(st, k) for k in COUNTS}


@functools.lru_cache(maxsize=None)
def _scene(name):
    import rt_hip

    return rt_hip.Scene.load(scene_path(name))


@functools.lru_cache(maxsize=None)
def _aa_bytes(name):
    """The antialias frame of a golden fixture's shape from the oracle's render_aa, once."""
    import orc

    m = manifest()[name]
    rgb, _, _ = orc.OracleScene(scene_path(m["scene"])).render_aa(m["width"], m["height"], m["depth"], samples=4,
                                                                 threads=4)
    return rgb


@functools.lru_cache(maxsize=None)
def _one_context(scene, W, H, D, S, weighted, fmt):
    """rt_render_samples of the full frame on one context, once: (records, counts)."""
    import rt_hip

    r = rt_hip.Renderer(0)
    try:
        r.upload(_scene(scene))
        rec, st = r.render_samples(_scene(scene).camera(), W, H, D, _pattern(S), _weights(S) if weighted else None,
                                   None, fmt)
    finally:
        r.close()
    rec.setflags(write=False)
    return rec, counts(st)


def _pattern(S):
    """S = 4: the antialias pattern; otherwise the first S offsets of the 3 x 3 grid."""
    import rt_hip

    return rt_hip.grid_pattern(2) if S == 4 else rt_hip.grid_pattern(3)[:S]


def _weights(S):
    w = np.random.default_rng(40 + S).uniform(0.0, 1.0, S) / S
    w[S // 2] = -1.5  # some pixel sums are below zero
    return [float(x) for x in w]


def _group(G, band=8, scene=None, variant=None):
    import rt_hip

    g = rt_hip.Group([0] * G, band=band, variant=variant)
    assert g.size == G
    if scene is not None:
        g.upload(_scene(scene))
    return g


def _check_aa(g, name):
    m = manifest()[name]
    W, H, D = m["width"], m["height"], m["depth"]
    rgb, st = g.render_samples(_scene(m["scene"]).camera(), W, H, D, _pattern(4))
    assert rgb.shape == (W * H, 3) and rgb.dtype == np.uint8
    want = _aa_bytes(name)
    assert rgb.tobytes() == want, f"{name} G={g.size}: {diff_summary(rgb.tobytes(), want)}"
    assert counts(st) == _one_context(m["scene"], W, H, D, 4, False, RGB8)[1]
    assert st.rays == 4 * W * H and st.kernel_ms > 0


# ---- 1. golden shapes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", [1, 8])
@pytest.mark.parametrize("G", [1, 2, 3, 5])
def test_group_matches_the_antialias_frame(G, band):
    g = _group(G, band, manifest()[AA]["scene"])
    try:
        _check_aa(g, AA)
    finally:
        g.close()


# ---- 2. members without rows -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["simple_2x2_d10", "simple_1x1_d10"])
def test_members_without_rows(name):
    """H < band: members 1 and 2 of three launch nothing, and what they report is the larger render made
    first -- which must not be added."""
    g = _group(3, 8, "simple")
    try:
        _, st = g.render_samples(_scene("simple").camera(), 40, 30, 3, _pattern(4))
        assert st.rays == 4 * 40 * 30
        _check_aa(g, name)
    finally:
        g.close()


# ---- 3. formats and device output ------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [RGB8, F32X3, F64X3])
def test_formats_on_the_host_and_on_the_device(fmt):
    import torch

    W, H, D, S = 37, 21, 4, 5
    want, cnt = _one_context("complex", W, H, D, S, True, fmt)
    cam = _scene("complex").camera()
    g = _group(3, 8, "complex")
    try:
        got, st = g.render_samples(cam, W, H, D, _pattern(S), _weights(S), fmt)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got, want) if fmt == RGB8 else same_bits(got, want).all()
        assert counts(st) == cnt
        nbytes, guard = W * H * RECORD[fmt][1], 4096
        dev = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
        assert dev.data_ptr() % 16 == 0
        torch.cuda.synchronize()  # the fill has landed before the group's streams start
        out, st = g.render_samples(cam, W, H, D, _pattern(S), _weights(S), fmt, out=dev, out_on_device=True)
        assert out is dev and counts(st) == cnt
        host = dev.cpu().numpy()
        assert host[:nbytes].tobytes() == got.tobytes()
        assert (host[nbytes:] == 0xA5).all(), "bytes behind the frame were written"
    finally:
        g.close()


# ---- 4. interleaving --------------------------------------------------------------------------------------
def test_the_three_group_calls_in_turn():
    """rt_group_render, rt_group_render_samples and rt_group_render_frames share the buffers and events
    of slot 0 (hazard (e) of rt_group.hip): each in turn, twice round, with record sizes 3 and 24."""
    m = manifest()[AA]
    W, H, D = m["width"], m["height"], m["depth"]
    cam = _scene("complex").camera()
    want64, cnt64 = _one_context("complex", W, H, D, 4, False, F64X3)
    g = _group(3, 8, "complex")
    try:
        for _ in range(2):
            rgb, _ = g.render(cam, W, H, D)
            assert bytes(rgb) == golden_rgb(AA)
            _check_aa(g, AA)
            frames, _ = g.render_frames([cam] * 3, W, H, D, batch=1)
            assert all(bytes(frames[f * W * H * 3:(f + 1) * W * H * 3]) == golden_rgb(AA) for f in range(3))
            f64, st = g.render_samples(cam, W, H, D, _pattern(4), fmt=F64X3)
            assert same_bits(f64, want64).all() and counts(st) == cnt64
    finally:
        g.close()


# ---- 5. errors ---------------------------------------------------------------------------------------------
def test_errors_leave_the_group_usable():
    import rt_hip
    import torch

    cam = _scene("complex").camera()
    g = _group(3)
    try:
        def status(*a, **kw):
            with pytest.raises(rt_hip.RtError) as e:
                g.render_samples(cam, 16, 12, 3, *a, **kw)
            assert "rt_group_render_samples" in g._L.rt_group_last_error(g._grp).decode()
            return e.value.status

        assert status(_pattern(4)) == NO_SCENE
        g.upload(_scene("complex"))
        assert status([]) == INVALID                               # no samples
        assert status([(0.0, 0.0)] * 65) == INVALID                # too many
        assert status(_pattern(4), fmt=3) == INVALID
        dev = torch.zeros((16 * 12 * 3 + 32,), dtype=torch.uint8, device="cuda:0")
        assert status(_pattern(4), out=dev.data_ptr() + 8, out_on_device=True) == INVALID
        with pytest.raises(rt_hip.RtError) as e:
            g.render_samples(cam, 16, 12, rt_hip.RT_MAX_DEPTH + 1, _pattern(4))
        assert e.value.status == DEPTH and "member 0" in str(e.value)  # a member call's error, through member_fail
        with pytest.raises(rt_hip.RtError) as e:
            g.render_samples(cam, 16, 12, 0, _pattern(4))
        assert e.value.status == INVALID and "member 0" in str(e.value)
        _check_aa(g, AA)
    finally:
        g.close()


def test_checked_build():
    g = _group(3, 8, manifest()[AA]["scene"], variant="check")
    try:
        _check_aa(g, AA)
        for i in range(3):
            g.member_stats(i)  # raises on RT_ERR_CHECK
    finally:
        g.close()


# ---- 6. the CLI --------------------------------------------------------------------------------------------
def test_cli_sample_devices(tmp_path):
    def ray_hip(*args):
        return subprocess.run([os.path.join(PKG, "ray_hip"), *args], cwd=tmp_path, capture_output=True, text=True,
                              timeout=300)

    size = ("--width", "97", "--height", "61", "--depth", "4")
    scene = scene_path("complex")
    for flags, out in ((("-a",), "aa.ppm"), (("--supersample", "2", "--sample-devices", "0,0,0"), "grp.ppm")):
        p = ray_hip(*flags, *size, "--out", out, scene)
        assert p.returncode == 0 and "GPU rendering time:" in p.stdout, p.stdout + p.stderr
    aa = open(tmp_path / "aa.ppm", "rb").read()
    assert aa.startswith(b"P3\n") and open(tmp_path / "grp.ppm", "rb").read() == aa
