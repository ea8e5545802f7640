"""CPU-only: the multi-sample entries' host side (rt_camera_sample_rays,
rt_trace_radiance_resolve[_async], rt_render_samples) and their fp64 checker,
tests/sample_ref.py: the exported symbols, the argument errors that return
before any HIP call, and the checker chain camera_sample_rays -> trace_paths ->
shade -> resolve pinned to the oracle's four-sample antialias framebuffer."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import material_cases as mc
import path_ref
import ray_ref
import rt_hip
import sample_ref
from test_radiance_host import F64_KEPT, same_values

# The F64_KEPT cases the chain reproduces with the antialias pattern's rays (the sample rays are not the
# one-sample rays those cases were chosen for); a case that did not would be named here with the reason.
AA_LEFT_OUT = ()
AA_KEPT = tuple(c for c in F64_KEPT if c not in AA_LEFT_OUT)
assert len(AA_KEPT) >= 4 and set(AA_LEFT_OUT) <= set(F64_KEPT)

NEW_SYMBOLS = ("rt_camera_sample_rays", "rt_trace_radiance_resolve", "rt_trace_radiance_resolve_async",
               "rt_render_samples")


def test_symbols_and_methods():
    assert rt_hip.lib().rt_abi_version() == 12  # new symbols only
    out = subprocess.check_output(["nm", "-D", "--defined-only", rt_hip.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported and name in rt_hip.SIGNATURES, name
    for name in ("camera_sample_rays", "trace_radiance_resolve", "trace_radiance_resolve_device", "render_samples"):
        assert callable(getattr(rt_hip.Renderer, name)), name


def test_grid_pattern():
    assert rt_hip.grid_pattern(1) == [(0.0, 0.0)]
    assert tuple(rt_hip.grid_pattern(2)) == sample_ref.AA_PATTERN  # main_gpu.cu:253-256, a fastest
    g3 = rt_hip.grid_pattern(3)
    assert len(g3) == 9 and g3[1] == (1 / 3, 0.0) and g3[3] == (0.0, 1 / 3) and g3[8] == (2 / 3, 2 / 3)
    assert len(rt_hip.grid_pattern(8)) == 64  # RT_MAX_SAMPLES
    with pytest.raises(ValueError):
        rt_hip.grid_pattern(0)


def test_argument_errors_need_no_gpu():
    L = rt_hip.lib()
    INVALID = 1  # RT_ERR_INVALID_ARG
    rays = (rt_hip.rt_ray * 8)()
    out = (C.c_double * 6)()
    off = (C.c_double * 8)(0, 0, .5, 0, 0, .5, .5, .5)
    w = (C.c_double * 4)(.25, .25, .25, .25)
    cam = rt_hip.rt_camera()
    st = rt_hip.rt_radiance_stats()
    p = lambda x: C.cast(x, C.c_void_p)  # noqa: E731
    assert L.rt_camera_sample_rays(None, C.byref(cam), 2, 2, None, off, 4, p(rays)) == INVALID
    for fmt in (rt_hip.RT_FB_RGB8, rt_hip.RT_FB_F32X3, rt_hip.RT_FB_F64X3):
        for wt in (None, w):
            assert L.rt_trace_radiance_resolve(None, p(rays), 2, 4, wt, 4, fmt, p(out), 0, C.byref(st)) == INVALID
            assert L.rt_trace_radiance_resolve_async(None, p(rays), 2, 4, wt, 4, fmt, p(out)) == INVALID
            assert L.rt_render_samples(None, C.byref(cam), 1, 2, 4, None, off, 4, wt, fmt, p(out), 0, 0,
                                       C.byref(st)) == INVALID
    assert L.rt_trace_radiance_resolve(None, None, 0, 1, None, 1, rt_hip.RT_FB_F64X3, None, 0, None) == INVALID


def test_one_zero_offset_is_camera_rays():
    cam = rt_hip.Scene.parse(mc.text(AA_KEPT[0], "dense")).camera()
    for W, H, rows in ((97, 61, None), (1, 1, None), (2, 2, None), (5, 21, rt_hip.rows_for_shard(21, 8, 2, 3))):
        a = sample_ref.camera_sample_rays(cam, W, H, [(0.0, 0.0)], rows)
        b = ray_ref.camera_rays(cam, W, H, rows)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (W, H)


def test_sample_ray_layout():
    """Pixel-major, a pixel's samples consecutive; a shard's padding rows are zero rays."""
    cam = rt_hip.Scene.parse(mc.text(AA_KEPT[0], "dense")).camera()
    W, H = 7, 21
    rows = rt_hip.rows_for_shard(H, 8, 2, 3)  # rows 16..20 and three of padding
    rays = sample_ref.camera_sample_rays(cam, W, H, sample_ref.AA_PATTERN, rows).reshape(rows.count, W, 4, 8)
    one = ray_ref.camera_rays(cam, W, H, rows).reshape(rows.count, W, 8)
    assert np.array_equal(rays[:, :, 0, :].view(np.uint64), one.view(np.uint64))  # sample 0 is the pixel's corner
    assert (rays[5:] == 0).all() and np.isinf(rays[:5, :, :, 6]).all()
    assert not np.array_equal(rays[0, 0, 1], rays[0, 0, 2])


def test_resolve_rules():
    c = np.array([[[-0.0, 1.0, 0.5]]])
    assert np.array_equal(sample_ref.resolve(c).view(np.uint64), c[:, 0].view(np.uint64))  # -0.0 kept
    c2 = np.array([[[-0.0, 0.1, 0.5], [-0.0, 0.2, 0.25]]])
    box = sample_ref.resolve(c2)
    assert np.array_equal(box.view(np.uint64), (((0.0 + c2[:, 0]) + c2[:, 1]) * 0.5).view(np.uint64))
    assert not np.signbit(box[0, 0])  # 0 + -0.0 is +0.0
    w = np.array([0.3, -0.7])
    got = sample_ref.resolve(c2, w)
    assert np.array_equal(got.view(np.uint64), ((0.0 + c2[:, 0] * w[0]) + c2[:, 1] * w[1]).view(np.uint64))
    one = sample_ref.resolve(c, [1.0])
    assert not np.signbit(one[0, 0])  # weighted, S = 1: 0 + (-0.0 * 1.0)


@pytest.mark.parametrize("case", AA_KEPT)
def test_checker_chain_reproduces_the_oracle_antialias(case):
    """camera_sample_rays (the antialias pattern) -> trace_paths -> shade -> resolve equals the oracle's
    render_aa framebuffer as values, and its ray counts."""
    W, H, D = mc.F64_SHAPE
    sc = rt_hip.Scene.parse(mc.text(case, "dense"))
    sa = path_ref.SceneArrays(sc)
    rays = sample_ref.camera_sample_rays(sc.camera(), W, H, rt_hip.grid_pattern(2))
    levels = path_ref.trace_paths(rays[:, 0:3], rays[:, 3:6], D, sa)
    got = sample_ref.resolve(path_ref.shade(levels, sa).reshape(W * H, 4, 3))
    want_rgb, counts, fb = mc.oracle_aa(case, W, H, D)
    n, segments, _, shadow = path_ref.counts(levels, sa)
    assert (n, segments - n, shadow) == (counts["primary"], counts["reflect"], counts["shadow"])
    same = same_values(got, fb.reshape(-1, 3))
    assert same.all(), "%d of %d channels differ" % (int((~same).sum()), same.size)
    assert path_ref.quantize(got).tobytes() == want_rgb
