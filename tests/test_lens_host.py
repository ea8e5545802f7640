"""No GPU: the thin-lens entries' symbols, signatures and argument errors (include/rt_hip.h,
"samples through a thin lens"), rt_hip.lens_pattern, and tests/lens_ref.py against sample_ref.py
(zero lens, focus 1.0) and against the geometry it states (the focal-plane property)."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import lens_ref
import material_cases as mc
import rt_hip
import sample_ref
from conftest import scene_path
from test_radiance_host import F64_KEPT, same_values

NEW_SYMBOLS = ("rt_camera_lens_rays", "rt_render_lens_samples_async", "rt_render_lens_samples",
               "rt_group_render_lens_samples")
INVALID = 1  # RT_ERR_INVALID_ARG


def test_symbols_and_methods():
    assert rt_hip.lib().rt_abi_version() == 12  # new symbols only
    out = subprocess.check_output(["nm", "-D", "--defined-only", rt_hip.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported and name in rt_hip.SIGNATURES, name
    for name in ("camera_lens_rays", "render_lens_samples", "render_lens_samples_async"):
        assert callable(getattr(rt_hip.Renderer, name)), name
    assert callable(rt_hip.Group.render_lens_samples) and callable(rt_hip.lens_pattern)


def test_argument_errors_need_no_gpu():
    """A NULL context or group, a NULL lens_xy, samples outside 1..64 and an unknown format are
    RT_ERR_INVALID_ARG; without a device no context exists, so each is tried with the NULL handle (the
    GPU tests repeat them on a live context and check that nothing was launched)."""
    L = rt_hip.lib()
    rays = (rt_hip.rt_ray * 8)()
    out = (C.c_double * 16)()
    off = (C.c_double * 8)(0, 0, .5, 0, 0, .5, .5, .5)
    lens = (C.c_double * 8)(.1, 0, 0, .1, -.1, 0, 0, -.1)
    w = (C.c_double * 4)(.25, .25, .25, .25)
    cam = rt_hip.rt_camera()
    st = rt_hip.rt_radiance_stats()
    p = lambda x: C.cast(x, C.c_void_p)  # noqa: E731
    for ln in (lens, None):
        for S in (4, 0, 65, -1):
            assert L.rt_camera_lens_rays(None, C.byref(cam), 2, 2, None, off, ln, 1.0, S, p(rays)) == INVALID
            for fmt in (rt_hip.RT_FB_RGB8, rt_hip.RT_FB_F32X3, rt_hip.RT_FB_F64X3, 3, -1):
                for wt in (None, w):
                    assert L.rt_render_lens_samples_async(None, C.byref(cam), 2, 2, 4, None, off, ln, 1.0, S, wt,
                                                          fmt, p(out)) == INVALID
                    assert L.rt_render_lens_samples(None, C.byref(cam), 2, 2, 4, None, off, ln, 1.0, S, wt, fmt,
                                                    p(out), 0, C.byref(st)) == INVALID
                    assert L.rt_group_render_lens_samples(None, C.byref(cam), 2, 2, 4, off, ln, 1.0, S, wt, fmt,
                                                          p(out), 0, C.byref(st)) == INVALID
    with pytest.raises(ValueError):  # the binding pairs offset s with lens point s
        rt_hip._lens_points([(0.0, 0.0)], 2)


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_lens_pattern(n):
    R = 0.375
    pts = rt_hip.lens_pattern(n, R)
    assert len(pts) == n * n == len(rt_hip.grid_pattern(n))
    assert all(math.hypot(x, y) <= R for x, y in pts)  # the square's corner (1, 1) maps to radius 1 exactly
    assert {(-x + 0.0, -y + 0.0) for x, y in pts} == {(x + 0.0, y + 0.0) for x, y in pts}  # (x,y) -> (-x,-y)
    assert all(x == 0.0 and y == 0.0 for x, y in rt_hip.lens_pattern(n, 0.0))
    if n > 1:
        assert len(set(pts)) == n * n
        # sample s takes cell n*n-1-s, a fastest: sample 0 the last cell (largest u and v)
        u = (n - 1 + 0.5) / n * 2.0 - 1.0
        assert pts[0] == (u * math.sqrt(1.0 - u * u / 2.0) * R,) * 2
        assert pts[0] == (-pts[-1][0], -pts[-1][1])
    else:
        assert pts == [(0.0, 0.0)]  # one cell: the centre of the lens
    with pytest.raises(ValueError):
        rt_hip.lens_pattern(0, 1.0)


def _cameras():
    cams = {"case:" + c: rt_hip.Scene.parse(mc.text(c, "dense")).camera() for c in F64_KEPT[:1]}
    for name in ("simple", "medium", "complex", "synth200"):
        cams[name] = rt_hip.Scene.load(scene_path(name)).camera()
    return cams


ZERO_SIZES = ((97, 61, None), (1, 1, None), (2, 2, None), (5, 21, "shard"))
# (camera, W, H) for which a zero lens and focus 1.0 do not give sample_ref's records in BITS (the values
# are equal everywhere): a -0.0 component can become +0.0 -- P + (R*0 + U*0) and dir0*1 - (R*0 + U*0) turn
# a -0.0 into +0.0 when the lens vector's zero is +0.0.  None of the cameras and sizes here has one.
ZERO_NOT_IN_BITS = ()


@pytest.mark.parametrize("name", sorted(_cameras()))
def test_zero_lens_and_unit_focus_is_the_pinhole(name):
    cam = _cameras()[name]
    pattern = rt_hip.grid_pattern(3)
    for W, H, rows in ZERO_SIZES:
        rows = rt_hip.rows_for_shard(21, 8, 2, 3) if rows else None
        a = lens_ref.camera_lens_rays(cam, W, H, pattern, [(0.0, 0.0)] * 9, 1.0, rows)
        b = sample_ref.camera_sample_rays(cam, W, H, pattern, rows)
        assert a.shape == b.shape and same_values(a, b).all(), (name, W, H)
        bits = bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
        assert bits == ((name, W, H) not in ZERO_NOT_IN_BITS), (name, W, H)


def test_lens_ray_layout_and_padding():
    cam = _cameras()["complex"]
    W, H = 7, 21
    rows = rt_hip.rows_for_shard(H, 8, 2, 3)  # rows 16..20 and three of padding
    pattern, lens = rt_hip.grid_pattern(2), rt_hip.lens_pattern(2, 0.25)
    rays = lens_ref.camera_lens_rays(cam, W, H, pattern, lens, 6.5, rows).reshape(rows.count, W, 4, 8)
    assert (rays[5:] == 0).all() and np.isinf(rays[:5, :, :, 6]).all() and (rays[:5, :, :, 7] == 0).all()
    pos, right, up = (np.array(list(v)) for v in (cam.position, cam.right, cam.up))
    for s, (lx, ly) in enumerate(lens):
        assert np.array_equal(rays[0, 0, s, 0:3], pos + (right * lx + up * ly))  # the origin: one per sample
        assert (rays[:5, :, s, 0:3] == rays[0, 0, s, 0:3]).all()
    assert np.allclose(np.linalg.norm(rays[:5, :, :, 3:6], axis=-1), 1.0, rtol=0, atol=4e-16)


def test_rays_of_one_pixel_meet_on_the_focal_plane():
    """For one pixel and one offset the rays from 16 lens points pass through F = P + dir0*focus.

    The bound, with eps = 2^-53 and M = |P| + focus*|dir0| + |lv| (Euclidean norms: no vector below is
    longer than M, so each rounding is at most eps*M per component):
      v = dir0*focus - lv     1 (scale) + 3 (lv: two products, one sum) + 1 (difference) = 5 roundings
      o = P + lv              3 + 1                                                      = 4 roundings
      d = v / |v|             the length is common to the components and moves no direction; the three
                              quotients turn d by at most eps, a miss of t*eps <= eps*M at F
      this test's own F, F - o, t*d and difference                                       = 5 roundings
    so the miss |F - o - t*d| is at most ((5 + 4 + 5)*sqrt(3) + 1) * eps * M < 26 * eps * M: 13 ulp of a
    focus distance of the size of M."""
    cam = _cameras()["complex"]
    W, H, x, y = 97, 61, 31, 17
    ox, oy = 0.25, 0.625
    for focus, aperture in ((7.5, 0.3), (0.75, 0.05), (120.0, 2.0)):
        lens = rt_hip.lens_pattern(4, aperture)
        assert len(set(lens)) == 16
        rays = lens_ref.camera_lens_rays(cam, W, H, [(ox, oy)] * 16, lens, focus).reshape(H, W, 16, 8)[y, x]
        dir0 = lens_ref.camera_dir(cam, W, H, H - 1 - y, ox, oy)[x]
        pos, right, up = (np.array(list(v)) for v in (cam.position, cam.right, cam.up))
        F = pos + dir0 * focus
        worst = 0.0
        for s, (lx, ly) in enumerate(lens):
            o, d = rays[s, 0:3], rays[s, 3:6]
            t = float(np.dot(F - o, d))
            miss = float(np.linalg.norm((F - o) - d * t))
            M = np.linalg.norm(pos) + focus * np.linalg.norm(dir0) + np.linalg.norm(right * lx + up * ly)
            assert t > 0 and miss <= 26 * 2.0 ** -53 * M, (focus, s, miss, M)
            worst = max(worst, miss / (2.0 ** -53 * M))
        print("focus %g aperture %g: worst miss %.2f eps*M" % (focus, aperture, worst))
        assert len({tuple(r[0:3]) for r in rays}) == 16  # and they do leave 16 different points
