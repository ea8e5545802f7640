"""GPU: multi-sample pixels resolved on the device (rt_camera_sample_rays,
rt_trace_radiance_resolve[_async], rt_render_samples, include/rt_hip.h), pinned

 1. to the render under rt_set_antialias(4) and to the oracle's render_aa, byte for
    byte, with the antialias pattern -- whole frames, one-row chunks, row shards;
 2. to the existing query: rt_trace_radiance(RT_FB_F64X3) of the same rays passed
    through tests/sample_ref.py's resolve, bit for bit, for arbitrary rays, sample
    counts and weights;
 3. at the edges: the reflection stack reused between samples, the grid-stride
    loop's second trip, bad rays, culling off, the bounds-checked build, the
    argument errors, a caller's stream, and the CLI's --supersample.

Every reference is computed once per process and never modified."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import path_ref
import ray_ref
import sample_ref
from conftest import PKG, manifest, scene_path
from test_gpu_paths import CAM, TWO, _fan, _scene
from test_gpu_radiance import _mirror_case
from test_radiance_host import same_values

pytestmark = pytest.mark.gpu

RGB8, F32X3, F64X3 = 0, 1, 2  # RT_FB_*
RECORD = {RGB8: (np.uint8, 3), F32X3: (np.float32, 12), F64X3: (np.float64, 24)}
INVALID, NO_SCENE, DEPTH = 1, 5, 7  # rt_status


def same_bits(a, b):
    """Elementwise: the same bit pattern, or a NaN on both sides."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


def negative_channels(c):
    """Channels write_ppm's quantiser makes negative: int(255.99 * min(1, c)) < 0."""
    c = np.asarray(c, np.float64)
    with np.errstate(all="ignore"):
        return int((np.trunc(255.99 * np.where(c < 1.0, c, 1.0)) < 0).sum())


def per_ray(r, o, d, S, depth, weights=None):
    """Reference 2: rt_trace_radiance(RT_FB_F64X3) of the rays through sample_ref.resolve, and its stats."""
    c, st = r.trace_radiance(o, d, depth, F64X3)
    return sample_ref.resolve(c.reshape(-1, S, 3), weights), st


def check_against(r, o, d, S, depth, weights, what):
    """The three formats of one resolve call against reference 2; returns the reference and the RGB8 stats."""
    want, st0 = per_ray(r, o, d, S, depth, weights)
    f64, st = r.trace_radiance_resolve(o, d, S, depth, weights, F64X3)
    assert f64.shape == want.shape and f64.dtype == np.float64
    assert same_bits(f64, want).all(), (what, np.flatnonzero(~same_bits(f64, want).all(axis=1)).tolist()[:8])
    assert (st.rays, st.segments, st.hits, st.shadow_rays, st.unaccelerated) == (
        st0.rays, st0.segments, st0.hits, st0.shadow_rays, st0.unaccelerated), what
    assert st.rays == o.shape[0] and st.negative_clamped == 0
    f32, _ = r.trace_radiance_resolve(o, d, S, depth, weights, F32X3)
    with np.errstate(all="ignore"):
        assert f32.dtype == np.float32 and same_bits(f32, want.astype(np.float32)).all(), what
    rgb, st8 = r.trace_radiance_resolve(o, d, S, depth, weights, RGB8)
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, path_ref.quantize(want)), what
    assert st8.negative_clamped == negative_channels(want), what
    assert (st8.rays, st8.segments) == (st0.rays, st0.segments)
    return want, st8


# ---- 1. the antialias pin ------------------------------------------------------------------------------
FIXTURES = ["complex_97x61_d4", "simple_2x2_d10", "simple_1x1_d10"]


@pytest.mark.parametrize("name", FIXTURES)
def test_antialias_pin(name):
    import orc
    import rt_hip
    import torch

    m = manifest()[name]
    W, H, D = m["width"], m["height"], m["depth"]
    n = W * H
    sc = rt_hip.Scene.load(scene_path(m["scene"]))
    cam = sc.camera()
    pattern = rt_hip.grid_pattern(2)
    r, r2 = rt_hip.Renderer(0), rt_hip.Renderer(0)
    try:
        r.upload(sc)
        r2.upload(sc)
        r.set_antialias(4)
        r2.set_antialias(4)
        want, st_aa = r.render(cam, W, H, D)
        want = bytes(want)
        oracle, _, _ = orc.OracleScene(scene_path(m["scene"])).render_aa(W, H, D, samples=4, threads=4)
        assert want == oracle
        shards = [rt_hip.rows_for_shard(H, 8, k, 3) for k in range(3)]
        want_shard = [bytes(r.render(cam, W, H, D, rows)[0]) for rows in shards]
        _, st_aa = r.render(cam, W, H, D)
        # what the context's other launches report, before
        rays1 = torch.zeros((n, 8), dtype=torch.float64, device="cuda:0")
        r.camera_rays(cam, W, H, None, rays1.data_ptr())
        k = min(n, 64)
        hits = torch.zeros((k, 2), dtype=torch.float64, device="cuda:0")
        r.trace_rays_device(rays1.data_ptr(), k, hits.data_ptr())
        verts = torch.zeros((D * k * 32,), dtype=torch.uint8, device="cuda:0")
        r.trace_paths_device(rays1.data_ptr(), k, D, verts.data_ptr())
        r.kernel_times()
        before = (r.stats().as_dict(), r.trace_stats().as_dict(), r.path_stats().as_dict(), r.info().launches)

        # RGB8: the render's bytes, the oracle's bytes and the render's counts
        rgb, st = r.render_samples(cam, W, H, D, pattern)
        assert rgb.shape == (n, 3) and rgb.tobytes() == want
        assert (st.rays, st.segments - st.rays, st.shadow_rays) == (st_aa.rays_primary, st_aa.rays_reflect,
                                                                   st_aa.rays_shadow)
        assert st.rays == 4 * n and st.negative_clamped == 0
        # one-row chunks (the smallest ray buffer), into a buffer that held other bytes
        out = np.full((n, 3), 0xA5, np.uint8)
        _, st1 = r.render_samples(cam, W, H, D, pattern, out=out, max_ray_bytes=1)
        assert out.tobytes() == want
        assert (st1.rays, st1.segments, st1.hits, st1.shadow_rays) == (st.rays, st.segments, st.hits, st.shadow_rays)
        assert r.radiance_stats().rays == 4 * W  # the most recent launch: the last row's
        # the device path, with a guard behind the image
        dev = torch.full((n * 3 + 4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        r.render_samples(cam, W, H, D, pattern, out=dev.data_ptr(), out_on_device=True, max_ray_bytes=5 * W * 4 * 64)
        got = dev.cpu().numpy()
        assert got[:n * 3].tobytes() == want and (got[n * 3:] == 0xA5).all()
        # every shard, padding rows included
        for rows, ws in zip(shards, want_shard):
            out = np.full((rows.count * W, 3), 0xA5, np.uint8)
            _, sts = r.render_samples(cam, W, H, D, pattern, rows=rows, out=out, max_ray_bytes=3 * W * 4 * 64)
            assert out.tobytes() == ws
            real = sum(1 for kk in range(rows.count)
                       if (kk // rows.band) * rows.band * rows.stride + rows.first * rows.band + kk % rows.band < H)
            assert sts.rays == 4 * W * real  # padding rows are not traced
            assert (out.reshape(rows.count, -1)[real:] == 0).all()

        # F64X3 / F32X3: the render's own antialias framebuffers of a second context, as values
        for fmt, tdtype in ((F64X3, torch.float64), (F32X3, torch.float32)):
            fb = torch.full((n * 3,), float("nan"), dtype=tdtype, device="cuda:0")
            torch.cuda.synchronize()  # the fill (torch's stream) lands before the tile
            r2.render_tile(cam, W, H, D, 0, 0, W, H, fmt, fb.data_ptr())
            r2.stats()
            fbw = fb.cpu().numpy().reshape(H, W, 3)[::-1].reshape(n, 3)  # j = 0 is the bottom row
            got, stf = r.render_samples(cam, W, H, D, pattern, fmt=fmt)
            assert got.dtype == RECORD[fmt][0]
            same = same_values(got, fbw)
            assert same.all(), (fmt, int((~same).sum()))
            assert np.isnan(fbw).any() == (name == "simple_1x1_d10")
            assert stf.negative_clamped == 0 and (stf.rays, stf.segments) == (st.rays, st.segments)

        # the sample rays themselves, and the two-call form on the device
        rays = torch.zeros((n * 4, 8), dtype=torch.float64, device="cuda:0")
        r.camera_sample_rays(cam, W, H, None, pattern, rays.data_ptr())
        dev = torch.zeros((n * 3 + 16,), dtype=torch.uint8, device="cuda:0")
        r.trace_radiance_resolve_device(rays.data_ptr(), n, 4, D, RGB8, dev.data_ptr())
        assert r.radiance_stats().rays == 4 * n
        assert dev.cpu().numpy()[:n * 3].tobytes() == want
        host = rays.cpu().numpy()
        assert same_bits(host, sample_ref.camera_sample_rays(cam, W, H, pattern)).all()

        # the context's other launches are left alone
        after = (r.stats().as_dict(), r.trace_stats().as_dict(), r.path_stats().as_dict(), r.info().launches)
        for got_d, want_d in zip(after[:3], before[:3]):
            # the same launch's events read a second time: the runtime's float differs in its last digits
            assert got_d.pop("kernel_ms") == pytest.approx(want_d.pop("kernel_ms"), rel=1e-4)
        assert after == before
        assert r.kernel_times() == []
        assert bytes(r.render(cam, W, H, D)[0]) == want  # rt_set_antialias still holds for the render
    finally:
        r.close()
        r2.close()


def test_sample_rays_match_the_checker(gpu_renderer):
    """A shard with padding rows, nine samples, an offset that is not finite; and one (0, 0) sample is
    rt_camera_rays bit for bit."""
    import rt_hip
    import torch

    sc = rt_hip.Scene.load(scene_path("complex"))
    cam = sc.camera()
    W, H = 37, 21
    rows = rt_hip.rows_for_shard(H, 8, 2, 3)
    for pattern in (rt_hip.grid_pattern(3), [(0.25, float("nan")), (float("inf"), 0.5), (-1.5, 2.0)]):
        S = len(pattern)
        rays = torch.full((rows.count * W * S + 1, 8), 7.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        gpu_renderer.camera_sample_rays(cam, W, H, rows, pattern, rays.data_ptr())
        gpu_renderer.radiance_stats()  # waits for the stream
        got = rays.cpu().numpy()
        assert same_bits(got[:-1], sample_ref.camera_sample_rays(cam, W, H, pattern, rows)).all()
        assert (got[-1] == 7.0).all()
    a = torch.zeros((W * H, 8), dtype=torch.float64, device="cuda:0")
    b = torch.zeros((W * H, 8), dtype=torch.float64, device="cuda:0")
    gpu_renderer.camera_sample_rays(cam, W, H, None, [(0.0, 0.0)], a.data_ptr())
    gpu_renderer.camera_rays(cam, W, H, None, b.data_ptr())
    gpu_renderer.radiance_stats()
    assert np.array_equal(a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64))


# ---- 2. the existing query as yardstick --------------------------------------------------------------
SAMPLES = (1, 2, 3, 5, 16, 64)
PIXELS = (1, 63, 64, 65, 129)
DEPTH4 = 4


@functools.lru_cache(maxsize=None)
def _batch(name):
    sc, sa = _scene(name)
    o, d = ray_ref.gen_rays(3, max(PIXELS) * max(SAMPLES), sa.centers, sa.radii, tuple(sc.camera().position))
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


def _weights(S):
    """Random weights, the first one negative and large: some pixel sums are below zero."""
    w = np.random.default_rng(100 + S).uniform(0.0, 1.0, S) / S
    w[0] = -1.5
    return w


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("name", ["simple", "complex"])
def test_resolve_equals_the_per_ray_query(gpu_renderer, name, S):
    gpu_renderer.upload(_scene(name)[0])
    o, d = _batch(name)
    clamped = 0
    for npix in PIXELS:
        n = npix * S
        want, st8 = check_against(gpu_renderer, o[:n], d[:n], S, DEPTH4, None, (name, S, npix, "box"))
        assert st8.negative_clamped == 0
        _, st8 = check_against(gpu_renderer, o[:n], d[:n], S, DEPTH4, _weights(S), (name, S, npix, "weights"))
        clamped += st8.negative_clamped
    assert clamped > 0


def test_single_sample_keeps_minus_zero(gpu_renderer):
    """One unweighted sample is the colour itself: a hit of reflectivity > 1 with no depth left stores
    col * (1 - refl), -0.0 for a zero channel, as rt_trace_radiance does; one sample weighted 1.0 goes
    through 0 + c * 1.0 and stores +0.0."""
    import material_cases as mc
    import rt_hip

    text = mc.text("refl_above_one_s01", "dense").replace("0.9 0.2 0.2", "0.9 0 0.2")  # sphere A: no green
    assert text != mc.text("refl_above_one_s01", "dense")
    sc = rt_hip.Scene.parse(text)
    W, H = 64, 48
    rays = ray_ref.camera_rays(sc.camera(), W, H)
    o, d = rays[:, 0:3], rays[:, 3:6]
    gpu_renderer.upload(sc)
    want, _ = gpu_renderer.trace_radiance(o, d, 1, F64X3)
    minus_zero = (want == 0.0) & np.signbit(want)
    assert minus_zero.any()
    got, _ = gpu_renderer.trace_radiance_resolve(o, d, 1, 1, None, F64X3)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    one, _ = gpu_renderer.trace_radiance_resolve(o, d, 1, 1, [1.0], F64X3)
    assert np.array_equal(one.view(np.uint64), sample_ref.resolve(want.reshape(-1, 1, 3), [1.0]).view(np.uint64))
    assert not np.signbit(one[minus_zero]).any()


# ---- 3. the reflection stack between samples ---------------------------------------------------------
@pytest.mark.parametrize("S", [2, 5])
def test_stack_reuse_between_samples(gpu_renderer, S):
    sc, sa, o, d, levels, _ = _mirror_case()
    D = len(levels)
    length = np.sum([lv["traced"] for lv in levels], axis=0)
    order = np.argsort(-length, kind="stable")  # longest first
    mixed = np.empty_like(order)
    mixed[0::2] = order[:(len(order) + 1) // 2]       # long, short, long, ...: a pixel's consecutive samples
    mixed[1::2] = order[::-1][:len(order) // 2]       # alternate long and short chains
    n = (len(mixed) // S) * S
    pick = mixed[:n]
    assert abs(int(length[pick[0]]) - int(length[pick[1]])) > 32
    gpu_renderer.upload(sc)
    for weights in (None, _weights(S)):
        want, st0 = per_ray(gpu_renderer, o[pick], d[pick], S, D, weights)
        got, st = gpu_renderer.trace_radiance_resolve(o[pick], d[pick], S, D, weights, F64X3)
        assert same_bits(got, want).all()
        assert (st.rays, st.segments, st.hits) == (n, int(length[pick].sum()), st0.hits)


# ---- 4. the grid-stride loop's second trip -----------------------------------------------------------
def test_second_trip(gpu_renderer):
    import rt_hip
    import torch

    sc = rt_hip.Scene.load(scene_path("simple"))
    sa = path_ref.SceneArrays(sc)
    S, nb, depth = 2, 4133, 4
    o, d = ray_ref.gen_rays(1, nb * S, sa.centers, sa.radii, tuple(sc.camera().position))
    levels = path_ref.trace_paths(o, d, depth, sa)
    gpu_renderer.upload(sc)
    want, _ = per_ray(gpu_renderer, o, d, S, depth)
    base, st0 = gpu_renderer.trace_radiance_resolve(o, d, S, depth, None, RGB8)
    assert np.array_equal(base, path_ref.quantize(want))
    n = 64 * 64 * torch.cuda.get_device_properties(0).multi_processor_count + 64 + 37
    small = np.zeros((nb, S, 8))
    small[:, :, 0:3], small[:, :, 3:6] = o.reshape(nb, S, 3), d.reshape(nb, S, 3)
    rays = torch.from_numpy(np.resize(small.reshape(nb, S * 8), (n, S * 8))).to("cuda:0")
    guard = 4096
    out = torch.full((n * 3 + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
    gpu_renderer.trace_radiance_resolve_device(rays.data_ptr(), n, S, depth, RGB8, out.data_ptr())
    st = gpu_renderer.radiance_stats()
    got = out.cpu().numpy()
    assert np.array_equal(got[:n * 3].reshape(n, 3), np.resize(base, (n, 3)))
    assert (got[n * 3:] == 0xA5).all()  # the guard after the buffer is untouched
    per_pixel = np.sum([lv["traced"] for lv in levels], axis=0).reshape(nb, S).sum(axis=1)
    assert (st.rays, st.segments) == (n * S, int(np.resize(per_pixel, n).sum()))


# ---- 5. bad rays -------------------------------------------------------------------------------------
def test_bad_rays(gpu_renderer):
    import rt_hip

    sc = rt_hip.Scene.parse(TWO + "light 3 4 0 1 1 1 1\n" + CAM)
    gpu_renderer.upload(sc)
    S, depth = 3, 3
    o, d = _fan()
    o, d = o[:63].copy(), d[:63].copy()  # 21 pixels
    clean64, _ = gpu_renderer.trace_radiance_resolve(o, d, S, depth, None, F64X3)
    clean8, _ = gpu_renderer.trace_radiance_resolve(o, d, S, depth, None, RGB8)
    assert np.isfinite(clean64).all()
    nan, inf = float("nan"), float("inf")
    for pixel, sample, bad in ((5, 0, (0.0, 0.0, 0.0)), (11, 1, (0.0, nan, -1.0)), (20, 2, (0.0, inf, -1.0)),
                               (0, 1, (0.0, 0.0, 0.0))):
        d2 = d.copy()
        d2[pixel * S + sample] = bad
        others = np.arange(21) != pixel
        for weights in (None, [0.5, 0.25, 0.25]):
            ref64, _ = gpu_renderer.trace_radiance_resolve(o, d, S, depth, weights, F64X3)
            ref8, _ = gpu_renderer.trace_radiance_resolve(o, d, S, depth, weights, RGB8)
            got64, st = gpu_renderer.trace_radiance_resolve(o, d2, S, depth, weights, F64X3)
            got8, st8 = gpu_renderer.trace_radiance_resolve(o, d2, S, depth, weights, RGB8)
            assert np.isnan(got64[pixel]).all() and (got8[pixel] == 255).all()
            assert np.array_equal(got64[others].view(np.uint64), ref64[others].view(np.uint64))
            assert np.array_equal(got8[others], ref8[others])
            assert st.rays == 63 and st.unaccelerated >= 1 and st8.negative_clamped == 0


# ---- 6. variants -------------------------------------------------------------------------------------
VARIANT_SHAPE = ("complex", 3, 129)


@functools.lru_cache(maxsize=None)
def _product(weighted):
    import rt_hip

    name, S, npix = VARIANT_SHAPE
    o, d = _batch(name)
    n = S * npix
    r = rt_hip.Renderer(0)
    try:
        r.upload(_scene(name)[0])
        want, st8 = check_against(r, o[:n], d[:n], S, DEPTH4, _weights(S) if weighted else None, "product")
        rgb, _ = r.trace_radiance_resolve(o[:n], d[:n], S, DEPTH4, _weights(S) if weighted else None, RGB8)
    finally:
        r.close()
    return want.tobytes(), rgb.tobytes(), (st8.rays, st8.segments, st8.hits, st8.shadow_rays)


def _check_variant(r, unculled=False):
    name, S, npix = VARIANT_SHAPE
    o, d = _batch(name)
    n = S * npix
    for weighted in (False, True):
        w = _weights(S) if weighted else None
        want64, want8, counts = _product(weighted)
        f64, st = r.trace_radiance_resolve(o[:n], d[:n], S, DEPTH4, w, F64X3)
        rgb, _ = r.trace_radiance_resolve(o[:n], d[:n], S, DEPTH4, w, RGB8)
        assert (f64.tobytes(), rgb.tobytes()) == (want64, want8)
        assert (st.rays, st.segments, st.hits, st.shadow_rays) == counts
        if unculled:
            assert st.unaccelerated == st.segments + st.shadow_rays and st.tests_cull == 0


def test_unculled_same_bytes(gpu_renderer):
    gpu_renderer.upload(_scene(VARIANT_SHAPE[0])[0])
    gpu_renderer.set_culling(False)
    try:
        _check_variant(gpu_renderer, unculled=True)
    finally:
        gpu_renderer.set_culling(True)


def test_checked_build():
    import rt_hip

    r = rt_hip.Renderer(0, variant="check")
    try:
        sc = _scene(VARIANT_SHAPE[0])[0]
        r.upload(sc)
        _check_variant(r)
        W, H, D = 37, 21, 4
        rgb, _ = r.render_samples(sc.camera(), W, H, D, rt_hip.grid_pattern(2), max_ray_bytes=1)
        r.stats()  # raises on RT_ERR_CHECK
        p = rt_hip.Renderer(0)
        try:
            p.upload(sc)
            p.set_antialias(4)
            assert rgb.tobytes() == bytes(p.render(sc.camera(), W, H, D)[0])
        finally:
            p.close()
    finally:
        r.close()


# ---- 7. errors and streams ---------------------------------------------------------------------------
def test_errors():
    import rt_hip
    import torch

    o, d = _fan()
    o, d = o[:64], d[:64]
    r = rt_hip.Renderer(0)
    L = r._L
    try:
        cam = rt_hip.Scene.parse(TWO + CAM).camera()
        pattern = rt_hip.grid_pattern(2)
        for call in (lambda: r.trace_radiance_resolve(o, d, 2, 3), lambda: r.render_samples(cam, 4, 4, 3, pattern)):
            with pytest.raises(rt_hip.RtError) as e:
                call()
            assert e.value.status == NO_SCENE
        sc = rt_hip.Scene.parse(TWO + "light 3 4 0 1 1 1 1\n" + CAM)
        r.upload(sc)
        cam = sc.camera()
        for call in (lambda: r.trace_radiance_resolve(o, d, 2, rt_hip.RT_MAX_DEPTH + 1),
                     lambda: r.render_samples(cam, 4, 4, rt_hip.RT_MAX_DEPTH + 1, pattern)):
            with pytest.raises(rt_hip.RtError) as e:
                call()
            assert e.value.status == DEPTH
        rays = torch.zeros((130, 8), dtype=torch.float64, device="cuda:0")
        out = torch.zeros((66 * 24 + 16,), dtype=torch.uint8, device="cuda:0")
        rp, op = rays.data_ptr(), out.data_ptr()
        off = (C.c_double * 130)()
        big = (C.c_double * 130)()
        rows = rt_hip.rt_rows(1, 0, 1, 1 << 20)
        bad = [
            # samples outside 1..RT_MAX_SAMPLES
            lambda: r.trace_radiance_resolve_device(rp, 64, 0, 3, F64X3, op),
            lambda: r.trace_radiance_resolve_device(rp, 1, 65, 3, F64X3, op),
            lambda: r.trace_radiance_resolve_device(rp, 64, -1, 3, F64X3, op),
            lambda: L.rt_camera_sample_rays(r.handle, C.byref(cam), 4, 4, None, off, 0, C.c_void_p(rp)),
            lambda: L.rt_camera_sample_rays(r.handle, C.byref(cam), 4, 4, None, big, 65, C.c_void_p(rp)),
            lambda: L.rt_render_samples(r.handle, C.byref(cam), 4, 4, 3, None, big, 65, None, RGB8, C.c_void_p(op), 1,
                                        0, None),
            lambda: L.rt_render_samples(r.handle, C.byref(cam), 4, 4, 3, None, off, 0, None, RGB8, C.c_void_p(op), 1,
                                        0, None),
            # more than 2^31-1 rays
            lambda: r.trace_radiance_resolve_device(rp, (1 << 30), 2, 3, F64X3, op),
            lambda: r.trace_radiance_resolve_device(rp, (1 << 31) // 64, 64, 3, F64X3, op),
            lambda: L.rt_camera_sample_rays(r.handle, C.byref(cam), 1 << 10, 1 << 20, C.byref(rows), off, 2,
                                            C.c_void_p(rp)),
            lambda: r.render_samples(cam, 1 << 26, 4, 3, rt_hip.grid_pattern(8), out=op, out_on_device=True),
            # NULL and misaligned pointers
            lambda: L.rt_camera_sample_rays(r.handle, C.byref(cam), 4, 4, None, None, 2, C.c_void_p(rp)),
            lambda: L.rt_camera_sample_rays(r.handle, None, 4, 4, None, off, 2, C.c_void_p(rp)),
            lambda: L.rt_camera_sample_rays(r.handle, C.byref(cam), 4, 4, None, off, 2, None),
            lambda: L.rt_camera_sample_rays(r.handle, C.byref(cam), 4, 4, None, off, 2, C.c_void_p(rp + 8)),
            lambda: r.trace_radiance_resolve_device(rp + 8, 64, 2, 3, F64X3, op),
            lambda: r.trace_radiance_resolve_device(rp, 64, 2, 3, F64X3, op + 8),
            lambda: r.trace_radiance_resolve_device(0, 64, 2, 3, F64X3, op),
            lambda: r.trace_radiance_resolve_device(rp, 64, 2, 3, F64X3, 0),
            lambda: L.rt_render_samples(r.handle, C.byref(cam), 4, 4, 3, None, None, 4, None, RGB8, C.c_void_p(op), 1,
                                        0, None),
            lambda: L.rt_render_samples(r.handle, C.byref(cam), 4, 4, 3, None, off, 4, None, RGB8, None, 1, 0, None),
            lambda: L.rt_render_samples(r.handle, C.byref(cam), 4, 4, 3, None, off, 4, None, RGB8, C.c_void_p(op + 8),
                                        1, 0, None),
            # depth and format
            lambda: r.trace_radiance_resolve_device(rp, 64, 2, 0, F64X3, op),
            lambda: r.trace_radiance_resolve_device(rp, 64, 2, 3, 3, op),
            lambda: r.render_samples(cam, 4, 4, 0, pattern),
            lambda: r.render_samples(cam, 4, 4, 3, pattern, fmt=-1),
        ]
        for i, call in enumerate(bad):
            try:
                rc = call()
            except rt_hip.RtError as e:
                rc = e.status
            assert rc == INVALID, (i, rc)
        assert r.radiance_stats().rays == 0  # nothing was launched
        # no pixels: a no-op
        none, st0 = r.trace_radiance_resolve(np.zeros((0, 3)), np.zeros((0, 3)), 4, 3)
        assert none.shape == (0, 3) and st0.rays == 0 and r.radiance_stats().rays == 0
        # rows->count * width * samples above the limit is fine for rt_render_samples: one row is the chunk
        got, st = r.trace_radiance_resolve(o, d, 2, 3)  # the context is fine
        assert st.rays == 64 and got.shape == (32, 3) and got.dtype == np.float64
    finally:
        r.close()


def test_device_path_and_streams():
    import rt_hip
    import torch

    name, S, npix = VARIANT_SHAPE
    o, d = _batch(name)
    n = S * npix
    host = np.zeros((n, 8), np.float64)
    host[:, 0:3], host[:, 3:6] = o[:n], d[:n]
    w = _weights(S)
    r = rt_hip.Renderer(0)
    side = torch.cuda.Stream()
    try:
        r.upload(_scene(name)[0])
        want = r.trace_radiance_resolve(o[:n], d[:n], S, DEPTH4, w, F64X3)[0].tobytes()
        assert torch.cuda.current_stream().cuda_stream == 0
        rays = torch.from_numpy(host).to("cuda:0")  # filled on the legacy NULL stream
        out = torch.zeros((npix * 24,), dtype=torch.uint8, device="cuda:0")
        r.trace_radiance_resolve_device(rays.data_ptr(), npix, S, DEPTH4, F64X3, out.data_ptr(), w)
        assert out.cpu().numpy().tobytes() == want  # read on the NULL stream, no host sync between
        assert r.radiance_stats().rays == n
        r.set_stream(side.cuda_stream)
        with torch.cuda.stream(side):
            out2 = torch.zeros((npix * 24,), dtype=torch.uint8, device="cuda:0")
            r.trace_radiance_resolve_device(rays.data_ptr(), npix, S, DEPTH4, F64X3, out2.data_ptr(), w)
            got = out2.cpu().numpy().tobytes()
        assert got == want
        # the synchronous call takes device memory too
        out3 = torch.zeros((npix * 24,), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()  # the side stream is not ordered with the NULL stream's fill
        st = rt_hip.rt_radiance_stats()
        wa = (C.c_double * S)(*w)
        rc = r._L.rt_trace_radiance_resolve(r.handle, C.c_void_p(rays.data_ptr()), npix, S, wa, DEPTH4, F64X3,
                                            C.c_void_p(out3.data_ptr()), 1, C.byref(st))
        assert rc == 0 and st.rays == n
        side.synchronize()
        assert out3.cpu().numpy().tobytes() == want
    finally:
        r.set_stream(None)
        r.close()


# ---- 8. the CLI --------------------------------------------------------------------------------------
def _ray_hip(tmp_path, *args):
    return subprocess.run([os.path.join(PKG, "ray_hip"), *args], cwd=tmp_path, capture_output=True, text=True,
                          timeout=300)


def test_cli_supersample(tmp_path):
    import rt_hip

    size = ("--width", "97", "--height", "61", "--depth", "4")
    scene = scene_path("complex")
    for flags, out in ((("-a",), "aa.ppm"), (("--supersample", "2"), "s2.ppm"), (("--supersample", "3"), "s3.ppm")):
        p = _ray_hip(tmp_path, *flags, *size, "--out", out, scene)
        assert p.returncode == 0 and "GPU rendering time:" in p.stdout, p.stdout + p.stderr
    aa = open(tmp_path / "aa.ppm", "rb").read()
    assert aa.startswith(b"P3\n") and open(tmp_path / "s2.ppm", "rb").read() == aa
    sc = rt_hip.Scene.load(scene)
    r = rt_hip.Renderer(0)
    try:
        r.upload(sc)
        rgb, _ = r.render_samples(sc.camera(), 97, 61, 4, rt_hip.grid_pattern(3))
    finally:
        r.close()
    rt_hip.write_ppm(str(tmp_path / "lib3.ppm"), rgb, 97, 61)
    s3 = open(tmp_path / "s3.ppm", "rb").read()
    assert s3 == open(tmp_path / "lib3.ppm", "rb").read() and s3 != aa
    for flags in (("--supersample", "2", "--gpus", "2"), ("--supersample", "2", "--devices", "0,0"),
                  ("--supersample", "2", "-a"), ("--supersample", "0"), ("--supersample", "9"), ("--supersample",)):
        p = _ray_hip(tmp_path, *flags, *size, scene)
        assert p.returncode == 2 and "usage:" in p.stderr, flags
