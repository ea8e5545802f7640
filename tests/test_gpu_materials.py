"""Shading on materials, lights and ambient outside the ranges every other test keeps to
(tests/material_cases.py), in every layout that quantises or counts a pixel.

Every comparison is against the CPU oracle (pinned to the reference on these very scenes by
test_material_cases_host.py).  Bars:

  `exact` cases (every shininess 0, 1 or a whole number in [1, 1024])   RGB8 byte-identical
  the others (pm1)           every channel within 1 of the oracle's; the number that differ is printed
  both                       rays_primary, rays_shadow and rays_reflect equal the oracle's, and
                             negative_clamped equals the oracle's `negative`: a one-ulp pow difference can
                             move that count only where a channel sits on the -1 / 255.99 boundary

The counter rt_stats.negative_clamped is non-zero in the `expects_negative` cases (the host test asserts
the oracle's is), so a kernel that never counted, counted a pixel in both the merged and a deferred kernel,
or stored a wrapped negative byte fails here.

Layouts: (a) one-frame render, (b) multi-frame launches (levels >= 2 in the deferred kernels), (c) row
shards, (d) rt_render_tile in the three framebuffer formats, (e) 4-sample antialias, (f) the global-stack
and defer-one-frame knob layouts, (g) the device group, (h) the ray_hip CLI's warning, (i) path queries'
`reflectivity > 0` rule."""
import os
import subprocess

import numpy as np
import pytest

import material_cases as mc
import path_ref
import ray_ref
from conftest import PKG, diff_summary, knob_variant
from test_gpu_tile_aa import MAX_ULP, ulp_diff
from test_oracle_vs_reference import p3

pytestmark = pytest.mark.gpu

BIG = (97, 61)


def _scene(case, form="dense"):
    import rt_hip

    return rt_hip.Scene.parse(mc.text(case, form))


def _pm1(got: bytes, want: bytes):
    """Every channel within 1 of the oracle's; returns the number of differing channels."""
    d = np.abs(np.frombuffer(got, np.uint8).astype(np.int16) - np.frombuffer(want, np.uint8).astype(np.int16))
    assert len(got) == len(want) and int(d.max()) <= 1, diff_summary(got, want)
    return int((d > 0).sum())


def check_bytes(case, got: bytes, want: bytes, where):
    if mc.is_exact(case):
        assert got == want, "%s: %s" % (where, diff_summary(got, want))
    else:
        nd = _pm1(got, want)
        print("%s: %d of %d channels differ" % (where, nd, len(want)))


def check_stats(st, counts, where, times=1):
    assert (st.rays_primary, st.rays_shadow, st.rays_reflect) == tuple(times * v for v in mc.ray_counts(counts)), where
    assert st.negative_clamped == times * counts["negative"], where
    if times and counts["negative"]:
        assert st.negative_clamped > 0


# ---- (a) one-frame render ----------------------------------------------------------------
@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("case", mc.NAMES)
def test_render(gpu_renderer, case, form):
    sc = _scene(case, form)
    gpu_renderer.upload(sc)
    culls = (True, False) if mc.expects_negative(case) else (True,)
    try:
        for cull in culls:
            gpu_renderer.set_culling(cull)
            for W, H, D in mc.combos(case, form):
                want, counts, _ = mc.oracle(case, form, W, H, D)
                where = "%s %s %dx%d d%d %s" % (case, form, W, H, D, "cull" if cull else "brute")
                rgb, st = gpu_renderer.render(sc.camera(), W, H, D)
                check_bytes(case, bytes(rgb), want, where)
                check_stats(st, counts, where)
    finally:
        gpu_renderer.set_culling(True)


# ---- (b) multi-frame launches ----------------------------------------------------------------
def _frames(r, cams, W, H, D, pad):
    import torch

    n = H * W * 3
    stride = n + pad
    buf = torch.full((len(cams) * stride,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()  # the fill (torch's stream) lands before the render
    r.render_frames_async(cams, W, H, D, None, buf.data_ptr(), stride)
    st = r.stats()
    host = buf.cpu().numpy()
    return ([host[f * stride:f * stride + n].tobytes() for f in range(len(cams))],
            [host[f * stride + n:(f + 1) * stride] for f in range(len(cams))], st)


@pytest.mark.parametrize("case", mc.NAMES)
def test_frames(gpu_renderer, case):
    """Three identical frames in one launch: reflection levels >= 2 go to render_deferred*, whose pixels are
    OR-ed into place and counted in that kernel.  With a frame stride 37 bytes larger than the frame at
    depth 4: the gaps keep their fill."""
    sc = _scene(case)
    gpu_renderer.upload(sc)
    W, H = BIG
    F = 3
    for D, pad in ((4, 0), (10, 0), (4, 37)):
        want, counts, _ = mc.oracle(case, "dense", W, H, D)
        frames, gaps, st = _frames(gpu_renderer, [sc.camera()] * F, W, H, D, pad)
        for f in range(F):
            check_bytes(case, frames[f], want, "%s frame %d of %d, d%d, pad %d" % (case, f, F, D, pad))
            assert (gaps[f] == 0xA5).all()
        check_stats(st, counts, "%s %d frames d%d" % (case, F, D), times=F)


# ---- (c) row shards -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.EXPECTS_NEGATIVE)
def test_row_shards(gpu_renderer, case):
    import rt_hip

    sc = _scene(case)
    gpu_renderer.upload(sc)
    W, H = BIG
    D, G, band = 4, 3, 8
    want, counts, _ = mc.oracle(case, "dense", W, H, D)
    img = np.zeros((H, W, 3), np.uint8)
    total = {"primary": 0, "shadow": 0, "reflect": 0, "negative": 0}
    for r in range(G):
        rows = rt_hip.rows_for_shard(H, band, r, G)
        rgb, st = gpu_renderer.render(sc.camera(), W, H, D, rows=rows)
        shard = np.frombuffer(bytes(rgb), np.uint8).reshape(rows.count, W, 3)
        for k in range(rows.count):
            y = (k // band) * band * G + r * band + k % band
            if y < H:
                img[y] = shard[k]
            else:
                assert not shard[k].any(), (r, k)  # padding rows are zero
        for q, v in (("primary", st.rays_primary), ("shadow", st.rays_shadow), ("reflect", st.rays_reflect),
                     ("negative", st.negative_clamped)):
            total[q] += v
    check_bytes(case, img.tobytes(), want, case + " shards")
    assert total == counts
    assert total["negative"] > 0


# ---- (d) rt_render_tile ---------------------------------------------------------------------------
def _tiles(W, H, t=16):
    for ty in range(0, H, t):
        for tx in range(0, W, t):
            yield tx, ty, t, t


def _render_tiles(r, sc, W, H, D, fmt, dtype, fill):
    """The whole image as 16x16 tiles into one device framebuffer; returns (numpy, the stats summed)."""
    import torch

    fb = torch.full((H * W * 3,), fill, dtype=dtype, device="cuda:0")
    torch.cuda.synchronize()  # the fill (torch's stream) lands before the tiles
    total = {"primary": 0, "shadow": 0, "reflect": 0, "negative": 0}
    for tx, ty, w, h in _tiles(W, H):
        r.render_tile(sc.camera(), W, H, D, tx, ty, w, h, fmt, fb.data_ptr())
        st = r.stats()
        for q, v in (("primary", st.rays_primary), ("shadow", st.rays_shadow), ("reflect", st.rays_reflect),
                     ("negative", st.negative_clamped)):
            total[q] += v
    return fb.cpu().numpy(), total


@pytest.mark.parametrize("case", mc.NAMES + tuple(mc.F64_CASES))
def test_tiles_rgb8(gpu_renderer, case):
    import rt_hip
    import torch

    sc = _scene(case)
    gpu_renderer.upload(sc)
    W, H, D = mc.F64_SHAPE
    want, counts, _ = mc.oracle(case, "dense", W, H, D)
    got, total = _render_tiles(gpu_renderer, sc, W, H, D, rt_hip.RT_FB_RGB8, torch.uint8, 7)
    check_bytes(case, got.tobytes(), want, case + " tiles")
    assert total == counts
    assert (total["negative"] > 0) == mc.expects_negative(case)


@pytest.mark.parametrize("case", tuple(mc.F64_CASES))
def test_tiles_unquantised(gpu_renderer, case):
    """F64_CASES: shininess 0 and 1 only (pow(x, 0) = 1, pow(x, 1) = x: no pow rounding, so RT_FB_F64X3 equals
    the oracle's framebuffer numerically, -0.0 equal to +0.0 and +inf to +inf), or -1 everywhere but the
    mirror (finite channels within MAX_ULP, the same channels +inf).  RT_FB_F32X3 is float(oracle) by the
    bound of test_gpu_tile_aa.test_tiles_f32_and_rgb8, +inf where the oracle is +inf or beyond FLT_MAX.
    The unquantised formats clamp nothing: negative_clamped is 0."""
    import rt_hip
    import torch

    sc = _scene(case)
    gpu_renderer.upload(sc)
    W, H, D = mc.F64_SHAPE
    _, counts, fb = mc.oracle(case, "dense", W, H, D)
    ref = fb[::-1]  # the tile framebuffer is indexed j*W + x with j = 0 the bottom row
    inf = np.isposinf(ref)
    fin = ~inf

    got, total = _render_tiles(gpu_renderer, sc, W, H, D, rt_hip.RT_FB_F64X3, torch.float64, float("nan"))
    got = got.reshape(H, W, 3)
    assert not np.isnan(got).any()
    assert np.array_equal(np.isposinf(got), inf) and not np.isneginf(got).any()
    d = ulp_diff(np.ascontiguousarray(got[fin]), np.ascontiguousarray(ref[fin]))
    print("%s f64: max %d ulp, %d of %d channels differ" % (case, int(d.max()), int((d > 0).sum()), d.size))
    assert int(d.max()) <= (MAX_ULP if case == "shin_minus_one" else 0), int((d > 0).sum())
    assert total == dict(counts, negative=0)

    got32, total32 = _render_tiles(gpu_renderer, sc, W, H, D, rt_hip.RT_FB_F32X3, torch.float32, float("nan"))
    got32 = got32.reshape(H, W, 3).astype(np.float64)
    with np.errstate(over="ignore"):
        want32 = ref.astype(np.float32).astype(np.float64)  # beyond FLT_MAX: inf
    big = np.isinf(want32)
    assert big[inf].all()
    assert not np.isnan(got32).any() and np.array_equal(got32[big], want32[big])
    ok = ~big
    err = np.abs(got32[ok] - ref[ok]) - (np.abs(ref[ok]) * 2.0**-23 + 2.0**-125)
    assert (err <= 0).all(), float(err.max())
    assert total32 == dict(counts, negative=0)


# ---- (e) antialias --------------------------------------------------------------------------
@pytest.fixture
def aa_renderer(gpu_renderer):
    gpu_renderer.set_antialias(4)
    yield gpu_renderer
    gpu_renderer.set_antialias(1)


@pytest.mark.parametrize("case", mc.AA_CASES)
def test_antialias(aa_renderer, case):
    sc = _scene(case)
    aa_renderer.upload(sc)
    for W, H, D in mc.AA_SHAPES:
        want, counts, _ = mc.oracle_aa(case, W, H, D)
        where = "%s antialias %dx%d d%d" % (case, W, H, D)
        rgb, st = aa_renderer.render(sc.camera(), W, H, D)
        check_bytes(case, bytes(rgb), want, where)
        check_stats(st, counts, where)
        assert st.rays_primary == 4 * W * H


# ---- (f) knob layouts -------------------------------------------------------------------------
@pytest.fixture(params=[{"RT_HIP_STACK": "1"}, {"RT_HIP_DEFER": "1"}], ids=["global-stack", "defer-one-frame"])
def layout_renderer(request, monkeypatch):
    """A fresh context per layout (the knobs are read at rt_create, by the tuning build)."""
    import rt_hip

    for k, v in request.param.items():
        monkeypatch.setenv(k, v)
    r = rt_hip.Renderer(0, variant=knob_variant())
    yield r
    r.close()


@pytest.mark.parametrize("case", mc.EXPECTS_NEGATIVE)
def test_knob_layouts(layout_renderer, case):
    sc = _scene(case)
    layout_renderer.upload(sc)
    W, H = BIG
    D = 4
    want, counts, _ = mc.oracle(case, "dense", W, H, D)
    rgb, st = layout_renderer.render(sc.camera(), W, H, D)
    check_bytes(case, bytes(rgb), want, case + " layout")
    check_stats(st, counts, case + " layout")
    assert st.negative_clamped > 0


# ---- (g) the device group -----------------------------------------------------------------------
@pytest.mark.parametrize("case", ["colour_negative", "ambient_negative"])
def test_group(case):
    import rt_hip

    sc = _scene(case)
    W, H = BIG
    D, F = 4, 3
    n = H * W * 3
    want, counts, _ = mc.oracle(case, "dense", W, H, D)
    g = rt_hip.Group([0, 0], band=8)
    try:
        g.upload(sc)
        rgb, st = g.render(sc.camera(), W, H, D)
        check_bytes(case, bytes(rgb), want, case + " group")
        check_stats(st, counts, case + " group")
        assert st.negative_clamped > 0
        rgb, st = g.render_frames([sc.camera()] * F, W, H, D, batch=2)
        assert len(rgb) == F * n
        for f in range(F):
            check_bytes(case, bytes(rgb[f * n:(f + 1) * n]), want, "%s group frame %d" % (case, f))
        check_stats(st, counts, case + " group frames", times=F)
    finally:
        g.close()


# ---- (h) the CLI ----------------------------------------------------------------------------------
def test_cli_warns_of_the_oracles_count(tmp_path):
    case, W, H, D = "colour_negative", 64, 48, 4
    want, counts, _ = mc.oracle(case, "dense", W, H, D)
    path = tmp_path / "scene.txt"
    path.write_text(mc.text(case))
    r = subprocess.run([os.path.join(PKG, "ray_hip"), "--width", str(W), "--height", str(H), "--depth", str(D),
                        str(path)], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert counts["negative"] > 0
    assert "warning: %d channels quantised below 0 were stored as 0" % counts["negative"] in r.stderr, r.stderr
    assert (tmp_path / "output_gpu.ppm").read_bytes() == p3(want, W, H)


# ---- (i) path queries -------------------------------------------------------------------------
@pytest.mark.parametrize("case", tuple(mc.PATH_CASES))
def test_paths_reflect_where_reflectivity_is_positive(gpu_renderer, case):
    """rt_trace_paths on the camera's rays: a vertex reflects where `reflectivity > 0` (main.cpp:43), so not
    at -0.5, -2, -1e-300, -0 or 0, and at 1e-300, 1.5 and 2.5; the levels traced are path_ref's, and the
    segments are the render's primary and reflection rays."""
    import rt_hip

    sc = _scene(case)
    gpu_renderer.upload(sc)
    W, H, D = mc.PATH_SHAPE
    rays = ray_ref.camera_rays(sc.camera(), W, H)
    o, d = rays[:, 0:3].copy(), rays[:, 3:6].copy()
    levels = path_ref.trace_paths(o, d, D, path_ref.SceneArrays(sc))
    verts, _, st = gpu_renderer.trace_paths(o, d, D)
    for k, lv in enumerate(levels):
        flags = np.where(lv["traced"], rt_hip.RT_VERTEX_TRACED
                         | np.where(lv["reflects"], rt_hip.RT_VERTEX_REFLECTS, 0), 0)
        assert np.array_equal(verts[k]["flags"], flags), (k, int((verts[k]["flags"] != flags).sum()))
        assert np.array_equal(verts[k]["sphere"], lv["sphere"]), k
    _, segments, hits, shadow = path_ref.counts(levels, path_ref.SceneArrays(sc))
    assert (st.rays, st.segments, st.hits, st.shadow_rays) == (W * H, segments, hits, shadow)
    _, rst = gpu_renderer.render(sc.camera(), W, H, D)
    assert st.segments == rst.rays_primary + rst.rays_reflect
    _, counts, _ = mc.oracle(case, "dense", W, H, D)
    assert (rst.rays_primary, rst.rays_shadow, rst.rays_reflect) == mc.ray_counts(counts)
    # the case does what its name says: a reflective sphere's hits reflect exactly where the rule allows
    refl = path_ref.SceneArrays(sc).refl
    lv0 = levels[0]
    hit = lv0["sphere"] >= 0
    assert np.array_equal(lv0["reflects"][hit], refl[lv0["sphere"][hit]] > 0)
    assert {1, 2, 3} <= set(lv0["sphere"][hit].tolist())  # A, B and C are all seen
