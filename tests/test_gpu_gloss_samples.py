"""GPU: the gloss table of the multi-sample entries (include/rt_hip.h, "samples with glossy reflections"):
rt_set_gloss_samples and every resolving radiance launch that reads it.

The yardstick (gloss_ref.device_chain) needs nothing of the feature: per sample the chain is run level by
level on a SECOND context -- rt_trace_paths (depth 1, surfaces) and rt_trace_radiance (depth 1, F64X3) --, the
reflection ray bent in numpy fp64 in between, the levels composited innermost first, and the samples
resolved by sample_ref.resolve.  Every comparison is of bits, and of the rays / segments / hits / shadow_rays
(and negative_clamped) counts.

The fixture is scenes/medium.txt seen from close by (its own camera, 28 units away, sees the metallic row
as a few pixels): a view in which every primary ray hits a sphere of roughness 0.2, one across two metallic
spheres and the sky, and the file's own sparse one.  Sphere 7 (the file's 0.05) is given roughness 0, so
that the fixture holds a mirror among rough spheres.  gloss_ref.host_chain counts on the CPU what each case
contains -- bent rays, refused perturbations, mirror spawns -- and the tests assert those counts.

Shapes as test_gpu_light_samples.py: W x 3 images, W a lane short of, at and past a wave and two waves."""
import contextlib
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import gloss_ref
import path_ref
import sample_ref
from conftest import PKG, scene_path
from test_gpu_lens import FOCUS, lens_fused, lens_rays
from test_gpu_light_samples import light_positions, sample_rays, upload_shifted
from test_gpu_samples import negative_channels, same_bits
from test_gpu_samples_async import F32X3, F64X3, GUARD, RGB8, _weights, fused, real_rows, same_records

pytestmark = pytest.mark.gpu

INVALID, NO_SCENE = 1, 5  # rt_status
FORMATS = (RGB8, F32X3, F64X3)
COUNTS = ("rays", "segments", "hits", "shadow_rays", "negative_clamped")
MIRROR_SPHERE = 7  # given roughness 0 in every fixture

CLOSE_UP = "camera -3 2 -17 -3 2 -20 40\n"   # every pixel hits sphere 6 (reflectivity 0.8, roughness 0.2)
MIXED = "camera -1.5 2 -17 -1.5 2 -20 60\n"  # spheres 6 and 7 (the mirror) and the sky between them
SPARSE = ""                                    # the file's own camera: under two thirds of the lanes hit
MEDIUM_FOCUS = 3.0                             # the lens forms: sharp at the metallic row of the close views


def counts(st):
    return {k: getattr(st, k) for k in COUNTS}


@functools.lru_cache(maxsize=None)
def _medium_text():
    with open(scene_path("medium")) as f:
        return f.read()


def fixture(view=CLOSE_UP, scale=1.0):
    """(scene, SceneArrays, roughness): medium.txt under `view`, the file's roughness column times `scale`
    with sphere 7 a mirror."""
    import rt_hip

    text = _medium_text() + view  # the last camera record wins
    sc = rt_hip.Scene.parse(text)
    rough = np.array(rt_hip.scene_roughness(text), np.float64) * scale
    assert rough.shape == (sc.num_spheres,) and rough[MIRROR_SPHERE] == 0.05 * scale
    rough[MIRROR_SPHERE] = 0.0
    return sc, path_ref.SceneArrays(sc), rough


def _patterns(S, B):
    import rt_hip

    return (rt_hip.grid_pattern(8)[:S], rt_hip.lens_pattern(8, 0.05)[:S],
            np.array(rt_hip.gloss_pattern(8, B), np.float64)[:S])


def coverage(sc, sa, rough, table, rays, D):
    """What the case contains, from the CPU alone: (bent-or-refused spawns, refused, mirror spawns)."""
    S = len(table)
    tot = np.zeros(3, np.int64)
    for s in range(S):
        tot += gloss_ref.coverage(gloss_ref.host_chain(rays[s::S, 0:3], rays[s::S, 3:6], D, sa, rough, table[s]))
    return tuple(int(x) for x in tot)


def yardstick(yard, sc, sa, rough, table, rays, D, lights=None):
    """rays: host records [npix * S, 8], a pixel's samples consecutive.  (colours [npix, S, 3], the counts
    summed, glossy [npix]: some sample's chain spawned off a sphere of roughness != 0 inside the table).
    lights = (a second context, a scene of its own to write into, the light table): sample s's radiance
    then runs there, under that sample's moved lights."""
    S = len(table)
    yard.upload(sc)
    cols = np.zeros((rays.shape[0] // S, S, 3))
    cnt = dict.fromkeys(COUNTS[:4], 0)
    glossy = np.zeros(rays.shape[0] // S, bool)
    base = light_positions(sc)
    for s in range(S):
        rad = yard
        if lights is not None:
            rad, lsc, ltab = lights
            upload_shifted(rad, lsc, base, ltab[s])
        c, n, info = gloss_ref.device_chain(yard, rad, sa, rough, table[s], rays[s::S, 0:3], rays[s::S, 3:6], D)
        cols[:, s] = c
        glossy |= info["glossy"]
        for k in cnt:
            cnt[k] += n[k]
    return cols, cnt, glossy


def expected(cols, cnt, weights, fmt):
    px = sample_ref.resolve(cols, weights)
    with np.errstate(all="ignore"):
        rec = px if fmt == F64X3 else px.astype(np.float32) if fmt == F32X3 else path_ref.quantize(px)
    return rec, dict(cnt, negative_clamped=negative_channels(px) if fmt == RGB8 else 0)


@contextlib.contextmanager
def table_set(r, rough, table):
    """The table on the (shared) context, cleared again behind the test."""
    r.set_gloss_samples(rough, table)
    try:
        yield
    finally:
        r.set_gloss_samples(None, None)


def launch(r, form, cam, W, H, D, pattern, lens, weights=None, rows=None, fmt=RGB8):
    if form == "lens":
        return lens_fused(r, cam, W, H, D, pattern, lens, MEDIUM_FOCUS, weights, rows, fmt)
    return fused(r, cam, W, H, D, pattern, weights, rows, fmt)


def form_rays(yard, form, cam, W, H, pattern, lens):
    if form == "lens":
        return lens_rays(yard, cam, W, H, pattern, lens, MEDIUM_FOCUS)[1]
    return sample_rays(yard, cam, W, H, pattern)


def check_forms(r, yard, fix, table, W, H, D, pattern, lens, weight_sets=(None,), forms=("pinhole", "lens"),
                fmts=FORMATS, what=""):
    """The fused pinhole and lens launches under `table` against the yardstick: records and counts.  Returns
    per form (the F64X3 records of the first weight set, its stats, the pinhole rays' coverage)."""
    sc, sa, rough = fix
    cam = sc.camera()
    r.upload(sc)
    out = {}
    for form in forms:
        rays = form_rays(yard, form, cam, W, H, pattern, lens)
        cols, cnt, _ = yardstick(yard, sc, sa, rough, table, rays, D)
        cover = coverage(sc, sa, rough, table, rays, D)
        with table_set(r, rough, table):
            for wi, w in enumerate(weight_sets):
                for fmt in fmts:
                    want, want_cnt = expected(cols, cnt, w, fmt)
                    got, st = launch(r, form, cam, W, H, D, pattern, lens, w, None, fmt)
                    assert got.dtype == want.dtype and got.shape == want.shape
                    assert same_records(got, want, fmt), (what, form, wi, fmt)
                    assert counts(st) == want_cnt, (what, form, wi, fmt)
                    if wi == 0 and fmt == fmts[-1]:
                        out[form] = (got, st, cover)
    return out


@pytest.fixture(scope="module")
def yard():
    """The yardstick's own context: it never holds a table."""
    import rt_hip

    r = rt_hip.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def yard2():
    """The context of the yardstick's radiance under a light table: it holds the moved lights."""
    import rt_hip

    r = rt_hip.Renderer(0)
    yield r
    r.close()


# ---- 1. bit equality with the yardstick ------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 63, 64, 65, 129])
def test_equals_the_level_by_level_chain(gpu_renderer, yard, W):
    D = 4
    fix = fixture(CLOSE_UP)
    for S in (1, 4):
        for B in (1, D - 1):  # B = 1: the bounces beyond the table are mirrors
            pattern, lens, table = _patterns(S, B)
            got = check_forms(gpu_renderer, yard, fix, table, W, 3, D, pattern, lens, (None, _weights(S)),
                              what=(W, S, B))
            glossy, refused, mirror = got["pinhole"][2]
            if W > 1:  # W - 1 = 0 gives NaN directions, which hit nothing: sky only
                assert glossy >= W * 3 * S  # every primary ray leaves a rough sphere
                assert B == 3 or mirror > 0  # the levels beyond the table
                assert B == 1 or refused > 0  # a perturbation through the surface, at a grazing second bounce
                assert S == 1 or mirror > 0  # B = 3: sphere 7 in a reflection
            else:
                assert (glossy, refused, mirror) == (0, 0, 0)


def test_equals_the_chain_at_64_samples(gpu_renderer, yard):
    pattern, lens, table = _patterns(64, 3)
    got = check_forms(gpu_renderer, yard, fixture(CLOSE_UP), table, 65, 3, 4, pattern, lens, (None, _weights(64)),
                      what="S = 64")
    glossy, refused, mirror = got["pinhole"][2]
    assert glossy > 0 and refused > 0 and mirror > 0


@pytest.mark.parametrize("D", [1, 2, 4])
def test_depths(gpu_renderer, yard, D):
    """Depth 1 spawns nothing (the table is set and never read), depth 2 bends its one bounce, depth 4 all
    three or the first only."""
    for B in sorted({1, max(1, D - 1)}):
        pattern, lens, table = _patterns(4, B)
        got = check_forms(gpu_renderer, yard, fixture(MIXED, 2.5), table, 65, 3, D, pattern, lens, (None,),
                          fmts=(RGB8, F64X3), what=(D, B))
        glossy, refused, mirror = got["pinhole"][2]
        assert (glossy > 0) == (D > 1) and (mirror > 0) == (D > 1)


# ---- 2. the views: 64 hit lanes, two spheres and the sky, the sparse file view ---------------------------
@pytest.mark.parametrize("name", ["close_up", "mixed", "sparse"])
def test_views_and_what_they_contain(gpu_renderer, yard, name):
    view, scale = {"close_up": (CLOSE_UP, 1.0), "mixed": (MIXED, 2.5), "sparse": (SPARSE, 2.5)}[name]
    W, H, D, S = 64, 3, 4, 4
    pattern, lens, table = _patterns(S, 3)
    got = check_forms(gpu_renderer, yard, fixture(view, scale), table, W, H, D, pattern, lens, (None,), what=name)
    rec, st, (glossy, refused, mirror) = got["pinhole"]
    print(name, "glossy %d refused %d mirror %d hits %d" % (glossy, refused, mirror, st.hits))
    assert glossy > 0  # reflective hits with roughness > 0
    if name == "close_up":
        assert st.hits >= W * H * S  # every primary ray hits: 64 hit lanes
    if name == "mixed":
        assert refused > 0 and mirror > 0  # refused perturbations, and the sphere of roughness 0
    if name == "sparse":
        assert 0 < st.hits and refused > 0


# ---- 3. table entries and roughness that are not finite ---------------------------------------------------
def test_entries_that_are_not_finite(gpu_renderer, yard):
    sc, sa, rough = fixture(MIXED, 2.5)
    pattern, lens, table = _patterns(4, 3)
    plain = check_forms(gpu_renderer, yard, (sc, sa, rough), table, 65, 3, 4, pattern, None, forms=("pinhole",),
                        fmts=(F64X3,))
    # a NaN in every entry of sample 2 and a NaN roughness on sphere 6: each is a mirror there (the `use`
    # comparison is false for a NaN), never an error
    bad = table.copy()
    bad[2, :, 1] = np.nan
    rough_nan = rough.copy()
    rough_nan[6] = np.nan
    for rg, tb, what in ((rough, bad, "table"), (rough_nan, table, "roughness")):
        got = check_forms(gpu_renderer, yard, (sc, sa, rg), tb, 65, 3, 4, pattern, lens, (None, _weights(4)),
                          what=what)
        assert np.isfinite(got["pinhole"][0]).all()
        assert not same_bits(got["pinhole"][0], plain["pinhole"][0]).all()
    # sample 2 all NaN is sample 2 without a table: the mirror
    cam = sc.camera()
    rays = sample_rays(yard, cam, 65, 3, pattern)
    cols_bad, _, _ = yardstick(yard, sc, sa, rough, bad, rays, 4)
    cols_none, _, _ = yardstick(yard, sc, sa, np.zeros_like(rough), table, rays, 4)
    assert same_bits(cols_bad[:, 2], cols_none[:, 2]).all() and not same_bits(cols_bad[:, 1], cols_none[:, 1]).all()
    # infinities follow the same rule as written: whatever the comparison makes of them, in bits
    inf = table.copy()
    inf[1, 0] = (np.inf, 0.0, -np.inf)
    inf[3, 1, 2] = -np.inf
    rough_inf = rough.copy()
    rough_inf[6] = np.inf
    for rg, tb, what in ((rough, inf, "inf table"), (rough_inf, table, "inf roughness")):
        check_forms(gpu_renderer, yard, (sc, sa, rg), tb, 65, 3, 4, pattern, None, (None,), ("pinhole",), what=what)


# ---- 4. the caller's rays --------------------------------------------------------------------------------
def test_resolve_of_the_callers_rays_honours_the_table(gpu_renderer, yard):
    import torch

    sc, sa, rough = fixture(MIXED, 2.5)
    S, npix, D = 4, 150, 4
    rng = np.random.default_rng(11)
    o = np.array([-1.5, 2.0, -17.0]) + rng.uniform(-0.2, 0.2, (npix * S, 3))
    d = np.array([0.0, 0.0, -3.0]) + rng.uniform(-1.5, 1.5, (npix * S, 3))  # any length
    rays = np.zeros((npix * S, 8))
    rays[:, 0:3], rays[:, 3:6] = o, d
    _, _, table = _patterns(S, 2)
    cols, cnt, glossy = yardstick(yard, sc, sa, rough, table, rays, D)
    assert glossy.any() and coverage(sc, sa, rough, table, rays, D)[1] > 0
    gpu_renderer.upload(sc)
    plain, _ = gpu_renderer.trace_radiance_resolve(o, d, S, D, None, F64X3)
    with table_set(gpu_renderer, rough, table):
        for w in (None, _weights(S)):
            for fmt in FORMATS:
                want, want_cnt = expected(cols, cnt, w, fmt)
                got, st = gpu_renderer.trace_radiance_resolve(o, d, S, D, w, fmt)
                assert same_records(got, want, fmt) and counts(st) == want_cnt, fmt
        # the _async entry itself, device memory
        dev_rays = torch.from_numpy(rays).to("cuda:0")
        out = torch.zeros((npix * 24 + 16,), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        gpu_renderer.trace_radiance_resolve_device(dev_rays.data_ptr(), npix, S, D, F64X3, out.data_ptr())
        gpu_renderer.radiance_stats()
        want, _ = expected(cols, cnt, None, F64X3)
        assert same_bits(out.cpu().numpy()[:npix * 24].view(np.float64).reshape(npix, 3), want).all()
    assert not same_bits(plain, want).all()  # and the table is what made them so


# ---- 5. the synchronous chunked form ---------------------------------------------------------------------
def test_render_samples_honours_the_table(gpu_renderer):
    sc, _, rough = fixture(MIXED, 2.5)
    cam = sc.camera()
    gpu_renderer.upload(sc)
    W, H, D, S = 37, 21, 4, 4
    pattern, _, table = _patterns(S, 3)
    plain, _ = fused(gpu_renderer, cam, W, H, D, pattern)
    with table_set(gpu_renderer, rough, table):
        for w in (None, _weights(S)):
            for fmt in FORMATS:
                want, st0 = fused(gpu_renderer, cam, W, H, D, pattern, w, None, fmt)
                got, st = gpu_renderer.render_samples(cam, W, H, D, pattern, w, None, fmt,
                                                      max_ray_bytes=W * S * 64)  # one row per chunk
                assert got.tobytes() == want.tobytes(), fmt
                assert counts(st) == counts(st0)
        assert want.shape == (W * H, 3)
        assert fused(gpu_renderer, cam, W, H, D, pattern)[0].tobytes() != plain.tobytes()
    sharp, _ = gpu_renderer.render_samples(cam, W, H, D, pattern)
    assert sharp.tobytes() == plain.tobytes()  # cleared: the chunked form follows


# ---- 6. a second grid-stride trip ------------------------------------------------------------------------
def test_second_trip_of_the_stack_bounded_grid(gpu_renderer, yard):
    """Depth 64 bounds the grid at 2,080 waves (133,120 lanes): 365 x 365 pixels of the two-mirror scene
    take a second trip, in which a lane's stack slots are reused across trips and samples.  One sphere is
    rough, the other a mirror; the table covers every bounce."""
    import rt_hip
    from test_gpu_radiance import MIRRORS_09

    W = H = 365
    D = rt_hip.RT_MAX_DEPTH
    assert W * H > 2080 * 64
    sc = rt_hip.Scene.parse(MIRRORS_09)
    fix = (sc, path_ref.SceneArrays(sc), np.array([0.02, 0.0]))
    pattern = rt_hip.grid_pattern(2)[:2]
    table = np.array(rt_hip.gloss_pattern(2, rt_hip.RT_MAX_GLOSS_BOUNCES), np.float64)[:2]
    got = check_forms(gpu_renderer, yard, fix, table, W, H, D, pattern, None, (None,), ("pinhole",), (RGB8, F64X3),
                      what="mirrors")
    st = got["pinhole"][1]
    assert st.rays == 2 * W * H and st.segments > 2 * st.rays


# ---- 7. with the light table set as well -----------------------------------------------------------------
def test_composes_with_the_light_table(gpu_renderer, yard, yard2):
    import rt_hip

    sc, sa, rough = fixture(MIXED, 2.5)
    lsc = fixture(MIXED)[0]  # the second context's scene: its lights are overwritten per sample
    cam = sc.camera()
    W, H, D, S = 65, 3, 4, 4
    pattern, lens, table = _patterns(S, 3)
    ltab = rt_hip.light_pattern(8, 1.5, sc.num_lights)[:S]
    gpu_renderer.upload(sc)
    try:
        for form in ("pinhole", "lens"):
            rays = form_rays(yard, form, cam, W, H, pattern, lens)
            cols, cnt, _ = yardstick(yard, sc, sa, rough, table, rays, D, (yard2, lsc, ltab))
            only_gloss, _, _ = yardstick(yard, sc, sa, rough, table, rays, D)
            assert not same_bits(cols, only_gloss).all()  # the moved lights are seen
            gpu_renderer.set_light_samples(ltab)
            gpu_renderer.set_gloss_samples(rough, table)
            for w in (None, _weights(S)):
                for fmt in FORMATS:
                    want, want_cnt = expected(cols, cnt, w, fmt)
                    got, st = launch(gpu_renderer, form, cam, W, H, D, pattern, lens, w, None, fmt)
                    assert same_records(got, want, fmt) and counts(st) == want_cnt, (form, fmt)
            # the light table alone again: the gloss table goes, the other stays
            gpu_renderer.set_gloss_samples(None, None)
            lights_only, _ = launch(gpu_renderer, form, cam, W, H, D, pattern, lens, None, None, F64X3)
            assert not same_bits(lights_only, expected(cols, cnt, None, F64X3)[0]).all()
    finally:
        gpu_renderer.set_gloss_samples(None, None)
        gpu_renderer.set_light_samples(None)


# ---- 8. tables that bend nothing, a cleared table ---------------------------------------------------------
def test_tables_that_bend_nothing_write_the_bytes_of_no_table(gpu_renderer):
    import rt_hip

    sc, _, rough = fixture(MIXED, 2.5)
    cam = sc.camera()
    gpu_renderer.upload(sc)
    W, H, D, S = 37, 21, 4, 4
    pattern, lens, table = _patterns(S, 3)

    def both(fmt, p=pattern, ln=lens):
        a, sa_ = fused(gpu_renderer, cam, W, H, D, p, None, None, fmt)
        b, sb = lens_fused(gpu_renderer, cam, W, H, D, p, ln, MEDIUM_FOCUS, None, None, fmt)
        return a.tobytes(), b.tobytes(), counts(sa_), counts(sb)

    none = {fmt: both(fmt) for fmt in FORMATS}
    try:
        gpu_renderer.set_gloss_samples(rough, np.zeros((S, 3, 3)))  # rd + 0 * roughness
        for fmt in FORMATS:
            assert both(fmt) == none[fmt], fmt
        gpu_renderer.set_gloss_samples(np.zeros_like(rough), table)  # roughness 0 everywhere: mirrors
        for fmt in FORMATS:
            assert both(fmt) == none[fmt], fmt
        gpu_renderer.set_gloss_samples(rough, table)
        assert both(RGB8)[:2] != none[RGB8][:2]
        gpu_renderer.set_gloss_samples(None, None)
        for fmt in FORMATS:
            assert both(fmt) == none[fmt], fmt
        # rt_upload_scene clears the table: another S is accepted and writes the bytes of no table
        gpu_renderer.set_gloss_samples(rough, table)
        gpu_renderer.upload(sc)
        for fmt in FORMATS:
            assert both(fmt) == none[fmt], fmt
        p9, l9 = rt_hip.grid_pattern(3), rt_hip.lens_pattern(3, 0.05)
        nine = both(RGB8, p9, l9)
        gpu_renderer.set_gloss_samples(rough, table)
        gpu_renderer.upload(sc)
        assert both(RGB8, p9, l9) == nine
    finally:
        gpu_renderer.set_gloss_samples(None, None)


# ---- 9. a table changes the image, and only where a chain leaves a rough sphere ---------------------------
def test_a_table_changes_only_pixels_that_leave_a_rough_sphere(gpu_renderer, yard):
    sc, sa, rough = fixture(MIXED, 2.5)
    cam = sc.camera()
    W, H, D, S = 97, 31, 4, 4
    pattern, _, table = _patterns(S, 3)
    rays = sample_rays(yard, cam, W, H, pattern)
    _, _, glossy = yardstick(yard, sc, sa, rough, table, rays, D)
    gpu_renderer.upload(sc)
    sharp, _ = fused(gpu_renderer, cam, W, H, D, pattern, None, None, F64X3)
    with table_set(gpu_renderer, rough, table):
        soft, st = fused(gpu_renderer, cam, W, H, D, pattern, None, None, F64X3)
    differ = ~same_bits(sharp, soft).all(axis=1)
    print("%d of %d pixels differ, %d leave a rough sphere" % (differ.sum(), W * H, glossy.sum()))
    assert differ.sum() > W * H // 20 and st.rays == S * W * H
    assert (~glossy).sum() > W * H // 20 and not differ[~glossy].any()


# ---- 10. shards, asynchronous calls, and the context's other reports -------------------------------------
ROWS_W, ROWS_H, ROWS_D = 37, 21, 4


def test_shards_are_slices_of_the_frame(gpu_renderer):
    import rt_hip

    sc, _, rough = fixture(MIXED, 2.5)
    cam = sc.camera()
    gpu_renderer.upload(sc)
    W, H, D = ROWS_W, ROWS_H, ROWS_D
    pattern, lens = rt_hip.grid_pattern(3), rt_hip.lens_pattern(3, 0.05)
    table = rt_hip.gloss_pattern(3, 2)
    with table_set(gpu_renderer, rough, table):
        for form in ("pinhole", "lens"):
            for fmt in FORMATS:
                full, stf = launch(gpu_renderer, form, cam, W, H, D, pattern, lens, None, None, fmt)
                full = full.reshape(H, W, 3)
                total = dict.fromkeys(COUNTS, 0)
                for k in range(3):
                    rows = rt_hip.rows_for_shard(H, 8, k, 3)
                    real = real_rows(rows, H)
                    assert (real < rows.count) == (k == 2)  # H is no multiple of the band
                    ys = [(i // 8) * 8 * 3 + k * 8 + i % 8 for i in range(real)]
                    rec, st = launch(gpu_renderer, form, cam, W, H, D, pattern, lens, None, rows, fmt)
                    rec = rec.reshape(rows.count, W, 3)
                    assert same_records(rec[:real], full[ys], fmt), (form, fmt, k)
                    assert (rec[real:].view(np.uint8) == 0).all()  # padding rows: zero bytes
                    assert st.rays == 9 * W * real
                    for key in COUNTS:
                        total[key] += getattr(st, key)
                assert total == counts(stf), (form, fmt)


def test_two_async_calls_and_nothing_else_moves():
    import rt_hip
    import torch

    sc, _, rough = fixture(MIXED, 2.5)
    cam = sc.camera()
    W, H, D = ROWS_W, ROWS_H, ROWS_D
    n = W * H
    pattern, lens, table = rt_hip.grid_pattern(2), rt_hip.lens_pattern(2, 0.05), rt_hip.gloss_pattern(2, 3)
    r = rt_hip.Renderer(0)
    side = torch.cuda.Stream()
    try:
        r.upload(sc)
        r.set_gloss_samples(rough, table)
        want_a, _ = fused(r, cam, W, H, D, pattern)  # the synchronous results
        want_b, st_b = lens_fused(r, cam, W, H, D, pattern, lens, MEDIUM_FOCUS, _weights(4), None, F64X3)
        host, _ = r.render_lens_samples(cam, W, H, D, pattern, lens, MEDIUM_FOCUS, _weights(4), None, F64X3)
        assert same_bits(host, want_b).all()
        r.set_gloss_samples(None, None)
        assert fused(r, cam, W, H, D, pattern)[0].tobytes() != want_a.tobytes()
        # what the context's other launches report, before
        r.render(cam, W, H, D)
        rays1 = torch.zeros((n, 8), dtype=torch.float64, device="cuda:0")
        r.camera_rays(cam, W, H, None, rays1.data_ptr())
        hits = torch.zeros((64, 2), dtype=torch.float64, device="cuda:0")
        r.trace_rays_device(rays1.data_ptr(), 64, hits.data_ptr())
        verts = torch.zeros((D * 64 * 32,), dtype=torch.uint8, device="cuda:0")
        r.trace_paths_device(rays1.data_ptr(), 64, D, verts.data_ptr())
        r.kernel_times()

        def reports():
            i = r.info()
            return (r.stats().as_dict(), r.trace_stats().as_dict(), r.path_stats().as_dict(), i.launches,
                    i.scratch_bytes)

        before = reports()
        r.set_gloss_samples(rough, table)
        a = torch.full((n * 3 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        b = torch.full((n * 24 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        r.set_stream(side.cuda_stream)
        r.render_samples_async(cam, W, H, D, pattern, a.data_ptr())
        r.render_lens_samples_async(cam, W, H, D, pattern, lens, MEDIUM_FOCUS, b.data_ptr(), _weights(4), None, F64X3)
        side.synchronize()  # the one wait
        ha, hb = a.cpu().numpy(), b.cpu().numpy()
        assert ha[:n * 3].tobytes() == want_a.tobytes() and (ha[n * 3:] == 0xA5).all()
        assert same_bits(hb[:n * 24].view(np.float64).reshape(n, 3), want_b).all() and (hb[n * 24:] == 0xA5).all()
        assert counts(r.radiance_stats()) == counts(st_b)  # the most recent launch: the second call's
        after = reports()
        for got_d, want_d in zip(after[:3], before[:3]):
            # the same launch's events read a second time: the runtime's float differs in its last digits
            assert got_d.pop("kernel_ms") == pytest.approx(want_d.pop("kernel_ms"), rel=1e-4)
        assert after == before
        assert r.kernel_times() == []
    finally:
        r.set_stream(None)
        r.close()


# ---- 11. the calls without a sample index ----------------------------------------------------------------
def test_unaffected_calls(gpu_renderer):
    import rt_hip
    import torch

    sc, _, rough = fixture(MIXED, 2.5)
    cam = sc.camera()
    gpu_renderer.upload(sc)
    W, H, D = ROWS_W, ROWS_H, ROWS_D
    rays = sample_rays(gpu_renderer, cam, W, H, [(0.0, 0.0)])
    o, d = rays[:, 0:3], rays[:, 3:6]

    def calls():
        rad, sr = gpu_renderer.trace_radiance(o, d, D)
        verts, _, sp = gpu_renderer.trace_paths(o, d, D)
        img, si = gpu_renderer.render(cam, W, H, D)
        fb = torch.zeros((W * H * 3 + 16,), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        gpu_renderer.render_tile(cam, W, H, D, 8, 8, 16, 8, RGB8, fb.data_ptr())
        tile = gpu_renderer.stats()
        return (rad.tobytes(), verts.tobytes(), bytes(img), fb.cpu().numpy().tobytes(), counts(sr),
                sp.as_dict()["segments"], si.rays, tile.rays)

    want = calls()
    with table_set(gpu_renderer, rough, rt_hip.gloss_pattern(1, 3)):  # one sample: rt_trace_radiance's own count
        assert calls() == want
    with table_set(gpu_renderer, rough, rt_hip.gloss_pattern(2, 3)):
        assert calls() == want


# ---- 12. errors ------------------------------------------------------------------------------------------
def test_errors():
    import rt_hip
    import torch

    r = rt_hip.Renderer(0)
    g = rt_hip.Group([0, 0])
    L = r._L
    try:
        W = H = 4
        out = torch.zeros((W * H * 24 + 16,), dtype=torch.uint8, device="cuda:0")
        rays = torch.zeros((W * H * 9 * 8 + 8,), dtype=torch.float64, device="cuda:0")
        host = np.zeros((W * H, 3), np.float64)
        op, rp = C.c_void_p(out.data_ptr()), C.c_void_p(rays.data_ptr())
        off, lens = (C.c_double * 130)(), (C.c_double * 130)()
        tab = (C.c_double * (65 * 64 * 3))()
        rg = (C.c_double * 64)()
        st = rt_hip.rt_radiance_stats()
        assert L.rt_set_gloss_samples(None, rg, tab, 4, 1) == INVALID  # a NULL ctx
        assert L.rt_group_set_gloss_samples(None, rg, tab, 4, 1) == INVALID
        assert L.rt_set_gloss_samples(r.handle, rg, tab, 4, 1) == NO_SCENE
        assert L.rt_set_gloss_samples(r.handle, None, None, 0, 0) == NO_SCENE
        assert L.rt_set_gloss_samples(r.handle, rg, tab, 0, 1) == INVALID  # the arguments first
        assert L.rt_set_gloss_samples(r.handle, None, tab, 4, 1) == INVALID
        assert L.rt_group_set_gloss_samples(g._grp, rg, tab, 4, 1) == NO_SCENE
        assert b"no scene" in L.rt_group_last_error(g._grp)
        sc = rt_hip.Scene.load(scene_path("simple"))
        assert sc.num_lights == 2 and sc.num_spheres <= 64
        rough = [0.5] * sc.num_spheres
        cam = sc.camera()
        r.upload(sc)
        g.upload(sc)
        pattern = rt_hip.grid_pattern(2)
        table = rt_hip.gloss_pattern(2, 2)
        none = fused(r, cam, W, H, 3, pattern)[0].tobytes()
        r.set_gloss_samples(rough, table)
        g.set_gloss_samples(rough, table)
        soft = fused(r, cam, W, H, 3, pattern)[0].tobytes()
        assert soft != none
        for S in (0, 65, -1):
            assert L.rt_set_gloss_samples(r.handle, rg, tab, S, 1) == INVALID
            assert L.rt_group_set_gloss_samples(g._grp, rg, tab, S, 1) == INVALID
            assert b"RT_MAX_SAMPLES" in L.rt_group_last_error(g._grp)
        for B in (0, 64, -1):
            assert L.rt_set_gloss_samples(r.handle, rg, tab, 4, B) == INVALID
            assert L.rt_group_set_gloss_samples(g._grp, rg, tab, 4, B) == INVALID
            assert b"RT_MAX_GLOSS_BOUNCES" in L.rt_group_last_error(g._grp)
        assert L.rt_set_gloss_samples(r.handle, None, tab, 4, 1) == INVALID  # a table without the roughness
        assert L.rt_group_set_gloss_samples(g._grp, None, tab, 4, 1) == INVALID
        assert b"roughness" in L.rt_group_last_error(g._grp)
        assert L.rt_set_gloss_samples(r.handle, rg, tab, 64, 63) == 0  # the largest table
        r.set_gloss_samples(rough, table)
        with pytest.raises(ValueError):
            r.set_gloss_samples(rough + [0.5], table)  # one roughness too many for the scene
        with pytest.raises(ValueError):
            r.set_gloss_samples(rough, [[(0.0, 0.0, 0.0)], [(0.0, 0.0, 0.0)] * 2])  # ragged
        assert fused(r, cam, W, H, 3, pattern)[0].tobytes() == soft  # the previous table is in force
        # a launch whose samples differ from the table's 4, on every entry that reads it
        cp = C.byref(cam)
        mismatch = [
            lambda: L.rt_trace_radiance_resolve_async(r.handle, rp, W * H, 9, None, 3, RGB8, op),
            lambda: L.rt_trace_radiance_resolve(r.handle, rp, W * H, 9, None, 3, RGB8, op, 1, C.byref(st)),
            lambda: L.rt_trace_radiance_resolve_async(r.handle, rp, 0, 9, None, 3, RGB8, op),  # also without rays
            lambda: L.rt_render_samples(r.handle, cp, W, H, 3, None, off, 9, None, RGB8, op, 1, 0, C.byref(st)),
            lambda: L.rt_render_samples_async(r.handle, cp, W, H, 3, None, off, 9, None, RGB8, op),
            lambda: L.rt_render_samples_async(r.handle, cp, W, H, 3, None, off, 1, None, RGB8, op),
            lambda: L.rt_render_lens_samples_async(r.handle, cp, W, H, 3, None, off, lens, 2.0, 9, None, RGB8, op),
            lambda: L.rt_render_lens_samples(r.handle, cp, W, H, 3, None, off, lens, 2.0, 9, None, RGB8, op, 1,
                                             C.byref(st)),
        ]
        for i, f in enumerate(mismatch):
            assert f() == INVALID, i
        hp = C.c_void_p(host.ctypes.data)
        group_calls = (
            ("rt_group_render_samples",
             lambda: L.rt_group_render_samples(g._grp, cp, W, H, 3, off, 9, None, F64X3, hp, 0, C.byref(st))),
            ("rt_group_render_lens_samples",
             lambda: L.rt_group_render_lens_samples(g._grp, cp, W, H, 3, off, lens, 2.0, 9, None, F64X3, hp, 0,
                                                    C.byref(st))))
        for name, f in group_calls:
            assert f() == INVALID
            err = L.rt_group_last_error(g._grp).decode()
            assert name in err and "gloss table" in err and "9" in err and "4" in err, err
        # two tables: each must match, whichever is the odd one
        nine_l, four_l = rt_hip.light_pattern(3, 0.5, 2), rt_hip.light_pattern(2, 0.5, 2)
        nine_g = rt_hip.gloss_pattern(3, 2)
        p9 = rt_hip.grid_pattern(3)
        for lt, gt, word in ((nine_l, table, "gloss table"), (four_l, nine_g, "light table")):
            r.set_light_samples(lt)
            r.set_gloss_samples(rough, gt)
            g.set_light_samples(lt)
            g.set_gloss_samples(rough, gt)
            assert L.rt_render_samples_async(r.handle, cp, W, H, 3, None, off, 9, None, RGB8, op) == INVALID
            assert L.rt_render_samples_async(r.handle, cp, W, H, 3, None, off, 4, None, RGB8, op) == INVALID
            assert group_calls[0][1]() == INVALID  # 9 samples
            assert word in L.rt_group_last_error(g._grp).decode()
        r.set_light_samples(nine_l)
        r.set_gloss_samples(rough, nine_g)
        fused(r, cam, W, H, 3, p9)  # both at 9: accepted
        r.set_light_samples(None)
        g.set_light_samples(None)
        r.set_gloss_samples(rough, table)
        g.set_gloss_samples(rough, table)
        assert (out.cpu().numpy() == 0).all() and (host == 0).all()  # nothing was written
        # the calls without a sample index take any count; the generator reads no table
        assert L.rt_camera_sample_rays(r.handle, cp, W, H, None, off, 9, rp) == 0
        assert L.rt_trace_radiance_async(r.handle, rp, W * H, 3, RGB8, op) == 0
        assert r.radiance_stats().rays == W * H
        assert fused(r, cam, W, H, 3, pattern)[0].tobytes() == soft
        got, _ = g.render_samples(cam, W, H, 3, pattern)
        assert got.tobytes() == soft
        # a scene without spheres takes the call and renders as without a table; the count is still checked
        empty = rt_hip.Scene.parse("light 0 5 0 1 1 1 1\nambient 0.3 0.3 0.3\ncamera 0 0 0 0 0 -1 60\n")
        assert empty.num_spheres == 0
        r.upload(empty)
        want = fused(r, empty.camera(), W, H, 3, pattern)[0].tobytes()
        r.set_gloss_samples([], table)
        assert fused(r, empty.camera(), W, H, 3, pattern)[0].tobytes() == want
        assert L.rt_render_samples_async(r.handle, C.byref(empty.camera()), W, H, 3, None, off, 9, None, RGB8,
                                         op) == INVALID
    finally:
        g.close()
        r.close()


# ---- 13. the check and tuning builds ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _variant_reference():
    """The mixed view at W = 65 by the yardstick on the product library, once."""
    import rt_hip

    S, W, H, D = 4, 65, 3, 4
    pattern, lens, table = _patterns(S, 3)
    sc, sa, rough = fixture(MIXED, 2.5)
    r = rt_hip.Renderer(0)
    try:
        ref = {form: yardstick(r, sc, sa, rough, table, form_rays(r, form, sc.camera(), W, H, pattern, lens), D)[:2]
               for form in ("pinhole", "lens")}
    finally:
        r.close()
    return (W, H, D, pattern, lens, table, rough), ref


@pytest.mark.parametrize("variant", ["check", "tuning"])
def test_variant_builds(variant):
    import rt_hip

    (W, H, D, pattern, lens, table, rough), ref = _variant_reference()
    r = rt_hip.Renderer(0, variant=variant)
    try:
        sc = fixture(MIXED, 2.5)[0]
        r.upload(sc)
        r.set_gloss_samples(rough, table)
        for form, (cols, cnt) in ref.items():
            for w in (None, _weights(4)):
                for fmt in FORMATS:
                    want, want_cnt = expected(cols, cnt, w, fmt)
                    got, st = launch(r, form, sc.camera(), W, H, D, pattern, lens, w, None, fmt)
                    assert same_records(got, want, fmt) and counts(st) == want_cnt, (form, fmt)
        r.stats()  # raises on RT_ERR_CHECK
    finally:
        r.close()


# ---- the CLI ---------------------------------------------------------------------------------------------
def test_cli_gloss(tmp_path):
    """One run (a process start costs seconds): --gloss with --gloss-bounces, --aperture and --light-radius
    through the device group, the path on which ray_hip restates gloss_pattern, reads the file's roughness
    column and calls rt_group_set_gloss_samples."""
    import rt_hip

    W, H, D, N = 37, 21, 4, 3
    scene = scene_path("medium")
    sc = rt_hip.Scene.load(scene)
    pattern, lens = rt_hip.grid_pattern(N), rt_hip.lens_pattern(N, 0.2)
    focus = 28.0
    r = rt_hip.Renderer(0)
    try:
        r.upload(sc)
        r.set_light_samples(rt_hip.light_pattern(N, 0.75, sc.num_lights))
        sharp, _ = r.render_lens_samples(sc.camera(), W, H, D, pattern, lens, focus)
        r.set_gloss_samples([x * 2.5 for x in rt_hip.scene_roughness(scene)], rt_hip.gloss_pattern(N, 2))
        soft, _ = r.render_lens_samples(sc.camera(), W, H, D, pattern, lens, focus)
    finally:
        r.close()
    assert soft.tobytes() != sharp.tobytes()
    p = subprocess.run([os.path.join(PKG, "ray_hip"), "--supersample", str(N), "--gloss", "2.5", "--gloss-bounces", "2",
                        "--light-radius", "0.75", "--aperture", "0.2", "--focus", str(focus), "--sample-devices", "0,0",
                        "--width", str(W), "--height", str(H), "--depth", str(D), "--p6", "--out", "out.ppm", scene],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "GPU rendering time:" in p.stdout, p.stdout + p.stderr
    assert open(tmp_path / "out.ppm", "rb").read() == b"P6\n%d %d\n255\n" % (W, H) + soft.tobytes()
