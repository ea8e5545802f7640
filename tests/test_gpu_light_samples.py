"""GPU: the light table of the multi-sample entries (include/rt_hip.h, "samples under area lights"):
rt_set_light_samples and every resolving radiance launch that reads it.

The yardstick needs nothing of the feature:

  1. scene_s: the scene with, for every light, the shifted position written into the scene's own light
     array -- numpy fp64 adds of the uploaded position and the table's offset;
  2. on a SECOND context scene_s is uploaded and rt_trace_radiance (RT_FB_F64X3) traces the sample-s rays
     (stride S) of rt_camera_sample_rays / rt_camera_lens_rays, or of the caller;
  3. sample_ref.resolve and the quantisers of path_ref / test_gpu_samples resolve them on the host.

For S samples that is S uploads of a small scene.  Every comparison is of bits.

Shapes as test_gpu_lens.py: the smallest at which the packed RGB8 store, a partial wave, more than one
wave and the grid-stride loop's second trip can each go wrong; H = 3 because H - 1 divides."""
import contextlib
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import material_cases as mc
import path_ref
import sample_ref
from conftest import PKG, manifest, scene_path
from test_gpu_lens import FOCUS, lens_fused, lens_rays
from test_gpu_radiance import _mirror_case
from test_gpu_samples import negative_channels, same_bits
from test_gpu_samples_async import (COUNTS, F32X3, F64X3, GUARD, RGB8, _weights, counts, fused, real_rows,
                                    same_records)
from test_radiance_host import F64_KEPT, same_values

pytestmark = pytest.mark.gpu

INVALID, NO_SCENE = 1, 5  # rt_status
FORMATS = (RGB8, F32X3, F64X3)
ZERO = dict.fromkeys(COUNTS, 0)
COMPLEX = ("file", "complex")
RADIUS = 0.5

# One sphere that fills a narrow view, three small ones between it and the lights, three lights.
_BODY = ("sphere 0 0 -10 6 0.8 0.7 0.6 0.3 1 20\nsphere 2 5 -5 1 0.2 0.9 0.3 0 1 10\n"
         "sphere -2 4 -4 0.8 0.9 0.2 0.2 0.5 1 30\nsphere 0.5 6 -7 0.7 0.3 0.3 0.9 0 1 5\n")
_LIGHTS = "light 4 10 0 1 1 1 0.5\nlight -5 9 -2 1 0.9 0.8 0.4\nlight 0 12 -8 0.8 0.9 1 0.4\n"
_AMB = "ambient 0.1 0.1 0.12\n"
CLOSE_UP = ("text", _BODY + _LIGHTS + _AMB + "camera 0 0 0 0 0 -10 30\n")   # every pixel hits: the lane-per-ray loop
SPARSE = ("text", _BODY + _LIGHTS + _AMB + "camera 0 0 30 0 0 -10 60\n")    # under a third hit: the wide form
ONE_LIGHT = ("text", _BODY + _LIGHTS.split("\n")[0] + "\n" + _AMB + "camera 0 0 0 0 0 -10 30\n")
ONE_LIGHT_FAR = ("text", _BODY + _LIGHTS.split("\n")[0] + "\n" + _AMB + "camera 0 0 30 0 0 -10 60\n")


def _load(spec):
    import rt_hip

    kind, v = spec
    return rt_hip.Scene.load(scene_path(v)) if kind == "file" else rt_hip.Scene.parse(v)


def light_positions(sc):
    return np.array([[sc.raw.lights[l].position[k] for k in range(3)] for l in range(sc.num_lights)],
                    np.float64).reshape(sc.num_lights, 3)


def upload_shifted(yard, ysc, base, row):
    """Step 1 and the upload of step 2: base + row (numpy fp64 adds) written into ysc's light array."""
    with np.errstate(all="ignore"):
        pos = base + np.asarray(row, np.float64).reshape(base.shape)
    for l in range(base.shape[0]):
        for k in range(3):
            ysc.raw.lights[l].position[k] = float(pos[l, k])
    yard.upload(ysc)


def yardstick(yard, spec, table, jobs, D):
    """jobs: host ray records [npix * S, 8], pixel-major with a pixel's samples consecutive.  Per job
    (colours [npix, S, 3] of rt_trace_radiance on the shifted scenes, the launches' counts summed)."""
    S = len(table)
    ysc = _load(spec)
    base = light_positions(ysc)
    cols = [np.zeros((rays.shape[0] // S, S, 3)) for rays in jobs]
    cnts = [dict(ZERO) for _ in jobs]
    for s in range(S):
        upload_shifted(yard, ysc, base, table[s])
        for j, rays in enumerate(jobs):
            rs = rays[s::S]
            c, st = yard.trace_radiance(rs[:, 0:3], rs[:, 3:6], D)
            cols[j][:, s] = c
            for k in COUNTS:
                cnts[j][k] += getattr(st, k)
    return list(zip(cols, cnts))


def expected(cols, cnt, weights, fmt):
    """Step 3: the records of `fmt` and the counts a resolving launch reports."""
    px = sample_ref.resolve(cols, weights)
    with np.errstate(all="ignore"):
        rec = px if fmt == F64X3 else px.astype(np.float32) if fmt == F32X3 else path_ref.quantize(px)
    return rec, dict(cnt, negative_clamped=negative_channels(px) if fmt == RGB8 else 0)


def sample_rays(r, cam, W, H, pattern, rows=None):
    """rt_camera_sample_rays into a device buffer, as host records [n, 8]."""
    import torch

    n = (rows.count if rows is not None else H) * W * len(pattern)
    rays = torch.zeros((n * 8 + 8,), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    r.camera_sample_rays(cam, W, H, rows, pattern, rays.data_ptr())
    torch.cuda.synchronize()
    return rays.cpu().numpy()[:n * 8].reshape(n, 8)


@contextlib.contextmanager
def table_set(r, table):
    """The table on the (shared) context, cleared again behind the test."""
    r.set_light_samples(table)
    try:
        yield
    finally:
        r.set_light_samples(None)


def _patterns(S, nl, radius=RADIUS):
    import rt_hip

    return rt_hip.grid_pattern(8)[:S], rt_hip.lens_pattern(8, 0.3)[:S], rt_hip.light_pattern(8, radius, nl)[:S]


def launch(r, form, cam, W, H, D, pattern, lens, weights=None, rows=None, fmt=RGB8):
    if form == "lens":
        return lens_fused(r, cam, W, H, D, pattern, lens, FOCUS, weights, rows, fmt)
    return fused(r, cam, W, H, D, pattern, weights, rows, fmt)


def check_forms(r, yard, spec, table, W, H, D, pattern, lens, weight_sets=(None,), forms=("pinhole", "lens"),
                fmts=FORMATS, skip_counts=(), what=""):
    """The fused pinhole and lens launches under `table` against the yardstick: records and counts."""
    sc = _load(spec)
    cam = sc.camera()
    r.upload(sc)
    jobs = {"pinhole": lambda: sample_rays(yard, cam, W, H, pattern),
            "lens": lambda: lens_rays(yard, cam, W, H, pattern, lens, FOCUS)[1]}
    ref = dict(zip(forms, yardstick(yard, spec, table, [jobs[f]() for f in forms], D)))
    out = {}
    with table_set(r, table):
        for form in forms:
            cols, cnt = ref[form]
            for wi, w in enumerate(weight_sets):
                for fmt in fmts:
                    want, want_cnt = expected(cols, cnt, w, fmt)
                    got, st = launch(r, form, cam, W, H, D, pattern, lens, w, None, fmt)
                    assert got.dtype == want.dtype and got.shape == want.shape
                    assert same_records(got, want, fmt), (what, form, wi, fmt)
                    have = counts(st)
                    for k in skip_counts:
                        have.pop(k), want_cnt.pop(k)
                    assert have == want_cnt, (what, form, wi, fmt)
                    assert st.rays == W * H * len(pattern)
                    out[form, wi, fmt] = (got, st)
    return out


@pytest.fixture(scope="module")
def yard():
    """The yardstick's own context: it never holds a table."""
    import rt_hip

    r = rt_hip.Renderer(0)
    yield r
    r.close()


# ---- 1. bit equality with the yardstick ------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 63, 64, 65, 129])
def test_equals_the_shifted_scenes(gpu_renderer, yard, W):
    nl = _load(COMPLEX).num_lights
    assert nl == 5
    for S in (1, 4):
        pattern, lens, table = _patterns(S, nl)
        assert len({tuple(o) for o in table[0]}) == nl  # the offsets differ per light
        check_forms(gpu_renderer, yard, COMPLEX, table, W, 3, 4, pattern, lens, (None, _weights(S)), what=(W, S))


def test_equals_the_shifted_scenes_at_64_samples(gpu_renderer, yard):
    pattern, lens, table = _patterns(64, 5)
    check_forms(gpu_renderer, yard, COMPLEX, table, 65, 3, 4, pattern, lens, (None, _weights(64)), what="S = 64")


# ---- 2. both branches of the light loop ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["close_up", "sparse", "one_light", "one_light_far"])
def test_both_light_loop_branches(gpu_renderer, yard, name):
    spec = {"close_up": CLOSE_UP, "sparse": SPARSE, "one_light": ONE_LIGHT, "one_light_far": ONE_LIGHT_FAR}[name]
    nl = _load(spec).num_lights
    W, H, D, S = 64, 3, 4, 4
    pattern, _, table = _patterns(S, nl, 1.5)
    got = check_forms(gpu_renderer, yard, spec, table, W, H, D, pattern, None, (None,), ("pinhole",), what=name)
    st = got["pinhole", 0, F64X3][1]
    assert st.shadow_rays == st.hits * nl
    if name in ("close_up", "one_light"):
        assert st.hits >= W * H * S  # every primary ray hits: 64 hit lanes, one light per pass
    else:
        assert 0 < st.hits < W * H * S // 3  # at most a third of a wave's lanes hit


# ---- 3. lights far outside the uploaded bound, and offsets that are not finite ---------------------------
def test_far_lights(gpu_renderer, yard):
    pattern, lens, table = _patterns(4, 5)
    table = [list(row) for row in table]
    table[1][0] = (1e3, 2e3, -1e3)
    table[3][0] = (0.0, -1.5e3, 0.0)  # below the scene: the light shines from underneath
    table[3][4] = (-1e3, 0.0, 1e3)
    # the yardstick's own query region follows its lights: `unaccelerated` is the one count that may differ
    got = check_forms(gpu_renderer, yard, COMPLEX, table, 65, 3, 4, pattern, lens, (None, _weights(4)),
                      skip_counts=("unaccelerated",), what="far")
    assert np.isfinite(got["pinhole", 0, F64X3][0]).all()


def test_offsets_that_are_not_finite(gpu_renderer, yard):
    pattern, lens, table = _patterns(4, 5)
    table = [list(row) for row in table]
    table[2][1] = (float("nan"), 0.0, float("inf"))
    # (the shifted scene's bound is not finite: it has no query region, and every lane of the yardstick is
    # unaccelerated)
    got = check_forms(gpu_renderer, yard, COMPLEX, table, 65, 3, 4, pattern, lens, (None, _weights(4)),
                      skip_counts=("unaccelerated",), what="nan")
    # a NaN direction: never shadowed, and std::max(0.0, NaN) makes its Phong terms 0.0 -- never an error
    assert np.isfinite(got["pinhole", 0, F64X3][0]).all()
    plain = check_forms(gpu_renderer, yard, COMPLEX, _patterns(4, 5)[2], 65, 3, 4, pattern, lens, fmts=(F64X3,))
    assert not same_bits(got["pinhole", 0, F64X3][0], plain["pinhole", 0, F64X3][0]).all()  # the light went dark


# ---- 4. the caller's rays --------------------------------------------------------------------------------
def test_resolve_of_the_callers_rays_honours_the_table(gpu_renderer, yard):
    import torch

    S, npix, D = 4, 150, 4
    rng = np.random.default_rng(11)
    o = np.array([0.0, 3.0, 12.0]) + rng.uniform(-1.0, 1.0, (npix * S, 3))
    d = np.array([0.0, -3.0, -32.0]) + rng.uniform(-12.0, 12.0, (npix * S, 3))  # any length
    rays = np.zeros((npix * S, 8))
    rays[:, 0:3], rays[:, 3:6] = o, d
    _, _, table = _patterns(S, 5)
    (cols, cnt), = yardstick(yard, COMPLEX, table, [rays], D)
    gpu_renderer.upload(_load(COMPLEX))
    plain, _ = gpu_renderer.trace_radiance_resolve(o, d, S, D, None, F64X3)
    with table_set(gpu_renderer, table):
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
    sc = _load(COMPLEX)
    cam = sc.camera()
    gpu_renderer.upload(sc)
    W, H, D, S = 37, 21, 4, 4
    pattern, _, table = _patterns(S, 5)
    plain, _ = fused(gpu_renderer, cam, W, H, D, pattern)
    with table_set(gpu_renderer, table):
        for w in (None, _weights(S)):
            for fmt in FORMATS:
                want, st0 = fused(gpu_renderer, cam, W, H, D, pattern, w, None, fmt)
                got, st = gpu_renderer.render_samples(cam, W, H, D, pattern, w, None, fmt,
                                                      max_ray_bytes=W * S * 64)  # one row per chunk
                assert got.tobytes() == want.tobytes(), fmt
                assert counts(st) == counts(st0)
        assert want.shape == (W * H, 3)
    soft, _ = gpu_renderer.render_samples(cam, W, H, D, pattern)
    assert soft.tobytes() == plain.tobytes()  # cleared: the chunked form follows


# ---- 6. / 7. a zero table, a cleared table ------------------------------------------------------------------
def test_zero_and_cleared_tables_write_the_bytes_of_no_table(gpu_renderer):
    import rt_hip

    sc = _load(COMPLEX)
    cam = sc.camera()
    lp = light_positions(sc)
    assert not (np.signbit(lp) & (lp == 0)).any()  # no -0.0 coordinate: L + 0.0 is L in bits
    gpu_renderer.upload(sc)
    W, H, D, S = 37, 21, 4, 4
    pattern, lens, table = _patterns(S, 5)

    def both(fmt, p=pattern, ln=lens):
        a, sa = fused(gpu_renderer, cam, W, H, D, p, None, None, fmt)
        b, sb = lens_fused(gpu_renderer, cam, W, H, D, p, ln, FOCUS, None, None, fmt)
        return a.tobytes(), b.tobytes(), counts(sa), counts(sb)

    none = {fmt: both(fmt) for fmt in FORMATS}
    gpu_renderer.set_light_samples(np.zeros((S, 5, 3)))
    try:
        for fmt in FORMATS:
            assert both(fmt) == none[fmt], fmt
        gpu_renderer.set_light_samples(table)
        assert both(RGB8)[:2] != none[RGB8][:2]
        gpu_renderer.set_light_samples(None)
        for fmt in FORMATS:
            assert both(fmt) == none[fmt], fmt
        # rt_upload_scene clears the table: another S is accepted and writes the bytes of no table
        gpu_renderer.set_light_samples(table)
        gpu_renderer.upload(sc)
        for fmt in FORMATS:
            assert both(fmt) == none[fmt], fmt
        p9, l9 = rt_hip.grid_pattern(3), rt_hip.lens_pattern(3, 0.3)
        nine = both(RGB8, p9, l9)
        gpu_renderer.set_light_samples(table)
        gpu_renderer.upload(sc)
        assert both(RGB8, p9, l9) == nine
    finally:
        gpu_renderer.set_light_samples(None)


# ---- 8. a radius changes the image, and only where something is hit --------------------------------------
def test_a_radius_changes_the_image(gpu_renderer):
    import rt_hip

    m = manifest()["complex_97x61_d4"]
    W, H, D = m["width"], m["height"], m["depth"]
    sc = rt_hip.Scene.load(scene_path(m["scene"]))
    cam = sc.camera()
    gpu_renderer.upload(sc)
    pattern = rt_hip.grid_pattern(4)
    rays = sample_rays(gpu_renderer, cam, W, H, pattern)
    _, sphere, _, _ = gpu_renderer.trace_rays(rays[:, 0:3], rays[:, 3:6])
    sky = (sphere.reshape(W * H, 16) < 0).all(axis=1)  # no sample's chain hits anything
    hard, _ = fused(gpu_renderer, cam, W, H, D, pattern, None, None, F64X3)
    with table_set(gpu_renderer, rt_hip.light_pattern(4, 1.0, sc.num_lights)):
        soft, st = fused(gpu_renderer, cam, W, H, D, pattern, None, None, F64X3)
    differ = ~same_bits(hard, soft).all(axis=1)
    sky_rows = sky.reshape(H, W).all(axis=1)
    print("%d of %d pixels differ, %d all-sky pixels, %d all-sky rows" % (differ.sum(), W * H, sky.sum(), sky_rows.sum()))
    assert differ.sum() > W * H // 20 and st.rays == 16 * W * H
    assert sky.any() and not differ[sky].any()
    assert sky_rows.any() and not differ.reshape(H, W)[sky_rows].any()


# ---- 9. shards, asynchronous calls, and the context's other reports --------------------------------------
ROWS_W, ROWS_H, ROWS_D = 37, 21, 4


def test_shards_are_slices_of_the_frame(gpu_renderer):
    import rt_hip

    sc = _load(COMPLEX)
    cam = sc.camera()
    gpu_renderer.upload(sc)
    W, H, D = ROWS_W, ROWS_H, ROWS_D
    pattern, lens, table = rt_hip.grid_pattern(3), rt_hip.lens_pattern(3, 0.25), rt_hip.light_pattern(3, RADIUS, 5)
    with table_set(gpu_renderer, table):
        for form in ("pinhole", "lens"):
            for fmt in FORMATS:
                full, stf = launch(gpu_renderer, form, cam, W, H, D, pattern, lens, None, None, fmt)
                full = full.reshape(H, W, 3)
                total = dict(ZERO)
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


def test_two_async_calls_and_nothing_else_moves(yard):
    import rt_hip
    import torch

    sc = _load(COMPLEX)
    cam = sc.camera()
    W, H, D = ROWS_W, ROWS_H, ROWS_D
    n = W * H
    pattern, lens, table = rt_hip.grid_pattern(2), rt_hip.lens_pattern(2, 0.3), rt_hip.light_pattern(2, RADIUS, 5)
    r = rt_hip.Renderer(0)
    side = torch.cuda.Stream()
    try:
        r.upload(sc)
        r.set_light_samples(table)
        want_a, _ = fused(r, cam, W, H, D, pattern)  # the synchronous results
        want_b, st_b = lens_fused(r, cam, W, H, D, pattern, lens, FOCUS, _weights(4), None, F64X3)
        host, _ = r.render_lens_samples(cam, W, H, D, pattern, lens, FOCUS, _weights(4), None, F64X3)
        assert same_bits(host, want_b).all()
        r.set_light_samples(None)
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
        r.set_light_samples(table)
        a = torch.full((n * 3 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        b = torch.full((n * 24 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        r.set_stream(side.cuda_stream)
        r.render_samples_async(cam, W, H, D, pattern, a.data_ptr())
        r.render_lens_samples_async(cam, W, H, D, pattern, lens, FOCUS, b.data_ptr(), _weights(4), None, F64X3)
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


# ---- 10. a second grid-stride trip -----------------------------------------------------------------------
def test_second_trip_of_the_stack_bounded_grid(gpu_renderer, yard):
    """Depth 64 bounds the grid at 2,080 waves (133,120 lanes): 365 x 365 pixels of the two-mirror scene
    take a second trip, in which a lane's stack slots are reused across trips and samples."""
    import rt_hip
    from test_gpu_radiance import MIRRORS_09

    W = H = 365
    D = rt_hip.RT_MAX_DEPTH
    assert W * H > 2080 * 64 and _mirror_case()[0].num_lights == 1
    pattern = rt_hip.grid_pattern(2)[:2]
    table = [[(0.4, -0.3, 0.2)], [(-0.5, 0.25, -0.125)]]
    got = check_forms(gpu_renderer, yard, ("text", MIRRORS_09), table, W, H, D, pattern, None, (None,), ("pinhole",),
                      (RGB8, F64X3), what="mirrors")
    st = got["pinhole", 0, F64X3][1]
    assert st.rays == 2 * W * H and st.segments > 2 * st.rays


# ---- 11. the calls without a sample index ----------------------------------------------------------------
def test_unaffected_calls(gpu_renderer):
    import rt_hip

    sc = _load(COMPLEX)
    cam = sc.camera()
    gpu_renderer.upload(sc)
    W, H, D = ROWS_W, ROWS_H, ROWS_D
    rays = sample_rays(gpu_renderer, cam, W, H, [(0.0, 0.0)])
    o, d = rays[:, 0:3], rays[:, 3:6]

    def calls():
        rad, sr = gpu_renderer.trace_radiance(o, d, D)
        verts, _, sp = gpu_renderer.trace_paths(o, d, D)
        img, si = gpu_renderer.render(cam, W, H, D)
        gpu_renderer.set_antialias(4)
        try:
            aa, sa = gpu_renderer.render(cam, W, H, D)
        finally:
            gpu_renderer.set_antialias(1)
        return (rad.tobytes(), verts.tobytes(), bytes(img), bytes(aa), counts(sr), sp.as_dict()["segments"], si.rays,
                sa.rays)

    want = calls()
    with table_set(gpu_renderer, rt_hip.light_pattern(1, 2.0, 5)):  # one sample: rt_trace_radiance's own count
        assert calls() == want
    with table_set(gpu_renderer, rt_hip.light_pattern(2, 2.0, 5)):
        assert calls() == want


# ---- 12. as values against the CPU checker ---------------------------------------------------------------
@pytest.mark.parametrize("case", F64_KEPT[:2])
def test_checker_chain_as_values(gpu_renderer, case):
    """Shininess 0 or 1 everywhere: pow rounds nothing, and the device's fp64 records are the chain's."""
    import rt_hip

    W, H, D, S = 48, 31, 4, 4
    sc = rt_hip.Scene.parse(mc.text(case, "dense"))
    pattern = rt_hip.grid_pattern(2)
    table = rt_hip.light_pattern(2, 0.75, sc.num_lights)
    sa = path_ref.SceneArrays(sc)
    base = sa.lpos.copy()
    rays = sample_ref.camera_sample_rays(sc.camera(), W, H, pattern)
    cols = np.zeros((W * H, S, 3))
    n = segments = hits = shadow = 0
    for s in range(S):
        sa.lpos = base + np.asarray(table[s], np.float64).reshape(base.shape)
        levels = path_ref.trace_paths(rays[s::S, 0:3], rays[s::S, 3:6], D, sa)
        cols[:, s] = path_ref.shade(levels, sa)
        c = path_ref.counts(levels, sa)
        n, segments, hits, shadow = n + c[0], segments + c[1], hits + c[2], shadow + c[3]
    want = sample_ref.resolve(cols)
    gpu_renderer.upload(sc)
    with table_set(gpu_renderer, table):
        got, st = fused(gpu_renderer, sc.camera(), W, H, D, pattern, None, None, F64X3)
        rgb, _ = fused(gpu_renderer, sc.camera(), W, H, D, pattern)
    same = same_values(got, want)
    assert same.all(), "%d of %d channels differ" % (int((~same).sum()), same.size)
    assert (st.rays, st.segments, st.hits, st.shadow_rays) == (n, segments, hits, shadow)
    assert np.array_equal(rgb, path_ref.quantize(want))


# ---- 13. errors ------------------------------------------------------------------------------------------
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
        tab = (C.c_double * (65 * 2 * 3))()
        st = rt_hip.rt_radiance_stats()
        assert L.rt_set_light_samples(None, tab, 4) == INVALID  # a NULL ctx
        assert L.rt_group_set_light_samples(None, tab, 4) == INVALID
        assert L.rt_set_light_samples(r.handle, tab, 4) == NO_SCENE
        assert L.rt_set_light_samples(r.handle, None, 0) == NO_SCENE
        assert L.rt_set_light_samples(r.handle, tab, 0) == INVALID  # the arguments first
        assert L.rt_group_set_light_samples(g._grp, tab, 4) == NO_SCENE
        assert b"no scene" in L.rt_group_last_error(g._grp)
        sc = rt_hip.Scene.load(scene_path("simple"))
        assert sc.num_lights == 2
        cam = sc.camera()
        r.upload(sc)
        g.upload(sc)
        pattern, lens_pts = rt_hip.grid_pattern(2), rt_hip.lens_pattern(2, 0.1)
        table = rt_hip.light_pattern(2, 0.5, 2)
        none = fused(r, cam, W, H, 3, pattern)[0].tobytes()
        r.set_light_samples(table)
        g.set_light_samples(table)
        soft = fused(r, cam, W, H, 3, pattern)[0].tobytes()
        assert soft != none
        for S in (0, 65, -1):
            assert L.rt_set_light_samples(r.handle, tab, S) == INVALID
            assert L.rt_group_set_light_samples(g._grp, tab, S) == INVALID
            assert b"RT_MAX_SAMPLES" in L.rt_group_last_error(g._grp)
        with pytest.raises(ValueError):
            r.set_light_samples([[(0.0, 0.0, 0.0)] * 3] * 4)  # three lights' offsets for a scene of two
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
        for name, f in (
                ("rt_group_render_samples",
                 lambda: L.rt_group_render_samples(g._grp, cp, W, H, 3, off, 9, None, F64X3, hp, 0, C.byref(st))),
                ("rt_group_render_lens_samples",
                 lambda: L.rt_group_render_lens_samples(g._grp, cp, W, H, 3, off, lens, 2.0, 9, None, F64X3, hp, 0,
                                                        C.byref(st)))):
            assert f() == INVALID
            err = L.rt_group_last_error(g._grp).decode()
            assert name in err and "light table" in err and "9" in err and "4" in err, err
        assert (out.cpu().numpy() == 0).all() and (host == 0).all()  # nothing was written
        # the calls without a sample index take any count; the generator reads no table
        assert L.rt_camera_sample_rays(r.handle, cp, W, H, None, off, 9, rp) == 0
        assert L.rt_trace_radiance_async(r.handle, rp, W * H, 3, RGB8, op) == 0
        assert r.radiance_stats().rays == W * H
        assert fused(r, cam, W, H, 3, pattern)[0].tobytes() == soft
        got, _ = g.render_samples(cam, W, H, 3, pattern)
        assert got.tobytes() == soft
        # a scene without lights takes the call and renders as without a table; the count is still checked
        dark = rt_hip.Scene.parse("sphere 0 0 -5 1 1 0 0 0 1 10\nambient 0.3 0.3 0.3\ncamera 0 0 0 0 0 -1 60\n")
        assert dark.num_lights == 0
        r.upload(dark)
        want = fused(r, dark.camera(), W, H, 3, pattern)[0].tobytes()
        r.set_light_samples([[]] * 4)
        assert fused(r, dark.camera(), W, H, 3, pattern)[0].tobytes() == want
        assert L.rt_render_samples_async(r.handle, C.byref(dark.camera()), W, H, 3, None, off, 9, None, RGB8, op) == INVALID
    finally:
        g.close()
        r.close()


# ---- 14. the check and tuning builds ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _variant_reference():
    """Case 1 at W = 65 by the yardstick on the product library, once."""
    import rt_hip

    S, W, H, D = 4, 65, 3, 4
    pattern, lens, table = _patterns(S, 5)
    r = rt_hip.Renderer(0)
    try:
        cam = _load(COMPLEX).camera()
        jobs = [sample_rays(r, cam, W, H, pattern), lens_rays(r, cam, W, H, pattern, lens, FOCUS)[1]]
        ref = yardstick(r, COMPLEX, table, jobs, D)
    finally:
        r.close()
    return (W, H, D, pattern, lens, table), dict(zip(("pinhole", "lens"), ref))


@pytest.mark.parametrize("variant", ["check", "tuning"])
def test_variant_builds(variant):
    import rt_hip

    (W, H, D, pattern, lens, table), ref = _variant_reference()
    r = rt_hip.Renderer(0, variant=variant)
    try:
        sc = _load(COMPLEX)
        r.upload(sc)
        r.set_light_samples(table)
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
def test_cli_light_radius(tmp_path):
    """One run (a process start costs seconds): --light-radius with --aperture through the device group, the
    path on which ray_hip restates light_pattern and lens_pattern and calls rt_group_set_light_samples."""
    import rt_hip

    W, H, D, N = 37, 21, 4, 3
    scene = scene_path("complex")
    sc = rt_hip.Scene.load(scene)
    pattern, lens = rt_hip.grid_pattern(N), rt_hip.lens_pattern(N, 0.2)
    r = rt_hip.Renderer(0)
    try:
        r.upload(sc)
        hard, _ = r.render_lens_samples(sc.camera(), W, H, D, pattern, lens, FOCUS)
        r.set_light_samples(rt_hip.light_pattern(N, 0.75, sc.num_lights))
        soft, _ = r.render_lens_samples(sc.camera(), W, H, D, pattern, lens, FOCUS)
    finally:
        r.close()
    assert soft.tobytes() != hard.tobytes()
    p = subprocess.run([os.path.join(PKG, "ray_hip"), "--supersample", str(N), "--light-radius", "0.75", "--aperture",
                        "0.2", "--focus", str(FOCUS), "--sample-devices", "0,0", "--width", str(W), "--height", str(H),
                        "--depth", str(D), "--p6", "--out", "out.ppm", scene],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "GPU rendering time:" in p.stdout, p.stdout + p.stderr
    assert open(tmp_path / "out.ppm", "rb").read() == b"P6\n%d %d\n255\n" % (W, H) + soft.tobytes()
