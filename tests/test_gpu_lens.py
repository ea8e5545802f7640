"""GPU: the thin-lens entries (include/rt_hip.h, "samples through a thin lens"): rt_camera_lens_rays,
rt_render_lens_samples_async and rt_render_lens_samples.  The yardsticks:

  * tests/lens_ref.py for the ray records, in bits;
  * rt_camera_lens_rays + rt_trace_radiance_resolve_async through a ray buffer on a SECOND context for the
    fused call's records and counts, in bits (the fused call promises that pair's records);
  * lens_ref -> path_ref -> sample_ref.resolve, the pure checker chain, as values where no pow is
    involved and within 1 per RGB8 channel where one is;
  * rt_render_samples_async for a zero lens with focus 1.0.

Shapes as test_gpu_samples_async.py: the smallest at which the pixel -> (row, column) arithmetic, the
padding suffix, the packed RGB8 store and the grid-stride loop's second trip can each go wrong."""
import ctypes as C
import functools

import numpy as np
import pytest

import lens_ref
import material_cases as mc
import path_ref
import sample_ref
from conftest import manifest, scene_path
from test_gpu_radiance import _mirror_case, check_pm1
from test_gpu_samples import same_bits
from test_gpu_samples_async import (COUNTS, F32X3, F64X3, GUARD, RECORD, RGB8, _weights, counts, fused, real_rows,
                                    same_records)
from test_radiance_host import F64_KEPT, same_values

pytestmark = pytest.mark.gpu

INVALID, NO_SCENE, DEPTH = 1, 5, 7  # rt_status
FORMATS = (RGB8, F32X3, F64X3)
ZERO = dict.fromkeys(COUNTS, 0)


def lens_fused(r, cam, W, H, D, pattern, lens, focus, weights=None, rows=None, fmt=RGB8):
    """One rt_render_lens_samples_async into a 0xA5-filled device buffer with a guard behind it: (records
    [n, 3], the radiance family's report afterwards); asserts that the guard is intact."""
    import torch

    n = (rows.count if rows is not None else H) * W
    nbytes = n * RECORD[fmt][1]
    dev = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert dev.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    r.render_lens_samples_async(cam, W, H, D, pattern, lens, focus, dev.data_ptr(), weights, rows, fmt)
    st = r.radiance_stats()  # waits for the stream
    got = dev.cpu().numpy()
    assert (got[nbytes:] == 0xA5).all(), "bytes behind the records were written"
    return got[:nbytes].view(RECORD[fmt][0]).reshape(n, 3), st


def lens_rays(r, cam, W, H, pattern, lens, focus, rows=None):
    """rt_camera_lens_rays into a device buffer: (the torch buffer, the records as numpy [n, 8])."""
    import torch

    n = (rows.count if rows is not None else H) * W * len(pattern)
    rays = torch.full((n * 8 + 8,), 7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    r.camera_lens_rays(cam, W, H, rows, pattern, lens, focus, rays.data_ptr())
    torch.cuda.synchronize()
    host = rays.cpu().numpy()
    assert (host[n * 8:] == 7.0).all()
    return rays, host[:n * 8].reshape(n, 8)


def two_step(yard, cam, W, H, D, pattern, lens, focus, weights=None, rows=None, fmt=RGB8):
    """The reference path: rt_camera_lens_rays into a ray buffer, then rt_trace_radiance_resolve_async of
    the REAL rows' rays (the padding rows of a shard are all-zero rays, which the fused call does not
    trace: its records are zero bytes).  Returns (records [count * W, 3], counts)."""
    import torch

    count = rows.count if rows is not None else H
    real = real_rows(rows, H) if rows is not None else H
    rays, _ = lens_rays(yard, cam, W, H, pattern, lens, focus, rows)
    dtype, size = RECORD[fmt]
    out = torch.zeros((count * W * size + 16,), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    cnt = dict(ZERO)
    if real:
        yard.trace_radiance_resolve_device(rays.data_ptr(), real * W, len(pattern), D, fmt, out.data_ptr(), weights)
        cnt = counts(yard.radiance_stats())
    torch.cuda.synchronize()
    return out.cpu().numpy()[:count * W * size].view(dtype).reshape(count * W, 3), cnt


def check_equal(r, yard, cam, W, H, D, pattern, lens, focus, weights=None, rows=None, fmts=FORMATS, what=""):
    """The fused lens call against the two-step reference of the yardstick context: records and counts."""
    out = {}
    real = real_rows(rows, H) if rows is not None else H
    for fmt in fmts:
        want, cnt = two_step(yard, cam, W, H, D, pattern, lens, focus, weights, rows, fmt)
        got, st = lens_fused(r, cam, W, H, D, pattern, lens, focus, weights, rows, fmt)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert same_records(got, want, fmt), (what, fmt)
        if real:
            assert counts(st) == cnt, (what, fmt)
            assert st.rays == real * W * len(pattern)
        out[fmt] = (got, st)
    return out


@pytest.fixture(scope="module")
def yard():
    """The yardstick's own context: the ray buffer path never runs on the context under test."""
    import rt_hip

    r = rt_hip.Renderer(0)
    yield r
    r.close()


def _complex(*renderers):
    import rt_hip

    sc = rt_hip.Scene.load(scene_path("complex"))
    for r in renderers:
        r.upload(sc)
    return sc, sc.camera()


def _pattern(S, aperture=0.3):
    import rt_hip

    return rt_hip.grid_pattern(8)[:S], rt_hip.lens_pattern(8, aperture)[:S]


FOCUS = 7.25  # in front of the complex scene's spheres (24 to 47 units from the camera): all of them blur
ROWS_W, ROWS_H, ROWS_D = 37, 21, 4


# ---- 1. the ray records --------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 4, 64])
@pytest.mark.parametrize("W,H,shard", [(97, 61, False), (1, 1, False), (2, 2, False), (5, 21, True)])
def test_lens_rays_equal_the_checker_in_bits(gpu_renderer, W, H, shard, S):
    import rt_hip

    cam = rt_hip.Scene.load(scene_path("complex")).camera()
    rows = rt_hip.rows_for_shard(21, 8, 2, 3) if shard else None
    pattern, lens = _pattern(S)
    _, got = lens_rays(gpu_renderer, cam, W, H, pattern, lens, FOCUS, rows)
    want = lens_ref.camera_lens_rays(cam, W, H, pattern, lens, FOCUS, rows)
    assert got.shape == want.shape and same_bits(got, want).all(), (W, H, S)
    if shard:
        assert (got.reshape(rows.count, -1)[5:] == 0).all()  # rows 16..20, then three of padding
    assert np.isnan(got[:, 3:6]).any() == (W == 1)  # W - 1 = 0: NaN directions, not an error


# ---- 2. the fused call against the ray buffer path -----------------------------------------------------
@pytest.mark.parametrize("W", [1, 63, 64, 65, 129])
def test_fused_equals_rays_then_resolve(gpu_renderer, yard, W):
    _, cam = _complex(gpu_renderer, yard)
    H = 5 if W == 1 else 3 if W < 129 else 2
    for S in (1, 2, 5, 64):
        pattern, lens = _pattern(S)
        for D in (1, 4):
            check_equal(gpu_renderer, yard, cam, W, H, D, pattern, lens, FOCUS, what=(W, S, D))
    pattern, lens = _pattern(5)
    check_equal(gpu_renderer, yard, cam, W, H, 4, pattern, lens, FOCUS, _weights(5), what=(W, "weighted"))


# ---- 3. the pure checker chain -------------------------------------------------------------------------
def _chain(sc, W, H, D, pattern, lens, focus):
    sa = path_ref.SceneArrays(sc)
    rays = lens_ref.camera_lens_rays(sc.camera(), W, H, pattern, lens, focus)
    levels = path_ref.trace_paths(rays[:, 0:3], rays[:, 3:6], D, sa)
    return sample_ref.resolve(path_ref.shade(levels, sa).reshape(W * H, len(pattern), 3)), path_ref.counts(levels, sa)


@pytest.mark.parametrize("case", F64_KEPT)
def test_checker_chain_as_values(gpu_renderer, case):
    """Shininess 0 or 1 everywhere: pow rounds nothing, and the device's fp64 records are the chain's."""
    import rt_hip

    W, H, D = 48, 31, 4
    sc = rt_hip.Scene.parse(mc.text(case, "dense"))
    pattern, lens = rt_hip.grid_pattern(2), rt_hip.lens_pattern(2, 0.2)
    want, (n, segments, hits, shadow) = _chain(sc, W, H, D, pattern, lens, 10.0)
    gpu_renderer.upload(sc)
    got, st = lens_fused(gpu_renderer, sc.camera(), W, H, D, pattern, lens, 10.0, fmt=F64X3)
    same = same_values(got, want)
    assert same.all(), "%d of %d channels differ" % (int((~same).sum()), same.size)
    assert (st.rays, st.segments, st.hits, st.shadow_rays) == (n, segments, hits, shadow)
    rgb, _ = lens_fused(gpu_renderer, sc.camera(), W, H, D, pattern, lens, 10.0)
    assert np.array_equal(rgb, path_ref.quantize(want))


def test_checker_chain_with_fractional_shininess(gpu_renderer):
    import rt_hip

    W, H, D = 48, 31, 4
    sc = rt_hip.Scene.parse(mc.text("shin_frac_edges", "dense"))
    pattern, lens = rt_hip.grid_pattern(2), rt_hip.lens_pattern(2, 0.2)
    want, _ = _chain(sc, W, H, D, pattern, lens, 10.0)
    gpu_renderer.upload(sc)
    rgb, _ = lens_fused(gpu_renderer, sc.camera(), W, H, D, pattern, lens, 10.0)
    check_pm1(rgb, path_ref.quantize(want), "shin_frac_edges through the lens")


# ---- 4. / 5. the pinhole limit, and a lens that is used ---------------------------------------------------
def test_zero_lens_and_unit_focus_write_the_pinhole_bytes(gpu_renderer):
    import rt_hip

    _, cam = _complex(gpu_renderer)
    pattern = rt_hip.grid_pattern(3)
    for fmt in FORMATS:
        for w in (None, _weights(9)):
            want, st0 = fused(gpu_renderer, cam, ROWS_W, ROWS_H, ROWS_D, pattern, w, None, fmt)
            got, st = lens_fused(gpu_renderer, cam, ROWS_W, ROWS_H, ROWS_D, pattern, [(0.0, 0.0)] * 9, 1.0, w, None, fmt)
            assert got.tobytes() == want.tobytes(), fmt
            assert counts(st) == counts(st0)


def test_an_aperture_changes_the_image(gpu_renderer):
    import rt_hip

    m = manifest()["complex_97x61_d4"]
    W, H, D = m["width"], m["height"], m["depth"]
    sc = rt_hip.Scene.load(scene_path(m["scene"]))
    gpu_renderer.upload(sc)
    pattern = rt_hip.grid_pattern(4)
    pinhole, _ = fused(gpu_renderer, sc.camera(), W, H, D, pattern)
    blurred, st = lens_fused(gpu_renderer, sc.camera(), W, H, D, pattern, rt_hip.lens_pattern(4, 0.4), FOCUS)
    differ = int((pinhole != blurred).any(axis=1).sum())
    print("%d of %d pixels differ" % (differ, W * H))
    assert differ > W * H // 20 and st.rays == 16 * W * H
    again, _ = gpu_renderer.render_lens_samples(sc.camera(), W, H, D, pattern, rt_hip.lens_pattern(4, 0.4), FOCUS)
    assert again.tobytes() == blurred.tobytes()  # the synchronous form, host memory


# ---- 6. shards -----------------------------------------------------------------------------------------
def _rows_cases():
    import rt_hip

    return [rt_hip.rows_for_shard(ROWS_H, 8, k, 3) for k in range(3)] + [rt_hip.rt_rows(3, 1, 2, 7)]


@pytest.mark.parametrize("case", range(4), ids=["shard0", "shard1", "shard2", "rows3127"])
def test_shards_are_slices_of_the_frame(gpu_renderer, yard, case):
    import rt_hip
    import torch

    _, cam = _complex(gpu_renderer, yard)
    rows = _rows_cases()[case]
    pattern, lens = rt_hip.grid_pattern(3), rt_hip.lens_pattern(3, 0.25)
    W, H, D = ROWS_W, ROWS_H, ROWS_D
    real = real_rows(rows, H)
    ys = [(k // rows.band) * rows.band * rows.stride + rows.first * rows.band + k % rows.band for k in range(real)]
    assert (real < rows.count) == (case == 2)
    for w in (None, _weights(9)):
        shard = check_equal(gpu_renderer, yard, cam, W, H, D, pattern, lens, FOCUS, w, rows, what=(case, w is None))
        for fmt, (rec, st) in shard.items():
            full, _ = lens_fused(gpu_renderer, cam, W, H, D, pattern, lens, FOCUS, w, None, fmt)
            full = full.reshape(H, W, 3)
            rec = rec.reshape(rows.count, W, 3)
            assert same_records(rec[:real], full[ys], fmt), (case, fmt)
            assert (rec[real:].view(np.uint8) == 0).all()  # padding records: zero bytes
            assert st.rays == 9 * W * real                 # and not counted
            # the synchronous form: host memory, device memory, the same records and the launch's stats
            host, sth = gpu_renderer.render_lens_samples(cam, W, H, D, pattern, lens, FOCUS, w, rows, fmt)
            assert same_records(host.reshape(rows.count, W, 3), rec, fmt) and counts(sth) == counts(st)
            dev = torch.full((rec.nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            _, std = gpu_renderer.render_lens_samples(cam, W, H, D, pattern, lens, FOCUS, w, rows, fmt,
                                                      out=dev.data_ptr(), out_on_device=True)
            got = dev.cpu().numpy()
            assert got[:rec.nbytes].tobytes() == rec.tobytes() and (got[rec.nbytes:] == 0xA5).all()
            assert counts(std) == counts(st)


def test_a_call_without_a_real_row_launches_nothing(gpu_renderer):
    import rt_hip

    _, cam = _complex(gpu_renderer)
    pattern, lens = rt_hip.grid_pattern(2), rt_hip.lens_pattern(2, 0.25)
    _, st = lens_fused(gpu_renderer, cam, 4, 4, 3, pattern, lens, FOCUS)
    assert st.rays == 64
    below = rt_hip.rt_rows(1, 4, 1, 2)  # two rows below the image: a memset and no launch
    rec, st2 = lens_fused(gpu_renderer, cam, 4, 4, 3, pattern, lens, FOCUS, rows=below, fmt=F64X3)
    assert (rec.view(np.uint8) == 0).all()
    assert counts(st2) == counts(st) and st2.kernel_ms == pytest.approx(st.kernel_ms, rel=1e-4)  # the report stayed
    host, sth = gpu_renderer.render_lens_samples(cam, 4, 4, 3, pattern, lens, FOCUS, rows=below, fmt=F64X3,
                                                 out=np.full((8, 3), 5.0))
    assert (host == 0).all() and counts(sth) == ZERO and sth.kernel_ms == 0  # the synchronous form: zero stats
    none, stn = gpu_renderer.render_lens_samples(cam, 4, 4, 3, pattern, lens, FOCUS, rows=rt_hip.rt_rows(1, 0, 1, 0))
    assert none.shape == (0, 3) and counts(stn) == ZERO
    assert counts(gpu_renderer.radiance_stats()) == counts(st)


# ---- 7. lens points and focus distances that are not ordinary --------------------------------------------
def test_any_double_is_allowed(gpu_renderer, yard):
    _, cam = _complex(gpu_renderer, yard)
    nan, inf = float("nan"), float("inf")
    pattern = [(0.0, 0.0), (0.5, 0.0), (0.0, 0.5)]
    W, H, D = ROWS_W, ROWS_H, ROWS_D
    bad_lens = [(nan, 0.1), (0.1, inf), (-0.2, -0.1)]
    got = check_equal(gpu_renderer, yard, cam, W, H, D, pattern, bad_lens, FOCUS, what="bad lens")
    assert np.isnan(got[F64X3][0]).all() and (got[RGB8][0] == 255).all()  # every pixel has a NaN sample
    # the negative lens point alone is an ordinary ray
    got = check_equal(gpu_renderer, yard, cam, W, H, D, pattern[2:], bad_lens[2:], FOCUS, fmts=(F64X3,))
    assert np.isfinite(got[F64X3][0]).all()
    lens = [(0.1, 0.0), (0.0, 0.1), (-0.1, -0.1)]
    for focus in (nan, 0.0, -3.0, inf, -0.0):
        got = check_equal(gpu_renderer, yard, cam, W, H, D, pattern, lens, focus, what=("focus", focus))
        if focus != focus or focus in (inf, -inf):
            assert np.isnan(got[F64X3][0]).all()  # NaN rays: misses of nothing, never an error
        else:
            assert np.isfinite(got[F64X3][0]).all()  # a zero or negative focus: rays that look elsewhere


# ---- 8. a second grid-stride trip ----------------------------------------------------------------------
def test_second_trip_of_the_stack_bounded_grid(gpu_renderer, yard):
    """Depth 64 bounds the grid at 2,080 waves (133,120 lanes): 365 x 365 pixels of the two-mirror scene
    take a second trip in which a lane's stack slots are reused across trips and samples."""
    import rt_hip

    sc = _mirror_case()[0]
    W = H = 365
    D = rt_hip.RT_MAX_DEPTH
    assert W * H > 2080 * 64
    gpu_renderer.upload(sc)
    yard.upload(sc)
    pattern, lens = rt_hip.grid_pattern(2)[:2], rt_hip.lens_pattern(2, 0.05)[:2]
    got = check_equal(gpu_renderer, yard, sc.camera(), W, H, D, pattern, lens, 1.0, fmts=(RGB8, F64X3), what="mirrors")
    st = got[F64X3][1]
    assert st.rays == 2 * W * H and st.segments > 2 * st.rays


# ---- 9. / 12. asynchrony and isolation -------------------------------------------------------------------
def test_two_calls_on_a_callers_stream_and_nothing_else_moves(yard):
    import rt_hip
    import torch

    sc, cam = _complex(yard)
    W, H, D = ROWS_W, ROWS_H, ROWS_D
    n = W * H
    p2, l2 = rt_hip.grid_pattern(2), rt_hip.lens_pattern(2, 0.3)
    p3, l3 = rt_hip.grid_pattern(3), rt_hip.lens_pattern(3, 0.2)
    want2, _ = two_step(yard, cam, W, H, D, p2, l2, FOCUS)
    want3, cnt3 = two_step(yard, cam, W, H, D, p3, l3, 5.5, _weights(9), None, F64X3)
    r = rt_hip.Renderer(0)
    side = torch.cuda.Stream()
    try:
        r.upload(sc)
        # what the context's other launches report, before
        r.render(cam, W, H, D)
        rays1 = torch.zeros((n, 8), dtype=torch.float64, device="cuda:0")
        r.camera_rays(cam, W, H, None, rays1.data_ptr())
        hits = torch.zeros((64, 2), dtype=torch.float64, device="cuda:0")
        r.trace_rays_device(rays1.data_ptr(), 64, hits.data_ptr())
        verts = torch.zeros((D * 64 * 32,), dtype=torch.uint8, device="cuda:0")
        r.trace_paths_device(rays1.data_ptr(), 64, D, verts.data_ptr())
        r.kernel_times()
        before = (r.stats().as_dict(), r.trace_stats().as_dict(), r.path_stats().as_dict(), r.info().launches,
                  r.info().scratch_bytes)

        a = torch.full((n * 3 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        b = torch.full((n * 24 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        r.set_stream(side.cuda_stream)
        r.render_lens_samples_async(cam, W, H, D, p2, l2, FOCUS, a.data_ptr())
        r.render_lens_samples_async(cam, W, H, D, p3, l3, 5.5, b.data_ptr(), _weights(9), None, F64X3)
        side.synchronize()  # the one wait
        ha, hb = a.cpu().numpy(), b.cpu().numpy()
        assert ha[:n * 3].tobytes() == want2.tobytes() and (ha[n * 3:] == 0xA5).all()
        assert same_bits(hb[:n * 24].view(np.float64).reshape(n, 3), want3).all() and (hb[n * 24:] == 0xA5).all()
        assert counts(r.radiance_stats()) == cnt3  # the most recent launch: the second call's

        after = (r.stats().as_dict(), r.trace_stats().as_dict(), r.path_stats().as_dict(), r.info().launches,
                 r.info().scratch_bytes)
        for got_d, want_d in zip(after[:3], before[:3]):
            # the same launch's events read a second time: the runtime's float differs in its last digits
            assert got_d.pop("kernel_ms") == pytest.approx(want_d.pop("kernel_ms"), rel=1e-4)
        assert after == before
        assert r.kernel_times() == []
    finally:
        r.set_stream(None)
        r.close()


# ---- 10. / 11. culling off, the check and tuning builds --------------------------------------------------
@functools.lru_cache(maxsize=None)
def _full_frame_reference():
    """The rows test's full frame by the ray buffer path of the product library, once."""
    import rt_hip

    sc = rt_hip.Scene.load(scene_path("complex"))
    r = rt_hip.Renderer(0)
    try:
        r.upload(sc)
        out = {}
        for weighted in (False, True):
            for fmt in (RGB8, F64X3):
                rec, cnt = two_step(r, sc.camera(), ROWS_W, ROWS_H, ROWS_D, rt_hip.grid_pattern(3),
                                    rt_hip.lens_pattern(3, 0.25), FOCUS, _weights(9) if weighted else None, None, fmt)
                rec.setflags(write=False)
                out[weighted, fmt] = (rec, cnt)
    finally:
        r.close()
    return sc, out


def _check_full_frame(r, unculled=False):
    import rt_hip

    sc, want = _full_frame_reference()
    for (weighted, fmt), (rec, cnt) in want.items():
        got, st = lens_fused(r, sc.camera(), ROWS_W, ROWS_H, ROWS_D, rt_hip.grid_pattern(3),
                             rt_hip.lens_pattern(3, 0.25), FOCUS, _weights(9) if weighted else None, None, fmt)
        assert same_records(got, rec, fmt), (weighted, fmt)
        if unculled:
            assert st.unaccelerated == st.segments + st.shadow_rays > 0 and st.tests_cull == 0
            cnt = dict(cnt, unaccelerated=st.unaccelerated)
        assert counts(st) == cnt, (weighted, fmt)


def test_unculled_same_bytes(gpu_renderer):
    gpu_renderer.upload(_full_frame_reference()[0])
    gpu_renderer.set_culling(False)
    try:
        _check_full_frame(gpu_renderer, unculled=True)
    finally:
        gpu_renderer.set_culling(True)


@pytest.mark.parametrize("variant", ["check", "tuning"])
def test_variant_builds(variant):
    import rt_hip

    r = rt_hip.Renderer(0, variant=variant)
    try:
        sc = _full_frame_reference()[0]
        r.upload(sc)
        _check_full_frame(r)
        _, got = lens_rays(r, sc.camera(), 5, 21, *_pattern(4), FOCUS, rt_hip.rows_for_shard(21, 8, 2, 3))
        want = lens_ref.camera_lens_rays(sc.camera(), 5, 21, *_pattern(4), FOCUS, rt_hip.rows_for_shard(21, 8, 2, 3))
        assert same_bits(got, want).all()
        r.stats()  # raises on RT_ERR_CHECK
    finally:
        r.close()


# ---- 13. errors, with no launch ------------------------------------------------------------------------
def test_errors():
    import rt_hip
    import torch

    r = rt_hip.Renderer(0)
    L = r._L
    try:
        out = torch.zeros((4 * 4 * 24 + 16,), dtype=torch.uint8, device="cuda:0")
        rays = torch.zeros((4 * 4 * 4 * 8 + 8,), dtype=torch.float64, device="cuda:0")
        op, rp = out.data_ptr(), rays.data_ptr()
        off = (C.c_double * 130)()
        lens = (C.c_double * 130)()
        st = rt_hip.rt_radiance_stats()
        ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
        ptr = lambda x: C.c_void_p(x) if x else None  # noqa: E731

        def fused_call(cam, W, H, D, rows, offsets, ln, S, weights, fmt, p):
            return L.rt_render_lens_samples_async(r.handle, ref(cam), W, H, D, ref(rows), offsets, ln, 2.0, S, weights,
                                                  fmt, ptr(p))

        def sync_call(cam, W, H, D, rows, offsets, ln, S, weights, fmt, p, on_device=1):
            return L.rt_render_lens_samples(r.handle, ref(cam), W, H, D, ref(rows), offsets, ln, 2.0, S, weights, fmt,
                                            ptr(p), on_device, C.byref(st))

        def rays_call(cam, W, H, rows, offsets, ln, S, p):
            return L.rt_camera_lens_rays(r.handle, ref(cam), W, H, ref(rows), offsets, ln, 2.0, S, ptr(p))

        cam = rt_hip.Scene.load(scene_path("simple")).camera()
        rows = rt_hip.rt_rows
        for call in (fused_call, sync_call):
            assert call(cam, 4, 4, 3, None, off, lens, 4, None, RGB8, op) == NO_SCENE
            assert call(cam, 4, 4, 3, rows(1, 0, 1, 0), off, lens, 4, None, RGB8, op) == 0  # no rows: before the scene
        sc = rt_hip.Scene.load(scene_path("simple"))
        r.upload(sc)
        cam = sc.camera()
        for call in (fused_call, sync_call):
            assert call(cam, 4, 4, rt_hip.RT_MAX_DEPTH + 1, None, off, lens, 4, None, RGB8, op) == DEPTH
            bad = [
                lambda: call(None, 4, 4, 3, None, off, lens, 4, None, RGB8, op),
                lambda: call(cam, 4, 4, 3, None, None, lens, 4, None, RGB8, op),
                lambda: call(cam, 4, 4, 3, None, off, None, 4, None, RGB8, op),  # a NULL lens_xy
                lambda: call(cam, 0, 4, 3, None, off, lens, 4, None, RGB8, op),
                lambda: call(cam, 4, -1, 3, None, off, lens, 4, None, RGB8, op),
                lambda: call(cam, 4, 4, 3, None, off, lens, 0, None, RGB8, op),
                lambda: call(cam, 4, 4, 3, None, off, lens, 65, None, RGB8, op),
                lambda: call(cam, 4, 4, 3, None, off, lens, -1, None, RGB8, op),
                lambda: call(cam, 4, 4, 3, rows(0, 0, 1, 4), off, lens, 4, None, RGB8, op),
                lambda: call(cam, 4, 4, 3, rows(1, 0, 0, 4), off, lens, 4, None, RGB8, op),
                lambda: call(cam, 4, 4, 3, rows(1, -1, 1, 4), off, lens, 4, None, RGB8, op),
                lambda: call(cam, 4, 4, 3, rows(1, 0, 1, -1), off, lens, 4, None, RGB8, op),
                lambda: call(cam, 1 << 26, 4, 3, None, off, lens, 64, None, RGB8, op),  # width * samples > 2^31-1
                lambda: call(cam, 4, 4, 3, None, off, lens, 4, None, 3, op),
                lambda: call(cam, 4, 4, 3, None, off, lens, 4, None, -1, op),
                lambda: call(cam, 4, 4, 0, None, off, lens, 4, None, RGB8, op),
                lambda: call(cam, 4, 4, 3, None, off, lens, 4, None, RGB8, 0),
                lambda: call(cam, 4, 4, 3, None, off, lens, 4, None, RGB8, op + 8),  # device memory: 16-byte aligned
                lambda: call(cam, 4, 4, 3, None, off, lens, 4, None, F64X3, op + 4),
                lambda: call(cam, 1 << 11, 1 << 20, 3, rows(1, 0, 1, 1 << 20), off, lens, 1, None, RGB8, op),
                lambda: call(cam, 1 << 16, 1 << 15, 3, None, off, lens, 1, None, RGB8, op),
            ]
            for i, f in enumerate(bad):
                assert f() == INVALID, (call.__name__, i)
            assert call(cam, 4, 4, 3, rows(1, 0, 1, 0), off, lens, 4, None, RGB8, 0) == 0  # count == 0 reads no pointer
        assert L.rt_render_lens_samples_async(None, C.byref(cam), 4, 4, 3, None, off, lens, 2.0, 4, None, RGB8,
                                              C.c_void_p(op)) == INVALID
        bad_rays = [
            lambda: L.rt_camera_lens_rays(None, C.byref(cam), 4, 4, None, off, lens, 2.0, 4, C.c_void_p(rp)),
            lambda: rays_call(None, 4, 4, None, off, lens, 4, rp),
            lambda: rays_call(cam, 4, 4, None, None, lens, 4, rp),
            lambda: rays_call(cam, 4, 4, None, off, None, 4, rp),  # a NULL lens_xy
            lambda: rays_call(cam, 4, 4, None, off, lens, 0, rp),
            lambda: rays_call(cam, 4, 4, None, off, lens, 65, rp),
            lambda: rays_call(cam, 0, 4, None, off, lens, 4, rp),
            lambda: rays_call(cam, 4, 4, None, off, lens, 4, 0),
            lambda: rays_call(cam, 4, 4, None, off, lens, 4, rp + 8),
            lambda: rays_call(cam, 4, 4, rows(0, 0, 1, 4), off, lens, 4, rp),
            lambda: rays_call(cam, 1 << 15, 1 << 15, None, off, lens, 2, rp),  # rays > 2^31-1
        ]
        for i, f in enumerate(bad_rays):
            assert f() == INVALID, ("rays", i)
        assert rays_call(cam, 4, 4, rows(1, 0, 1, 0), off, lens, 4, rp) == 0
        s0 = r.radiance_stats()
        assert s0.rays == 0 and s0.kernel_ms == 0  # nothing was launched
        assert (out.cpu().numpy() == 0).all() and (rays.cpu().numpy() == 0).all()
        # the report of a launch survives the failures and the no-ops behind it
        r.render_lens_samples_async(cam, 4, 4, 3, rt_hip.grid_pattern(2), rt_hip.lens_pattern(2, 0.1), 2.0, op)
        assert r.radiance_stats().rays == 64
        assert fused_call(cam, 4, 4, 3, None, off, None, 4, None, RGB8, op) == INVALID
        assert sync_call(cam, 4, 4, 3, None, off, lens, 4, None, 3, op) == INVALID
        assert fused_call(cam, 4, 4, 3, rows(1, 0, 1, 0), off, lens, 4, None, RGB8, op) == 0
        assert r.radiance_stats().rays == 64
    finally:
        r.close()
