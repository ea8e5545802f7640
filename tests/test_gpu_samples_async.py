"""GPU: rt_render_samples_async (include/rt_hip.h), the fused form of rt_render_samples -- one
launch whose lanes form their pixels' sample rays, no ray buffer, no host wait.  The yardstick is
existing code throughout: rt_render_samples on a SECOND context (its chunks, its ray records), the
render under rt_set_antialias(4), the oracle's render_aa and rt_trace_radiance.  Every comparison is
of bits: the two calls promise the same records.

Shapes: the smallest at which the lane's pixel -> (row, column) arithmetic, the padding suffix, the
packed RGB8 store (whole waves of 64 records from a dword boundary) and the grid-stride loop's second
trip can each go wrong."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import manifest, scene_path
from test_gpu_radiance import _mirror_case
from test_gpu_samples import same_bits

pytestmark = pytest.mark.gpu

RGB8, F32X3, F64X3 = 0, 1, 2  # RT_FB_*
RECORD = {RGB8: (np.uint8, 3), F32X3: (np.float32, 12), F64X3: (np.float64, 24)}
INVALID, NO_SCENE, DEPTH = 1, 5, 7  # rt_status
GUARD = 4096
COUNTS = ("rays", "segments", "hits", "shadow_rays", "unaccelerated", "negative_clamped")


def counts(st):
    return {k: getattr(st, k) for k in COUNTS}


def real_rows(rows, H):
    return sum(1 for k in range(rows.count)
               if (k // rows.band) * rows.band * rows.stride + rows.first * rows.band + k % rows.band < H)


def fused(r, cam, W, H, D, pattern, weights=None, rows=None, fmt=RGB8):
    """One rt_render_samples_async into a 0xA5-filled device buffer with a guard behind it.  Returns
    (records as a numpy [n, 3] array, the launch's stats); asserts that the guard is intact."""
    import torch

    n = (rows.count if rows is not None else H) * W
    nbytes = n * RECORD[fmt][1]
    dev = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert dev.data_ptr() % 16 == 0
    torch.cuda.synchronize()  # the fill has landed
    r.render_samples_async(cam, W, H, D, pattern, dev.data_ptr(), weights, rows, fmt)
    st = r.radiance_stats()  # waits for the stream
    got = dev.cpu().numpy()
    assert (got[nbytes:] == 0xA5).all(), "bytes behind the records were written"
    return got[:nbytes].view(RECORD[fmt][0]).reshape(n, 3), st


def same_records(got, want, fmt):
    if fmt == RGB8:
        return bool(np.array_equal(got, want))
    return bool(same_bits(got, want).all())


def check_equal(r, yard, cam, W, H, D, pattern, weights=None, rows=None, fmts=(RGB8, F32X3, F64X3), what=""):
    """The fused call against rt_render_samples of the yardstick context: records and counts."""
    out = {}
    for fmt in fmts:
        want, st0 = yard.render_samples(cam, W, H, D, pattern, weights, rows, fmt)
        got, st = fused(r, cam, W, H, D, pattern, weights, rows, fmt)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert same_records(got, want, fmt), (what, fmt)
        assert counts(st) == counts(st0), (what, fmt)
        out[fmt] = (got, st)
    return out


@pytest.fixture(scope="module")
def yard():
    """The yardstick's own context: rt_render_samples never runs on the context under test."""
    import rt_hip

    r = rt_hip.Renderer(0)
    yield r
    r.close()


def _weights(S, seed=7):
    """Normalised-ish random weights with one negative and large, so some pixel sums are below zero."""
    w = np.random.default_rng(seed + S).uniform(0.0, 1.0, S) / S
    w[S // 2] = -1.5
    return [float(x) for x in w]


# ---- 1. the antialias pin ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["complex_97x61_d4", "simple_2x2_d10", "simple_1x1_d10"])
def test_antialias_pin(gpu_renderer, yard, name):
    import orc
    import rt_hip

    m = manifest()[name]
    W, H, D = m["width"], m["height"], m["depth"]
    sc = rt_hip.Scene.load(scene_path(m["scene"]))
    cam = sc.camera()
    pattern = rt_hip.grid_pattern(2)
    gpu_renderer.upload(sc)
    yard.upload(sc)
    yard.set_antialias(4)
    try:
        want = bytes(yard.render(cam, W, H, D)[0])
    finally:
        yard.set_antialias(1)
    oracle, _, _ = orc.OracleScene(scene_path(m["scene"])).render_aa(W, H, D, samples=4, threads=4)
    assert want == oracle
    got = check_equal(gpu_renderer, yard, cam, W, H, D, pattern, what=name)
    rgb, st = got[RGB8]
    assert rgb.tobytes() == want
    assert st.rays == 4 * W * H
    assert np.isnan(got[F64X3][0]).any() == (name == "simple_1x1_d10")  # W - 1 = 0: NaN rays


# ---- 2. rows -------------------------------------------------------------------------------------------
ROWS_W, ROWS_H, ROWS_D = 37, 21, 4


def _rows_cases():
    import rt_hip

    return [rt_hip.rows_for_shard(ROWS_H, 8, k, 3) for k in range(3)] + [rt_hip.rt_rows(3, 1, 2, 7), None]


@pytest.mark.parametrize("weighted", [False, True], ids=["box", "weighted"])
@pytest.mark.parametrize("case", range(5), ids=["shard0", "shard1", "shard2", "rows3127", "full"])
def test_rows(gpu_renderer, yard, case, weighted):
    import rt_hip

    sc = rt_hip.Scene.load(scene_path("complex"))
    cam = sc.camera()
    gpu_renderer.upload(sc)
    yard.upload(sc)
    rows = _rows_cases()[case]
    pattern = rt_hip.grid_pattern(3)
    w = _weights(9) if weighted else None
    got = check_equal(gpu_renderer, yard, cam, ROWS_W, ROWS_H, ROWS_D, pattern, w, rows, what=(case, weighted))
    count = rows.count if rows is not None else ROWS_H
    real = real_rows(rows, ROWS_H) if rows is not None else ROWS_H
    assert (real < count) == (case == 2)  # 21 rows in bands of 8: the third shard ends in padding rows
    for fmt, (rec, st) in got.items():
        assert st.rays == 9 * ROWS_W * real  # padding rows are not traced
        assert (rec.reshape(count, -1)[real:].view(np.uint8) == 0).all()  # and are zero bytes
    if weighted:
        assert got[RGB8][1].negative_clamped > 0 and got[F64X3][1].negative_clamped == 0


# ---- 3. pixel -> (row, column) ---------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 5), (63, 3), (64, 3), (65, 3), (129, 2)])
def test_pixel_to_row_and_column(gpu_renderer, yard, W, H):
    import rt_hip

    sc = rt_hip.Scene.load(scene_path("complex"))
    cam = sc.camera()
    gpu_renderer.upload(sc)
    yard.upload(sc)
    for S in (1, 2, 5, 64):
        pattern = rt_hip.grid_pattern(8)[:S]
        for D in (1, 4):
            check_equal(gpu_renderer, yard, cam, W, H, D, pattern, what=(W, H, S, D))
    check_equal(gpu_renderer, yard, cam, W, H, 4, rt_hip.grid_pattern(8)[:5], _weights(5), what=(W, H, "weighted"))


# ---- 4. offsets ----------------------------------------------------------------------------------------
def test_offsets_that_are_not_finite(gpu_renderer, yard):
    import rt_hip

    sc = rt_hip.Scene.load(scene_path("complex"))
    gpu_renderer.upload(sc)
    yard.upload(sc)
    pattern = [(0.25, float("nan")), (float("inf"), 0.5), (-1.5, 2.0)]
    rows = rt_hip.rows_for_shard(ROWS_H, 8, 2, 3)
    for rw in (None, rows):
        got = check_equal(gpu_renderer, yard, sc.camera(), ROWS_W, ROWS_H, ROWS_D, pattern, rows=rw, what="nan pattern")
        real = real_rows(rw, ROWS_H) if rw is not None else ROWS_H
        assert np.isnan(got[F64X3][0][:real * ROWS_W]).all()  # every pixel has a NaN sample
        assert (got[RGB8][0][:real * ROWS_W] == 255).all()
    # without the two bad samples the pixels are finite: the negative offset alone is an ordinary ray
    got = check_equal(gpu_renderer, yard, sc.camera(), ROWS_W, ROWS_H, ROWS_D, pattern[2:], fmts=(F64X3,))
    assert np.isfinite(got[F64X3][0]).all()


def test_single_sample_keeps_minus_zero(gpu_renderer):
    """One unweighted (0, 0) sample is rt_trace_radiance of rt_camera_rays, bit for bit: a hit of
    reflectivity > 1 with no depth left stores col * (1 - refl), -0.0 for a zero channel."""
    import material_cases as mc
    import rt_hip
    import torch

    text = mc.text("refl_above_one_s01", "dense").replace("0.9 0.2 0.2", "0.9 0 0.2")  # sphere A: no green
    assert text != mc.text("refl_above_one_s01", "dense")
    sc = rt_hip.Scene.parse(text)
    cam = sc.camera()
    W, H = 64, 48
    gpu_renderer.upload(sc)
    rays = torch.zeros((W * H, 8), dtype=torch.float64, device="cuda:0")
    want = torch.zeros((W * H, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    gpu_renderer.camera_rays(cam, W, H, None, rays.data_ptr())
    gpu_renderer.trace_radiance_device(rays.data_ptr(), W * H, 1, F64X3, want.data_ptr())
    gpu_renderer.radiance_stats()
    want = want.cpu().numpy()
    minus_zero = (want == 0.0) & np.signbit(want)
    assert minus_zero.any()
    got, st = fused(gpu_renderer, cam, W, H, 1, [(0.0, 0.0)], fmt=F64X3)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert st.rays == W * H
    one, _ = fused(gpu_renderer, cam, W, H, 1, [(0.0, 0.0)], weights=[1.0], fmt=F64X3)
    assert not np.signbit(one[minus_zero]).any()  # 0 + c * 1.0


# ---- 5. a second grid-stride trip ----------------------------------------------------------------------
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
    pattern = rt_hip.grid_pattern(2)[:2]
    got = check_equal(gpu_renderer, yard, sc.camera(), W, H, D, pattern, fmts=(RGB8, F64X3), what="mirrors")
    st = got[F64X3][1]
    assert st.rays == 2 * W * H and st.segments > 2 * st.rays  # every ray hits a mirror, the central ones bounce on


def test_second_trip_of_the_full_grid(gpu_renderer, yard):
    import rt_hip
    import torch

    sc = rt_hip.Scene.load(scene_path("simple"))
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 64 * 64
    W = 1025
    H = (lanes + 1024) // W + 1
    assert lanes < W * H < lanes + 3 * W
    gpu_renderer.upload(sc)
    yard.upload(sc)
    got = check_equal(gpu_renderer, yard, sc.camera(), W, H, 1, rt_hip.grid_pattern(2)[:2], fmts=(RGB8,), what="full grid")
    assert got[RGB8][1].rays == 2 * W * H


# ---- 6. asynchrony and isolation -----------------------------------------------------------------------
def test_two_calls_on_a_callers_stream_and_nothing_else_moves(yard):
    """Two calls back to back on a caller's stream, no host wait between them, into two buffers.
    The context is fresh and only ever makes the fused call after its other launches: nothing public
    reports the size of the radiance family's ray staging (rt_get_info's scratch_bytes covers the
    render scratch only), so instead of that size this checks that such a context -- whose staging
    was never allocated -- renders correctly, and that every report of the other families is unchanged."""
    import rt_hip
    import torch

    sc = rt_hip.Scene.load(scene_path("complex"))
    cam = sc.camera()
    W, H, D = ROWS_W, ROWS_H, ROWS_D
    n = W * H
    yard.upload(sc)
    p2, p3 = rt_hip.grid_pattern(2), rt_hip.grid_pattern(3)
    want2 = yard.render_samples(cam, W, H, D, p2)[0].tobytes()
    want3, st3 = yard.render_samples(cam, W, H, D, p3, _weights(9), None, F64X3)
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
        before = (r.stats().as_dict(), r.trace_stats().as_dict(), r.path_stats().as_dict(), r.info().launches)

        a = torch.full((n * 3 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        b = torch.full((n * 24 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        r.set_stream(side.cuda_stream)
        r.render_samples_async(cam, W, H, D, p2, a.data_ptr())
        r.render_samples_async(cam, W, H, D, p3, b.data_ptr(), _weights(9), None, F64X3)
        side.synchronize()  # the one wait
        ha, hb = a.cpu().numpy(), b.cpu().numpy()
        assert ha[:n * 3].tobytes() == want2 and (ha[n * 3:] == 0xA5).all()
        assert same_bits(hb[:n * 24].view(np.float64).reshape(n, 3), want3).all() and (hb[n * 24:] == 0xA5).all()
        assert counts(r.radiance_stats()) == counts(st3)  # the most recent launch: the second call's

        after = (r.stats().as_dict(), r.trace_stats().as_dict(), r.path_stats().as_dict(), r.info().launches)
        for got_d, want_d in zip(after[:3], before[:3]):
            # the same launch's events read a second time: the runtime's float differs in its last digits
            assert got_d.pop("kernel_ms") == pytest.approx(want_d.pop("kernel_ms"), rel=1e-4)
        assert after == before
        assert r.kernel_times() == []
    finally:
        r.set_stream(None)
        r.close()


# ---- 7. variants ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _full_frame_product():
    """Case 2's full frame from rt_render_samples of the product library, once."""
    import rt_hip

    sc = rt_hip.Scene.load(scene_path("complex"))
    r = rt_hip.Renderer(0)
    try:
        r.upload(sc)
        out = {}
        for weighted in (False, True):
            for fmt in (RGB8, F64X3):
                rec, st = r.render_samples(sc.camera(), ROWS_W, ROWS_H, ROWS_D, rt_hip.grid_pattern(3),
                                           _weights(9) if weighted else None, None, fmt)
                rec.setflags(write=False)
                out[weighted, fmt] = (rec, counts(st))
    finally:
        r.close()
    return sc, out


def _check_full_frame(r, unculled=False):
    import rt_hip

    sc, want = _full_frame_product()
    for (weighted, fmt), (rec, cnt) in want.items():
        got, st = fused(r, sc.camera(), ROWS_W, ROWS_H, ROWS_D, rt_hip.grid_pattern(3),
                        _weights(9) if weighted else None, None, fmt)
        assert same_records(got, rec, fmt), (weighted, fmt)
        if unculled:
            assert st.unaccelerated == st.segments + st.shadow_rays > 0 and st.tests_cull == 0
            cnt = dict(cnt, unaccelerated=st.unaccelerated)
        assert counts(st) == cnt, (weighted, fmt)


def test_unculled_same_bytes(gpu_renderer):
    gpu_renderer.upload(_full_frame_product()[0])
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
        r.upload(_full_frame_product()[0])
        _check_full_frame(r)
        r.stats()  # raises on RT_ERR_CHECK
    finally:
        r.close()


# ---- 8. errors, with no launch -------------------------------------------------------------------------
def test_errors():
    import rt_hip
    import torch

    r = rt_hip.Renderer(0)
    L = r._L
    try:
        out = torch.zeros((4 * 4 * 24 + 16,), dtype=torch.uint8, device="cuda:0")
        op = out.data_ptr()
        off = (C.c_double * 130)()

        def call(cam, W, H, D, rows, offsets, S, weights, fmt, ptr):
            return L.rt_render_samples_async(r.handle, C.byref(cam) if cam is not None else None, W, H, D,
                                             C.byref(rows) if rows is not None else None, offsets, S, weights, fmt,
                                             C.c_void_p(ptr) if ptr else None)

        cam = rt_hip.Scene.load(scene_path("simple")).camera()
        assert call(cam, 4, 4, 3, None, off, 4, None, RGB8, op) == NO_SCENE
        assert call(cam, 4, 4, 3, rt_hip.rt_rows(1, 0, 1, 0), off, 4, None, RGB8, op) == 0  # no rows: before the scene
        sc = rt_hip.Scene.load(scene_path("simple"))
        r.upload(sc)
        cam = sc.camera()
        assert call(cam, 4, 4, rt_hip.RT_MAX_DEPTH + 1, None, off, 4, None, RGB8, op) == DEPTH
        rows = rt_hip.rt_rows
        bad = [
            # rt_render_samples' argument table
            lambda: L.rt_render_samples_async(None, C.byref(cam), 4, 4, 3, None, off, 4, None, RGB8, C.c_void_p(op)),
            lambda: call(None, 4, 4, 3, None, off, 4, None, RGB8, op),
            lambda: call(cam, 4, 4, 3, None, None, 4, None, RGB8, op),
            lambda: call(cam, 0, 4, 3, None, off, 4, None, RGB8, op),
            lambda: call(cam, 4, -1, 3, None, off, 4, None, RGB8, op),
            lambda: call(cam, 4, 4, 3, None, off, 0, None, RGB8, op),
            lambda: call(cam, 4, 4, 3, None, off, 65, None, RGB8, op),
            lambda: call(cam, 4, 4, 3, None, off, -1, None, RGB8, op),
            lambda: call(cam, 4, 4, 3, rows(0, 0, 1, 4), off, 4, None, RGB8, op),
            lambda: call(cam, 4, 4, 3, rows(1, 0, 0, 4), off, 4, None, RGB8, op),
            lambda: call(cam, 4, 4, 3, rows(1, -1, 1, 4), off, 4, None, RGB8, op),
            lambda: call(cam, 4, 4, 3, rows(1, 0, 1, -1), off, 4, None, RGB8, op),
            lambda: call(cam, 1 << 26, 4, 3, None, off, 64, None, RGB8, op),  # width * samples > 2^31-1
            lambda: call(cam, 4, 4, 3, None, off, 4, None, 3, op),
            lambda: call(cam, 4, 4, 3, None, off, 4, None, -1, op),
            lambda: call(cam, 4, 4, 0, None, off, 4, None, RGB8, op),
            # out_device
            lambda: call(cam, 4, 4, 3, None, off, 4, None, RGB8, 0),
            lambda: call(cam, 4, 4, 3, None, off, 4, None, RGB8, op + 8),
            lambda: call(cam, 4, 4, 3, None, off, 4, None, F64X3, op + 4),
            # rows->count * width > 2^31-1: one launch has at most that many pixels
            lambda: call(cam, 1 << 11, 1 << 20, 3, rows(1, 0, 1, 1 << 20), off, 1, None, RGB8, op),
            lambda: call(cam, 1 << 16, 1 << 15, 3, None, off, 1, None, RGB8, op),
        ]
        for i, f in enumerate(bad):
            assert f() == INVALID, i
        assert call(cam, 4, 4, 3, rows(1, 0, 1, 0), off, 4, None, RGB8, op) == 0  # count == 0: a no-op
        assert call(cam, 4, 4, 3, rows(1, 0, 1, 0), off, 4, None, RGB8, 0) == 0   # ... that reads no pointer
        st = r.radiance_stats()
        assert st.rays == 0 and st.kernel_ms == 0  # nothing was launched
        assert (out.cpu().numpy() == 0).all()
        # the report of a launch survives the failures and the no-ops behind it
        r.render_samples_async(cam, 4, 4, 3, rt_hip.grid_pattern(2), op)
        assert r.radiance_stats().rays == 64
        assert call(cam, 4, 4, 3, None, off, 4, None, RGB8, op + 8) == INVALID
        assert call(cam, 4, 4, 3, rows(1, 0, 1, 0), off, 4, None, RGB8, op) == 0
        pad = rows(1, 4, 1, 2)  # two rows below the image: a memset and no launch
        assert call(cam, 4, 4, 3, pad, off, 4, None, RGB8, op) == 0
        assert r.radiance_stats().rays == 64
        assert (out.cpu().numpy()[:2 * 4 * 3] == 0).all()
    finally:
        r.close()
