"""GPU: ray queries (rt_trace_rays / rt_trace_rays_async / rt_trace_stats /
rt_camera_rays, include/rt_hip.h) against tests/ray_ref.py, the numpy
restatement of sphere.h:26-59 and scene.h:41-61 that test_rays_host.py pins to
the oracle.  Every comparison covers all rays: t as bit patterns, sphere and
occluded exactly.

A scene's batch is generated once (ray_ref.gen_rays, seed 1, 4133 rays; its
reference hit share is asserted to lie in [0.25, 0.85]) and the smaller batches
are its first n rays, so the references are computed once per scene."""
import ctypes as C
import functools

import numpy as np
import pytest

import ray_ref
from conftest import golden_rgb, manifest, scene_path

pytestmark = pytest.mark.gpu

N_FULL = 4133  # 64 full waves and a ragged tail of 37 rays
SIZES = [1, 63, 64, 65, N_FULL]  # one lane, a partial wave, a full wave, a wave plus one, many workgroups
HIT_DTYPE = np.dtype([("t", np.float64), ("sphere", np.int32), ("occluded", np.int32)])


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class Batch:
    """A scene's rays with their reference answers (never modified afterwards)."""

    def __init__(self, scene, o, d, seed=1):
        self.scene = scene
        self.centers, self.radii = ray_ref.spheres_of(scene)
        self.o, self.d = o, d
        self.t, self.sphere = ray_ref.closest(o, d, self.centers, self.radii)
        self.tmax, self.cls = ray_ref.gen_tmax(seed + 100, self.t)
        self.occ = ray_ref.occluded(self.t, self.sphere, self.tmax)

    @property
    def hit_share(self):
        return float((self.sphere >= 0).mean())


@functools.lru_cache(maxsize=None)
def scene_batch(name, n=N_FULL, seed=1):
    import rt_hip

    sc = rt_hip.Scene.load(scene_path(name))
    centers, radii = ray_ref.spheres_of(sc)
    o, d = ray_ref.gen_rays(seed, n, centers, radii, tuple(sc.camera().position))
    b = Batch(sc, o, d, seed)
    # a degenerate batch must not pass silently
    assert 0.25 <= b.hit_share <= 0.85, b.hit_share
    assert sorted(set(b.cls.tolist())) == list(range(len(ray_ref.TMAX_CLASSES)))
    hitting = b.sphere >= 0
    assert float((b.occ[hitting] == 0).mean()) >= 0.10
    return b


def _query_region(scene):
    """The scene's bounds (spheres and lights) grown on every side by their own diagonal."""
    c, r = ray_ref.spheres_of(scene)
    pts_lo = [c - np.abs(r)[:, None]] + [np.array([scene.light(i)["position"]]) for i in range(scene.num_lights)]
    pts_hi = [c + np.abs(r)[:, None]] + pts_lo[1:]
    lo, hi = np.concatenate(pts_lo).min(axis=0), np.concatenate(pts_hi).max(axis=0)
    diag = float(np.sqrt(((hi - lo) ** 2).sum()))
    return lo - diag, hi + diag, diag


def unaccelerated(b, n):
    """Rays of the batch's first n that must take the every-sphere sweep: an
    origin outside the query region (or not finite), or a direction that is
    not finite once normalised."""
    rlo, rhi, _ = _query_region(b.scene)
    o, d = b.o[:n], ray_ref.normalize(b.d[:n])
    with np.errstate(invalid="ignore"):
        inside = ((o >= rlo) & (o <= rhi)).all(axis=1)
    return int((~(inside & np.isfinite(d).all(axis=1))).sum())


def check_parity(r, b, n):
    """Both modes on the first n rays of the batch, against the reference."""
    import rt_hip

    o, d, tmax = b.o[:n], b.d[:n], b.tmax[:n]
    t, s, occ, st = r.trace_rays(o, d, tmax, rt_hip.RT_QUERY_CLOSEST)
    assert np.array_equal(s, b.sphere[:n]), f"sphere: {int((s != b.sphere[:n]).sum())} of {n} differ"
    assert np.array_equal(_bits(t), _bits(b.t[:n])), f"t: {int((_bits(t) != _bits(b.t[:n])).sum())} of {n} differ"
    assert np.array_equal(occ, b.occ[:n]), f"occluded: {int((occ != b.occ[:n]).sum())} of {n} differ"
    assert (st.rays, st.hits) == (n, int((b.sphere[:n] >= 0).sum()))
    t2, s2, occ2, st2 = r.trace_rays(o, d, tmax, rt_hip.RT_QUERY_OCCLUDED)
    assert np.array_equal(occ2, b.occ[:n]), f"occluded mode: {int((occ2 != b.occ[:n]).sum())} of {n} differ"
    assert np.array_equal(occ2, occ)  # the two modes agree
    assert np.array_equal(_bits(t2), _bits(np.full(n, 1e20))) and (s2 == -1).all()
    assert (st2.rays, st2.hits) == (n, int(b.occ[:n].sum()))
    assert st.rays_unaccelerated == st2.rays_unaccelerated == unaccelerated(b, n)
    return st, st2


# ---- 1. parity --------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["simple", "medium", "complex", "synth200"])
def test_parity(gpu_renderer, name, n):
    b = scene_batch(name)
    gpu_renderer.upload(b.scene)
    check_parity(gpu_renderer, b, n)


# ---- 2. a scene above kBvhAlwaysAbove: every lane walks the BVH -----------------
def test_large_scene(gpu_renderer):
    b = scene_batch("synth10k", 2048)
    assert b.scene.num_spheres == 10000
    gpu_renderer.upload(b.scene)
    st, _ = check_parity(gpu_renderer, b, 2048)
    assert st.rays_unaccelerated == 0
    assert st.tests_exact < 2048 * 10000 // 20  # the walk, not a sweep over the spheres


# ---- 3. edge rays -----------------------------------------------------------
TWO_SPHERES = "sphere 0 0 -5 1 1 0 0 0 1 10\nsphere 0 0 5 1 0 1 0 0 1 10\nlight 3 4 0 1 1 1 1\ncamera 0 0 0 0 0 -1 60\n"


def test_edge_rays(gpu_renderer):
    import rt_hip

    sc = rt_hip.Scene.parse(TWO_SPHERES)
    rlo, rhi, diag = _query_region(sc)
    nan, inf = float("nan"), float("inf")
    eps = 1e-6 * diag
    rays = [  # origin, direction, expected to take the every-sphere sweep
        ((1, 0, 0), (0, 0, -1), False),           # tangent to sphere 0 at t = 5 and, behind, to sphere 1 at t = -5
        ((1, 0, 0), (0, 0, -7.5), False),         # the same, direction not normalised
        ((-1, 0, 0), (0, 0, 1), False),           # the other way: sphere 0 is the one behind
        ((0, 0, 0), (0, 0, 0), True),             # zero direction
        ((nan, 0, 0), (0, 0, -1), True),          # NaN origin component
        ((0, inf, 0), (0, 0, -1), True),          # infinite origin component
        ((0, 0, 0), (0, nan, -1), True),          # NaN direction
        ((0, 0, 0), (inf, 0, -1), True),          # infinite direction
        ((0, 0, -5 - 1e6), (0, 0, 1), True),      # 1e6 from sphere 0, aimed at it
        ((0, 0, -5 - 1e12), (0, 0, 1), True),     # 1e12 from it
        ((0.25, 0.5, rhi[2] - eps), (-0.25, -0.5, -5 - (rhi[2] - eps)), False),  # just inside R, aimed at sphere 0
        ((0.25, 0.5, rhi[2] + eps), (-0.25, -0.5, -5 - (rhi[2] + eps)), True),   # just outside
        ((rlo[0] + eps, 0, 0), (1, 0.01, 0.2), False),
        ((rlo[0] - eps, 0, 0), (1, 0.01, 0.2), True),
        ((0, 0, 0), (0, 0, 1), False),            # origin between the spheres
        ((0, 0, -5.5), (0, 1, 0), False),         # origin inside sphere 0
        ((1, -3, -5), (0, 1, 0), False),          # tangent to sphere 0 alone: disc == 0, t = 3
    ]
    o = np.array([r[0] for r in rays], np.float64)
    d = np.array([r[1] for r in rays], np.float64)
    slow = int(sum(r[2] for r in rays))
    b = Batch(sc, o, d)
    # what the batch is for
    # the negative tangent root is kept (sphere.h:42-47) and is the smaller t
    assert (b.t[0], b.sphere[0]) == (-5.0, 1) and (b.t[1], b.sphere[1]) == (-5.0, 1)
    assert (b.t[2], b.sphere[2]) == (-5.0, 0) and (b.t[16], b.sphere[16]) == (3.0, 0)
    assert (b.sphere[3:8] == -1).all() and (b.t[3:8] == 1e20).all()
    assert b.sphere[8] == 0 and abs(b.t[8] - (1e6 - 1)) < 1e-3  # the 1e6 ray hits
    assert b.sphere[10] >= 0 and b.sphere[11] >= 0
    b.tmax = np.where(np.arange(len(rays)) % 2 == 0, np.inf, b.tmax)
    b.tmax[2] = -1.0  # a negative limit beaten by the negative tangent root
    b.occ = ray_ref.occluded(b.t, b.sphere, b.tmax)
    assert b.occ[2] == 1
    gpu_renderer.upload(sc)
    assert unaccelerated(b, len(rays)) == slow  # both far rays among them
    check_parity(gpu_renderer, b, len(rays))
    # no rays, and rays before any scene
    t, s, occ, st = gpu_renderer.trace_rays(np.zeros((0, 3)), np.zeros((0, 3)))
    assert len(t) == len(s) == len(occ) == 0 and st.rays == 0
    fresh = rt_hip.Renderer(0)
    try:
        with pytest.raises(rt_hip.RtError) as e:
            fresh.trace_rays(o, d)
        assert e.value.status == 5  # RT_ERR_NO_SCENE
        assert fresh.trace_stats().rays == 0
    finally:
        fresh.close()
    with pytest.raises(rt_hip.RtError) as e:
        gpu_renderer.trace_rays(o, d, mode=2)
    assert e.value.status == 1  # RT_ERR_INVALID_ARG


# ---- 4. work accounting -----------------------------------------------------------
def test_unculled_tests_every_sphere(gpu_renderer):
    import rt_hip

    b = scene_batch("complex")
    gpu_renderer.upload(b.scene)
    n, m = N_FULL, b.scene.num_spheres
    gpu_renderer.set_culling(False)
    try:
        t, s, occ, st = gpu_renderer.trace_rays(b.o, b.d, b.tmax, rt_hip.RT_QUERY_CLOSEST)
    finally:
        gpu_renderer.set_culling(True)
    assert st.tests_exact == n * m and st.rays_unaccelerated == n
    assert np.array_equal(s, b.sphere) and np.array_equal(_bits(t), _bits(b.t)) and np.array_equal(occ, b.occ)
    assert (st.rays, st.hits) == (n, int((b.sphere >= 0).sum()))


def _camera_rays(r, cam, W, H, rows=None):
    """rt_camera_rays into a torch buffer: (the buffer, its [count*W, 8] host copy)."""
    import torch

    count = rows.count if rows is not None else H
    buf = torch.full((count * W, 8), 7.0, dtype=torch.float64, device="cuda:0")
    r.camera_rays(cam, W, H, rows, buf.data_ptr())
    return buf, buf.cpu().numpy()


def test_camera_rays_take_the_accelerated_path(gpu_renderer):
    import rt_hip
    import torch

    W, H = 128, 72
    sc = rt_hip.Scene.load(scene_path("complex"))
    gpu_renderer.upload(sc)
    rays, host = _camera_rays(gpu_renderer, sc.camera(), W, H)
    hits = torch.zeros((W * H, 2), dtype=torch.float64, device="cuda:0")
    gpu_renderer.trace_rays_device(rays.data_ptr(), W * H, hits.data_ptr(), rt_hip.RT_QUERY_CLOSEST)
    st = gpu_renderer.trace_stats()
    ratio = st.tests_exact / (W * H * sc.num_spheres)
    print(f"complex {W}x{H} camera rays: tests_exact / (rays * spheres) = {ratio:.4f}")
    assert (st.rays, st.rays_unaccelerated) == (W * H, 0)  # the camera lies in the query region
    assert ratio <= 0.5  # a loose cap: the culled path ran
    c, rad = ray_ref.spheres_of(sc)
    t_ref, s_ref = ray_ref.closest(host[:, 0:3], host[:, 3:6], c, rad)
    got = hits.cpu().numpy().view(HIT_DTYPE).reshape(-1)
    assert np.array_equal(got["sphere"], s_ref) and np.array_equal(_bits(got["t"]), _bits(t_ref))
    assert st.hits == int((s_ref >= 0).sum())


# ---- 5. rt_camera_rays ------------------------------------------------------------
@pytest.mark.parametrize("W,H,shard", [(2, 2, None), (1, 1, None), (37, 19, None), (37, 19, (8, 1, 2))])
def test_camera_rays_equal_get_ray(gpu_renderer, W, H, shard):
    import rt_hip

    sc = rt_hip.Scene.load(scene_path("simple"))
    cam = sc.camera()
    rows = rt_hip.rows_for_shard(H, *shard) if shard else None
    _, got = _camera_rays(gpu_renderer, cam, W, H, rows)
    want = ray_ref.camera_rays(cam, W, H, rows)
    assert got.shape == want.shape
    # bit-equal; a NaN equals a NaN (its sign and payload are not arithmetic results)
    assert ((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all()
    if (W, H) == (1, 1):
        assert np.isnan(got[0, 3:6]).all()  # u = 0/0, as the simple_1x1_d10 golden
    if shard:
        pad = [k for k in range(rows.count) if (k // 8) * 8 * 2 + 8 + k % 8 >= H]
        assert pad and all((got.reshape(rows.count, W, 8)[k] == 0).all() for k in pad)


def test_camera_ray_misses_are_the_renderers_sky(gpu_renderer):
    """simple.txt at 64x48, depth 1: every pixel whose closest-hit query misses
    shows the sky colour (main.cpp:28-29) of its twice-normalised direction."""
    import orc
    import rt_hip

    W, H = 64, 48
    sc = rt_hip.Scene.load(scene_path("simple"))
    gpu_renderer.upload(sc)
    rgb, _ = gpu_renderer.render(sc.camera(), W, H, 1)
    img = np.frombuffer(bytes(rgb), np.uint8).reshape(H * W, 3)
    _, rays = _camera_rays(gpu_renderer, sc.camera(), W, H)
    t, s, _, st = gpu_renderer.trace_rays(rays[:, 0:3], rays[:, 3:6])
    miss = s < 0
    assert miss.mean() >= 0.25 and (~miss).mean() >= 0.25
    d2 = ray_ref.normalize(rays[:, 3:6])  # Ray() normalises get_ray's direction again
    tt = 0.5 * (d2[:, 1] + 1.0)
    sky = np.stack([1.0 * (1.0 - tt) + k * tt for k in (0.5, 0.7, 1.0)], axis=1)
    for i in np.flatnonzero(miss):
        assert tuple(img[i]) == tuple(orc.quantize(float(v)) for v in sky[i]), i


# ---- 6. separation from the renders -----------------------------------------------
def test_queries_leave_the_renders_alone():
    import rt_hip

    name = "complex_97x61_d4"
    m = manifest()[name]
    W, H, D = m["width"], m["height"], m["depth"]
    b = scene_batch("complex")
    r = rt_hip.Renderer(0)
    try:
        r.upload(b.scene)
        launches0 = r.info().launches
        r.kernel_times()
        rgb1, st1 = r.render(b.scene.camera(), W, H, D)
        check_parity(r, b, N_FULL)
        after = r.stats()  # still the render's
        for f in ("rays_primary", "rays_shadow", "rays_reflect", "tests_exact", "tests_cull", "kernel_ms"):
            assert getattr(after, f) == getattr(st1, f), f
        rgb2, st2 = r.render(b.scene.camera(), W, H, D)
        assert bytes(rgb1) == bytes(rgb2) == golden_rgb(name)
        assert (st2.rays_primary, st2.rays_shadow, st2.rays_reflect) == (st1.rays_primary, st1.rays_shadow,
                                                                         st1.rays_reflect)
        assert len(r.kernel_times()) == 2
        assert r.info().launches == launches0 + 2
    finally:
        r.close()


# ---- 7. the other BVH layouts (tuning build) -----------------------------------------
KNOB_SETS = {
    "always": {"RT_HIP_BVH_ALWAYS": "1"},
    "always_two_child": {"RT_HIP_BVH_ALWAYS": "1", "RT_HIP_BVH4": "0"},
    "always_stackless": {"RT_HIP_BVH_ALWAYS": "1", "RT_HIP_BVH_ORDERED": "0"},
    "no_bvh": {"RT_HIP_BVH": "0"},
}


@pytest.fixture(params=list(KNOB_SETS))
def query_layout_renderer(request, monkeypatch):
    import rt_hip

    for k, v in KNOB_SETS[request.param].items():
        monkeypatch.setenv(k, v)
    r = rt_hip.Renderer(0, variant="tuning")  # reads the knobs at rt_create
    yield r
    r.close()


def test_layouts(query_layout_renderer):
    b = scene_batch("complex")
    query_layout_renderer.upload(b.scene)
    check_parity(query_layout_renderer, b, N_FULL)


# ---- 8. the bounds-checked build --------------------------------------------------
def test_checked_build():
    import rt_hip

    r = rt_hip.Renderer(0, variant="check")
    try:
        for name, n in (("medium", N_FULL), ("synth10k", 2048)):
            b = scene_batch(name, n)
            r.upload(b.scene)
            check_parity(r, b, n)
        r.stats()  # raises on RT_ERR_CHECK
    finally:
        r.close()


# ---- 9. the device path -----------------------------------------------------------
def test_device_path_and_streams():
    import rt_hip
    import torch

    b = scene_batch("complex")
    n = N_FULL
    host_rays = np.zeros((n, 8), np.float64)
    host_rays[:, 0:3], host_rays[:, 3:6], host_rays[:, 6] = b.o, b.d, b.tmax
    r = rt_hip.Renderer(0)
    side = torch.cuda.Stream()
    try:
        r.upload(b.scene)
        want = {}
        for mode in (rt_hip.RT_QUERY_CLOSEST, rt_hip.RT_QUERY_OCCLUDED):
            t, s, occ, _ = r.trace_rays(b.o, b.d, b.tmax, mode)
            h = np.zeros(n, HIT_DTYPE)
            h["t"], h["sphere"], h["occluded"] = t, s, occ
            want[mode] = h.tobytes()
        assert torch.cuda.current_stream().cuda_stream == 0
        rays = torch.from_numpy(host_rays).to("cuda:0")  # filled on the legacy NULL stream
        for mode in (rt_hip.RT_QUERY_CLOSEST, rt_hip.RT_QUERY_OCCLUDED):
            hits = torch.zeros((n, 2), dtype=torch.float64, device="cuda:0")
            r.trace_rays_device(rays.data_ptr(), n, hits.data_ptr(), mode)
            assert hits.cpu().numpy().tobytes() == want[mode]  # read on the NULL stream, no host sync between
            assert r.trace_stats().rays == n
        r.set_stream(side.cuda_stream)
        for mode in (rt_hip.RT_QUERY_CLOSEST, rt_hip.RT_QUERY_OCCLUDED):
            with torch.cuda.stream(side):
                hits = torch.zeros((n, 2), dtype=torch.float64, device="cuda:0")
                r.trace_rays_device(rays.data_ptr(), n, hits.data_ptr(), mode)
                got = hits.cpu().numpy().tobytes()
            assert got == want[mode]
        # the synchronous call takes device memory too
        hits = torch.zeros((n, 2), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()  # the side stream is not ordered with the NULL stream's fill
        st = rt_hip.rt_query_stats()
        rc = r._L.rt_trace_rays(r.handle, rt_hip.RT_QUERY_CLOSEST, C.c_void_p(rays.data_ptr()), n,
                                C.c_void_p(hits.data_ptr()), 1, C.byref(st))
        assert rc == 0 and st.rays == n
        side.synchronize()
        assert hits.cpu().numpy().tobytes() == want[rt_hip.RT_QUERY_CLOSEST]
    finally:
        r.set_stream(None)
        r.close()
