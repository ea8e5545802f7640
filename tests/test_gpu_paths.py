"""GPU: path queries (rt_trace_paths / rt_trace_paths_async / rt_path_stats_get,
include/rt_hip.h) against tests/path_ref.py, the numpy restatement of trace_ray
that test_paths_host.py pins to the oracle-made goldens.  Every comparison
covers all records: floating-point fields as bit patterns, integers exactly.

A scene's batch is generated once (ray_ref.gen_rays, seed 1, 1061 rays) and the
smaller batches are its first n rays; the references are computed once per
(scene, n, depth) and never modified."""
import ctypes as C
import functools

import numpy as np
import pytest

import path_ref
import ray_ref
from conftest import golden_rgb, manifest, scene_path
from test_gpu_rays import KNOB_SETS, _query_region

pytestmark = pytest.mark.gpu

N_FULL = 1061  # 16 full waves and a ragged tail of 37 rays
SIZES = [1, 63, 64, 65, N_FULL]
FILL = 0xA5
TRACED, REFLECTS = 1, 2  # RT_VERTEX_*


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _scene(name):
    import rt_hip

    sc = rt_hip.Scene.load(scene_path(name))
    return sc, path_ref.SceneArrays(sc)


@functools.lru_cache(maxsize=None)
def _rays(name, n=N_FULL, seed=1):
    sc, sa = _scene(name)
    return ray_ref.gen_rays(seed, n, sa.centers, sa.radii, tuple(sc.camera().position))


@functools.lru_cache(maxsize=None)
def _ref(name, n, depth, total=N_FULL):
    o, d = _rays(name, total)
    return path_ref.trace_paths(o[:n], d[:n], depth, _scene(name)[1])


def level_counts(levels):
    return [int(lv["traced"].sum()) for lv in levels]


def check_records(levels, verts, surf, fill=None):
    """Every vertex of every level and every written surface against the checker.
    `fill`: the byte the surface buffer held before the call (untraced levels keep it);
    None: the buffer was zeros (Renderer.trace_paths)."""
    depth = len(levels)
    assert verts.shape[0] == depth
    for k, lv in enumerate(levels):
        v = verts[k]
        flags = np.where(lv["traced"], TRACED | np.where(lv["reflects"], REFLECTS, 0), 0)
        assert np.array_equal(v["sphere"], lv["sphere"]), (k, int((v["sphere"] != lv["sphere"]).sum()))
        assert np.array_equal(_bits(v["t"]), _bits(lv["t"])), (k, int((_bits(v["t"]) != _bits(lv["t"])).sum()))
        assert np.array_equal(v["flags"], flags), (k, int((v["flags"] != flags).sum()))
        assert np.array_equal(v["shadowed"], lv["shadowed"]), (k, int((v["shadowed"] != lv["shadowed"]).sum()))
        assert (v["reserved"] == 0).all(), k
        if surf is None:
            continue
        tr = lv["traced"]
        for f in ("dir", "hit", "normal", "view"):
            got, want = _bits(surf[k][f][tr]), _bits(lv[f][tr])
            # a NaN equals a NaN (its sign and payload are not arithmetic results)
            same = (got == want) | (np.isnan(surf[k][f][tr]) & np.isnan(lv[f][tr]))
            assert same.all(), (k, f, int((~same).sum()))
        raw = np.ascontiguousarray(surf[k][~tr]).view(np.uint8)
        assert (raw == (0 if fill is None else fill)).all(), k  # untraced: not touched


def check_stats(st, levels, sa, unaccel=0):
    n, segments, hits, shadow = path_ref.counts(levels, sa)
    assert (st.rays, st.segments, st.hits, st.shadow_rays) == (n, segments, hits, shadow)
    if unaccel is not None:
        assert st.unaccelerated == unaccel


def check_parity(r, name, n, depth, total=N_FULL, unaccel=0):
    """Both forms (with and without surfaces) on the first n rays of the scene's batch."""
    sa = _scene(name)[1]
    o, d = _rays(name, total)
    levels = _ref(name, n, depth, total)
    verts, surf, st = r.trace_paths(o[:n], d[:n], depth, surfaces=True)
    check_records(levels, verts, surf)
    check_stats(st, levels, sa, unaccel)
    verts2, none, st2 = r.trace_paths(o[:n], d[:n], depth)
    assert none is None and verts2.tobytes() == verts.tobytes()
    check_stats(st2, levels, sa, unaccel)
    assert (st2.tests_exact, st2.tests_cull) == (st.tests_exact, st.tests_cull)
    return st


# ---- 1. parity ------------------------------------------------------------------
# The batch condition at depth 4: some rays reach level 3 and some end at each
# earlier level.  simple.txt has one reflective sphere, and a ray that leaves a
# sphere cannot come back to it, so no path in it is longer than two segments:
# there the condition is that both of those lengths occur.
LONGEST = {"simple": 2, "medium": 4, "complex": 4, "synth200": 4}


@pytest.mark.parametrize("name", list(LONGEST))
def test_batch_is_not_degenerate(name):
    sa = _scene(name)[1]
    assert int((sa.refl > 0).sum()) >= (1 if name == "simple" else 2)
    c = level_counts(_ref(name, N_FULL, 4)) + [0]
    ends = [c[k] - c[k + 1] for k in range(4)]  # paths whose last traced level is k
    assert all(e > 0 for e in ends[:LONGEST[name]]), ends
    assert all(e == 0 for e in ends[LONGEST[name]:]), ends
    hits0 = float((_ref(name, N_FULL, 4)[0]["sphere"] >= 0).mean())
    assert 0.25 <= hits0 <= 0.85, hits0


@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(LONGEST))
def test_parity(gpu_renderer, name, n, depth):
    gpu_renderer.upload(_scene(name)[0])
    check_parity(gpu_renderer, name, n, depth)


# ---- 2. untouched and sentinel ----------------------------------------------------
def test_untouched_and_sentinel(gpu_renderer):
    import rt_hip
    import torch

    name, n, depth = "complex", N_FULL, 4
    sc, sa = _scene(name)
    o, d = _rays(name)
    levels = _ref(name, n, depth)
    assert 0 < level_counts(levels)[3] < level_counts(levels)[1] < n
    gpu_renderer.upload(sc)
    host = np.zeros((n, 8))
    host[:, 0:3], host[:, 3:6] = o[:n], d[:n]
    rays = torch.from_numpy(host).to("cuda:0")
    vbytes, sbytes, guard = depth * n * 32, depth * n * 96, 4096
    vbuf = torch.full((vbytes + guard,), FILL, dtype=torch.uint8, device="cuda:0")
    sbuf = torch.full((sbytes + guard,), FILL, dtype=torch.uint8, device="cuda:0")
    gpu_renderer.trace_paths_device(rays.data_ptr(), n, depth, vbuf.data_ptr(), sbuf.data_ptr())
    st = gpu_renderer.path_stats()
    vh, sh = vbuf.cpu().numpy(), sbuf.cpu().numpy()
    verts = vh[:vbytes].view(rt_hip.VERTEX_DTYPE).reshape(depth, n)
    surf = sh[:sbytes].view(rt_hip.SURFACE_DTYPE).reshape(depth, n)
    check_records(levels, verts, surf, fill=FILL)  # every vertex overwritten, untraced surfaces keep the fill
    check_stats(st, levels, sa)
    assert (vh[vbytes:] == FILL).all() and (sh[sbytes:] == FILL).all()
    # surf = NULL: the guard placed after verts is untouched
    vbuf.fill_(FILL)
    gpu_renderer.trace_paths_device(rays.data_ptr(), n, depth, vbuf.data_ptr(), 0)
    vh2 = vbuf.cpu().numpy()
    assert vh2[:vbytes].tobytes() == vh[:vbytes].tobytes() and (vh2[vbytes:] == FILL).all()


# ---- 3. long and uneven chains ------------------------------------------------------
MIRRORS = ("sphere 0 0 -5 4 1 1 1 1 1 10\nsphere 0 0 5 4 1 1 1 1 1 10\nlight 3 4 0 1 1 1 1\n"
           "camera 0 0 0 0 0 -1 60\n")


def test_long_and_uneven_chains(gpu_renderer):
    import rt_hip

    sc = rt_hip.Scene.parse(MIRRORS)
    sa = path_ref.SceneArrays(sc)
    assert (sa.refl == 1.0).all()
    D = rt_hip.RT_MAX_DEPTH
    ang = np.linspace(0.0, 0.12, 65)  # ray 0 exactly along +z, the rest fanned in the x-z plane
    o = np.zeros((65, 3))
    d = np.stack([np.sin(ang), np.zeros(65), np.cos(ang)], axis=1)
    assert tuple(d[0]) == (0.0, 0.0, 1.0)
    levels = path_ref.trace_paths(o, d, D, sa)
    length = np.sum([lv["traced"] for lv in levels], axis=0)
    assert length[0] == D and len(set(length.tolist())) >= 5 and length.min() < 8  # uneven chains
    gpu_renderer.upload(sc)
    verts, surf, st = gpu_renderer.trace_paths(o, d, D, surfaces=True)
    assert (verts["flags"][:, 0] & TRACED).all()  # ray 0 is traced on all 64 levels
    check_records(levels, verts, surf)
    check_stats(st, levels, sa)
    with pytest.raises(rt_hip.RtError) as e:
        gpu_renderer.trace_paths(o, d, D + 1)
    assert e.value.status == 7  # RT_ERR_DEPTH
    with pytest.raises(rt_hip.RtError) as e:
        gpu_renderer.trace_paths(o, d, 0)
    assert e.value.status == 1  # RT_ERR_INVALID_ARG


# ---- 4. lights ----------------------------------------------------------------------
TWO = "sphere 0 0 -5 1 1 0 0 0.5 1 10\nsphere 0 0 5 1 0 1 0 0 1 10\n"
CAM = "camera 0 0 0 0 0 -1 60\n"


def _fan():
    """65 rays from the origin, about half towards each sphere, most of them hitting."""
    k = np.arange(65)
    x = (k - 32) / 32.0 * 0.22
    d = np.stack([x, 0.03 * np.cos(k), np.where(k % 2 == 0, -1.0, 1.0)], axis=1)
    return np.zeros((65, 3)), d


def _light_lines(positions):
    return "".join("light %r %r %r 1 1 1 1\n" % tuple(float(v) for v in p) for p in positions)


def _run_lights(r, text, o, d, depth=2):
    import rt_hip

    sc = rt_hip.Scene.parse(text)
    sa = path_ref.SceneArrays(sc)
    levels = path_ref.trace_paths(o, d, depth, sa)
    r.upload(sc)
    verts, surf, st = r.trace_paths(o, d, depth, surfaces=True)
    check_records(levels, verts, surf)
    rlo, rhi, _ = _query_region(sc)
    check_stats(st, levels, sa, unaccel=path_ref.unaccelerated(levels, o, sa, rlo, rhi))
    return levels, verts, st


def test_no_lights(gpu_renderer):
    o, d = _fan()
    levels, verts, st = _run_lights(gpu_renderer, TWO + CAM, o, d)
    assert (levels[0]["sphere"] >= 0).sum() >= 32
    assert (verts["shadowed"] == 0).all() and st.shadow_rays == 0 and st.hits > 0


def test_light_63_is_bit_63(gpu_renderer):
    o, d = _fan()
    rng = np.random.default_rng(5)
    pos = np.concatenate([rng.uniform(-6, 6, (63, 3)), [[3.0, 0.5, -5.0]]])  # the last one beside sphere 0
    levels, verts, st = _run_lights(gpu_renderer, TWO + _light_lines(pos) + CAM, o, d)
    hit = levels[0]["sphere"] >= 0
    bit63 = (levels[0]["shadowed"][hit] >> np.uint64(63)) & np.uint64(1)
    assert 0 < int(bit63.sum()) < int(hit.sum())  # some hits shadowed from light 63, some lit
    assert np.array_equal((verts[0]["shadowed"][hit] >> np.uint64(63)) & np.uint64(1), bit63)
    assert st.shadow_rays == 64 * st.hits


def test_65_lights_is_an_error(gpu_renderer):
    import rt_hip

    o, d = _fan()
    pos = np.random.default_rng(6).uniform(-6, 6, (65, 3))
    sc = rt_hip.Scene.parse(TWO + _light_lines(pos) + CAM)
    assert sc.num_lights == 65
    gpu_renderer.upload(sc)
    with pytest.raises(rt_hip.RtError) as e:
        gpu_renderer.trace_paths(o, d, 2)
    assert e.value.status == 1  # RT_ERR_INVALID_ARG
    t, s, _, _ = gpu_renderer.trace_rays(o, d)  # the scene itself is fine
    assert (s >= 0).sum() >= 32


def test_light_at_a_hit_point(gpu_renderer):
    """The ray along -z hits sphere 0 at (0, 0, -4) exactly; a light there gives
    in_shadow a NaN direction: not shadowed, as in the checker."""
    o, d = _fan()
    d[0] = (0.0, 0.0, -1.0)
    levels, verts, st = _run_lights(gpu_renderer, TWO + _light_lines([(0.0, 0.0, -4.0), (3.0, 4.0, 0.0)]) + CAM, o, d)
    assert tuple(levels[0]["hit"][0]) == (0.0, 0.0, -4.0) and levels[0]["sphere"][0] == 0
    assert int(verts[0]["shadowed"][0]) & 1 == 0
    assert st.unaccelerated == 1  # that shadow query took the every-sphere sweep
    assert (levels[0]["shadowed"] != 0).any()  # the light casts shadows elsewhere


# ---- 5. edge rays -------------------------------------------------------------------
def test_edge_rays(gpu_renderer):
    import rt_hip

    text = TWO + "light 3 4 0 1 1 1 1\n" + CAM
    sc = rt_hip.Scene.parse(text)
    sa = path_ref.SceneArrays(sc)
    rlo, rhi, diag = _query_region(sc)
    nan, inf = float("nan"), float("inf")
    eps = 1e-6 * diag
    rays = [  # origin, direction, level 0 takes the every-sphere sweep
        ((0, 0, 0), (0, 0, 0), True),             # zero direction
        ((0, 0, 0), (0, nan, -1), True),          # NaN direction
        ((0, 0, 0), (inf, 0, -1), True),          # infinite direction
        ((nan, 0, 0), (0, 0, -1), True),          # NaN origin component
        ((0, 0, -5 - 1e6), (0, 0, 1), True),      # far outside R, aimed at sphere 0
        ((0.25, 0.5, rhi[2] + eps), (-0.25, -0.5, -5 - (rhi[2] + eps)), True),   # just outside R
        ((0.25, 0.5, rhi[2] - eps), (-0.25, -0.5, -5 - (rhi[2] - eps)), False),  # just inside
        ((rlo[0] - eps, 0, 0), (1, 0.01, 0.2), True),
        ((0, 0, 0), (0.1, 0, -1), False),
        ((0, 0, -5.5), (0, 1, 0), False),         # origin inside sphere 0
    ]
    o = np.array([r[0] for r in rays], np.float64)
    d = np.array([r[1] for r in rays], np.float64)
    outside = int(sum(r[2] for r in rays))
    levels = path_ref.trace_paths(o, d, 3, sa)
    assert levels[0]["traced"].all() and (levels[0]["sphere"][:4] == -1).all()  # traced misses, never an error
    assert not levels[1]["traced"][:4].any() and levels[0]["sphere"][4] == 0 and levels[1]["traced"][4]
    want_slow = path_ref.unaccelerated(levels, o, sa, rlo, rhi)
    assert want_slow >= outside
    gpu_renderer.upload(sc)
    verts, surf, st = gpu_renderer.trace_paths(o, d, 3, surfaces=True)
    check_records(levels, verts, surf)
    check_stats(st, levels, sa, unaccel=want_slow)
    assert st.unaccelerated >= outside
    # no rays
    verts0, _, st0 = gpu_renderer.trace_paths(np.zeros((0, 3)), np.zeros((0, 3)), 3)
    assert verts0.shape == (3, 0) and st0.rays == 0
    # rays before any scene
    fresh = rt_hip.Renderer(0)
    try:
        with pytest.raises(rt_hip.RtError) as e:
            fresh.trace_paths(o, d, 3)
        assert e.value.status == 5  # RT_ERR_NO_SCENE
        assert fresh.path_stats().rays == 0
    finally:
        fresh.close()


def test_zero_sphere_scene(gpu_renderer):
    import rt_hip

    sc = rt_hip.Scene.parse("light 3 4 0 1 1 1 1\n" + CAM)
    assert sc.num_spheres == 0
    o, d = _fan()
    gpu_renderer.upload(sc)
    verts, surf, st = gpu_renderer.trace_paths(o, d, 3, surfaces=True)
    levels = path_ref.trace_paths(o, d, 3, sc)
    check_records(levels, verts, surf)
    assert (st.rays, st.segments, st.hits, st.shadow_rays) == (65, 65, 0, 0)


def test_unculled_same_bits(gpu_renderer):
    name, n, depth = "complex", N_FULL, 4
    sc, sa = _scene(name)
    levels = _ref(name, n, depth)
    _, segments, _, shadow = path_ref.counts(levels, sa)
    gpu_renderer.upload(sc)
    gpu_renderer.set_culling(False)
    try:
        st = check_parity(gpu_renderer, name, n, depth, unaccel=segments + shadow)
    finally:
        gpu_renderer.set_culling(True)
    assert st.unaccelerated == st.segments + st.shadow_rays
    assert st.tests_exact >= segments * sc.num_spheres and st.tests_cull == 0


# ---- 6. tied to the render --------------------------------------------------------------
def test_tied_to_the_render():
    import rt_hip
    import torch

    name = "complex_97x61_d4"
    m = manifest()[name]
    W, H, D = m["width"], m["height"], m["depth"]
    sc, sa = _scene(m["scene"])
    n = W * H
    r = rt_hip.Renderer(0)
    try:
        r.upload(sc)
        launches0 = r.info().launches
        r.kernel_times()
        rgb1, st1 = r.render(sc.camera(), W, H, D)
        rays = torch.zeros((n, 8), dtype=torch.float64, device="cuda:0")
        r.camera_rays(sc.camera(), W, H, None, rays.data_ptr())
        vbuf = torch.zeros((D * n * 32,), dtype=torch.uint8, device="cuda:0")
        sbuf = torch.zeros((D * n * 96,), dtype=torch.uint8, device="cuda:0")
        r.trace_paths_device(rays.data_ptr(), n, D, vbuf.data_ptr(), sbuf.data_ptr())
        st = r.path_stats()
        verts = vbuf.cpu().numpy().view(rt_hip.VERTEX_DTYPE).reshape(D, n)
        surf = sbuf.cpu().numpy().view(rt_hip.SURFACE_DTYPE).reshape(D, n)
        # the counts are the manifest's and the render's
        assert {"primary": st.rays, "reflect": st.segments - st.rays, "shadow": st.shadow_rays} == m["rays"]
        assert (st1.rays_primary, st1.rays_reflect, st1.rays_shadow) == (st.rays, st.segments - st.rays,
                                                                         st.shadow_rays)
        assert st.unaccelerated == 0
        # level 0 is the closest-hit query's answer
        hits = torch.zeros((n, 2), dtype=torch.float64, device="cuda:0")
        r.trace_rays_device(rays.data_ptr(), n, hits.data_ptr(), rt_hip.RT_QUERY_CLOSEST)
        h = hits.cpu().numpy().view(np.dtype([("t", np.float64), ("sphere", np.int32), ("occluded", np.int32)]))
        h = h.reshape(-1)
        assert np.array_equal(h["sphere"], verts[0]["sphere"]) and np.array_equal(_bits(h["t"]), _bits(verts[0]["t"]))
        # the checker's shading of the GPU's records is the golden image
        levels = [{"traced": (verts[k]["flags"] & TRACED) != 0, "sphere": verts[k]["sphere"],
                   "reflects": (verts[k]["flags"] & REFLECTS) != 0, "shadowed": verts[k]["shadowed"],
                   "dir": surf[k]["dir"], "hit": surf[k]["hit"], "normal": surf[k]["normal"], "view": surf[k]["view"]}
                  for k in range(D)]
        assert path_ref.quantize(path_ref.shade(levels, sa)).tobytes() == golden_rgb(name)
        # the renders are left alone
        after = r.stats()
        for f in ("rays_primary", "rays_shadow", "rays_reflect", "tests_exact", "tests_cull", "kernel_ms"):
            assert getattr(after, f) == getattr(st1, f), f
        assert r.trace_stats().rays == n  # the ray query's, not the path's
        rgb2, st2 = r.render(sc.camera(), W, H, D)
        assert bytes(rgb1) == bytes(rgb2) == golden_rgb(name)
        assert (st2.rays_primary, st2.rays_shadow, st2.rays_reflect) == (st1.rays_primary, st1.rays_shadow,
                                                                         st1.rays_reflect)
        assert len(r.kernel_times()) == 2
        assert r.info().launches == launches0 + 2
        assert r.path_stats().segments == st.segments  # still the path launch's
    finally:
        r.close()


# ---- 7. a scene above kBvhAlwaysAbove: every lane walks the BVH ---------------------------
def test_large_scene(gpu_renderer):
    sc, sa = _scene("synth10k")
    assert sc.num_spheres == 10000
    gpu_renderer.upload(sc)
    st = check_parity(gpu_renderer, "synth10k", 1024, 3, total=1024)
    levels = _ref("synth10k", 1024, 3, 1024)
    _, segments, _, shadow = path_ref.counts(levels, sa)
    assert level_counts(levels)[2] > 0
    assert st.unaccelerated == 0
    assert st.tests_exact < (segments + shadow) * 10000 // 20  # the walks, not a sweep over the spheres


# ---- 8. the other BVH layouts (tuning build) and the bounds-checked build -------------------
@pytest.fixture(params=list(KNOB_SETS))
def path_layout_renderer(request, monkeypatch):
    import rt_hip

    for k, v in KNOB_SETS[request.param].items():
        monkeypatch.setenv(k, v)
    r = rt_hip.Renderer(0, variant="tuning")  # reads the knobs at rt_create
    yield r
    r.close()


def test_layouts(path_layout_renderer):
    path_layout_renderer.upload(_scene("complex")[0])
    check_parity(path_layout_renderer, "complex", N_FULL, 4)


def test_checked_build():
    import rt_hip

    r = rt_hip.Renderer(0, variant="check")
    try:
        for name, n, depth in (("medium", N_FULL, 4), ("synth10k", 1024, 3)):
            r.upload(_scene(name)[0])
            check_parity(r, name, n, depth, total=n)
        r.stats()  # raises on RT_ERR_CHECK
    finally:
        r.close()


# ---- 9. the device path and streams ----------------------------------------------------------
def test_device_path_and_streams():
    import rt_hip
    import torch

    name, n, depth = "complex", N_FULL, 4
    sc, sa = _scene(name)
    o, d = _rays(name)
    host_rays = np.zeros((n, 8), np.float64)
    host_rays[:, 0:3], host_rays[:, 3:6] = o, d
    r = rt_hip.Renderer(0)
    side = torch.cuda.Stream()
    try:
        r.upload(sc)
        verts, surf, _ = r.trace_paths(o, d, depth, surfaces=True)
        check_records(_ref(name, n, depth), verts, surf)
        want_v, want_s = verts.tobytes(), surf.tobytes()
        assert torch.cuda.current_stream().cuda_stream == 0
        rays = torch.from_numpy(host_rays).to("cuda:0")  # filled on the legacy NULL stream
        vbuf = torch.zeros((depth * n * 32,), dtype=torch.uint8, device="cuda:0")
        sbuf = torch.zeros((depth * n * 96,), dtype=torch.uint8, device="cuda:0")
        r.trace_paths_device(rays.data_ptr(), n, depth, vbuf.data_ptr(), sbuf.data_ptr())
        assert vbuf.cpu().numpy().tobytes() == want_v  # read on the NULL stream, no host sync between
        assert sbuf.cpu().numpy().tobytes() == want_s
        assert r.path_stats().rays == n
        r.set_stream(side.cuda_stream)
        with torch.cuda.stream(side):
            vbuf2 = torch.zeros((depth * n * 32,), dtype=torch.uint8, device="cuda:0")
            r.trace_paths_device(rays.data_ptr(), n, depth, vbuf2.data_ptr(), 0)
            got = vbuf2.cpu().numpy().tobytes()
        assert got == want_v
        # the synchronous call takes device memory too
        vbuf3 = torch.zeros((depth * n * 32,), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()  # the side stream is not ordered with the NULL stream's fill
        st = rt_hip.rt_path_stats()
        rc = r._L.rt_trace_paths(r.handle, C.c_void_p(rays.data_ptr()), n, depth, C.c_void_p(vbuf3.data_ptr()), None,
                                 1, C.byref(st))
        assert rc == 0 and st.rays == n
        side.synchronize()
        assert vbuf3.cpu().numpy().tobytes() == want_v
    finally:
        r.set_stream(None)
        r.close()
