"""GPU: radiance queries (rt_trace_radiance / rt_trace_radiance_async /
rt_radiance_stats_get, include/rt_hip.h), pinned four ways:

 A. to the goldens (RGB8 bytes and ray counts) and to the render kernels' own
    unquantised framebuffers for the same camera rays, with no tolerance;
 B. to the oracle's fp64 framebuffer on the scenes without pow rounding
    (test_radiance_host.py pins the checker to them first and names the cases);
 C. to tests/path_ref.py for arbitrary rays, within 1 per RGB8 channel (glibc's
    pow against the device's: the project's bar for fractional powers);
 D. at the edges: the lights-over-lanes pass, the reflection stack, the
    grid-stride loop, bad rays, culling off, the other library variants, the
    device path and the argument errors.

Every reference is computed once per process and never modified."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import material_cases as mc
import path_ref
import query_cases as qc
import ray_ref
from conftest import golden_rgb, manifest, scene_path
from test_gpu_paths import CAM, MIRRORS, N_FULL, SIZES, TWO, _fan, _light_lines, _rays, _ref, _scene
from test_gpu_rays import KNOB_SETS, _query_region
from test_radiance_host import F64_KEPT, same_values

pytestmark = pytest.mark.gpu

RGB8, F32X3, F64X3 = 0, 1, 2  # RT_FB_*
RECORD = {RGB8: (np.uint8, 3), F32X3: (np.float32, 12), F64X3: (np.float64, 24)}


def check_counts(st, levels, sa, unaccel=0):
    n, segments, hits, shadow = path_ref.counts(levels, sa)
    assert (st.rays, st.segments, st.hits, st.shadow_rays) == (n, segments, hits, shadow)
    if unaccel is not None:
        assert st.unaccelerated == unaccel


def check_pm1(got, want, what):
    """RGB8 within 1 per channel; prints the number of channels that differ."""
    d = np.abs(np.asarray(got, np.int16) - np.asarray(want, np.int16))
    print("%s: %d of %d channels differ, %d by 2 or more" % (what, int((d > 0).sum()), d.size, int((d > 1).sum())))
    assert int((d > 1).sum()) == 0, what


def device_radiance(r, rays, n, depth, fmt):
    """rt_trace_radiance_async on a torch buffer of rt_ray records: (numpy [n, 3], stats)."""
    import torch

    dtype, size = RECORD[fmt]
    out = torch.zeros((n * size + 16,), dtype=torch.uint8, device="cuda:0")
    r.trace_radiance_device(rays.data_ptr(), n, depth, fmt, out.data_ptr())
    st = r.radiance_stats()
    return out.cpu().numpy()[:n * size].view(dtype).reshape(n, 3), st


# ---- A. the goldens and the render ----------------------------------------------------------------
FIXTURES = ["complex_97x61_d4", "simple_2x2_d10", "simple_1x1_d10", "mirrorfrac_320x240_d6", "synth10k_384x216_d6"]


@pytest.mark.parametrize("name", FIXTURES)
def test_tied_to_the_goldens_and_the_render(name):
    import rt_hip
    import torch

    m = manifest()[name]
    W, H, D = m["width"], m["height"], m["depth"]
    sc = rt_hip.Scene.load(scene_path(m["scene"]))
    n = W * H
    r, r2 = rt_hip.Renderer(0), rt_hip.Renderer(0)
    try:
        r.upload(sc)
        r2.upload(sc)
        # what the context's other launches report, before
        rgb1, st1 = r.render(sc.camera(), W, H, D)
        assert bytes(rgb1) == golden_rgb(name)
        rays = torch.zeros((n, 8), dtype=torch.float64, device="cuda:0")
        r.camera_rays(sc.camera(), W, H, None, rays.data_ptr())
        k = min(n, 64)
        hits = torch.zeros((k, 2), dtype=torch.float64, device="cuda:0")
        r.trace_rays_device(rays.data_ptr(), k, hits.data_ptr())
        verts = torch.zeros((D * k * 32,), dtype=torch.uint8, device="cuda:0")
        r.trace_paths_device(rays.data_ptr(), k, D, verts.data_ptr())
        before = (r.stats().as_dict(), r.trace_stats().as_dict(), r.path_stats().as_dict(), r.info().launches)
        assert len(r.kernel_times()) == 1 and before[1]["rays"] == k and before[2]["rays"] == k
        assert r.radiance_stats().as_dict() == rt_hip.rt_radiance_stats().as_dict()  # zeros before the first

        # RGB8: the golden's bytes and the manifest's counts
        rgb, st = device_radiance(r, rays, n, D, RGB8)
        assert rgb.tobytes() == golden_rgb(name)
        assert {"primary": st.rays, "reflect": st.segments - st.rays, "shadow": st.shadow_rays} == m["rays"]
        assert (st1.rays_primary, st1.rays_reflect, st1.rays_shadow) == (st.rays, st.segments - st.rays, st.shadow_rays)
        assert st.negative_clamped == 0
        # every-sphere sweeps: none, except for a camera ray whose direction is not finite (W - 1 = 0
        # divides 0 by 0), which the acceleration rule of rt_trace_rays sends there
        host_rays = rays.cpu().numpy()
        bad = int((~np.isfinite(host_rays[:, 3:6]).all(axis=1)).sum())
        assert bad == (1 if name == "simple_1x1_d10" else 0)
        assert st.unaccelerated == bad

        # F64X3 / F32X3: the render's own framebuffers of a second context, as values, no tolerance
        for fmt, tdtype in ((F64X3, torch.float64), (F32X3, torch.float32)):
            fb = torch.full((n * 3,), float("nan"), dtype=tdtype, device="cuda:0")
            torch.cuda.synchronize()  # the fill (torch's stream) lands before the tile
            r2.render_tile(sc.camera(), W, H, D, 0, 0, W, H, fmt, fb.data_ptr())
            r2.stats()
            want = fb.cpu().numpy().reshape(H, W, 3)[::-1].reshape(n, 3)  # j = 0 is the bottom row
            got, stf = device_radiance(r, rays, n, D, fmt)
            same = same_values(got, want)
            assert same.all(), (fmt, int((~same).sum()))
            assert np.isnan(want).any() == (name == "simple_1x1_d10")
            assert stf.negative_clamped == 0 and (stf.rays, stf.segments, stf.shadow_rays) == (st.rays, st.segments,
                                                                                                  st.shadow_rays)
        # the context's other launches are left alone
        after = (r.stats().as_dict(), r.trace_stats().as_dict(), r.path_stats().as_dict(), r.info().launches)
        assert after == before
        assert r.kernel_times() == []
        rgb2, st2 = r.render(sc.camera(), W, H, D)
        assert bytes(rgb2) == bytes(rgb1)
        assert len(r.kernel_times()) == 1 and r.info().launches == before[3] + 1
        assert r.radiance_stats().segments == st.segments  # still the radiance launch's
    finally:
        r.close()
        r2.close()


# ---- B. the oracle in fp64 ------------------------------------------------------------------------
@pytest.mark.parametrize("case", F64_KEPT)
def test_oracle_fp64(gpu_renderer, case):
    import rt_hip
    import torch

    W, H, D = mc.F64_SHAPE
    n = W * H
    sc = rt_hip.Scene.parse(mc.text(case, "dense"))
    want_rgb, counts, fb = mc.oracle(case, "dense", W, H, D)
    gpu_renderer.upload(sc)
    rays = torch.zeros((n, 8), dtype=torch.float64, device="cuda:0")
    gpu_renderer.camera_rays(sc.camera(), W, H, None, rays.data_ptr())
    got, st = device_radiance(gpu_renderer, rays, n, D, F64X3)
    same = same_values(got, fb.reshape(n, 3))
    assert same.all(), int((~same).sum())
    assert st.negative_clamped == 0  # the unquantised formats clamp nothing
    rgb, st8 = device_radiance(gpu_renderer, rays, n, D, RGB8)
    assert rgb.tobytes() == want_rgb
    assert st8.negative_clamped == counts["negative"]
    assert (st8.negative_clamped > 0) == (case in mc.F64_EXPECTS_NEGATIVE)
    assert (st8.rays, st8.segments - st8.rays, st8.shadow_rays) == (counts["primary"], counts["reflect"],
                                                                  counts["shadow"])


# ---- C. arbitrary rays against path_ref --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _colour(name, n, depth, total=N_FULL):
    c = path_ref.shade(_ref(name, n, depth, total), _scene(name)[1])
    c.setflags(write=False)
    return c


@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["simple", "medium", "complex", "synth200"])
def test_parity(gpu_renderer, name, n, depth):
    sc, sa = _scene(name)
    o, d = _rays(name)
    gpu_renderer.upload(sc)
    rgb, st = gpu_renderer.trace_radiance(o[:n], d[:n], depth, RGB8)
    assert rgb.shape == (n, 3) and rgb.dtype == np.uint8
    check_pm1(rgb, path_ref.quantize(_colour(name, n, depth)), "%s n=%d depth=%d" % (name, n, depth))
    check_counts(st, _ref(name, n, depth), sa)
    assert st.negative_clamped == 0


# ---- D. edges ----------------------------------------------------------------------------------------
# -- the lights-over-lanes lattice, shininess 1: pow(x, 1) is x, so every bit is the checker's
def _chunks(sa, size=path_ref.MAX_LIGHTS):
    """sa's lights in runs of at most 64 (path_ref's shadow masks have 64 bits)."""
    out = []
    for l0 in range(0, max(sa.lpos.shape[0], 1), size):
        part = copy.copy(sa)
        part.lpos, part.lcol = sa.lpos[l0:l0 + size], sa.lcol[l0:l0 + size]
        out.append(part)
    return out


def shade_any(o, d, depth, sa):
    """path_ref.shade for a scene of any number of lights: (colours, the levels of the first 64 lights, the
    hits x lights of all).  The geometry does not depend on the lights, so each run of 64 gets its own
    trace_paths (the same levels, that run's shadow masks); Scene::shade's sum then runs over all the runs
    in file order, with path_ref.shade's expressions."""
    parts = _chunks(sa)
    runs = [path_ref.trace_paths(o, d, depth, p) for p in parts]
    n = runs[0][0]["traced"].shape[0]
    below = np.zeros((n, 3))
    with np.errstate(all="ignore"):
        for k in reversed(range(depth)):
            lv = runs[0][k]
            col = np.zeros((n, 3))
            tr, s = lv["traced"], lv["sphere"]
            miss = np.flatnonzero(tr & (s < 0))
            st = 0.5 * (lv["dir"][miss, 1] + 1.0)
            col[miss] = np.ones((1, 3)) * (1.0 - st)[:, None] + np.array([[0.5, 0.7, 1.0]]) * st[:, None]
            h = np.flatnonzero(tr & (s >= 0))
            if h.size:
                si = s[h]
                point, normal, view = lv["hit"][h], lv["normal"][h], lv["view"][h]
                mcol, refl, shin = sa.color[si], sa.refl[si], sa.shin[si]
                color = sa.ambient[None, :] * mcol
                for part, run in zip(parts, runs):
                    shadowed = run[k]["shadowed"][h]
                    for l in range(part.lpos.shape[0]):
                        lit = ((shadowed >> np.uint64(l)) & np.uint64(1)) == 0
                        light_dir = ray_ref.normalize(part.lpos[l][None, :] - point)
                        ndl = path_ref.max0(path_ref.dot(normal, light_dir))
                        diffuse = (mcol * (1.0 - refl)[:, None]) * ndl[:, None]
                        v = light_dir * -1.0
                        reflect_dir = v - (normal * 2.0) * path_ref.dot(v, normal)[:, None]
                        rdv = path_ref.max0(path_ref.dot(reflect_dir, view))
                        spec = np.zeros(h.size)
                        spec[lit] = path_ref._pow(rdv[lit], shin[lit]).astype(np.float64)
                        specular = (part.lcol[l][None, :] * path_ref.K_SPECULAR) * spec[:, None]
                        color = np.where(lit[:, None], (specular + diffuse) + color, color)
                mixed = color * (1.0 - refl)[:, None] + below[h] * refl[:, None]
                col[h] = np.where((refl > 0)[:, None], mixed, color)
            below = col
    hits = sum(int((lv["traced"] & (lv["sphere"] >= 0)).sum()) for lv in runs[0])
    return below, runs[0], hits * sa.lpos.shape[0]


def _shininess_one(text):
    """The scene text with every sphere's shininess (its last field) set to 1."""
    lines = []
    for line in text.splitlines():
        if line.startswith("sphere"):
            line = " ".join(line.split()[:-1] + ["1"])
        lines.append(line)
    return "\n".join(lines) + "\n"


@functools.lru_cache(maxsize=None)
def _lattice_scene(nl):
    import rt_hip

    text = _shininess_one(qc.lattice_text(max(nl, 2)))
    if nl == 0:
        text = "".join(line + "\n" for line in text.splitlines() if not line.startswith("light"))
    sc = rt_hip.Scene.parse(text)
    sa = path_ref.SceneArrays(sc)
    assert sc.num_lights == nl and (sa.shin == 1.0).all()
    return sc, sa


@pytest.mark.parametrize("nl", (0,) + qc.LATTICE_NL + (65, 130))
def test_lights_over_lanes_lattice(gpu_renderer, nl):
    sc, sa = _lattice_scene(nl)
    gpu_renderer.upload(sc)
    for h in qc.LATTICE_H:
        o, d, lanes = qc.lattice_rays(h)
        want, levels, shadow = shade_any(o, d, 2, sa)
        assert np.array_equal(np.flatnonzero(levels[0]["sphere"] >= 0), lanes)
        if nl <= path_ref.MAX_LIGHTS:  # the generalised checker is path_ref.shade where that one applies
            assert np.array_equal(want.view(np.uint64), path_ref.shade(levels, sa).view(np.uint64))
        got, st = gpu_renderer.trace_radiance(o, d, 2, F64X3)
        same = same_values(got, want)
        assert same.all(), (nl, h, np.flatnonzero(~same.all(axis=1)).tolist())
        n, segments, hits, _ = path_ref.counts(levels, sa)
        assert (st.rays, st.segments, st.hits, st.shadow_rays) == (n, segments, hits, shadow)
    assert nl == 0 or shadow > 0


# -- the reflection stack
# test_gpu_paths.MIRRORS with reflectivity 0.9 and shininess 1: the chains are the same (reflectivity > 0),
# every level contributes to the colour, and no pow rounds
MIRRORS_09 = ("sphere 0 0 -5 4 1 0.8 0.6 0.9 1 1\nsphere 0 0 5 4 0.5 0.7 1 0.9 1 1\nlight 3 4 0 1 1 1 1\n"
              "camera 0 0 0 0 0 -1 60\n")


@functools.lru_cache(maxsize=None)
def _mirror_case():
    import rt_hip

    sc = rt_hip.Scene.parse(MIRRORS_09)
    sa = path_ref.SceneArrays(sc)
    D = rt_hip.RT_MAX_DEPTH
    ang = np.linspace(0.0, 0.12, 65)  # ray 0 exactly along +z, the rest fanned in the x-z plane
    o = np.zeros((65, 3))
    d = np.stack([np.sin(ang), np.zeros(65), np.cos(ang)], axis=1)
    levels = path_ref.trace_paths(o, d, D, sa)
    length = np.sum([lv["traced"] for lv in levels], axis=0)
    assert length[0] == D and len(set(length.tolist())) >= 5 and length.min() < 8  # uneven chains
    want = path_ref.shade(levels, sa)
    want.setflags(write=False)
    return sc, sa, o, d, levels, want


def test_long_and_uneven_chains(gpu_renderer):
    sc, sa, o, d, levels, want = _mirror_case()
    gpu_renderer.upload(sc)
    got, st = gpu_renderer.trace_radiance(o, d, len(levels), F64X3)
    same = same_values(got, want)
    assert same.all(), np.flatnonzero(~same.all(axis=1)).tolist()
    check_counts(st, levels, sa)
    rgb, _ = gpu_renderer.trace_radiance(o, d, len(levels), RGB8)
    assert np.array_equal(rgb, path_ref.quantize(want))


def test_stack_slots_are_reused_not_shared(gpu_renderer):
    """The same batch at depth 64 with another n, large enough for a second trip of the grid-stride loop
    whatever the grid: 65 rays repeated land on other lanes in every repetition, and every ray's colour
    is its colour in the batch of 65."""
    import torch

    sc, sa, o, d, levels, want = _mirror_case()
    D = len(levels)
    gpu_renderer.upload(sc)
    small, _ = gpu_renderer.trace_radiance(o, d, D, F64X3)
    n = 64 * 64 * torch.cuda.get_device_properties(0).multi_processor_count + 64 + 37
    big, st = gpu_renderer.trace_radiance(np.resize(o, (n, 3)), np.resize(d, (n, 3)), D, F64X3)
    assert np.array_equal(big.view(np.uint64), np.resize(small, (n, 3)).view(np.uint64))
    per_ray = np.sum([lv["traced"] for lv in levels], axis=0)
    assert (st.rays, st.segments) == (n, int(np.resize(per_ray, n).sum()))
    first, _ = gpu_renderer.trace_radiance(o[:33], d[:33], D, F64X3)
    assert np.array_equal(first.view(np.uint64), small[:33].view(np.uint64))


def test_depth_one_needs_no_stack():
    """A context whose first radiance launch has depth 1 (no stack exists yet), then a deeper one, then
    depth 1 again."""
    import rt_hip

    name = "complex"
    sc, sa = _scene(name)
    o, d = _rays(name)
    r = rt_hip.Renderer(0)
    try:
        r.upload(sc)
        for depth in (1, 4, 1):
            rgb, st = r.trace_radiance(o, d, depth, RGB8)
            check_pm1(rgb, path_ref.quantize(_colour(name, N_FULL, depth)), "fresh context, depth %d" % depth)
            check_counts(st, _ref(name, N_FULL, depth), sa)
    finally:
        r.close()


# -- the grid-stride loop's second trip
def test_second_trip(gpu_renderer):
    import rt_hip
    import torch

    sc = rt_hip.Scene.load(scene_path("simple"))
    sa = path_ref.SceneArrays(sc)
    nb, depth = 4133, 4
    o, d = ray_ref.gen_rays(1, nb, sa.centers, sa.radii, tuple(sc.camera().position))
    levels = path_ref.trace_paths(o, d, depth, sa)
    gpu_renderer.upload(sc)
    base, st0 = gpu_renderer.trace_radiance(o, d, depth, RGB8)
    check_pm1(base, path_ref.quantize(path_ref.shade(levels, sa)), "simple, 4133 rays")
    check_counts(st0, levels, sa)
    n = 64 * 64 * torch.cuda.get_device_properties(0).multi_processor_count + 64 + 37
    host = np.zeros((n, 8))
    host[:, 0:3], host[:, 3:6] = np.resize(o, (n, 3)), np.resize(d, (n, 3))
    rays = torch.from_numpy(host).to("cuda:0")
    guard = 4096
    out = torch.full((n * 3 + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
    gpu_renderer.trace_radiance_device(rays.data_ptr(), n, depth, RGB8, out.data_ptr())
    st = gpu_renderer.radiance_stats()
    got = out.cpu().numpy()
    assert np.array_equal(got[:n * 3].reshape(n, 3), np.resize(base, (n, 3)))
    assert (got[n * 3:] == 0xA5).all()  # the guard after the buffer is untouched
    per_ray = np.sum([lv["traced"] for lv in levels], axis=0)
    assert (st.rays, st.segments) == (n, int(np.resize(per_ray, n).sum()))


# -- bad rays, a light at a hit point, no spheres
def test_bad_rays(gpu_renderer):
    import rt_hip

    sc = rt_hip.Scene.parse(TWO + "light 3 4 0 1 1 1 1\n" + CAM)
    sa = path_ref.SceneArrays(sc)
    nan, inf = float("nan"), float("inf")
    o = np.array([(0, 0, 0), (0, 0, 0), (0, 0, 0), (nan, 0, 0), (0, 0, 0)], np.float64)
    d = np.array([(0, 0, 0), (0, nan, -1), (inf, 0, -1), (0, 0, -1), (0.1, 0, -1)], np.float64)
    levels = path_ref.trace_paths(o, d, 3, sa)
    assert levels[0]["traced"].all() and (levels[0]["sphere"][:4] == -1).all() and levels[0]["sphere"][4] == 0
    want = path_ref.shade(levels, sa)
    assert np.isnan(want[0]).all() and np.isnan(want[1]).all()  # the sky of a NaN direction
    gpu_renderer.upload(sc)
    got, st = gpu_renderer.trace_radiance(o, d, 3, F64X3)
    same = same_values(got[:4], want[:4])  # sky only: no pow
    assert same.all(), (got, want)
    rlo, rhi, _ = _query_region(sc)
    check_counts(st, levels, sa, unaccel=path_ref.unaccelerated(levels, o, sa, rlo, rhi))
    assert st.unaccelerated >= 4
    rgb, st8 = gpu_renderer.trace_radiance(o, d, 3, RGB8)
    # write_ppm's std::min(1.0, c) returns 1.0 for a NaN: the reference's byte is 255 (the golden
    # simple_1x1_d10 is such a pixel), and nothing is counted as clamped
    fin = ~np.isnan(want)
    assert (rgb[~fin] == 255).all() and (path_ref.quantize(want)[~fin] == 255).all() and st8.negative_clamped == 0
    check_pm1(rgb[fin], path_ref.quantize(want)[fin], "bad rays")
    # no rays: a no-op
    none, st0 = gpu_renderer.trace_radiance(np.zeros((0, 3)), np.zeros((0, 3)), 3)
    assert none.shape == (0, 3) and st0.rays == 0


def test_light_at_a_hit_point(gpu_renderer):
    import rt_hip

    o, d = _fan()
    d[0] = (0.0, 0.0, -1.0)
    sc = rt_hip.Scene.parse(TWO + _light_lines([(0.0, 0.0, -4.0), (3.0, 4.0, 0.0)]) + CAM)
    sa = path_ref.SceneArrays(sc)
    levels = path_ref.trace_paths(o, d, 2, sa)
    assert tuple(levels[0]["hit"][0]) == (0.0, 0.0, -4.0) and int(levels[0]["shadowed"][0]) & 1 == 0
    want = path_ref.shade(levels, sa)
    assert np.isfinite(want).all()
    gpu_renderer.upload(sc)
    rgb, st = gpu_renderer.trace_radiance(o, d, 2, RGB8)
    check_pm1(rgb, path_ref.quantize(want), "a light at a hit point")
    check_counts(st, levels, sa, unaccel=1)  # that shadow query took the every-sphere sweep


def test_zero_sphere_scene(gpu_renderer):
    import rt_hip

    sc = rt_hip.Scene.parse("light 3 4 0 1 1 1 1\n" + CAM)
    o, d = _fan()
    want = path_ref.shade(path_ref.trace_paths(o, d, 3, sc), sc)
    gpu_renderer.upload(sc)
    got, st = gpu_renderer.trace_radiance(o, d, 3, F64X3)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))  # all sky
    assert (st.rays, st.segments, st.hits, st.shadow_rays) == (65, 65, 0, 0)


# -- culling off
def test_unculled_same_bytes(gpu_renderer):
    name, n, depth = "complex", N_FULL, 4
    sc, sa = _scene(name)
    o, d = _rays(name)
    gpu_renderer.upload(sc)
    want64, _ = gpu_renderer.trace_radiance(o, d, depth, F64X3)
    want8, _ = gpu_renderer.trace_radiance(o, d, depth, RGB8)
    gpu_renderer.set_culling(False)
    try:
        got64, st = gpu_renderer.trace_radiance(o, d, depth, F64X3)
        got8, _ = gpu_renderer.trace_radiance(o, d, depth, RGB8)
    finally:
        gpu_renderer.set_culling(True)
    assert got64.tobytes() == want64.tobytes() and got8.tobytes() == want8.tobytes()
    check_counts(st, _ref(name, n, depth), sa, unaccel=None)
    assert st.unaccelerated == st.segments + st.shadow_rays and st.tests_cull == 0


# -- the other BVH layouts (tuning build) and the bounds-checked build
VARIANT_RUNS = (("medium", N_FULL, 4), ("synth10k", 1024, 3))


@functools.lru_cache(maxsize=None)
def _product_bytes(name, n, depth):
    """The product library's answers (F64X3, RGB8) for a variant run, from a context of its own."""
    import rt_hip

    o, d = _rays(name, n)
    r = rt_hip.Renderer(0)
    try:
        r.upload(_scene(name)[0])
        f64, _ = r.trace_radiance(o, d, depth, F64X3)
        rgb, _ = r.trace_radiance(o, d, depth, RGB8)
    finally:
        r.close()
    check_pm1(rgb, path_ref.quantize(_colour(name, n, depth, n)), "%s, product build" % name)
    return f64.tobytes(), rgb.tobytes()


def _check_variant(r):
    for name, n, depth in VARIANT_RUNS:
        o, d = _rays(name, n)
        r.upload(_scene(name)[0])
        f64, st = r.trace_radiance(o, d, depth, F64X3)
        rgb, _ = r.trace_radiance(o, d, depth, RGB8)
        assert (f64.tobytes(), rgb.tobytes()) == _product_bytes(name, n, depth), name
        check_counts(st, _ref(name, n, depth, n), _scene(name)[1])


@pytest.fixture(params=list(KNOB_SETS))
def radiance_layout_renderer(request, monkeypatch):
    import rt_hip

    for k, v in KNOB_SETS[request.param].items():
        monkeypatch.setenv(k, v)
    r = rt_hip.Renderer(0, variant="tuning")  # reads the knobs at rt_create
    yield r
    r.close()


def test_layouts(radiance_layout_renderer):
    _check_variant(radiance_layout_renderer)


def test_checked_build():
    import rt_hip

    r = rt_hip.Renderer(0, variant="check")
    try:
        _check_variant(r)
        r.stats()  # raises on RT_ERR_CHECK
    finally:
        r.close()


# -- the device path and streams
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
        want, _ = r.trace_radiance(o, d, depth, F64X3)
        want = want.tobytes()
        assert torch.cuda.current_stream().cuda_stream == 0
        rays = torch.from_numpy(host_rays).to("cuda:0")  # filled on the legacy NULL stream
        out = torch.zeros((n * 24,), dtype=torch.uint8, device="cuda:0")
        r.trace_radiance_device(rays.data_ptr(), n, depth, F64X3, out.data_ptr())
        assert out.cpu().numpy().tobytes() == want  # read on the NULL stream, no host sync between
        assert r.radiance_stats().rays == n
        r.set_stream(side.cuda_stream)
        with torch.cuda.stream(side):
            out2 = torch.zeros((n * 24,), dtype=torch.uint8, device="cuda:0")
            r.trace_radiance_device(rays.data_ptr(), n, depth, F64X3, out2.data_ptr())
            got = out2.cpu().numpy().tobytes()
        assert got == want
        # the synchronous call takes device memory too
        out3 = torch.zeros((n * 24,), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()  # the side stream is not ordered with the NULL stream's fill
        st = rt_hip.rt_radiance_stats()
        rc = r._L.rt_trace_radiance(r.handle, C.c_void_p(rays.data_ptr()), n, depth, F64X3,
                                    C.c_void_p(out3.data_ptr()), 1, C.byref(st))
        assert rc == 0 and st.rays == n
        side.synchronize()
        assert out3.cpu().numpy().tobytes() == want
    finally:
        r.set_stream(None)
        r.close()


# -- errors that need a context
def test_errors():
    import rt_hip
    import torch

    o, d = _fan()
    r = rt_hip.Renderer(0)
    try:
        with pytest.raises(rt_hip.RtError) as e:
            r.trace_radiance(o, d, 3)
        assert e.value.status == 5  # RT_ERR_NO_SCENE
        assert r.radiance_stats().rays == 0
        r.upload(rt_hip.Scene.parse(TWO + "light 3 4 0 1 1 1 1\n" + CAM))
        with pytest.raises(rt_hip.RtError) as e:
            r.trace_radiance(o, d, rt_hip.RT_MAX_DEPTH + 1)
        assert e.value.status == 7  # RT_ERR_DEPTH
        for depth, fmt in ((0, F64X3), (3, 3), (3, -1)):
            with pytest.raises(rt_hip.RtError) as e:
                r.trace_radiance(o, d, depth, fmt)
            assert e.value.status == 1  # RT_ERR_INVALID_ARG
        rays = torch.zeros((66, 8), dtype=torch.float64, device="cuda:0")
        out = torch.zeros((66 * 24 + 16,), dtype=torch.uint8, device="cuda:0")
        for rp, op in ((rays.data_ptr() + 8, out.data_ptr()), (rays.data_ptr(), out.data_ptr() + 8)):
            with pytest.raises(rt_hip.RtError) as e:
                r.trace_radiance_device(rp, 65, 3, F64X3, op)
            assert e.value.status == 1
        assert r.radiance_stats().rays == 0  # nothing was launched
        got, st = r.trace_radiance(o, d, 3)  # the context is fine
        assert st.rays == 65 and got.shape == (65, 3) and got.dtype == np.float64
    finally:
        r.close()
