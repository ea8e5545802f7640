"""CPU-only: the ray queries' checker and host side.  tests/ray_ref.py (the
numpy restatement of sphere.h:26-59 and scene.h:41-61 every GPU ray test
compares with) equals the oracle's orc_intersect in the hit flag and the bits
of t; the rt_ray / rt_hit layouts, the exported symbols and the argument
errors that return before any HIP call."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import orc
import ray_ref
import rt_hip
from conftest import scene_path

SCENES = ["simple", "medium", "complex", "synth200", "synth10k"]


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _scene(name):
    sc = rt_hip.Scene.load(scene_path(name))
    centers, radii = ray_ref.spheres_of(sc)
    return sc, centers, radii


@pytest.mark.parametrize("name", SCENES)
def test_ray_ref_equals_oracle_intersect(name):
    """At least 2,000 (ray, sphere) pairs per shipped scene: the generator's
    rays, each against the sphere it was aimed from / at (where one exists)
    and against random others."""
    sc, centers, radii = _scene(name)
    n = 700
    o, d = ray_ref.gen_rays(1, n, centers, radii, tuple(sc.camera().position))
    dn = ray_ref.normalize(d)  # the oracle takes the Ray's stored (normalised) direction
    t_best, s_best = ray_ref.closest(o, d, centers, radii)
    share = float((s_best >= 0).mean())
    assert 0.25 <= share <= 0.85, share  # a non-degenerate batch
    rng = np.random.default_rng(2)
    pick = rng.integers(0, len(radii), (n, 3))
    pick[:, 0] = np.where(s_best >= 0, s_best, pick[:, 0])  # the scan's own winner among them
    pairs = hits = 0
    for i in range(n):
        hit, t = ray_ref.intersect(o[i], dn[i], centers[pick[i]], radii[pick[i]])
        for k, s in enumerate(pick[i]):
            want_hit, want_t = orc.intersect(tuple(centers[s]), float(radii[s]), tuple(o[i]), tuple(dn[i]))
            assert bool(hit[0, k]) == want_hit, (i, s)
            if want_hit:
                assert _bits(t[0, k]) == _bits(want_t), (i, s, t[0, k], want_t)
                hits += 1
            pairs += 1
        if s_best[i] >= 0:
            assert hit[0, 0] and _bits(t[0, 0]) == _bits(t_best[i])
    assert pairs >= 2000
    assert 0 < hits < pairs  # both outcomes sampled


HAND = [
    # origin, direction, centre, radius, hit, t
    ((1, 0, 0), (0, 0, -1), (0, 0, -5), 1.0, True, 5.0),    # tangent, disc == 0, positive root
    ((1, 0, 0), (0, 0, -1), (0, 0, 5), 1.0, True, -5.0),    # tangent behind the origin: the negative root is kept
    ((0, 0, 0), (0, 0, -1), (0, 0, -0.5), 2.0, True, 2.5),  # origin inside: the far root
    ((0, 0, 0), (0, 0, -1), (0, 0, 5), 1.0, False, 0.0),    # wholly behind the origin
]


@pytest.mark.parametrize("o,d,c,r,want_hit,want_t", HAND)
def test_ray_ref_hand_made_cases(o, d, c, r, want_hit, want_t):
    hit, t = ray_ref.intersect([o], ray_ref.normalize([d]), [c], [r])
    orc_hit, orc_t = orc.intersect(c, r, o, d)
    assert bool(hit[0, 0]) == orc_hit == want_hit
    if want_hit:
        assert _bits(t[0, 0]) == _bits(orc_t) == _bits(want_t)
    tb, sb = ray_ref.closest([o], [d], [c], [r])
    assert (int(sb[0]), float(tb[0])) == ((0, want_t) if want_hit else (-1, 1e20))


def test_ray_ref_scan_order_and_nan():
    """Ties keep the lowest index; a NaN t and a t >= 1e20 are never recorded."""
    c = [(0, 0, -5), (0, 0, -5), (0, 0, -3)]
    t, s = ray_ref.closest([(0, 0, 0)], [(0, 0, -2)], c[:2], [1.0, 1.0])
    assert (float(t[0]), int(s[0])) == (4.0, 0)
    t, s = ray_ref.closest([(0, 0, 0)], [(0, 0, -2)], c, [1.0, 1.0, 1.0])
    assert (float(t[0]), int(s[0])) == (2.0, 2)
    for bad in [(0, 0, 0), (np.nan, 0, -1), (np.inf, 0, -1)]:
        t, s = ray_ref.closest([(0, 0, 0)], [bad], c, [1.0, 1.0, 1.0])
        assert (float(t[0]), int(s[0])) == (1e20, -1)
    t, s = ray_ref.closest([(0, 0, 0)], [(0, 0, -1)], [(0, 0, -3e20)], [1.0])
    assert (float(t[0]), int(s[0])) == (1e20, -1)
    assert list(ray_ref.occluded([4.0, 4.0, 4.0, 1e20], [0, 0, 0, -1], [np.inf, 4.0, np.nan, np.inf])) == [1, 0, 0, 0]


def test_tmax_classes_all_occur():
    tmax, cls = ray_ref.gen_tmax(3, np.linspace(1.0, 2.0, 70))
    assert sorted(set(cls.tolist())) == list(range(len(ray_ref.TMAX_CLASSES)))
    assert np.isnan(tmax[cls == 6]).all() and (tmax[cls == 5] == -1.0).all()


def test_query_struct_layouts_and_symbols():
    assert C.sizeof(rt_hip.rt_ray) == 64 and C.sizeof(rt_hip.rt_hit) == 16
    assert C.sizeof(rt_hip.rt_query_stats) == 48
    assert (rt_hip.RT_QUERY_CLOSEST, rt_hip.RT_QUERY_OCCLUDED) == (0, 1)
    out = subprocess.check_output(["nm", "-D", "--defined-only", rt_hip.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("rt_trace_rays", "rt_trace_rays_async", "rt_trace_stats", "rt_camera_rays"):
        assert name in exported and name in rt_hip.SIGNATURES, name


def test_query_argument_errors_need_no_gpu():
    L = rt_hip.lib()
    INVALID = 1  # RT_ERR_INVALID_ARG
    rays = (rt_hip.rt_ray * 2)()
    hits = (rt_hip.rt_hit * 2)()
    st = rt_hip.rt_query_stats()
    cam = rt_hip.rt_camera()
    p = lambda x: C.cast(x, C.c_void_p)  # noqa: E731
    assert L.rt_trace_rays(None, 0, p(rays), 2, p(hits), 0, C.byref(st)) == INVALID
    assert L.rt_trace_rays(None, 0, None, 0, None, 0, None) == INVALID
    assert L.rt_trace_rays_async(None, 1, p(rays), 2, p(hits)) == INVALID
    assert L.rt_trace_stats(None, C.byref(st)) == INVALID
    assert L.rt_camera_rays(None, C.byref(cam), 4, 4, None, p(rays)) == INVALID
