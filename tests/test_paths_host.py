"""CPU-only: the path query's checker and host side.  tests/path_ref.py (the
numpy restatement of trace_ray every GPU path test compares with) reproduces
oracle-made goldens byte for byte, and its ray counts are the manifest's; the
rt_vertex / rt_surface / rt_path_stats layouts, the exported symbols and the
argument errors that return before any HIP call."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import path_ref
import ray_ref
import rt_hip
from conftest import golden_rgb, manifest, scene_path


@pytest.mark.parametrize("name", ["complex_97x61_d4", "simple_2x2_d10"])
def test_checker_reproduces_golden(name):
    m = manifest()[name]
    W, H, D = m["width"], m["height"], m["depth"]
    sc = rt_hip.Scene.load(scene_path(m["scene"]))
    rays = ray_ref.camera_rays(sc.camera(), W, H)  # PPM row order; Ray() normalises the direction again
    sa = path_ref.SceneArrays(sc)
    levels = path_ref.trace_paths(rays[:, 0:3], rays[:, 3:6], D, sa)
    assert len(levels) == D
    n, segments, hits, shadow = path_ref.counts(levels, sa)
    assert {"primary": n, "reflect": segments - n, "shadow": shadow} == m["rays"]
    assert hits * sc.num_lights == shadow
    rgb = path_ref.quantize(path_ref.shade(levels, sa))
    assert rgb.tobytes() == golden_rgb(name)


def test_checker_levels_are_consistent():
    """A level is traced exactly where the one above spawned a reflection; the
    untraced records hold the sentinel values."""
    sc = rt_hip.Scene.load(scene_path("complex"))
    c, r = ray_ref.spheres_of(sc)
    o, d = ray_ref.gen_rays(1, 1061, c, r, tuple(sc.camera().position))
    levels = path_ref.trace_paths(o, d, 4, sc)
    assert levels[0]["traced"].all()
    t0, s0 = ray_ref.closest(o, d, c, r)
    assert np.array_equal(levels[0]["sphere"], s0)
    assert np.array_equal(levels[0]["t"].view(np.uint64), t0.view(np.uint64))
    for k, lv in enumerate(levels):
        if k + 1 < len(levels):
            assert np.array_equal(levels[k + 1]["traced"], lv["reflects"])
        else:
            assert not lv["reflects"].any()  # depth - (k+1) >= 1 fails at the last level
        un = ~lv["traced"]
        assert (lv["t"][un] == 1e20).all() and (lv["sphere"][un] == -1).all() and (lv["shadowed"][un] == 0).all()
        assert (lv["shadowed"][lv["sphere"] < 0] == 0).all()
    assert levels[3]["traced"].any()  # some paths are four segments long


def test_path_struct_layouts_and_symbols():
    v, s, st = rt_hip.rt_vertex, rt_hip.rt_surface, rt_hip.rt_path_stats
    assert C.sizeof(v) == 32 and C.sizeof(s) == 96 and C.sizeof(st) == 64
    assert [(f, getattr(v, f).offset) for f, _ in v._fields_] == [("t", 0), ("sphere", 8), ("flags", 12),
                                                                  ("shadowed", 16), ("reserved", 24)]
    assert [(f, getattr(s, f).offset) for f, _ in s._fields_] == [("dir", 0), ("hit", 24), ("normal", 48), ("view", 72)]
    assert [(f, getattr(st, f).offset) for f, _ in st._fields_] == [
        ("rays", 0), ("segments", 8), ("hits", 16), ("shadow_rays", 24), ("tests_exact", 32), ("tests_cull", 40),
        ("unaccelerated", 48), ("kernel_ms", 56)]
    assert rt_hip.VERTEX_DTYPE.itemsize == 32 and rt_hip.SURFACE_DTYPE.itemsize == 96
    assert [rt_hip.VERTEX_DTYPE.fields[f][1] for f in ("t", "sphere", "flags", "shadowed", "reserved")] == [0, 8, 12,
                                                                                                          16, 24]
    assert (rt_hip.RT_PATH_MAX_LIGHTS, rt_hip.RT_VERTEX_TRACED, rt_hip.RT_VERTEX_REFLECTS) == (64, 1, 2)
    assert rt_hip.lib().rt_abi_version() == 12  # new symbols only
    out = subprocess.check_output(["nm", "-D", "--defined-only", rt_hip.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("rt_trace_paths", "rt_trace_paths_async", "rt_path_stats_get"):
        assert name in exported and name in rt_hip.SIGNATURES, name


def test_path_argument_errors_need_no_gpu():
    L = rt_hip.lib()
    INVALID = 1  # RT_ERR_INVALID_ARG
    rays = (rt_hip.rt_ray * 2)()
    verts = (rt_hip.rt_vertex * 8)()
    st = rt_hip.rt_path_stats()
    p = lambda x: C.cast(x, C.c_void_p)  # noqa: E731
    assert L.rt_trace_paths(None, p(rays), 2, 4, p(verts), None, 0, C.byref(st)) == INVALID
    assert L.rt_trace_paths(None, None, 0, 1, None, None, 0, None) == INVALID
    assert L.rt_trace_paths_async(None, p(rays), 2, 4, p(verts), None) == INVALID
    assert L.rt_path_stats_get(None, C.byref(st)) == INVALID
