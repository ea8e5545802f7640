"""CPU-only: the radiance query's host side and its fp64 checker.  The exported
symbols, the rt_radiance_stats layout and the argument errors that return
before any HIP call; and tests/path_ref.py's shade(), which the GPU tests of
rt_trace_radiance compare unquantised colours with, pinned to the oracle's fp64
framebuffer on the scenes whose shininess involves no pow rounding."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import material_cases as mc
import path_ref
import ray_ref
import rt_hip

# The F64_CASES the checker reproduces in fp64: tier B of test_gpu_radiance.py runs these.  One is left out
# by name: with a shininess of -1 the specular term is pow(rdv, -1), and at rdv == 0 the reference's glibc
# pow returns +inf (the case is tagged has_inf) where path_ref's math.pow raises "math domain error", so the
# checker cannot shade that scene at all.  The render's own F64X3 of it is compared with the oracle by
# test_gpu_materials.py.
F64_LEFT_OUT = ("shin_minus_one",)
F64_KEPT = tuple(c for c in mc.F64_CASES if c not in F64_LEFT_OUT)
assert len(F64_KEPT) >= 4 and set(F64_LEFT_OUT) <= set(mc.F64_CASES)


def same_values(a, b):
    """Elementwise a == b with a NaN matching a NaN (-0.0 equals +0.0, +inf equals +inf)."""
    a, b = np.asarray(a), np.asarray(b)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def test_radiance_struct_layout_and_symbols():
    st = rt_hip.rt_radiance_stats
    assert C.sizeof(st) == 72
    assert [(f, getattr(st, f).offset) for f, _ in st._fields_] == [
        ("rays", 0), ("segments", 8), ("hits", 16), ("shadow_rays", 24), ("tests_exact", 32), ("tests_cull", 40),
        ("unaccelerated", 48), ("negative_clamped", 56), ("kernel_ms", 64)]
    assert rt_hip.lib().rt_abi_version() == 12  # new symbols only
    out = subprocess.check_output(["nm", "-D", "--defined-only", rt_hip.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("rt_trace_radiance", "rt_trace_radiance_async", "rt_radiance_stats_get"):
        assert name in exported and name in rt_hip.SIGNATURES, name
    for name in ("trace_radiance", "trace_radiance_device", "radiance_stats"):
        assert callable(getattr(rt_hip.Renderer, name)), name


def test_radiance_argument_errors_need_no_gpu():
    L = rt_hip.lib()
    INVALID = 1  # RT_ERR_INVALID_ARG
    rays = (rt_hip.rt_ray * 2)()
    out = (C.c_double * 6)()
    st = rt_hip.rt_radiance_stats()
    p = lambda x: C.cast(x, C.c_void_p)  # noqa: E731
    for fmt in (rt_hip.RT_FB_RGB8, rt_hip.RT_FB_F32X3, rt_hip.RT_FB_F64X3):
        assert L.rt_trace_radiance(None, p(rays), 2, 4, fmt, p(out), 0, C.byref(st)) == INVALID
        assert L.rt_trace_radiance_async(None, p(rays), 2, 4, fmt, p(out)) == INVALID
    assert L.rt_trace_radiance(None, None, 0, 1, rt_hip.RT_FB_F64X3, None, 0, None) == INVALID
    assert L.rt_radiance_stats_get(None, C.byref(st)) == INVALID


def _checker(case):
    W, H, D = mc.F64_SHAPE
    sc = rt_hip.Scene.parse(mc.text(case, "dense"))
    sa = path_ref.SceneArrays(sc)
    rays = ray_ref.camera_rays(sc.camera(), W, H)
    levels = path_ref.trace_paths(rays[:, 0:3], rays[:, 3:6], D, sa)
    return levels, sa


def test_the_case_left_out_cannot_be_shaded():
    assert mc.has_inf("shin_minus_one")
    levels, sa = _checker("shin_minus_one")
    with pytest.raises(ValueError):  # math.pow(0.0, -1.0)
        path_ref.shade(levels, sa)


@pytest.mark.parametrize("case", F64_KEPT)
def test_checker_reproduces_the_oracle_in_fp64(case):
    """camera_rays -> trace_paths -> shade equals the oracle's fp64 framebuffer as values.  The cases'
    shininess is 0 or 1 everywhere: pow(x, 0) is 1 and pow(x, 1) is x, no rounding."""
    W, H, D = mc.F64_SHAPE
    levels, sa = _checker(case)  # PPM row order, as the oracle's framebuffer
    got = path_ref.shade(levels, sa)
    _, counts, fb = mc.oracle(case, "dense", W, H, D)
    n, segments, _, shadow = path_ref.counts(levels, sa)
    assert (n, segments - n, shadow) == (counts["primary"], counts["reflect"], counts["shadow"])
    same = same_values(got, fb.reshape(-1, 3))
    assert same.all(), "%d of %d channels differ" % (int((~same).sum()), same.size)
