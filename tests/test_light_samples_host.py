"""No GPU: the light table's symbols, signatures and argument errors (include/rt_hip.h, "samples under
area lights"), rt_hip.light_pattern against the pattern it states and against the restatement ray_hip
--light-radius computes, and ray_hip's usage errors."""
import ctypes as C
import math
import os
import subprocess

import pytest

import rt_hip
from conftest import PKG, scene_path

NEW_SYMBOLS = ("rt_set_light_samples", "rt_group_set_light_samples")
INVALID = 1  # RT_ERR_INVALID_ARG


def test_symbols_and_methods():
    assert rt_hip.lib().rt_abi_version() == 12  # new symbols only
    out = subprocess.check_output(["nm", "-D", "--defined-only", rt_hip.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported and name in rt_hip.SIGNATURES, name
        restype, argtypes = rt_hip.SIGNATURES[name]
        assert restype is C.c_int and argtypes == [C.c_void_p, C.POINTER(C.c_double), C.c_int]
        fn = getattr(rt_hip.lib(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes
    assert "rt_light_samples" not in exported  # the group's view of a member stays inside the library
    assert callable(rt_hip.Renderer.set_light_samples) and callable(rt_hip.Group.set_light_samples)
    assert callable(rt_hip.light_pattern)
    for variant in rt_hip.VARIANTS.values():  # the test builds export them too
        out = subprocess.check_output(["nm", "-D", "--defined-only", variant], text=True)
        assert all(" " + name + "\n" in out for name in NEW_SYMBOLS), variant


def test_argument_errors_need_no_gpu():
    """Without a device no context exists: the NULL handle, with every kind of table and count."""
    L = rt_hip.lib()
    tab = (C.c_double * 12)()
    for t in (tab, None):
        for S in (4, 1, 0, 65, -1):
            assert L.rt_set_light_samples(None, t, S) == INVALID
            assert L.rt_group_set_light_samples(None, t, S) == INVALID


def test_the_binding_checks_the_table_shape():
    ok, s = rt_hip._light_table([[(0.0, 1.0, 2.0), (3.0, 4.0, 5.0)]] * 3, 2)
    assert s == 3 and list(ok)[:6] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0] and len(ok) == 18
    assert rt_hip._light_table(None, 2) == (None, 0)
    empty, s = rt_hip._light_table([[]] * 4, 0)  # a scene without lights: an empty table of four samples
    assert s == 4 and len(empty) == 1
    for bad in ([[(0.0, 0.0, 0.0)]] * 3,                      # one light's offsets for a scene of two
                [[(0.0, 0.0, 0.0)] * 2, [(0.0, 0.0, 0.0)]],   # ragged
                [[(0.0, 0.0), (0.0, 0.0)]]):                  # pairs
        with pytest.raises(ValueError):
            rt_hip._light_table(bad, 2)


def _disk(n, s, radius):
    """Point s of lens_pattern(n, radius), restated as ray_hip's disk_point states it."""
    c = n * n - 1 - s
    a, b = c % n, c // n
    u = (a + 0.5) / n * 2.0 - 1.0
    v = (b + 0.5) / n * 2.0 - 1.0
    return u * math.sqrt(1.0 - v * v / 2.0) * radius, v * math.sqrt(1.0 - u * u / 2.0) * radius


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_light_pattern(n):
    R, nl = 0.75, 7
    tab = rt_hip.light_pattern(n, R, nl)
    assert len(tab) == n * n == len(rt_hip.grid_pattern(n)) and all(len(row) == nl for row in tab)
    disk = rt_hip.lens_pattern(n, R)
    for s, row in enumerate(tab):
        for l, (x, y, z) in enumerate(row):
            assert y == 0.0 and math.hypot(x, z) <= R              # the horizontal plane, within the radius
            assert (x, z) == disk[(s + 17 * l) % (n * n)]          # the rotation by 17 l
            assert (x, z) == _disk(n, (s + 17 * l) % (n * n), R)   # ray_hip's restatement, the same doubles
    for l in range(nl):  # every light sees every point of the disk once
        assert sorted((o[l][0], o[l][2]) for o in tab) == sorted(disk)
    if n * n > 1 and 17 % (n * n):
        assert tab[0][0] != tab[0][1]  # and two lights do not move together
    assert all(o == (0.0, 0.0, 0.0) for row in rt_hip.light_pattern(n, 0.0, nl) for o in row)
    assert rt_hip.light_pattern(n, R, 0) == [[]] * (n * n)
    with pytest.raises(ValueError):
        rt_hip.light_pattern(0, R, nl)
    with pytest.raises(ValueError):
        rt_hip.light_pattern(n, R, -1)


def test_cli_usage_errors(tmp_path):
    scene = scene_path("simple")
    for flags in (("--light-radius", "0.5"),                              # only with --supersample
                  ("-a", "--light-radius", "0.5"),
                  ("--supersample", "2", "--light-radius", "-0.1"),       # R >= 0
                  ("--supersample", "2", "--light-radius", "nan"),
                  ("--supersample", "2", "--light-radius", "x"),
                  ("--supersample", "2", "--light-radius", "0.5x"),
                  ("--supersample", "2", "--light-radius"),
                  ("--aperture", "0.2", "--light-radius", "0.5")):
        p = subprocess.run([os.path.join(PKG, "ray_hip"), *flags, "--width", "8", "--height", "8", scene],
                           cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and p.stderr.startswith("usage:"), flags
        assert "--light-radius" in p.stderr
    assert not any(tmp_path.iterdir())  # nothing was rendered
