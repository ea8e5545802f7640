"""No GPU: the gloss table's host half (include/rt_hip.h, "samples with glossy reflections") -- the roughness
column of a scene file (rt_scene_parse_roughness / rt_scene_load_roughness), rt_hip.gloss_pattern against
the pattern it states and the restatement ray_hip --gloss computes, the symbols, the NULL-handle errors, the
binding's shape checks, ray_hip's usage errors, and the arithmetic of the tests' own yardstick (gloss_ref)
on a hand-made sphere."""
import ctypes as C
import glob
import math
import os
import subprocess

import numpy as np
import pytest

import gloss_ref
import path_ref
import rt_hip
from conftest import PKG, SCENES, scene_path

NEW_SYMBOLS = ("rt_set_gloss_samples", "rt_group_set_gloss_samples", "rt_scene_parse_roughness",
               "rt_scene_load_roughness")
INVALID, IO = 1, 6  # rt_status

MALFORMED = ("# a comment\n"
             "sphere 0 0 -5 1 1 0 0 0.5 0.25 10\n"
             "sphere 1 0 -5 1 1 0 0 0.5 0.125\n"              # short: nine numbers
             "  sphere 2 0 -5 1 1 0 0 0.5 0.75 10 trailing\n"  # leading blanks, a trailing token
             "sphere 3 0 -5 1 1 0 x 0.5 0.5 10\n"             # not a number
             "sphre 4 0 -5 1 1 0 0 0.5 0.5 10\n"              # unknown record
             "light 0 5 0 1 1 1 1\n"
             "sphere 5 0 -5 1 1 0 0 0 -0.0 10\n"
             "sphere 6 0 -5 1 1 0 0 0 1e400 10\n")            # out of range for a double: the record fails


# ---- the roughness column --------------------------------------------------------------------------------
def _roughness(call, arg):
    n = C.c_int(-1)
    assert call(arg, None, 0, C.byref(n)) == 0  # the sizing call: out NULL, capacity 0
    out = (C.c_double * (n.value + 2))(*([7.0] * (n.value + 2)))
    m = C.c_int(-1)
    assert call(arg, out, n.value, C.byref(m)) == 0 and m.value == n.value
    assert list(out[n.value:]) == [7.0, 7.0]  # nothing behind the capacity
    return list(out[:n.value])


def test_roughness_of_every_shipped_scene_lines_up_with_the_parser():
    L = rt_hip.lib()
    paths = sorted(glob.glob(os.path.join(SCENES, "*.txt")))
    assert len(paths) >= 4
    for path in paths:
        sc = rt_hip.Scene.load(path)
        got = _roughness(L.rt_scene_load_roughness, os.fsencode(path))
        assert len(got) == sc.num_spheres, path
        with open(path) as f:
            text = f.read()
        assert _roughness(L.rt_scene_parse_roughness, text.encode()) == got
        assert rt_hip.scene_roughness(path) == got and rt_hip.scene_roughness(text) == got
        # column 9 of the accepted records, restated: every shipped record is well formed
        want = [float(line.split()[9]) for line in text.splitlines() if line.strip().startswith("sphere")]
        assert got == want, path


def test_roughness_of_medium():
    got = rt_hip.scene_roughness(scene_path("medium"))
    assert got[5:10] == [0.1, 0.2, 0.05, 0.3, 0.2]  # the metallic row
    assert got[:5] == [1.0] * 5 and got[-1] == 1.0 and len(got) == 44
    assert min(got) == 0.05 and max(got) == 1.0


def test_roughness_skips_what_the_parser_skips():
    sc = rt_hip.Scene.parse(MALFORMED)
    assert sc.num_spheres == 3 and sc.warnings == 4
    got = rt_hip.scene_roughness(MALFORMED)
    assert got[:2] == [0.25, 0.75] and got[2] == 0.0 and math.copysign(1.0, got[2]) == -1.0 and len(got) == 3
    assert [sc.sphere(i)["center"][0] for i in range(3)] == [0.0, 2.0, 5.0]  # index i is scene.spheres[i]
    assert rt_hip.scene_roughness("ambient 1 1 1\n") == []


def test_roughness_capacity_and_errors(tmp_path, capfd):
    L = rt_hip.lib()
    text = MALFORMED.encode()
    n = C.c_int(-1)
    out = (C.c_double * 3)(7.0, 7.0, 7.0)
    assert L.rt_scene_parse_roughness(text, out, 2, C.byref(n)) == 0  # fewer than there are: the first two
    assert n.value == 3 and list(out) == [0.25, 0.75, 7.0]
    for call, arg in ((L.rt_scene_parse_roughness, text), (L.rt_scene_load_roughness, b"/nonexistent")):
        assert call(None, out, 3, C.byref(n)) == INVALID
        assert call(arg, out, 3, None) == INVALID
        assert call(arg, out, -1, C.byref(n)) == INVALID
        assert call(arg, None, 3, C.byref(n)) == INVALID
    assert L.rt_scene_load_roughness(os.fsencode(tmp_path / "missing.txt"), out, 3, C.byref(n)) == IO
    cap = capfd.readouterr()
    assert cap.out == "" and cap.err == ""  # silent: the warnings are rt_scene_parse's


def test_parse_output_and_warnings_are_unchanged(capfd):
    sc = rt_hip.Scene.parse(MALFORMED, verbose=True)
    cap = capfd.readouterr()  # (the "Loaded scene" line waits in the library's own stdout buffer)
    assert cap.err == ("Warning: Invalid sphere at line 3, skipping\nWarning: Invalid sphere at line 5, skipping\n"
                       "Warning: Unknown type 'sphre' at line 6, skipping\n"
                       "Warning: Invalid sphere at line 9, skipping\n")
    assert sc.sphere(1) == {"center": (2.0, 0.0, -5.0), "radius": 1.0, "color": (1.0, 0.0, 0.0),
                            "reflectivity": 0.5, "shininess": 10.0}


# ---- symbols, handles, shapes ----------------------------------------------------------------------------
def test_symbols_and_methods():
    assert rt_hip.lib().rt_abi_version() == 12  # new symbols only
    out = subprocess.check_output(["nm", "-D", "--defined-only", rt_hip.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported and name in rt_hip.SIGNATURES, name
        restype, argtypes = rt_hip.SIGNATURES[name]
        fn = getattr(rt_hip.lib(), name)
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == argtypes
    assert rt_hip.SIGNATURES["rt_set_gloss_samples"][1] == [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                           C.c_int, C.c_int]
    assert "rt_gloss_samples" not in exported  # the group's view of a member stays inside the library
    assert callable(rt_hip.Renderer.set_gloss_samples) and callable(rt_hip.Group.set_gloss_samples)
    assert rt_hip.RT_MAX_GLOSS_BOUNCES == rt_hip.RT_MAX_DEPTH - 1 == 63
    for variant in rt_hip.VARIANTS.values():  # the test builds export them too
        out = subprocess.check_output(["nm", "-D", "--defined-only", variant], text=True)
        assert all(" " + name + "\n" in out for name in NEW_SYMBOLS), variant


def test_argument_errors_need_no_gpu():
    """Without a device no context exists: the NULL handle, with every kind of table and count."""
    L = rt_hip.lib()
    tab, rough = (C.c_double * 12)(), (C.c_double * 4)()
    for t in (tab, None):
        for rg in (rough, None):
            for S, B in ((4, 1), (1, 1), (0, 1), (65, 1), (4, 0), (4, 64), (-1, -1)):
                assert L.rt_set_gloss_samples(None, rg, t, S, B) == INVALID
                assert L.rt_group_set_gloss_samples(None, rg, t, S, B) == INVALID


def test_the_binding_checks_the_shapes():
    rough, tab, s, b = rt_hip._gloss_table([0.5, 0.25], [[(0.0, 1.0, 2.0), (3.0, 4.0, 5.0)]] * 3, 2)
    assert (s, b) == (3, 2) and list(tab)[:6] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0] and len(tab) == 18
    assert list(rough) == [0.5, 0.25]
    assert rt_hip._gloss_table([0.5], None, 2) == (None, None, 0, 0)  # cleared: nothing is checked
    assert rt_hip._gloss_table(None, None, None) == (None, None, 0, 0)
    rough, tab, s, b = rt_hip._gloss_table([], [[(0.0, 0.0, 0.0)]] * 4, 0)  # a scene without spheres
    assert (s, b) == (4, 1) and len(rough) == 1
    _, _, s, b = rt_hip._gloss_table(np.zeros(2), np.zeros((5, 3, 3)), 2)  # arrays
    assert (s, b) == (5, 3)
    for rg, bad in (([0.5], [[(0.0, 0.0, 0.0)]]),                                # one roughness for two spheres
                    ([0.5] * 3, [[(0.0, 0.0, 0.0)]]),
                    ([0.5] * 2, [[(0.0, 0.0, 0.0)] * 2, [(0.0, 0.0, 0.0)]]),     # ragged
                    ([0.5] * 2, [[(0.0, 0.0)]])):                                # pairs
        with pytest.raises(ValueError):
            rt_hip._gloss_table(rg, bad, 2)


# ---- gloss_pattern ---------------------------------------------------------------------------------------
def _disk(n, s):
    """Point s of lens_pattern(n, 1.0), restated as ray_hip's disk_point states it."""
    c = n * n - 1 - s
    a, b = c % n, c // n
    u = (a + 0.5) / n * 2.0 - 1.0
    v = (b + 0.5) / n * 2.0 - 1.0
    return u * math.sqrt(1.0 - v * v / 2.0) * 1.0, v * math.sqrt(1.0 - u * u / 2.0) * 1.0


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_gloss_pattern(n):
    nb, nn = 4, n * n
    tab = rt_hip.gloss_pattern(n, nb)
    assert len(tab) == nn == len(rt_hip.grid_pattern(n)) and all(len(row) == nb for row in tab)
    assert tab == rt_hip.gloss_pattern(n, nb)  # deterministic
    assert [row[:2] for row in tab] == rt_hip.gloss_pattern(n, 2)  # a bounce does not depend on the count
    disk = rt_hip.lens_pattern(n, 1.0)
    for s, row in enumerate(tab):
        for b, (x, y, z) in enumerate(row):
            i = (s + 17 * (b + 1)) % nn
            assert (x, y) == disk[i] == _disk(n, i)  # ray_hip's restatement, the same doubles
            h = (2 * ((7 * i + 3) % nn) + 1) / nn - 1.0
            assert -1.0 < h < 1.0 and z == h * math.sqrt(max(0.0, 1.0 - x * x - y * y))
            assert x * x + y * y + z * z <= 1.0  # the unit ball
    for b in range(nb):  # every bounce sees every point of the disk once
        assert sorted(row[b][:2] for row in tab) == sorted(disk)
    if nn > 1 and 17 % nn:
        assert tab[0][0] != tab[0][1]  # and two bounces are not bent alike
    with pytest.raises(ValueError):
        rt_hip.gloss_pattern(0, nb)
    with pytest.raises(ValueError):
        rt_hip.gloss_pattern(n, 0)


# ---- the yardstick's own arithmetic ----------------------------------------------------------------------
def test_bend_on_a_hand_made_sphere():
    """A ray down -z onto the top of a unit sphere's cap: normal (0, 0, 1) at the pole, 45 degrees off it
    on the side.  Numbers chosen so that every step is exact."""
    d = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])
    nrm = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])
    rough = np.array([0.5, 0.5, 0.0])
    pts = np.array([[0.5, 0.25, 0.5], [0.0, 0.0, -4.0]])
    # level 0: rd = d - 2 n (d.n); rp = rd + g * roughness
    chosen, use = gloss_ref.bend(d, nrm, rough, pts, 0)
    assert chosen.tolist() == [[0.25, 0.125, 1.25],    # bent: (0, 0, 1) + (0.25, 0.125, 0.25)
                               [1.0, 0.0, 0.0],        # the horizon: dot(rd, n) = 0, the product is not > 0
                               [0.0, 0.0, 1.0]]        # roughness 0: the mirror
    assert use.tolist() == [True, False, False]
    # level 1: g = (0, 0, -4) pushes rp = (0, 0, 1 - 2) through the surface: refused, the mirror
    chosen, use = gloss_ref.bend(d, nrm, rough, pts, 1)
    assert chosen.tolist() == [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]] and not use.any()
    # level 2: k >= bounces, and no table at all
    for p, k in ((pts, 2), (pts, 63), (None, 0)):
        chosen, use = gloss_ref.bend(d, nrm, rough, p, k)
        assert chosen.tolist() == [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]] and not use.any()
    # a NaN anywhere refuses; an entry exactly in the tangent plane (rp.n = 0) does too
    for g in ([np.nan, 0.0, 0.0], [0.0, 0.0, np.nan], [0.0, 0.0, -2.0]):
        chosen, use = gloss_ref.bend(d[:1], nrm[:1], rough[:1], np.array([g]), 0)
        assert chosen.tolist() == [[0.0, 0.0, 1.0]] and not use.any()
    chosen, use = gloss_ref.bend(d[:1], nrm[:1], np.array([np.nan]), pts, 0)
    assert chosen.tolist() == [[0.0, 0.0, 1.0]] and not use.any()
    # a ray from inside (d.n > 0: rd points inward): the perturbed ray must stay inside too
    chosen, use = gloss_ref.bend([[0.0, 0.0, 1.0]], [[0.0, 0.0, 1.0]], [0.5], [[0.5, 0.0, 1.0]], 0)
    assert chosen.tolist() == [[0.25, 0.0, -0.5]] and use.tolist() == [True]
    chosen, use = gloss_ref.bend([[0.0, 0.0, 1.0]], [[0.0, 0.0, 1.0]], [0.5], [[0.5, 0.0, 4.0]], 0)
    assert chosen.tolist() == [[0.0, 0.0, -1.0]] and use.tolist() == [False]


def test_host_chain_on_one_sphere():
    """One reflective sphere: a ray at its pole spawns once and leaves for the sky; with the table the
    spawn is counted as glossy and bent, with roughness 0 or no table as a mirror."""
    sc = rt_hip.Scene.parse("sphere 0 0 -5 1 1 1 1 0.5 0.3 10\nlight 0 5 0 1 1 1 1\n")
    sa = path_ref.SceneArrays(sc)
    o, d = np.zeros((2, 3)), np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])  # a hit and a miss
    pts = np.array([[0.5, 0.0, 0.0]])
    for rough, p, depth, want in (([0.5], pts, 3, (1, 0, 0)), ([0.0], pts, 3, (0, 0, 1)), ([0.5], None, 3, (0, 0, 1)),
                                  ([0.5], pts, 1, (0, 0, 0))):
        lv = gloss_ref.host_chain(o, d, depth, sa, rough, p)
        assert gloss_ref.coverage(lv) == want
        assert [int(x["traced"].sum()) for x in lv] == ([2, 1, 0] if depth == 3 else [2])
        assert lv[0]["sphere"].tolist() == [0, -1]
    # the bent ray is the mirror ray plus g * roughness, normalised: it still misses everything
    lv = gloss_ref.host_chain(o, d, 2, sa, [0.5], pts)
    assert lv[0]["use"].tolist() == [True, False] and lv[1]["sphere"].tolist() == [-1, -1]


def test_cli_usage_errors(tmp_path):
    scene = scene_path("simple")
    for flags in (("--gloss", "0.5"),                                         # only with --supersample
                  ("-a", "--gloss", "0.5"),
                  ("--supersample", "2", "--gloss"),
                  ("--supersample", "2", "--gloss", "x"),
                  ("--supersample", "2", "--gloss", "0.5x"),
                  ("--supersample", "2", "--gloss-bounces", "2"),             # only with --gloss
                  ("--supersample", "2", "--gloss", "1", "--gloss-bounces", "0"),
                  ("--supersample", "2", "--gloss", "1", "--gloss-bounces", "64"),
                  ("--aperture", "0.2", "--gloss", "0.5")):
        p = subprocess.run([os.path.join(PKG, "ray_hip"), *flags, "--width", "8", "--height", "8", scene],
                           cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and p.stderr.startswith("usage:"), flags
        assert "--gloss" in p.stderr
    assert not any(tmp_path.iterdir())  # nothing was rendered
