"""GPU: the two forms of the closest-hit list scans (rt_device.h cam_closest,
grid_closest).

A wave whose scanning lanes all have a2_ok(a2) and a binnable cell runs the
scan loop with `fast` and `all` compiled out; any other wave runs the loop as
it was.  A lane's bits are the same in both, so every render equals the oracle
(oracle/orc.py) byte for byte and ray count for ray count: as a one-frame
launch repeated from one position (the second launch has the camera grid and
the sphere grids) and as a three-frame launch, at 64x48 and 24x16, depth 4,
on the product build and the check build.

 * all-common waves: the ring scene (camera-grid scans of every tile,
   sphere-grid scans of the reflections off the ring's mirrors and the ground);
 * waves whose camera-grid lanes partly leave the scan: 60 small spheres with
   their centres on the ray of one pixel (computed here from the camera as
   rt_device.h camera_dir does).  That ray meets all 60 (checked below), the
   list of its direction's cell must hold every sphere its ray can report, so
   the cell holds more than kCgSlots = 48 entries whatever the grid's N: its
   lanes are told to sweep while their neighbours in the tile scan (the later
   launches are checked to have used the camera grid);
 * waves whose reflection rays partly fail sg_usable: two mirrors side by
   side, one of them studded with 40 small matt spheres that overlap its
   origin ball -- more than kSgMaxGlobal = 32, so its sphere grid is refused
   (rho2 = -1; checked: the scene has one grid fewer than the same scene
   without the studs).  Its reflection rays sweep (`rest = alive && !grid`)
   beside the neighbouring mirror's, which scan that mirror's grid, in the
   tiles that hold both;
 * mirrors beside matt spheres: waves where some lanes scan a sphere grid and
   the others have no reflection ray;
 * all-rare waves: a 1x1, a 1x16 and a 24x1 image (W - 1 = 0 or H - 1 = 0
   makes every camera ray NaN: no cell, every sphere tested).
A camera ray is NaN in every lane or in none, and a reflection ray's direction
is renormalised (a2 within 2^-48 of 2), so a wave that mixes scanning lanes
with `all` or not-`fast` lanes cannot be made by a scene; the guard is the
wave's ballot over exactly these two lane predicates, and the general loop it
falls back to is the text all waves ran before."""
import math
import os

import pytest

from conftest import SCENES, diff_summary
from test_gpu_light_paths import LIGHTS, _ring, _scene

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (24, 16)]
DEPTH = 4


RING = _ring(lambda k: "20")
PIXEL = {(64, 48): (29, 20), (24, 16): (13, 9)}  # the pixel whose ray carries the sixty spheres


def _pixel_ray(W, H):
    """Origin and (unnormalised) direction of PIXEL's camera ray, as rt_device.h camera_dir forms it."""
    import rt_hip

    cam = rt_hip.Scene.parse(_scene(RING, LIGHTS)).camera()
    i, j = PIXEL[(W, H)]
    su, sv = (i / (W - 1) - 0.5) * cam.scale, (j / (H - 1) - 0.5) * cam.scale
    d = [cam.forward[k] + cam.right[k] * su + cam.up[k] * sv for k in range(3)]
    return list(cam.position), d


def _on_pixel_ray(W, H, n=60):
    o, d = _pixel_ray(W, H)
    ln = math.sqrt(sum(c * c for c in d))
    out = []
    for k in range(n):
        t = (4.0 + 0.3 * k) / ln
        out.append("sphere %.17g %.17g %.17g 0.02 0.%d 0.9 0.3 %s 0.5 20" % (
            o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2], k % 10, "0.6" if k % 5 == 0 else "0.0"))
    return out


def _spheres_met(text, o, d):
    """How many of the scene's spheres the line o + t d, t > 0, passes through (in double; the margin is wide)."""
    n = 0
    for line in text.splitlines():
        w = line.split()
        if w and w[0] == "sphere":
            c, r = [float(v) for v in w[1:4]], float(w[4])
            oc = [o[k] - c[k] for k in range(3)]
            a, b = sum(v * v for v in d), 2.0 * sum(oc[k] * d[k] for k in range(3))
            cc = sum(v * v for v in oc) - r * r
            disc = b * b - 4.0 * a * cc
            n += disc > 0.25 * b * b * 1e-6 and -b > 0.0 and cc > 0.0
    return n


MIRRORS = ["sphere 1.0 1 -10 1 0.9 0.9 0.9 0.9 0.5 50", "sphere -1.0 1 -10 1 0.9 0.7 0.5 0.8 0.5 50"]


def _studs(n=40):
    """n small matt spheres centred on the surface of the first mirror, on the side the camera sees."""
    out = []
    for k in range(n):
        z = 0.15 + 0.8 * (k + 0.5) / n  # towards the camera
        rho, phi = math.sqrt(1.0 - z * z), 2.399963229728653 * k
        out.append("sphere %.17g %.17g %.17g 0.03 0.2 0.8 0.%d 0.0 0.5 20" % (
            1.0 + rho * math.cos(phi), 1.0 + rho * math.sin(phi), -10.0 + z, k % 10))
    return out


NAMES = ["ring", "sixty_on_one_pixel_ray", "mirror_with_refused_grid", "mirrors_beside_matt"]


def _text(name, W, H):
    if name == "ring":
        return _scene(RING, LIGHTS)
    if name == "sixty_on_one_pixel_ray":
        return _scene(RING + _on_pixel_ray(W, H), LIGHTS[:2])
    if name == "mirror_with_refused_grid":
        return _scene(RING + MIRRORS + _studs(), LIGHTS)
    return _scene(_ring(lambda k: "20", n=36) + ["sphere 1.5 1 -10 1 0.9 0.9 0.9 0.9 0.5 50",
                                                 "sphere -1.5 1 -10 1 0.9 0.5 0.5 0.0 0.5 50"], LIGHTS)


def _check(r, text, W, H, D, what):
    import orc
    import rt_hip
    import torch

    sc = rt_hip.Scene.parse(text)
    cam = sc.camera()
    r.upload(sc)
    want, cnt, _ = orc.OracleScene(text=text).render(W, H, D, threads=16)
    counts = (cnt["primary"], cnt["shadow"], cnt["reflect"])
    for launch in range(3):  # one position again: the later launches scan the grids
        rgb, st = r.render(cam, W, H, D)
        got = bytes(rgb)
        assert got == want, "%s %dx%d launch %d: %s" % (what, W, H, launch, diff_summary(got, want))
        assert (st.rays_primary, st.rays_shadow, st.rays_reflect) == counts, (what, W, H, launch)
    F, stride = 3, W * H * 3
    buf = torch.full((F * stride,), 77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    r.render_frames_async([cam] * F, W, H, D, None, buf.data_ptr(), stride)
    st3 = r.stats()
    host = bytes(buf.cpu().numpy())
    for f in range(F):
        frame = host[f * stride:(f + 1) * stride]
        assert frame == want, "%s %dx%d frame %d of 3: %s" % (what, W, H, f, diff_summary(frame, want))
    assert (st3.rays_primary, st3.rays_shadow, st3.rays_reflect) == tuple(F * c for c in counts), (what, W, H)
    return r.info(), st  # st: the last one-frame launch's statistics


@pytest.fixture(scope="module")
def check_renderer():
    import rt_hip

    r = rt_hip.Renderer(0, variant="check")
    yield r
    r.close()


@pytest.fixture(params=["product", "check"])
def renderer(request):
    return request.getfixturevalue("gpu_renderer" if request.param == "product" else "check_renderer")


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", NAMES)
def test_scan_scenes_byte_identical(name, size, renderer):
    W, H = size
    text = _text(name, W, H)
    if name == "sixty_on_one_pixel_ray":  # the pixel's ray meets more spheres than a cell has slots
        o, d = _pixel_ray(W, H)
        assert _spheres_met(text, o, d) >= 60
    info, st = _check(renderer, text, W, H, DEPTH, name)
    assert info.cam_grid_last == 1, "the later launches did not scan a camera grid"
    assert info.sphere_grids > 0
    # tests_cull counts the sweeps' bounding tests: with the grids on, only the
    # lanes a grid could not serve (an overflowed cell, a refused grid) sweep
    if name in ("ring", "mirrors_beside_matt"):
        assert st.tests_cull == 0, st.tests_cull
    else:
        assert st.tests_cull > 0, "no lane left the scans to sweep"
    if name == "mirror_with_refused_grid":  # the studded mirror has no grid, its neighbour has
        plain, pst = _check(renderer, _scene(RING + MIRRORS, LIGHTS), W, H, DEPTH, "the two mirrors without studs")
        assert info.sphere_grids == plain.sphere_grids - 1, (info.sphere_grids, plain.sphere_grids)
        assert pst.tests_cull == 0, pst.tests_cull


@pytest.mark.parametrize("size", [(1, 1), (1, 16), (24, 1)], ids=["1x1", "1x16", "24x1"])
def test_nan_camera_rays(size, renderer):
    with open(os.path.join(SCENES, "simple.txt")) as f:
        text = f.read()
    _check(renderer, text, size[0], size[1], DEPTH, "simple")
