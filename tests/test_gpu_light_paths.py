"""GPU: the two forms of a light iteration in the kFast render kernels.

A wave whose lanes all pass the light's guards (rt_device.h light_common: the
shadow direction on renormalized()'s near-one path, a usable distance, a
binnable grid cell, the host's off_free bound) runs the straight-line shadow
query (shadow_cells<true>), any other wave the general one; a lane's bits are
the same in both.  The scenes here make waves that are all-common, all-rare
and mixed within one 8x8 tile, and every render is compared with the oracle
(oracle/orc.py) byte for byte and ray count for ray count: as a one-frame
launch (sparse waves spread their light loop over the lanes) and as a
three-frame launch (four tiles per wave, the deferred kernel), at 64x48 and
24x16, depth 4.  The fuzz generators (tests/fuzz_gen.py) add a fixed number
of scenes of a fixed seed."""
import os
import random

import pytest

import fuzz_gen
from conftest import SCENES, diff_summary

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (24, 16)]
DEPTH = 4


def _ring(shin_of, n=24, x0=0.0):
    """A big sphere in the middle of the view, a ring of small ones around it
    and a ground sphere; shin_of(k) is sphere k's shininess (k = 0: the big one)."""
    import math

    out = ["sphere %.17g 0 -20 3 0.9 0.2 0.2 0.0 1.0 %s" % (x0, shin_of(0))]
    for k in range(1, n + 1):
        a = 2 * math.pi * k / n
        out.append("sphere %.17g %.17g %.17g 0.8 0.2 0.%d 0.9 %s 0.5 %s" % (
            x0 + 6.5 * math.cos(a), 0.5 + 4.5 * math.sin(a), -20 + 2.0 * math.sin(3 * a), k % 10,
            "0.8" if k % 6 == 0 else "0.0", shin_of(k)))
    out.append("sphere %.17g -103 -20 100 0.5 0.5 0.5 0.3 1.0 %s" % (x0, shin_of(n + 1)))
    return out


def _scene(spheres, lights, x0=0.0):
    cam = "camera %.17g 2 5 %.17g 0 -20 60\n" % (x0, x0)
    return "\n".join(spheres + lights + ["ambient 0.1 0.1 0.1"]) + "\n" + cam


LIGHTS = ["light 10 10 -10 1.0 1.0 1.0 0.7", "light -10 10 -10 1.0 1.0 0.8 0.5", "light 0 12 -2 0.6 0.6 1.0 0.5"]


def _scenes():
    s = {}
    # int_pow's domain needs shininess x floor(log2 rdv) >= -900: with 1000 it
    # holds only where rdv >= 0.5 (around the highlight), pow_call elsewhere
    s["shininess_1000_among_20"] = _scene(_ring(lambda k: "1000" if k == 0 else "20"), LIGHTS)
    s["fractional_shininess"] = _scene(_ring(lambda k: "33.3" if k in (0, 5, 11) else "%d" % (5 + 5 * (k % 4))), LIGHTS)
    # a light 0.0005 outside the big sphere (inside a shadow ray's EPSILON overshoot, scene.h:72-82)
    s["light_just_outside_sphere"] = _scene(_ring(lambda k: "20"), LIGHTS + ["light 0 3.0005 -20 1.0 0.9 0.8 1"])
    # the whole scene 1e9 along x: its box is small against its coordinates, the
    # host's off_free bound fails and every shadow ray checks its line itself
    x0 = 1e9
    s["coordinates_of_1e9"] = _scene(_ring(lambda k: "20", x0=x0),
                                     ["light %.17g 10 -10 1.0 1.0 1.0 0.7" % (x0 + 10),
                                      "light %.17g 10 -10 1.0 1.0 0.8 0.5" % (x0 - 10)], x0=x0)
    return s


TEXTS = _scenes()


def _check(r, text, W, H, D, what, camera=None):
    import orc
    import rt_hip
    import torch

    sc = rt_hip.Scene.parse(text)
    cam = camera if camera is not None else sc.camera()
    r.upload(sc)
    want, cnt, _ = orc.OracleScene(text=text).render(W, H, D, threads=16, camera=camera)
    counts = (cnt["primary"], cnt["shadow"], cnt["reflect"])
    rgb, st = r.render(cam, W, H, D)
    got = bytes(rgb)
    assert got == want, "%s %dx%d one frame: %s" % (what, W, H, diff_summary(got, want))
    assert (st.rays_primary, st.rays_shadow, st.rays_reflect) == counts, (what, W, H)
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


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_rare_lane_scenes_byte_identical(name, size, gpu_renderer):
    _check(gpu_renderer, TEXTS[name], size[0], size[1], DEPTH, name)


@pytest.mark.parametrize("size", [(1, 1)] + SIZES, ids=["1x1"] + ["%dx%d" % s for s in SIZES])
def test_nan_camera_ray(size, gpu_renderer):
    """simple.txt at 1x1 depth 10: W - 1 = 0 makes the camera ray NaN, every
    lane of the wave rare; the same scene at the other sizes beside it."""
    with open(os.path.join(SCENES, "simple.txt")) as f:
        text = f.read()
    _check(gpu_renderer, text, size[0], size[1], 10 if size == (1, 1) else DEPTH, "simple")


# (generator, seed, scenes): fixed counts, a few seconds each
FUZZ = [("general", 5201, 40), ("near", 5202, 40), ("margin", 5203, 40)]


@pytest.mark.parametrize("case", FUZZ, ids=[c[0] for c in FUZZ])
def test_fuzz_scenes_byte_identical(case, gpu_renderer):
    import orc
    import rt_hip
    import torch

    gen, seed, count = case
    rng = random.Random(seed)
    for k in range(count):
        text = fuzz_gen.margin_scene(rng) if gen == "margin" else fuzz_gen.scene(rng, near=(gen == "near"))
        W, H = SIZES[k & 1]
        try:
            # every scene also as three frames of one launch (index 2 of check_scene's cycle)
            fuzz_gen.check_scene(gpu_renderer, text, W, H, DEPTH, rng, 2, threads=16, torch=torch, orc=orc,
                                 rt_hip=rt_hip)
        except fuzz_gen.Mismatch as e:
            pytest.fail("fuzz[%s] seed %d scene %d (%dx%d d%d): %s\n%s" % (gen, seed, k, W, H, DEPTH, e, text))
