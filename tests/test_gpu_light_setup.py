"""GPU: the per-light setup of the render kernels' lane-per-ray light loop.

shade_hit (rt_kernel.hip) reads the light grid's descriptor once per call,
carries the current light's row of the grid tables from one light to the next,
loads the row's global-list range through the scalar path and the lane's own
sphere where the light's iteration starts, and decides the own-sphere pre-test
of the straight-line form with lane predicates.  The scenes cover the first,
the last and the only light, global lists beside empty cell lists, each class
of the pre-test, and light distances outside [2^-300, 2^300] (where the
shared-reciprocal quotients of rt_device.h div3_shared would not be exact: the
light direction is formed with IEEE divisions, whatever the distance).  A
lane's bits are what they were, so every render here equals the oracle
(oracle/orc.py) byte for byte and ray count for ray count: as a one-frame
launch and as a three-frame launch (four tiles per wave, the deferred kernel),
at 64x48 and 24x16, depth 4."""
import random

import pytest

import fuzz_gen
from test_gpu_light_paths import LIGHTS, _check, _ring, _scene

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (24, 16)]
DEPTH = 4

SEVEN = LIGHTS + ["light 4 6 0 0.9 0.7 0.7 0.4", "light -6 3 -12 0.7 0.9 0.7 0.4", "light 0 20 -20 0.8 0.8 0.8 0.3",
                  "light 12 1 -25 0.7 0.7 0.9 0.4"]


def _scaled(text, k):
    """Every coordinate and radius of a scene text multiplied by k (a power of
    two: the same geometry up to scale, every product exact)."""
    out = []
    for line in text.splitlines():
        w = line.split()
        if not w:
            continue
        nscaled = {"sphere": 4, "light": 3, "camera": 6}.get(w[0], 0)
        for i in range(1, 1 + nscaled):
            w[i] = "%.17g" % (float(w[i]) * k)
        out.append(" ".join(w))
    return "\n".join(out) + "\n"


RING = _ring(lambda k: "20")

TEXTS = {
    # the carried row and the one-ahead loads at the only, the first and the last light
    "lights_1": _scene(RING, LIGHTS[:1]),
    "lights_2": _scene(RING, LIGHTS[:2]),
    "lights_7": _scene(RING, SEVEN),
    # lights whose global list holds a sphere around (or all but around) them, so most of their cells' own
    # lists are empty: inside the big sphere, inside the ground sphere, and 0.0005 outside the big one
    "light_inside_big_sphere": _scene(RING, LIGHTS + ["light 0.5 0.25 -20 1.0 0.9 0.8 1"]),
    "light_inside_ground_sphere": _scene(RING, ["light 0 -50 -20 1.0 0.9 0.8 1"] + LIGHTS[:1]),
    "light_just_outside_big_sphere_first": _scene(RING, ["light 0 3.0005 -20 1.0 0.9 0.8 1"] + LIGHTS),
    # div3_ok (rt_device.h) fails in every lane of every light: all distances below 2^-300
    "scaled_2_pow_minus_320": _scaled(_scene(RING, LIGHTS), 2.0 ** -320),
    # ... and in every lane of one light (distance above 2^300) between two ordinary ones
    "light_at_1e95": _scene(RING, [LIGHTS[0], "light 1e95 0 0 1.0 1.0 1.0 0.7", LIGHTS[1]]),
    # every hit on the inside of one sphere: c < 0 in the pre-test, with the lights inside it (no decision) ...
    "inside_one_sphere_lights_inside": ("sphere 0 0 0 50 0.8 0.8 0.8 0.3 1.0 20\n"
                                        "light 10 10 -10 1.0 1.0 1.0 0.7\nlight -5 3 2 1.0 1.0 0.8 0.5\n"
                                        "ambient 0.1 0.1 0.1\ncamera 0 2 5 0 0 -20 60\n"),
    # ... and far outside it (dist^2 > 6 r^2: in shadow by the pre-test alone)
    "inside_one_sphere_lights_outside": ("sphere 0 0 0 5 0.8 0.8 0.8 0.3 1.0 20\n"
                                         "light 10 10 -10 1.0 1.0 1.0 0.7\nlight -10 10 -10 1.0 1.0 0.8 0.5\n"
                                         "ambient 0.1 0.1 0.1\ncamera 0 2 1 0 0 -20 60\n"),
    # lights behind the ground sphere: b > 0 with disc of both signs for the lanes on the ring, c < 0 on the ground
    "lights_behind_ground_sphere": _scene(RING, ["light 0 -300 -20 1.0 1.0 1.0 0.8", "light 130 -110 -20 1.0 0.9 0.8 0.6",
                                                 LIGHTS[2]]),
}


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_light_setup_scenes_byte_identical(name, size, gpu_renderer):
    _check(gpu_renderer, TEXTS[name], size[0], size[1], DEPTH, name)


def test_check_build():
    """The bounds-checked build: the carried row, the scalar load of the global
    range and the early own-sphere load stay inside their tables."""
    import rt_hip

    r = rt_hip.Renderer(0, variant="check")
    try:
        _check(r, TEXTS["lights_7"], 24, 16, DEPTH, "lights_7, check build")
        _check(r, TEXTS["light_inside_ground_sphere"], 24, 16, DEPTH, "light_inside_ground_sphere, check build")
    finally:
        r.close()


# (generator, seed, scenes): fixed counts, a few seconds each
FUZZ = [("general", 7301, 20), ("near", 7302, 20), ("margin", 7303, 20)]


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
