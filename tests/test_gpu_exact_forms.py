"""GPU: the predicated exact ray-sphere test of the render kernels' list loops.

The shadow lists, the camera grid, the sphere grids and the BVH / grid-line
leaf tests decide a candidate with lane predicates and wave-uniform branches
(rt_device.h exact_num, shadow_exact, closest_test): the square root, the
division and the rare classes (a numerator in the band around the light's
distance, a tiny numerator, a lane that is not `fast`) are entered by the
whole wave when some lane needs them.  A lane's bits are what the chain of
per-lane branches gave it, so every render here equals the oracle
(oracle/orc.py) byte for byte and ray count for ray count: as a one-frame
launch (the wide light loop, one tile per wave) and as a three-frame launch
(four tiles per wave, the deferred kernel), at 64x48 and 24x16, depth 4.  The
scenes put each rare class into waves of its own and beside ordinary lanes;
the fuzz generators (tests/fuzz_gen.py) add 20 scenes each of a fixed seed."""
import os
import random

import pytest

import fuzz_gen
from conftest import SCENES
from test_gpu_light_paths import LIGHTS, _check, _ring, _scene

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (24, 16)]
DEPTH = 4

# the camera exactly on the surface of a sphere, in dyadic coordinates: c =
# |o - C|^2 - r^2 = 0 for every camera ray, so disc = b^2 and one numerator is
# exactly 0 -- the tiny-numerator (cold) class in every lane of every wave
CAMERA_ON_SPHERE = ("sphere 0 0 -5 5 0.8 0.3 0.3 0.3 1.0 20\n"
                    "sphere 1.5 0.5 -3 0.5 0.2 0.8 0.3 0.5 1.0 10\n"
                    "sphere -1 -0.5 -2 0.25 0.2 0.3 0.9 0.0 1.0 40\n"
                    "light 0 3 -4 1.0 1.0 1.0 0.8\nlight 2 0 -1 0.8 0.8 1.0 0.5\nambient 0.1 0.1 0.1\n"
                    "camera 0 0 0 0 0 -1 60\n")

# a light exactly on the big sphere's surface (centre 0 0 -20, radius 3) and
# one 0.0005 outside it: shadow roots at the edge of the band around the
# light's distance
LIGHT_ON_SPHERE = _scene(_ring(lambda k: "20"), LIGHTS + ["light 0 3 -20 1.0 0.9 0.8 1", "light 3.0005 0 -20 0.9 1.0 0.8 1"])

# two unit spheres touching on the camera's axis-aligned central line, lights
# on the coordinate axes through the point of contact: exactly tangent lines
TANGENT = ("sphere 1 0 -5 1 1 1 1 0 1 1\nsphere -1 0 -5 1 1 0 1 0.3 1 3\nsphere 0 2 -5 1 0.3 1 1 0.5 1 8\n"
           "light 0 0 10 1 1 1 1\nlight 0 -6 -5 1 1 1 0.6\nlight 0 1 3 0.8 0.8 1 0.5\ncamera 0 0 0 0 0 -5 60\n")

# the rare classes beside ordinary lanes: at 24x16 an 8x8 tile of this scene
# holds pixels of the ring (ordinary), of the sphere the camera sits on (cold),
# of the touching pair (tangent) and points lit from the light on the surface
MIXED = ("sphere 0 -2 0 2 0.7 0.7 0.7 0.4 1.0 20\n"  # the camera at 0 0 0 is on it
         "sphere 1 0 -5 1 1 1 1 0 1 1\nsphere -1 0 -5 1 1 0 1 0.3 1 3\n" +
         "\n".join(_ring(lambda k: "20" if k % 3 else "33.3", n=12)) + "\n" +
         "light 0 3 -20 1.0 0.9 0.8 1\nlight 0 0 10 1 1 1 0.7\nlight -10 10 -10 1.0 1.0 0.8 0.5\n"
         "ambient 0.1 0.1 0.1\ncamera 0 0 0 0 0 -5 60\n")

TEXTS = {
    "ring_all_ordinary": _scene(_ring(lambda k: "20"), LIGHTS),
    "camera_on_sphere": CAMERA_ON_SPHERE,
    "light_on_and_just_outside_sphere": LIGHT_ON_SPHERE,
    "tangent_axis_aligned": TANGENT,
    "mixed_in_one_tile": MIXED,
}


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_class_scenes_byte_identical(name, size, gpu_renderer):
    _check(gpu_renderer, TEXTS[name], size[0], size[1], DEPTH, name)


@pytest.mark.parametrize("size", [(1, 1), (2, 2)], ids=["1x1", "2x2"])
@pytest.mark.parametrize("name", ["simple", "mixed_in_one_tile"])
def test_tiny_images(name, size, gpu_renderer):
    """1x1: W - 1 = 0 makes the camera ray NaN; 2x2: stretched rays.  Lanes
    that are not `fast`, in a wave with nothing else."""
    if name == "simple":
        with open(os.path.join(SCENES, "simple.txt")) as f:
            text = f.read()
    else:
        text = TEXTS[name]
    _check(gpu_renderer, text, size[0], size[1], DEPTH, name)


def test_check_build():
    """The bounds-checked build on the mixed scene: no device index of the
    predicated loops is out of range."""
    import rt_hip

    r = rt_hip.Renderer(0, variant="check")
    try:
        _check(r, MIXED, 24, 16, DEPTH, "mixed, check build")
    finally:
        r.close()


# (generator, seed, scenes): fixed counts, a few seconds each
FUZZ = [("general", 6101, 20), ("near", 6102, 20), ("margin", 6103, 20)]


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
