"""GPU: the lane predicates of the render kernel's common light iteration.

shade_hit's lane-per-ray loop (rt_kernel.hip, kFast && kTwoForms) decides per
light and wave between the straight-line shadow query and the general one
(rt_device.h light_common).  The guard's forms changed, its decisions did not:
the loop no longer tests lg.on (the host picks these kernels only with the
light grids on), the host's off_free bound is folded once per call into the
width of the one range compare on renorm_near_one's t, and the three usable()
tests are one compare on the smallest exponent.  (The own-sphere pre-test's
bound formed once per hit and the branch-free cell of the same plan were
measured and not kept, profiles/r15a; their scenes stay, the texts they
exercise are the loop's.)  A lane's bits are what they
were, so every render equals the oracle (oracle/orc.py) byte for byte and ray
count for ray count: as a one-frame launch and as a three-frame launch, at
64x48 and 24x16, depth 4, on the product build and on the check build.

The scenes, per guard:
 * a zero component of the light direction (usable()'s x == 0 allowance): the
   lights share x with the camera and the big sphere, z with the big sphere.
   Whether a hit point's coordinate equals the light's exactly is up to the
   camera rays' rounding and no scene text forces it; the class is produced and
   counted by tests/native/predicate_forms_check.cpp (components 0, -0);
 * the scene moved 1e9 along x: off_free is false, every wave of every light
   is rare (the bound is per scene, so there is no mixed wave of this guard);
 * a light inside and one just outside a sphere: the own-sphere pre-test's
   c < 0 lanes beside c > 0 lanes in one tile, dist^2 on both sides of 6 r^2;
 * squared radii outside (1e-200, 1e38): every ray that leaves the ring hits
   the inside of a sphere of radius 2e19 around the scene, with a light 1e20
   away (dist^2 > 6 r^2, c < 0 by rounding in some lanes: the bound must be the
   one that never decides), in tiles that also hold ring spheres; and a sphere
   of radius 1e-101 around the camera, hit by every camera ray.  A shadow
   origin inside that sphere cannot be made (the query starts 0.001 off the
   hit point), so r^2 <= 1e-200 with c < 0 is the CPU checker's as well;
 * a NaN camera ray (1x1 image): all lanes rare by t = NaN.
t just outside [-4, 6], components one ulp below 2^-959 and a NaN distance
are no scene's to make: the CPU checker generates them.
The fuzz generators (tests/fuzz_gen.py) add 3 x 20 scenes at fixed seeds."""
import os
import random

import pytest

import fuzz_gen
from conftest import SCENES
from test_gpu_light_paths import LIGHTS, _check, _ring, _scene

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (24, 16)]
DEPTH = 4
RING = _ring(lambda k: "20")

TEXTS = {
    "all_common": _scene(RING, LIGHTS),
    # x of camera, look-at point and big sphere is 0; z of the big sphere is -20
    "light_shares_coordinates": _scene(RING, ["light 0 12 -20 1.0 1.0 1.0 0.7", "light 0 2 5 0.8 0.8 1.0 0.5",
                                             "light 7 0 -20 1.0 0.9 0.8 0.5"]),
    "moved_1e9_along_x": _scene(_ring(lambda k: "20", x0=1e9),
                                ["light %.17g 10 -10 1.0 1.0 1.0 0.7" % (1e9 + 10),
                                 "light %.17g 10 -10 1.0 1.0 0.8 0.5" % (1e9 - 10),
                                 "light %.17g 12 -2 0.6 0.6 1.0 0.5" % 1e9], x0=1e9),
    "light_inside_and_just_outside_a_sphere": _scene(RING, ["light 0.5 0.25 -20 1.0 0.9 0.8 1", LIGHTS[0],
                                                            "light 0 3.0005 -20 1.0 0.9 0.8 1"]),
    "radius_2e19_around_the_scene": _scene(RING + ["sphere 0 0 0 2e19 0.3 0.4 0.6 0.0 1.0 20"],
                                           [LIGHTS[0], "light 1e20 0 0 1.0 1.0 1.0 0.7", LIGHTS[1]]),
    "radius_1e-101_around_the_camera": _scene(RING + ["sphere 0 2 5 1e-101 0.9 0.9 0.9 0.5 1.0 20"], LIGHTS),
}


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
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_predicate_scenes_byte_identical(name, size, renderer):
    _check(renderer, TEXTS[name], size[0], size[1], DEPTH, name)


def test_nan_camera_ray(renderer):
    """simple.txt at 1x1: W - 1 = 0 makes the camera ray NaN, every lane rare."""
    with open(os.path.join(SCENES, "simple.txt")) as f:
        text = f.read()
    _check(renderer, text, 1, 1, DEPTH, "simple 1x1")


# (generator, seed, scenes): fixed counts
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
