"""The generated cases of the ray- and path-query tests, with their references:

  SCENES          a fixed list of (generator, seed) scenes from tests/fuzz_gen.py,
                  and dust: tiny spheres in a large box
  rays / paths / batch   per scene, a ray_ref.gen_rays batch ("gen", 1061 rays),
                  the scene's own camera rays at 33x17 ("cam"), rays from far
                  outside the query region ("far") and rays aimed at sphere
                  limbs from the region's outer shell ("limb"), their
                  path_ref.trace_paths levels and their ray-query answers
  gen_tmax_edges  tmax at the limits where the occlusion test changes its method
  lattice_*       one wave of rays with h hit lanes scattered over it, in a
                  scene of nl lights (path_kernel's lights-over-lanes pass)

Shared by test_query_cases_host.py (which pins the references to the oracle on
these scenes and asserts that the set is not degenerate) and the GPU tests
that compare the kernels with them.  Every reference is computed once per
process and never modified."""
import functools
import random

import numpy as np

import fuzz_gen
import path_ref
import ray_ref

def dust(rng):
    """64 spheres of radius about 1e-3 scattered over a box of 100: the largest radius says nothing about
    the scene's size, so the fp32 boxes' and prefilters' margins hold only if they are sized from the query
    region's diameter (a ray that grazes a sphere within 1e-5 is within an fp32 rounding of missing it)."""
    lines = []
    for _ in range(64):
        lines.append("sphere %.9g %.9g %.9g %.9g %.3f %.3f %.3f %.2f 0.5 20" % (
            rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(0.5e-3, 2e-3),
            rng.random(), rng.random(), rng.random(), rng.choice([0.0, 0.5, 1.0])))
    lines += ["light 40 60 30 1 1 1 1", "light -55 10 -20 1 1 1 1", "camera 0 0 60 0 0 -1 60"]
    return "\n".join(lines) + "\n"


GENERATORS = {
    "scene": lambda rng: fuzz_gen.scene(rng),
    "near": lambda rng: fuzz_gen.scene(rng, near=True),
    "margin": fuzz_gen.margin_scene,
    "dust": dust,
}

# (generator, seed): the scene is GENERATORS[generator](random.Random(seed)).  Chosen on the CPU for the
# sphere counts, offsets, negative radii, light counts and mirror clouds noted beside them;
# test_query_cases_host.py asserts those properties and the set's conditions.
SCENES = [
    ("scene", 2),     # 1 sphere, 2 lights
    ("scene", 6),     # 2 spheres, 6 lights
    ("scene", 3),     # 30 spheres, 5 lights
    ("scene", 5),     # 200 spheres, 4 lights
    ("scene", 7),     # 700 spheres, 3 lights
    ("scene", 17),    # 1100 spheres, 6 lights
    ("scene", 9),     # 1500 spheres, 3 lights, a mirror cloud
    ("scene", 12),    # 1500 spheres, no lights
    ("near", 19),     # 1 sphere, 4 lights
    ("near", 4),      # 30 spheres, 3 lights, a mirror cloud
    ("near", 13),     # 200 spheres, 5 lights
    ("near", 35),     # 700 spheres, 5 lights
    ("near", 25),     # 1100 spheres, 3 lights, a mirror cloud
    ("near", 11),     # 1500 spheres spread over 3000, 2 lights
    ("margin", 0),    # 4 spheres, mirrors, a light on a surface
    ("margin", 5),    # 46 spheres, 6 negative radii, moved ~900
    ("margin", 8),    # 4 spheres moved 1e5, mirrors, a negative radius
    ("margin", 1),    # 206 spheres, 12 negative radii, mirrors, moved 1e3
    ("margin", 3),    # 206 spheres moved 1e6, 17 negative radii
    ("margin", 7),    # 1115 spheres moved 1e5, 48 negative radii
    ("margin", 11),   # 1102 spheres moved 1e6, mirrors, 53 negative radii
    ("margin", 37),   # 1106 spheres at the origin, 52 negative radii
    ("dust", 0),      # 64 spheres a hundred-thousandth of the scene's size, 2 lights
]
LARGE = [(g, s) for g, s in SCENES if (g, s) in {("scene", 17), ("scene", 9), ("scene", 12), ("near", 25),
                                                 ("near", 11), ("margin", 7), ("margin", 11), ("margin", 37)}]
SUBSET = [("margin", 3), ("margin", 11)]  # one below kBvhAlwaysAbove = 1024 spheres, one above: the other builds

W, H, DEPTH = 33, 17, 4
N_GEN = 1061  # 16 full waves and a ragged tail of 37 rays
N_FAR = 101  # one full wave and a ragged tail of 37 rays
FAR = (15.0, 1e4, 1e8, 1e12, 1e16, 1e18)  # distances of the far origins, in diagonals of the scene's bounds
N_LIMB = 229  # three full waves and a ragged tail of 37 rays
LIMB = (0.0, 1e-12, -1e-12, 1e-10, -1e-10, 1e-8, -1e-8, 1e-6, -1e-6, 1e-4, -1e-4)  # relative to the tangent
KINDS = ("gen", "cam", "far", "limb")


def scene_id(case):
    return "%s%d" % case


@functools.lru_cache(maxsize=None)
def scene_text(gen, seed):
    return GENERATORS[gen](random.Random(seed))


@functools.lru_cache(maxsize=None)
def scene(gen, seed):
    """(rt_hip.Scene, path_ref.SceneArrays) of a generated scene."""
    import rt_hip

    sc = rt_hip.Scene.parse(scene_text(gen, seed))
    return sc, path_ref.SceneArrays(sc)


@functools.lru_cache(maxsize=None)
def rays(gen, seed, kind):
    """(origins, directions) of a batch of the scene: "gen" = ray_ref.gen_rays, "cam" = its camera's rays at
    W x H, "far" and "limb" below."""
    sc, sa = scene(gen, seed)
    if kind == "cam":
        r = ray_ref.camera_rays(sc.camera(), W, H)
        return r[:, 0:3].copy(), r[:, 3:6].copy()
    if kind == "far":
        # every other ray starts far behind its gen_rays origin, outside the query region: its wave holds
        # lanes of both sweeps.  From 1e16 diagonals on the hit point's rounding error exceeds the region,
        # so the shadow rays and the reflection leave from outside it too.
        o, d = ray_ref.gen_rays(300 + seed, N_FAR, sa.centers, sa.radii, tuple(sc.camera().position))
        diag = bounds(sc)[2]
        odd = np.arange(1, N_FAR, 2)
        back = np.array([FAR[k % len(FAR)] for k in range(odd.size)]) * diag
        o[odd] -= ray_ref.normalize(d[odd]) * back[:, None]
        return o, d
    if kind == "limb":
        return limb_rays(gen, seed)[:2]
    return ray_ref.gen_rays(100 + seed, N_GEN, sa.centers, sa.radii, tuple(sc.camera().position))


@functools.lru_cache(maxsize=None)
def limb_rays(gen, seed):
    """(origins, directions, the sphere aimed at, e) of the scene's "limb" batch.  A ray is aimed at a
    sphere's limb: the sine of its angle with the line to the centre is (r / D) (1 + e), e from LIMB, so it
    is tangent up to rounding, or passes just inside or outside.  The
    even rays start in the shell of the query region outside the scene's bounds, up to 0.9 diagonals from
    them, where the fp32 boxes' and prefilters' margins (sized for the region) matter most; the odd ones
    inside the bounds."""
    sc, sa = scene(gen, seed)
    n = N_LIMB
    rng = np.random.default_rng(500 + seed)
    lo, hi, diag = bounds(sc)
    sign = rng.choice([-1.0, 1.0], (n, 3))
    shell = 0.5 * (lo + hi) + sign * (0.5 * (hi - lo) + 0.9 * diag * rng.uniform(0.5, 1.0, (n, 1)))
    o = np.where((np.arange(n) % 2 == 0)[:, None], shell, lo + (hi - lo) * rng.random((n, 3)))
    s = rng.integers(0, len(sa.radii), n)
    to_c = sa.centers[s] - o
    dist = np.sqrt((to_c ** 2).sum(axis=1))
    u = to_c / dist[:, None]
    p = np.cross(u, rng.normal(size=(n, 3)))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    e = np.array([LIMB[k % len(LIMB)] for k in range(n)])
    sin = np.minimum(np.abs(sa.radii[s]) / dist * (1.0 + e), 0.999)  # an origin inside the sphere: any direction
    d = u * np.sqrt(1.0 - sin * sin)[:, None] + p * sin[:, None]
    return o, d * rng.uniform(0.5, 2.0, (n, 1)), s, e  # any direction length


@functools.lru_cache(maxsize=None)
def paths(gen, seed, kind):
    o, d = rays(gen, seed, kind)
    return path_ref.trace_paths(o, d, DEPTH, scene(gen, seed)[1])


def bounds(sc):
    """The scene's bounds (spheres and lights) and their diagonal: (lo, hi, diag)."""
    c, r = ray_ref.spheres_of(sc)
    pts_lo = [c - np.abs(r)[:, None]] + [np.array([sc.light(i)["position"]]) for i in range(sc.num_lights)]
    pts_hi = [c + np.abs(r)[:, None]] + pts_lo[1:]
    lo, hi = np.concatenate(pts_lo).min(axis=0), np.concatenate(pts_hi).max(axis=0)
    return lo, hi, float(np.sqrt(((hi - lo) ** 2).sum()))


def query_region(sc):
    """The bounds grown on every side by their own diagonal: (lo, hi)."""
    lo, hi, diag = bounds(sc)
    return lo - diag, hi + diag


def slow_rays(sc, o, d):
    """bool [n]: the rays that must take the every-sphere sweep (origin outside the query region or not
    finite, or a direction that is not finite once normalised)."""
    rlo, rhi = query_region(sc)
    with np.errstate(invalid="ignore"):
        inside = ((o >= rlo) & (o <= rhi)).all(axis=1)
    return ~(inside & np.isfinite(ray_ref.normalize(d)).all(axis=1))


def paths_unaccelerated(gen, seed, kind, first_level=0):
    """path_ref.unaccelerated of the batch's levels first_level .. DEPTH - 1."""
    sc, sa = scene(gen, seed)
    levels = paths(gen, seed, kind)
    rlo, rhi = query_region(sc)
    org = rays(gen, seed, kind)[0]
    if first_level > 0:
        up = levels[first_level - 1]
        org = up["hit"] + up["normal"] * path_ref.EPSILON
    return path_ref.unaccelerated(levels[first_level:], org, sa, rlo, rhi)


# ---- tmax at the occlusion test's thresholds -----------------------------------------------
# The limits at which the occlusion test changes its method (rt_device.h sweep_shadow): it decides
# t < tmax without a division when the numerator lies outside q(1 +- 2^-48), and takes the exact test for
# tmax < 2^-900, a NaN tmax and a tmax clamped at 1e20.
REL_EXPONENTS = (46, 47, 48, 49, 50, 52)
ULP_STEPS = (1, 2, 4)
TMAX_EDGE_CLASSES = (ray_ref.TMAX_CLASSES
                     + tuple("t(1%s2^-%d)" % (s, k) for k in REL_EXPONENTS for s in "+-")
                     + tuple("t%s%dulp" % (s, k) for k in ULP_STEPS for s in "+-")
                     + ("1e20", "below1e20", "1e21", "dblmax", "2^-900", "2^-901", "denorm_min"))


def _step_ulps(x, k, towards):
    for _ in range(k):
        x = np.nextafter(x, towards)
    return x


def gen_tmax_edges(seed, t_ref):
    """ray_ref.gen_tmax's classes (left as they are), then around the reference's closest t: t(1 +- 2^-k)
    for k in REL_EXPONENTS, t moved by +-1, +-2 and +-4 ulps, and the constants 1e20, the double below it,
    1e21, DBL_MAX, 2^-900, 2^-901 and 5e-324 (TMAX_EDGE_CLASSES, in that order).  Returns (tmax [n], class
    index [n])."""
    rng = np.random.default_rng(seed)
    t_ref = np.asarray(t_ref, np.float64)
    n = t_ref.shape[0]
    cls = np.arange(n) % len(TMAX_EDGE_CLASSES)
    rng.shuffle(cls)
    rows = [np.full(n, np.inf), t_ref, np.nextafter(t_ref, np.inf), 0.5 * t_ref, np.zeros(n), np.full(n, -1.0),
            np.full(n, np.nan)]
    for k in REL_EXPONENTS:
        rows += [t_ref * (1.0 + 2.0 ** -k), t_ref * (1.0 - 2.0 ** -k)]
    for k in ULP_STEPS:
        rows += [_step_ulps(t_ref, k, np.inf), _step_ulps(t_ref, k, -np.inf)]
    rows += [np.full(n, v) for v in (1e20, np.nextafter(1e20, 0.0), 1e21, np.finfo(np.float64).max, 2.0 ** -900,
                                     2.0 ** -901, 5e-324)]
    assert len(rows) == len(TMAX_EDGE_CLASSES)
    return np.stack(rows)[cls, np.arange(n)], cls


class RayBatch:
    """Rays with their ray-query answers, the attributes test_gpu_rays.check_parity reads."""

    def __init__(self, sc, o, d, t, sphere, tmax_seed):
        self.scene, self.o, self.d, self.t, self.sphere = sc, o, d, t, sphere
        self.tmax, self.cls = gen_tmax_edges(tmax_seed, t)
        self.occ = ray_ref.occluded(t, sphere, self.tmax)

    @property
    def hit_share(self):
        return float((self.sphere >= 0).mean())


@functools.lru_cache(maxsize=None)
def batch(gen, seed, kind):
    """The scene's batch as a ray query: level 0 of its paths is the closest hit."""
    o, d = rays(gen, seed, kind)
    lv = paths(gen, seed, kind)[0]
    return RayBatch(scene(gen, seed)[0], o, d, lv["t"], lv["sphere"], 200 + seed)


N_EDGE = 4133  # 64 full waves and a ragged tail of 37 rays


@functools.lru_cache(maxsize=None)
def edge_batch(which):
    """4133 gen_rays rays with the edge classes of tmax, on complex.txt ("complex") or a generated scene."""
    import rt_hip
    from conftest import scene_path

    sc = rt_hip.Scene.load(scene_path("complex")) if which == "complex" else scene(*which)[0]
    c, r = ray_ref.spheres_of(sc)
    o, d = ray_ref.gen_rays(7, N_EDGE, c, r, tuple(sc.camera().position))
    t, s = ray_ref.closest(o, d, c, r)
    return RayBatch(sc, o, d, t, s, 8)


# ---- the lights-over-lanes lattice ---------------------------------------------------------
LATTICE_NL = (2, 3, 7, 13, 32, 33, 63, 64)
LATTICE_H = (1, 2, 3, 5, 8, 13, 21, 31, 32, 33, 64)
LATTICE_SEED = 0  # chosen so that the references meet test_query_cases_host.py's lattice conditions
_MIRROR = (0.0, 0.0, -5.0)  # TWO's reflective sphere, radius 1


@functools.lru_cache(maxsize=None)
def lattice_text(nl):
    """The reflective sphere at (0, 0, -5), eight occluders of radius 0.6 two units from its centre (none
    between it and the origin), and nl lights: the first and the last beside the cap the rays hit, the rest
    in (-6, 6)^3."""
    rng = np.random.default_rng([LATTICE_SEED, nl])
    lines = ["sphere 0 0 -5 1 1 0 0 0.5 1 10"]
    k = 0
    while k < 8:
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        if u[2] > 0.6:  # in or near the cone of the rays from the origin
            continue
        p = np.array(_MIRROR) + 2.0 * u
        lines.append("sphere %r %r %r 0.6 0 1 0 0 1 10" % tuple(float(v) for v in p))
        k += 1
    pos = rng.uniform(-6.0, 6.0, (nl, 3))
    # the first and the last light graze the cap the rays hit: lit from one side of it, behind the mirror's
    # own horizon from the other
    pos[0], pos[nl - 1] = (5.0, 0.5, -4.15), (-0.5, -5.0, -4.15)
    for p in pos:
        lines.append("light %r %r %r 1 1 1 1" % tuple(float(v) for v in p))
    lines.append("camera 0 0 0 0 0 -1 60")
    return "\n".join(lines) + "\n"


@functools.lru_cache(maxsize=None)
def lattice_rays(h):
    """64 rays from the origin: h of them, at the lanes of a seeded permutation, aimed into the mirror's
    cone; the others aimed away from every sphere.  Returns (origins, directions, the hit lanes sorted)."""
    rng = np.random.default_rng([LATTICE_SEED, 1000 + h])
    lanes = np.sort(rng.permutation(64)[:h])
    d = np.stack([rng.uniform(-0.5, 0.5, 64), rng.uniform(-0.5, 0.5, 64), np.ones(64)], axis=1)  # +z: a miss
    rad = 0.18 * np.sqrt(rng.random(h))  # tan of the angle off the axis; the cone's edge is at 0.204
    ang = rng.uniform(0.0, 2.0 * np.pi, h)
    d[lanes] = np.stack([rad * np.cos(ang), rad * np.sin(ang), -np.ones(h)], axis=1)
    return np.zeros((64, 3)), d, lanes


@functools.lru_cache(maxsize=None)
def lattice_ref(nl, h):
    """(rt_hip.Scene, SceneArrays, origins, directions, hit lanes, the depth-2 levels) of a lattice case."""
    import rt_hip

    sc = rt_hip.Scene.parse(lattice_text(nl))
    sa = path_ref.SceneArrays(sc)
    o, d, lanes = lattice_rays(h)
    return sc, sa, o, d, lanes, path_ref.trace_paths(o, d, 2, sa)
