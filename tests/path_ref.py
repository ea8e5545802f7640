"""numpy restatement of the reference's trace_ray, the checker of the path
query's tests (rt_trace_paths):

  trace_ray's skeleton   src/main.cpp:16-58     -> trace_paths
  Sphere::normal_at      include/sphere.h:62-64 -> trace_paths (normal)
  Scene::in_shadow       include/scene.h:65-86  -> in_shadow
  Scene::shade           include/scene.h:89-121 -> shade
  trace_ray's compositing and sky, main.cpp:28-29, 52-53 -> shade
  write_ppm's quantiser  src/main.cpp:85-87     -> quantize

It builds on ray_ref (normalize, closest).  Every expression keeps the
reference's operand order and association; numpy's elementwise fp64 operations
are correctly rounded and never contracted, so the path records are the
reference's bit for bit, and the colours are too wherever glibc's pow is the
one called (math.pow, not numpy's vectorised pow).  test_paths_host.py pins it
to the oracle-made goldens and their ray counts."""
from __future__ import annotations

import math

import numpy as np

import ray_ref

INF = ray_ref.INF
EPSILON = 0.001      # ray_math_constants.h:22
K_SPECULAR = 0.5     # scene.h:38
MAX_LIGHTS = 64      # RT_PATH_MAX_LIGHTS: bits of the shadow mask

_pow = np.frompyfunc(math.pow, 2, 1)


class SceneArrays:
    """The fields of an rt_hip.Scene the checker reads, as arrays."""

    def __init__(self, scene):
        m, nl = scene.num_spheres, scene.num_lights
        self.centers, self.radii = ray_ref.spheres_of(scene)
        sp = [scene.sphere(i) for i in range(m)]
        self.color = np.array([s["color"] for s in sp], np.float64).reshape(m, 3)
        self.refl = np.array([s["reflectivity"] for s in sp], np.float64)
        self.shin = np.array([s["shininess"] for s in sp], np.float64)
        lt = [scene.light(i) for i in range(nl)]
        self.lpos = np.array([l["position"] for l in lt], np.float64).reshape(nl, 3)
        self.lcol = np.array([l["color"] for l in lt], np.float64).reshape(nl, 3)
        self.ambient = np.array(list(scene.raw.ambient), np.float64)


def _arrays(scene):
    return scene if isinstance(scene, SceneArrays) else SceneArrays(scene)


def dot(a, b):
    """dot(), vec3.h:23-25: a.x*b.x + a.y*b.y + a.z*b.z."""
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def length(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def max0(x):
    """std::max(0.0, x): x when 0.0 < x, else 0.0 (a NaN gives 0.0)."""
    return np.where(0.0 < x, x, 0.0)


def shadow_ray(hit, lpos):
    """The ray in_shadow builds for one light (scene.h:70-76): (origin, the
    direction handed to Ray(), the light distance)."""
    to_light = lpos[None, :] - hit
    dist = length(to_light)
    ldir = ray_ref.normalize(to_light)
    return hit + ldir * EPSILON, ldir, dist


def in_shadow(hit, lpos, sa):
    """Scene::in_shadow for points hit [k,3] and one light: bool [k].  Ray()
    normalises the direction again (ray_ref.closest does)."""
    if hit.shape[0] == 0:
        return np.zeros(0, bool)
    with np.errstate(all="ignore"):
        so, ldir, dist = shadow_ray(hit, lpos)
        t, s = ray_ref.closest(so, ldir, sa.centers, sa.radii)
        return (s >= 0) & (t < dist)


def trace_paths(o, d, depth, scene):
    """The geometric skeleton of trace_ray(Ray(o[i], d[i]), scene, depth) for
    every ray: a list of `depth` levels, each a dict of arrays over the n rays

      traced [n] bool     this level's ray was traced
      t [n], sphere [n]   find_intersection's answer (1e20, -1 on a miss or an
                          untraced level)
      reflects [n] bool   a reflection ray was spawned (the next level is traced)
      shadowed [n] uint64 bit l: in_shadow(hit, lights[l])
      dir, hit, normal, view [n,3]   the direction stored in the level's Ray,
                          ray.origin + ray.direction*t, normal_at(hit) and
                          (ray.origin - hit).normalized(); zeros where the
                          level is untraced, hit / normal / view zeros on a miss
    """
    sa = _arrays(scene)
    nl = sa.lpos.shape[0]
    assert nl <= MAX_LIGHTS
    org = np.array(np.asarray(o, np.float64).reshape(-1, 3))
    n = org.shape[0]
    dirs = ray_ref.normalize(d)  # Ray(o, d), ray.h:12
    alive = np.ones(n, bool)
    levels = []
    for k in range(depth):
        lv = {"traced": alive.copy(), "t": np.full(n, INF), "sphere": np.full(n, -1, np.int32),
              "reflects": np.zeros(n, bool), "shadowed": np.zeros(n, np.uint64),
              "dir": np.zeros((n, 3)), "hit": np.zeros((n, 3)), "normal": np.zeros((n, 3)), "view": np.zeros((n, 3))}
        idx = np.flatnonzero(alive)
        nxt = np.zeros(n, bool)
        if idx.size:
            with np.errstate(all="ignore"):
                ok, dk = org[idx], dirs[idx]
                # the stored direction is already normalised; closest() divides by its length once more only
                # for a caller's direction, so hand it the bits as they are
                t, s = _closest_stored(ok, dk, sa)
                lv["t"][idx], lv["sphere"][idx], lv["dir"][idx] = t, s, dk
                h = np.flatnonzero(s >= 0)
                hi = idx[h]
                hit = ok[h] + dk[h] * t[h, None]                                   # main.cpp:32
                normal = ray_ref.normalize(hit - sa.centers[s[h]])                 # sphere.h:62-64
                view = ray_ref.normalize(ok[h] - hit)                              # main.cpp:38
                lv["hit"][hi], lv["normal"][hi], lv["view"][hi] = hit, normal, view
                mask = np.zeros(h.size, np.uint64)
                for l in range(nl):
                    mask |= in_shadow(hit, sa.lpos[l], sa).astype(np.uint64) << np.uint64(l)
                lv["shadowed"][hi] = mask
                spawn = (sa.refl[s[h]] > 0) & (depth - (k + 1) >= 1)               # main.cpp:43, :17
                sp = np.flatnonzero(spawn)
                dd, nn = dk[h][sp], normal[sp]
                rdir = dd - (nn * 2.0) * dot(dd, nn)[:, None]                      # main.cpp:45
                org[hi[sp]] = hit[sp] + nn * EPSILON                               # main.cpp:48
                dirs[hi[sp]] = ray_ref.normalize(rdir)
                lv["reflects"][hi[sp]] = True
                nxt[hi[sp]] = True
        alive = nxt
        levels.append(lv)
    return levels


def _closest_stored(o, dn, sa):
    """find_intersection for rays whose stored direction is dn (no further
    normalisation): ray_ref.closest's scan over ray_ref.intersect."""
    n = o.shape[0]
    t_out = np.full(n, INF)
    s_out = np.full(n, -1, np.int32)
    for k in range(0, n, 256):
        hit, t = ray_ref.intersect(o[k:k + 256], dn[k:k + 256], sa.centers, sa.radii)
        if hit.shape[1] == 0:
            continue
        key = np.where(hit & (t < INF), t, np.inf)
        idx = np.argmin(key, axis=1)
        best = key[np.arange(key.shape[0]), idx]
        ok = best < INF
        t_out[k:k + 256] = np.where(ok, best, INF)
        s_out[k:k + 256] = np.where(ok, idx, -1)
    return t_out, s_out


def counts(levels, scene):
    """(rays, segments, hits, shadow_rays) of a path batch: the launch's
    rt_path_stats, and the manifest's primary / reflect + primary / shadow."""
    sa = _arrays(scene)
    segments = int(sum(int(lv["traced"].sum()) for lv in levels))
    hits = int(sum(int((lv["traced"] & (lv["sphere"] >= 0)).sum()) for lv in levels))
    return int(levels[0]["traced"].shape[0]), segments, hits, hits * sa.lpos.shape[0]


def unaccelerated(levels, origins, scene, rlo, rhi):
    """Closest-hit and shadow queries of the batch that must take the
    every-sphere sweep: the segment's / shadow ray's origin lies outside the
    region [rlo, rhi] (or is not finite) or its normalised direction is not
    finite.  `origins` are the level-0 origins."""
    sa = _arrays(scene)

    def slow(o, dn):
        with np.errstate(invalid="ignore"):
            inside = ((o >= rlo) & (o <= rhi)).all(axis=1)
        return int((~(inside & np.isfinite(dn).all(axis=1))).sum())

    total = 0
    org = np.asarray(origins, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        for lv in levels:
            tr = lv["traced"]
            total += slow(org[tr], lv["dir"][tr])
            h = tr & (lv["sphere"] >= 0)
            for l in range(sa.lpos.shape[0]):
                so, ldir, _ = shadow_ray(lv["hit"][h], sa.lpos[l])
                total += slow(so, ray_ref.normalize(ldir))
            org = lv["hit"] + lv["normal"] * EPSILON  # the next level's origin where it is traced
    return total


def shade(levels, scene):
    """trace_ray's colour [n,3] from the path records: Scene::shade per hit
    (the lights whose shadow bit is clear, in file order), the sky on a miss,
    and main.cpp:53's compositing from the deepest level up.  Reads traced,
    sphere, reflects, shadowed, dir, hit, normal and view of each level."""
    sa = _arrays(scene)
    n = levels[0]["traced"].shape[0]
    below = np.zeros((n, 3))  # trace_ray(depth 0): black
    with np.errstate(all="ignore"):
        for lv in reversed(levels):
            col = np.zeros((n, 3))
            tr = np.asarray(lv["traced"], bool)
            s = np.asarray(lv["sphere"])
            miss = np.flatnonzero(tr & (s < 0))
            st = 0.5 * (lv["dir"][miss, 1] + 1.0)                                   # main.cpp:28-29
            col[miss] = np.ones((1, 3)) * (1.0 - st)[:, None] + np.array([[0.5, 0.7, 1.0]]) * st[:, None]
            h = np.flatnonzero(tr & (s >= 0))
            if h.size:
                si = s[h]
                point, normal, view = lv["hit"][h], lv["normal"][h], lv["view"][h]
                mc, refl, shin = sa.color[si], sa.refl[si], sa.shin[si]
                color = sa.ambient[None, :] * mc                                    # scene.h:92
                shadowed = np.asarray(lv["shadowed"], np.uint64)[h]
                for l in range(sa.lpos.shape[0]):
                    lit = ((shadowed >> np.uint64(l)) & np.uint64(1)) == 0
                    light_dir = ray_ref.normalize(sa.lpos[l][None, :] - point)      # scene.h:104
                    ndl = max0(dot(normal, light_dir))
                    diffuse = (mc * (1.0 - refl)[:, None]) * ndl[:, None]           # scene.h:107
                    v = light_dir * -1.0
                    reflect_dir = v - (normal * 2.0) * dot(v, normal)[:, None]      # vec3.h:31-33
                    rdv = max0(dot(reflect_dir, view))
                    spec = np.zeros(h.size)
                    spec[lit] = _pow(rdv[lit], shin[lit]).astype(np.float64)        # glibc pow, scene.h:113
                    specular = (sa.lcol[l][None, :] * K_SPECULAR) * spec[:, None]
                    color = np.where(lit[:, None], (specular + diffuse) + color, color)  # scene.h:117
                mirror = refl > 0                                                   # main.cpp:43
                mixed = color * (1.0 - refl)[:, None] + below[h] * refl[:, None]    # main.cpp:53
                col[h] = np.where(mirror[:, None], mixed, color)
            below = col
    return below


def quantize(rgb):
    """write_ppm's int(255.99 * std::min(1.0, c)) per channel as uint8 [n,3]; a
    negative value is stored as 0, as the library and the goldens do."""
    c = np.asarray(rgb, np.float64)
    v = 255.99 * np.where(c < 1.0, c, 1.0)
    return np.clip(np.trunc(v), 0, 255).astype(np.uint8)
