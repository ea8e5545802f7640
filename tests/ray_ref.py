"""numpy restatement of the reference's ray-sphere test and closest-hit scan,
the checker of the ray-query tests (rt_trace_rays):

  Vec3::normalized       include/vec3.h:19-20   -> normalize
  Sphere::intersect      include/sphere.h:26-59 -> intersect
  Scene::find_intersection include/scene.h:41-61 -> closest
  Scene::in_shadow's test  include/scene.h:78-82 -> occluded
  Camera::get_ray        include/camera.h:17-25 -> camera_rays
  the ray generator of the tests                -> gen_rays, gen_tmax

Every expression keeps the reference's operand order and association;
numpy's elementwise fp64 operations are correctly rounded and never
contracted, so the results are the reference's bit for bit (checked against
the oracle's orc_intersect in test_rays_host.py)."""
from __future__ import annotations

import numpy as np

INF = 1e20  # INFINITY_DOUBLE, ray_math_constants.h:23


def normalize(v):
    """Vec3::normalized: len = sqrt(x*x + y*y + z*z), then x/len, y/len, z/len."""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        ln = np.sqrt((x * x + y * y) + z * z)
        return np.stack([x / ln, y / ln, z / ln], axis=1)


def spheres_of(scene):
    """(centres [m,3], radii [m]) of an rt_hip.Scene."""
    m = scene.num_spheres
    c = np.array([scene.sphere(i)["center"] for i in range(m)], np.float64).reshape(m, 3)
    r = np.array([scene.sphere(i)["radius"] for i in range(m)], np.float64)
    return c, r


def intersect(o, d, centers, radii):
    """Sphere::intersect for rays (o, d) [n,3] (d as stored in the Ray: already
    normalised) against spheres [m]: (hit [n,m] bool, t [n,m]); t is 0 where
    hit is false (find_intersection's temp_t)."""
    o = np.asarray(o, np.float64).reshape(-1, 1, 3)
    d = np.asarray(d, np.float64).reshape(-1, 1, 3)
    c = np.asarray(centers, np.float64).reshape(1, -1, 3)
    r = np.asarray(radii, np.float64).reshape(1, -1)
    with np.errstate(all="ignore"):
        ocx, ocy, ocz = o[..., 0] - c[..., 0], o[..., 1] - c[..., 1], o[..., 2] - c[..., 2]
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        a = (dx * dx + dy * dy) + dz * dz
        b = 2.0 * ((ocx * dx + ocy * dy) + ocz * dz)
        cc = ((ocx * ocx + ocy * ocy) + ocz * ocz) - r * r
        disc = b * b - (4 * a) * cc
        a2 = 2 * a
        neg = disc < 0
        tangent = ~neg & (disc == 0)
        t0 = -b / a2
        sq = np.sqrt(np.where(neg, 0.0, disc))
        t1 = (-b - sq) / a2
        t2 = (-b + sq) / a2
        tmax = np.where(t1 < t2, t2, t1)  # std::max(t1, t2)
        tmin = np.where(t2 < t1, t2, t1)  # std::min(t1, t2)
        behind = ~neg & ~tangent & (tmax < 0)
        t = np.where(tmin < 0, tmax, tmin)
        hit = ~neg & ~behind
        t = np.where(tangent, t0, t)
        t = np.where(hit, t, 0.0)
    hit, t = np.broadcast_arrays(hit, t)
    return hit, t


def closest(origins, directions, centers, radii, chunk=256):
    """Scene::find_intersection for Ray(origin, direction) (the direction is
    normalised once here, as Ray() does): (t [n], sphere [n] int32); t = 1e20 and
    sphere = -1 on a miss.  File order with strict <: ties keep the lowest
    index; a NaN t is never recorded."""
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    d = normalize(directions)
    n = o.shape[0]
    t_out = np.full(n, INF)
    s_out = np.full(n, -1, np.int32)
    for k in range(0, n, chunk):
        hit, t = intersect(o[k:k + chunk], d[k:k + chunk], centers, radii)
        if hit.shape[1] == 0:
            continue
        with np.errstate(all="ignore"):
            key = np.where(hit & (t < INF), t, np.inf)  # NaN < x is false: never recorded
        idx = np.argmin(key, axis=1)  # the first minimum: the lowest index of a tie
        best = key[np.arange(key.shape[0]), idx]
        ok = best < INF
        t_out[k:k + chunk] = np.where(ok, best, INF)
        s_out[k:k + chunk] = np.where(ok, idx, -1)
    return t_out, s_out


def occluded(t, sphere, tmax):
    """in_shadow's test with tmax for the light distance: find_intersection
    found a sphere (so its t < 1e20) and t < tmax."""
    with np.errstate(all="ignore"):
        return ((np.asarray(sphere) >= 0) & (np.asarray(t) < np.asarray(tmax, np.float64))).astype(np.int32)


def camera_rays(cam, W, H, rows=None):
    """get_ray's rays for output rows `rows` (an rt_rows; None = every row) as
    [count*W, 8] rt_ray records: origin, the once-normalised direction, tmax =
    +inf, reserved = 0; padding rows (y >= H) are all zero."""
    band, first, stride, count = (rows.band, rows.first, rows.stride, rows.count) if rows is not None else (1, 0, 1, H)
    out = np.zeros((count, W, 8), np.float64)
    fwd, right, up = (np.array(list(v), np.float64) for v in (cam.forward, cam.right, cam.up))
    xs = np.arange(W, dtype=np.float64)
    for k in range(count):
        y = (k // band) * band * stride + first * band + k % band
        if y >= H:
            continue
        j = H - 1 - y
        with np.errstate(all="ignore"):
            u = xs / np.float64(W - 1)
            v = np.float64(j) / np.float64(H - 1)
            su = ((u - 0.5) * cam.scale) * 1.0
            sv = (v - 0.5) * cam.scale
            d = (fwd[None, :] + right[None, :] * su[:, None]) + up[None, :] * sv
        out[k, :, 0:3] = np.array(list(cam.position), np.float64)
        out[k, :, 3:6] = normalize(d)
        out[k, :, 6] = np.inf
    return out.reshape(count * W, 8)


def gen_rays(seed, n, centers, radii, cam_pos):
    """The tests' ray batch: a third of the rays start uniformly in the
    spheres' bounding box with normally distributed directions, a third on a
    random sphere (centre + n*(r + 1e-3)) with a direction in the outward
    hemisphere, the rest at the camera, aimed at a random sphere's centre plus
    N(0, 1.5 r) jitter.  Returns (origins [n,3], directions [n,3])."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centers, np.float64)
    r = np.abs(np.asarray(radii, np.float64))
    lo, hi = (c - r[:, None]).min(axis=0), (c + r[:, None]).max(axis=0)
    kind = np.arange(n) % 3
    rng.shuffle(kind)
    o = np.empty((n, 3))
    d = np.empty((n, 3))
    # in the box
    m = kind == 0
    o[m] = lo + (hi - lo) * rng.random((int(m.sum()), 3))
    d[m] = rng.normal(size=(int(m.sum()), 3))
    # leaving a sphere
    m = kind == 1
    k = int(m.sum())
    s = rng.integers(0, len(r), k)
    nrm = rng.normal(size=(k, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    o[m] = c[s] + nrm * (r[s] + 1e-3)[:, None]
    dd = rng.normal(size=(k, 3))
    flip = (dd * nrm).sum(axis=1) < 0
    dd[flip] = -dd[flip]
    d[m] = dd
    # from the camera
    m = kind == 2
    k = int(m.sum())
    s = rng.integers(0, len(r), k)
    target = c[s] + rng.normal(size=(k, 3)) * (1.5 * r[s])[:, None]
    o[m] = np.asarray(cam_pos, np.float64)
    d[m] = target - o[m]
    return o, d


TMAX_CLASSES = ("inf", "t", "next", "half", "zero", "minus", "nan")


def gen_tmax(seed, t_ref):
    """A tmax per ray from the classes +inf, the reference's closest t (strict
    <: that sphere does not occlude), nextafter(t, +inf), 0.5 t, 0, -1 and
    NaN.  Returns (tmax [n], class index [n])."""
    rng = np.random.default_rng(seed)
    t_ref = np.asarray(t_ref, np.float64)
    n = t_ref.shape[0]
    cls = np.arange(n) % len(TMAX_CLASSES)
    rng.shuffle(cls)
    table = np.stack([np.full(n, np.inf), t_ref, np.nextafter(t_ref, np.inf), 0.5 * t_ref, np.zeros(n),
                      np.full(n, -1.0), np.full(n, np.nan)])
    return table[cls, np.arange(n)], cls
